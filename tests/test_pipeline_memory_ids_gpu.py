"""Stable memory ids in the batched pipeline: every row carries an int64 id
that follows it through append, eviction and forgetting; a step names the
memories it recalled and the memory each message became; rows are found and
forgotten by id. All comparisons are exact."""

import numpy as np
import pytest
import torch

from vainplex_openclaw_amd.pipeline.engine import (
    V_DENY,
    FirewallPipeline,
    PipelineConfig,
    make_memory_id,
    split_memory_id,
)
from vainplex_openclaw_amd.pipeline.synth import TOOL_RISKS, SynthBatch, synthetic_conversations

pytestmark = pytest.mark.gpu

BASE = dict(batch=256, dim=256, vocab=4096, index_size=2048, topk=8)
N0, SPARE = 2048, 600
PRE = 1 << 62


def _cfg(**kw):
    kw.setdefault("memory_ids", True)
    return PipelineConfig(**BASE, ingest=True, ingest_capacity=SPARE, **kw)


def make_batch(seed):
    """240 distinct random-letter messages (content without clusters, so no
    two rows tie) and 16 synthetic conversation messages, injections and
    credentials among them, so that some message is denied."""
    rng = np.random.default_rng(seed)
    msgs = [rng.integers(97, 123, size=300, dtype=np.uint8).tobytes() for _ in range(240)]
    agents = rng.integers(0, 64, size=240).astype(np.int32)
    risks = rng.choice(TOOL_RISKS, size=240).astype(np.float32)
    conv = synthetic_conversations(256, seed=seed)
    pick = list(np.nonzero(conv.labels == 1)[0][:6]) + list(np.nonzero(conv.labels == 2)[0][:4])
    pick += list(np.nonzero(conv.labels == 0)[0][:16 - len(pick)])
    assert len(pick) == 16
    msgs += [conv.messages[i] for i in pick]
    assert len(set(msgs)) == len(msgs), "identical messages would tie in recall"
    return SynthBatch(msgs, np.concatenate([agents, conv.agent_idx[pick]]),
                      np.concatenate([risks, conv.tool_risk[pick]]),
                      np.concatenate([np.zeros(240, dtype=np.int8), conv.labels[pick]]))


@pytest.fixture(scope="module")
def batches():
    return [make_batch(s) for s in (101, 102, 103, 104)]


def _check_kept(out):
    keep = out["verdict"] != V_DENY
    kept = int(keep.sum())
    assert 200 < kept < BASE["batch"], "the batch must hold kept and denied messages"
    return keep


def _bits(t):
    return t.view(torch.int16)


def _assert_ids_resolve(pipe, handed, agents=None):
    """Every id handed out so far is gone or names a row that holds the
    message's feature row bitwise (and its agent as owner); returns how
    many are still there."""
    ids = torch.cat([h[0] for h in handed])
    feats = torch.cat([h[1] for h in handed])
    rows = pipe.memory_rows(ids)
    assert rows.dtype == torch.int32 and rows.shape == ids.shape
    assert int(rows.max()) < pipe.n_rows
    live = rows >= 0
    r = rows[live].long()
    assert torch.equal(pipe.index_ids[r], ids[live])
    assert torch.equal(_bits(pipe.index[r]), _bits(feats[live]))
    if agents is not None:
        own = torch.cat(agents)
        assert torch.equal(pipe.index_owner[r], own[live])
    return int(live.sum())


def test_layout_after_one_step(batches):
    pipe = FirewallPipeline(_cfg(), device="cuda:0")
    assert pipe.index_ids.dtype == torch.int64 and pipe.index_ids.shape == (N0 + SPARE,)
    want = PRE + torch.arange(N0, dtype=torch.int64, device="cuda:0")
    assert torch.equal(pipe.index_ids[:N0], want)
    assert split_memory_id(int(pipe.index_ids[7])) == (True, 0, 7)
    assert (pipe.index_ids[N0:] == -1).all()
    assert pipe.messages_seen == 0

    out = pipe.step(batches[0])
    keep = _check_kept(out)
    mem = out["memory_ids"]
    assert mem.dtype == torch.int64 and mem.shape == (BASE["batch"],)
    assert torch.equal(mem < 0, ~keep) and (mem[~keep] == -1).all()
    pos = torch.arange(BASE["batch"], device="cuda:0")
    assert torch.equal(mem[keep], pos[keep])  # rank 0, first step: seq = batch position
    assert pipe.messages_seen == BASE["batch"]
    rows = pipe.memory_rows(mem[keep])
    assert (rows >= N0).all()
    assert torch.equal(_bits(pipe.index[rows.long()]), _bits(out["features"][keep]))
    # ids in any order, as a list, unknown and negative ones among them
    some = [int(mem[keep][3]), -1, 12345678, int(mem[keep][0]), PRE + 5, PRE + N0]
    assert pipe.memory_rows(some).tolist() == [int(rows[3]), -1, -1, int(rows[0]), 5, -1]

    out2 = pipe.step(batches[1])
    keep2 = _check_kept(out2)
    assert torch.equal(out2["memory_ids"][keep2], pos[keep2] + BASE["batch"])
    assert int(out2["memory_ids"][keep2][0]) == make_memory_id(0, BASE["batch"] + int(pos[keep2][0]))


@pytest.mark.parametrize("isolation", [False, True])
def test_ids_follow_rows_through_eviction(batches, isolation):
    pipe = FirewallPipeline(_cfg(ingest_full="evict", recall_isolation=isolation),
                            device="cuda:0")
    handed, agents = [], []
    for step, b in enumerate(batches[:3]):
        out = pipe.step(b)
        keep = _check_kept(out)
        assert (out["memory_ids"][keep] >= 0).all()
        handed.append((out["memory_ids"][keep], out["features"][keep]))
        agents.append(torch.from_numpy(b.agent_idx).cuda()[keep].to(torch.int32))
        still = _assert_ids_resolve(pipe, handed, agents if isolation else None)
        if step < 2:
            assert pipe.forgotten == 0 and still == sum(h[0].numel() for h in handed)
    assert pipe.forgotten > 0, "the third step must overrun the spare rows"
    assert pipe.ingest_dropped == 0
    live = pipe.index_ids[:pipe.n_rows]
    assert (live >= 0).all()
    assert torch.unique(live).numel() == pipe.n_rows
    # the last step's rows were appended after the eviction: all there
    assert (pipe.memory_rows(handed[2][0]) >= 0).all()


def test_recall_names_memories(batches):
    pipe = FirewallPipeline(_cfg(), device="cuda:0")
    out1 = pipe.step(batches[0])
    keep = _check_kept(out1)
    ids_before = pipe.index_ids.clone()
    out2 = pipe.step(batches[0])
    rm = out2["recall_mem_ids"]
    assert rm.dtype == torch.int64 and rm.shape == (BASE["batch"], BASE["topk"])
    assert torch.equal(rm[keep][:, 0], out1["memory_ids"][keep])
    rid = out2["recall_ids"].long()
    want = torch.where(rid >= 0, ids_before[rid.clamp_min(0)], torch.full_like(rid, -1))
    assert torch.equal(rm, want)
    # the first step recalled preloaded rows only
    r1 = out1["recall_mem_ids"]
    assert ((r1 == -1) | (r1 >= PRE)).all() and (r1 >= PRE).any()
    assert torch.equal(r1[r1 >= 0] - PRE, out1["recall_ids"][r1 >= 0].long())


def test_forget_by_id(batches):
    pipe = FirewallPipeline(_cfg(), device="cuda:0")
    out = pipe.step(batches[0])
    keep = _check_kept(out)
    mem, feats = out["memory_ids"][keep], out["features"][keep]
    gen = torch.Generator(device="cuda:0").manual_seed(0)
    order = torch.randperm(mem.numel(), generator=gen, device="cuda:0")
    chosen = torch.cat([mem[order[:30]], PRE + torch.arange(100, 120, device="cuda:0")])
    rest = torch.cat([mem[order[30:]], PRE + torch.arange(0, 100, device="cuda:0"),
                      PRE + torch.arange(120, N0, device="cuda:0")])
    rest_rows = pipe.memory_rows(rest).long()
    rest_bits = _bits(pipe.index[rest_rows]).clone()
    n, epoch = pipe.n_rows, pipe.forget_epoch
    arg = torch.cat([chosen, chosen[:7], torch.tensor([99999999, PRE + N0 + 3, -1],
                                                       device="cuda:0")])
    assert pipe.forget(ids=arg) == 50
    assert pipe.n_rows == n - 50 and pipe.forget_epoch == epoch + 1 and pipe.forgotten == 50
    assert (pipe.memory_rows(chosen) == -1).all()
    now = pipe.memory_rows(rest).long()
    assert (now >= 0).all() and int(now.max()) < pipe.n_rows
    assert torch.equal(_bits(pipe.index[now]), rest_bits)
    assert torch.equal(pipe.index_ids[now], rest)
    # a sequence works, and ids that are gone are ignored
    assert pipe.forget(ids=chosen.tolist()) == 0 and pipe.forget_epoch == epoch + 1
    assert pipe.forget(ids=[int(rest[0])]) == 1
    out2 = pipe.step(batches[0])
    gone = torch.cat([chosen, rest[:1]])
    for key in ("recall_mem_ids", "memory_ids"):
        assert not torch.isin(out2[key], gone).any(), key
    with pytest.raises(ValueError):
        pipe.forget(count=1, ids=[1])
    with pytest.raises(ValueError):
        pipe.forget(min_salience=0.5, ids=[1])
    with pytest.raises(ValueError):
        pipe.forget(count=1, min_salience=0.5)
    with pytest.raises(ValueError):
        pipe.forget()


def test_dedup_reports_the_reinforced_row(batches):
    pipe = FirewallPipeline(_cfg(ingest_dedup=0.98), device="cuda:0")
    out1 = pipe.step(batches[0])
    keep = _check_kept(out1)
    assert pipe.ingest_merged_index == 0
    stored1 = out1["memory_ids"] >= 0
    n, in_batch1 = pipe.n_rows, pipe.ingest_merged_batch
    out2 = pipe.step(batches[0])
    keep2 = _check_kept(out2)
    merged = pipe.ingest_merged_index
    assert merged > 200
    assert pipe.n_rows == n + int(keep2.sum()) - merged - (pipe.ingest_merged_batch - in_batch1)
    # a repeated message reinforced the row it became in the first step
    both = stored1 & (out2["memory_ids"] >= 0) & (out2["memory_ids"] < BASE["batch"])
    assert int(both.sum()) > 200
    assert torch.equal(out2["memory_ids"][both], out1["memory_ids"][both])
    rows = pipe.memory_rows(out2["memory_ids"][both]).long()
    assert (pipe.salience[rows] == 1.0).all()
    assert (out2["memory_ids"][~keep2] == -1).all()


def test_off_switch(batches):
    off = FirewallPipeline(PipelineConfig(**BASE), device="cuda:0")
    ing = FirewallPipeline(_cfg(memory_ids=False), device="cuda:0")
    on = FirewallPipeline(_cfg(), device="cuda:0")
    assert off.index_ids is None and ing.index_ids is None
    o_off, o_ing, o_on = (p.step(batches[0]) for p in (off, ing, on))
    assert set(o_ing) == set(o_off)
    assert set(o_on) == set(o_off) | {"recall_mem_ids", "memory_ids"}
    for k in ("verdict", "risk", "recall_ids", "recall_scores"):
        assert torch.equal(o_on[k], o_ing[k]), k
    for p in (off, ing):
        with pytest.raises(ValueError):
            p.memory_rows([1])
        with pytest.raises(ValueError):
            p.forget(ids=[1])
