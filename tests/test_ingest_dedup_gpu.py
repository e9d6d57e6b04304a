"""Ingest dedup on the GPU: the two kernels of csrc/ingest_dedup.hip
against their fp64 references, and PipelineConfig.ingest_dedup in the
batched pipeline (repeated texts, agent isolation, a replay of the rule on
synthetic conversations, eviction in the same step, and off = unchanged)."""

import numpy as np
import pytest
import torch

from test_ingest_dedup import (MARGIN, TAU, assert_batch_margin, assert_recall_margin,
                               batch_case, recall_case, stored_rows_are_apart, _unit)
from vainplex_openclaw_amd.ops import gpu as g
from vainplex_openclaw_amd.pipeline.engine import V_DENY, FirewallPipeline, PipelineConfig
from vainplex_openclaw_amd.pipeline.synth import (TOOL_RISKS, SynthBatch,
                                                  synthetic_conversations)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _cuda(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


# -- batch_first_similar_kernel ----------------------------------------------

# the kernel's tile is 128 rows: one short of it, the tile, one row past
# it, and several tiles with a ragged last one
@pytest.mark.parametrize("owners", [False, True])
@pytest.mark.parametrize("D", [128, 1024])
@pytest.mark.parametrize("B", [1, 2, 127, 128, 129, 300])
def test_batch_first_similar_matches_reference(B, D, owners):
    F, elig, owner = batch_case(B, D, 0, owners)
    pairs = assert_batch_margin(F, elig, owner)
    assert B < 100 or pairs >= 90
    want = g.reference_batch_first_similar(F, elig, TAU, owner)
    Fg, eg, og = _cuda(F, elig, owner)
    got = g.batch_first_similar(Fg, eg, TAU, og)
    again = g.batch_first_similar(Fg, eg, TAU, og)
    assert got.dtype == torch.int32 and got.is_cuda
    assert torch.equal(got.cpu(), want)
    assert torch.equal(got, again)


@pytest.mark.parametrize("pair", [(127, 128), (5, 290)])
def test_batch_first_similar_single_pair_across_tiles(pair):
    B, D = 300, 128
    F = _unit(torch.Generator().manual_seed(3), B, D).bfloat16()
    F[pair[1]] = F[pair[0]]
    elig = torch.ones(B, dtype=torch.bool)
    assert assert_batch_margin(F, elig, None) == 1
    want = torch.arange(B, dtype=torch.int32)
    want[pair[1]] = pair[0]
    assert torch.equal(g.reference_batch_first_similar(F, elig, TAU), want)
    got = g.batch_first_similar(*_cuda(F, elig), TAU)
    assert torch.equal(got.cpu(), want)


# -- recall_dup_rows_kernel --------------------------------------------------

@pytest.mark.parametrize("owners", [False, True])
@pytest.mark.parametrize("D", [128, 1024])
@pytest.mark.parametrize("k", [1, 8, 16])
@pytest.mark.parametrize("B", [1, 65, 300])
def test_recall_dup_rows_matches_reference(B, k, D, owners):
    F, ids, X, xo, qo = recall_case(B, k, D, 0, owners)
    hits = assert_recall_margin(F, ids, X, xo, qo)
    assert B < 10 or 0 < hits < B
    want_row, want_dot = g.reference_recall_dup_rows(F, ids, X, TAU, xo, qo)
    Fg, ig, Xg, xog, qog = _cuda(F, ids, X, xo, qo)
    row, dot = g.recall_dup_rows(Fg, ig, Xg, TAU, xog, qog)
    assert row.dtype == torch.int32 and dot.dtype == torch.float32 and row.is_cuda
    assert torch.equal(row.cpu(), want_row)
    found = want_row >= 0
    err = (dot.cpu()[found].double() - want_dot[found]).abs()
    assert (err <= 1e-4).all()


def test_recall_dup_rows_equal_dots_go_to_the_lowest_id():
    # rows that are bitwise equal give equal dots in any arithmetic
    gen = torch.Generator().manual_seed(5)
    X = _unit(gen, 64, 256).bfloat16()
    X[40] = X[7]
    X[23] = X[7]
    F = X[[7, 7, 9]].clone()
    ids = torch.tensor([[40, 3, 23, 7, 23, -1, 64, 1 << 30],
                        [40, 40, 23, 2, 2, -5, 63, 64],
                        [40, 3, 23, 7, 23, -1, 64, 5]], dtype=torch.int32)
    row, dot = g.recall_dup_rows(*_cuda(F, ids, X), TAU)
    assert row.tolist() == [7, 23, -1]
    assert torch.equal(row.cpu(), g.reference_recall_dup_rows(F, ids, X, TAU)[0])
    assert float(dot[0]) == float(dot[1]) >= TAU


# -- the pipeline ------------------------------------------------------------

BASE = dict(batch=256, dim=256, vocab=4096, index_size=2048, topk=8)
N0, SPARE = 2048, 600
TAU_TEXT = 0.98
KEYS = ("verdict", "risk", "logits", "features", "recall_ids", "recall_scores",
        "trust_scores", "validation")


def _cfg(**kw):
    kw.setdefault("ingest_capacity", SPARE)
    return PipelineConfig(**BASE, ingest=True, **kw)


def _repeated_batch():
    """8 distinct random-letter texts, each 32 times, under 4 agents: 8
    copies of every (text, agent) pair. Returns the batch and text ids."""
    rng = np.random.default_rng(11)
    texts = [rng.integers(97, 123, size=300, dtype=np.uint8).tobytes() for _ in range(8)]
    text_of = np.arange(256) % 8
    agent = ((np.arange(256) // 8) % 4).astype(np.int32)
    batch = SynthBatch([texts[t] for t in text_of], agent,
                       rng.choice(TOOL_RISKS, size=256).astype(np.float32),
                       np.zeros(256, dtype=np.int8))
    return batch, torch.from_numpy(text_of).to(DEV)


def _assert_texts_apart(feats, text_of):
    """Identical texts are within TAU_TEXT, distinct texts below it by
    MARGIN: what the counts below rest on."""
    S = feats.double() @ feats.double().T
    same = text_of.unsqueeze(1) == text_of.unsqueeze(0)
    assert float(S[same].min()) >= TAU_TEXT
    assert float(S[~same].max()) <= TAU_TEXT - MARGIN


def _groups(key, keep):
    """The distinct values of `key` among the kept messages."""
    return torch.unique(key[keep])


@pytest.mark.parametrize("isolation", [False, True])
def test_repeated_texts_are_stored_once(isolation):
    batch, text_of = _repeated_batch()
    agent = torch.from_numpy(batch.agent_idx).to(DEV)
    pipe = FirewallPipeline(_cfg(ingest_dedup=TAU_TEXT, recall_isolation=isolation),
                            device=DEV)
    # what may merge: the same text, and under isolation the same agent too
    key = text_of * 64 + agent if isolation else text_of

    out1 = pipe.step(batch)
    _assert_texts_apart(out1["features"], text_of)
    keep1 = out1["verdict"] != V_DENY
    kept1, stored1 = int(keep1.sum()), _groups(key, keep1)
    assert kept1 > 200
    assert stored1.numel() > 0
    assert pipe.n_rows == N0 + stored1.numel()
    assert pipe.ingest_merged_index == 0
    assert pipe.ingest_merged_batch == kept1 - stored1.numel()
    # the stored rows are the first kept copy of each group, in batch order
    pos = torch.arange(256, device=DEV)
    firsts = torch.stack([pos[keep1 & (key == k_)].min() for k_ in stored1]).sort().values
    assert torch.equal(pipe.index[N0:pipe.n_rows].view(torch.int16),
                       out1["features"][firsts].view(torch.int16))
    assert (pipe.salience[N0:pipe.n_rows] == 1.0).all()

    n1 = pipe.n_rows
    out2 = pipe.step(batch)
    torch.cuda.synchronize()
    keep2 = out2["verdict"] != V_DENY
    kept2 = int(keep2.sum())
    assert kept2 > 200
    assert pipe.n_rows == n1, "step 2 stores nothing: every kept message has its row"
    assert pipe.ingest_merged_index == kept2
    assert pipe.ingest_merged_batch == kept1 - stored1.numel()
    assert pipe.ingest_dropped == 0
    # the rows that were met again carry exactly the salience of a fresh copy
    met = torch.isin(key[firsts], _groups(key, keep2))
    assert met.any()
    assert (pipe.salience[N0:n1][met] == 1.0).all()
    assert (pipe.salience[:N0] < 1.0).all()

    if isolation:
        # step 2 appended nothing, so the index is as its recall saw it
        dup_row, _ = g.recall_dup_rows(out2["features"], out2["recall_ids"],
                                       pipe.index[:n1], TAU_TEXT,
                                       xowner=pipe.index_owner[:n1],
                                       qowner=agent.to(torch.int32))
        assert (dup_row[keep2] >= N0).all()
        assert torch.equal(pipe.index_owner[dup_row[keep2].long()], agent[keep2].to(torch.int32))
        want = torch.bincount(pipe.index_owner[:n1].long(), minlength=pipe.cfg.n_agents)
        assert torch.equal(pipe.owner_counts, want)


def _replay(index, owner, out, agent, tau):
    """The rule of FirewallPipeline._dedup from the reference_* functions,
    on the index as the step's recall saw it, on CPU: (merged into the
    index, merged within the batch, bool mask of the messages to store,
    first, dup_row, gap). gap is the smallest distance from tau of a dot
    the rule compares with it (fp64): a kept message against its recalled
    rows, and the eligible pairs; the fp64 replay and the fp32 kernels
    decide alike while it exceeds the fp32 accumulation error."""
    feats = out["features"].cpu()
    keep = (out["verdict"] != V_DENY).cpu()
    ids = out["recall_ids"].cpu()
    ids = torch.where(keep.unsqueeze(1), ids, torch.full_like(ids, -1))
    qo = None if owner is None else agent.cpu().to(torch.int32)
    xo = None if owner is None else owner.cpu()
    X = index.cpu()
    dup_row, _ = g.reference_recall_dup_rows(feats, ids, X, tau, xo, qo)
    in_index = dup_row >= 0
    elig = keep & ~in_index
    first = g.reference_batch_first_similar(feats, elig, tau, qo)
    store = first == torch.arange(first.numel(), dtype=torch.int32)

    idl = ids.long()
    ok = (idl >= 0) & (idl < X.shape[0])
    safe = idl.clamp(0, X.shape[0] - 1)
    if xo is not None:
        ok &= xo[safe] == qo.unsqueeze(1)
    rec = (X.double()[safe] * feats.double().unsqueeze(1)).sum(2)[ok]
    S = feats.double() @ feats.double().T
    pair = torch.tril(elig.unsqueeze(1) & elig.unsqueeze(0), -1)
    if qo is not None:
        pair &= qo.unsqueeze(1) == qo.unsqueeze(0)
    gap = float((torch.cat([rec, S[pair]]) - tau).abs().min())
    print(f"tau={tau}: smallest distance of a compared dot from tau {gap:.3e}, "
          f"merged {int(in_index.sum())} + {int((elig & ~store).sum())}, "
          f"stored {int(store.sum())}")
    return int(in_index.sum()), int((elig & ~store).sum()), store, first, dup_row, gap


# dim 256: fp32 accumulation of products whose magnitudes sum to at most 1
# errs by at most about 256 * 2^-24 = 1.5e-5
REPLAY_MARGIN = 2e-5
TAU_SYNTH = 0.95


def _synthetic_steps():
    """Two batches of synthetic conversations. The second repeats 96
    messages of the first (copies of index rows by then), brings 96 new
    ones and repeats 64 of those, each repeat under its own agent: it
    merges into the index, merges within the batch and stores new rows,
    with and without isolation."""
    a = synthetic_conversations(BASE["batch"], seed=0)
    b = synthetic_conversations(BASE["batch"], seed=1)
    pick = lambda x, y: np.concatenate([x[:96], y[:96], y[:64]])
    mixed = SynthBatch(a.messages[:96] + b.messages[:96] + b.messages[:64],
                       pick(a.agent_idx, b.agent_idx), pick(a.tool_risk, b.tool_risk),
                       pick(a.labels, b.labels))
    return a, mixed


@pytest.mark.parametrize("isolation", [False, True])
def test_synthetic_steps_follow_the_reference_rule(isolation):
    batches = _synthetic_steps()
    pipe = FirewallPipeline(_cfg(ingest_dedup=TAU_SYNTH, recall_isolation=isolation),
                            device=DEV)
    merged_index = merged_batch = 0
    for batch in batches:
        n = pipe.n_rows
        index = pipe.index[:n].clone()
        owner = None if pipe.index_owner is None else pipe.index_owner[:n].clone()
        agent = torch.from_numpy(batch.agent_idx).to(DEV)
        out = pipe.step(batch)
        torch.cuda.synchronize()
        mi, mb, store, first, _, gap = _replay(index, owner, out, agent, TAU_SYNTH)
        assert gap >= REPLAY_MARGIN
        merged_index += mi
        merged_batch += mb
        assert int(store.sum()) > 0
        assert pipe.n_rows == n + int(store.sum())
        assert pipe.ingest_merged_index == merged_index
        assert pipe.ingest_merged_batch == merged_batch
        assert torch.equal(pipe.index[n:pipe.n_rows].view(torch.int16).cpu(),
                           out["features"].cpu()[store].view(torch.int16))
        assert (pipe.salience[n:pipe.n_rows] == 1.0).all()
        qo = agent.cpu().to(torch.int32) if isolation else None
        assert stored_rows_are_apart(out["features"].cpu(), first, qo, TAU_SYNTH)
        if isolation:
            want = torch.bincount(pipe.index_owner[:pipe.n_rows].long(),
                                  minlength=pipe.cfg.n_agents)
            assert torch.equal(pipe.owner_counts, want)
    assert merged_index > 0 and merged_batch > 0


def test_evicting_step_keeps_the_rows_it_matched():
    a, mixed = _synthetic_steps()
    spare = 24
    pipe = FirewallPipeline(_cfg(ingest_dedup=TAU_SYNTH, ingest_full="evict",
                                 ingest_capacity=spare), device=DEV)
    pipe.step(a)
    free = pipe.capacity - pipe.n_rows
    n = pipe.n_rows
    index = pipe.index[:n].clone()
    epoch = pipe.forget_epoch
    out = pipe.step(mixed)  # must not raise
    torch.cuda.synchronize()
    mi, _mb, store, _first, dup_row, gap = _replay(index, None, out, None, TAU_SYNTH)
    assert gap >= REPLAY_MARGIN
    assert int(store.sum()) > free, "step 2 must overrun the spare rows"
    assert pipe.forget_epoch == epoch + 1 and pipe.ingest_dropped == 0
    assert mi > 0
    # every matched row is still live, wherever the compaction put it
    matched = index[torch.unique(dup_row[dup_row >= 0]).long().to(DEV)].view(torch.int16)
    live = pipe.index[:pipe.n_rows].view(torch.int16)
    there = (matched.unsqueeze(1) == live.unsqueeze(0)).all(dim=2).any(dim=1)
    assert there.all()
    # and the new rows are in, after the eviction
    k_new = int(store.sum())
    assert torch.equal(live[pipe.n_rows - k_new:].cpu(),
                       out["features"].cpu()[store].view(torch.int16))


def test_dedup_off_changes_nothing():
    batch = synthetic_conversations(BASE["batch"], seed=0)
    outs, rows = [], []
    for cfg in (_cfg(), _cfg(ingest_dedup=0.0)):
        pipe = FirewallPipeline(cfg, device=DEV)
        steps = [pipe.step(batch), pipe.step(batch)]
        torch.cuda.synchronize()
        assert pipe.ingest_merged_index == 0 and pipe.ingest_merged_batch == 0
        outs.append(steps)
        rows.append(pipe.n_rows)
    assert rows[0] == rows[1] > N0
    for x, y in zip(*outs):
        assert set(x) == set(y)
        for k_ in KEYS:
            assert torch.equal(x[k_], y[k_]), k_
