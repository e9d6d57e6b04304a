"""Forgetting in the batched pipeline: ingest_full="evict" keeps a full
shard learning, forget() by count and by salience floor, under plain,
agent-isolated and banded recall; the defaults change nothing; and the
Membrane index drops rows on the GPU."""

import dataclasses
import math

import pytest
import torch

from test_index_forget import check_remove
from vainplex_openclaw_amd.ops import gpu as g
from vainplex_openclaw_amd.pipeline.engine import V_DENY, FirewallPipeline, PipelineConfig
from vainplex_openclaw_amd.pipeline.synth import synthetic_conversations

pytestmark = pytest.mark.gpu

# dim 512: a scale row is a multiple of 16 B, see docs/NOTES-NEXT.md
BASE = dict(batch=256, dim=512, vocab=4096, index_size=2048, topk=8)
N0, SPARE = 2048, 600
CAP = N0 + SPARE


def _cfg(**kw):
    return PipelineConfig(**BASE, ingest=True, ingest_capacity=SPARE, **kw)


@pytest.fixture(scope="module")
def batch():
    return synthetic_conversations(BASE["batch"], seed=0)


def _kept(out):
    return int((out["verdict"] != V_DENY).sum())


def _assert_fp4_copy_live(pipe):
    o4, o_s = g.to_fp4_mx(pipe.index[:pipe.n_rows])
    assert torch.equal(pipe.index4[0][:pipe.n_rows], o4)
    assert torch.equal(pipe.index4[1][:pipe.n_rows], o_s)


def _step_snap(pipe, batch):
    """A step, with the index and the owners as its recall saw them: the
    step's own ingest may forget, and recall_ids name rows as of the
    recall."""
    index = pipe.index.clone()
    owner = None if pipe.index_owner is None else pipe.index_owner.clone()
    n = pipe.n_rows
    out = pipe.step(batch)
    torch.cuda.synchronize()
    assert int(out["recall_ids"].max()) < n
    return out, index, owner


def _assert_top1_is_the_message(index, out):
    keep = out["verdict"] != V_DENY
    top1 = out["recall_ids"][keep][:, 0].long()
    assert (top1 >= 0).all()
    f = out["features"][keep].float()
    r = index[top1].float()
    cos = (f * r).sum(dim=1) / (f.norm(dim=1) * r.norm(dim=1))
    assert float(cos.min()) >= 0.99


def _keys(index, salience):
    """One int16 row per index row: its vector's bits and its salience's."""
    n = index.shape[0]
    return torch.cat([index.view(torch.int16),
                      salience.contiguous().view(torch.int16).view(n, 2)], dim=1)


def _assert_survivors(pipe, index0, sal0, dead):
    """The live rows are, as a multiset of (vector, salience) pairs and bit
    for bit, the rows of the snapshot that `dead` does not mark. The batch
    may hold duplicate messages, so rows are compared by content."""
    n, n_new = index0.shape[0], pipe.n_rows
    assert n_new == n - int(dead.sum())
    keys = torch.cat([_keys(index0, sal0),
                      _keys(pipe.index[:n_new], pipe.salience[:n_new])])
    cls = torch.unique(keys, dim=0, return_inverse=True)[1]
    want = torch.sort(cls[:n][~dead]).values
    got = torch.sort(cls[n:]).values
    assert torch.equal(got, want)


def _run_evict(batch, **kw):
    """Four steps of the same batch; the third overruns the spare rows."""
    pipe = FirewallPipeline(_cfg(ingest_full="evict", **kw), device="cuda:0")
    for _ in range(2):
        pipe.step(batch)
        assert pipe.forget_epoch == 0 and pipe.forgotten == 0
    before = pipe.n_rows
    out3 = pipe.step(batch)
    kept3 = _kept(out3)
    free = CAP - before
    assert kept3 > free, "the third step must overrun the spare rows"
    want = min(max(kept3 - free, math.ceil(pipe.cfg.evict_frac * CAP)), before)
    assert pipe.forgotten == want
    assert pipe.n_rows == before - want + kept3 <= CAP
    assert pipe.forget_epoch == 1 and pipe.ingest_dropped == 0
    return pipe, out3


def test_evict_keeps_learning(batch):
    pipe, out3 = _run_evict(batch)
    n3 = pipe.n_rows
    # the rows appended after the eviction are the kept feature rows
    keep3 = out3["verdict"] != V_DENY
    assert torch.equal(pipe.index[n3 - _kept(out3):n3].view(torch.int16),
                       out3["features"][keep3].view(torch.int16))
    out4, index, _owner = _step_snap(pipe, batch)
    assert pipe.ingest_dropped == 0 and pipe.n_rows <= CAP
    _assert_top1_is_the_message(index, out4)
    _assert_fp4_copy_live(pipe)


def test_forget_count_between_steps(batch):
    pipe = FirewallPipeline(_cfg(), device="cuda:0")
    pipe.step(batch)
    n = pipe.n_rows
    sal = pipe.salience[:n].clone()
    tag = pipe.index[:n].clone()
    m = 300
    dead = g.evict_mask(sal, m)
    assert pipe.forget(count=m) == m
    assert pipe.n_rows == n - m and pipe.forgotten == m and pipe.forget_epoch == 1
    # the survivors are the rows evict_mask keeps, each with its salience
    # and its vector, bit for bit; only their order may differ
    _assert_survivors(pipe, tag, sal, dead)
    _assert_fp4_copy_live(pipe)
    out, index, _owner = _step_snap(pipe, batch)
    _assert_top1_is_the_message(index, out)
    with pytest.raises(ValueError):
        pipe.forget()
    with pytest.raises(ValueError):
        pipe.forget(count=1, min_salience=0.5)
    assert pipe.forget(count=0) == 0 and pipe.forget_epoch == 1


def test_forget_min_salience(batch):
    pipe = FirewallPipeline(_cfg(), device="cuda:0")
    pipe.step(batch)
    n = pipe.n_rows
    rows = torch.tensor([0, 5, 900, N0 - 1, N0, n - 1], device="cuda:0")
    pipe.salience[rows] = torch.tensor([0.01, 0.015, 0.02, 0.0199, 0.01, 0.02],
                                       device="cuda:0")
    sal = pipe.salience[:n].clone()
    assert int((sal <= 0.02).sum()) == rows.numel()
    tag = pipe.index[:n].clone()
    dead = torch.zeros(n, dtype=torch.bool, device="cuda:0")
    dead[rows] = True
    assert pipe.forget(min_salience=0.02) == rows.numel()
    assert float(pipe.salience[:pipe.n_rows].min()) > 0.02
    _assert_survivors(pipe, tag, sal, dead)
    assert pipe.forget(min_salience=0.02) == 0 and pipe.forget_epoch == 1


def test_evict_with_isolation(batch):
    pipe, _out3 = _run_evict(batch, recall_isolation=True)
    want = torch.bincount(pipe.index_owner[:pipe.n_rows].long(), minlength=pipe.cfg.n_agents)
    assert torch.equal(pipe.owner_counts, want)
    out4, index, owner = _step_snap(pipe, batch)
    _assert_top1_is_the_message(index, out4)
    agent = torch.from_numpy(batch.agent_idx).cuda()
    ids = out4["recall_ids"].long()
    own = owner[ids.clamp_min(0)]
    assert ((own == agent.unsqueeze(1)) | (ids < 0)).all()
    want = torch.bincount(pipe.index_owner[:pipe.n_rows].long(), minlength=pipe.cfg.n_agents)
    assert torch.equal(pipe.owner_counts, want)


def test_forget_banded(batch):
    pipe = FirewallPipeline(_cfg(recall_mode="threshold_banded", hot_frac=0.05),
                            device="cuda:0")
    pipe.step(batch)
    # the appended rows are at salience 1.0, every other row below: the
    # hot band is in the tail, and all of it moves when 400 rows go
    pipe._refresh_hot_band()
    assert int(pipe.hot_idx.min()) >= N0
    assert pipe.forget(count=400) == 400
    assert pipe.n_rows < N0
    assert int(pipe.hot_idx.max()) < pipe.n_rows
    assert int(pipe.is_hot[:pipe.n_rows].sum()) == pipe.hot_idx.numel()
    assert not pipe.is_hot[pipe.n_rows:].any()
    assert torch.equal(pipe.hot_X.view(torch.int16),
                       pipe.index[pipe.hot_idx].view(torch.int16))
    out, index, _owner = _step_snap(pipe, batch)
    _assert_top1_is_the_message(index, out)
    _run_evict(batch, recall_mode="threshold_banded")


def test_defaults_and_drop_unchanged(batch):
    f = {x.name: x.default for x in dataclasses.fields(PipelineConfig)}
    assert f["ingest_full"] == "drop" and f["evict_frac"] == 0.01
    with pytest.raises(ValueError):
        FirewallPipeline(_cfg(ingest_full="ring"), device="cuda:0")
    outs = []
    for cfg in (_cfg(), _cfg(ingest_full="drop")):
        pipe = FirewallPipeline(cfg, device="cuda:0")
        steps = [pipe.step(batch) for _ in range(4)]
        torch.cuda.synchronize()
        assert pipe.n_rows == CAP and pipe.ingest_dropped > 0
        assert pipe.forgotten == 0 and pipe.forget_epoch == 0
        outs.append(steps)
    for a, b in zip(*outs):
        assert set(a) == set(b)
        for k in ("verdict", "risk", "logits", "features", "recall_ids",
                  "recall_scores", "trust_scores", "validation"):
            assert torch.equal(a[k], b[k]), k


def test_salience_index_remove_gpu():
    check_remove("cuda:0")
