"""Online memory ingest in the batched pipeline: a step appends its
non-denied messages to the live recall index and the next step recalls
them, under plain, agent-isolated and banded recall; a full index drops
and counts; with ingest off nothing changes."""

import dataclasses

import pytest
import torch

from vainplex_openclaw_amd.pipeline.engine import V_DENY, FirewallPipeline, PipelineConfig
from vainplex_openclaw_amd.pipeline.synth import synthetic_conversations

pytestmark = pytest.mark.gpu

BASE = dict(batch=256, dim=256, vocab=4096, index_size=2048, topk=8)
N0, SPARE = 2048, 600


def _cfg(**kw):
    return PipelineConfig(**BASE, ingest=True, ingest_capacity=SPARE, **kw)


@pytest.fixture(scope="module")
def batch():
    return synthetic_conversations(BASE["batch"], seed=0)


def _two_steps(cfg, batch):
    """Step the same batch twice; returns the pipeline, step 1's keep mask
    and step 2's output."""
    pipe = FirewallPipeline(cfg, device="cuda:0")
    out1 = pipe.step(batch)
    keep = out1["verdict"] != V_DENY
    kept = int(keep.sum())
    assert 200 < kept < BASE["batch"], "the batch must hold kept and denied messages"
    assert pipe.n_rows == N0 + kept
    assert pipe.ingest_dropped == 0
    # the appended rows are the kept feature rows, in batch order
    feats = out1["features"]
    assert torch.equal(pipe.index[N0:pipe.n_rows].view(torch.int16),
                       feats[keep].view(torch.int16))
    assert (pipe.salience[N0:pipe.n_rows] == 1.0).all()
    out2 = pipe.step(batch)
    torch.cuda.synchronize()
    return pipe, keep, kept, out2


def _assert_recalls_ingested(pipe, keep, kept, out2):
    top1 = out2["recall_ids"][keep][:, 0].long()
    assert (top1 >= N0).all() and (top1 < N0 + kept).all()
    # the batch may hold duplicate messages: compare vectors, not positions
    f = out2["features"][keep].float()
    r = pipe.index[top1].float()
    cos = (f * r).sum(dim=1) / (f.norm(dim=1) * r.norm(dim=1))
    assert float(cos.min()) >= 0.99
    return top1


def test_second_step_recalls_ingested_rows(batch):
    pipe, keep, kept, out2 = _two_steps(_cfg(), batch)
    _assert_recalls_ingested(pipe, keep, kept, out2)
    assert pipe.n_rows == N0 + kept + int((out2["verdict"] != V_DENY).sum())
    # the fp4 copy of the appended rows is what a bulk build gives
    from vainplex_openclaw_amd.ops import gpu as g
    o4, o_s = g.to_fp4_mx(pipe.index[N0:pipe.n_rows])
    assert torch.equal(pipe.index4[0][N0:pipe.n_rows], o4)
    assert torch.equal(pipe.index4[1][N0:pipe.n_rows], o_s)


def test_ingest_with_isolation(batch):
    pipe, keep, kept, out2 = _two_steps(_cfg(recall_isolation=True), batch)
    top1 = _assert_recalls_ingested(pipe, keep, kept, out2)
    agent = torch.from_numpy(batch.agent_idx).cuda()
    assert torch.equal(pipe.index_owner[top1], agent[keep].to(torch.int32))
    # no recalled row belongs to another agent
    ids = out2["recall_ids"].long()
    own = pipe.index_owner[ids.clamp_min(0)]
    assert ((own == agent.unsqueeze(1)) | (ids < 0)).all()
    want = torch.bincount(pipe.index_owner[:pipe.n_rows].long(), minlength=pipe.cfg.n_agents)
    assert torch.equal(pipe.owner_counts, want)


def test_ingest_banded(batch):
    pipe, keep, kept, out2 = _two_steps(_cfg(recall_mode="threshold_banded"), batch)
    _assert_recalls_ingested(pipe, keep, kept, out2)


def test_full_index_drops_and_counts(batch):
    pipe, _keep, _kept, _out2 = _two_steps(_cfg(), batch)
    before = pipe.n_rows
    out3 = pipe.step(batch)
    kept3 = int((out3["verdict"] != V_DENY).sum())
    assert before + kept3 > N0 + SPARE, "the third step must overrun the spare rows"
    assert pipe.n_rows == N0 + SPARE == pipe.index.shape[0]
    assert pipe.ingest_dropped == before + kept3 - (N0 + SPARE) > 0
    out4 = pipe.step(batch)  # a full index keeps serving
    assert pipe.n_rows == N0 + SPARE
    assert out4["recall_ids"].shape == (BASE["batch"], BASE["topk"])
    assert int(out4["recall_ids"].max()) < N0 + SPARE


def test_ingest_off_changes_nothing(batch):
    """ingest=False (with a capacity that must then be ignored) against a
    config that never names the new fields."""
    outs = []
    for cfg in (PipelineConfig(**BASE),
                PipelineConfig(**BASE, ingest=False, ingest_capacity=SPARE)):
        pipe = FirewallPipeline(cfg, device="cuda:0")
        assert pipe.index.shape[0] == N0 and pipe.salience.shape[0] == N0
        assert pipe.index4[0].shape[0] == N0
        steps = [pipe.step(batch), pipe.step(batch)]
        torch.cuda.synchronize()
        assert pipe.n_rows == N0
        outs.append(steps)
    keys = set(outs[0][0])
    for a, b in zip(*outs):
        assert set(a) == set(b) == keys
        for k in ("verdict", "risk", "logits", "features", "recall_ids",
                  "recall_scores", "trust_scores", "validation"):
            assert torch.equal(a[k], b[k]), k


def test_step_result_keys_unchanged(batch):
    off = FirewallPipeline(PipelineConfig(**BASE), device="cuda:0").step(batch)
    on = FirewallPipeline(_cfg(), device="cuda:0").step(batch)
    assert set(on) == set(off)


def test_ingest_rejects_fp8_index_modes():
    with pytest.raises(ValueError):
        FirewallPipeline(_cfg(recall_mode="two_stage"), device="cuda:0")
    with pytest.raises(ValueError):
        FirewallPipeline(_cfg(recall_fp4=False, recall_fp8=True), device="cuda:0")


def test_config_fields():
    f = {x.name: x.default for x in dataclasses.fields(PipelineConfig)}
    assert f["ingest"] is False and f["ingest_capacity"] == 0
