"""PipelineConfig.recall_overflow in the batched pipeline with online ingest.

A 65536-row index, ingest on, and STEPS batches of 4096 template-built synth
messages from two agents. The template messages land within a small cosine
of each other, so from the second step on (~3700 rows ingested, ~1850 per
agent) every query has more hits above its Gaussian-tail threshold than the
1024-slot candidate buffer holds. The "direct" pipeline (same seed, same
batches) must report that overflow, and sends those queries to the direct
kernel; the "rescan" pipeline must rescan them and send none to the direct
kernel, with and without agent isolation.
"""

import pytest
import torch

from vainplex_openclaw_amd.pipeline.engine import FirewallPipeline, PipelineConfig
from vainplex_openclaw_amd.pipeline.synth import synthetic_batch

pytestmark = pytest.mark.gpu

BATCH, STEPS, N0, AGENTS = 4096, 4, 65536, 2
BASE = dict(batch=BATCH, dim=1024, index_size=N0, topk=16, n_agents=AGENTS,
            ingest=True, ingest_capacity=STEPS * BATCH)


@pytest.fixture(scope="module")
def batches():
    return [synthetic_batch(BATCH, seed=i, n_agents=AGENTS) for i in range(STEPS)]


def _run(batches, **kw):
    pipe = FirewallPipeline(PipelineConfig(**BASE, **kw), device="cuda:0")
    outs = []
    for b in batches:
        n_live = pipe.n_rows
        out = pipe.step(b)
        outs.append((out["recall_scores"], out["recall_ids"], n_live,
                     torch.from_numpy(b.agent_idx).cuda()))
    torch.cuda.synchronize()
    return pipe, outs


@pytest.fixture(scope="module")
def direct(batches):
    return _run(batches)[0]


def test_direct_pipeline_overflows(direct):
    assert direct.cfg.recall_overflow == "direct"
    assert direct.recall_overflowed > 0
    assert direct.recall_rescanned == 0
    # every overflowed query went to the direct kernel
    assert direct.recall_direct_fallbacks >= direct.recall_overflowed


@pytest.mark.parametrize("isolation", [False, True], ids=["shared", "isolated"])
def test_rescan_pipeline(batches, direct, isolation):
    pipe, outs = _run(batches, recall_overflow="rescan", recall_isolation=isolation)
    assert pipe.recall_overflowed > 0
    if not isolation:
        # the same index and thresholds, step for step
        assert pipe.recall_overflowed == direct.recall_overflowed
    assert pipe.recall_rescanned > 0
    assert pipe.recall_direct_fallbacks == 0
    for scores, ids, n_rows, agent in outs:
        assert ids.shape == (BATCH, 16)
        assert (((ids >= 0) & (ids < n_rows)) | (ids == -1)).all()
        assert (scores[:, 1:] <= scores[:, :-1]).all()
        if isolation:
            own = pipe.index_owner[ids.long().clamp_min(0)]
            assert ((own == agent.unsqueeze(1).to(own.dtype)) | (ids < 0)).all()


def test_recall_overflow_is_validated():
    with pytest.raises(ValueError):
        FirewallPipeline(PipelineConfig(**BASE, recall_overflow="never"), device="cuda:0")
    with pytest.raises(ValueError):
        FirewallPipeline(PipelineConfig(**{**BASE, "ingest": False}, recall_mode="direct",
                                        recall_overflow="rescan"), device="cuda:0")
    assert PipelineConfig().recall_overflow == "direct"
