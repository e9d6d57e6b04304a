"""Agent-isolated recall on the GPU: the owner filter of the direct kernel,
the fp4x4 and bf16 threshold paths, banded mode, the pipeline flag and
SalienceIndex, each against the fp32 masked dense reference
(ops.gpu.reference_owned_topk).
"""

import numpy as np
import pytest
import torch

from vainplex_openclaw_amd.ops import gpu as g

pytestmark = pytest.mark.gpu


def _unit(n, d, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(n, d, generator=gen, device="cuda")
    return torch.nn.functional.normalize(x, dim=1).bfloat16()


def _owners_with_sizes(sizes, nq, seed):
    """Row owners with the given per-owner row counts (shuffled), and query
    owners cycling over all owners."""
    gen = torch.Generator().manual_seed(seed)
    xo = torch.cat([torch.full((n,), o, dtype=torch.int32) for o, n in enumerate(sizes)])
    xo = xo[torch.randperm(xo.numel(), generator=gen)]
    qo = (torch.arange(nq) % len(sizes)).to(torch.int32)
    return xo.cuda(), qo.cuda()


def _check_against_reference(scores, ids, ref_s, ref_i, xo, qo, k, counts):
    ids_np, ref_np = ids.cpu().numpy(), ref_i.cpu().numpy()
    vals, ref_vals = scores.cpu().numpy(), ref_s.cpu().numpy()
    xo_np, qo_np = xo.cpu().numpy(), qo.cpu().numpy()
    for q in range(ids_np.shape[0]):
        have = min(k, int(counts[qo_np[q]]))
        real = ids_np[q][ids_np[q] >= 0]
        assert (xo_np[real] == qo_np[q]).all(), f"q={q}: foreign id"
        assert len(set(real)) == len(real), f"q={q}: duplicate id"
        inter = len(set(real) & set(ref_np[q][ref_np[q] >= 0]))
        assert inter >= have - 2, f"q={q}: {inter}/{have}"
        if have:
            assert abs(vals[q][0] - ref_vals[q][0]) < 2e-2
    return ids_np, qo_np


@pytest.mark.parametrize("nq,nx,D,k", [(70, 1613, 128, 8), (300, 4096, 256, 16)])
def test_direct_kernel_owner_filter(nq, nx, D, k):
    Q, X = _unit(nq, D, 1), _unit(nx, D, 2)
    rest = nx - 3
    sizes = [rest // 2, rest // 4, rest // 8, rest - rest // 2 - rest // 4 - rest // 8, 3]
    xo, qo = _owners_with_sizes(sizes, nq, 5)
    scores, ids = g.topk_recall(Q, X, k, owner=xo, qowner=qo)
    ref_s, ref_i = g.reference_owned_topk(Q, X, k, xo, qo)
    ids_np, qo_np = _check_against_reference(scores, ids, ref_s, ref_i, xo, qo, k, sizes)
    small = qo_np == 4
    assert small.sum() > 0
    # exactly min(k, n_owned) = 3 filled slots, the rest at fill values
    assert ((ids_np[small] >= 0).sum(axis=1) == 3).all()
    assert (scores[torch.from_numpy(small).cuda()][:, 3:] == -1e30).all()
    # unfiltered queries through the filtered launch see every row
    wild = torch.full_like(qo, -1)
    ws, wi = g.topk_recall(Q, X, k, owner=xo, qowner=wild)
    ps, pi = g.topk_recall(Q, X, k)
    assert torch.equal(wi.sort(dim=1).values, pi.sort(dim=1).values)
    # owner=None is the call without the keyword arguments
    ns, ni = g.topk_recall(Q, X, k, owner=None, qowner=None)
    assert torch.equal(ns, ps) and torch.equal(ni, pi)
    es, ei = g.ext().topk_recall(Q, X, k, 4)
    es2, ei2 = g.ext().topk_recall(Q, X, k, 4, xowner=None, qowner=None)
    assert torch.equal(es, es2) and torch.equal(ei, ei2)


def test_threshold_fp4x4_owner_filter():
    """fp4x4 owned scan + exact rescore; the 10-row owner forces the
    owner-filtered direct fallback."""
    nq, nx, D, k = 512, 32768, 1024, 16
    torch.manual_seed(11)
    Q = torch.nn.functional.normalize(torch.randn(nq, D, device="cuda"), dim=1).bfloat16()
    X = torch.nn.functional.normalize(torch.randn(nx, D, device="cuda"), dim=1).bfloat16()
    sizes = [16384, 8192, 4096, 2048, 1024, 512, 502, 10]
    assert sum(sizes) == nx
    xo, qo = _owners_with_sizes(sizes, nq, 7)
    X4 = g.to_fp4_mx(X)
    counts = torch.bincount(xo.long(), minlength=len(sizes))
    scores, ids = g.topk_recall_threshold(Q, X, k, X4=X4, q4=True, owner=xo, qowner=qo,
                                          owner_counts=counts)
    ref_s, ref_i = g.reference_owned_topk(Q, X, k, xo, qo)
    ids_np, qo_np = _check_against_reference(scores, ids, ref_s, ref_i, xo, qo, k, sizes)
    assert ((ids_np[qo_np == 7] >= 0).sum(axis=1) == 10).all()
    assert ((ids_np[qo_np != 7] >= 0).sum(axis=1) == k).all()
    # without the cached counts: same result
    s2, i2 = g.topk_recall_threshold(Q, X, k, X4=X4, q4=True, owner=xo, qowner=qo)
    assert torch.equal(i2.sort(dim=1).values, ids.sort(dim=1).values)
    assert torch.allclose(s2, scores, rtol=0, atol=1e-6)
    # scans without an owner filter refuse owners
    with pytest.raises(NotImplementedError):
        g.topk_recall_threshold(Q, X, k, X4=X4, q4=False, owner=xo, qowner=qo)
    with pytest.raises(NotImplementedError):
        g.topk_recall_threshold(Q, X, k, X8=g.to_fp8_bytes(X), owner=xo, qowner=qo)


def test_salience_weighted_owner_filter_and_banded():
    torch.manual_seed(5)
    nq, nx, d, k = 64, 8192, 256, 8
    Q = torch.nn.functional.normalize(torch.randn(nq, d, device="cuda"), dim=1).bfloat16()
    X = torch.nn.functional.normalize(torch.randn(nx, d, device="cuda"), dim=1).bfloat16()
    sal = torch.rand(nx, device="cuda") * 0.9 + 0.1
    xo = torch.randint(0, 5, (nx,), dtype=torch.int32, device="cuda")
    qo = torch.randint(0, 5, (nq,), dtype=torch.int32, device="cuda")
    dense = torch.matmul(Q.float(), X.float().T)

    def check(got_s, got_i):
        assert (got_i >= 0).all()
        assert (xo[got_i.long()] == qo.unsqueeze(1)).all(), "foreign id"
        srt = got_i.sort(dim=1).values
        assert (srt[:, 1:] != srt[:, :-1]).all(), "duplicate id"
        exact_w = torch.gather(dense, 1, got_i.long()) * sal[got_i.long()]
        assert (got_s - exact_w).abs().max().item() < 1e-3

    got_s, got_i = g.topk_recall_threshold(Q, X, k, salience=sal, owner=xo, qowner=qo)
    check(got_s, got_i)
    ref_w, _ = g.reference_owned_topk(Q, X, k, xo, qo, salience=sal)
    regret = 1.0 - got_s.sum(dim=1) / ref_w.sum(dim=1).clamp_min(1e-6)
    assert regret.max().item() < 0.05, regret.max().item()

    hot_idx = torch.topk(sal, 64).indices
    for x4 in (None, g.to_fp4_mx(X)):
        bs, bi = g.topk_recall_threshold_banded(
            Q, X, k, salience=sal, hot_idx=hot_idx, X4=x4, owner=xo, qowner=qo)
        check(bs, bi)


def test_encoder_short_dim_matches_reference():
    """The isolation pipeline case runs at dim=256: one short encoder chunk."""
    from vainplex_openclaw_amd.pipeline.synth import synthetic_batch

    msgs = synthetic_batch(64, seed=3).messages
    gen = np.random.default_rng(0)
    embed = ((gen.random((4096, 256), dtype=np.float32) - 0.5) * 0.1)
    embed_t = torch.from_numpy(embed).cuda().bfloat16()
    b, o = g.pack_messages(msgs)
    got = g.encode_messages(b, o, embed_t, normalize=True).float().cpu().numpy()
    want = g.reference_encode(msgs, embed_t.float().cpu().numpy(), normalize=True)
    assert got.shape == (64, 256)
    # unit-norm rows: components < 0.5, bf16 output rounding < 2^-10
    assert np.abs(got - want).max() < 2e-3


def test_pipeline_recall_isolation():
    from vainplex_openclaw_amd.pipeline.engine import FirewallPipeline, PipelineConfig
    from vainplex_openclaw_amd.pipeline.synth import synthetic_batch

    base = dict(batch=256, index_size=8192, dim=256, n_agents=8)
    iso = FirewallPipeline(PipelineConfig(recall_isolation=True, **base))
    off_a = FirewallPipeline(PipelineConfig(**base))
    off_b = FirewallPipeline(PipelineConfig(recall_isolation=False, **base))
    assert off_a.index_owner is None
    # the flag leaves the index contents alone
    assert torch.equal(iso.index, off_a.index)
    counts = torch.bincount(iso.index_owner.long(), minlength=8)
    assert torch.equal(iso.owner_counts, counts) and int(counts.min()) > 0
    for step in range(2):
        batch = synthetic_batch(256, seed=40 + step, n_agents=8)
        out = iso.step(batch)
        ids = out["recall_ids"]
        agent = torch.from_numpy(batch.agent_idx).to(ids.device)
        real = ids >= 0
        assert int(real.sum()) > 0
        own = iso.index_owner[ids.long().clamp_min(0)]
        assert (~real | (own == agent.unsqueeze(1))).all()
        oa, ob = off_a.step(batch), off_b.step(batch)
        assert torch.equal(oa["recall_ids"], ob["recall_ids"])
        assert torch.equal(oa["recall_scores"], ob["recall_scores"])
    with pytest.raises(ValueError):
        FirewallPipeline(PipelineConfig(recall_isolation=True, recall_mode="two_stage", **base))


def test_pipeline_recall_isolation_direct_mode():
    from vainplex_openclaw_amd.pipeline.engine import FirewallPipeline, PipelineConfig
    from vainplex_openclaw_amd.pipeline.synth import synthetic_batch

    cfg = PipelineConfig(batch=256, index_size=8192, dim=256, n_agents=8,
                         recall_isolation=True, recall_mode="direct")
    pipe = FirewallPipeline(cfg)
    batch = synthetic_batch(256, seed=50, n_agents=8)
    ids = pipe.step(batch)["recall_ids"]
    agent = torch.from_numpy(batch.agent_idx).to(ids.device)
    own = pipe.index_owner[ids.long().clamp_min(0)]
    assert (ids >= 0).all() and (own == agent.unsqueeze(1)).all()


def test_salience_index_small_owner_gpu():
    from vainplex_openclaw_amd.membrane.index import SalienceIndex

    query = "the quarterly revenue report for the northern region is due on friday"
    idx = SalienceIndex(dim=1024, device="cuda:0", capacity=16)
    idx.add("A", [f"a{i}" for i in range(60)],
            [f"{query} and item {i} needs review" for i in range(60)])
    b_texts = [
        "zebra crossing painted yesterday near the old mill",
        "my cat prefers tuna over chicken on weekdays",
        "compile flags -O3 and loop unrolling explained",
    ]
    idx.add("B", ["b0", "b1", "b2"], b_texts)
    got = idx.search("B", query, k=2)
    q = idx.encode([query]).float()
    sims = (idx.encode(b_texts).to(torch.bfloat16).float() @ q.to(torch.bfloat16).float().T)
    sims = sims.reshape(-1).cpu().numpy()
    order = np.argsort(-sims)[:2]
    assert [r for r, _ in got] == [f"b{i}" for i in order]
    assert np.allclose([s for _, s in got], sims[order], atol=2e-2)
    assert len(idx.search("B", query, k=5)) == 3
    assert idx.search("C", query, k=2) == []
    assert all(r.startswith("a") for r, _ in idx.search("A", query, k=8))
