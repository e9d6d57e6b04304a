"""The bin rule of the dropped-hit histogram (ops.gpu.hist_bin_spec) and the
rescan plan built on it (ops.gpu.overflow_rescan_plan), on CPU tensors.

The hist scan kernels implement hist_bin_spec bit for bit
(test_scan_fp4_hist_gpu.py); here the rule itself is pinned down: a score on
an edge belongs to the bin below it, one ulp above to the bin above, scores
far past the last edge to the open last bin, and a tiny w sends every hit to
the last bin. The plan is checked on hand-built histograms and, as a
property, on random fp32 score rows: a rescan at theta2 keeps exactly
expect_n hits.
"""

import pytest
import torch

from vainplex_openclaw_amd.ops import gpu as g

NB = g.HIST_NB
INF = float("inf")


def _ulp_up(x):
    return torch.nextafter(x, torch.full_like(x, INF))


def _ulp_down(x):
    return torch.nextafter(x, torch.full_like(x, -INF))


THETA_W = [(0.5, 0.002), (0.0, 1.0 / 256), (-0.25, 0.005), (0.123456, 3.3e-4),
           (0.9, 6.5e-4), (100.0, 0.37)]


@pytest.mark.parametrize("theta,w", THETA_W)
def test_edges_are_the_fp64_rule(theta, w):
    th = torch.tensor([theta], dtype=torch.float32)
    ww = torch.tensor([w], dtype=torch.float32)
    e = g.hist_edges(th, ww)
    assert e.shape == (1, NB + 1) and e.dtype == torch.float32
    import numpy as np
    want = [np.float32(np.float64(j) * np.float64(ww[0].item()) + np.float64(th[0].item()))
            for j in range(NB + 1)]
    assert e[0].tolist() == [float(x) for x in want]
    assert (e[0, 1:] > e[0, :-1]).all()


@pytest.mark.parametrize("theta,w", THETA_W)
def test_bin_on_and_next_to_every_edge(theta, w):
    th = torch.tensor([theta], dtype=torch.float32)
    ww = torch.tensor([w], dtype=torch.float32)
    e = g.hist_edges(th, ww)[0]
    j = torch.arange(1, NB)
    on = e[1:NB].unsqueeze(0)
    # edge(j) itself closes bin j - 1; one ulp above opens bin j
    assert torch.equal(g.hist_bin_spec(on, th, ww)[0], j - 1)
    assert torch.equal(g.hist_bin_spec(_ulp_up(on), th, ww)[0], j)
    assert torch.equal(g.hist_bin_spec(_ulp_down(on), th, ww)[0], j - 1)
    # the first score above theta sits in bin 0
    assert int(g.hist_bin_spec(_ulp_up(th).unsqueeze(0), th, ww)) == 0
    # edge(NB) bounds nothing: the last bin is open above
    top = e[NB].reshape(1, 1)
    assert int(g.hist_bin_spec(top, th, ww)) == NB - 1
    assert int(g.hist_bin_spec(_ulp_up(top), th, ww)) == NB - 1


def test_bin_matches_search_over_edges():
    gen = torch.Generator().manual_seed(5)
    th = torch.rand(64, generator=gen) * 0.8
    ww = (1.0625 - th) / NB
    v = th.unsqueeze(1) + torch.rand(64, 4000, generator=gen) * (1.2 - th).unsqueeze(1)
    v = torch.maximum(v, _ulp_up(th).unsqueeze(1))
    e = g.hist_edges(th, ww)
    # bin = number of inner edges strictly below v
    want = (v.unsqueeze(2) > e[:, 1:NB].unsqueeze(1)).sum(dim=2)
    assert torch.equal(g.hist_bin_spec(v, th, ww), want)


def test_far_past_hi_inf_and_nan_land_in_range():
    th = torch.tensor([0.5], dtype=torch.float32)
    ww = torch.tensor([0.002], dtype=torch.float32)
    v = torch.tensor([[2.0, 1e30, 3.4e38, INF]], dtype=torch.float32)
    assert g.hist_bin_spec(v, th, ww)[0].tolist() == [NB - 1] * 4
    b = g.hist_bin_spec(torch.tensor([[float("nan")]]), th, ww)
    assert 0 <= int(b) < NB


def test_tiny_w_sends_every_hit_to_the_last_bin():
    th = torch.tensor([0.5, -0.3, 7.0], dtype=torch.float32)
    ww = torch.full((3,), 1e-30, dtype=torch.float32)
    v = torch.stack([_ulp_up(th), th + 0.01, th + 100.0], dim=1)
    assert (g.hist_bin_spec(v, th, ww) == NB - 1).all()


# ---- the plan on hand-built histograms ------------------------------------

CAP = 32


def _query(theta, w, retained_bins, dropped_bins):
    """Scores in the middle of the given bins; returns (scores[CAP], hist[NB],
    count)."""
    assert len(retained_bins) == CAP
    mid = torch.tensor([theta + (b + 0.5) * w for b in retained_bins], dtype=torch.float32)
    hist = torch.zeros(NB, dtype=torch.int32)
    for b in dropped_bins:
        hist[b] += 1
    return mid, hist, CAP + len(dropped_bins)


def _plan(queries, need, theta=0.25, w=0.003):
    cs = torch.stack([q[0] for q in queries])
    hist = torch.stack([q[1] for q in queries])
    counts = torch.tensor([q[2] for q in queries], dtype=torch.int32)
    th = torch.full((len(queries),), theta, dtype=torch.float32)
    ww = torch.full((len(queries),), w, dtype=torch.float32)
    return g.overflow_rescan_plan(cs, counts, hist, th, ww, CAP, need), th, ww


def test_plan_set_that_fits_exactly():
    # bins 200.. hold exactly CAP hits (20 retained + 12 dropped); bin 199
    # holds one more
    q = _query(0.25, 0.003, [200 + i % 20 for i in range(20)] + [5] * 12,
               [210] * 12 + [199] + [3] * 40)
    (theta2, expect_n, ok), th, ww = _plan([q], need=16)
    assert int(expect_n) == CAP and bool(ok)
    assert float(theta2) == float(g.hist_edges(th, ww)[0, 200])


def test_plan_bin_that_jumps_past_cap_is_not_ok():
    # 5 hits above bin 100, then bin 100 alone holds CAP + 3
    q = _query(0.25, 0.003, [100] * 30 + [150, 151], [100] * 5 + [160, 170, 180])
    (theta2, expect_n, ok), th, ww = _plan([q], need=16)
    assert int(expect_n) == 5 and not bool(ok)
    assert float(theta2) == float(g.hist_edges(th, ww)[0, 101])
    # the same histogram is fine for a query that needs 5 or fewer
    (_, expect_n, ok), _, _ = _plan([q], need=5)
    assert int(expect_n) == 5 and bool(ok)


def test_plan_need_per_query():
    q = _query(0.25, 0.003, [100] * 30 + [150, 151], [100] * 5 + [160, 170, 180])
    need = torch.tensor([16, 5, 6, 1])
    (_, expect_n, ok), _, _ = _plan([q, q, q, q], need=need)
    assert expect_n.tolist() == [5, 5, 5, 5]
    assert ok.tolist() == [False, True, False, True]


def test_plan_last_bin_over_cap_fits_nowhere():
    q = _query(0.25, 0.003, [NB - 1] * CAP, [NB - 1] * 3)
    (theta2, expect_n, ok), _, _ = _plan([q], need=1)
    assert float(theta2) == INF and int(expect_n) == 0 and not bool(ok)


def test_plan_leaves_fitting_queries_untouched():
    over = _query(0.25, 0.003, [200] * CAP, [10] * 9)
    cs = torch.full((CAP,), -1e30)
    cs[:7] = torch.tensor([0.3, 0.31, 0.4, 0.5, 0.6, 0.7, 0.26])
    fit = (cs, torch.zeros(NB, dtype=torch.int32), 7)
    full = (over[0], torch.zeros(NB, dtype=torch.int32), CAP)  # exactly cap: fits
    none = (torch.full((CAP,), -1e30), torch.zeros(NB, dtype=torch.int32), 0)
    (theta2, expect_n, ok), th, _ = _plan([fit, over, full, none], need=4)
    assert theta2[[0, 2, 3]].tolist() == th[[0, 2, 3]].tolist()
    assert expect_n.tolist() == [7, CAP, CAP, 0]
    assert ok.tolist() == [False, True, False, False]
    assert float(theta2[1]) > float(th[1])


# ---- property: a rescan at theta2 keeps exactly expect_n hits ---------------

@pytest.mark.parametrize("seed", range(6))
def test_plan_expect_n_is_the_count_above_theta2(seed):
    gen = torch.Generator().manual_seed(100 + seed)
    nq, n, cap = 48, 3000, 64
    # clustered tails: a Gaussian bulk plus per-query clusters near the top,
    # some with exact duplicates
    scores = torch.randn(nq, n, generator=gen) * 0.05
    n_hot = torch.randint(0, 400, (nq,), generator=gen)
    hot = 0.6 + 0.35 * torch.rand(nq, n, generator=gen) ** 3
    scores = torch.where(torch.arange(n).unsqueeze(0) < n_hot.unsqueeze(1), hot, scores)
    scores[::7, :90] = scores[::7, :1]
    theta = torch.quantile(scores, 0.9, dim=1) * torch.rand(nq, generator=gen)
    hi = torch.full((nq,), 1.0625)
    w = (hi - theta) / NB
    hits = scores > theta.unsqueeze(1)
    counts = hits.sum(dim=1).to(torch.int32)
    assert int((counts > cap).sum()) > nq // 2
    # the scan keeps the first cap arrivals in some order: take a random one
    order = torch.rand(nq, n, generator=gen).masked_fill(~hits, 2.0).argsort(dim=1)
    kept = order[:, :cap]
    kept_live = torch.arange(cap).unsqueeze(0) < counts.unsqueeze(1)
    cs = torch.where(kept_live, scores.gather(1, kept), torch.full((nq, cap), -1e30))
    dropped = hits.clone()
    dropped.scatter_(1, kept, False)
    bins = g.hist_bin_spec(scores, theta, w)
    hist = torch.zeros(nq, NB, dtype=torch.int64)
    hist.scatter_add_(1, bins, dropped.long())

    theta2, expect_n, ok = g.overflow_rescan_plan(
        cs, counts, hist.to(torch.int32), theta, w, cap, need=16)
    over = counts > cap
    got = (scores > theta2.unsqueeze(1)).sum(dim=1)
    assert torch.equal(got, expect_n)
    assert (expect_n[over] <= cap).all()
    assert torch.equal(ok, over & (expect_n >= 16))
    assert torch.equal(theta2[~over], theta[~over])
    # the largest set that fits: one bin lower would not
    e = g.hist_edges(theta, w)
    for q in over.nonzero().flatten().tolist():
        j = int((e[q, :NB] == theta2[q]).nonzero()[0]) if theta2[q] != INF else NB
        assert j >= 1
        assert int((scores[q] > e[q, j - 1]).sum()) > cap
