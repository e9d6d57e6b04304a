"""fp4x4 threshold scan with the dropped-hit histogram
(topk_scan_fp4_hist_kernel, topk_scan_fp4_owned_hist_kernel) against the
dense v1 score matrix of test_scan_fp4_v10.py.

cap = 64 and theta at the per-query 0.90 quantile (about 161 hits per query
of 1613 columns) overflow the buffer; every third query has theta at the
0.999 quantile (one or two hits) instead, so overflowing and fitting queries
share every wave. For every query:
  - counts is the dense hit count,
  - hist sums to max(counts - cap, 0),
  - hist + bins(retained scores) is the histogram of ALL dense hits under
    ops.gpu.hist_bin_spec, exactly: the kernel's bin rule is the spec's, bit
    for bit, and retained plus dropped hits are all the hits,
  - the retained (id, score) pairs are dense hits, bit for bit, no id twice.
The owned entry is checked the same way against the owner-masked dense
matrix, with the owners of test_scan_fp4_owned_v10.py (3 owners, unfiltered
queries -1 / -7 in rows 0..127 and at row 290).

Then the plan (ops.gpu.overflow_rescan_plan) and a rescan of the overflowed
rows with the plain v10 / owned kernels at theta2 (ops.gpu.fp4x4_rescan):
counts2 == expect_n <= cap, exactly.
"""

import pytest
import torch

from vainplex_openclaw_amd.ops import gpu as g

from test_scan_fp4_v10 import FAMILIES, _case, _id
from test_scan_fp4_owned_v10 import _owners

pytestmark = pytest.mark.gpu

NB = g.HIST_NB
CAP = 64
SHAPES = [(300, 1613, 2, 128), (300, 1613, 2, 512), (300, 1613, 2, 1024)]
CASES = [(f, s, o) for f in FAMILIES for s in SHAPES for o in (False, True)]


def _theta_w(dense):
    theta = torch.quantile(dense, 0.90, dim=1)
    high = torch.quantile(dense, 0.999, dim=1)
    third = torch.arange(dense.shape[0], device="cuda") % 3 == 2
    theta = torch.where(third, high, theta).contiguous()
    # bins up to a little over the largest score: every bin region is used
    hi = dense.max(dim=1).values * 1.0625
    w = ((hi - theta) / NB).contiguous()
    assert (w > 0).all()
    return theta, w


def _hist_of(bins, mask):
    h = torch.zeros(bins.shape[0], NB, dtype=torch.int64, device=bins.device)
    h.scatter_add_(1, bins, mask.long())
    return h


@pytest.mark.parametrize(
    "family,shape,owned", CASES,
    ids=[f"{f}-{_id(s)}-{'owned' if o else 'plain'}" for f, s, o in CASES])
def test_hist_scan_and_rescan(family, shape, owned):
    c = _case(family, *shape)
    nq, nx = c["nq"], c["nx"]
    dense = c["dense_v1"]
    theta, w = _theta_w(dense)
    mask = dense > theta.unsqueeze(1)
    own = {}
    if owned:
        xo, qo = _owners(3, nq, nx)
        own = {"xowner": xo, "qowner": qo}
        eligible = (qo < 0).unsqueeze(1) | (xo.unsqueeze(0) == qo.unsqueeze(1))
        assert int((mask & ~eligible).sum()) > 0  # the filter bites
        mask = mask & eligible
    want_n = mask.sum(dim=1)
    over = want_n > CAP
    # both kinds of query, next to each other. With owners a third of 161
    # hits mostly fits: the 17 unfiltered queries at the 0.90 quantile
    # overflow for sure, a few owned ones may.
    assert int(over.sum()) >= (17 if owned else nq // 3)
    assert int((~over & (want_n > 0)).sum()) > nq // 6

    cs, ci, cn, hist = g.ext().topk_scan_threshold_fp4x4_hist(
        c["Q4"], c["QS"], c["X4"], c["XS"], theta, w, CAP, c["S"], **own)
    torch.cuda.synchronize()
    assert hist.shape == (nq, NB) and hist.dtype == torch.int32
    assert torch.equal(cn.long(), want_n)
    assert torch.equal(hist.sum(dim=1).long(), (want_n - CAP).clamp_min(0))
    assert (hist >= 0).all()

    # retained pairs: dense hits, bit for bit, each id once
    live = torch.arange(CAP, device="cuda").unsqueeze(0) < cn.unsqueeze(1)
    ids = ci.long().clamp_min(0)
    assert (ci[live] >= 0).all() and (ci[~live] == -1).all()
    assert mask.gather(1, ids)[live].all()
    assert torch.equal(cs[live].view(torch.int32),
                       dense.gather(1, ids)[live].view(torch.int32))
    seen = torch.zeros(nq, nx, dtype=torch.int64, device="cuda")
    seen.scatter_add_(1, ids, live.long())
    assert int(seen.max()) == 1

    # hist + bins(retained) == bins(all dense hits), exactly
    all_bins = _hist_of(g.hist_bin_spec(dense, theta, w), mask)
    kept_bins = _hist_of(g.hist_bin_spec(cs, theta, w), live)
    assert torch.equal(hist.long() + kept_bins, all_bins)
    # the dropped hits reach past the first bins (a clamp to bin 0 would pass
    # the sum check above)
    assert int(hist[:, NB // 2:].sum()) > 0

    # plan + rescan: the edge is the scan's own comparison
    theta2, expect_n, ok = g.overflow_rescan_plan(cs, cn, hist, theta, w, CAP, need=16)
    assert torch.equal(ok, over & (expect_n >= 16))
    assert int(ok.sum()) > 0
    rows = over.nonzero(as_tuple=True)[0]
    assert torch.isfinite(theta2[rows]).all()
    th2 = theta2[rows]
    # the plain v10 / owned kernels on the gathered rows
    cs2, ci2, cn2 = g.fp4x4_rescan(
        c["Q4"], c["QS"], (c["X4"], c["XS"]), theta2, rows, CAP,
        own.get("xowner"), own.get("qowner"), n_swaths=c["S"])
    torch.cuda.synchronize()
    assert torch.equal(cn2.long(), expect_n[rows])
    assert (cn2 <= CAP).all()
    assert torch.equal(cn2.long(), (mask[rows] & (dense[rows] > th2.unsqueeze(1))).sum(dim=1))
    # the largest set that fits: the next lower edge would overflow
    e = g.hist_edges(theta, w)[rows]
    j = (e[:, :NB] == th2.unsqueeze(1)).long().argmax(dim=1)
    assert (j >= 1).all()
    lower = e.gather(1, (j - 1).unsqueeze(1))
    assert ((mask[rows] & (dense[rows] > lower)).sum(dim=1) > CAP).all()


def test_no_overflow_leaves_hist_zero():
    c = _case("gauss", *SHAPES[1])
    theta = torch.quantile(c["dense_v1"], 0.99, dim=1).contiguous()  # ~16 hits
    w = torch.full_like(theta, 1e-3)
    cs, ci, cn, hist = g.ext().topk_scan_threshold_fp4x4_hist(
        c["Q4"], c["QS"], c["X4"], c["XS"], theta, w, CAP, c["S"])
    cs0, ci0, cn0 = g.ext().topk_scan_threshold_fp4x4(
        c["Q4"], c["QS"], c["X4"], c["XS"], theta, CAP, c["S"], 10)
    torch.cuda.synchronize()
    assert int(cn.max()) <= CAP and int(hist.abs().sum()) == 0
    assert torch.equal(cn, cn0)
    assert torch.equal(cs.sort(dim=1).values, cs0.sort(dim=1).values)


def test_tiny_w_counts_every_dropped_hit_in_the_last_bin():
    c = _case("gauss", *SHAPES[0])
    theta = torch.quantile(c["dense_v1"], 0.90, dim=1).contiguous()
    w = torch.full_like(theta, 1e-30)
    cs, ci, cn, hist = g.ext().topk_scan_threshold_fp4x4_hist(
        c["Q4"], c["QS"], c["X4"], c["XS"], theta, w, CAP, c["S"])
    torch.cuda.synchronize()
    assert int(hist[:, :NB - 1].sum()) == 0
    assert torch.equal(hist[:, NB - 1].long(), (cn.long() - CAP).clamp_min(0))
    theta2, expect_n, ok = g.overflow_rescan_plan(cs, cn, hist, theta, w, CAP, need=16)
    assert not bool(ok.any())
