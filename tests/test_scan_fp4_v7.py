"""fp4x4 threshold scan v7 (any-hit fast path, hoisted staging addresses,
prestaged tile boundary) against the v1 kernel in the same process.

v1 is tied to the fp32 reference by test_topk_recall_threshold_fp4x4; here
v7 must reproduce v1's candidates bit for bit. Shapes are the smallest at
which the new code paths differ: two query blocks (the second with 44 live
rows), two swaths with several tile boundaries and a ragged 77-row last
tile, and K depths np = 1, 2, 3, 8 (single-pair interval, restaging the
buffers just read, odd tail interval, production depth), plus a single
tile with nothing to prestage.
"""

import functools

import pytest
import torch

from vainplex_openclaw_amd.ops import gpu as g

pytestmark = pytest.mark.gpu

V1, V7 = 0, 7
CAP = 4096
FILL_SCORE = -1e30
FILL_ID = -1

SHAPES = [
    (300, 1613, 2, 128),
    (300, 1613, 2, 256),
    (300, 1613, 2, 384),
    (300, 1613, 2, 1024),
    (256, 256, 1, 1024),
]
IDS = [f"nq{nq}-nx{nx}-S{s}-D{d}" for nq, nx, s, d in SHAPES]


def _scan(c, theta, variant):
    cs, ci, cn = g.ext().topk_scan_threshold_fp4x4(
        c["Q4"], c["QS"], c["X4"], c["XS"], theta.contiguous(), CAP, c["S"], variant)
    torch.cuda.synchronize()
    return cs, ci, cn


def _dense(cs, ci, cn, nx):
    """[nq, nx] score matrix from a scan that kept every column."""
    nq = cs.shape[0]
    assert (cn == nx).all(), "dense scan must keep every column"
    ids = ci[:, :nx].long()
    assert (ids.sort(dim=1).values == torch.arange(nx, device=ids.device)).all()
    out = torch.full((nq, nx), float("nan"), device=cs.device)
    out.scatter_(1, ids, cs[:, :nx])
    return out


def _sorted_lists(cs, ci, cn):
    """Per-row (id, score) lists sorted by id; unused slots pushed to the end."""
    pos = torch.arange(cs.shape[1], device=cs.device).unsqueeze(0)
    live = pos < cn.unsqueeze(1)
    key = torch.where(live, ci.long(), torch.full_like(ci, 2**31 - 1).long())
    key, order = key.sort(dim=1)
    sc = torch.where(live, cs, torch.zeros_like(cs)).gather(1, order)
    return key, sc.view(torch.int32)


@functools.lru_cache(maxsize=None)
def _case(nq, nx, S, D):
    torch.manual_seed(11)
    Q = torch.nn.functional.normalize(torch.randn(nq, D, device="cuda"), dim=1).bfloat16()
    X = torch.nn.functional.normalize(torch.randn(nx, D, device="cuda"), dim=1).bfloat16()
    Q4, QS = g.to_fp4_mx(Q)
    X4, XS = g.to_fp4_mx(X)
    c = {"Q4": Q4, "QS": QS, "X4": X4, "XS": XS, "S": S, "nq": nq, "nx": nx}
    lo = torch.full((nq,), -1e9, device="cuda")
    c["dense_v1"] = _dense(*_scan(c, lo, V1), nx)
    return c


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_dense_matches_v1(shape):
    c = _case(*shape)
    lo = torch.full((c["nq"],), -1e9, device="cuda")
    cs, ci, cn = _scan(c, lo, V7)
    assert (cn == c["nx"]).all()
    got = _dense(cs, ci, cn, c["nx"])
    assert torch.equal(got.view(torch.int32), c["dense_v1"].view(torch.int32))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_quantile_theta_matches_v1(shape):
    c = _case(*shape)
    theta = torch.quantile(c["dense_v1"], 0.995, dim=1)
    cs1, ci1, cn1 = _scan(c, theta, V1)
    cs7, ci7, cn7 = _scan(c, theta, V7)
    assert int(cn1.sum()) > 0
    assert torch.equal(cn7, cn1)
    assert torch.equal(cn1.long(), (c["dense_v1"] > theta.unsqueeze(1)).sum(dim=1))
    ids1, sc1 = _sorted_lists(cs1, ci1, cn1)
    ids7, sc7 = _sorted_lists(cs7, ci7, cn7)
    assert torch.equal(ids7, ids1)
    assert torch.equal(sc7, sc1)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_single_hit_lands(shape):
    c = _case(*shape)
    top = c["dense_v1"].topk(2, dim=1)
    a, b = top.values[:, 0], top.values[:, 1]
    theta = (a + b) * 0.5
    # exact ties (and midpoints that round onto the top score) cannot
    # isolate one hit
    ok = (a > theta) & ~(b > theta)
    assert float((~ok).float().mean()) <= 0.05
    cs, ci, cn = _scan(c, theta, V7)
    assert (cn[ok] == 1).all()
    assert torch.equal(ci[ok, 0].long(), top.indices[ok, 0])
    assert torch.equal(cs[ok, 0].view(torch.int32), a[ok].view(torch.int32))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_no_hit_leaves_buffers_untouched(shape):
    c = _case(*shape)
    hi = torch.full((c["nq"],), 1e9, device="cuda")
    cs, ci, cn = _scan(c, hi, V7)
    assert (cn == 0).all()
    assert (cs == torch.tensor(FILL_SCORE, dtype=torch.float32, device="cuda")).all()
    assert (ci == FILL_ID).all()
