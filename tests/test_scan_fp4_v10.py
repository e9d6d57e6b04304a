"""fp4x4 threshold scan v10 (v9 on the fragment swizzle that is conflict-free
on the real ds_read_b128 lane groups) against the v1 kernel in the same
process.

v1 is tied to the fp32 reference by test_topk_recall_threshold_fp4x4; v10
changes only where a 16 B slot sits inside its 64 B LDS row, on the staging
and on the read side together, so it must reproduce v1's candidates bit for
bit. Shapes, input families and checks are those of test_scan_fp4_v9.py:
two query blocks (the second with 44 live rows), two swaths with several
tile boundaries and a ragged 77-row last tile (the row clamp in the
swizzled source offsets runs), K depths np = 1, 2, 3, 4, 5, 8, plus a
single tile. Every tile has all four row quads and all four kgrp, so every
(quad, slot) entry of the new slot function is exercised by every case.

A wrong slot swaps 32-element blocks of a row under the scales of other
blocks. On normalised Gaussian rows neighbouring blocks have like
magnitudes; the block-scaled family (each 32-element block times
2**randint(-6, 7) before normalising) makes such a swap change the score
by orders of magnitude.
"""

import functools

import pytest
import torch

from vainplex_openclaw_amd.ops import gpu as g

pytestmark = pytest.mark.gpu

V1, V9, V10 = 0, 9, 10
CAP = 4096
FILL_SCORE = -1e30
FILL_ID = -1

SHAPES = [
    (300, 1613, 2, 128),
    (300, 1613, 2, 256),
    (300, 1613, 2, 384),
    (300, 1613, 2, 512),
    (300, 1613, 2, 640),
    (300, 1613, 2, 1024),
    (256, 256, 1, 1024),
]
# the v7 file's own shapes: its cap on ambiguous single-hit rows is known
# to hold there on Gaussian rows
SINGLE_HIT_SHAPES = [
    (300, 1613, 2, 128),
    (300, 1613, 2, 256),
    (300, 1613, 2, 384),
    (300, 1613, 2, 1024),
    (256, 256, 1, 1024),
]
FAMILIES = ["gauss", "blockscaled"]


def _id(shape):
    nq, nx, s, d = shape
    return f"nq{nq}-nx{nx}-S{s}-D{d}"


def _scan(c, theta, variant, scan_only=False):
    cs, ci, cn = g.ext().topk_scan_threshold_fp4x4(
        c["Q4"], c["QS"], c["X4"], c["XS"], theta.contiguous(), CAP, c["S"], variant,
        scan_only)
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


def _rows(n, D, family):
    v = torch.randn(n, D, device="cuda")
    if family == "blockscaled":
        e = torch.randint(-6, 7, (n, D // 32, 1), device="cuda")
        v = (v.view(n, D // 32, 32) * torch.exp2(e.float())).view(n, D)
    return torch.nn.functional.normalize(v, dim=1).bfloat16()


@functools.lru_cache(maxsize=None)
def _case(family, nq, nx, S, D):
    """Operands and the v1 dense score matrix; computed once per shape and
    shared (read-only) with test_scan_fp4_owned_v10.py."""
    torch.manual_seed(11)
    Q4, QS = g.to_fp4_mx(_rows(nq, D, family))
    X4, XS = g.to_fp4_mx(_rows(nx, D, family))
    c = {"Q4": Q4, "QS": QS, "X4": X4, "XS": XS, "S": S, "nq": nq, "nx": nx}
    lo = torch.full((nq,), -1e9, device="cuda")
    c["dense_v1"] = _dense(*_scan(c, lo, V1), nx)
    return c


# block-scaled D = 128 and D = 512 first: the cheapest proof of the slot map
DENSE_CASES = (
    [("blockscaled", SHAPES[0]), ("blockscaled", SHAPES[3])]
    + [("blockscaled", s) for i, s in enumerate(SHAPES) if i not in (0, 3)]
    + [("gauss", s) for s in SHAPES]
)
ALL_CASES = [(f, s) for f in FAMILIES for s in SHAPES]


def _ids(cases):
    return [f"{f}-{_id(s)}" for f, s in cases]


@pytest.mark.parametrize("family,shape", DENSE_CASES, ids=_ids(DENSE_CASES))
def test_dense_matches_v1(family, shape):
    c = _case(family, *shape)
    lo = torch.full((c["nq"],), -1e9, device="cuda")
    cs, ci, cn = _scan(c, lo, V10)
    assert (cn == c["nx"]).all()
    got = _dense(cs, ci, cn, c["nx"])
    assert torch.equal(got.view(torch.int32), c["dense_v1"].view(torch.int32))


@pytest.mark.parametrize("family,shape", ALL_CASES, ids=_ids(ALL_CASES))
def test_quantile_theta_matches_v1(family, shape):
    c = _case(family, *shape)
    theta = torch.quantile(c["dense_v1"], 0.995, dim=1)
    cs1, ci1, cn1 = _scan(c, theta, V1)
    cs10, ci10, cn10 = _scan(c, theta, V10)
    assert int(cn1.sum()) > 0
    assert torch.equal(cn10, cn1)
    assert torch.equal(cn1.long(), (c["dense_v1"] > theta.unsqueeze(1)).sum(dim=1))
    ids1, sc1 = _sorted_lists(cs1, ci1, cn1)
    ids10, sc10 = _sorted_lists(cs10, ci10, cn10)
    assert torch.equal(ids10, ids1)
    assert torch.equal(sc10, sc1)


@pytest.mark.parametrize("family,shape", ALL_CASES, ids=_ids(ALL_CASES))
def test_no_hit_leaves_buffers_untouched(family, shape):
    c = _case(family, *shape)
    hi = torch.full((c["nq"],), 1e9, device="cuda")
    cs, ci, cn = _scan(c, hi, V10)
    assert (cn == 0).all()
    assert (cs == torch.tensor(FILL_SCORE, dtype=torch.float32, device="cuda")).all()
    assert (ci == FILL_ID).all()


@pytest.mark.parametrize("shape", SINGLE_HIT_SHAPES,
                         ids=[_id(s) for s in SINGLE_HIT_SHAPES])
def test_single_hit_lands(shape):
    c = _case("gauss", *shape)
    top = c["dense_v1"].topk(2, dim=1)
    a, b = top.values[:, 0], top.values[:, 1]
    theta = (a + b) * 0.5
    # exact ties (and midpoints that round onto the top score) cannot
    # isolate one hit
    ok = (a > theta) & ~(b > theta)
    assert float((~ok).float().mean()) <= 0.05
    cs, ci, cn = _scan(c, theta, V10)
    assert (cn[ok] == 1).all()
    assert torch.equal(ci[ok, 0].long(), top.indices[ok, 0])
    assert torch.equal(cs[ok, 0].view(torch.int32), a[ok].view(torch.int32))


def test_scan_only_launches():
    c = _case("blockscaled", *SHAPES[4])
    theta = torch.quantile(c["dense_v1"], 0.995, dim=1)
    cs, ci, cn = _scan(c, theta, V10, scan_only=True)
    # the K-loops ran without the epilogue: nothing is appended
    assert cs.shape == (c["nq"], CAP) and ci.shape == (c["nq"], CAP)
    assert (cn == 0).all()


def test_dense_matches_v9():
    c = _case("blockscaled", *SHAPES[5])
    lo = torch.full((c["nq"],), -1e9, device="cuda")
    d9 = _dense(*_scan(c, lo, V9), c["nx"])
    d10 = _dense(*_scan(c, lo, V10), c["nx"])
    assert torch.equal(d10.view(torch.int32), d9.view(torch.int32))
