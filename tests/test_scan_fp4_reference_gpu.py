"""Every kernel that computes the MXFP4 scaled dot product, against the fp64
decode reference (ops.gpu.reference_fp4x4_scores): the nibbles decoded with
the e2m1 grid, times 2^(scale - 127), fp64 matmul on the GPU. Nothing here
compares a kernel with another kernel.

Each scan runs dense (theta = -1e9, CAP = 4096 >= nx, two swaths), its
candidates are un-scattered by id into an [nq, nx] matrix, and every cell
must satisfy |got - ref| <= bound with bound = D * 2^-22 * sum |q_i||x_i|
(derived in reference_scores_bound; a worst case for an fp32 accumulator,
not a measured figure). tests/test_fp4_reference.py shows on the CPU that
this bound tells a right kernel from the old 16 B piece clamp of the scale
sheets by orders of magnitude at every D below but 512 and 1024.

Shapes: (nq, nx) = (303, 1613), (301, 1614), (302, 1615): two query blocks
with a ragged second one, several X tiles per swath, a ragged last tile,
and every residue of rows * D/32 mod 16, on both operands. D = 128 .. 1024
in steps of 128: every scale row pitch, the 16 B staging path (512, 1024)
and the dword path (the rest).

Each test prints the largest err / bound it saw (pytest -s shows it);
profiles/README.md, "fp4 scan vs fp64 reference", records them.
"""

import functools

import pytest
import torch

from vainplex_openclaw_amd.ops import gpu as g

from test_fp4_reference import DEPTHS, FAMILIES, SHAPES, rows

pytestmark = pytest.mark.gpu

CAP = 4096
S = 2
V1, V10 = 0, 10
OTHER_VARIANTS = [1, 2, 4, 7, 9]  # v2, v3, v5, v7, v9
FEW_DEPTHS = [128, 640, 1024]
FP8_DEPTHS = [128, 640, 1024, 1280, 2048]


def _sid(shape):
    return f"nq{shape[0]}-nx{shape[1]}"


@functools.lru_cache(maxsize=None)
def _rows(family, D):
    """bf16 rows for the largest shape; smaller shapes take leading rows."""
    torch.manual_seed(11)
    nq = max(s[0] for s in SHAPES)
    nx = max(s[1] for s in SHAPES)
    return rows(nq, D, family, "cuda"), rows(nx, D, family, "cuda")


@functools.lru_cache(maxsize=None)
def _case(family, D, nq, nx):
    """Operands and (ref, bound); computed once, shared read-only."""
    Q, X = _rows(family, D)
    Q4, QS = g.to_fp4_mx(Q[:nq])
    X4, XS = g.to_fp4_mx(X[:nx])
    ref, bound = g.reference_fp4x4_scores(Q4, QS, X4, XS)
    return {"Q4": Q4, "QS": QS, "X4": X4, "XS": XS, "nq": nq, "nx": nx,
            "ref": ref, "bound": bound,
            "lo": torch.full((nq,), -1e9, device="cuda")}


def _dense(cs, ci, cn, nx):
    """[nq, nx] score matrix from a scan that kept every column."""
    nq = cs.shape[0]
    assert (cn == nx).all(), "dense scan must keep every column"
    ids = ci[:, :nx].long()
    assert (ids.sort(dim=1).values == torch.arange(nx, device=ids.device)).all()
    out = torch.full((nq, nx), float("nan"), device=cs.device)
    out.scatter_(1, ids, cs[:, :nx])
    return out


def _check(name, got, ref, bound, mask=None):
    """|got - ref| <= bound on every cell (of mask); prints the worst ratio."""
    err = (got.double() - ref).abs()
    ratio = torch.where(bound > 0, err / bound, torch.zeros_like(err))
    over = ~(err <= bound)  # a NaN is over
    if mask is not None:
        ratio, over = ratio[mask], over[mask]
    print(f"\nfp4ref {name} max_err_over_bound={float(ratio.max()):.3e} "
          f"cells_over={int(over.sum())}")
    assert int(over.sum()) == 0


def _scan(c, variant):
    out = g.ext().topk_scan_threshold_fp4x4(
        c["Q4"], c["QS"], c["X4"], c["XS"], c["lo"], CAP, S, variant, False)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
@pytest.mark.parametrize("D", DEPTHS)
@pytest.mark.parametrize("variant", [V1, V10], ids=["v1", "v10"])
def test_fp4x4_scan_vs_fp64(variant, D, shape, family):
    c = _case(family, D, *shape)
    got = _dense(*_scan(c, variant), c["nx"])
    _check(f"variant{variant} D{D} {_sid(shape)} {family}", got, c["ref"], c["bound"])


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("D", FEW_DEPTHS)
@pytest.mark.parametrize("variant", OTHER_VARIANTS)
def test_fp4x4_scan_other_variants_vs_fp64(variant, D, family):
    c = _case(family, D, *SHAPES[0])
    got = _dense(*_scan(c, variant), c["nx"])
    _check(f"variant{variant} D{D} {_sid(SHAPES[0])} {family}", got, c["ref"], c["bound"])


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("D", FEW_DEPTHS)
def test_owned_scan_unfiltered_vs_fp64(D, family):
    """qowner = -1 everywhere: the owned kernel returns the full matrix."""
    c = _case(family, D, *SHAPES[0])
    nq, nx = c["nq"], c["nx"]
    xo = (torch.arange(nx, device="cuda") % 3).int()
    qo = torch.full((nq,), -1, dtype=torch.int32, device="cuda")
    cs, ci, cn = g.ext().topk_scan_threshold_fp4x4_owned(
        c["Q4"], c["QS"], c["X4"], c["XS"], c["lo"], xo, qo, CAP, S)
    torch.cuda.synchronize()
    _check(f"owned-wild D{D} {family}", _dense(cs, ci, cn, nx), c["ref"], c["bound"])


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("D", FEW_DEPTHS)
def test_owned_scan_round_robin_vs_fp64(D, family):
    """Three owners round-robin over rows and queries: a query's candidates
    are exactly its owner's columns, scores within bound."""
    c = _case(family, D, *SHAPES[0])
    nq, nx = c["nq"], c["nx"]
    xo = (torch.arange(nx, device="cuda") % 3).int()
    qo = (torch.arange(nq, device="cuda") % 3).int()
    cs, ci, cn = g.ext().topk_scan_threshold_fp4x4_owned(
        c["Q4"], c["QS"], c["X4"], c["XS"], c["lo"], xo, qo, CAP, S)
    torch.cuda.synchronize()
    mine = xo.unsqueeze(0) == qo.unsqueeze(1)
    assert torch.equal(cn.long(), mine.sum(dim=1))
    live = torch.arange(CAP, device="cuda").unsqueeze(0) < cn.unsqueeze(1)
    assert (ci[live] >= 0).all() and (ci[live] < nx).all() and (ci[~live] == -1).all()
    got = torch.full((nq, nx), float("nan"), device="cuda")
    seen = torch.zeros(nq, nx, dtype=torch.int64, device="cuda")
    ids = ci.long().clamp_min(0)
    seen.scatter_add_(1, ids, live.long())
    assert torch.equal(seen, mine.long())  # each of its columns once, no other
    r = torch.arange(nq, device="cuda").unsqueeze(1).expand_as(ids)
    got[r[live], ids[live]] = cs[live]
    _check(f"owned-rr D{D} {family}", got, c["ref"], c["bound"], mask=mine)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("D", FEW_DEPTHS)
def test_hist_scan_vs_fp64(D, family):
    """Dense, nothing dropped: scores within bound, histogram all zero."""
    c = _case(family, D, *SHAPES[0])
    w = torch.full((c["nq"],), 0.25, device="cuda")
    cs, ci, cn, hist = g.ext().topk_scan_threshold_fp4x4_hist(
        c["Q4"], c["QS"], c["X4"], c["XS"], c["lo"], w, CAP, S)
    torch.cuda.synchronize()
    assert int(hist.abs().sum()) == 0
    _check(f"hist D{D} {family}", _dense(cs, ci, cn, c["nx"]), c["ref"], c["bound"])


@functools.lru_cache(maxsize=None)
def _case_fp8(family, D, nq, nx):
    torch.manual_seed(12)
    Q = rows(nq, D, family, "cuda")
    X = rows(nx, D, family, "cuda")
    Q8 = g.to_fp8_bytes(Q)
    X4, XS = g.to_fp4_mx(X)
    q = Q8.view(torch.float8_e4m3fn).float().double()  # x8 units, natural order
    x = g.reference_fp4_decode(X4, XS, natural_order=True)
    ref, bound = g.reference_scores_bound(q, x)
    return Q8, X4, XS, ref, bound


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
@pytest.mark.parametrize("D", FP8_DEPTHS)
def test_fp8xfp4_scan_vs_fp64(D, shape, family):
    """fp8 Q x fp4 X (topk_scan_mx4_kernel), fed by the same scale staging;
    scores and theta in the x8 units of to_fp8_bytes."""
    nq, nx = shape
    Q8, X4, XS, ref, bound = _case_fp8(family, D, nq, nx)
    lo = torch.full((nq,), -1e9, device="cuda")
    cs, ci, cn = g.ext().topk_scan_threshold_fp4(Q8, X4, XS, lo, CAP, S)
    torch.cuda.synchronize()
    _check(f"fp8xfp4 D{D} {_sid(shape)} {family}", _dense(cs, ci, cn, nx), ref, bound)
