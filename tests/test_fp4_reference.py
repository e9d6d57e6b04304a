"""The fp64 decode reference of the MXFP4 scaled dot product
(ops.gpu.reference_fp4_decode, reference_fp4x4_scores), checked on the CPU,
and the proof that the bound it carries tells a right scan from the scale
staging bug the fp4 scans used to share.

The old rule (all fp4 scans before the row clamp): the e8m0 scale array
[rows][sb], sb = D/32, was staged in 16 B pieces and a piece that started
past the array's last whole 16 B was taken from that last whole 16 B. For
sb % 16 != 0 pieces straddle rows, and with rows * sb % 16 != 0 the tail of
the array, live rows included, was scored with the scale bytes from 16 B
earlier. _old_piece_clamp below applies that rule to a scale array; the
power check shows that at the shapes of test_scan_fp4_reference_gpu.py such
scores leave the bound by whole rows or columns at every D but 512 and 1024,
where the rule moved no live byte.

Shapes, depths and input families are shared with the GPU file, which
imports them from here.
"""

import functools

import pytest
import torch

from vainplex_openclaw_amd.ops import gpu as g

# (nq, nx): two query blocks with a ragged second one, several X tiles per
# swath (S = 2), a ragged last tile, and every residue of rows * sb mod 16
# the old clamp could hit, on both operands
SHAPES = [(303, 1613), (301, 1614), (302, 1615)]
DEPTHS = [128, 256, 384, 512, 640, 768, 896, 1024]
EXACT_DEPTHS = (512, 1024)  # sb % 16 == 0: the old rule was exact there
FAMILIES = ["gauss", "blockscaled"]


def rows(n, D, family, device):
    """Normalised bf16 rows; blockscaled: each 32-element block times
    2**randint(-6, 7) first, so a wrong scale or a swapped block changes a
    score by orders of magnitude."""
    v = torch.randn(n, D, device=device)
    if family == "blockscaled":
        e = torch.randint(-6, 7, (n, D // 32, 1), device=device)
        v = (v.view(n, D // 32, 32) * torch.exp2(e.float())).view(n, D)
    return torch.nn.functional.normalize(v, dim=1).bfloat16()


@functools.lru_cache(maxsize=None)
def _operands(family, D):
    """Quantised operands for the largest shape; smaller shapes slice them."""
    torch.manual_seed(11)
    nq = max(s[0] for s in SHAPES)
    nx = max(s[1] for s in SHAPES)
    Q4, QS = g.to_fp4_mx(rows(nq, D, family, "cpu"))
    X4, XS = g.to_fp4_mx(rows(nx, D, family, "cpu"))
    return Q4, QS, X4, XS


def _case(family, D, nq, nx):
    Q4, QS, X4, XS = _operands(family, D)
    return Q4[:nq], QS[:nq].contiguous(), X4[:nx], XS[:nx].contiguous()


def _old_piece_clamp(S):
    """Scale array as the fp4 scans used to see it: byte o taken from
    min(o & ~15, last) + (o & 15), last = the array's last whole 16 B."""
    flat = S.reshape(-1)
    total = flat.numel()
    last = max((total >> 4) * 16 - 16, 0)
    o = torch.arange(total)
    src = torch.minimum(o & ~15, torch.tensor(last)) + (o & 15)
    return flat[src].view_as(S)


@pytest.mark.parametrize("D", [128, 640])
def test_decode_natural_order_roundtrip(D):
    torch.manual_seed(0)
    n = 64
    X = torch.nn.functional.normalize(torch.randn(n, D), dim=1).bfloat16()
    X4, XS = g.to_fp4_mx(X)
    dec_p = g.reference_fp4_decode(X4, XS)
    dec = g.reference_fp4_decode(X4, XS, natural_order=True)
    assert dec.dtype == torch.float64 and dec.shape == (n, D)
    perm = (torch.arange(0, D, 128).unsqueeze(1) + g.fp4_perm128().unsqueeze(0)).reshape(-1)
    assert torch.equal(dec[:, perm], dec_p)
    # the assertion of test_to_fp4_mx_roundtrip_cpu
    err = (dec - X.double()).abs()
    grp_max = dec_p.abs().view(n, D // 32, 32).amax(2).repeat_interleave(32, 1)
    gm = torch.empty_like(grp_max)
    gm[:, perm] = grp_max
    assert (err <= gm / 3 + 0.08).all()
    cos = torch.nn.functional.cosine_similarity(dec, X.double(), dim=1)
    assert cos.min() > 0.98


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("D", [128, 640])
def test_stored_order_dot_equals_natural_order_dot(D, family):
    Q4, QS, X4, XS = _case(family, D, 37, 95)
    ref, bound = g.reference_fp4x4_scores(Q4, QS, X4, XS)
    assert ref.dtype == torch.float64 and ref.shape == (37, 95)
    assert bound.dtype == torch.float64 and bound.shape == (37, 95)
    qn = g.reference_fp4_decode(Q4, QS, natural_order=True)
    xn = g.reference_fp4_decode(X4, XS, natural_order=True)
    # Exactly: a product of two decoded values has at most 6 significant
    # bits, and a row's block exponents span far fewer than the 53 - 6 -
    # log2(D) bits that would make a partial sum round, so the fp64 sums
    # are exact in any order.
    assert torch.equal(qn @ xn.T, ref)
    # (a bound of exactly 0 happens: every product of the cell is 0)
    assert (bound >= 0).all() and (bound > 0).any()
    assert torch.equal(bound, (qn.abs() @ xn.abs().T) * (D * 2.0 ** -22))


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"nq{s[0]}-nx{s[1]}")
@pytest.mark.parametrize("D", DEPTHS)
def test_bound_separates_old_piece_clamp(D, shape, family):
    nq, nx = shape
    Q4, QS, X4, XS = _case(family, D, nq, nx)
    ref, bound = g.reference_fp4x4_scores(Q4, QS, X4, XS)
    old, _ = g.reference_fp4x4_scores(Q4, _old_piece_clamp(QS), X4, _old_piece_clamp(XS))
    bad = (old - ref).abs() > bound
    # the rows and columns whose scale bytes the old rule moved
    q_hit = (_old_piece_clamp(QS) != QS).any(dim=1)
    x_hit = (_old_piece_clamp(XS) != XS).any(dim=1)
    if D in EXACT_DEPTHS:
        assert not q_hit.any() and not x_hit.any()
        assert int(bad.sum()) == 0
    else:
        # At least one operand is hit, every hit row and column leaves the
        # bound as a row or column, and nothing else does. Not in literally
        # every cell: where the moved scale bytes weigh terms that cancel
        # or are zero the cell stays inside (measured 92 % to 100 % of a hit
        # row's or column's cells outside), so the line is drawn at half.
        assert q_hit.any() or x_hit.any()
        assert (bad[q_hit].float().mean(dim=1) > 0.5).all()
        assert (bad[:, x_hit].float().mean(dim=0) > 0.5).all()
        assert not bad[~q_hit][:, ~x_hit].any()
    # a right fp32 kernel stays inside: fp32 matmul of the decoded operands
    q, x = g.reference_fp4_decode(Q4, QS), g.reference_fp4_decode(X4, XS)
    f32 = (q.float() @ x.float().T).double()
    assert ((f32 - ref).abs() <= bound).all()


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("delta", [-1, 1])
@pytest.mark.parametrize("D", [128, 640, 1024])
def test_one_scale_byte_off_by_one_leaves_bound(D, delta, family):
    nq, nx = SHAPES[0]
    Q4, QS, X4, XS = _case(family, D, nq, nx)
    ref, bound = g.reference_fp4x4_scores(Q4, QS, X4, XS)
    # a live row of the ragged second query block, a byte inside the row
    row, byte = nq - 2, (D // 32) // 2
    QS2 = QS.clone()
    QS2[row, byte] = int(QS[row, byte]) + delta
    got, _ = g.reference_fp4x4_scores(Q4, QS2, X4, XS)
    bad = (got - ref).abs() > bound
    assert bool(bad[row].any())
    assert not bool(bad[torch.arange(nq) != row].any())
    # and on the X side: a column
    col = nx - 3
    XS2 = XS.clone()
    XS2[col, byte] = int(XS[col, byte]) + delta
    got, _ = g.reference_fp4x4_scores(Q4, QS, X4, XS2)
    bad = (got - ref).abs() > bound
    assert bool(bad[:, col].any())
    assert not bool(bad[:, torch.arange(nx) != col].any())
