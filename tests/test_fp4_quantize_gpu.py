"""csrc/fp4_quantize.hip against the torch oracle ops.gpu.to_fp4_mx: the
fused quantize and the index append must be bit-for-bit what the oracle
builds, so appended rows are indistinguishable from bulk-built ones.

Shapes: one row, three rows (a partial wave), 257 x 384 (24 lanes per row,
rows straddle waves and blocks), 1000 x 1024 (one wave per row, several
blocks), 65 x 2048 (two waves per row, the widest supported row)."""

import functools
import math

import pytest
import torch

from test_fp4_spec import crafted_rows
from vainplex_openclaw_amd.ops import gpu as g

pytestmark = pytest.mark.gpu

SHAPES = [(1, 128), (3, 128), (257, 384), (1000, 1024), (65, 2048)]
KINDS = ["normal", "tiny", "huge", "crafted"]
SENTINEL = 0xA5
ROW0 = 1613


def crafted(D, n=None):
    """The crafted rows widened to D: chunk j holds the rows rolled by j, so
    every chunk position sees every row; cycled to n rows when given."""
    base = crafted_rows()
    x = torch.cat([base.roll(j, dims=0) for j in range(D // 128)], dim=1)
    if n is not None:
        x = x[torch.arange(n) % x.shape[0]]
    return x.contiguous()


@functools.lru_cache(maxsize=None)
def _input(n, D, kind):
    if kind == "crafted":
        return crafted(D, n).cuda()
    gen = torch.Generator().manual_seed(n * 7 + D)
    x = torch.randn(n, D, generator=gen)
    x = x * {"normal": 1.0, "tiny": 1e-30, "huge": 1e30}[kind]
    return x.bfloat16().cuda()


def _check(x):
    o4, o_s = g.to_fp4_mx(x)
    # the oracle itself: its GPU result is its CPU result
    c4, c_s = g.to_fp4_mx(x.cpu())
    assert torch.equal(o_s.cpu(), c_s), "oracle scales differ between GPU and CPU"
    assert torch.equal(o4.cpu(), c4), "oracle codes differ between GPU and CPU"
    k4, k_s = g.quantize_fp4_mx(x)
    torch.cuda.synchronize()
    assert k4.shape == o4.shape and k_s.shape == o_s.shape
    assert torch.equal(k_s, o_s), "scale bytes differ"
    assert torch.equal(k4, o4), "code bytes differ"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{n}x{d}" for n, d in SHAPES])
def test_quantize_matches_oracle(shape, kind):
    _check(_input(*shape, kind))


@pytest.mark.parametrize("D", [128, 384, 1024, 2048])
def test_quantize_every_crafted_row(D):
    """Zero row, single non-zero, the signed midpoints under a 6.0 max (ties),
    -0.01 next to 6.0 (negative zero), maxima 1.5 * 2^j, subnormals."""
    _check(crafted(D).cuda())


def test_quantize_into_preallocated_rows():
    x = _input(257, 384, "normal")
    x4 = torch.full((300, 192), SENTINEL, dtype=torch.uint8, device="cuda")
    xs = torch.full((300, 12), SENTINEL, dtype=torch.uint8, device="cuda")
    g.quantize_fp4_mx(x, out=(x4[:257], xs[:257]))
    o4, o_s = g.to_fp4_mx(x)
    assert torch.equal(x4[:257], o4) and torch.equal(xs[:257], o_s)
    assert (x4[257:] == SENTINEL).all() and (xs[257:] == SENTINEL).all()


def test_quantize_rejects_bad_shapes():
    with pytest.raises(RuntimeError):
        g.quantize_fp4_mx(torch.zeros(4, 192, dtype=torch.bfloat16, device="cuda"))
    with pytest.raises(RuntimeError):
        g.quantize_fp4_mx(torch.zeros(4, 4096, dtype=torch.bfloat16, device="cuda"))
    with pytest.raises(RuntimeError):
        g.quantize_fp4_mx(torch.zeros(4, 128, dtype=torch.float32, device="cuda"))


# -- index_append ------------------------------------------------------------

def _sentinel(shape, dtype):
    nbytes = math.prod(shape) * torch.empty((), dtype=dtype).element_size()
    return torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device="cuda").view(dtype).view(shape)


def _feats(D, m=50):
    x = torch.cat([crafted(D), _input(257, D, "normal").cpu()[: m]])[:m]
    return x.contiguous().cuda()


def _src_idx(n, m):
    """Non-monotone, with a repeated entry as soon as n > 1."""
    idx = (torch.arange(n) * 37 + 11) % m
    if n > 1:
        idx[n // 2] = idx[0]
    return idx.to(torch.int32).cuda()


@pytest.mark.parametrize("D", [384, 1024])
@pytest.mark.parametrize("n", [0, 1, 77])
def test_index_append_window(n, D):
    m, cap = 50, ROW0 + 77 + 9
    feats = _feats(D, m)
    owner_src = (torch.arange(m, dtype=torch.int32) * 5 + 3).cuda()
    src = _src_idx(n, m)
    bufs = {
        "index": _sentinel((cap, D), torch.bfloat16),
        "x4": _sentinel((cap, D // 2), torch.uint8),
        "xs": _sentinel((cap, D // 32), torch.uint8),
        "owner": _sentinel((cap,), torch.int32),
        "sal": _sentinel((cap,), torch.float32),
    }
    want = {k: v.clone() for k, v in bufs.items()}
    rows = feats[src.long()]
    w = slice(ROW0, ROW0 + n)
    if n:
        o4, o_s = g.to_fp4_mx(rows)
        want["index"][w] = rows
        want["x4"][w] = o4
        want["xs"][w] = o_s
        want["owner"][w] = owner_src[src.long()]
        want["sal"][w] = 0.75
    g.index_append(feats, src, ROW0, bufs["index"], bufs["x4"], bufs["xs"],
                   owner_dst=bufs["owner"], owner_src=owner_src,
                   salience_dst=bufs["sal"], salience_init=0.75)
    torch.cuda.synchronize()
    for k in bufs:
        # the window holds the oracle's rows, every other byte the sentinel
        assert torch.equal(bufs[k].view(torch.uint8), want[k].view(torch.uint8)), k


def test_index_append_without_src_idx():
    D, m, cap = 384, 50, ROW0 + 50
    feats = _feats(D, m)
    index = _sentinel((cap, D), torch.bfloat16)
    x4 = _sentinel((cap, D // 2), torch.uint8)
    xs = _sentinel((cap, D // 32), torch.uint8)
    g.index_append(feats, None, ROW0, index, x4, xs)
    o4, o_s = g.to_fp4_mx(feats)
    assert torch.equal(index[ROW0:].view(torch.int16), feats.view(torch.int16))
    assert torch.equal(x4[ROW0:], o4) and torch.equal(xs[ROW0:], o_s)
    assert (x4[:ROW0] == SENTINEL).all() and (xs[:ROW0] == SENTINEL).all()
    assert (index[:ROW0].view(torch.uint8) == SENTINEL).all()


@pytest.mark.parametrize("drop", ["fp4", "owner", "salience", "all"])
def test_index_append_optional_destinations(drop):
    D, m, n, cap = 384, 50, 77, ROW0 + 77
    feats = _feats(D, m)
    owner_src = torch.arange(m, dtype=torch.int32, device="cuda")
    src = _src_idx(n, m)
    index = _sentinel((cap, D), torch.bfloat16)
    x4 = _sentinel((cap, D // 2), torch.uint8)
    xs = _sentinel((cap, D // 32), torch.uint8)
    owner = _sentinel((cap,), torch.int32)
    sal = _sentinel((cap,), torch.float32)
    fp4_on = drop not in ("fp4", "all")
    own_on = drop not in ("owner", "all")
    sal_on = drop not in ("salience", "all")
    g.index_append(
        feats, src, ROW0, index,
        x4 if fp4_on else None, xs if fp4_on else None,
        owner_dst=owner if own_on else None, owner_src=owner_src if own_on else None,
        salience_dst=sal if sal_on else None, salience_init=1.0)
    torch.cuda.synchronize()
    rows = feats[src.long()]
    w = slice(ROW0, ROW0 + n)
    assert torch.equal(index[w].view(torch.int16), rows.view(torch.int16))
    o4, o_s = g.to_fp4_mx(rows)
    if fp4_on:
        assert torch.equal(x4[w], o4) and torch.equal(xs[w], o_s)
    else:
        assert (x4 == SENTINEL).all() and (xs == SENTINEL).all()
    if own_on:
        assert torch.equal(owner[w], owner_src[src.long()])
    else:
        assert (owner.view(torch.uint8) == SENTINEL).all()
    if sal_on:
        assert (sal[w] == 1.0).all()
    else:
        assert (sal.view(torch.uint8) == SENTINEL).all()


def test_index_append_rejects_window_past_capacity():
    D, m, cap = 128, 8, 100
    feats = torch.zeros(m, D, dtype=torch.bfloat16, device="cuda")
    index = _sentinel((cap, D), torch.bfloat16)
    with pytest.raises(RuntimeError):
        g.index_append(feats, None, cap - m + 1, index)
    with pytest.raises(RuntimeError):
        g.index_append(feats, _src_idx(9, m), cap - 8, index)
    with pytest.raises(RuntimeError):
        g.index_append(feats, None, -1, index)
    with pytest.raises(RuntimeError):  # destination of another width
        g.index_append(feats, None, 0, _sentinel((cap, 256), torch.bfloat16))
    with pytest.raises(RuntimeError):  # owner destination without a source
        g.index_append(feats, None, 0, index, owner_dst=_sentinel((cap,), torch.int32))
    torch.cuda.synchronize()
    assert (index.view(torch.uint8) == SENTINEL).all()
    g.index_append(feats, None, cap - m, index)  # the last window that fits
    torch.cuda.synchronize()
    assert (index[cap - m:].view(torch.int16) == 0).all()


# -- a grown index scans like a rebuilt one ------------------------------------

def _id_score_sets(cs, ci, cn, nx):
    assert (cn == nx).all(), "the scan must keep every column"
    ids, order = ci[:, :nx].long().sort(dim=1)
    assert (ids == torch.arange(nx, device=ids.device)).all()
    return cs[:, :nx].gather(1, order).view(torch.int32)


@pytest.mark.parametrize("D", [128, 1024])
def test_grown_index_scans_like_rebuilt(D):
    n0, add, nq, cap_rows = ROW0, 300, 300, ROW0 + 300 + 40
    gen = torch.Generator().manual_seed(D + 1)
    X = torch.nn.functional.normalize(torch.randn(n0 + add, D, generator=gen), dim=1)
    X = X.bfloat16().cuda()
    Q = torch.nn.functional.normalize(torch.randn(nq, D, generator=gen), dim=1)
    Q4, QS = g.to_fp4_mx(Q.bfloat16().cuda())

    index = torch.zeros(cap_rows, D, dtype=torch.bfloat16, device="cuda")
    x4 = torch.zeros(cap_rows, D // 2, dtype=torch.uint8, device="cuda")
    xs = torch.zeros(cap_rows, D // 32, dtype=torch.uint8, device="cuda")
    index[:n0] = X[:n0]
    b4, bs = g.to_fp4_mx(X[:n0])
    x4[:n0], xs[:n0] = b4, bs
    g.index_append(X[n0:].contiguous(), None, n0, index, x4, xs)

    nx = n0 + add
    r4, rs = g.to_fp4_mx(X)
    theta = torch.full((nq,), -1e9, device="cuda")
    grown = g.ext().topk_scan_threshold_fp4x4(Q4, QS, x4[:nx], xs[:nx], theta, 4096, 0)
    rebuilt = g.ext().topk_scan_threshold_fp4x4(Q4, QS, r4, rs, theta, 4096, 0)
    torch.cuda.synchronize()
    assert torch.equal(_id_score_sets(*grown, nx), _id_score_sets(*rebuilt, nx))
    assert torch.equal(index[:nx].view(torch.int16), X.view(torch.int16))
