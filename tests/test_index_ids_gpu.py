"""The memory-id column in the index kernels: the append kernel writes
id_base + source row, the move kernel carries the 8-byte column with the
rows, and find_rows returns the row of every wanted id. All comparisons are
exact, on integers and bit patterns."""

import pytest
import torch

from vainplex_openclaw_amd.ops import gpu as g

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -77
HI = (1 << 62) | (9 << 48)


# -- append ---------------------------------------------------------------------

def _append_case(D, with_ids):
    gen = torch.Generator(device=DEV).manual_seed(D)
    m, cap, row0 = 70, 128, 11
    feats = torch.randn(m, D, generator=gen, device=DEV).bfloat16()
    src = torch.randperm(m, generator=gen, device=DEV)[:37].to(torch.int32)
    src[5] = m + 3  # out of range: its destination row stays as it is
    index = torch.full((cap, D), 3.0, dtype=torch.bfloat16, device=DEV)
    x4 = torch.full((cap, D // 2), 0xAB, dtype=torch.uint8, device=DEV)
    xs = torch.full((cap, D // 32), 0xCD, dtype=torch.uint8, device=DEV)
    owner = torch.full((cap,), -5, dtype=torch.int32, device=DEV)
    owner_src = torch.arange(m, dtype=torch.int32, device=DEV) % 7
    sal = torch.full((cap,), 0.25, device=DEV)
    ids = torch.full((cap,), SENTINEL, dtype=torch.int64, device=DEV)
    kw = dict(id_dst=ids, id_base=HI + 1000) if with_ids else {}
    g.index_append(feats, src, row0, index, x4, xs, owner_dst=owner, owner_src=owner_src,
                   salience_dst=sal, salience_init=1.0, **kw)
    torch.cuda.synchronize()
    return src, row0, (index.view(torch.int16), x4, xs, owner, sal), ids


@pytest.mark.parametrize("D", [128, 1024])
def test_append_writes_ids(D):
    src, row0, with_out, ids = _append_case(D, True)
    want = torch.full_like(ids, SENTINEL)
    good = torch.ones(src.numel(), dtype=torch.bool, device=DEV)
    good[5] = False
    dst = row0 + torch.arange(src.numel(), device=DEV)
    want[dst[good]] = HI + 1000 + src[good].long()
    assert torch.equal(ids, want)
    assert int(ids[row0 + 5]) == SENTINEL
    # the other outputs are what they are without an id column
    _src, _row0, without_out, untouched = _append_case(D, False)
    assert (untouched == SENTINEL).all()
    for a, b in zip(with_out, without_out):
        assert torch.equal(a, b)


# -- move -----------------------------------------------------------------------

def _move_buffers():
    gen = torch.Generator(device=DEV).manual_seed(5)
    cap, D = 300, 128
    index = torch.randn(cap, D, generator=gen, device=DEV).bfloat16()
    x4 = torch.randint(0, 256, (cap, D // 2), generator=gen, device=DEV, dtype=torch.uint8)
    xs = torch.randint(0, 256, (cap, D // 32), generator=gen, device=DEV, dtype=torch.uint8)
    owner = torch.randint(0, 64, (cap,), generator=gen, device=DEV, dtype=torch.int32)
    sal = torch.rand(cap, generator=gen, device=DEV)
    # preload and rank bits set, and both 32-bit halves differ from row to
    # row: a move that truncates to 32 bits, or moves one half, shows
    ids = HI | (torch.randperm(cap, generator=gen, device=DEV).long() << 33) \
        | torch.randperm(cap, generator=gen, device=DEV).long()
    perm = torch.randperm(cap, generator=gen, device=DEV)
    src, dst = perm[:97].to(torch.int32), perm[97:194].to(torch.int32)
    return dict(index=index, X4=x4, XS=xs, owner=owner, salience=sal, ids=ids), src, dst


def _bits(name, t):
    return t.view(torch.int16) if name == "index" else t


def test_move_carries_ids_with_all_buffers():
    bufs, src, dst = _move_buffers()
    want = {k: v.clone() for k, v in bufs.items()}
    for v in want.values():
        v[dst.long()] = v[src.long()]
    g.index_move_rows(src, dst, **bufs)
    torch.cuda.synchronize()
    for k in bufs:
        assert torch.equal(_bits(k, bufs[k]), _bits(k, want[k])), k
    assert int(bufs["ids"].min()) >= HI  # no truncation to 32 bits


def test_move_ids_alone():
    bufs, src, dst = _move_buffers()
    ids = bufs["ids"]
    before = ids.clone()
    want = before.clone()
    want[dst.long()] = want[src.long()]
    g.index_move_rows(src, dst, ids=ids)
    torch.cuda.synchronize()
    assert torch.equal(ids, want)
    rest = torch.ones(ids.numel(), dtype=torch.bool, device=DEV)
    rest[dst.long()] = False
    assert torch.equal(ids[rest], before[rest])


# -- find -----------------------------------------------------------------------

N_COL = 100_003


@pytest.fixture(scope="module")
def column():
    gen = torch.Generator(device=DEV).manual_seed(11)
    raw = torch.randint(0, 1 << 62, (N_COL + 64,), generator=gen, device=DEV, dtype=torch.int64)
    col = torch.unique(raw)
    assert col.numel() >= N_COL
    col = col[torch.randperm(col.numel(), generator=gen, device=DEV)][:N_COL].contiguous()
    return col


def _wanted(col, m, seed):
    """m wanted ids: the edge cases first, as many as fit, then present and
    absent ids at random."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    present = set(col.tolist())
    edge = [int(col[0]), int(col[-1]), int(col.min()), int(col.max()), -1,
            int(col[0]), int(col[17]), int(col[17]),
            # present ids with another high word
            int(col[5]) ^ (1 << 40), int(col[6]) ^ (1 << 61), int(col[7]) ^ (1 << 32),
            0, (1 << 62) + 5, -(1 << 40)]
    for e in edge[8:11]:
        assert e not in present
    pick = col[torch.randint(0, col.numel(), (m,), generator=gen, device=DEV)]
    absent = torch.randint(0, 1 << 62, (m,), generator=gen, device=DEV, dtype=torch.int64)
    rnd = torch.where(torch.rand(m, generator=gen, device=DEV) < 0.6, pick, absent)
    want = torch.cat([torch.tensor(edge, dtype=torch.int64, device=DEV), rnd])[:m]
    return want[torch.randperm(m, generator=gen, device=DEV)]


@pytest.mark.parametrize("m", [1, 5, 4096, 4097, 9000])
def test_find_rows_matches_reference(column, m):
    want = _wanted(column, m, seed=m)
    got = g.find_rows(column, want)
    torch.cuda.synchronize()
    ref = g.reference_find_rows(column, want)
    assert got.dtype == torch.int32 and got.shape == (m,)
    assert torch.equal(got, ref)
    if m >= 4096:
        assert int((ref >= 0).sum()) > m // 3 and int((ref < 0).sum()) > m // 4
        hit = ref >= 0
        assert torch.equal(column[ref[hit].long()], want[hit])


def test_find_rows_first_and_last_row(column):
    want = torch.stack([column[-1], column[0], column[-2], column[1]])
    assert g.find_rows(column, want).tolist() == [N_COL - 1, 0, N_COL - 2, 1]


def test_find_rows_unaligned_view(column):
    view = column[1:]
    assert view.data_ptr() % 16 == 8
    for sub in (view, view[:-1], view[:2], view[:1]):
        want = torch.cat([_wanted(column, 5000, seed=2), sub[:1], sub[-1:], column[:1]])
        got = g.find_rows(sub, want)
        assert torch.equal(got, g.reference_find_rows(sub, want))
        assert got[-3:].tolist() == [0, sub.numel() - 1, -1]


def test_find_rows_empty(column):
    none = torch.empty(0, dtype=torch.int64, device=DEV)
    got = g.find_rows(none, column[:3])
    assert got.tolist() == [-1, -1, -1] and got.dtype == torch.int32
    got = g.find_rows(column, none)
    assert got.shape == (0,) and got.dtype == torch.int32 and got.is_cuda


def test_find_rows_id_held_twice(column):
    col = column[:5001].clone()
    col[4000] = col[123]
    col[77] = col[4999]
    want = torch.stack([col[123], col[4999], col[0]])
    got = g.find_rows(col, want)
    assert got.tolist() == [4000, 4999, 0]
    assert torch.equal(got, g.reference_find_rows(col, want))
