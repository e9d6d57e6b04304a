"""Owner-filtered fp4x4 threshold scan on the v10 K-loop (transposed scale
sheets, op_sel, counted waits, group-aware fragment swizzle) against the
unfiltered v1 dense score matrix, masked on the host.

Expected candidates of query q: every column c with
    score[q, c] > theta[q]  and  (qowner[q] < 0 or xowner[c] == qowner[q]).
Counts and the id-sorted id and score lists must match bit for bit: the
owned kernel shares its K-loop with the unfiltered v10 scan, which
reproduces v1.

Shapes (300, 1613, 2, D), D = 128, 512, 1024 (np = 1, 4, 8): two query
blocks, the second with 44 live rows, two swaths, a ragged 77-row last
tile. Owners are drawn with 1, 3 and 64 distinct ids. Unfiltered queries
(-1, and one -7: any negative id is unfiltered) sit in rows 0..127 and at
row 290 only, so the wave that owns rows 128..255 has no unfiltered query
and runs the second, owner-aware gate, while the others skip it.
"""

import functools

import pytest
import torch

from vainplex_openclaw_amd.ops import gpu as g

from test_scan_fp4_v10 import CAP, FAMILIES, _case, _id, _sorted_lists

pytestmark = pytest.mark.gpu

SHAPES = [(300, 1613, 2, 128), (300, 1613, 2, 512), (300, 1613, 2, 1024)]
N_OWNERS = [1, 3, 64]
CASES = [(f, s, n) for f in FAMILIES for s in SHAPES for n in N_OWNERS]
SENTINEL = 2**31 - 1


@functools.lru_cache(maxsize=None)
def _owners(n_owners, nq, nx):
    gen = torch.Generator().manual_seed(100 + n_owners)
    xo = torch.randint(0, n_owners, (nx,), generator=gen, dtype=torch.int32)
    qo = torch.randint(0, n_owners, (nq,), generator=gen, dtype=torch.int32)
    rows = torch.arange(nq)
    qo[((rows % 5 == 0) & (rows < 128)) | (rows == 290)] = -1
    qo[35] = -7
    return xo.cuda(), qo.cuda()


@pytest.mark.parametrize(
    "family,shape,n_owners", CASES,
    ids=[f"{f}-{_id(s)}-owners{n}" for f, s, n in CASES])
def test_owned_matches_masked_v1(family, shape, n_owners):
    c = _case(family, *shape)
    nq, nx = c["nq"], c["nx"]
    xo, qo = _owners(n_owners, nq, nx)
    dense = c["dense_v1"]
    theta = torch.quantile(dense, 0.99, dim=1)
    eligible = (qo < 0).unsqueeze(1) | (xo.unsqueeze(0) == qo.unsqueeze(1))
    mask = (dense > theta.unsqueeze(1)) & eligible
    want_n = mask.sum(dim=1)
    assert int(want_n.sum()) > 0 and int(want_n.max()) <= CAP
    # the filter must bite: some scores above theta are foreign
    if n_owners > 1:
        assert int(((dense > theta.unsqueeze(1)) & ~eligible).sum()) > 0

    cs, ci, cn = g.ext().topk_scan_threshold_fp4x4_owned(
        c["Q4"], c["QS"], c["X4"], c["XS"], theta.contiguous(), xo, qo, CAP, c["S"])
    torch.cuda.synchronize()
    assert torch.equal(cn.long(), want_n)

    cols = torch.arange(nx, device="cuda").unsqueeze(0).expand(nq, nx)
    want_ids, order = torch.where(mask, cols, torch.full_like(cols, SENTINEL)).sort(dim=1)
    want_sc = torch.where(mask, dense, torch.zeros_like(dense)).gather(1, order)
    got_ids, got_sc = _sorted_lists(cs, ci, cn)
    assert torch.equal(got_ids[:, :nx], want_ids)
    assert (got_ids[:, nx:] == SENTINEL).all()
    assert torch.equal(got_sc[:, :nx], want_sc.view(torch.int32))
