"""Owner-filtered fp4x4 threshold scan against the unfiltered v7 scan in the
same process, bit for bit.

At the same theta the owned scan must append exactly v7's candidates that
pass the owner filter on the host (xowner[id] == qowner[q], or qowner[q] <
0): same ids, same score bits, same counts. Shapes reuse the v7 test's
reasons: two query blocks (the second with 44 live rows), two swaths, a
ragged 77-row last tile, K depths np = 1 and 8, plus a single tile.
"""

import functools

import pytest
import torch

from vainplex_openclaw_amd.ops import gpu as g

pytestmark = pytest.mark.gpu

V7 = 7
CAP = 4096
FILL_SCORE = -1e30
FILL_ID = -1
BIG = 2**31 - 1

SHAPES = [
    (300, 1613, 2, 128),
    (300, 1613, 2, 1024),
    (256, 256, 1, 1024),
]
IDS = [f"nq{nq}-nx{nx}-S{s}-D{d}" for nq, nx, s, d in SHAPES]
LAYOUTS = ["one_owner", "seven_random", "mod16", "first_last_column",
           "empty_owner", "wildcard_mix"]
THETAS = ["all", "q995", "none"]


def _sorted_lists(cs, ci, live):
    """Per-row (id, score bits) lists sorted by id; dead slots pushed to the end."""
    key = torch.where(live, ci.long(), torch.full_like(ci, BIG).long())
    key, order = key.sort(dim=1)
    sc = torch.where(live, cs, torch.zeros_like(cs)).gather(1, order)
    return key, sc.view(torch.int32)


def _live(cn, cap):
    pos = torch.arange(cap, device=cn.device).unsqueeze(0)
    return pos < cn.unsqueeze(1)


@functools.lru_cache(maxsize=None)
def _case(nq, nx, S, D):
    torch.manual_seed(11)
    Q = torch.nn.functional.normalize(torch.randn(nq, D, device="cuda"), dim=1).bfloat16()
    X = torch.nn.functional.normalize(torch.randn(nx, D, device="cuda"), dim=1).bfloat16()
    Q4, QS = g.to_fp4_mx(Q)
    X4, XS = g.to_fp4_mx(X)
    c = {"Q4": Q4, "QS": QS, "X4": X4, "XS": XS, "S": S, "nq": nq, "nx": nx}

    def v7(theta):
        out = g.ext().topk_scan_threshold_fp4x4(
            Q4, QS, X4, XS, theta.contiguous(), CAP, S, V7)
        torch.cuda.synchronize()
        return out

    lo = torch.full((nq,), -1e9, device="cuda")
    cs, ci, cn = v7(lo)
    assert (cn == nx).all()
    dense = torch.full((nq, nx), float("nan"), device="cuda")
    dense.scatter_(1, ci[:, :nx].long(), cs[:, :nx])
    thetas = {
        "all": lo,
        "q995": torch.quantile(dense, 0.995, dim=1),
        "none": torch.full((nq,), 1e9, device="cuda"),
    }
    c["theta"] = thetas
    c["v7"] = {"all": (cs, ci, cn)}
    for name in ("q995", "none"):
        c["v7"][name] = v7(thetas[name])
    assert int(c["v7"]["q995"][2].sum()) > 0
    return c


def _owners(layout, nq, nx):
    gen = torch.Generator().manual_seed(23)

    def rnd(n, hi):
        return torch.randint(0, hi, (n,), generator=gen, dtype=torch.int32)

    if layout == "one_owner":
        xo, qo = torch.zeros(nx, dtype=torch.int32), torch.zeros(nq, dtype=torch.int32)
    elif layout == "seven_random":
        xo, qo = rnd(nx, 7), rnd(nq, 7)
    elif layout == "mod16":
        # every 16-column group holds exactly one eligible column per owner
        xo, qo = (torch.arange(nx) % 16).to(torch.int32), rnd(nq, 16)
    elif layout == "first_last_column":
        xo, qo = rnd(nx, 4), rnd(nq, 4)
        xo[0] = 9
        xo[nx - 1] = 9
        qo[::5] = 9
        qo[nq - 1] = 9
    elif layout == "empty_owner":
        xo, qo = rnd(nx, 4), rnd(nq, 4)
        qo[::4] = 5
        qo[nq - 1] = 5
    elif layout == "wildcard_mix":
        xo, qo = rnd(nx, 7), rnd(nq, 7)
        qo[0:16:2] = -1          # unfiltered and filtered rows in one 16-row group
        qo[nq - 10 : nq : 3] = -1
    else:
        raise AssertionError(layout)
    return xo.cuda(), qo.cuda()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_owned_scan_equals_filtered_v7(shape, layout):
    c = _case(*shape)
    nq, nx = c["nq"], c["nx"]
    xo, qo = _owners(layout, nq, nx)
    for name in THETAS:
        theta = c["theta"][name]
        cs7, ci7, cn7 = c["v7"][name]
        live7 = _live(cn7, CAP)
        own7 = xo[ci7.long().clamp_min(0)]
        elig7 = live7 & ((qo.unsqueeze(1) < 0) | (own7 == qo.unsqueeze(1)))
        want_ids, want_sc = _sorted_lists(cs7, ci7, elig7)
        want_cn = elig7.sum(dim=1).to(torch.int32)

        cs, ci, cn = g.ext().topk_scan_threshold_fp4x4_owned(
            c["Q4"], c["QS"], c["X4"], c["XS"], theta.contiguous(), xo, qo, CAP, c["S"])
        torch.cuda.synchronize()
        assert torch.equal(cn, want_cn), (layout, name)
        live = _live(cn, CAP)
        got_ids, got_sc = _sorted_lists(cs, ci, live)
        assert torch.equal(got_ids, want_ids), (layout, name)
        assert torch.equal(got_sc, want_sc), (layout, name)

        # every returned id belongs to the query's owner
        own = xo[ci.long().clamp_min(0)]
        assert (~live | (qo.unsqueeze(1) < 0) | (own == qo.unsqueeze(1))).all()
        # slots past the count are untouched
        assert (cs[~live] == torch.tensor(FILL_SCORE, device="cuda")).all()
        assert (ci[~live] == FILL_ID).all()

        if layout == "one_owner":
            assert torch.equal(cn, cn7)
        if layout == "first_last_column" and name == "all":
            nine = qo == 9
            assert (cn[nine] == 2).all()
            assert (got_ids[nine][:, :2] == torch.tensor([0, nx - 1], device="cuda")).all()
        if layout == "empty_owner":
            empty = qo == 5
            assert int(empty.sum()) > 0
            assert (cn[empty] == 0).all()
            assert (cs[empty] == torch.tensor(FILL_SCORE, device="cuda")).all()
            assert (ci[empty] == FILL_ID).all()
        if name == "none":
            assert (cn == 0).all()
        if name == "all" and layout == "wildcard_mix":
            assert (cn[qo < 0] == nx).all()


def test_owned_binding_checks_owner_operands():
    c = _case(*SHAPES[2])
    nq, nx = c["nq"], c["nx"]
    theta = c["theta"]["none"]
    xo, qo = _owners("seven_random", nq, nx)
    args = (c["Q4"], c["QS"], c["X4"], c["XS"], theta)
    scan = g.ext().topk_scan_threshold_fp4x4_owned
    with pytest.raises(RuntimeError):
        scan(*args, xo.long(), qo, CAP, c["S"])           # dtype
    with pytest.raises(RuntimeError):
        scan(*args, xo[:-1].contiguous(), qo, CAP, c["S"])  # length
    with pytest.raises(RuntimeError):
        scan(*args, xo, qo.cpu(), CAP, c["S"])            # device
    with pytest.raises(RuntimeError):
        scan(*args, xo, torch.cat([qo, qo])[::2], CAP, c["S"])  # contiguity
