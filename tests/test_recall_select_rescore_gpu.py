"""select_rescore (csrc/recall_epilogue.hip): the threshold recall epilogue
in one launch, against reference_select_rescore (the torch steps it
replaces) and fp64 dots of the same bf16 rows. The candidate buffers are
built here; no scan runs.

Score bound, a priori and for any summation order: bf16 x bf16 products are
exact in fp32, so an fp32 sum of D of them is within (D - 1) 2^-24 sum|q_i
x_i| of the exact dot; the salience multiply adds one rounding, 2^-24
|score|."""

import numpy as np
import pytest
import torch

from vainplex_openclaw_amd.ops import gpu as g

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NX = 300
NQ = 12
NEG = np.float32(-1e30)
U = 2.0 ** -24
# chosen on the CPU, with the reference alone: at least 90 % of the queries of
# every case below have a settled order (asserted in the test)
SEED = 2000


def _counts(cap, sel, k):
    c = [0, 1, k - 1, k, sel - 1, sel, sel + 1, cap, cap + 50, cap // 2, 2, min(cap, sel + 7)]
    assert len(c) == NQ
    return torch.tensor(c, dtype=torch.int32)


def _unit(n, D, gen):
    """Unit rows with most of their energy in the first four dimensions: the
    scores then spread over about +-1 instead of +-1/sqrt(D), while the bound
    (which grows with D sum|q_i x_i|) stays put, so that at D = 1024 too most
    neighbouring scores lie further apart than the bound."""
    v = torch.randn(n, D, generator=gen)
    v[:, :4] *= 32.0
    return torch.nn.functional.normalize(v, dim=1).bfloat16()


def _case(cap, sel, k, D, with_sal, seed):
    """CPU tensors (cs, ci, counts, Q, X, salience). Of a query's filled
    slots the first min(n, NX) hold distinct rows with scan score = exact dot
    + noise; a buffer longer than the index repeats rows at scan scores too
    low to be selected (sel < NX). Slot order is shuffled."""
    gen = torch.Generator().manual_seed(seed)
    Q = _unit(NQ, D, gen)
    X = _unit(NX, D, gen)
    sal = (torch.rand(NX, generator=gen) * 0.9 + 0.1) if with_sal else None
    counts = _counts(cap, sel, k)
    cs = torch.full((NQ, cap), -1e30, dtype=torch.float32)
    ci = torch.full((NQ, cap), -1, dtype=torch.int32)
    dots = Q.float() @ X.float().T
    for q in range(NQ):
        n = min(int(counts[q]), cap)
        if n == 0:
            continue
        ids = torch.randperm(NX, generator=gen)[:n]
        s = dots[q, ids] + 0.02 * torch.randn(ids.numel(), generator=gen)
        if n > NX:
            extra = torch.randint(0, NX, (n - NX,), generator=gen)
            ids = torch.cat([ids, extra])
            s = torch.cat([s, -5.0 - torch.rand(n - NX, generator=gen)])
        order = torch.randperm(n, generator=gen)
        cs[q, :n] = s[order]
        ci[q, :n] = ids[order].to(torch.int32)
    return cs, ci, counts, Q, X, sal


def _exact_and_bound(Q, X, sal, ids):
    """fp64 weighted dots of the rows `ids` [nq, j] (id -1: nan) and the
    a-priori bound on an fp32 evaluation of each."""
    q = Q.float().numpy().astype(np.float64)
    x = X.float().numpy().astype(np.float64)
    gid = np.clip(ids, 0, None)
    prod = q[:, None, :] * x[gid]  # [nq, j, D]
    exact = prod.sum(axis=2)
    bound = (Q.shape[1] - 1) * U * np.abs(prod).sum(axis=2)
    if sal is not None:
        exact = exact * sal.numpy().astype(np.float64)[gid]
        bound = bound + U * np.abs(exact)
    exact[ids < 0] = np.nan
    return exact, bound


def _comparable(Q, X, sal, ref_s, ref_i, k):
    """Queries whose reference order is settled: every two neighbours among
    the reference's top k + 1 valid entries lie more than twice the bound
    apart (ref_* hold k + 1 columns where sel allows)."""
    _, bound = _exact_and_bound(Q, X, sal, ref_i)
    ok = np.ones(ref_s.shape[0], dtype=bool)
    for q in range(ref_s.shape[0]):
        v = ref_i[q] >= 0
        s, b = ref_s[q][v].astype(np.float64), bound[q][v]
        gaps = s[:-1] - s[1:]
        ok[q] = bool((gaps > 2.0 * np.maximum(b[:-1], b[1:])).all())
    return ok


def _gpu(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


SHAPES = [(64, 32), (1024, 32), (1024, 128)]  # (cap, sel): sel <= cap


@pytest.mark.parametrize("with_sal", [False, True])
@pytest.mark.parametrize("D", [8, 128, 1024])
@pytest.mark.parametrize("k", [1, 16])
@pytest.mark.parametrize("cap,sel", SHAPES)
def test_select_rescore_matches_reference(cap, sel, k, D, with_sal):
    cs, ci, counts, Q, X, sal = _case(cap, sel, k, D, with_sal, seed=SEED + cap + sel + k + D)
    # the reference alone, on the CPU, one column wider to see the gap behind
    # the k-th entry; the seed must leave at least 90 % of the queries settled
    kk = min(k + 1, sel)
    ref_s, ref_i = g.reference_select_rescore(cs, ci, counts, Q, X, sal, sel, kk)
    ref_s, ref_i = ref_s.numpy(), ref_i.numpy()
    settled = _comparable(Q, X, sal, ref_s, ref_i, k)
    share = settled.mean()
    print(f"cap={cap} sel={sel} k={k} D={D} sal={with_sal}: "
          f"{int(settled.sum())}/{NQ} queries compared ({100 * share:.0f} %)")
    assert share >= 0.9

    got_s, got_i = g.select_rescore(*_gpu(cs, ci, counts, Q, X, sal), sel, k)
    again_s, again_i = g.select_rescore(*_gpu(cs, ci, counts, Q, X, sal), sel, k)
    assert got_s.dtype == torch.float32 and got_i.dtype == torch.int32
    assert got_s.shape == (NQ, k) and got_i.shape == (NQ, k) and got_s.is_cuda
    assert torch.equal(got_s, again_s) and torch.equal(got_i, again_i)
    got_s, got_i = got_s.cpu().numpy(), got_i.cpu().numpy()

    # (d) padding past the valid candidates, valid ids before it
    for q in range(NQ):
        nv = min(int(counts[q]), cap, sel, k)
        assert (got_i[q, :nv] >= 0).all() and (got_i[q, :nv] < NX).all()
        assert (got_i[q, nv:] == -1).all() and (got_s[q, nv:] == NEG).all()
        # returned ids are candidates of this query
        assert np.isin(got_i[q, :nv], ci[q].numpy()).all()

    # (a) scores against the fp64 dots of the same bf16 rows
    exact, bound = _exact_and_bound(Q, X, sal, got_i)
    v = got_i >= 0
    err = np.abs(got_s.astype(np.float64) - exact)
    if v.any():
        print(f"  max score err {err[v].max():.3e}, max err/bound {np.max(err[v] / bound[v]):.3f}")
    assert (err[v] <= bound[v]).all()
    # sorted descending
    assert (got_s[:, :-1] >= got_s[:, 1:]).all()

    # (b) ids equal the reference's where its order is settled
    assert np.array_equal(got_i[settled], ref_i[settled][:, :k])


def test_unsupported_width_takes_reference_path():
    cap, sel, k, D = 64, 32, 16, 12  # D % 8 != 0
    cs, ci, counts, Q, X, sal = _case(cap, sel, k, D, True, seed=5)
    want_s, want_i = g.reference_select_rescore(cs, ci, counts, Q, X, sal, sel, k)
    got_s, got_i = g.select_rescore(*_gpu(cs, ci, counts, Q, X, sal), sel, k)
    assert got_s.is_cuda and got_i.dtype == torch.int32
    exact, bound = _exact_and_bound(Q, X, sal, got_i.cpu().numpy())
    v = got_i.cpu().numpy() >= 0
    assert (np.abs(got_s.cpu().numpy().astype(np.float64) - exact)[v] <= bound[v]).all()
    settled = _comparable(Q, X, sal, *[t.numpy() for t in g.reference_select_rescore(
        cs, ci, counts, Q, X, sal, sel, k + 1)], k)
    assert settled.mean() >= 0.9
    assert np.array_equal(got_i.cpu().numpy()[settled], want_i.numpy()[settled])


@pytest.mark.parametrize("with_sal", [False, True])
def test_ties_go_to_the_lower_row_id(with_sal):
    """Q = e0, so a row's exact score is its first element, chosen here
    (bf16-exact values). Equal rows and equal scan scores: the lower id wins
    at the sel boundary, in the final order and at the k boundary, also
    where the higher id sits in the earlier slot."""
    cap, sel, k, D = 64, 32, 16, 128
    Q = torch.zeros(1, D)
    Q[0, 0] = 1.0
    X = torch.zeros(NX, D)
    X[:, 0] = 0.25
    ids = list(range(100, 140))           # 40 candidates
    scan = {i: 10.0 - 0.1 * (i - 100) for i in range(100, 131)}  # 31 clear winners
    scan[131] = scan[132] = 5.0           # tie for the last selected place
    for i in range(133, 140):
        scan[i] = 1.0 - 0.01 * i
    X[131, 0] = X[132, 0] = 2.0           # either would come out on top
    X[105, 0] = X[110, 0] = 1.5           # tie inside the top k
    mid = [101, 102, 103, 104, 106, 107, 108, 109, 111, 112, 113, 114]
    for j, i in enumerate(mid):
        X[i, 0] = 1.0 + (12 - j) / 32.0   # 1.375 down to 1.03125, distinct
    X[120, 0] = X[125, 0] = 0.75          # tie for the k-th place
    want = [131, 105, 110] + mid + [120]
    assert len(want) == k

    order = sorted(ids, reverse=True)     # higher ids in the earlier slots
    cs = torch.full((1, cap), -1e30)
    ci = torch.full((1, cap), -1, dtype=torch.int32)
    cs[0, :40] = torch.tensor([scan[i] for i in order])
    ci[0, :40] = torch.tensor(order, dtype=torch.int32)
    counts = torch.tensor([40], dtype=torch.int32)
    sal = torch.ones(NX) if with_sal else None
    got_s, got_i = g.select_rescore(
        *_gpu(cs, ci, counts, Q.bfloat16(), X.bfloat16(), sal), sel, k)
    assert got_i[0].tolist() == want
    assert got_s[0].tolist() == [float(X[i, 0]) for i in want]


def test_threshold_recall_with_salience_through_the_new_path():
    # as test_salience_weighted_recall_matches_dense: exact weighted scores of
    # the returned ids, near-zero regret against the dense weighted top-k, and
    # a ranking that differs from the unweighted one
    torch.manual_seed(5)
    nq, nx, d, k = 64, 8192, 256, 8
    Q = torch.nn.functional.normalize(torch.randn(nq, d, device=DEV), dim=1).bfloat16()
    X = torch.nn.functional.normalize(torch.randn(nx, d, device=DEV), dim=1).bfloat16()
    sal = torch.rand(nx, device=DEV) * 0.9 + 0.1
    got_s, got_i = g.topk_recall_threshold(Q, X, k, salience=sal)
    assert (got_i >= 0).all()
    exact, bound = _exact_and_bound(Q.cpu(), X.cpu(), sal.cpu(), got_i.cpu().numpy())
    err = np.abs(got_s.cpu().numpy().astype(np.float64) - exact)
    print(f"max score err {err.max():.3e}, max err/bound {np.max(err / bound):.3f}")
    assert (err <= bound).all()
    dense = torch.matmul(Q.float(), X.float().T)
    ref_w = torch.topk(dense * sal.unsqueeze(0), k, dim=1).values
    regret = 1.0 - got_s.sum(dim=1) / ref_w.sum(dim=1).clamp_min(1e-6)
    assert regret.max().item() < 0.05, regret.max().item()
    raw_s, raw_i = g.topk_recall_threshold(Q, X, k)
    assert not torch.equal(raw_i, got_i)
