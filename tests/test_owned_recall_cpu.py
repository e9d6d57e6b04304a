"""Agent-isolated recall, CPU side: SalienceIndex filters by owner BEFORE the
top-k, the fp32 masked reference, and the per-owner scan thresholds.
"""

import math

import numpy as np
import torch

from vainplex_openclaw_amd.membrane.index import SalienceIndex
from vainplex_openclaw_amd.ops import gpu as g

QUERY = "the quarterly revenue report for the northern region is due on friday"


def _shared_index(dim=128, device=None):
    """Agent A: 60 rows sharing the query's wording. Agent B: 3 unrelated."""
    idx = SalienceIndex(dim=dim, vocab=4096, device=device, capacity=16)
    a_texts = [f"{QUERY} and item {i} needs review" for i in range(60)]
    idx.add("A", [f"a{i}" for i in range(60)], a_texts)
    b_texts = [
        "zebra crossing painted yesterday near the old mill",
        "my cat prefers tuna over chicken on weekdays",
        "compile flags -O3 and loop unrolling explained",
    ]
    idx.add("B", ["b0", "b1", "b2"], b_texts)
    return idx, b_texts


def test_small_owner_gets_its_own_top_k():
    idx, b_texts = _shared_index()
    got = idx.search("B", QUERY, k=2)
    # B's rows by exact cosine, best first
    q = np.asarray(idx.encode([QUERY]))[0]
    sims = np.asarray(idx.encode(b_texts)) @ q
    order = np.argsort(-sims)[:2]
    assert [r for r, _ in got] == [f"b{i}" for i in order]
    assert np.allclose([s for _, s in got], sims[order], atol=1e-5)


def test_agent_without_rows_gets_nothing():
    idx, _ = _shared_index()
    assert idx.search("C", QUERY, k=2) == []
    assert SalienceIndex(dim=128, vocab=4096).search("A", QUERY, k=2) == []


def test_sole_owner_matches_unfiltered_top_k():
    idx = SalienceIndex(dim=128, vocab=4096, capacity=16)
    texts = [f"note {i}: {QUERY if i % 3 == 0 else 'unrelated filler words here'} {i}"
             for i in range(40)]
    idx.add("A", [f"r{i}" for i in range(40)], texts)
    got = idx.search("A", QUERY, k=5)
    # the list the unfiltered search gave: global argsort of all rows
    q = np.asarray(idx.encode([QUERY]))[0]
    sims = idx._mat_np[: idx.size] @ q
    order = np.argsort(-sims)[:5]
    assert got == [(f"r{i}", float(sims[i])) for i in order]


def test_owner_vector_grows_with_matrix():
    idx, _ = _shared_index()  # capacity 16 -> grown twice
    assert idx.capacity >= 63
    assert idx._owner_np[:60].tolist() == [0] * 60
    assert idx._owner_np[60:63].tolist() == [1] * 3


def test_reference_owned_topk_matches_brute_force():
    torch.manual_seed(3)
    nq, nx, D, k = 7, 50, 16, 4
    Q = torch.randn(nq, D)
    X = torch.randn(nx, D)
    owner = torch.randint(0, 3, (nx,), dtype=torch.int32)
    owner[[5, 31]] = 3                      # owner 3 holds 2 rows < k
    qowner = torch.tensor([0, 1, 2, 3, -1, 4, 1], dtype=torch.int32)  # 4 owns nothing
    sal = torch.rand(nx) + 0.1
    for salience in (None, sal):
        vals, ids = g.reference_owned_topk(Q, X, k, owner, qowner, salience=salience)
        assert vals.shape == (nq, k) and ids.shape == (nq, k)
        for q in range(nq):
            rows = []
            for j in range(nx):
                if qowner[q] < 0 or owner[j] == qowner[q]:
                    s = float(Q[q] @ X[j])
                    if salience is not None:
                        s *= float(salience[j])
                    rows.append((s, j))
            rows.sort(key=lambda t: -t[0])
            want = rows[:k]
            assert ids[q].tolist() == [j for _, j in want] + [-1] * (k - len(want))
            assert np.allclose(vals[q, : len(want)].tolist(), [s for s, _ in want], atol=1e-5)
            assert (vals[q, len(want):] == -1e30).all()
    # the short and the empty owner
    assert (ids[3] >= 0).sum() == 2 and (ids[5] == -1).all()


def test_reference_owned_topk_k_beyond_index():
    Q, X = torch.randn(2, 8), torch.randn(3, 8)
    owner = torch.zeros(3, dtype=torch.int32)
    vals, ids = g.reference_owned_topk(Q, X, 5, owner, torch.tensor([0, -1], dtype=torch.int32))
    assert ids.shape == (2, 5) and (ids[:, 3:] == -1).all() and (ids[:, :3] >= 0).all()


def _scalar_theta(mu, sigma, nx, target, margin):
    """The unfiltered path's formula (one p for the whole index)."""
    p = min(0.5, max(target / max(nx, 1), 1e-12))
    lo, hi = 0.0, 9.0
    for _ in range(200):
        mid = (lo + hi) / 2
        if 0.5 * math.erfc(mid / math.sqrt(2)) > p:
            lo = mid
        else:
            hi = mid
    return mu + sigma * ((lo + hi) / 2 - margin)


def test_owned_thresholds():
    mu = torch.full((6,), 0.01)
    sigma = torch.full((6,), 0.03)
    n_owned = torch.tensor([0, 10, 300, 5000, 80000, 1_000_000])
    theta = g.owned_thresholds(mu, sigma, n_owned, 128, z_margin=0.25)
    assert theta.dtype == mu.dtype and theta.shape == mu.shape
    assert math.isinf(float(theta[0])) and theta[0] > 0      # empty owner
    live = theta[1:]
    assert torch.isfinite(live).all()
    assert (live[1:] >= live[:-1]).all()                     # monotone in n_owned
    assert live[-1] > live[0]
    # n_owned <= 2 * target: p clamps at 0.5, z = 0
    assert torch.allclose(live[0], mu[0] - 0.25 * sigma[0])
    # one owner holding every row: the scalar formula
    for nx in (4096, 1_000_000, 50_000_000):
        for margin in (0.0, 0.25):
            got = g.owned_thresholds(mu, sigma, torch.full((6,), nx), 128, z_margin=margin)
            want = _scalar_theta(mu, sigma, nx, 128, margin)
            assert torch.allclose(got, want, rtol=0, atol=1e-6)
