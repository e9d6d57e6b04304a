"""topk_recall_threshold(overflow="rescan") on clustered content, against the
fp32 dense top-k.

D = 512, k = 16, cap = 256, target_candidates = 32. X holds 4096 Gaussian
unit rows and 8 clusters of 600 rows; cluster row j is cos(phi_j) c +
sin(phi_j) u_j with u_j a unit vector orthogonal to the centroid c. The
cosines fall from 0.97 in steps of 0.002 for the first 32 rows and in steps
of 0.0007 after that (0.51 at row 599). Q is 300 rows: every third one a
Gaussian unit query, the others the 8 centroids in turn. A centroid query
has 573..593 rows above its Gaussian-tail threshold (~0.51), more than twice
the buffer, so it overflows, and the plan places 250..256 of them.

What the rescan has to deliver is the true top-16 inside the `sel` = 128
candidates that are exact-rescored, ranked by fp4 score. Checked on the CPU
with to_fp4_mx codes dequantised in torch (all 200 centroid queries,
unfiltered): the worst fp4 rank of a true top-16 row is 21 (of 128 allowed),
28 for the salience-weighted top-16; the lowest fp4 score of a true top-16
row is 0.9010 against 0.8361 for the best row outside the true top-128, a
margin of 0.080 (fp4 score noise is ~0.009). Under the owner filter a query
sees a subset of its cluster, so the gaps only grow.

The Gaussian queries are drawn orthogonal to the 8 centroids. A plain
Gaussian query has a common offset q.c on each cluster's 600 rows, which
inflates its sigma estimate: on the CPU some then keep as few as 14 hits
and underflow into the direct kernel, rescan or not. Orthogonal ones keep
71..108 hits, so direct_fallback == 0 is a statement about the overflow
path. Their 16th score still sits at the threshold (worst margin 0.007
sigma on the CPU, fp4 noise 0.2 sigma): whether the fp4 scan finds the exact
top-16 of a Gaussian query is the threshold estimate's business and the
same in both modes. So the dense fp32 top-k is asserted on the centroid
queries, and the Gaussian queries are asserted equal to overflow="direct",
bit for bit.

Owners: 3, drawn 60 / 20 / 20 % over the rows, so a query of owner 0 sees
~360 rows of its cluster (overflows) and one of owner 1 or 2 ~120 (fits);
every 11th query is unfiltered (-1). Salience is 0.95 + 0.05 * rand: enough
to reorder neighbours 0.002 apart, and the weighted top-16 stays inside the
true cosine top-128 (0.94 * 0.95 > 0.84).

Without the feature every test here fails with a TypeError on the `overflow`
keyword.
"""

import functools

import pytest
import torch

from vainplex_openclaw_amd.ops import gpu as g

pytestmark = pytest.mark.gpu

D, K, CAP, TARGET = 512, 16, 256, 32
N_GAUSS, N_CLUSTERS, PER_CLUSTER, NQ = 4096, 8, 600, 300
KW = dict(cap=CAP, target_candidates=TARGET)


def cluster_cosines():
    j = torch.arange(PER_CLUSTER, dtype=torch.float64)
    head = 0.97 - 0.002 * j
    tail = (0.97 - 0.002 * 31) - 0.0007 * (j - 31)
    return torch.where(j < 32, head, tail)


def build(device):
    """(Q bf16 [NQ, D], X bf16 [nx, D], is_cluster_query bool [NQ])."""
    gen = torch.Generator().manual_seed(2024)
    unit = lambda t: torch.nn.functional.normalize(t, dim=1)  # noqa: E731
    cent = unit(torch.randn(N_CLUSTERS, D, generator=gen, dtype=torch.float64))
    cos = cluster_cosines().unsqueeze(1)
    sin = (1.0 - cos * cos).sqrt()
    rows = [unit(torch.randn(N_GAUSS, D, generator=gen, dtype=torch.float64))]
    for c in cent:
        u = torch.randn(PER_CLUSTER, D, generator=gen, dtype=torch.float64)
        u = unit(u - (u @ c).unsqueeze(1) * c.unsqueeze(0))
        rows.append(cos * c.unsqueeze(0) + sin * u)
    X = torch.cat(rows)
    X = X[torch.randperm(X.shape[0], generator=gen)]
    # Gaussian queries, drawn orthogonal to the centroids (see the docstring)
    qg = torch.randn(NQ, D, generator=gen, dtype=torch.float64)
    basis = torch.linalg.qr(cent.T).Q  # [D, 8] orthonormal span of the centroids
    qg = unit(qg - (qg @ basis) @ basis.T)
    i = torch.arange(NQ)
    is_cluster = i % 3 != 2
    Q = torch.where(is_cluster.unsqueeze(1), cent[i % N_CLUSTERS], qg)
    return (Q.float().bfloat16().to(device).contiguous(),
            X.float().bfloat16().to(device).contiguous(), is_cluster.to(device))


@functools.lru_cache(maxsize=None)
def _data():
    Q, X, is_cluster = build("cuda")
    X4 = g.quantize_fp4_mx(X)
    gen = torch.Generator().manual_seed(7)
    nx = X.shape[0]
    sal = (0.95 + 0.05 * torch.rand(nx, generator=gen)).cuda()
    xo = torch.multinomial(torch.tensor([0.6, 0.2, 0.2]), nx, replacement=True,
                           generator=gen).to(torch.int32).cuda()
    qo = torch.randint(0, 3, (NQ,), generator=gen, dtype=torch.int32)
    qo[::11] = -1
    return {"Q": Q, "X": X, "X4": X4, "is_cluster": is_cluster, "sal": sal,
            "xo": xo, "qo": qo.cuda(), "dense": Q.float() @ X.float().T}


def _recall(d, overflow, **kw):
    stats = {}
    s, i = g.topk_recall_threshold(d["Q"], d["X"], K, X4=d["X4"], overflow=overflow,
                                   stats=stats, **KW, **kw)
    torch.cuda.synchronize()
    return s, i, stats


def test_rescan_matches_dense_topk():
    d = _data()
    s, i, stats = _recall(d, "rescan")
    want = torch.topk(d["dense"], K, dim=1)
    cq = d["is_cluster"]
    assert torch.equal(i[cq].long(), want.indices[cq])
    assert torch.allclose(s[cq], want.values[cq], rtol=0, atol=1e-5)
    n_cluster = int(cq.sum())
    assert stats["overflowed"] == n_cluster
    assert stats["rescanned"] == n_cluster
    assert stats["direct_fallback"] == 0


def test_rescan_matches_dense_topk_with_salience():
    d = _data()
    s, i, stats = _recall(d, "rescan", salience=d["sal"])
    weighted = d["dense"] * d["sal"].unsqueeze(0)
    want = torch.topk(weighted, K, dim=1)
    # the weights reorder the cluster heads
    plain = torch.topk(d["dense"], K, dim=1).indices
    cq = d["is_cluster"]
    assert not torch.equal(want.indices[cq], plain[cq])
    assert torch.equal(i[cq].long(), want.indices[cq])
    assert torch.allclose(s[cq], want.values[cq], rtol=0, atol=1e-5)
    assert stats["rescanned"] > 0 and stats["direct_fallback"] == 0


def test_rescan_matches_dense_topk_with_owners():
    d = _data()
    s, i, stats = _recall(d, "rescan", owner=d["xo"], qowner=d["qo"])
    want_s, want_i = g.reference_owned_topk(d["Q"], d["X"], K, d["xo"], d["qo"])
    cq = d["is_cluster"]
    assert torch.equal(i[cq].long(), want_i[cq].long())
    assert torch.allclose(s[cq], want_s[cq], rtol=0, atol=1e-5)
    # owner 0 and the unfiltered cluster queries overflow, owners 1, 2 fit
    assert 0 < stats["rescanned"] < int(d["is_cluster"].sum())
    assert stats["rescanned"] == stats["overflowed"]
    assert stats["direct_fallback"] == 0


def test_gaussian_queries_match_direct_mode():
    d = _data()
    s_r, i_r, st_r = _recall(d, "rescan")
    s_d, i_d, st_d = _recall(d, "direct")
    gq = ~d["is_cluster"]
    assert torch.equal(i_r[gq], i_d[gq])
    assert torch.equal(s_r[gq], s_d[gq])
    # direct mode sends every overflowed query to the direct kernel
    assert st_d["overflowed"] == st_r["overflowed"] > 0
    assert st_d["rescanned"] == 0
    assert st_d["direct_fallback"] == st_d["overflowed"]
    # and both modes agree on the centroid queries
    assert torch.equal(i_r, i_d)


def test_duplicate_cluster_falls_back_to_direct():
    d = _data()
    # one query whose top CAP + 44 rows are exact duplicates: no bin edge
    # separates them, nothing above them, so no threshold fits
    gen = torch.Generator().manual_seed(3)
    c = torch.nn.functional.normalize(torch.randn(1, D, generator=gen), dim=1)
    dup = c.bfloat16().cuda()
    X = torch.cat([d["X"], dup.expand(CAP + 44, D)]).contiguous()
    Q = torch.cat([d["Q"][:40], dup]).contiguous()
    X4 = g.quantize_fp4_mx(X)
    stats = {}
    s, i = g.topk_recall_threshold(Q, X, K, X4=X4, overflow="rescan", stats=stats, **KW)
    torch.cuda.synchronize()
    want = torch.topk(Q.float() @ X.float().T, K, dim=1)
    assert stats["direct_fallback"] == 1
    assert stats["overflowed"] == stats["rescanned"] + 1
    cq = torch.cat([d["is_cluster"][:40], torch.ones(1, dtype=torch.bool, device="cuda")])
    assert torch.allclose(s[cq], want.values[cq], rtol=0, atol=1e-5)
    # the duplicate query returns K of the duplicate rows (any K of them)
    assert (i[-1].long() >= d["X"].shape[0]).all()
    assert torch.equal(i[:-1][cq[:-1]].long(), want.indices[:-1][cq[:-1]])


def test_rescan_needs_the_fp4x4_scan():
    d = _data()
    with pytest.raises(NotImplementedError):
        g.topk_recall_threshold(d["Q"], d["X"], K, overflow="rescan", **KW)
    with pytest.raises(NotImplementedError):
        g.topk_recall_threshold(d["Q"], d["X"], K, X4=d["X4"], q4=False,
                                overflow="rescan", **KW)
    with pytest.raises(ValueError):
        g.topk_recall_threshold(d["Q"], d["X"], K, X4=d["X4"], overflow="never", **KW)
