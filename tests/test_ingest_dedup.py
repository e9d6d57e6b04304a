"""Ingest dedup, the rule: reference_batch_first_similar and
reference_recall_dup_rows on hand-made cases, the torch path of both ops
against them, and the config field. The case builders are shared with
test_ingest_dedup_gpu.py."""

import dataclasses
import math

import pytest
import torch

from vainplex_openclaw_amd.ops import gpu as g
from vainplex_openclaw_amd.pipeline.engine import PipelineConfig

TAU = 0.9
MARGIN = 1e-3  # fp32 accumulation over D <= 1024 errs by about D * 2^-24 = 6e-5


def _unit(gen, *shape):
    return torch.nn.functional.normalize(
        torch.randn(*shape, generator=gen, dtype=torch.float64), dim=-1)


def _at_cosine(gen, a, cos):
    """Unit vectors at cosine `cos` (a float, or one per row as [n, 1]) to
    the unit rows `a`; cosine 1.0 gives `a` itself, bit for bit."""
    cos = torch.as_tensor(cos, dtype=torch.float64)
    r = _unit(gen, *a.shape)
    r = torch.nn.functional.normalize(r - (r * a).sum(-1, keepdim=True) * a, dim=-1)
    return cos * a + torch.sqrt(1.0 - cos * cos) * r


def clustered_rows(B, D, seed):
    """bf16 [B, D]: 7 random unit centres, a row is normalize(centre + 0.15
    * unit noise); a third of the rows stand alone; from B = 16 on the last
    eight rows are four pairs at cosine 0.91, 0.89, 0.91, 0.89. Below B = 16
    every row comes from the first centre, so that B = 2 holds a pair."""
    gen = torch.Generator().manual_seed(seed)
    centres = _unit(gen, 7, D)
    which = torch.randint(0, 7, (B,), generator=gen)
    alone = torch.rand(B, generator=gen, dtype=torch.float64) < 1.0 / 3.0
    rows = torch.nn.functional.normalize(centres[which] + 0.15 * _unit(gen, B, D), dim=1)
    rows = torch.where(alone.unsqueeze(1), _unit(gen, B, D), rows)
    if B < 16:
        rows = torch.nn.functional.normalize(centres[:1] + 0.15 * _unit(gen, B, D), dim=1)
    else:
        a = _unit(gen, 4, D)
        b = _at_cosine(gen, a, torch.tensor([[0.91], [0.89], [0.91], [0.89]]))
        rows[B - 8:] = torch.stack([a, b], dim=1).reshape(8, D)
    return rows.bfloat16()


def batch_case(B, D, seed, owners):
    """(F, elig, owner): clustered rows, about 70 % eligible, 3 owners."""
    gen = torch.Generator().manual_seed(seed + 1000)
    F = clustered_rows(B, D, seed)
    elig = torch.rand(B, generator=gen) < 0.7
    owner = torch.randint(0, 3, (B,), generator=gen, dtype=torch.int32) if owners else None
    return F, elig, owner


def assert_batch_margin(F, elig, owner, tau=TAU):
    """No eligible same-owner pair within MARGIN of tau (fp64 on the bf16
    values); returns the number of such pairs above tau."""
    S = F.double() @ F.double().T
    pair = torch.tril(elig.unsqueeze(1) & elig.unsqueeze(0), -1)
    if owner is not None:
        pair &= owner.unsqueeze(1) == owner.unsqueeze(0)
    gap = (S[pair] - tau).abs()
    assert gap.numel() == 0 or float(gap.min()) >= MARGIN
    return int((S[pair] >= tau).sum())


def recall_case(B, k, D, seed, owners, n=400):
    """(F, ids, X, xowner, qowner) for recall_dup_rows. X: random unit rows;
    row 2t+1 is at cosine 0.97 to row 2t for t < 50. Message i is a copy of
    row 2t at cosine 1.0, 0.96 or 0.80 (below tau), t = i % 50, so a slot
    list that names 2t and 2t+1 holds two rows above tau with a clear gap.
    ids: the target and its partner when k allows, then random ids from
    [-3, n + 40) (-1 and out of range included), repeated ids, shuffled."""
    gen = torch.Generator().manual_seed(seed)
    X = _unit(gen, n, D)
    X[1:100:2] = _at_cosine(gen, X[0:100:2], 0.97)
    t = torch.arange(B) % 50
    cos = torch.tensor([1.0, 0.96, 0.80], dtype=torch.float64)[torch.arange(B) % 3]
    F = _at_cosine(gen, X[2 * t], cos.unsqueeze(1))
    ids = torch.randint(-3, n + 40, (B, k), generator=gen, dtype=torch.int32)
    ids[:, 0] = (2 * t).to(torch.int32)
    if k >= 8:
        ids[:, 1] = (2 * t + 1).to(torch.int32)
        ids[:, 2] = ids[:, 0]   # a repeated id
        ids[:, 3] = -1
        ids[:, 4] = n           # one past the last row
    # every fifth message does not recall its target at all
    ids[torch.arange(B) % 5 == 4, 0] = -1
    perm = torch.argsort(torch.rand(B, k, generator=gen), dim=1)
    ids = torch.gather(ids, 1, perm)
    xowner = qowner = None
    if owners:
        xowner = torch.randint(0, 3, (n,), generator=gen, dtype=torch.int32)
        qowner = xowner[2 * t].clone()
        # every fourth message belongs to another agent than its target
        other = torch.arange(B) % 4 == 3
        qowner[other] = (qowner[other] + 1) % 3
    return F.bfloat16(), ids, X.bfloat16(), xowner, qowner


def assert_recall_margin(F, ids, X, xowner, qowner, tau=TAU):
    """Of the rows a message may match, none has its dot within MARGIN of
    tau, and the two best dots above tau, if on different rows, are MARGIN
    apart (fp64 on the bf16 values). Returns how many messages match."""
    n = X.shape[0]
    idl = ids.long()
    ok = (idl >= 0) & (idl < n)
    safe = idl.clamp(0, n - 1)
    dots = (X.double()[safe] * F.double().unsqueeze(1)).sum(2)
    if xowner is not None:
        ok &= xowner[safe] == qowner.unsqueeze(1)
    assert float((dots[ok] - tau).abs().min()) >= MARGIN
    hits = 0
    for i in range(F.shape[0]):
        best = {}
        for d, r, o in zip(dots[i].tolist(), idl[i].tolist(), ok[i].tolist()):
            if o and d >= tau:
                best[r] = d
        top = sorted(best.values(), reverse=True)
        assert len(top) < 2 or top[0] - top[1] >= MARGIN
        hits += bool(top)
    return hits


def _plane(*degrees, D=32):
    """Unit vectors in one plane, at the given angles."""
    a = torch.tensor(degrees, dtype=torch.float64) * math.pi / 180.0
    v = torch.zeros(len(degrees), D, dtype=torch.float64)
    v[:, 0], v[:, 1] = torch.cos(a), torch.sin(a)
    return v.bfloat16()


def _all(n):
    return torch.ones(n, dtype=torch.bool)


# -- the batch rule -----------------------------------------------------------

def test_first_is_strictly_earlier():
    one = _plane(0)
    assert g.reference_batch_first_similar(one, _all(1), TAU).tolist() == [0]
    same = _plane(0, 0, 0)
    # a row is within tau of itself, and that does not count
    assert g.reference_batch_first_similar(same, _all(3), TAU).tolist() == [0, 0, 0]
    # the later copy never becomes the first of the earlier one
    far = _plane(0, 90, 0)
    assert g.reference_batch_first_similar(far, _all(3), TAU).tolist() == [0, 1, 0]


def test_ineligible_earlier_copy_is_skipped():
    F = _plane(0, 0, 0)
    elig = torch.tensor([False, True, True])
    assert g.reference_batch_first_similar(F, elig, TAU).tolist() == [-1, 1, 1]
    elig = torch.tensor([True, False, True])
    assert g.reference_batch_first_similar(F, elig, TAU).tolist() == [0, -1, 0]


def test_owners_separate():
    F = _plane(0, 0, 0, 0)
    owner = torch.tensor([0, 1, 0, 1], dtype=torch.int32)
    assert g.reference_batch_first_similar(F, _all(4), TAU, owner).tolist() == [0, 1, 0, 1]
    assert g.reference_batch_first_similar(F, _all(4), TAU).tolist() == [0, 0, 0, 0]


def test_threshold_is_inclusive_and_plain_dot():
    # rows are not re-normalised: half-length copies score 0.25
    F = (_plane(0, 0).double() * 0.5).bfloat16()
    assert g.reference_batch_first_similar(F, _all(2), 0.25).tolist() == [0, 0]
    assert g.reference_batch_first_similar(F, _all(2), 0.26).tolist() == [0, 1]


def stored_rows_are_apart(F, first, owner, tau=TAU):
    """Consequence 1: no two stored rows of one owner have a dot >= tau."""
    B = first.numel()
    stored = first == torch.arange(B, dtype=first.dtype)
    S = F.double() @ F.double().T
    pair = torch.tril(stored.unsqueeze(1) & stored.unsqueeze(0), -1)
    if owner is not None:
        pair &= owner.unsqueeze(1) == owner.unsqueeze(0)
    return not bool((S[pair] >= tau).any())


@pytest.mark.parametrize("owners", [False, True])
def test_consequence_1_stored_rows_are_apart(owners):
    F, elig, owner = batch_case(300, 128, 0, owners)
    assert assert_batch_margin(F, elig, owner) > 300
    first = g.reference_batch_first_similar(F, elig, TAU, owner)
    stored = first == torch.arange(300, dtype=torch.int32)
    assert 0 < int(stored.sum()) < int(elig.sum())
    assert not (stored & ~elig).any() and (first[~elig] == -1).all()
    assert stored_rows_are_apart(F, first, owner)


def test_consequence_2_single_link():
    # A~B, B~C, A and C apart: C is dropped for B, which is dropped for A,
    # so C is below tau to every stored row
    F = _plane(0, 20, 40)
    S = F.double() @ F.double().T
    assert S[1, 0] >= TAU and S[2, 1] >= TAU and S[2, 0] < TAU
    first = g.reference_batch_first_similar(F, _all(3), TAU)
    assert first.tolist() == [0, 0, 1]


# -- the index rule -----------------------------------------------------------

def test_recall_dup_rows_rule():
    X = _plane(0, 0, 10, 90, 0)           # rows 0, 1 and 4 are bitwise equal
    F = _plane(0, 90, 45)
    ids = torch.tensor([[4, 2, 1, -1, 7],     # tie of rows 4 and 1 -> 1; 2 is lower
                        [3, 3, 0, 5, -1],     # a repeated id, ids past the end
                        [0, 2, 3, -1, -1]],   # nothing within tau
                       dtype=torch.int32)
    row, dot = g.reference_recall_dup_rows(F, ids, X, TAU)
    assert row.tolist() == [1, 3, -1]
    assert abs(float(dot[0]) - float((F[0].double() ** 2).sum())) < 1e-12
    # owners: message 0 may only match rows of owner 1
    xo = torch.tensor([1, 0, 1, 0, 1], dtype=torch.int32)
    qo = torch.tensor([1, 1, 0], dtype=torch.int32)
    row, _ = g.reference_recall_dup_rows(F, ids, X, TAU, xo, qo)
    assert row.tolist() == [4, -1, -1]
    # the best dot wins over the lower id
    row, _ = g.reference_recall_dup_rows(_plane(10), torch.tensor([[0, 2]], dtype=torch.int32),
                                         X, TAU)
    assert row.tolist() == [2]
    # no candidates, no rows
    row, _ = g.reference_recall_dup_rows(F, ids[:, :0], X, TAU)
    assert row.tolist() == [-1, -1, -1]
    row, _ = g.reference_recall_dup_rows(F, ids, X[:0], TAU)
    assert row.tolist() == [-1, -1, -1]


# -- the torch path of the ops -----------------------------------------------

@pytest.mark.parametrize("owners", [False, True])
@pytest.mark.parametrize("B,D", [(1, 128), (2, 128), (129, 128), (300, 256)])
def test_batch_first_similar_torch_path(B, D, owners):
    F, elig, owner = batch_case(B, D, 1, owners)
    assert_batch_margin(F, elig, owner)
    got = g.batch_first_similar(F, elig, TAU, owner)
    assert got.dtype == torch.int32
    assert torch.equal(got, g.reference_batch_first_similar(F, elig, TAU, owner))


@pytest.mark.parametrize("owners", [False, True])
@pytest.mark.parametrize("B,k,D", [(1, 1, 128), (65, 8, 128), (300, 16, 256)])
def test_recall_dup_rows_torch_path(B, k, D, owners):
    F, ids, X, xo, qo = recall_case(B, k, D, 2, owners)
    hits = assert_recall_margin(F, ids, X, xo, qo)
    assert B < 10 or 0 < hits < B
    row, dot = g.recall_dup_rows(F, ids, X, TAU, xo, qo)
    want_row, want_dot = g.reference_recall_dup_rows(F, ids, X, TAU, xo, qo)
    assert row.dtype == torch.int32 and dot.dtype == torch.float32
    assert torch.equal(row, want_row)
    found = want_row >= 0
    assert ((dot[found].double() - want_dot[found]).abs() <= 1e-4).all()
    with pytest.raises(ValueError):
        g.recall_dup_rows(F, ids, X, TAU, xowner=torch.zeros(X.shape[0], dtype=torch.int32))


# -- the config field ---------------------------------------------------------

def test_config_field():
    f = {x.name: x.default for x in dataclasses.fields(PipelineConfig)}
    assert f["ingest_dedup"] == 0.0
    assert PipelineConfig().ingest_dedup == 0.0
    assert PipelineConfig(ingest=True, ingest_dedup=1.0).ingest_dedup == 1.0
    for bad in (-0.1, 1.01, 2.0, float("nan")):
        with pytest.raises(ValueError):
            PipelineConfig(ingest=True, ingest_dedup=bad)
    with pytest.raises(ValueError):
        PipelineConfig(ingest_dedup=0.95)
    with pytest.raises(ValueError):
        PipelineConfig(ingest=False, ingest_dedup=0.95)
