"""Forgetting for the live recall index, the parts that need no GPU: the
eviction rule (ops.gpu.evict_mask), the hole-filling plan
(ops.gpu.forget_plan), index_forget on the torch-indexing path, and the
Membrane index and engine dropping pruned records' rows. All comparisons
are exact."""

import numpy as np
import pytest
import torch

from vainplex_openclaw_amd.membrane.engine import MembraneEngine
from vainplex_openclaw_amd.membrane.index import SalienceIndex
from vainplex_openclaw_amd.ops import gpu as g


def edge_masks(n):
    """name -> bool[n] dead masks that hit every corner of the plan (also
    used by the GPU kernel test)."""
    idx = torch.arange(n)
    masks = {
        "none": torch.zeros(n, dtype=torch.bool),
        "all": torch.ones(n, dtype=torch.bool),
        "tail": idx >= n - max(1, n // 10),
        "prefix": idx < max(1, n // 10),
        "alternating": idx % 2 == 0,
    }
    gen = torch.Generator().manual_seed(n)
    for p in (0.01, 0.3, 0.9):
        masks[f"random{p}"] = torch.rand(n, generator=gen) < p
    return masks


# -- evict_mask --------------------------------------------------------------

def _saliences(n):
    rng = np.random.default_rng(7)
    half_floor = rng.random(n).astype(np.float32)
    half_floor[rng.permutation(n)[: n // 2]] = 0.01
    return {
        "random": rng.random(n).astype(np.float32),
        "all_equal": np.full(n, 0.5, dtype=np.float32),
        "half_floor": half_floor,
        # rows ingested in one step share a value bit for bit
        "blocks": np.repeat(rng.random(n // 16 + 1).astype(np.float32), 16)[:n],
    }


@pytest.mark.parametrize("kind", ["random", "all_equal", "half_floor", "blocks"])
def test_evict_mask_matches_stable_argsort(kind):
    n = 257
    s = _saliences(n)[kind]
    order = np.lexsort((np.arange(n), s))  # by (salience, row)
    for count in (0, 1, 5, n // 2, n - 1, n, n + 3, -4):
        c = min(max(count, 0), n)
        want = np.zeros(n, dtype=bool)
        want[order[:c]] = True
        got = g.evict_mask(torch.from_numpy(s), count)
        assert got.dtype == torch.bool and got.shape == (n,)
        assert int(got.sum()) == c, (kind, count)
        assert np.array_equal(got.numpy(), want), (kind, count)


# -- forget_plan -------------------------------------------------------------

def _check_plan(dead):
    n = dead.numel()
    n_new, dst, src = g.forget_plan(dead)
    assert isinstance(n_new, int) and n_new == n - int(dead.sum())
    assert dst.dtype == torch.int32 and src.dtype == torch.int32
    assert len(dst) == len(src)
    d, s, dd = dst.numpy(), src.numpy(), dead.numpy()
    assert (d < n_new).all() and (s >= n_new).all() and (s < n).all()
    assert np.array_equal(d, np.flatnonzero(dd[:n_new]))
    assert np.array_equal(s, np.flatnonzero(~dd[n_new:]) + n_new)
    assert (np.diff(d) > 0).all() and (np.diff(s) > 0).all()
    return n_new, dst, src


@pytest.mark.parametrize("n", [1, 2, 64, 1000])
def test_forget_plan_edges_and_random(n):
    for name, dead in edge_masks(n).items():
        n_new, dst, _src = _check_plan(dead)
        if name == "none":
            assert n_new == n and len(dst) == 0
        if name == "all":
            assert n_new == 0 and len(dst) == 0
        if name == "tail":
            assert len(dst) == 0  # a pure truncation moves nothing
        if name == "prefix" and n > 1:
            assert len(dst) == min(int(dead.sum()), n_new) > 0


def test_forget_plan_single_row():
    for dead in (torch.tensor([True]), torch.tensor([False])):
        n_new, dst, src = _check_plan(dead)
        assert n_new == int(not dead[0]) and len(dst) == len(src) == 0


# -- index_forget, torch-indexing path ---------------------------------------

def _tagged(n, cap, D):
    """Buffers whose every row is a function of its row id."""
    i = torch.arange(cap)
    owner = i.to(torch.int32)
    index = (i.unsqueeze(1) * 3 + torch.arange(D).unsqueeze(0)).to(torch.float32).bfloat16()
    x4 = ((i.unsqueeze(1) * 7 + torch.arange(D // 2).unsqueeze(0)) % 256).to(torch.uint8)
    xs = ((i.unsqueeze(1) * 5 + torch.arange(D // 32).unsqueeze(0)) % 256).to(torch.uint8)
    sal = (i.float() + 0.5) / cap
    return index, x4, xs, owner, sal


@pytest.mark.parametrize("name", list(edge_masks(8)))
def test_index_forget_cpu_tagged_rows(name):
    n, cap, D = 200, 230, 128
    dead = edge_masks(n)[name]
    index, x4, xs, owner, sal = _tagged(n, cap, D)
    ref = [t.clone() for t in (index, x4, xs, owner, sal)]
    n_new = g.index_forget(dead, index=index, X4=x4, XS=xs, owner=owner, salience=sal)
    assert n_new == n - int(dead.sum())
    tags = owner[:n_new].long()
    kept = torch.nonzero(~dead).flatten()
    assert torch.equal(torch.sort(tags).values, kept)
    # every live row carries one original row in all its buffers
    for got, orig in zip((index, x4, xs, owner, sal), ref):
        a, b = got[:n_new], orig[tags]
        if a.dtype == torch.bfloat16:
            a, b = a.view(torch.int16), b.view(torch.int16)
        assert torch.equal(a, b)
    # spare capacity is not touched
    for got, orig in zip((index, x4, xs, owner, sal), ref):
        assert torch.equal(got[n:].float(), orig[n:].float())


def test_index_move_rows_cpu_subset_and_checks():
    owner = torch.arange(10, dtype=torch.int32)
    g.index_move_rows(torch.tensor([8, 9], dtype=torch.int32),
                      torch.tensor([0, 3], dtype=torch.int32), owner=owner)
    assert owner.tolist() == [8, 1, 2, 9, 4, 5, 6, 7, 8, 9]
    with pytest.raises(ValueError):
        g.index_move_rows(torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.int32))


# -- Membrane ----------------------------------------------------------------

TEXTS = [f"memo {i}: the {w} deploy ticket {i * 37} is owned by team {i % 5}"
         for i, w in enumerate(["blue", "green", "red", "amber", "violet", "grey"] * 4)]


def _filled_index(device=None):
    idx = SalienceIndex(dim=64, vocab=512, device=device, capacity=8)
    for a, agent in enumerate(("a", "b")):
        idx.add(agent, [f"{agent}{i}" for i in range(len(TEXTS))], TEXTS)
    return idx


def check_remove(device=None):
    """remove() on a two-agent index: shared by the CPU and the GPU test."""
    idx = _filled_index(device)
    before = {(ag, i): idx.search(ag, TEXTS[i], 3) for ag in "ab" for i in range(len(TEXTS))}
    gone = ["a0", "a5", "b23", "b7", "a22"]
    assert idx.remove(gone + ["nope", "a5"]) == len(gone)
    n = 2 * len(TEXTS) - len(gone)
    assert idx.size == n == len(idx.ids) == len(idx.owners)
    assert not set(gone) & set(idx.ids) and len(set(idx.ids)) == n
    assert all(rid[0] == ag for rid, ag in zip(idx.ids, idx.owners))
    for (ag, i), old in before.items():
        new = idx.search(ag, TEXTS[i], 3)
        assert not {rid for rid, _ in new} & set(gone)
        # the surviving hits keep their scores: same vectors, same query;
        # the bound is what reordering a 64-term fp32 dot product of unit
        # vectors can change (64 * 2^-24 < 1e-5)
        old_scores = dict(old)
        for rid, score in new:
            if rid in old_scores:
                assert abs(score - old_scores[rid]) <= 1e-5
        if f"{ag}{i}" not in gone:
            assert new[0][0] == f"{ag}{i}" and new[0][1] > 0.99
    # every record left is still found, under its own agent only
    for ag in "ab":
        hits = idx.search(ag, TEXTS[0], idx.size)
        assert {rid for rid, _ in hits} == {r for r in idx.ids if r[0] == ag}
    assert idx.remove(gone) == 0 and idx.remove([]) == 0 and idx.size == n
    assert idx.remove(list(idx.ids)) == n and idx.size == 0
    assert idx.search("a", TEXTS[0], 3) == []
    idx.add("a", ["again"], [TEXTS[1]])
    assert idx.search("a", TEXTS[1], 1)[0][0] == "again"


def test_salience_index_remove_cpu():
    check_remove(None)


def test_decay_pass_removes_index_rows(tmp_path):
    now = [1_000_000.0]
    e = MembraneEngine(str(tmp_path), dim=64, clock=lambda: now[0])
    for i in range(12):
        e.remember("a", TEXTS[i])
    now[0] += 400 * 24 * 3600.0  # far past any half-life: all at the floor
    fresh = [e.remember("a", TEXTS[12 + i]) for i in range(3)]
    e.flush_buffer()
    assert e.index.size == 15
    n = e.decay_pass("a")
    assert n == 12
    assert e.index.size == 15 - n == e.store.count("a")
    assert set(e.index.ids) == {r["id"] for r in fresh}
    got = e.retrieve("a", TEXTS[13], limit=2)
    assert got and got[0]["record"]["id"] == fresh[1]["id"]
    assert e.decay_pass("a") == 0 and e.index.size == 3
