"""Stable memory ids, the parts that run without a GPU: the id layout, the
torch rule of find_rows, the id column through the CPU paths of the row
movers, the payload of the multi-rank candidate merge and the two result
fields of FirewallService."""

import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from vainplex_openclaw_amd.ops import gpu as g
from vainplex_openclaw_amd.parallel.collectives import globalize_ids, merge_topk_candidates
from vainplex_openclaw_amd.pipeline.engine import (
    PipelineConfig,
    make_memory_id,
    split_memory_id,
)
from vainplex_openclaw_amd.pipeline.service import FirewallService

WORLD = 2


# -- id layout ----------------------------------------------------------------

def test_memory_id_round_trip():
    top_seq = (1 << 48) - 1
    for pre in (False, True):
        for rank in (0, 1, 7, 16383):
            for seq in (0, 1, 12345, 1 << 32, top_seq):
                mid = make_memory_id(rank, seq, preloaded=pre)
                assert 0 <= mid < (1 << 63)
                assert split_memory_id(mid) == (pre, rank, seq)
    assert make_memory_id(0, 5) == 5
    assert make_memory_id(3, 5) == (3 << 48) | 5
    assert make_memory_id(3, 5, preloaded=True) == (1 << 62) | (3 << 48) | 5
    assert make_memory_id(16383, top_seq, preloaded=True) == (1 << 63) - 1


def test_memory_id_overflow_raises():
    for rank, seq in ((16384, 0), (-1, 0), (0, 1 << 48), (0, -1)):
        with pytest.raises(ValueError):
            make_memory_id(rank, seq)
    for bad in (-1, 1 << 63):
        with pytest.raises(ValueError):
            split_memory_id(bad)


def test_config_flag_defaults_off():
    assert PipelineConfig().memory_ids is False


# -- find_rows, the torch rule -------------------------------------------------

def _naive_find(col, want):
    out = []
    for w in want.tolist():
        rows = [r for r, v in enumerate(col.tolist()) if v == w and w >= 0]
        out.append(max(rows) if rows else -1)
    return out


def test_reference_find_rows():
    hi = 1 << 62
    col = torch.tensor([50, hi | 3, 7, 1 << 40, 7, 0, (5 << 48) | 9, -1], dtype=torch.int64)
    want = torch.tensor([7, 7, -1, 0, hi | 3, 8, (5 << 48) | 9, 9, 50, 1 << 40, (1 << 40) + 1,
                         -5, hi], dtype=torch.int64)
    got = g.reference_find_rows(col, want)
    assert got.dtype == torch.int32
    assert got.tolist() == _naive_find(col, want)
    assert got.tolist()[:3] == [4, 4, -1]  # an id held twice: the highest row; -1: never
    # CPU tensors take the same rule through the public entry
    assert torch.equal(g.find_rows(col, want), got)


def test_reference_find_rows_empty():
    col = torch.tensor([3, 4], dtype=torch.int64)
    none = torch.empty(0, dtype=torch.int64)
    assert g.reference_find_rows(none, col).tolist() == [-1, -1]
    out = g.reference_find_rows(col, none)
    assert out.shape == (0,) and out.dtype == torch.int32


def test_reference_find_rows_random():
    gen = torch.Generator().manual_seed(3)
    col = torch.randint(0, 200, (300,), generator=gen, dtype=torch.int64)
    want = torch.randint(-3, 260, (500,), generator=gen, dtype=torch.int64)
    assert g.reference_find_rows(col, want).tolist() == _naive_find(col, want)


# -- the id column through the CPU row movers ---------------------------------

def _buffers(cap, D, gen):
    index = torch.randn(cap, D, generator=gen).bfloat16()
    owner = torch.randint(0, 9, (cap,), generator=gen, dtype=torch.int32)
    sal = torch.rand(cap, generator=gen)
    ids = (1 << 62) | (5 << 48) | torch.randperm(cap, generator=gen).to(torch.int64)
    return index, owner, sal, ids


def test_move_rows_cpu_with_ids():
    gen = torch.Generator().manual_seed(1)
    cap = 40
    index, owner, sal, ids = _buffers(cap, 24, gen)
    perm = torch.randperm(cap, generator=gen)
    src, dst = perm[:11].to(torch.int32), perm[11:22].to(torch.int32)
    ref = [t.clone() for t in (index, owner, sal, ids)]
    for t in ref:
        t[dst.long()] = t[src.long()]
    g.index_move_rows(src, dst, index=index, owner=owner, salience=sal, ids=ids)
    for got, want in zip((index.view(torch.int16), owner, sal, ids),
                         (ref[0].view(torch.int16), ref[1], ref[2], ref[3])):
        assert torch.equal(got, want)
    # the id column alone
    ids2 = ref[3].clone()
    want2 = ids2.clone()
    want2[src.long()] = want2[dst.long()]
    g.index_move_rows(dst, src, ids=ids2)
    assert torch.equal(ids2, want2)


def test_index_forget_cpu_with_ids():
    gen = torch.Generator().manual_seed(2)
    cap, n = 50, 45
    index, owner, sal, ids = _buffers(cap, 16, gen)
    before = {int(i): (index[r].clone(), int(owner[r])) for r, i in enumerate(ids[:n])}
    dead = torch.rand(n, generator=gen) < 0.4
    gone = set(ids[:n][dead].tolist())
    n_new = g.index_forget(dead, index=index, owner=owner, salience=sal, ids=ids)
    assert n_new == n - len(gone)
    assert set(ids[:n_new].tolist()) == set(before) - gone
    for r in range(n_new):
        row, own = before[int(ids[r])]
        assert torch.equal(index[r].view(torch.int16), row.view(torch.int16))
        assert int(owner[r]) == own


# -- merge_topk_candidates with a payload --------------------------------------

def test_merge_payload_world1():
    s = torch.randn(4, 3)
    i = torch.arange(12, dtype=torch.int32).reshape(4, 3)
    p = torch.arange(12, dtype=torch.int64).reshape(4, 3) + (1 << 50)
    out = merge_topk_candidates(s, i, 0, 4, 1, 3, payload=p)
    assert len(out) == 3
    assert torch.equal(out[0], s) and torch.equal(out[1], i) and torch.equal(out[2], p)
    out = merge_topk_candidates(s, i, 0, 4, 1, 3)
    assert len(out) == 2 and torch.equal(out[1], i)


def _run_worker(rank, fn, port):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)
    try:
        fn(rank)
    finally:
        dist.destroy_process_group()


def _check_merge_payload(rank):
    # every rank scores all 4 queries against its 10-row shard; the score
    # grows with the global id, so the global top-2 are rows 9 and 8 of rank 1
    B, k, shard = 2, 2, 10
    local_ids = torch.tensor([[9, 8], [9, 8], [9, -1], [9, 8]], dtype=torch.int32)
    gids = globalize_ids(local_ids, rank, shard)
    scores = torch.where(local_ids < 0, torch.tensor(-1e30), gids.float() / 100.0)
    # the payload a pipeline would carry: the memory ids of its local rows
    payload = torch.where(local_ids < 0, torch.tensor(-1, dtype=torch.int64),
                          (rank << 48) | (local_ids.long() + 1000))
    s, i, p = merge_topk_candidates(scores, gids, rank, B, WORLD, k, payload=payload)
    assert p.dtype == torch.int64 and p.shape == (B, k)
    if rank == 0:
        assert i.tolist() == [[19, 18], [19, 18]]
        assert p.tolist() == [[(1 << 48) | 1009, (1 << 48) | 1008]] * 2
    else:
        # query 2 (the first of rank 1) has one candidate on either rank
        assert i.tolist() == [[19, 9], [19, 18]]
        assert p.tolist() == [[(1 << 48) | 1009, 1009], [(1 << 48) | 1009, (1 << 48) | 1008]]
    s2, i2 = merge_topk_candidates(scores, gids, rank, B, WORLD, k)
    assert torch.equal(s2, s) and torch.equal(i2, i)


def test_gloo_merge_payload():
    mp.spawn(_run_worker, args=(_check_merge_payload, 29641), nprocs=WORLD, join=True)


# -- FirewallService -----------------------------------------------------------

class _Stub:
    def __init__(self, with_ids):
        self.with_ids = with_ids

    def step(self, batch):
        n = len(batch.messages)
        res = {
            "verdict": torch.zeros(n, dtype=torch.int8),
            "risk": torch.zeros(n),
            "hits": {},
            "recall_ids": torch.full((n, 2), 7, dtype=torch.int32),
        }
        if self.with_ids:
            res["memory_ids"] = (3 << 48) + torch.arange(n, dtype=torch.int64)
            res["recall_mem_ids"] = torch.tensor([[(1 << 62) | 5, -1]] * n, dtype=torch.int64)
        return res


def test_service_passes_memory_ids_through():
    svc = FirewallService(_Stub(True), max_wait_ms=1.0)
    try:
        out = svc.check(b"hello")
        assert out["memoryId"] == 3 << 48
        assert out["recallMemoryIds"] == [(1 << 62) | 5, -1]
        assert out["recallIds"] == [7, 7]
    finally:
        svc.close()


def test_service_without_memory_ids_adds_nothing():
    svc = FirewallService(_Stub(False), max_wait_ms=1.0)
    try:
        out = svc.check(b"hello")
        assert set(out) == {"verdict", "risk", "hits", "recallIds"}
    finally:
        svc.close()
