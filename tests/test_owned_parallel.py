"""allgather_owners under gloo (world_size=2): gathered query owners line up
row for row with the gathered queries.
"""

import os

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from vainplex_openclaw_amd.parallel.collectives import allgather_owners, allgather_queries

WORLD = 2


def _run_worker(rank, fn, port):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)
    try:
        fn(rank)
    finally:
        dist.destroy_process_group()


def test_world1_passthrough():
    qo = torch.tensor([3, -1, 0], dtype=torch.int32)
    assert allgather_owners(qo, 1) is qo


def _check_owners_follow_queries(rank):
    B, D = 3, 4
    # query row b of rank r carries its owner in every component
    my_owner = torch.tensor([10 * rank + b for b in range(B)], dtype=torch.int32)
    if rank == 1:
        my_owner[1] = -1  # an unfiltered query travels as is
    feats = my_owner.float().unsqueeze(1).expand(B, D).contiguous()
    q_all = allgather_queries(feats, WORLD)
    o_all = allgather_owners(my_owner, WORLD)
    assert o_all.dtype == torch.int32 and o_all.shape == (WORLD * B,)
    assert o_all.tolist() == [0, 1, 2, 10, -1, 12]
    assert torch.equal(q_all[:, 0], o_all.float())
    assert torch.equal(o_all[rank * B : (rank + 1) * B], my_owner)


def test_gloo_allgather_owners():
    mp.spawn(_run_worker, args=(_check_owners_follow_queries, 29641), nprocs=WORLD, join=True)
