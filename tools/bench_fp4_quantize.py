#!/usr/bin/env python3
"""Measurements for the fused MXFP4 quantize / index-append kernel
(csrc/fp4_quantize.hip); results live in profiles/README.md, section
"fp4 quantize-append".

  quantize   quantize_fp4_mx vs to_fp4_mx at 4096 x 1024 (the per-step Q)
             and 1M x 1024 (one index build chunk): ms and GB/s, hipEvent
             timed, alternating the two. Bytes = 2 B read + 0.53125 B
             written per element (codes D/2 + scales D/32 per row).
  append     index_append alone at the per-step shape (kept rows of a 4096
             batch into a large index): ms and GB/s, bytes = 2 B read +
             2.53125 B written per element.
  ingest     the pipeline step at the bench shape with ingest off, off plus
             a host read of the kept count, and on: the first difference is
             the host read, the second the append, its bookkeeping and what
             the grown index does to recall. Run for two kinds of content:
             the template-built synthetic messages of bench.py (heavily
             clustered: a query has thousands of near-duplicates among the
             ingested rows) and random-letter messages (no clusters). Also
             prints per-stage hipEvent ms and how many queries per step took
             the direct-kernel fallback of the threshold recall.

Every mode needs a GPU and prints one JSON line per measurement.
"""

import argparse
import gc
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from vainplex_openclaw_amd.ops import gpu as g  # noqa: E402


def _time(fn, iters, warmup=3, reps=1):
    """Per-call ms over `iters` hipEvent windows of `reps` back-to-back calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) / reps)
    ts.sort()
    return {"ms_median": ts[len(ts) // 2], "ms_min": ts[0], "ms_max": ts[-1]}


def mode_quantize(args):
    for n, iters, reps in ((4096, 50, 20), (1_000_000, 10, 1)):
        D = 1024
        x = torch.nn.functional.normalize(
            torch.randn(n, D, device="cuda"), dim=1).bfloat16()
        a4, a_s = g.to_fp4_mx(x)
        b4, b_s = g.quantize_fp4_mx(x)
        same = bool(torch.equal(a4, b4) and torch.equal(a_s, b_s))
        del a4, a_s, b4, b_s
        nbytes = n * D * (2 + 0.5 + 1 / 32)
        res = {}
        # alternate the two so both see the same machine state
        for rnd in range(2):
            for name, fn in (("to_fp4_mx", lambda: g.to_fp4_mx(x)),
                             ("quantize_fp4_mx", lambda: g.quantize_fp4_mx(x))):
                t = _time(fn, iters, reps=reps)
                res.setdefault(name, []).append(t)
        for name, runs in res.items():
            for rnd, t in enumerate(runs):
                print(json.dumps({
                    "mode": "quantize", "op": name, "shape": [n, D], "round": rnd,
                    "bit_exact": same, **{k: round(v, 4) for k, v in t.items()},
                    "GBps_median": round(nbytes / t["ms_median"] / 1e6, 1)}), flush=True)


def mode_append(args):
    D, m, cap = 1024, 4096, 2_000_000
    feats = torch.nn.functional.normalize(
        torch.randn(m, D, device="cuda"), dim=1).bfloat16()
    src = torch.nonzero(torch.rand(m, device="cuda") < 0.92).flatten().to(torch.int32)
    n = int(src.numel())
    index = torch.zeros(cap, D, dtype=torch.bfloat16, device="cuda")
    x4 = torch.zeros(cap, D // 2, dtype=torch.uint8, device="cuda")
    xs = torch.zeros(cap, D // 32, dtype=torch.uint8, device="cuda")
    owner = torch.zeros(cap, dtype=torch.int32, device="cuda")
    owner_src = torch.zeros(m, dtype=torch.int32, device="cuda")
    sal = torch.ones(cap, device="cuda")
    row = [0]

    def fn():
        g.index_append(feats, src, row[0], index, x4, xs, owner, owner_src, sal, 1.0)
        row[0] = (row[0] + n) % (cap - n)

    t = _time(fn, 50, reps=20)
    nbytes = n * D * (2 + 2 + 0.5 + 1 / 32)
    print(json.dumps({"mode": "append", "rows": n, "D": D,
                      **{k: round(v, 4) for k, v in t.items()},
                      "GBps_median": round(nbytes / t["ms_median"] / 1e6, 1)}), flush=True)


def mode_ingest(args):
    from vainplex_openclaw_amd.pipeline.engine import (
        V_DENY, FirewallPipeline, PipelineConfig, StagingRing)
    from vainplex_openclaw_amd.pipeline.synth import TOOL_RISKS, SynthBatch, synthetic_batch

    def random_batch(n, seed):
        rng = np.random.default_rng(seed)
        msgs = [rng.integers(97, 123, size=300, dtype=np.uint8).tobytes() for _ in range(n)]
        return SynthBatch(msgs, rng.integers(0, 64, size=n).astype(np.int32),
                          rng.choice(TOOL_RISKS, size=n).astype(np.float32),
                          np.zeros(n, dtype=np.int8))

    # queries that overflow or underflow the threshold scan's candidate
    # buffer are redone by the direct kernel: count them
    fallback = []
    direct = g.topk_recall

    def counting_direct(Q, X, k, *a, **kw):
        fallback.append(int(Q.shape[0]))
        return direct(Q, X, k, *a, **kw)

    g.topk_recall = counting_direct

    shard = (args.index // 128) * 128
    make = {"synthetic": lambda i: synthetic_batch(args.batch, seed=i),
            "random": lambda i: random_batch(args.batch, i)}
    total = args.steps + args.warmup
    variants = [(c, v) for _ in range(args.rounds) for c in args.content.split(",")
                for v in ("off", "off+read", "on")]
    for content, v in variants:
        pool = [make[content](i) for i in range(4)]
        del fallback[:]
        cfg = PipelineConfig(batch=args.batch, dim=args.dim, index_size=shard,
                             ingest=(v == "on"),
                             ingest_capacity=(total + 3) * args.batch)
        pipe = FirewallPipeline(cfg, device="cuda:0")
        ring = StagingRing(pipe, max_bytes=8 << 20, max_msgs=max(args.batch, 8192) + 1)
        nxt = ring.stage(pool[0])
        kept = 0
        for i in range(total):
            if i == args.warmup:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            cur, nxt = nxt, ring.stage(pool[(i + 1) % len(pool)])
            out = pipe.step(None, staged=cur)
            if v == "off+read":
                kept += int(torch.nonzero(out["verdict"] != V_DENY).numel())
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / args.steps * 1000
        rows_after, fb = pipe.n_rows, sum(fallback) / total
        # per-stage timing outside the timed loop (the profiler synchronizes)
        pipe.profiler.enabled = True
        for i in range(3):
            pipe.step(None, staged=ring.stage(pool[i % len(pool)]))
            pipe.profiler.commit()
        stages = {k: round(x, 3) for k, x in pipe.profiler.summary().items()}
        print(json.dumps({"mode": "ingest", "content": content, "variant": v,
                          "ms_per_step": round(ms, 3), "rows_after": rows_after,
                          "dropped": pipe.ingest_dropped, "index_rows": shard,
                          "batch": args.batch, "fallback_queries_per_step": round(fb, 1),
                          "stage_ms": stages}), flush=True)
        del pipe, ring, nxt, cur, out
        gc.collect()
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["quantize", "append", "ingest"])
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--index", type=int, default=50_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--content", default="synthetic,random",
                    help="ingest mode: comma list of synthetic, random")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    {"quantize": mode_quantize, "append": mode_append, "ingest": mode_ingest}[args.mode](args)


if __name__ == "__main__":
    main()
