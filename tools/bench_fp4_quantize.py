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
             --overflow direct|rescan|direct,rescan picks
             PipelineConfig.recall_overflow; with both, every round runs the
             two modes one after the other (alternating), ingest on only,
             and each line carries recall ms per step and the pipeline's
             recall_overflowed / recall_rescanned / recall_direct_fallbacks
             per step. Results: profiles/README.md, "recall overflow rescan".
             --dedup TAU[,TAU...] adds one ingest-on variant per threshold
             with PipelineConfig.ingest_dedup = TAU, alternating with plain
             ingest on (the yardstick) in every round; every line carries
             ingest_merged_index / ingest_merged_batch, rows_after and the
             overflow counters. Results: profiles/README.md, "ingest dedup".
             --memory-ids runs, per round, plain ingest on, ingest on with
             PipelineConfig.memory_ids, and plain ingest on again: the
             first two are the pair, the two plain runs the spread.
             Results: profiles/README.md, "memory ids and snapshots".
  dedup      the two ingest-dedup kernels (csrc/ingest_dedup.hip) alone at
             the per-step shape (--batch x --dim, k = 16 recalled ids into a
             1M-row index): ms, hipEvent timed, on rows without duplicates,
             on clustered rows and on a batch of identical rows (every pair
             a hit: the most atomics the batch kernel can issue).
  forget     forgetting at the index shape (--index x --dim, 50M x 1024):
             1 % of the rows evicted from a salience vector with realistic
             ties. evict_mask and forget_plan ms; the move kernel
             (csrc/index_forget.hip) ms and GB/s, bytes = read + written,
             against the same plan executed with torch indexing on the same
             buffers, alternating the two; then the pipeline with
             ingest_full="evict" driven past a full shard: the evicting
             step's ms against the median plain step, per kind of content
             (--content). Results live in profiles/README.md, section
             "index forget".
  find       find_rows (csrc/index_ids.hip) against reference_find_rows
             (torch sort + searchsorted) on a column of --index distinct ids
             (50M) for 1, 4096 and 65 536 wanted ids, half of them present:
             wall ms around a device synchronise and the peak of
             torch.cuda.max_memory_allocated over what was allocated before
             the call, the two paths alternating.
  snapshot   FirewallPipeline.save_memory / load_memory at --index x --dim
             (1M x 1024 is the recorded shape), memory_ids and
             recall_isolation on: wall seconds and bytes written, to a
             temporary directory that is removed afterwards.

Every mode needs a GPU and prints one JSON line per measurement.
"""

import argparse
import gc
import json
import math
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


def random_batch(n, seed):
    """Random-letter messages: content without clusters."""
    from vainplex_openclaw_amd.pipeline.synth import TOOL_RISKS, SynthBatch

    rng = np.random.default_rng(seed)
    msgs = [rng.integers(97, 123, size=300, dtype=np.uint8).tobytes() for _ in range(n)]
    return SynthBatch(msgs, rng.integers(0, 64, size=n).astype(np.int32),
                      rng.choice(TOOL_RISKS, size=n).astype(np.float32),
                      np.zeros(n, dtype=np.int8))


def mode_ingest(args):
    from vainplex_openclaw_amd.pipeline.engine import (
        V_DENY, FirewallPipeline, PipelineConfig, StagingRing)
    from vainplex_openclaw_amd.pipeline.synth import synthetic_batch

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
    modes = args.overflow.split(",")
    for m in modes:
        if m not in ("direct", "rescan"):
            raise SystemExit(f"--overflow: unknown mode {m!r}")
    # comparing the two overflow modes: ingest on only, the modes alternate
    ingest_variants = ("on",) if len(modes) > 1 else ("off", "off+read", "on")
    taus = [float(t) for t in args.dedup.split(",")] if args.dedup else []
    if taus:
        # against plain ingest on, the parent's step, in the same round
        ingest_variants = ("on",) + tuple(f"on+dedup={t}" for t in taus)
    if args.memory_ids:
        ingest_variants = ("on", "on+ids", "on")
    variants = [(c, v, m) for _ in range(args.rounds) for c in args.content.split(",")
                for v in ingest_variants for m in modes]
    for content, v, overflow in variants:
        pool = [make[content](i) for i in range(4)]
        del fallback[:]
        cfg = PipelineConfig(batch=args.batch, dim=args.dim, index_size=shard,
                             ingest=v.startswith("on"),
                             ingest_capacity=(total + 3) * args.batch,
                             ingest_dedup=float(v.partition("=")[2] or 0.0),
                             memory_ids=v.endswith("+ids"),
                             recall_overflow=overflow)
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
        merged = {"ingest_merged_index": pipe.ingest_merged_index,
                  "ingest_merged_batch": pipe.ingest_merged_batch}
        counters = {k: round(getattr(pipe, k) / total, 1) for k in
                    ("recall_overflowed", "recall_rescanned", "recall_direct_fallbacks")}
        # per-stage timing outside the timed loop (the profiler synchronizes)
        pipe.profiler.enabled = True
        for i in range(3):
            pipe.step(None, staged=ring.stage(pool[i % len(pool)]))
            pipe.profiler.commit()
        stages = {k: round(x, 3) for k, x in pipe.profiler.summary().items()}
        print(json.dumps({"mode": "ingest", "content": content, "variant": v,
                          "overflow": overflow, "ms_per_step": round(ms, 3),
                          "recall_ms_per_step": stages.get("recall"),
                          **{k + "_per_step": x for k, x in counters.items()},
                          "rows_after": rows_after, **merged,
                          "dropped": pipe.ingest_dropped, "index_rows": shard,
                          "batch": args.batch, "fallback_queries_per_step": round(fb, 1),
                          "stage_ms": stages}), flush=True)
        del pipe, ring, nxt, cur, out
        gc.collect()
        torch.cuda.empty_cache()


def mode_dedup(args):
    B, D, k, n = args.batch, args.dim, 16, 1_000_000
    gen = torch.Generator(device="cuda").manual_seed(0)

    def unit(*shape):
        return torch.nn.functional.normalize(
            torch.randn(*shape, generator=gen, device="cuda"), dim=-1)

    X = unit(n, D).bfloat16()
    ids = torch.randint(0, n, (B, k), generator=gen, device="cuda", dtype=torch.int32)
    xowner = torch.randint(0, 64, (n,), generator=gen, device="cuda", dtype=torch.int32)
    qowner = torch.randint(0, 64, (B,), generator=gen, device="cuda", dtype=torch.int32)
    centres = unit(64, D)
    which = torch.randint(0, 64, (B,), generator=gen, device="cuda")
    rows = {"distinct": unit(B, D).bfloat16(),
            "clustered": torch.nn.functional.normalize(
                centres[which] + 0.15 * unit(B, D), dim=1).bfloat16(),
            "identical": unit(1, D).bfloat16().expand(B, D).contiguous()}
    elig = torch.ones(B, dtype=torch.bool, device="cuda")
    for name, F in rows.items():
        for owners in (False, True):
            qo = qowner if owners else None
            first = g.batch_first_similar(F, elig, 0.9, qo)
            stored = int((first == torch.arange(B, device="cuda")).sum())
            t = _time(lambda: g.batch_first_similar(F, elig, 0.9, qo), 30, reps=10)
            print(json.dumps({"mode": "dedup", "op": "batch_first_similar", "rows": name,
                              "owners": owners, "shape": [B, D], "stored": stored,
                              **{k_: round(v, 4) for k_, v in t.items()}}), flush=True)
    F = rows["distinct"]
    for owners in (False, True):
        own = dict(xowner=xowner, qowner=qowner) if owners else {}
        t = _time(lambda: g.recall_dup_rows(F, ids, X, 0.9, **own), 30, reps=10)
        print(json.dumps({"mode": "dedup", "op": "recall_dup_rows", "owners": owners,
                          "shape": [B, k, D], "index_rows": n,
                          **{k_: round(v, 4) for k_, v in t.items()}}), flush=True)


def _realistic_salience(n, batch_rows=3750, seed=3):
    """A salience vector with the ties a long-running shard has: rows
    ingested in one step and never recalled share a value bit for bit
    (0.9999^age, floored at 0.01, so the oldest 40 % sit on the floor), and
    2 % of the rows were recalled at some time and carry values of their
    own."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    steps = (n + batch_rows - 1) // batch_rows
    # the oldest step first; age chosen so that 40 % of the steps are floored
    age = torch.arange(steps, 0, -1, device="cuda", dtype=torch.float64)
    age = age * (math.log(0.01) / math.log(0.9999) / (0.6 * steps))
    per_step = (0.9999 ** age).clamp_min(0.01).float()
    sal = per_step.repeat_interleave(batch_rows)[:n].contiguous()
    hit = torch.rand(n, generator=gen, device="cuda") < 0.02
    own = torch.rand(n, generator=gen, device="cuda")
    return torch.where(hit, sal + 0.25 * own * (1.0 - sal), sal)


def mode_forget(args):
    from vainplex_openclaw_amd.pipeline.engine import (
        FirewallPipeline, PipelineConfig, StagingRing)
    from vainplex_openclaw_amd.pipeline.synth import synthetic_batch

    D = args.dim
    n = (args.index // 128) * 128
    count = n // 100
    index = torch.empty(n, D, dtype=torch.bfloat16, device="cuda")
    x4 = torch.empty(n, D // 2, dtype=torch.uint8, device="cuda")
    xs = torch.empty(n, D // 32, dtype=torch.uint8, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(1)
    for buf in (index.view(torch.int16), x4.view(torch.int16), xs.view(torch.int16)):
        for i in range(0, n, 1_000_000):
            c = buf[i:i + 1_000_000]
            c.copy_(torch.randint(-32768, 32768, c.shape, generator=gen,
                                  dtype=torch.int16, device="cuda"))
    owner = torch.arange(n, dtype=torch.int32, device="cuda")
    sal = _realistic_salience(n)
    uniq = int(torch.unique(sal).numel())
    common = {"mode": "forget", "rows": n, "D": D, "evict": count}

    def emit(op, t, **kw):
        print(json.dumps({**common, "op": op, **{k: round(v, 4) for k, v in t.items()}, **kw}),
              flush=True)

    dead = g.evict_mask(sal, count)
    assert int(dead.sum()) == count
    emit("evict_mask", _time(lambda: g.evict_mask(sal, count), 5, warmup=1),
         distinct_saliences=uniq)
    n_new, dst, src = g.forget_plan(dead)
    emit("forget_plan", _time(lambda: g.forget_plan(dead), 5, warmup=1),
         n_new=n_new, moved=int(dst.numel()))

    # the move is idempotent (sources stay, destinations are rewritten with
    # the same bytes), so the kernel and the baseline run the same plan
    # again and again on the same buffers: no second copy of the index
    m = int(dst.numel())
    row_bytes = 2 * D + D // 2 + D // 32 + 4 + 4
    nbytes = 2 * m * row_bytes  # read + written
    bufs = dict(index=index, X4=x4, XS=xs, owner=owner, salience=sal)

    def by_indexing():
        s, d = src.long(), dst.long()
        for b in bufs.values():
            b[d] = b[s]

    res = {}
    for rnd in range(2):
        for name, fn in (("index_move_rows", lambda: g.index_move_rows(src, dst, **bufs)),
                         ("torch_indexing", by_indexing)):
            res.setdefault(name, []).append(_time(fn, 5, warmup=1))
    probe = torch.arange(0, m, max(1, m // 4096), device="cuda")
    same = all(bool(torch.equal(b[dst[probe].long()].view(torch.uint8),
                                b[src[probe].long()].view(torch.uint8)))
               for b in bufs.values())
    for name, runs in res.items():
        for rnd, t in enumerate(runs):
            emit(name, t, round=rnd, moved=m, bytes=nbytes, rows_match=same,
                 GBps_median=round(nbytes / t["ms_median"] / 1e6, 1))
    del index, x4, xs, owner, sal, dead, dst, src, bufs, probe
    gc.collect()
    torch.cuda.empty_cache()

    # the pipeline driven past a full shard: one evicting step against the
    # plain steps around it (host clock, a synchronize after every step)
    make = {"synthetic": lambda i: synthetic_batch(args.batch, seed=i),
            "random": lambda i: random_batch(args.batch, i)}
    total = args.steps + args.warmup
    for content, rnd in ((c, r) for c in args.content.split(",") for r in range(args.rounds)):
        pool = [make[content](i) for i in range(4)]
        cfg = PipelineConfig(batch=args.batch, dim=D, index_size=n, ingest=True,
                             ingest_capacity=(args.warmup + 2) * args.batch,
                             ingest_full="evict")
        pipe = FirewallPipeline(cfg, device="cuda:0")
        ring = StagingRing(pipe, max_bytes=8 << 20, max_msgs=max(args.batch, 8192) + 1)
        plain, evicting = [], []
        for i in range(total):
            staged = ring.stage(pool[i % len(pool)])
            epoch = pipe.forget_epoch
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pipe.step(None, staged=staged)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1000
            if pipe.forget_epoch != epoch:
                evicting.append(round(ms, 3))
            elif i >= args.warmup:
                plain.append(ms)
        plain.sort()
        print(json.dumps({"mode": "forget", "op": "ingest_evict", "content": content,
                          "round": rnd,
                          "index_rows": n, "capacity": pipe.capacity, "batch": args.batch,
                          "evict_frac": cfg.evict_frac, "forgotten": pipe.forgotten,
                          "dropped": pipe.ingest_dropped, "rows_after": pipe.n_rows,
                          "plain_step_ms_median": round(plain[len(plain) // 2], 3),
                          "plain_steps": len(plain), "evicting_step_ms": evicting}),
              flush=True)
        del pipe, ring, staged
        gc.collect()
        torch.cuda.empty_cache()


def mode_find(args):
    n = args.index
    gen = torch.Generator(device="cuda").manual_seed(0)
    # distinct ids in no order: even numbers, so that odd ones are absent
    col = torch.randperm(n, generator=gen, device="cuda") * 2 + (1 << 48)
    paths = (("find_rows", g.find_rows), ("reference_find_rows", g.reference_find_rows))
    for m in (1, 4096, 65536):
        pick = col[torch.randint(0, n, (m,), generator=gen, device="cuda")]
        want = pick + (torch.arange(m, device="cuda") & 1)  # every other one absent
        outs = {}
        for rnd in range(-1, args.rounds):  # round -1 warms both paths up
            for name, fn in paths:
                gc.collect()
                torch.cuda.empty_cache()
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                before = torch.cuda.memory_allocated()
                t0 = time.perf_counter()
                out = fn(col, want)
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) * 1000
                peak = torch.cuda.max_memory_allocated() - before
                outs[name] = out
                if rnd < 0:
                    continue
                print(json.dumps({"mode": "find", "op": name, "rows": n, "wanted": m,
                                  "round": rnd, "ms": round(ms, 3),
                                  "peak_extra_MB": round(peak / 1e6, 2),
                                  "found": int((out >= 0).sum())}), flush=True)
        print(json.dumps({"mode": "find", "wanted": m, "paths_equal": bool(
            torch.equal(outs["find_rows"], outs["reference_find_rows"]))}), flush=True)
        del outs, out


def mode_snapshot(args):
    import shutil
    import tempfile

    from vainplex_openclaw_amd.pipeline.engine import FirewallPipeline, PipelineConfig

    cfg = PipelineConfig(batch=args.batch, dim=args.dim, index_size=args.index,
                         recall_isolation=True, memory_ids=True, ingest=True,
                         ingest_capacity=args.batch)
    pipe = FirewallPipeline(cfg, device="cuda:0")
    other = FirewallPipeline(cfg, device="cuda:0")
    root = tempfile.mkdtemp(prefix="memory-snapshot-")
    try:
        for rnd in range(args.rounds):
            path = os.path.join(root, f"snap{rnd}")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            man = pipe.save_memory(path)
            t1 = time.perf_counter()
            other.load_memory(path)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            same = bool(torch.equal(other.index4[0][:pipe.n_rows], pipe.index4[0][:pipe.n_rows])
                        and torch.equal(other.index_ids, pipe.index_ids))
            print(json.dumps({"mode": "snapshot", "rows": pipe.n_rows, "dim": args.dim,
                              "round": rnd, "bytes": sum(man["files"].values()),
                              "save_s": round(t1 - t0, 3), "load_s": round(t2 - t1, 3),
                              "restored_equal": same}), flush=True)
            shutil.rmtree(path)
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["quantize", "append", "ingest", "forget", "dedup",
                                     "find", "snapshot"])
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--index", type=int, default=50_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--overflow", default="direct",
                    help="ingest mode: PipelineConfig.recall_overflow, direct, rescan "
                         "or direct,rescan (alternating)")
    ap.add_argument("--dedup", default="",
                    help="ingest mode: comma list of PipelineConfig.ingest_dedup "
                         "thresholds, each a variant beside plain ingest on")
    ap.add_argument("--memory-ids", action="store_true",
                    help="ingest mode: plain ingest on, ingest on with memory ids, plain "
                         "ingest on again, per round")
    ap.add_argument("--content", default="synthetic,random",
                    help="ingest and forget modes: comma list of synthetic, random")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    {"quantize": mode_quantize, "append": mode_append, "ingest": mode_ingest,
     "forget": mode_forget, "dedup": mode_dedup, "find": mode_find,
     "snapshot": mode_snapshot}[args.mode](args)


if __name__ == "__main__":
    main()
