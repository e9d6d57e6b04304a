#!/usr/bin/env python3
"""Microbenchmark for the recall kernels: isolates scan dtype (bf16 vs
fp8), candidate width k, and queue effects. Prints one line per config.
"""

import argparse
import sys
import time

import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.abspath(__file__)) + "/..")

from vainplex_openclaw_amd.ops import gpu as g


def timed(fn, iters=3, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4_194_304)
    ap.add_argument("--nq", type=int, default=4096)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--short", action="store_true", help="1 iter of the two main configs")
    args = ap.parse_args()

    torch.manual_seed(0)
    dev = "cuda:0"
    Q = torch.nn.functional.normalize(torch.randn(args.nq, args.dim, device=dev), dim=1).bfloat16()
    X = torch.nn.functional.normalize(torch.randn(args.rows, args.dim, device=dev), dim=1).bfloat16()
    X8 = g.to_fp8_bytes(X)
    Q8 = g.to_fp8_bytes(Q)

    configs = [
        ("bf16 k=16", lambda: g.topk_recall(Q, X, 16)),
        ("fp8  k=16", lambda: g.topk_recall_fp8(Q8, X8, 16)),
    ]
    if not args.short:
        configs += [
            ("bf16 k=32", lambda: g.topk_recall(Q, X, 32)),
            ("fp8  k=32", lambda: g.topk_recall_fp8(Q8, X8, 32)),
            ("two-stage k=16 (of=4)", lambda: g.topk_recall_two_stage(Q, X, X8, 16)),
            ("two-stage k=16 (of=2)", lambda: g.topk_recall_two_stage(Q, X, X8, 16, overfetch=2)),
        ]
    iters = 1 if args.short else args.iters
    for name, fn in configs:
        ms = timed(fn, iters=iters, warmup=1)
        gb = args.rows * args.dim * (1 if "fp8" in name else 2) / 1e9
        work_tf = 2 * args.nq * args.rows * args.dim / 1e12
        print(f"{name:24s} {ms:9.2f} ms   {work_tf/ms*1000:7.1f} TF/s   index {gb:.1f} GB")




def scan_only_bench():
    import torch, time
    from vainplex_openclaw_amd.ops import gpu as g
    torch.manual_seed(0)
    dev = "cuda:0"
    rows, nq, dim = 4_194_304, 4096, 1024
    Q = torch.nn.functional.normalize(torch.randn(nq, dim, device=dev), dim=1).bfloat16()
    X = torch.nn.functional.normalize(torch.randn(rows, dim, device=dev), dim=1).bfloat16()
    X8 = g.to_fp8_bytes(X); Q8 = g.to_fp8_bytes(Q)
    for name, fn in [
        ("scan-only bf16 S=16", lambda: g.ext().topk_scan_only(Q, X, 16, False)),
        ("scan-only fp8  S=16", lambda: g.ext().topk_scan_only(Q8, X8, 16, True)),
        ("scan-only MX   S=16", lambda: g.ext().topk_scan_only(Q8, X8, 16, True, True)),
        ("scan-only MX   S=8",  lambda: g.ext().topk_scan_only(Q8, X8, 8, True, True)),
        ("scan-only bf16 S=8",  lambda: g.ext().topk_scan_only(Q, X, 8, False)),
        ("scan-only bf16 S=32", lambda: g.ext().topk_scan_only(Q, X, 32, False)),
    ]:
        ms = timed(fn, iters=3, warmup=1)
        print(f"{name:24s} {ms:9.2f} ms   {2*nq*rows*dim/1e12/ms*1000:7.1f} TF/s")




def threshold_bench():
    import torch
    from vainplex_openclaw_amd.ops import gpu as g
    torch.manual_seed(0)
    dev = "cuda:0"
    rows, nq, dim = 4_194_304, 4096, 1024
    Q = torch.nn.functional.normalize(torch.randn(nq, dim, device=dev), dim=1).bfloat16()
    X = torch.nn.functional.normalize(torch.randn(rows, dim, device=dev), dim=1).bfloat16()
    X8 = g.to_fp8_bytes(X)
    X4 = g.to_fp4_mx(X)
    for name, fn in [
        ("thresh bf16 k=16", lambda: g.topk_recall_threshold(Q, X, 16)),
        ("thresh fp8  k=16", lambda: g.topk_recall_threshold(Q, X, 16, X8=X8, mx=False)),
        ("thresh MX   k=16", lambda: g.topk_recall_threshold(Q, X, 16, X8=X8)),
        ("thresh fp4  k=16", lambda: g.topk_recall_threshold(Q, X, 16, X4=X4, q4=False)),
        ("thresh fp4x4 k=16", lambda: g.topk_recall_threshold(Q, X, 16, X4=X4)),
        ("thresh bf16 k=32", lambda: g.topk_recall_threshold(Q, X, 32)),
        ("direct bf16 k=16", lambda: g.topk_recall(Q, X, 16)),
    ]:
        ms = timed(fn, iters=2, warmup=1)
        print(f"{name:24s} {ms:9.2f} ms   {2*nq*rows*dim/1e12/ms*1000:7.1f} TF/s")


def fp4_scan_bench(variants=(("v7", 7), ("v9", 9), ("v10", 10)), iters=5):
    """fp4x4 threshold scan at 4.2M x 4096 x 1024 with production-like
    theta (tools/ab_fp4v2.py): full vs scan-only (epilogue skipped) per
    kernel variant; the difference is that kernel's epilogue share."""
    import torch
    from vainplex_openclaw_amd.ops import gpu as g
    torch.manual_seed(7)
    dev = "cuda:0"
    rows, nq, dim, cap = 4_194_304, 4096, 1024, 1024
    X = torch.nn.functional.normalize(torch.randn(rows, dim, device=dev), dim=1).bfloat16()
    Q = torch.nn.functional.normalize(torch.randn(nq, dim, device=dev), dim=1).bfloat16()
    X4, XS = g.to_fp4_mx(X)
    Q4, QS = g.to_fp4_mx(Q)
    s = torch.matmul(Q, X[:65536].T).float()
    theta = (s.mean(dim=1) + 4.2 * s.std(dim=1)).contiguous()
    del X, s
    for name, variant in variants:
        ms = {}
        for mode, scan_only in (("full", False), ("scan-only", True)):
            fn = lambda: g.ext().topk_scan_threshold_fp4x4(
                Q4, QS, X4, XS, theta, cap, 0, variant, scan_only)
            ms[mode] = timed(fn, iters=iters, warmup=2)
            hits = int(fn()[2].sum())
            print(f"fp4x4 {name} {mode:10s} {ms[mode]:9.3f} ms   "
                  f"{2*nq*rows*dim/1e12/ms[mode]*1000:7.1f} TF/s   hits {hits}")
        print(f"fp4x4 {name} epilogue   {ms['full'] - ms['scan-only']:9.3f} ms   "
              f"{100 * (ms['full'] - ms['scan-only']) / ms['full']:5.1f} % of full")


def timed_median(fn, iters=9, warmup=3):
    """Median of per-iteration device times (ms)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return sorted(ts)[len(ts) // 2]


def fp4_owned_scan_bench(n_owners, iters=9):
    """Cost of the in-kernel owner filter at the fp4_scan_bench shape, one
    session: v9 and v10 unfiltered (the yardsticks; the owned kernel shares
    v10's K-loop), then the owned kernel with 1 owner (same candidates as
    the unfiltered scans) and with `n_owners` uniform random
    owners. Thresholds are per owner (ops.gpu.owned_thresholds) with the
    candidate target that makes the 1-owner theta the unfiltered bench's
    mu + 4.2 sigma, so every config expects the same candidates per query."""
    import math
    torch.manual_seed(7)
    dev = "cuda:0"
    rows, nq, dim, cap = 4_194_304, 4096, 1024, 1024
    X = torch.nn.functional.normalize(torch.randn(rows, dim, device=dev), dim=1).bfloat16()
    Q = torch.nn.functional.normalize(torch.randn(nq, dim, device=dev), dim=1).bfloat16()
    X4, XS = g.to_fp4_mx(X)
    Q4, QS = g.to_fp4_mx(Q)
    s = torch.matmul(Q, X[:65536].T).float()
    mu, sigma = s.mean(dim=1), s.std(dim=1)
    del X, s
    target = 0.5 * math.erfc(4.2 / math.sqrt(2.0)) * rows
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)

    def owned(n):
        xo = torch.randint(0, n, (rows,), generator=gen, dtype=torch.int32, device=dev)
        qo = torch.randint(0, n, (nq,), generator=gen, dtype=torch.int32, device=dev)
        n_owned = torch.bincount(xo.long(), minlength=n)[qo.long()]
        th = g.owned_thresholds(mu, sigma, n_owned, target).contiguous()
        return lambda: g.ext().topk_scan_threshold_fp4x4_owned(
            Q4, QS, X4, XS, th, xo, qo, cap, 0)

    theta = (mu + 4.2 * sigma).contiguous()
    configs = [
        ("v9 unfiltered", lambda: g.ext().topk_scan_threshold_fp4x4(
            Q4, QS, X4, XS, theta, cap, 0, 9, False)),
        ("v10 unfiltered", lambda: g.ext().topk_scan_threshold_fp4x4(
            Q4, QS, X4, XS, theta, cap, 0, 10, False)),
        ("owned, 1 owner", owned(1)),
    ]
    if n_owners > 1:
        configs.append((f"owned, {n_owners} owners", owned(n_owners)))
    for name, fn in configs:
        ms = timed_median(fn, iters=iters)
        hits = int(fn()[2].sum())
        print(f"fp4x4 {name:20s} {ms:9.3f} ms (median of {iters})   "
              f"{2*nq*rows*dim/1e12/ms*1000:7.1f} TF/s   hits {hits}")


def fp4_hist_scan_bench(iters=9, rounds=3):
    """What the dropped-hit histogram costs a scan that drops nothing: the
    v10 scan against topk_scan_fp4_hist_kernel, and the owned scan (1 owner)
    against topk_scan_fp4_owned_hist_kernel, at the fp4_scan_bench shape and
    theta (no query overflows cap = 1024), alternating, `rounds` rounds of
    medians of `iters`."""
    torch.manual_seed(7)
    dev = "cuda:0"
    rows, nq, dim, cap = 4_194_304, 4096, 1024, 1024
    X = torch.nn.functional.normalize(torch.randn(rows, dim, device=dev), dim=1).bfloat16()
    Q = torch.nn.functional.normalize(torch.randn(nq, dim, device=dev), dim=1).bfloat16()
    X4, XS = g.to_fp4_mx(X)
    Q4, QS = g.to_fp4_mx(Q)
    s = torch.matmul(Q, X[:65536].T).float()
    theta = (s.mean(dim=1) + 4.2 * s.std(dim=1)).contiguous()
    del X, s
    w = ((1.0625 - theta) / g.HIST_NB).contiguous()
    xo = torch.zeros(rows, dtype=torch.int32, device=dev)
    qo = torch.zeros(nq, dtype=torch.int32, device=dev)
    e = g.ext()
    configs = [
        ("v10", lambda: e.topk_scan_threshold_fp4x4(Q4, QS, X4, XS, theta, cap, 0, 10, False)),
        ("v10 + hist", lambda: e.topk_scan_threshold_fp4x4_hist(
            Q4, QS, X4, XS, theta, w, cap, 0)),
        ("owned", lambda: e.topk_scan_threshold_fp4x4_owned(
            Q4, QS, X4, XS, theta, xo, qo, cap, 0)),
        ("owned + hist", lambda: e.topk_scan_threshold_fp4x4_hist(
            Q4, QS, X4, XS, theta, w, cap, 0, xowner=xo, qowner=qo)),
    ]
    for rnd in range(rounds):
        for name, fn in configs:
            ms = timed_median(fn, iters=iters)
            out = fn()
            print(f"fp4x4 round {rnd} {name:14s} {ms:9.3f} ms (median of {iters})   "
                  f"hits {int(out[2].sum())}   max/query {int(out[2].max())}   "
                  f"hist {int(out[3].sum()) if len(out) > 3 else '-'}")


if __name__ == "__main__":
    import sys as _sys
    if "--fp4-scan" in _sys.argv and "--hist" in _sys.argv:
        fp4_hist_scan_bench()
    elif "--fp4-scan" in _sys.argv and "--owners" in _sys.argv:
        fp4_owned_scan_bench(int(_sys.argv[_sys.argv.index("--owners") + 1]))
    elif "--fp4-scan" in _sys.argv:
        fp4_scan_bench()
    elif "--scan-only" in _sys.argv:
        scan_only_bench()
    elif "--threshold" in _sys.argv:
        threshold_bench()
    else:
        main()
