#!/usr/bin/env python
"""Timings of the posterior summaries.

1. The moments update (aehmc_summary_update, split chains) on draws [64, 4096, 10^4] and [1000, 4096, 100] against
   `torch.var_mean(samples, dim=0)` followed by the same cross-chain arithmetic in torch, on the same tensor.  The update
   reads every byte once: its bytes/s are set beside the HBM rate.  Each candidate is warmed up, then timed with HIP
   events over `--reps` alternating repetitions; the median and the spread are reported.
2. k_summary_final alone on the moments of c3's shape ([2, 4096, 10^4]: what every summary.run pays once), and the
   autocovariance call of summarize() on [1000, 4096, 100] (every lag of the 500-draw segments).
3. summary.run against kernel.sample(keep_samples=False) at c3's shape (bench.py: 4096 chains, 10^4 coordinates, dense
   metric) for `--transitions` transitions, alternating, same seeds.

    python tools/summary_bench.py [--reps 7] [--transitions 4] [--skip-c3] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def torch_cross_chain(x):
    """What a user would write: per-chain moments over the draws of each half, then the cross-chain statistics."""
    N = x.shape[0]
    h = N // 2
    v0, m0 = torch.var_mean(x[:h], dim=0)
    v1, m1 = torch.var_mean(x[N - h:], dim=0)
    v, m = torch.cat([v0, v1]), torch.cat([m0, m1])
    W, Bn = v.mean(dim=0), m.var(dim=0)
    varp = W * (h - 1) / h + Bn
    return m.mean(dim=0), torch.sqrt(varp), torch.sqrt(varp / W), torch.sqrt(Bn / m.shape[0])


def bench_update(shape, reps):
    from aehmc_amd import summary
    N, C, D = shape
    x = torch.randn(N, C, D, dtype=torch.float64, device="cuda")
    acc = summary.Accumulator(N, C, (D,))

    def ours():
        acc.mean.zero_()
        acc.m2.zero_()
        acc.seen = 0
        return acc.update(x).result()

    def update_only():
        acc._eng.summary_update(x, 0, N, 2, acc.mean, acc.m2)  # (folds on top of what is there: timing only)

    got, ref = ours(), torch_cross_chain(x)
    for a, b in zip((got.mean, got.sd, got.rhat, got.mcse_chains), ref):
        assert torch.allclose(a, b, rtol=1e-9, atol=1e-12)
    t = {"update": [], "update+final": [], "torch": []}
    for _ in range(reps):  # alternate the candidates: drift of the shared host hits them alike
        t["update"] += timed(update_only, 1, warmup=1)
        t["update+final"] += timed(ours, 1, warmup=1)
        t["torch"] += timed(lambda: torch_cross_chain(x), 1, warmup=1)
    nbytes = x.numel() * 8
    out = {"shape": list(shape), "bytes": nbytes}
    for k, v in t.items():
        out[k] = {"median_ms": float(np.median(v)), "min_ms": min(v), "max_ms": max(v)}
    out["update"]["TB_per_s"] = nbytes / (out["update"]["median_ms"] * 1e-3) / 1e12
    out["torch_over_ours"] = out["torch"]["median_ms"] / out["update+final"]["median_ms"]
    return out


def bench_final_and_acov(reps):
    from aehmc_amd import summary
    from aehmc_amd.engine import get_engine
    eng = get_engine()
    out = {}
    C, D = 4096, 10_000
    mean = torch.randn(2, C, D, dtype=torch.float64, device="cuda")
    m2 = torch.rand(2, C, D, dtype=torch.float64, device="cuda") * 31
    ms = timed(lambda: eng.summary_final(64, 2, mean, m2), reps)
    out["final_c3_shape"] = {"moments_bytes": 2 * mean.numel() * 8, "median_ms": float(np.median(ms)), "min_ms": min(ms),
                             "max_ms": max(ms), "TB_per_s_two_passes_over_the_means_one_over_m2":
                                 3 * mean.numel() * 8 / (float(np.median(ms)) * 1e-3) / 1e12}
    del mean, m2
    N, C, D = 1000, 4096, 100
    x = torch.randn(N, C, D, dtype=torch.float64, device="cuda")
    acc = summary.Accumulator(N, C, (D,)).update(x)
    ms = timed(lambda: eng.summary_autocov(x, 2, N // 2, acc.mean), reps, warmup=1)
    mac = 2 * C * D * sum(N // 2 - k for k in range(N // 2))
    out["autocov"] = {"shape": [N, C, D], "lags": N // 2, "median_ms": float(np.median(ms)), "min_ms": min(ms),
                      "max_ms": max(ms), "multiply_adds": mac, "Tmac_per_s": mac / (float(np.median(ms)) * 1e-3) / 1e12}
    ms = timed(lambda: summary.summarize(x), max(2, reps // 2), warmup=1)
    out["summarize"] = {"shape": [N, C, D], "median_ms": float(np.median(ms)), "min_ms": min(ms), "max_ms": max(ms)}
    return out


def bench_c3(transitions, reps):
    from bench import build_c3
    from aehmc_amd import RandomStream, nuts, summary, targets
    C, D = 4096, 10_000
    Sigma, P = build_c3(D, "cuda")
    target = targets.DenseMVN(torch.zeros(D, dtype=torch.float64, device="cuda"), P)
    eps = 0.5 * D ** -0.25
    q0 = torch.as_tensor(np.random.default_rng(1234).standard_normal((C, D)), device="cuda")
    state = nuts.new_state(q0, target)
    times = {"plain": [], "summary.run": []}
    for rep in range(reps + 1):  # (the first repetition warms both up and is dropped)
        for name in ("plain", "summary.run"):
            kernel = nuts.new_kernel(RandomStream(seeds=[1000 + c for c in range(C)]), target, max_num_expansions=10)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if name == "plain":
                kernel.sample(state, eps, Sigma, transitions, keep_samples=False)
            else:
                summary.run(kernel, state, eps, Sigma, transitions)
            torch.cuda.synchronize()
            if rep:
                times[name].append(time.perf_counter() - t0)
    out = {"chains": C, "D": D, "transitions": transitions}
    for k, v in times.items():
        out[k] = {"median_s": float(np.median(v)), "min_s": min(v), "max_s": max(v)}
    out["overhead"] = out["summary.run"]["median_s"] / out["plain"]["median_s"] - 1.0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--transitions", type=int, default=4)
    ap.add_argument("--skip-c3", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {}

    def stage(name, value):  # (the file is rewritten after every stage: a run cut short keeps what it measured)
        res[name] = value
        print(json.dumps({name: value}), flush=True)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)

    stage("update", [bench_update(s, args.reps) for s in ((64, 4096, 10_000), (1000, 4096, 100))])
    stage("final_and_autocov", bench_final_and_acov(args.reps))
    if not args.skip_c3:
        stage("c3", bench_c3(args.transitions, max(2, args.reps // 3)))

if __name__ == "__main__":
    main()
