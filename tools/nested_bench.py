#!/usr/bin/env python
"""Timings of the nested R-hat, 4096 chains in 64 superchains.

1. `summary.nested_rhat(samples, 64, window=1)` on stored draws [1000, 4096, 100] against the torch expression of the
   same quantities on the same tensor.
2. One `NestedAccumulator.update` of a 1 GiB chunk at D = 10^4 (3 draws): with window=1 (three windows end in the chunk:
   k_nested_window alone) and inside one long window (k_nested_fold alone), against the torch expression of the
   windowed quantities and against torch.var_mean over the draws.
Each candidate is warmed up, then timed with HIP events over `--reps` alternating repetitions; the median and the spread
are reported, and the bytes of the chunk per second beside them.

3. `--launches`: nothing is timed; a run of 1000 draws of [64, 8] is folded whole and in chunks of 1, 7 and 250 with
   window=1 and window=4.  Put under `rocprofv3 --kernel-trace --stats`, the calls of k_nested_window and k_nested_fold
   divided by the updates printed here are the launches per update.

    python tools/nested_bench.py [--reps 7] [--only stored|chunk] [--out FILE.json] | --launches
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

C, K = 4096, 64


def timed(fn):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def torch_nested(x, w):
    """What a user would write for windows of w draws of x [N, C, D]: (nested_rhat, between, within, mean, mcse)."""
    N, _, D = x.shape
    xw = x.reshape(N // w, w, K, C // K, D)
    if w > 1:
        s2, a = torch.var_mean(xw, dim=1)
    else:
        a, s2 = xw[:, 0], None
    btil, abar_k = torch.var_mean(a, dim=2)
    within = btil if s2 is None else btil + s2.mean(dim=2)
    within = within.mean(dim=1)
    between, abar = torch.var_mean(abar_k, dim=1)
    return torch.sqrt(1.0 + between / within), between, within, abar, torch.sqrt(between / K)


def summarise(t, nbytes):
    out = {}
    for k, v in t.items():
        med = float(np.median(v))
        out[k] = {"median_ms": med, "min_ms": min(v), "max_ms": max(v), "TB_per_s": nbytes / (med * 1e-3) / 1e12}
    return out


def check(got, ref):
    for a, b in zip((got.nested_rhat, got.between, got.within, got.mean, got.mcse_superchains), ref):
        assert torch.allclose(a, b.reshape(a.shape), rtol=1e-9, atol=1e-12)


def bench_stored(reps):
    from aehmc_amd import summary
    N, D = 1000, 100
    x = torch.randn(N, C, D, dtype=torch.float64, device="cuda")
    check(summary.nested_rhat(x, K, window=1), torch_nested(x, 1))
    t = {"nested_rhat": [], "torch": []}
    for _ in range(reps):
        t["nested_rhat"].append(timed(lambda: summary.nested_rhat(x, K, window=1)))
        t["torch"].append(timed(lambda: torch_nested(x, 1)))
    out = {"shape": [N, C, D], "window": 1, "bytes": x.numel() * 8, **summarise(t, x.numel() * 8)}
    out["torch_over_ours"] = out["torch"]["median_ms"] / out["nested_rhat"]["median_ms"]
    return out


def bench_chunk(reps):
    from aehmc_amd import summary
    D = 10_000
    T = (1 << 30) // (8 * C * D)
    x = torch.randn(T, C, D, dtype=torch.float64, device="cuda")
    ends = summary.NestedAccumulator(T, C, (D,), K, window=1)
    inside = summary.NestedAccumulator(64 * T, C, (D,), K)
    check(ends.update(x).result(), torch_nested(x, 1))

    def update(acc):
        acc.seen = 0
        acc.update(x)

    t = {"update_window_1": [], "update_inside_a_window": [], "torch_window_1": [], "torch_var_mean": []}
    for _ in range(reps):
        t["update_window_1"].append(timed(lambda: update(ends)))
        t["update_inside_a_window"].append(timed(lambda: update(inside)))
        t["torch_window_1"].append(timed(lambda: torch_nested(x, 1)))
        t["torch_var_mean"].append(timed(lambda: torch.var_mean(x, dim=0)))
    return {"shape": [T, C, D], "bytes": x.numel() * 8, **summarise(t, x.numel() * 8)}


def launches():
    from aehmc_amd import summary
    N, Cs, D = 1000, 64, 8
    x = torch.randn(N, Cs, D, dtype=torch.float64, device="cuda")
    updates = 0
    for w in (1, 4):
        for chunk in (N, 1, 7, 250):
            acc = summary.NestedAccumulator(N, Cs, (D,), 8, window=w)
            for lo in range(0, N, chunk):
                acc.update(x[lo:lo + chunk])
                updates += 1
            acc.result()
    torch.cuda.synchronize()
    print(json.dumps({"updates": updates, "draws": N, "windows": [1, 4], "chunks": [N, 1, 7, 250]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--only", choices=("stored", "chunk"), default=None,
                    help="one of the two shapes alone (a kernel trace then holds one shape per kernel)")
    args = ap.parse_args()
    if args.launches:
        return launches()
    res = {}
    for name, fn in (("stored", bench_stored), ("chunk", bench_chunk)):
        if args.only not in (None, name):
            continue
        res[name] = fn(args.reps)
        print(json.dumps({name: res[name]}), flush=True)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
