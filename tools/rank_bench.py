"""Times summary.rank_normalize on the device against (a) the bytes its passes move at the achievable HBM rate and
(b) a torch composition of the same ranks (sort along the pooled axis, searchsorted for the two bounds, ndtri).
Warm-up, repeated timed calls between device events, median.  Prints one JSON line per shape.

  python tools/rank_bench.py [--reps 7] [--once N C D]   (--once: a single call, for a kernel trace)"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from aehmc_amd import summary  # noqa: E402

HBM = 6.3e12  # achievable bytes / s
SHAPES = [(500, 4096, 100), (1000, 64, 1000)]


def composition(x):
    """The normal scores of x [N, C, D] by torch alone."""
    N, C, D = x.shape
    xt = x.reshape(N * C, D).t().contiguous()
    s = torch.sort(xt, dim=1).values
    lo = torch.searchsorted(s, xt, right=False)
    hi = torch.searchsorted(s, xt, right=True)
    r = (lo + hi + 1).to(torch.float64) * 0.5
    z = torch.special.ndtri((r - 0.375) / (N * C + 0.25))
    return z.t().contiguous().reshape(N, C, D)


def timed(f, reps):
    f()
    f()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--once", type=int, nargs=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    g = torch.Generator(device="cuda").manual_seed(1)
    if args.once:
        x = torch.randn(*args.once, dtype=torch.float64, device="cuda", generator=g)
        summary.rank_normalize(x)
        torch.cuda.synchronize()
        return
    for N, C, D in SHAPES:
        x = torch.randn(N, C, D, dtype=torch.float64, device="cuda", generator=g)
        z = summary.rank_normalize(x)
        ref = composition(x)
        err = float(((z - ref).abs() / ref.abs().clamp_min(1e-300)).max())
        del z, ref
        # per draw: keys 8 B read + 8 B written; 8 passes of 8 B counted, 8 B read and 8 B scattered; 8 B read and
        # 8 B written for the result (the bisection's reads of the sorted column not counted)
        moved = (16 + 8 * 24 + 16) * N * C * D
        res = {"shape": [N, C, D], "pooled_draws": N * C, "bytes_moved": moved, "floor_ms": moved / HBM * 1e3,
               "max_rel_diff_vs_composition": err}
        res["rank_normalize_ms"], res["rank_normalize_min_ms"], res["rank_normalize_max_ms"] = timed(
            lambda: summary.rank_normalize(x), args.reps)
        res["ranks_ms"] = timed(lambda: summary.ranks(x), args.reps)[0]
        res["torch_composition_ms"], res["torch_composition_min_ms"], res["torch_composition_max_ms"] = timed(
            lambda: composition(x), args.reps)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
