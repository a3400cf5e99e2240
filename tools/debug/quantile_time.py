#!/usr/bin/env python3
"""Quantiles by radix select against the cheapest sort-based route.

  select   summary.quantiles(samples, (0.05, 0.5, 0.95)) on samples [N, C, D]
  sort     torch.sort(samples.reshape(-1, D), dim=0) -- reading three rows of it would give the same quantiles
usage: quantile_time.py [--draws N] [--chains C] [--dim D] [--repeats K]
Times are HIP events around one call, after one warm-up call of each; the two are timed alternately and the median,
minimum and maximum of the repeats are reported.  Bandwidth of the select = sweeps * 8 passes * N C D 8 bytes / time
(the bytes the histogram passes read; the counters are small beside them)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from aehmc_amd import summary  # noqa: E402

PROBS = (0.05, 0.5, 0.95)
PASSES, RANKS_PER_SWEEP = 8, 8


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def sweeps(R, probs):
    ranks = set()
    for p in probs:
        lo = int(np.floor(p * (R - 1)))
        ranks |= {lo, min(lo + 1, R - 1)}
    return -(-len(ranks) // RANKS_PER_SWEEP)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=500)
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--dim", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    N, C, D = args.draws, args.chains, args.dim
    g = torch.Generator(device="cuda").manual_seed(0)
    samples = torch.randn(N, C, D, dtype=torch.float64, device="cuda", generator=g)
    samples = samples * (0.5 + torch.rand(D, dtype=torch.float64, device="cuda", generator=g)) + 3.0

    def select():
        return summary.quantiles(samples, PROBS)

    def sort():
        return torch.sort(samples.reshape(-1, D), dim=0).values

    q = select()
    s = sort()
    R = N * C
    rows = [int(np.floor(p * (R - 1))) for p in PROBS]
    agree = all(bool(((s[r] <= q[i]) & (q[i] <= s[min(r + 1, R - 1)])).all()) for i, r in enumerate(rows))
    del s
    t_sel, t_sort = [], []
    for _ in range(args.repeats):
        t_sel.append(event_ms(select)[0])
        ms, s = event_ms(sort)
        del s
        t_sort.append(ms)
    nbytes = sweeps(R, PROBS) * PASSES * R * D * 8
    med = statistics.median(t_sel)
    print(json.dumps(dict(shape=[N, C, D], probs=PROBS, sweeps=sweeps(R, PROBS), passes=PASSES,
                          quantiles_between_sorted_neighbours=agree,
                          select_ms=med, select_ms_min=min(t_sel), select_ms_max=max(t_sel),
                          select_bytes=nbytes, select_tb_per_s=nbytes / (med * 1e-3) / 1e12,
                          sort_ms=statistics.median(t_sort), sort_ms_min=min(t_sort), sort_ms_max=max(t_sort),
                          sort_over_select=statistics.median(t_sort) / med)), flush=True)


if __name__ == "__main__":
    main()
