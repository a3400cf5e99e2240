"""Wall time of the ChEES calls against the launch-rate floor: chees.sample(N) and chees.run(N) at C chains of a
DiagGaussian target with a diagonal metric, and kernel.sample with an int L of the same total leapfrog count (one launch
for the whole call: what the jittered call can at best cost).  Uses the public interface only, so the same file times
any commit.  Per configuration: warm-up calls first, then `--repeats` device-synchronised wall times; median, min and
max are reported, per call and per transition, one JSON line each.

    python tools/debug/chees_launch_time.py [--chains 4096] [--dims 20 100] [--n 200] [--repeats 9]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import aehmc_amd as aa  # noqa: E402
from aehmc_amd import chees, targets  # noqa: E402


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def report(what, D, C, n, times, **extra):
    ms = sorted(1e3 * t for t in times)
    row = dict(what=what, D=D, C=C, transitions=n, median_ms=statistics.median(ms), min_ms=ms[0], max_ms=ms[-1],
               us_per_transition_median=1e3 * statistics.median(ms) / n, us_per_transition_min=1e3 * ms[0] / n,
               us_per_transition_max=1e3 * ms[-1] / n, repeats=len(ms), **extra)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--dims", type=int, nargs="+", default=[20, 100])
    ap.add_argument("--n", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    C, n = args.chains, args.n
    for D in args.dims:
        sigma = np.linspace(1.0, 3.0, D)
        target = targets.DiagGaussian(np.zeros(D), sigma)
        imm = torch.as_tensor(np.linspace(0.8, 1.6, D), device="cuda")
        q0 = torch.as_tensor(np.random.default_rng(D).normal(size=(C, D)), device="cuda")
        kernel = aa.hmc.new_kernel(aa.RandomStream(seeds=range(C)), target)
        state = aa.hmc.new_state(q0, target)
        eps, T = 0.3, 3.0
        lengths = [chees.num_integration_steps(eps, T, 1 + i) for i in range(n)]
        total = sum(lengths)
        L = max(1, round(total / n))
        report("chees.sample", D, C, n, timed(lambda: chees.sample(kernel, state, eps, imm, T, n), args.warmup, args.repeats),
               leapfrogs=total)
        report("chees.sample keep_samples=False", D, C, n,
               timed(lambda: chees.sample(kernel, state, eps, imm, T, n, keep_samples=False), args.warmup, args.repeats),
               leapfrogs=total)
        report("kernel.sample int L (floor)", D, C, n,
               timed(lambda: kernel.sample(state, eps, imm, L, n), args.warmup, args.repeats), leapfrogs=L * n, L=L)
        report("chees.run", D, C, n, timed(lambda: chees.run(kernel, state, n, imm), args.warmup, args.repeats))
        _, (eps_w, _, T_w), _ = chees.run(kernel, state, n, imm)
        print(json.dumps(dict(what="chees.run result", D=D, step_size=eps_w, trajectory_length=T_w,
                              mean_final_length=0.5 * T_w / eps_w)), flush=True)


if __name__ == "__main__":
    main()
