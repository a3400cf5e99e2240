#!/usr/bin/env python3
"""What generalised HMC and the MEADS warm-up cost: 4096 chains at D = 20 and D = 100.

  sample   ghmc kernel.sample(200) against hmc kernel.sample(200) with L = 1 at the same shape (diagonal Gaussian), in the
           same process, alternating; the HMC figure is measured twice (hmc, hmc_again) to give the spread
  run      meads.run per step (--steps of them in one engine call)
  profile  one meads.run of --steps steps and nothing else: the process to put under `rocprofv3 --kernel-trace --stats`
           for the split between the transition, the two rank-C products and the small kernels
usage: meads_time.py [sample] [run] [profile] [--chains C] [--steps N]
Times are host wall-clock around a synchronised region of back-to-back calls: one warm-up region each, then 5 repeats
with the things compared taken in turn; the median, divided by the calls of a region."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from aehmc_amd import RandomStream, ghmc, hmc, meads, targets  # noqa: E402


def timed(fns, calls, repeats=5):
    """``fns``: name -> callable, timed ALTERNATELY so that whatever else the host does falls on all of them alike.
    Returns name -> (median, min, max) seconds per call."""
    def region(name):
        for _ in range(calls):
            fns[name]()
        torch.cuda.synchronize()
    out = {name: [] for name in fns}
    for name in fns:
        region(name)
    for _ in range(repeats):
        for name in fns:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            region(name)
            out[name].append((time.perf_counter() - t0) / calls)
    return {name: (statistics.median(v), min(v), max(v)) for name, v in out.items()}


def setup(C, D):
    sigma = np.linspace(1.0, 3.0, D)
    tgt = targets.DiagGaussian(np.zeros(D), sigma)
    q0 = torch.as_tensor(np.random.default_rng(0).normal(size=(C, D)) * sigma, device="cuda")
    return tgt, q0, torch.as_tensor(sigma, device="cuda")


def part_sample(C, D, n=200, calls=40):
    tgt, q0, scale = setup(C, D)
    gk = ghmc.new_kernel(RandomStream(seeds=list(range(C))), tgt)
    gs = ghmc.new_state(q0.clone(), tgt)
    hk = hmc.new_kernel(RandomStream(seeds=list(range(C))), tgt)
    hs = hmc.new_state(q0.clone(), tgt)
    imm = scale * scale
    res = timed({"hmc": lambda: hk.sample(hs, 0.3, imm, 1, n, keep_samples=False),
                 "ghmc": lambda: gk.sample(gs, 0.3, scale, 0.6, 0.3, n, keep_samples=False),
                 "hmc_again": lambda: hk.sample(hs, 0.3, imm, 1, n, keep_samples=False)}, calls)
    for what, (med, lo, hi) in res.items():
        print(json.dumps(dict(part="sample", what=what, C=C, D=D, transitions=n, ms=med * 1e3, ms_min=lo * 1e3,
                              ms_max=hi * 1e3, us_per_transition=med * 1e6 / n)), flush=True)
    h = [res["hmc"][0], res["hmc_again"][0]]
    print(json.dumps(dict(part="sample", C=C, D=D, ghmc_over_hmc=res["ghmc"][0] / statistics.mean(h),
                          hmc_spread=abs(h[0] - h[1]) / statistics.mean(h))), flush=True)


def part_run(C, D, steps, calls=3):
    tgt, q0, _ = setup(C, D)
    kernel = ghmc.new_kernel(RandomStream(seeds=list(range(C))), tgt)
    state = ghmc.new_state(q0.clone(), tgt)
    res = timed({"meads_run": lambda: meads.run(kernel, state, steps)}, calls)
    med, lo, hi = res["meads_run"]
    _, (eps, _, alpha, delta), _ = meads.run(kernel, state, steps)
    print(json.dumps(dict(part="run", C=C, D=D, steps=steps, ms=med * 1e3, ms_min=lo * 1e3, ms_max=hi * 1e3,
                          us_per_step=med * 1e6 / steps, step_size=eps, alpha=alpha, delta=delta)), flush=True)


def part_profile(C, D, steps):
    tgt, q0, _ = setup(C, D)
    kernel = ghmc.new_kernel(RandomStream(seeds=list(range(C))), tgt)
    meads.run(kernel, ghmc.new_state(q0.clone(), tgt), steps)
    torch.cuda.synchronize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("parts", nargs="*", default=["sample", "run"])
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--dims", type=int, nargs="*", default=[20, 100])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("meads_time.py measures on the GPU: no device found")
    for D in args.dims:
        if "sample" in args.parts:
            part_sample(args.chains, D)
        if "run" in args.parts:
            part_run(args.chains, D, args.steps)
        if "profile" in args.parts:
            part_profile(args.chains, D, args.steps)
