#!/usr/bin/env python3
"""What the ChEES warm-up costs and what it buys.

  a        aehmc_chees_update (diagonal metric) against aehmc_pooled_adapt_update (slow stage, diagonal metric) and
           against one HMC transition of the same shape (diagonal Gaussian, L = 32): 4096 x 100 (the c2 shape) and
           4096 x 10^4.  The update reads [C, D] five times (5 C D 8 bytes), the pooled one twice.
  b        sigma = linspace(1, 10, 20) Gaussian, 4096 chains: metric from window_adaptation.run(pooled=True), then
           chees.run + chees.sample against NUTS with the same metric adaptation; min-coordinate ESS per second of sampling
usage: chees_time.py [a] [b] [--chains C]
Times are host wall-clock around a synchronised region of back-to-back calls that lasts about half a second: one warm-up
region each, then 5 repeats with the things compared taken in turn; the median, divided by the calls of a region."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from aehmc_amd import RandomStream, chees, hmc, nuts, summary, targets, window_adaptation  # noqa: E402
from aehmc_amd.engine import get_engine  # noqa: E402


def timed(fns, calls, repeats=5):
    """``fns``: name -> callable, timed ALTERNATELY (a, b, ..., a, b, ...) so that whatever else the host does falls on
    all of them alike.  A region is ``calls[name]`` back-to-back calls ending in a synchronise, sized to last about half
    a second.  Returns name -> (median, min, max) seconds per call."""
    def region(name):
        fn = fns[name]
        for _ in range(calls[name]):
            fn()
        torch.cuda.synchronize()
    out = {name: [] for name in fns}
    for name in fns:
        region(name)
    for _ in range(repeats):
        for name in fns:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            region(name)
            out[name].append((time.perf_counter() - t0) / calls[name])
    return {name: (statistics.median(v), min(v), max(v)) for name, v in out.items()}


def part_a(C, D, calls):
    eng = get_engine()
    r = np.random.default_rng(0)
    q0 = torch.as_tensor(r.normal(size=(C, D)), device="cuda")
    q1 = q0 + 0.1 * torch.as_tensor(r.normal(size=(C, D)), device="cuda")
    mom = torch.as_tensor(r.normal(size=(C, D)), device="cuda")
    imm = torch.ones(D, dtype=torch.float64, device="cuda")
    a = torch.full((C,), 0.7, dtype=torch.float64, device="cuda")
    acc = torch.ones(C, dtype=torch.int32, device="cuda")
    st, cst = eng.chees_alloc(C)
    eng.chees_init(C, 1.0, 1.0, cst)
    pst, pcst = eng.pooled_adapt_alloc(C, D, False)
    eng.pooled_adapt_init(C, D, 1.0, pcst)
    tgt = targets.DiagGaussian(np.zeros(D), np.ones(D))
    kernel = hmc.new_kernel(RandomStream(seeds=list(range(C))), tgt)
    box = [hmc.new_state(q0.clone(), tgt)]

    def step():
        info, _ = kernel(box[0], 0.05, imm, 32)
        box[0] = info.state._replace(momentum=None)
    res = timed({"chees_update": lambda: eng.chees_update(C, D, 0, 0.651, 0.025, 1000, q0, q1, mom, imm, 0.0, acc, a, cst),
                 "pooled_adapt_update": lambda: eng.pooled_adapt_update(C, D, 1, 0, 0, 0.8, a, q1, pcst),
                 "hmc_transition_L32": step}, calls)
    for what, (med, lo, hi) in res.items():
        extra = {}
        if what == "chees_update":
            extra = dict(bytes_read=5 * C * D * 8, read_GBps=5 * C * D * 8 / med / 1e9)
        elif what == "pooled_adapt_update":
            extra = dict(bytes_read=2 * C * D * 8, read_GBps=2 * C * D * 8 / med / 1e9)
        print(json.dumps(dict(part="a", what=what, C=C, D=D, calls_per_region=calls[what], us=med * 1e6, us_min=lo * 1e6,
                              us_max=hi * 1e6, **extra)), flush=True)
    print(json.dumps(dict(part="a", C=C, D=D, chees_over_pooled=res["chees_update"][0] / res["pooled_adapt_update"][0],
                          chees_over_transition=res["chees_update"][0] / res["hmc_transition_L32"][0])), flush=True)


def part_b(C, num_warmup=400, num_samples=500):
    sigma = np.linspace(1.0, 10.0, 20)
    tgt = targets.DiagGaussian(np.zeros(20), sigma)
    q0 = torch.as_tensor(np.random.default_rng(0).normal(size=(C, 20)), device="cuda")

    def report(name, draws, seconds, info, **extra):
        s = summary.summarize(draws, max_lag=100)
        print(json.dumps(dict(part="b", sampler=name, chains=C, draws=num_samples, sample_s=seconds,
                              ess_min=float(s.ess.min()), ess_min_per_s=float(s.ess.min()) / seconds,
                              rhat_max=float(s.rhat.max()), **extra)), flush=True)

    kernel = hmc.new_kernel(RandomStream(seeds=list(range(C))), tgt)
    state = hmc.new_state(q0.clone(), tgt)
    t0 = time.perf_counter()
    state, (eps0, imm), _ = window_adaptation.run(kernel, state, num_warmup, pooled=True, num_integration_steps=8)
    state, (eps, imm, T), _ = chees.run(kernel, state, num_warmup, imm)
    torch.cuda.synchronize()
    warm = time.perf_counter() - t0
    chees.sample(kernel, state, eps, imm, T, 16)  # (first use of every length's route)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    draws, info, acc, _ = chees.sample(kernel, state, eps, imm, T, num_samples, first=17)
    torch.cuda.synchronize()
    report("chees", draws, time.perf_counter() - t0, info, warmup_s=warm, step_size=eps, trajectory_length=T,
           mean_accept=float(acc.mean()),
           leapfrogs_per_chain=sum(chees.num_integration_steps(eps, T, 17 + i) for i in range(num_samples)))
    del draws
    kernel = nuts.new_kernel(RandomStream(seeds=list(range(C))), tgt)
    state = nuts.new_state(q0.clone(), tgt)
    t0 = time.perf_counter()
    state, (eps, imm), _ = window_adaptation.run(kernel, state, 2 * num_warmup, pooled=True)
    torch.cuda.synchronize()
    warm = time.perf_counter() - t0
    kernel.sample(state, eps, imm, 16)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    draws, info, acc, _ = kernel.sample(state, eps, imm, num_samples)
    torch.cuda.synchronize()
    report("nuts", draws, time.perf_counter() - t0, info, warmup_s=warm, step_size=eps, mean_accept=float(acc.mean()))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("parts", nargs="*", default=["a", "b"])
    ap.add_argument("--chains", type=int, default=4096)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("chees_time.py measures on the GPU: no device found")
    if "a" in args.parts:
        part_a(args.chains, 100, dict(chees_update=10000, pooled_adapt_update=10000, hmc_transition_L32=6000))
        part_a(args.chains, 10000, dict(chees_update=1200, pooled_adapt_update=3000, hmc_transition_L32=200))
    if "b" in args.parts:
        part_b(args.chains)
