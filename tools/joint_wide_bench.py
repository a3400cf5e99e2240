#!/usr/bin/env python3
"""Throughput of a traced joint density above 2048 coordinates (Neal's funnel as a Python function): NUTS sample(N) and
HMC (L = 32) sample(N) on the workgroup-per-chain kernels compiled against the traced program (engine option
"joint_wide" 1, the default), or on the lock-step path ("joint_wide" 0: the density evaluated a workgroup per live chain
between the stage kernels).  Leapfrogs per second, device-synchronised, after a warm-up call (which also compiles).
usage: python tools/joint_wide_bench.py [--dims 4096,10000] [--chains 4096] [--nuts-samples 100] [--hmc-samples 20]
                                        [--max-exp 6] [--joint-wide 1] [--only nuts|hmc] [--json out.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aehmc_amd import RandomStream, hmc, nuts, targets  # noqa: E402
from aehmc_amd.engine import get_engine  # noqa: E402


def funnel(q):
    v, x = q[0], q[1:]
    return -v * v / 18.0 + (-0.5 * x * x * np.exp(-v) - 0.5 * v).sum()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="4096,10000")
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--nuts-samples", type=int, default=100)
    ap.add_argument("--hmc-samples", type=int, default=20)
    ap.add_argument("--max-exp", type=int, default=6)
    ap.add_argument("--joint-wide", type=int, default=1)
    ap.add_argument("--only", choices=("nuts", "hmc"), default=None)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    eng = get_engine()
    eng.set_option("joint_wide", args.joint_wide)
    C, rows = args.chains, []
    for D in (int(d) for d in args.dims.split(",")):
        tgt = targets.from_callable(funnel, D)
        r = np.random.default_rng(D)
        q0 = torch.as_tensor(r.standard_normal((C, D)), device="cuda")
        q0[:, 0] = 0.0  # (v = 0: every x_i ~ N(0, 1) there)
        imm = torch.ones(D, dtype=torch.float64, device="cuda")
        imm[0] = 2.0 / D  # (given x, v has a standard deviation of about sqrt(2 / D): its scale in the metric)
        eps = 0.5 * D ** -0.25
        for sampler in ("nuts", "hmc"):
            if args.only and sampler != args.only:
                continue
            if sampler == "nuts":
                kern = nuts.new_kernel(RandomStream(seeds=list(range(C))), tgt, max_num_expansions=args.max_exp)
                state = nuts.new_state(q0, tgt)
                run = lambda s, n: kern.sample(s, eps, imm, n, keep_samples=False)  # noqa: E731
                n = args.nuts_samples
            else:
                kern = hmc.new_kernel(RandomStream(seeds=list(range(C))), tgt)
                state = hmc.new_state(q0, tgt)
                run = lambda s, n: kern.sample(s, eps, imm, 32, n, keep_samples=False)  # noqa: E731
                n = args.hmc_samples
            _, info, _, _ = run(state, 2)  # warm-up (compiles the program)
            state = info.state._replace(momentum=None)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, info, acc, div = run(state, n)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            nleap = int(info.n_leapfrog.sum().item()) if sampler == "nuts" else C * n * 32
            row = dict(sampler=sampler, D=D, C=C, samples=n, joint_wide=args.joint_wide, eps=eps, seconds=dt,
                       leapfrogs=nleap, leapfrog_per_s=nleap / dt, acc_mean=float(acc.float().mean().item()),
                       divergent=int(div.sum().item()))
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
