#!/usr/bin/env python3
"""Pooled against per-chain window adaptation, and the rank-C update against the GEMM.

  a        dense MVN, D = 200, 4096 chains, NUTS: run(300, is_mass_matrix_full=True) + sample(100), per chain and pooled
  b        the c3 shape, D = 10^4, 4096 chains: one slow-window pooled update against a transition of the same run;
           aehmc_syrk_tn (C D^2 useful flops) and aehmc_gemm_nt at M = N = 10^4, K = 4096 in the same session
usage: pooled_adapt_time.py [a] [b] [--chains C] [--dim-b D]
Times are host wall-clock around a synchronised region: one warm-up call first, then the median of the repeats."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from aehmc_amd import RandomStream, nuts, targets, window_adaptation  # noqa: E402
from aehmc_amd.engine import get_engine  # noqa: E402


def timed(fn, repeats=5):
    fn()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return statistics.median(out), min(out), max(out)


def part_a(C):
    D = 200
    r = np.random.default_rng(0)
    B = r.normal(size=(D, D)) / np.sqrt(D)
    cov = B @ B.T + 0.5 * np.eye(D)
    prec = np.linalg.inv(cov)
    tgt = targets.DenseMVN(np.zeros(D), 0.5 * (prec + prec.T))
    q0 = torch.as_tensor(r.normal(size=(C, D)), device="cuda")
    for pooled in (False, True):
        kernel = nuts.new_kernel(RandomStream(seeds=list(range(C))), tgt)
        state = nuts.new_state(q0.clone(), tgt)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        state, (eps, imm), _ = window_adaptation.run(kernel, state, 300, is_mass_matrix_full=True, pooled=pooled)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        kernel.sample(state, eps, imm, 5, keep_samples=False)  # (first use of the sampling route)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        _, info, acc, div = kernel.sample(state, eps, imm, 100, keep_samples=False)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        print(json.dumps(dict(part="a", pooled=pooled, D=D, chains=C, warmup_300_s=t1 - t0, sample_100_s=t3 - t2,
                              ms_per_transition=(t3 - t2) * 10, leapfrogs=int(info.n_leapfrog.sum().item()),
                              mean_accept=float(acc.mean().item()), divergences=int(div.sum().item()))), flush=True)


def part_b(C, D):
    eng = get_engine()
    r = np.random.default_rng(1)
    X = torch.as_tensor(r.normal(size=(C, D)), device="cuda")
    S = torch.zeros(D, D, dtype=torch.float64, device="cuda")
    b = X.mean(0)
    med, lo, hi = timed(lambda: eng.syrk_tn(X, S, b, 0.5, b))
    print(json.dumps(dict(part="b", what="aehmc_syrk_tn", C=C, D=D, s=med, s_min=lo, s_max=hi,
                          useful_tflops=C * D * D / med / 1e12)), flush=True)
    A = torch.as_tensor(r.normal(size=(D, C)), device="cuda")
    med, lo, hi = timed(lambda: eng.gemm_nt(A, A))
    print(json.dumps(dict(part="b", what="aehmc_gemm_nt M=N=D K=C", C=C, D=D, s=med, s_min=lo, s_max=hi,
                          tflops=2 * C * D * D / med / 1e12)), flush=True)
    del A
    st, cst = eng.pooled_adapt_alloc(C, D, True)
    eng.pooled_adapt_init(C, D, 1.0, cst)
    a = torch.full((C,), 0.8, dtype=torch.float64, device="cuda")
    med, lo, hi = timed(lambda: eng.pooled_adapt_update(C, D, 1, 0, 0, 0.8, a, X, cst))
    print(json.dumps(dict(part="b", what="pooled update, slow window", C=C, D=D, s=med, s_min=lo, s_max=hi)), flush=True)
    # a transition of the c3 kind: dense-precision target under a dense metric (whitened lock-step NUTS)
    idx = torch.arange(D, device="cuda")
    prec = torch.zeros(D, D, dtype=torch.float64, device="cuda")
    prec[idx, idx] = 1.0 + torch.rand(D, dtype=torch.float64, device="cuda")
    prec[idx[:-1], idx[1:]] = 0.2
    prec[idx[1:], idx[:-1]] = 0.2
    tgt = targets.DenseMVN(torch.zeros(D, dtype=torch.float64, device="cuda"), prec)
    imm = torch.eye(D, dtype=torch.float64, device="cuda")
    kernel = nuts.new_kernel(RandomStream(seeds=list(range(C))), tgt, max_num_expansions=5)
    state = nuts.new_state(X.clone(), tgt)
    box = [state]

    def step():
        info, _ = kernel(box[0], 0.2, imm)
        box[0] = info.state._replace(momentum=None)

    med, lo, hi = timed(step, repeats=3)
    print(json.dumps(dict(part="b", what="NUTS transition (max 5 expansions)", C=C, D=D, s=med, s_min=lo, s_max=hi)),
          flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("parts", nargs="*", default=["a", "b"])
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--dim-b", type=int, default=10000)
    args = ap.parse_args()
    if "a" in args.parts:
        part_a(args.chains)
    if "b" in args.parts:
        part_b(args.chains, args.dim_b)
