#!/usr/bin/env python3
"""The pointwise log-likelihood kernel and the streaming WAIC fold beside what a user wrote before.

The README regression at `loo`'s documented shape: 4096 chains x 100 draws x 1000 observations (a 3.3 GB array).
  a   loglik(samples) -- transforms.Model.pointwise, one kernel behind the constraining map -- against the torch
      expression on model.unravel(model.constrain(samples)): time and torch.cuda.max_memory_allocated of each
  b   WaicAccumulator.update(draws), the log-likelihood never stored, against update_log_lik(loglik(draws))
  c   bytes/s of (a): the array written plus the positions read, over the call's time, against HBM's rate
usage: pointwise_time.py [--chains C] [--draws N] [--obs M] [--repeats K]
Times are device events on the current stream around the call, after one warm-up call of the same shape (which also
compiles the program); the median of the repeats, with the smallest and the largest.  The clocks the device reports
are printed first."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from aehmc_amd import summary, transforms as tf  # noqa: E402

HBM_PEAK, HBM_ACHIEVABLE = 8.0e12, 6.3e12  # bytes/s: the data sheet's rate and what a streaming kernel reaches


def timed(fn, repeats):
    fn()  # warm-up: code objects, allocator
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--draws", type=int, default=100)
    ap.add_argument("--obs", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    C, N, M = a.chains, a.draws, a.obs
    try:
        clocks = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        print("\n".join(line for line in clocks.splitlines() if "clk" in line.lower())[:2000], flush=True)
    except (OSError, subprocess.SubprocessError):
        print("clocks: not available", flush=True)
    r = np.random.default_rng(0)
    X = r.normal(size=(M, 5))
    y = X @ r.normal(size=5) + 0.7 * r.normal(size=M)
    model = tf.Model({"w": tf.Real(5), "sigma": tf.Positive()},
                     lambda w, sigma: np.sum(-0.5 * ((y - X @ w) / sigma) ** 2 - np.log(sigma)) - 0.5 * np.sum(w * w) - sigma)
    loglik = model.pointwise(lambda w, sigma: -0.5 * ((y - X @ w) / sigma) ** 2 - np.log(sigma) - 0.5 * np.log(2 * np.pi))
    samples = torch.as_tensor(np.concatenate([0.3 * r.normal(size=(N, C, 5)), -0.3 + 0.1 * r.normal(size=(N, C, 1))], axis=2),
                              device="cuda")
    Xd, yd = torch.as_tensor(X, device="cuda"), torch.as_tensor(y, device="cuda")

    def as_torch():
        un = model.unravel(model.constrain(samples))
        sigma = un["sigma"][..., None]
        return -0.5 * ((yd - un["w"] @ Xd.T) / sigma) ** 2 - torch.log(sigma) - 0.5 * np.log(2 * np.pi)

    out_bytes, in_bytes = N * C * M * 8, N * C * model.dim * 8
    res = dict(shape=dict(chains=C, draws=N, observations=M, array_GB=out_bytes / 1e9))
    diff = (loglik(samples) - as_torch()).abs().max().item()
    res["max_abs_difference_kernel_torch"] = diff
    for name, fn in (("kernel", lambda: loglik(samples)), ("torch", as_torch)):
        med, lo, hi = timed(fn, a.repeats)
        res[f"a_{name}"] = dict(ms=med, ms_min=lo, ms_max=hi, peak_GB=peak_bytes(fn) / 1e9)
    k = res["a_kernel"]
    rate = (out_bytes + in_bytes) / (k["ms"] * 1e-3)
    res["c_kernel_bytes_per_s"] = dict(TB_per_s=rate / 1e12, of_hbm_peak=rate / HBM_PEAK, of_hbm_achievable=rate / HBM_ACHIEVABLE)

    def fused():
        return summary.WaicAccumulator(loglik).update(samples)

    def stored():
        return summary.WaicAccumulator(loglik).update_log_lik(loglik(samples))

    same = torch.equal(fused().state, stored().state)
    for name, fn in (("fused", fused), ("stored", stored)):
        med, lo, hi = timed(fn, a.repeats)
        res[f"b_{name}"] = dict(ms=med, ms_min=lo, ms_max=hi, peak_GB=peak_bytes(fn) / 1e9)
    res["b_states_bit_equal"] = same
    print(json.dumps(res, indent=1), flush=True)


if __name__ == "__main__":
    main()
