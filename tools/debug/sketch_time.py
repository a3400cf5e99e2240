#!/usr/bin/env python3
"""The streaming quantile sketch beside the streaming moments, and beside the sampling of the chunk it folds (DESIGN.md
section 4).

  a   4096 chains x 10^4 coordinates, 3 draws: the default chunk of summary.run at the headline shape
  b   4096 chains x 100 coordinates, 500 draws; also one kernel.sample chunk of that size (NUTS and HMC L = 32 on a
      diagonal Gaussian under a diagonal metric) beside its sketch fold
usage: sketch_time.py [a] [b] [--bins B ...] [--repeats K]
Both folds read the same buffer once: aehmc_summary_sketch_update against aehmc_summary_update (split chains, the call of
summary.run).  Times are HIP events around one call, after two warm-up calls of each; the two are timed alternately and
the median, minimum and maximum of the repeats are reported.  Bandwidth = T C D 8 bytes / time (the counters are small
beside the draws)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from aehmc_amd import RandomStream, hmc, nuts, summary, targets  # noqa: E402


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return dict(ms=statistics.median(ms), ms_min=min(ms), ms_max=max(ms))


def folds(part, x, bins, repeats):
    """x [T, C, D]: the sketch fold at every grid size against the moments fold of the same buffer."""
    T, C, D = x.shape
    nbytes = x.numel() * 8
    acc = summary.Accumulator(1 << 20, C, (D,))  # (a long run: every call folds draws 0 ... T - 1 of its first half)
    eng = acc._eng

    def moments():
        eng.summary_update(x, 0, acc.num_draws, 2, acc.mean, acc.m2)

    for B in bins:
        sk = summary.QuantileSketch(C, (D,), bins=B).fit(x[:1])

        def sketch():
            eng.summary_sketch_update(x, B, sk._lo, sk._inv, sk.counts)

        for _ in range(2):
            moments()
            sketch()
        t_m, t_s = [], []
        for _ in range(repeats):
            t_m.append(event_ms(moments))
            t_s.append(event_ms(sketch))
        m, s = stats(t_m), stats(t_s)
        below, above = int(sk.counts[:, 0].sum().item()), int(sk.counts[:, B + 1].sum().item())
        print(json.dumps(dict(part=part, shape=[T, C, D], bins=B, bytes=nbytes, moments=m, sketch=s,
                              sketch_over_moments=s["ms"] / m["ms"], moments_tb_per_s=nbytes / (m["ms"] * 1e-3) / 1e12,
                              sketch_tb_per_s=nbytes / (s["ms"] * 1e-3) / 1e12,
                              share_outside_grid=(below + above) / float(sk.counts.sum().item()))), flush=True)


def sampling(T, C, D, repeats):
    """One kernel.sample chunk into a reused buffer beside the sketch fold of that chunk."""
    g = torch.Generator(device="cuda").manual_seed(1)
    mu = torch.randn(D, dtype=torch.float64, device="cuda", generator=g) * 2.0
    sigma = 0.5 + torch.rand(D, dtype=torch.float64, device="cuda", generator=g)
    tgt = targets.DiagGaussian(mu, sigma)
    q0 = mu + sigma * torch.randn(C, D, dtype=torch.float64, device="cuda", generator=g)
    buf = torch.empty(T * C * D, dtype=torch.float64, device="cuda")
    for name, mod, extra in (("nuts", nuts, ()), ("hmc L=32", hmc, (32,))):
        kernel = mod.new_kernel(RandomStream(seeds=list(range(C))), tgt)
        box = [mod.new_state(q0.clone(), tgt)]
        sk = summary.QuantileSketch(C, (D,))
        last = []

        def sample():
            samples, info, _, _ = kernel.sample(box[0], 0.3, sigma**2, *extra, T, into=buf)
            box[0] = info.state._replace(momentum=None)
            last[:] = [samples.reshape(T, C, D)]

        def fold():
            sk.update(last[0])

        sample()
        fold()
        t_k, t_s = [], []
        for _ in range(repeats):
            t_k.append(event_ms(sample))
            t_s.append(event_ms(fold))
        k, s = stats(t_k), stats(t_s)
        print(json.dumps(dict(part="b", what=f"kernel.sample chunk ({name}) and its sketch fold", shape=[T, C, D],
                              bins=sk.bins, sample=k, sketch=s, sketch_share_of_sampling=s["ms"] / k["ms"],
                              resolved_at_0p05_0p95=bool(sk.resolved((0.05, 0.95)).all().item()))), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("parts", nargs="*", default=["a", "b"])
    ap.add_argument("--bins", type=int, nargs="+", default=[64, 2048, 4096])
    ap.add_argument("--repeats", type=int, default=9)
    args = ap.parse_args()
    g = torch.Generator(device="cuda").manual_seed(0)
    for part, (T, C, D) in (("a", (3, 4096, 10_000)), ("b", (500, 4096, 100))):
        if part not in args.parts:
            continue
        x = torch.randn(T, C, D, dtype=torch.float64, device="cuda", generator=g)
        x = x * (0.5 + torch.rand(D, dtype=torch.float64, device="cuda", generator=g)) + 3.0
        folds(part, x, args.bins, args.repeats)
        del x
        if part == "b":
            sampling(T, C, D, max(3, args.repeats // 2))
