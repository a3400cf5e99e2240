#!/usr/bin/env python3
"""The constraining map (aehmc_constrain, csrc/constrain.cuh) beside a torch expression of the same maps, and what
summary.run(constrain=model) adds to a chunk.

  a   rows [100 x 4096, 100]               (328 MB in)
  b   rows [3 x 4096, 10^4]                (983 MB in: one default chunk of summary.run at the headline shape)
      each for a coordinate-wise spec (Real, LowerBound, UpperBound, Interval in equal parts) and for a spec whose first
      half is blocks of Ordered(64) and Simplex(64)
  run summary.run with and without constrain= on one kernel (NUTS, 4096 chains, a coordinate-wise model of 100
      coordinates), the difference per chunk
usage: constrain_time.py [a] [b] [run] [--repeats K] [--limit SECONDS]
Times are HIP events around one call after two warm-up calls, kernel and torch alternately; median, minimum and maximum
of the repeats.  A step stops repeating once it has used --limit seconds.  Bandwidth = (R D_in + R D_out) 8 bytes / time:
one read and one write."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from aehmc_amd import RandomStream, nuts, summary  # noqa: E402
from aehmc_amd import transforms as tf  # noqa: E402


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return dict(ms=statistics.median(ms), ms_min=min(ms), ms_max=max(ms), n=len(ms))


def timed(fns, repeats, limit):
    """every function of `fns` in turn, `repeats` times or until `limit` seconds have passed"""
    for fn in fns:
        fn()
        fn()
    torch.cuda.synchronize()
    out, t0 = [[] for _ in fns], time.monotonic()
    for _ in range(repeats):
        for ms, fn in zip(out, fns):
            ms.append(event_ms(fn))
        if time.monotonic() - t0 > limit:
            break
    return [stats(ms) for ms in out]


def coordinate_wise(D):
    q = D // 4
    lo = np.linspace(-2.0, 2.0, q)
    return tf.Model({"r": tf.Real(D - 3 * q), "l": tf.LowerBound(lo, q), "u": tf.UpperBound(3.0, q),
                     "i": tf.Interval(lo, lo + 1.5, q)}, lambda **kw: 0.0)


def with_segments(D):
    spec, used, k = {}, 0, 0
    while used + 64 + 63 <= D // 2:
        spec[f"o{k}"], spec[f"s{k}"] = tf.Ordered(64), tf.Simplex(64)
        used, k = used + 127, k + 1
    if not spec:  # (a short row: one Ordered(64), and a Simplex over half of what is left)
        spec["o0"], spec["s0"] = tf.Ordered(64), tf.Simplex((D - 64) // 2 + 1)
        used = 64 + (D - 64) // 2
    rest = D - used
    spec["l"], spec["i"] = tf.LowerBound(0.5, rest // 2), tf.Interval(-1.0, 1.0, rest - rest // 2)
    return tf.Model(spec, lambda **kw: 0.0)


def torch_expression(model):
    """the same maps in torch: one indexed expression per coordinate-wise kind, a cumsum per Ordered block, a
    log_softmax per Simplex block, written into one output"""
    tab, dev = model.table, "cuda"
    idx = {k: (torch.as_tensor(np.flatnonzero(tab["kind"] == k), device=dev), torch.as_tensor(tab["first"][tab["kind"] == k], device=dev))
           for k in range(4)}
    lo, hi = torch.as_tensor(tab["lo"], device=dev), torch.as_tensor(tab["hi"], device=dev)
    segs = [(t.kind, model._in[name], model._out[name]) for name, t in model.spec.items() if t.kind >= 4]

    def fn(x, out):
        for k, (o, i) in idx.items():
            if not len(o):
                continue
            v = x[:, i]
            if k == 0:
                out[:, o] = v
            elif k == 1:
                out[:, o] = lo[o] + torch.exp(v)
            elif k == 2:
                out[:, o] = hi[o] - torch.exp(v)
            else:
                out[:, o] = lo[o] + (hi[o] - lo[o]) * torch.sigmoid(v)
        for k, s_in, s_out in segs:
            v = x[:, s_in]
            if k == 4:
                out[:, s_out] = torch.cat([v[:, :1], torch.exp(v[:, 1:])], dim=1).cumsum(dim=1)
            else:
                out[:, s_out] = torch.log_softmax(torch.cat([v, torch.zeros_like(v[:, :1])], dim=1), dim=1).exp()
        return out

    return fn


def maps(part, R, D, repeats, limit):
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(R, D, dtype=torch.float64, device="cuda", generator=g)
    for name, model in (("coordinate-wise", coordinate_wise(D)), ("Ordered(64) and Simplex(64) blocks", with_segments(D))):
        out = torch.empty(R, model.constrained_dim, dtype=torch.float64, device="cuda")
        ref = torch.empty_like(out)
        expr = torch_expression(model)
        nbytes = (x.numel() + out.numel()) * 8
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        model.constrain(x, out=out)
        peak_kernel = torch.cuda.max_memory_allocated() - base
        torch.cuda.reset_peak_memory_stats()
        expr(x, ref)
        peak_torch = torch.cuda.max_memory_allocated() - base
        k, t = timed([lambda: model.constrain(x, out=out), lambda: expr(x, ref)], repeats, limit)
        fin = torch.isfinite(ref)
        print(json.dumps(dict(part=part, spec=name, rows=R, d_in=D, d_out=model.constrained_dim, bytes=nbytes, kernel=k, torch=t,
                              kernel_gb_per_s=nbytes / (k["ms"] * 1e-3) / 1e9, torch_over_kernel=t["ms"] / k["ms"],
                              temporaries_kernel_bytes=peak_kernel, temporaries_torch_bytes=peak_torch,
                              max_abs_diff=float((out[fin] - ref[fin]).abs().max()))), flush=True)
        del out, ref


def run_overhead(repeats, limit):
    C, D, T, chunks = 4096, 100, 50, 4
    model = tf.Model({"s": tf.Positive(D)}, lambda s: np.sum(2.0 * np.log(s) - 2.0 * s))
    kernel = nuts.new_kernel(RandomStream(seeds=list(range(C))), model)
    g = torch.Generator(device="cuda").manual_seed(2)
    state = nuts.new_state(0.3 * torch.randn(C, D, dtype=torch.float64, device="cuda", generator=g), model)
    imm = np.ones(D)
    N = T * chunks

    def plain():
        summary.run(kernel, state, 0.4, imm, N, chunk=T)

    def constrained():
        summary.run(kernel, state, 0.4, imm, N, chunk=T, constrain=model)

    # (the two runs draw different transitions -- one kernel, one generator --; their lengths differ by the trees, so the
    # map is also timed alone on a chunk-sized buffer)
    p, c = timed([plain, constrained], repeats, limit)
    x = torch.randn(T * C, D, dtype=torch.float64, device="cuda", generator=g)
    out = torch.empty_like(x)
    m, = timed([lambda: model.constrain(x, out=out)], repeats, limit)
    print(json.dumps(dict(part="run", chains=C, d=D, draws=N, chunk=T, run=p, run_with_constrain=c,
                          extra_ms_per_chunk=(c["ms"] - p["ms"]) / chunks, map_alone_ms_per_chunk=m["ms"],
                          share_of_a_chunk=m["ms"] / (p["ms"] / chunks))), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("parts", nargs="*", default=["a", "b", "run"])
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--limit", type=float, default=60.0)
    args = ap.parse_args()
    for part, (R, D) in (("a", (100 * 4096, 100)), ("b", (3 * 4096, 10_000))):
        if part in args.parts:
            maps(part, R, D, args.repeats, args.limit)
    if "run" in args.parts:
        run_overhead(max(3, args.repeats // 2), args.limit)
