"""numpy restatement of the streaming quantile sketch of include/aehmc_hip.h ("streaming quantiles: a histogram sketch"),
written from its definition.  Imports nothing from aehmc_amd.

x is [R, D] (pooled draws, coordinate).  Coordinate d has B bins between lo[d] and hi[d]:
  width = (hi - lo) / B, inv = 1 / width (fp64, computed once);
  t = (x - lo) * inv (two rounded operations); slot = B + 2 if t is NaN, 0 if t < 0, B + 1 if t >= B, else 1 + trunc(t).
Counters [D, B + 3]: slot 0 below, 1 ... B interior, B + 1 above, B + 2 NaN.
Quantile at p over R = all counted draws: h = p (R - 1), k = floor(h), g = h - k, k1 = min(k + 1, R - 1); rank r lies in
the slot j with cum[j-1] <= r < cum[j] (cum over slots 0 ... B + 1) at
  pos(r) = lo + width * ((j - 1) + (r - cum[j-1] + 0.5) / count[j]),
estimate = pos(k) + g * (pos(k1) - pos(k)); resolved: both slots interior and no NaN counted; a coordinate with a NaN is
NaN."""
import numpy as np

import quantile_ref as qr


def widths(lo, hi, B):
    """(width, inv): the two arrays the kernels are handed."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    width = (hi - lo) / np.float64(B)
    with np.errstate(divide="ignore"):
        return width, np.float64(1.0) / width


def fit_grid(x, span=8.0):
    """(lo, hi) [D]: the default grid from the exact quartiles of x [R, D]."""
    q = qr.quantiles(x, (0.25, 0.5, 0.75))
    with np.errstate(invalid="ignore"):
        scale = (q[2] - q[0]) / np.float64(1.349)
    scale = np.where(np.isfinite(scale) & (scale != 0.0), scale, 1.0)
    reach = np.float64(span) * scale
    return q[1] - reach, q[1] + reach


def slots(x, lo, hi, B):
    """The slot of every entry of x [..., D] (int64)."""
    x = np.asarray(x, dtype=np.float64)
    _, inv = widths(lo, hi, B)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (x - lo) * inv
        inner = np.where(np.isnan(t) | (t < 0) | (t >= B), 0.0, t)
    out = 1 + np.trunc(inner).astype(np.int64)
    out = np.where(t >= B, B + 1, out)
    out = np.where(t < 0, 0, out)
    return np.where(np.isnan(t), B + 2, out)


def counts(x, lo, hi, B):
    """[D, B + 3] int64 from x [R, D]."""
    s = slots(x, lo, hi, B)
    return np.stack([np.bincount(s[:, d], minlength=B + 3) for d in range(s.shape[1])]).astype(np.int64)


def locate(cnt, r, B):
    """The slot j of 0 ... B + 1 with cum[j-1] <= r < cum[j] in one coordinate's counters, and cum[j-1]; (None, None)
    when no slot holds the rank (NaN draws are part of the total)."""
    cum = np.cumsum(cnt[:B + 2])
    j = int(np.searchsorted(cum, r, side="right"))
    if j > B + 1:
        return None, None
    return j, int(cum[j - 1]) if j else 0


def quantiles(cnt, lo, hi, B, probs):
    """(estimate [Q, D], resolved [Q, D] bool, slot of rank k [Q, D]) from counters cnt [D, B + 3]."""
    cnt = np.asarray(cnt, dtype=np.int64)
    D = cnt.shape[0]
    lo, hi = np.broadcast_to(np.asarray(lo, dtype=np.float64), (D,)), np.broadcast_to(np.asarray(hi, dtype=np.float64), (D,))
    width, _ = widths(lo, hi, B)
    R = int(cnt[0].sum())
    est = np.full((len(probs), D), np.nan)
    res = np.zeros((len(probs), D), dtype=bool)
    slot_k = np.full((len(probs), D), -1, dtype=np.int64)
    for i, p in enumerate(probs):
        h = np.float64(p) * np.float64(R - 1)
        k = int(np.floor(h))
        g = h - np.floor(h)
        k1 = min(k + 1, R - 1)
        for d in range(D):
            pos, inner = [], []
            for r in (k, k1):
                j, below = locate(cnt[d], r, B)
                if j is None:
                    pos.append(np.float64(np.nan))
                    inner.append(False)
                    continue
                inside = (np.float64(r - below) + 0.5) / np.float64(cnt[d, j])
                pos.append(lo[d] + width[d] * (np.float64(j - 1) + inside))
                inner.append(1 <= j <= B)
                if r == k:
                    slot_k[i, d] = j
            if cnt[d, B + 2] == 0:
                with np.errstate(invalid="ignore", over="ignore"):
                    est[i, d] = pos[0] + g * (pos[1] - pos[0])
                res[i, d] = inner[0] and inner[1]
    return est, res, slot_k


# the cases of tests/test_sketch_host.py and tests/test_gpu_sketch.py: what holds on the GPU is first pinned on the CPU
# (N, C, D): R = N C in {1, 15, 1961, 129, 16384}; D = 17 and 65 straddle tiles of 16 (8) coordinates, D = 1 with 16384
# rows splits the rows over several workgroups
SHAPES = [(1, 1, 1), (5, 3, 2), (37, 53, 17), (129, 1, 65), (4, 4096, 1)]
BINS = (64, 2048, 4096)  # the tile is 8 coordinates wide at 4096
PROBS = (0.0, 0.05, 0.25, 1.0 / 3.0, 0.5, 0.95, 1.0)
_draws = {}


def draws(N, C, D):
    """x [N C, D]: normal draws with a location and a scale per coordinate (the generator of
    tests/test_gpu_quantiles.py::draws); never written to."""
    if (N, C, D) not in _draws:
        r = np.random.default_rng(9000 + N + C + D)
        x = r.normal(size=(N * C, D)) * (0.5 + r.random(D)) + r.normal(size=D) * 3.0
        x.setflags(write=False)
        _draws[(N, C, D)] = x
    return _draws[(N, C, D)]
