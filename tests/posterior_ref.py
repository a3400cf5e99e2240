"""numpy / scipy restatement of the highest-density interval, the MCSE of a quantile, the MCSE of the standard deviation
and the posterior table of include/aehmc_hip.h ("highest-density intervals and the MCSE of quantiles") and
aehmc_amd/summary.py, written from their definitions: ArviZ's unimodal hdi, posterior::mcse_quantile (ArviZ's
_mcse_quantile) and posterior::mcse_sd.  ESS and quantiles by tests/summary_ref.py and tests/quantile_ref.py, the
rank-normalised columns by tests/rank_ref.py, the beta quantile by scipy.special.betaincinv.  Imports nothing from
aehmc_amd."""
import os
import sys

import numpy as np
from scipy.special import betaincinv

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import quantile_ref as qr  # noqa: E402
import rank_ref as rr  # noqa: E402
import summary_ref as sr  # noqa: E402

P_LO, P_HI = 0.1586553, 0.8413447  # Phi(-1) and Phi(1) to the seven digits of posterior and ArviZ
DELTA = 1e-6                       # `unsure`: a scaled beta quantile this close to an integer


def hdi_width(R, prob):
    """m: the interval spans the order statistics i ... i + m (ArviZ's interval_idx_inc, held to R - 1)."""
    return min(int(np.floor(np.float64(prob) * np.float64(R))), R - 1)


def hdi(x, prob):
    """x [R, D] -> (lower [D], upper [D], index [D] int64): of the windows s[i + m] - s[i] of every sorted column the
    narrowest, the first of equally narrow ones.  Zeros of both signs are +0.0; a NaN width (inf - inf) counts as +inf;
    a column with a NaN gives NaN, NaN, -1."""
    x = np.asarray(x, dtype=np.float64)
    R, D = x.shape
    m = hdi_width(R, prob)
    s = np.sort(x + 0.0, axis=0)
    with np.errstate(invalid="ignore"):
        w = s[m:] - s[:R - m]
    w[np.isnan(w)] = np.inf
    idx = np.argmin(w, axis=0).astype(np.int64)  # (the first of the minima)
    cols = np.arange(D)
    lower, upper = s[idx, cols].copy(), s[idx + m, cols].copy()
    bad = np.isnan(x).any(axis=0)
    lower[bad] = upper[bad] = np.nan
    idx[bad] = -1
    return lower, upper, idx


def hdi_brute(x, prob):
    """The same by the definition, O(R^2): every pair of order statistics m apart is looked at, column by column."""
    x = np.asarray(x, dtype=np.float64)
    R, D = x.shape
    m = hdi_width(R, prob)
    lower, upper, idx = np.empty(D), np.empty(D), np.empty(D, dtype=np.int64)
    for d in range(D):
        s = sorted(float(v) + 0.0 for v in x[:, d])
        best, at = None, -1
        for i in range(R):
            for j in range(i, R):
                if j - i != m:
                    continue
                w = s[j] - s[i]
                if w != w:
                    w = float("inf")
                if best is None or w < best:
                    best, at = w, i
        lower[d], upper[d], idx[d] = s[at], s[at + m], at
    return lower, upper, idx


def mcse_quantile_from_ess(x, probs, ess):
    """x [S, D], ess [Q, D] -> (mcse [Q, D], ranks [2, Q, D] int64, unsure [Q, D]).  An ess that is NaN, infinite or
    <= 0, or a column with a NaN, gives NaN and ranks -1."""
    x = np.asarray(x, dtype=np.float64)
    S, D = x.shape
    s = np.sort(x + 0.0, axis=0)
    bad = np.isnan(x).any(axis=0)
    Q = len(probs)
    out = np.full((Q, D), np.nan)
    ranks = np.full((2, Q, D), -1, dtype=np.int64)
    unsure = np.zeros((Q, D), dtype=bool)
    for q, p in enumerate(probs):
        p = np.float64(p)
        for d in range(D):
            e = np.float64(ess[q][d])
            if not (np.isfinite(e) and e > 0) or bad[d]:
                continue
            a, b = e * p + 1.0, e * (1.0 - p) + 1.0
            a1, a2 = betaincinv(a, b, P_LO), betaincinv(a, b, P_HI)
            for v in (a1 * S, a2 * S):
                unsure[q, d] |= abs(v - np.rint(v)) < DELTA
            lo = int(max(np.floor(a1 * S), 1.0)) - 1
            hi = int(min(np.ceil(a2 * S), float(S))) - 1
            ranks[0, q, d], ranks[1, q, d] = lo, hi
            with np.errstate(invalid="ignore"):
                out[q, d] = (s[hi, d] - s[lo, d]) / 2.0
    return out, ranks, unsure


def indicator_ess(x, probs, max_lag=None):
    """x [N, C, D] -> (ess [Q, D], near [D]): the split-chain ESS of the indicators x <= quantile(x, p)."""
    x = np.asarray(x, dtype=np.float64)
    N, C, D = x.shape
    q = qr.quantiles(x.reshape(N * C, D), list(probs))
    ess, near = np.empty((len(probs), D)), np.zeros(D, dtype=bool)
    for i in range(len(probs)):
        with np.errstate(invalid="ignore"):
            res = sr.summarize((x <= q[i]).astype(np.float64), split=True, max_lag=max_lag)
        ess[i] = res["ess"]
        near |= res["near"]
    return ess, near


def mcse_quantile(x, probs, max_lag=None):
    """x [N, C, D] -> dict: mcse [Q, D], ranks [2, Q, D], ess [Q, D], unsure [D] (a1 S or a2 S within DELTA of an
    integer at some probability), near [D] (summary_ref.summarize's flag, of any indicator)."""
    x = np.asarray(x, dtype=np.float64)
    N, C, D = x.shape
    ess, near = indicator_ess(x, probs, max_lag)
    out, ranks, unsure = mcse_quantile_from_ess(x.reshape(N * C, D), probs, ess)
    return {"mcse": out, "ranks": ranks, "ess": ess, "unsure": unsure.any(axis=0), "near": near}


def mcse_sd(x, max_lag=None):
    """x [N, C, D] -> (mcse_sd [D], near [D]): posterior::mcse_sd."""
    x = np.asarray(x, dtype=np.float64)
    c = x - x.mean(axis=(0, 1))
    c2 = c * c
    res = sr.summarize(c2, split=True, max_lag=max_lag)
    evar = c2.mean(axis=(0, 1))
    varvar = ((c2 * c2).mean(axis=(0, 1)) - evar * evar) / res["ess"]
    return np.sqrt(varvar / evar / 4.0), res["near"]


def table(x, prob=0.9, max_lag=None):
    """x [N, C, D] -> dict of [D] arrays, the fields of summary.PosteriorTable, and `near` (any deciding pair sum of
    any of the estimators within 1e-9 of zero)."""
    x = np.asarray(x, dtype=np.float64)
    N, C, D = x.shape
    s = sr.summarize(x, max_lag=max_lag)
    r = rr.rank_summarize(x, max_lag=max_lag)
    lower, upper, _ = hdi(x.reshape(N * C, D), prob)
    msd, near_sd = mcse_sd(x, max_lag)
    return {"mean": s["mean"], "sd": s["sd"], "hdi_lower": lower, "hdi_upper": upper, "mcse_mean": s["mcse"],
            "mcse_sd": msd, "ess_bulk": r["ess_bulk"], "ess_tail": r["ess_tail"], "rhat": r["rhat"],
            "near": s["near"] | r["near"] | r["near_folded"] | r["near_tail"] | near_sd}
