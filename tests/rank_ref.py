"""Reference pipeline of the rank-normalised diagnostics (Vehtari, Gelman, Simpson, Carpenter, Buerkner 2021): ranks by
scipy.stats.rankdata, normal scores by scipy.special.ndtri, folding about numpy's median, estimators by the numpy
restatement of tests/summary_ref.py and tests/quantile_ref.py.  Imports nothing from aehmc_amd.

Also `ndtri_as241`: a numpy restatement of the formula the device evaluates for Phi^-1 (Wichura's AS 241, PPND16,
without its far-tail branch), so that the formula and its coefficients can be checked without a GPU."""
import os
import sys

import numpy as np
from scipy.special import ndtri
from scipy.stats import rankdata

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import quantile_ref as qr  # noqa: E402
import summary_ref as sr  # noqa: E402

A = (3.3871328727963666080e0, 1.3314166789178437745e2, 1.9715909503065514427e3, 1.3731693765509461125e4,
     4.5921953931549871457e4, 6.7265770927008700853e4, 3.3430575583588128105e4, 2.5090809287301226727e3)
B = (1.0, 4.2313330701600911252e1, 6.8718700749205790830e2, 5.3941960214247511077e3, 2.1213794301586595867e4,
     3.9307895800092710610e4, 2.8729085735721942674e4, 5.2264952788528545610e3)
C = (1.42343711074968357734e0, 4.63033784615654529590e0, 5.76949722146069140550e0, 3.64784832476320460504e0,
     1.27045825245236838258e0, 2.41780725177450611770e-1, 2.27238449892691845833e-2, 7.74545014278341407640e-4)
D = (1.0, 2.05319162663775882187e0, 1.67638483018380384940e0, 6.89767334985100004550e-1, 1.48103976427480074590e-1,
     1.51986665636164571966e-2, 5.47593808499534494600e-4, 1.05075007164441684324e-9)


def _horner(coef, r):
    out = np.full_like(r, coef[-1])
    for c in coef[-2::-1]:
        out = out * r + c
    return out


def ndtri_as241(p):
    """Phi^-1(p) for p with sqrt(-log(min(p, 1 - p))) <= 5 (p >= 1.4e-11): the device's formula, operation by
    operation."""
    p = np.asarray(p, dtype=np.float64)
    q = p - 0.5
    out = np.empty_like(p)
    mid = np.abs(q) <= 0.425
    r = 0.180625 - q[mid] * q[mid]
    out[mid] = q[mid] * _horner(A, r) / _horner(B, r)
    t = ~mid
    r = np.sqrt(-np.log(np.where(q[t] < 0.0, p[t], 0.5 - q[t])))
    assert np.all(r <= 5.0), "the far tail of AS 241 is not part of the device's formula"
    r = r - 1.6
    z = _horner(C, r) / _horner(D, r)
    out[t] = np.where(q[t] < 0.0, -z, z)
    return out


def ranks(x):
    """x [S, D] -> average ranks [S, D] (1-based) of every column; a column with a NaN is all NaN."""
    return rankdata(np.asarray(x, dtype=np.float64), method="average", axis=0)


def fold(x):
    x = np.asarray(x, dtype=np.float64)
    return np.abs(x - np.quantile(x, 0.5, axis=0))


def scores(r):
    """ranks [S, D] -> normal scores."""
    return ndtri((r - 0.375) / (r.shape[0] + 0.25))


def rank_summarize(x, max_lag=None, prob=0.05):
    """x [N, C, D] -> dict of [D] arrays: rhat, rhat_bulk, rhat_folded, ess_bulk, ess_tail, lag_truncated; near /
    near_folded / near_tail: the `near` flag of summary_ref.summarize for the bulk series, the folded series and the
    tail indicators."""
    x = np.asarray(x, dtype=np.float64)
    N, Cn, Dn = x.shape
    pooled = x.reshape(N * Cn, Dn)
    bulk = sr.summarize(scores(ranks(pooled)).reshape(x.shape), max_lag=max_lag)
    folded = sr.summarize(scores(ranks(fold(pooled))).reshape(x.shape), max_lag=max_lag)
    tail, near_tail, _ = qr.tail_ess(x, prob=prob, max_lag=max_lag)
    return {"rhat": np.maximum(bulk["rhat"], folded["rhat"]), "rhat_bulk": bulk["rhat"], "rhat_folded": folded["rhat"],
            "ess_bulk": bulk["ess"], "ess_tail": tail, "lag_truncated": bulk["lag_truncated"], "near": bulk["near"],
            "near_folded": folded["near"], "near_tail": near_tail}
