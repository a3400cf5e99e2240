"""numpy restatement of the order statistics, quantiles and tail ESS of include/aehmc_hip.h ("order statistics and
quantiles of the stored draws"), written from their definition.  Imports nothing from aehmc_amd.

x is [R, D] (pooled draws, coordinate).  The quantile at p is numpy's default "linear" rule (R type 7), written out:
  h = p (R - 1), lo = floor(h), g = h - lo, a = x_(lo), b = x_(min(lo + 1, R - 1)), d = b - a,
  q = a + d g if g < 0.5, else b - d (1 - g).
A coordinate that holds a NaN is NaN for every rank and probability."""
import numpy as np

import summary_ref as sr


def order_statistics(x, ranks):
    """[M, D]: the ranks-th smallest (0-based) values of every column of x [R, D]."""
    x = np.asarray(x, dtype=np.float64)
    out = np.sort(x, axis=0)[np.asarray(ranks, dtype=np.int64)]
    out[:, np.isnan(x).any(axis=0)] = np.nan
    return out


def quantiles(x, probs):
    """[Q, D] at the probabilities probs (a sequence)."""
    x = np.asarray(x, dtype=np.float64)
    R = x.shape[0]
    s = np.sort(x, axis=0)
    out = np.empty((len(probs), x.shape[1]))
    with np.errstate(invalid="ignore"):
        for i, p in enumerate(probs):
            h = np.float64(p) * np.float64(R - 1)
            lo = int(np.floor(h))
            g = h - np.floor(h)
            a, b = s[lo], s[min(lo + 1, R - 1)]
            d = b - a
            out[i] = a + d * g if g < 0.5 else b - d * (1.0 - g)
    out[:, np.isnan(x).any(axis=0)] = np.nan
    return out


def tail_ess(x, prob=0.05, max_lag=None):
    """x [N, C, D] -> (tail ESS [D], near [D], lag_truncated [D]): the smaller split-chain ESS (summary_ref.summarize)
    of the indicators x <= q at the prob and the 1 - prob quantile of the pooled draws; near / lag_truncated: either
    indicator's flag."""
    x = np.asarray(x, dtype=np.float64)
    N, C, D = x.shape
    q = quantiles(x.reshape(N * C, D), (prob, 1.0 - prob))
    res = [sr.summarize((x <= q[i]).astype(np.float64), split=True, max_lag=max_lag) for i in range(2)]
    return (np.minimum(res[0]["ess"], res[1]["ess"]), res[0]["near"] | res[1]["near"],
            res[0]["lag_truncated"] | res[1]["lag_truncated"])
