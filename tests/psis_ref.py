"""numpy restatement of Pareto-smoothed importance sampling, PSIS-LOO and WAIC as include/aehmc_hip.h ("Pareto-smoothed
importance sampling") and aehmc_amd/summary.py define them, written from the papers' definitions: Vehtari, Simpson,
Gelman, Yao & Gabry, "Pareto smoothed importance sampling", and Zhang & Stephens (2009) for the generalised-Pareto fit
with the prior constants 3 and 10 that ArviZ's ``_gpdfit`` and R's ``loo`` use.  Imports nothing from aehmc_amd.

Every function takes ``dtype``: np.float64, or np.longdouble to see how much of a result is rounding.  The decisions
that are integers or thresholds (the tail size M, the floor log(DBL_MIN) of the cutoff, the weight cut 10 DBL_EPSILON)
are taken in fp64 whatever the dtype, so that both runs smooth the same draws.

Per column x [R] of log ratios, reff > 0:
    mx = max(x); a NaN, a non-finite mx or a reff that is not finite and > 0: every output NaN, tail_len -1.
    y = x - mx, s = sort(y), M = ceil(min(R / 5, 3 sqrt(R / reff))) held to [0, R - 1],
    cut = max(s[R - M - 1], log(DBL_MIN)), tail = {y > cut}, n = #tail <= M.
    n <= 4: k = +inf, nothing smoothed.  Otherwise t = exp(tail, ascending) - exp(cut), (k, sigma) = gpdfit(t); k not
    finite or sigma not > 0: k = NaN, nothing smoothed.  Otherwise place j of the tail gets
    min(log(sigma gpinv((j + 0.5) / n, k) + exp(cut)), 0), and tied tail draws, occupying places lo ... hi - 1 with
    hi - lo > 1, all get log(sum_{p = lo}^{hi - 1} exp(value of place p) / (hi - lo)).
    lw = y - log(sum(exp(y))); with v: log_mean = logsumexp(lw + v)."""
import numpy as np

LOG_TINY = float(np.log(np.finfo(np.float64).tiny))  # log(DBL_MIN) = -708.3964185322641
EPS = float(np.finfo(np.float64).eps)
PRIOR_BS, PRIOR_K = 3, 10


def tail_size(R, reff=1.0):
    """M, in fp64."""
    with np.errstate(all="ignore"):
        M = np.ceil(min(np.float64(R) / 5.0, 3.0 * np.sqrt(np.float64(R) / np.float64(reff))))
    return int(min(max(M, 0.0), R - 1))


def gpinv(p, k):
    """The quantile function of the generalised Pareto distribution of shape k and scale 1."""
    if abs(float(k)) < EPS:
        return -np.log1p(-p)
    return np.expm1(-k * np.log1p(-p)) / k


def gpdfit(t):
    """(k, sigma) of ascending t [n] > 0, n >= 5: Zhang & Stephens' posterior-mean estimate with the weakly informative
    prior on k (ten pseudo-observations at 0.5).  Not checked for finiteness: the caller does that."""
    dt = t.dtype.type
    n = len(t)
    m = 30 + int(np.floor(np.sqrt(n)))
    with np.errstate(all="ignore"):
        i = np.arange(1, m + 1).astype(dt)
        b = (1 - np.sqrt(dt(m) / (i - dt(0.5)))) / (PRIOR_BS * t[int(n / 4 + 0.5) - 1]) + 1 / t[-1]
        ki = np.log1p(-b[:, None] * t[None, :]).mean(axis=1)
        L = n * (np.log(-b / ki) - ki - 1)
        w = 1 / np.exp(L[None, :] - L[:, None]).sum(axis=1)
        keep = w >= 10 * EPS
        w = w[keep] / w[keep].sum()
        bp = (b[keep] * w).sum()
        kp = np.log1p(-bp * t).mean()
        sigma = -kp / bp
        k = (n * kp + PRIOR_K * dt(0.5)) / (n + PRIOR_K)
    return k, sigma


def logsumexp(a):
    """log sum exp(a) of a 1-d array: -inf entries count nothing, a +inf gives +inf, a NaN gives NaN."""
    dt = a.dtype.type
    if np.isnan(a).any():
        return dt(np.nan)
    m = a.max()
    if not np.isfinite(m):
        return m
    return m + np.log(np.exp(a - m).sum())


def psislw_column(x, reff=1.0, v=None, dtype=np.float64, tie_rule=True, rng=None):
    """(lw [R], k, tail_len, log_mean or None) of one column.  ``tie_rule=False``: ArviZ's psislw, place j of the tail
    going to the j-th tail draw of an argsort; ``rng`` then shuffles the order of tied draws in that argsort."""
    x = np.asarray(x, dtype=np.float64)
    R = len(x)
    nan = dtype(np.nan)
    with np.errstate(invalid="ignore"):
        bad = bool(np.isnan(x).any()) or not np.isfinite(x.max()) or not (np.isfinite(reff) and reff > 0)
    if bad:
        return np.full(R, nan, dtype=dtype), nan, -1, (None if v is None else nan)
    y = x.astype(dtype) - dtype(x.max())
    M = tail_size(R, reff)
    s = np.sort(y)
    cut = max(s[R - M - 1], dtype(LOG_TINY))
    idx = np.flatnonzero(y > cut)
    n = len(idx)
    lw = y.copy()
    k = dtype(np.inf)
    if n > 4:
        if rng is not None:
            idx = rng.permutation(idx)
        order = idx[np.argsort(y[idx], kind="stable")]
        st = y[order]
        ecut = np.exp(cut)
        k, sigma = gpdfit(np.exp(st) - ecut)
        if np.isfinite(k) and sigma > 0:
            p = (np.arange(n).astype(dtype) + dtype(0.5)) / n
            with np.errstate(all="ignore"):
                sm = np.minimum(np.log(sigma * gpinv(p, k) + ecut), dtype(0))
            if tie_rule:
                lo = 0
                while lo < n:
                    hi = lo + 1
                    while hi < n and st[hi] == st[lo]:
                        hi += 1
                    if hi - lo > 1:
                        acc = dtype(0)
                        for q in range(lo, hi):
                            acc = acc + np.exp(sm[q])
                        sm[lo:hi] = np.log(acc / (hi - lo))
                    lo = hi
            lw[order] = sm
        else:
            k = nan
    with np.errstate(divide="ignore"):
        lw = lw - np.log(np.exp(lw).sum())
    mean = None
    if v is not None:
        with np.errstate(invalid="ignore"):
            mean = logsumexp(lw + np.asarray(v, dtype=np.float64).astype(dtype))
    return lw, k, n, mean


def psislw(x, reff=1.0, v=None, dtype=np.float64, tie_rule=True, rng=None):
    """x [R, D] (and v [R, D]) -> dict(lw [R, D], k [D], tail_len [D] int64, log_mean [D] or None); reff a float or [D]."""
    x = np.asarray(x, dtype=np.float64)
    R, D = x.shape
    reff = np.broadcast_to(np.asarray(reff, dtype=np.float64), (D,))
    lw = np.empty((R, D), dtype=dtype)
    k = np.empty(D, dtype=dtype)
    n = np.empty(D, dtype=np.int64)
    mean = None if v is None else np.empty(D, dtype=dtype)
    for d in range(D):
        lw[:, d], k[d], n[d], md = psislw_column(x[:, d], float(reff[d]), None if v is None else v[:, d], dtype,
                                                 tie_rule, rng)
        if v is not None:
            mean[d] = md
    return {"lw": lw, "k": k, "tail_len": n, "log_mean": mean}


def k_threshold(S):
    return min(1.0 - 1.0 / np.log10(S), 0.7)


def loo(ll, reff=1.0, dtype=np.float64):
    """PSIS-LOO of the pointwise log-likelihood ll [S, n_data]: log ratios -ll, elpd_i = log sum_s w_s exp(ll_s)."""
    ll = np.asarray(ll, dtype=np.float64)
    S, n_data = ll.shape
    r = psislw(-ll, reff, ll, dtype)
    lld = ll.astype(dtype)
    lppd_i = np.array([logsumexp(lld[:, d]) for d in range(n_data)], dtype=dtype) - np.log(dtype(S))
    elpd_i = r["log_mean"]
    with np.errstate(invalid="ignore"):
        warn = bool(np.any(r["k"] > k_threshold(S)))
    return {"elpd": elpd_i.sum(), "se": np.sqrt(n_data * np.var(elpd_i)), "p": (lppd_i - elpd_i).sum(),
            "elpd_i": elpd_i, "pareto_k": r["k"], "lppd_i": lppd_i, "tail_len": r["tail_len"],
            "k_threshold": k_threshold(S), "warning": warn}


def waic(ll, dtype=np.float64):
    """WAIC of ll [S, n_data]: p_i the sample variance (divisor S - 1, as in R's loo) of the pooled draws."""
    ll = np.asarray(ll, dtype=np.float64)
    S, n_data = ll.shape
    lld = ll.astype(dtype)
    lppd_i = np.array([logsumexp(lld[:, d]) for d in range(n_data)], dtype=dtype) - np.log(dtype(S))
    with np.errstate(all="ignore"):
        p_i = np.var(lld, axis=0, ddof=1)
    elpd_i = lppd_i - p_i
    return {"elpd": elpd_i.sum(), "se": np.sqrt(n_data * np.var(elpd_i)), "p": p_i.sum(), "elpd_i": elpd_i, "p_i": p_i,
            "lppd_i": lppd_i}
