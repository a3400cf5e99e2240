"""numpy restatement of the posterior-summary formulas (include/aehmc_hip.h, "posterior summaries"), written from
their definition and Stan's published split R-hat / ESS formulas.  Imports nothing from aehmc_amd.

x is [N, C, D] (draw, chain, coordinate).  With n draws per split chain and m split chains:
  W = mean of the chains' variances (ddof 1), B/n = variance of the chains' means (ddof 1, 0 when m = 1),
  var+ = W (n - 1) / n + B/n, rhat = sqrt(var+ / W), mcse_chains = sqrt((B/n) / m), ess_chains = var+ / mcse_chains^2,
  rho_k = 1 - (W - acov_k) / var+ with acov_k the chain-averaged biased autocovariance, pair sums
  P_j = rho_2j + rho_2j+1 taken while positive (P_0 always), clipped to the one before,
  tau = -1 + 2 sum P_j + (even term of the first non-positive pair if positive) >= 1 / log10(m n),
  ess = m n / tau, mcse = sd / sqrt(ess)."""
import numpy as np


def split_chains(x, split=True):
    """[N, C, D] -> [n, m, D]: first and last N // 2 draws of every chain as chains of their own (segment-major)."""
    x = np.asarray(x, dtype=np.float64)
    if not split:
        return x
    N = x.shape[0]
    h = N // 2
    return np.concatenate([x[:h], x[N - h:]], axis=1)


def autocovariance(z, K):
    """[K, D]: biased autocovariance (divided by n) of every chain of z [n, m, D] about its own mean, chain-averaged."""
    n = z.shape[0]
    c = z - z.mean(axis=0)
    out = np.empty((K, z.shape[2]))
    for k in range(K):
        out[k] = (c[:n - k] * c[k:]).sum(axis=0).mean(axis=0) / n
    return out


def summarize(x, split=True, max_lag=None, near=1e-9):
    """dict of [D] arrays: mean, sd, rhat, ess, mcse, ess_chains, mcse_chains, lag_truncated, and `near`: whether a
    pair sum that decided where the sequence stops lay within `near` of zero (the one discrete decision)."""
    z = split_chains(x, split)
    n, m, D = z.shape
    K = n if max_lag is None else min(int(max_lag) + 1, n)
    cm = z.mean(axis=0)                                    # [m, D]
    W = z.var(axis=0, ddof=1).mean(axis=0)
    Bn = cm.var(axis=0, ddof=1) if m > 1 else np.zeros(D)
    varp = W * (n - 1) / n + Bn
    acov = autocovariance(z, K)
    res = {k: np.full(D, np.nan) for k in ("rhat", "ess", "ess_chains", "mcse_chains")}
    res["mean"], res["sd"] = cm.mean(axis=0), np.sqrt(varp)
    res["mcse"], res["lag_truncated"], res["near"] = np.zeros(D), np.zeros(D, dtype=bool), np.zeros(D, dtype=bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        if m > 1:
            res["mcse_chains"] = np.sqrt(Bn / m)
    for d in range(D):
        if not varp[d] > 0:
            continue
        with np.errstate(divide="ignore", invalid="ignore"):
            res["rhat"][d] = np.sqrt(varp[d] / W[d])
            if m > 1:
                res["ess_chains"][d] = varp[d] / (Bn[d] / m)
            rho = 1.0 - (W[d] - acov[:, d]) / varp[d]
        rho[0] = 1.0
        total = prev = rho[0] + rho[1]
        extra, k = 0.0, 2
        while True:
            if k + 1 >= K:
                res["lag_truncated"][d] = True
                break
            P = rho[k] + rho[k + 1]
            if abs(P) < near:
                res["near"][d] = True
            if not P > 0:
                extra = max(rho[k], 0.0)
                break
            prev = min(P, prev)
            total += prev
            k += 2
        tau = max(-1.0 + 2.0 * total + extra, 1.0 / np.log10(m * n))
        res["ess"][d] = m * n / tau
        res["mcse"][d] = res["sd"][d] / np.sqrt(res["ess"][d])
    return res


def ar1(rng, N, C, D, phi, loc=0.0, scale=1.0):
    """Stationary AR(1) series [N, C, D] of marginal N(loc, scale^2): ESS = N C (1 - phi) / (1 + phi)."""
    x = np.empty((N, C, D))
    x[0] = rng.standard_normal((C, D))
    s = np.sqrt(1.0 - phi * phi)
    for t in range(1, N):
        x[t] = phi * x[t - 1] + s * rng.standard_normal((C, D))
    return loc + scale * x
