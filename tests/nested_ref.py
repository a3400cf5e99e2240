"""Plain numpy float64 restatement of the nested R-hat of Margossian, Hoffman, Sountsov, Riou-Durand, Vehtari and Gelman
("Nested R-hat: assessing the convergence of Markov chain Monte Carlo when running many short chains"), by two-pass
formulas: what aehmc_amd.summary.nested_rhat / NestedAccumulator (csrc/nested.cuh) are held to.

x is [N, C, D]: N draws of C = K M chains, chain c in superchain c // M.  All quantities per coordinate and per window of
w draws (window=None: one window of all N)."""
import numpy as np

FIELDS = ("nested_rhat", "between", "within", "mean", "mcse_superchains")


def window_stats(xw, K):
    """xw [n, C, D], one window -> dict of [D] arrays."""
    n, C, D = xw.shape
    M = C // K
    a = xw.mean(axis=0)                                                        # a_c          [C, D]
    s2 = ((xw - a) ** 2).sum(axis=0) / (n - 1) if n > 1 else np.zeros((C, D))  # s2_c         [C, D]
    a, s2 = a.reshape(K, M, D), s2.reshape(K, M, D)
    abar_k = a.mean(axis=1)                                                    # superchain means [K, D]
    abar = abar_k.mean(axis=0)
    between = ((abar_k - abar) ** 2).sum(axis=0) / (K - 1)
    b_tilde = ((a - abar_k[:, None]) ** 2).sum(axis=1) / (M - 1) if M > 1 else np.zeros((K, D))
    w_tilde = s2.mean(axis=1)
    within = (b_tilde + w_tilde).mean(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        rhat = np.sqrt(1.0 + between / within)
    return {"nested_rhat": rhat, "between": between, "within": within, "mean": abar,
            "mcse_superchains": np.sqrt(between / K)}


def nested_rhat(x, K, window=None):
    """dict of the FIELDS: [D] arrays with window=None, [N // window, D] otherwise."""
    x = np.asarray(x, dtype=np.float64)
    N, C, D = x.shape
    assert K >= 2 and C % K == 0
    if window is None:
        return window_stats(x, K)
    assert N % window == 0
    rows = [window_stats(x[i:i + window], K) for i in range(0, N, window)]
    return {f: np.stack([r[f] for r in rows]) for f in FIELDS}


def classical_rhat(x):
    """The unsplit classical R-hat of x [N, C, D]: sqrt(((n - 1) / n W + B / n) / W)."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    a = x.mean(axis=0)
    W = (((x - a) ** 2).sum(axis=0) / (n - 1)).mean(axis=0)
    Bn = ((a - a.mean(axis=0)) ** 2).sum(axis=0) / (x.shape[1] - 1)
    return np.sqrt(((n - 1) / n * W + Bn) / W)


def draws(seed, N, K, M, D, offset=1e4):
    """Seeded normals [N, K M, D] with a scale per coordinate, a shift per superchain and per chain, and an offset per
    coordinate spread over [-offset, offset]."""
    r = np.random.default_rng(seed)
    x = r.standard_normal((N, K, M, D)) * (0.5 + r.random(D))
    x += 0.3 * r.standard_normal((1, K, 1, D)) + 0.1 * r.standard_normal((1, K, M, D))
    x += np.linspace(-offset, offset, D) if D > 1 else offset
    return x.reshape(N, K * M, D)
