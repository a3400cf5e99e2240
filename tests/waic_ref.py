"""The streaming WAIC fold of csrc/pointwise.cuh restated in numpy, operation for operation -- the same parts (PART
consecutive rows of a call, the last one shorter), the same order inside a part and the same ascending merge behind the
state -- and an exact reference computed from the same doubles with mpmath at 50 digits.

mean and M2 use + - * / only, every operation rounded on its own on both sides (the library is built with
-ffp-contract=off), so the device's are these bits; m is a selection; s goes through exp, where two math libraries may
differ in the last place.

Allowances (U = 2^-53, S draws): lppd_i within 4 (S + 64) U absolute -- a sequential sum of S terms in [0, 1] relative
to a sum >= 1 gives S U, the rescalings and the arguments of exp (|l - m| rounded, exp within a few ulp) a few more per
term, log and the final subtraction a constant number; p_i within 4 S U kappa_i p_i, kappa_i = sqrt(1 + mean_i^2 /
var_i): the bound of Chan, Golub & LeVeque (1983) for updating algorithms, S kappa U, times 4 for the part merges."""
import numpy as np

PART = 256  # csrc/pointwise.cuh: PW_PART
U = 2.0 ** -53


def fold_part(x):
    """x [n, n_obs] -> (m, s, mean, M2), each [n_obs]: the draws of one part, in order"""
    n_obs = x.shape[1]
    m, s, mean, m2 = np.full(n_obs, -np.inf), np.zeros(n_obs), np.zeros(n_obs), np.zeros(n_obs)
    with np.errstate(all="ignore"):
        for k, l in enumerate(x, start=1):
            up = l > m
            s_up = s * np.exp(m - l) + 1.0
            s_stay = s + np.where(l == m, 1.0, np.exp(l - m))
            s = np.where(l == -np.inf, s, np.where(up, s_up, s_stay))
            m = np.where(up, l, m)
            d = l - mean
            mean = mean + d / float(k)
            m2 = m2 + d * (l - mean)
    return m, s, mean, m2


def merge(a, na, b, nb):
    """part b (nb draws) behind state a (na draws)"""
    if na == 0:
        return tuple(np.array(v, copy=True) for v in b)
    (ma, sa, meana, m2a), (mb, sb, meanb, m2b) = a, b
    with np.errstate(all="ignore"):
        up = mb > ma
        s = np.where(up, sa * np.exp(ma - mb) + sb, sa + sb * np.where(mb == ma, 1.0, np.exp(mb - ma)))
        m = np.where(up, mb, ma)
        n, d = float(na + nb), meanb - meana
        mean = meana + d * (float(nb) / n)
        m2 = (m2a + m2b) + (d * d) * (float(na) * float(nb) / n)
    return m, s, mean, m2


class Fold:
    def __init__(self, n_obs):
        self.state = (np.full(n_obs, -np.inf), np.zeros(n_obs), np.zeros(n_obs), np.zeros(n_obs))
        self.n = 0

    def update(self, x):
        x = np.asarray(x, dtype=np.float64).reshape(-1, self.state[0].shape[0])
        for r0 in range(0, x.shape[0], PART):
            blk = x[r0:r0 + PART]
            self.state = merge(self.state, self.n, fold_part(blk), blk.shape[0])
            self.n += blk.shape[0]
        return self

    def merge(self, other):
        self.state = merge(self.state, self.n, other.state, other.n)
        self.n += other.n
        return self

    def result(self):
        m, s, _, m2 = self.state
        with np.errstate(all="ignore"):
            return (m + np.log(s)) - np.log(float(self.n)), m2 / (float(self.n) - 1.0)


def exact(x):
    """(lppd, p, kappa) per column of x [S, n_obs] from the same doubles at 50 digits; -inf counts as exp = 0 in lppd and
    makes p NaN, a NaN makes both NaN"""
    import mpmath
    mp = mpmath.mp.clone()
    mp.dps = 50
    S, n_obs = x.shape
    lppd, p, kappa = np.empty(n_obs), np.empty(n_obs), np.empty(n_obs)
    for j in range(n_obs):
        col = x[:, j]
        if np.isnan(col).any():
            lppd[j] = p[j] = kappa[j] = np.nan
            continue
        fin = [mp.mpf(float(v)) for v in col if v != -np.inf]
        top = max(fin) if fin else None
        lppd[j] = float(top + mp.log(mp.fsum(mp.exp(v - top) for v in fin)) - mp.log(S)) if fin else -np.inf
        if len(fin) < S or S < 2:
            p[j] = kappa[j] = np.nan
            continue
        mean = mp.fsum(fin) / S
        ss = mp.fsum((v - mean) ** 2 for v in fin)
        p[j] = float(ss / (S - 1))
        kappa[j] = float(mp.sqrt(1 + mean * mean / (ss / S))) if ss > 0 else np.inf
    return lppd, p, kappa


def allowances(S, p, kappa):
    return 4.0 * (S + 64) * U, 4.0 * S * U * kappa * p
