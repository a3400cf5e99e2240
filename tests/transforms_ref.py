"""The transforms of aehmc_amd/transforms.py and csrc/constrain.cuh, restated: numpy (theta, ldj, inverse, in the operation
order of the header's table), mpmath closed forms at 50 digits, and the ALLOWANCE of every value.  Shared by
tests/test_transforms_host.py and tests/test_gpu_transforms.py.

The criterion is |got - want| <= allowance, an absolute number per output built the way tests/dual_ref.py builds its own
(its `ulp`, `lib`, `rnd` are imported): E_np + 2 ulp per forwarded library function (exp, log; log1p measured here by the
same recipe), half an ulp per IEEE operation counted from the formula, an error carried through an operation by that
operation's derivative, a sum's allowance the sum of its terms' allowances, and half an ulp of the reference for its one
rounding to fp64.  No number is taken from a build of the kernel.  Where the closed form is not finite (exp overflow, a
NaN or inf - inf among the inputs) the criterion is the IEEE class: NaN, +inf or -inf."""
import math

import numpy as np

from dual_ref import _mp, lib, rnd, ulp

REAL, LOWER, UPPER, INTERVAL, ORDERED, SIMPLEX = range(6)
NAMES = ("Real", "LowerBound", "UpperBound", "Interval", "Ordered", "Simplex")


# ---------------------------------------------------------------------------------------------- numpy restatement
def softplus_np(x):  # max(x, 0) + log1p(exp(-|x|))
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def theta_np(kind, x, lo=0.0, hi=0.0):
    """one segment: x [n_in] -> theta [n_out]; lo, hi floats or arrays [n_out]"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        if kind == REAL:
            return x.copy()
        if kind == LOWER:
            return lo + np.exp(x)
        if kind == UPPER:
            return hi - np.exp(x)
        if kind == INTERVAL:
            e = np.exp(-np.abs(x))
            s = np.where(x >= 0, 1.0 / (1.0 + e), np.where(np.isnan(x), np.nan, e / (1.0 + e)))
            y = lo + (hi - lo) * s
            return np.where((s == 1.0) | (y > hi), hi, y)
        if kind == ORDERED:
            out = np.empty_like(x)
            t = out[0] = x[0]
            for j in range(1, len(x)):
                t = out[j] = t + np.exp(x[j])
            return out
        xt = np.concatenate([x, [0.0]])
        m = xt[0]
        for v in xt[1:]:
            m = v if v > m else m
        tot = np.exp(xt[0] - m)
        for v in xt[1:]:
            tot = tot + np.exp(v - m)
        L = m + np.log(tot)
        return np.exp(xt - L)


def ldj_np(kind, x, lo=0.0, hi=0.0):
    """one segment's log |det J|"""
    x = np.asarray(x, dtype=np.float64)
    if kind == REAL:
        return 0.0
    if kind in (LOWER, UPPER):
        return _sum_np(x)
    if kind == INTERVAL:
        return _sum_np(np.log(np.asarray(hi, dtype=np.float64) - lo) - softplus_np(x) - softplus_np(-x))
    if kind == ORDERED:
        return _sum_np(x[1:])
    xt = np.concatenate([x, [0.0]])
    m = xt.max()
    tot = np.exp(xt[0] - m)
    for v in xt[1:]:
        tot = tot + np.exp(v - m)
    return _sum_np(xt) - float(len(xt)) * (m + np.log(tot))


def _sum_np(v):
    v = np.atleast_1d(v)
    t = v[0]
    for w in v[1:]:
        t = t + w
    return float(t)


def inverse_np(kind, t, lo=0.0, hi=0.0):
    t = np.asarray(t, dtype=np.float64)
    if kind == REAL:
        return t.copy()
    if kind == LOWER:
        return np.log(t - lo)
    if kind == UPPER:
        return np.log(hi - t)
    if kind == INTERVAL:
        u = (t - lo) / (np.asarray(hi, dtype=np.float64) - lo)
        return np.log(u) - np.log1p(-u)
    if kind == ORDERED:
        return np.concatenate([t[:1], np.log(t[1:] - t[:-1])])
    lt = np.log(t)
    return lt[:-1] - lt[-1]


# ---------------------------------------------------------------------------------------------- 50 digits
def _ctx():
    """mpmath's context at 50 digits or more: mpmath's own differentiation calls the closed forms at a raised precision,
    which they must not lower"""
    import mpmath
    if mpmath.mp.dps < 50:
        mpmath.mp.dps = 50
    return mpmath.mp


def _vec(v, n):
    return np.broadcast_to(np.asarray(v, dtype=np.float64), (n,))


def _mpf(mp, v):
    return v if isinstance(v, mp.mpf) else mp.mpf(float(v))  # (an mpf passes: theta_mp is differentiated by mpmath)


def theta_mp(kind, x, lo=0.0, hi=0.0):
    """one segment at 50 digits: a list of mpf (nan / inf where the closed form has them)"""
    mp = _ctx()
    x = [_mpf(mp, v) for v in (x if isinstance(x, (list, tuple)) else np.atleast_1d(x))]
    n_out = len(x) + (kind == SIMPLEX)
    lo, hi = [_mpf(mp, v) for v in _vec(lo, n_out)], [_mpf(mp, v) for v in _vec(hi, n_out)]
    if kind == REAL:
        return x
    if kind == LOWER:
        return [a + mp.exp(v) for a, v in zip(lo, x)]
    if kind == UPPER:
        return [b - mp.exp(v) for b, v in zip(hi, x)]
    if kind == INTERVAL:
        def s(v):
            if mp.isnan(v):
                return mp.nan
            return 1 / (1 + mp.exp(-v)) if v >= 0 else mp.exp(v) / (1 + mp.exp(v))
        return [a + (b - a) * s(v) for a, b, v in zip(lo, hi, x)]
    if kind == ORDERED:
        out = [x[0]]
        for v in x[1:]:
            out.append(out[-1] + mp.exp(v))
        return out
    xt = x + [mp.mpf(0)]
    if any(mp.isnan(v) for v in xt) or any(v == mp.inf for v in xt):
        return [mp.nan] * len(xt)
    L = _lse_mp(mp, xt)
    return [mp.exp(v - L) for v in xt]


def _lse_mp(mp, xt):
    m = max(xt)
    return m + mp.log(mp.fsum(mp.exp(v - m) for v in xt))


def ldj_mp(kind, x, lo=0.0, hi=0.0):
    mp = _ctx()
    x = [_mpf(mp, v) for v in np.atleast_1d(x)]
    n_out = len(x) + (kind == SIMPLEX)
    lo, hi = [_mpf(mp, v) for v in _vec(lo, n_out)], [_mpf(mp, v) for v in _vec(hi, n_out)]
    if kind == REAL:
        return mp.mpf(0)
    if kind in (LOWER, UPPER):
        return mp.fsum(x)
    if kind == INTERVAL:
        sp = lambda v: (v if v > 0 else 0) + mp.log1p(mp.exp(-abs(v)))  # noqa: E731
        return mp.fsum(mp.log(b - a) - sp(v) - sp(-v) for a, b, v in zip(lo, hi, x))
    if kind == ORDERED:
        return mp.fsum(x[1:])
    xt = x + [mp.mpf(0)]
    return mp.fsum(xt) - len(xt) * _lse_mp(mp, xt)


def to_float(v):
    mp = _mp()
    if mp.isnan(v):
        return math.nan
    try:
        return float(v)
    except OverflowError:
        return math.copysign(math.inf, float(mp.sign(v)))


# ---------------------------------------------------------------------------------------------- allowances
_E1P = {}


def lib1p(args):
    """E_np + 2 for log1p, measured as dual_ref.e_np measures its own table (which has no log1p)"""
    args = np.ascontiguousarray(args, dtype=np.float64)
    key = args.tobytes()
    if key not in _E1P:
        mp = _mp()
        want = np.array([float(mp.log1p(mp.mpf(float(a)))) for a in args])
        got = np.log1p(args)
        fin = np.isfinite(want) & (np.abs(want) >= 2.2250738585072014e-308)
        _E1P[key] = (float(np.max(np.abs(got[fin] - want[fin]) / ulp(want[fin]))) if fin.any() else 0.0) + 2.0
    return _E1P[key]


def _f(v):
    return to_float(v)


def _exp_allow(arg):
    """absolute allowance of a forwarded exp at the fp64 argument `arg` (exact argument)"""
    arg = float(arg)
    if not np.isfinite(arg):
        return 0.0
    with np.errstate(all="ignore"):
        w = float(np.exp(arg))
    return lib("exp", [arg]) * ulp(w) if np.isfinite(w) else 0.0


def _log_allow(arg):
    w = float(np.log(arg))
    return lib("log", [arg]) * ulp(w)


def _lse_allow(mp, xt):
    """(L at 50 digits, its allowance): m = max (a selection, exact); d_j = xt_j - m, one rounding; E_j = exp(d_j), the
    error of d_j carried by exp' = E_j plus the library's; tot: the sum of the terms' allowances plus one rounding per
    addition (of the partial sum); log(tot): carried by 1 / tot plus the library's; L = m + log(tot), one rounding."""
    m = max(xt)
    a_tot, part = 0.0, mp.mpf(0)
    for j, v in enumerate(xt):
        d = v - m
        E = mp.exp(d)
        if np.isfinite(_f(d)):  # (a coordinate at -inf contributes an exact 0)
            a_tot += _f(E) * rnd(1, _f(d)) + _exp_allow(_f(d))
        part += E
        if j:
            a_tot += rnd(1, _f(part))
    lg = mp.log(part)
    a_log = a_tot / _f(part) + _log_allow(_f(part))
    L = m + lg
    return L, a_log + rnd(1, _f(L))


def theta_allowance(kind, x, lo=0.0, hi=0.0):
    """(want [n_out] fp64 -- the 50-digit value rounded once --, allowance [n_out]) of one segment"""
    mp = _mp()
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    want_mp = theta_mp(kind, x, lo, hi)
    want = np.array([_f(v) for v in want_mp])
    n_out = len(want)
    lo, hi = _vec(lo, n_out), _vec(hi, n_out)
    allow = np.zeros(n_out)
    half = lambda w: 0.5 * ulp(w) if np.isfinite(w) else 0.0  # noqa: E731 (the reference's own rounding)
    if kind == REAL:
        return want, allow
    if kind in (LOWER, UPPER):  # exp (library), one addition
        for j in range(n_out):
            if np.isfinite(want[j]):
                allow[j] = _exp_allow(x[j]) + rnd(1, want[j]) + half(want[j])
        return want, allow
    if kind == INTERVAL:
        for j in range(n_out):
            if not np.isfinite(x[j]) and np.isnan(x[j]):
                continue
            w = hi[j] - lo[j]
            a_w = rnd(1, w)
            e = float(np.exp(-abs(x[j])))           # t = exp(-|x|): the library's allowance
            a_e = _exp_allow(-abs(x[j]))
            d = 1.0 + e
            a_d = a_e + rnd(1, d)                   # d = 1 + t: one rounding
            if x[j] >= 0:                           # s = 1 / d: carried by 1 / d^2, one rounding
                s = 1.0 / d
                a_s = a_d / (d * d) + rnd(1, s)
            else:                                   # s = t / d: carried by 1 / d and t / d^2, one rounding
                s = e / d
                a_s = a_e / d + s * a_d / d + rnd(1, s)
            p = w * s                               # p = w s: both errors carried, one rounding; y = lo + p: one rounding
            a_p = abs(w) * a_s + s * a_w + rnd(1, p)
            allow[j] = a_p + rnd(1, want[j]) + half(want[j])
        return want, allow
    if kind == ORDERED:  # t_j = t_{j-1} + exp(x_j): the running allowance, the library's, one rounding
        a = 0.0
        for j in range(1, n_out):
            if not np.isfinite(want[j]):
                break
            a += _exp_allow(x[j]) + rnd(1, want[j])
            allow[j] = a + half(want[j])
        return want, allow
    if not np.isfinite(want).all():
        return want, allow
    xt = [_mpf(mp, v) for v in x] + [mp.mpf(0)]
    L, a_L = _lse_allow(mp, xt)
    for j in range(n_out):  # z = xt_j - L: one rounding; y = exp(z): carried by y, plus the library's
        z = _f(xt[j] - L)
        if np.isfinite(z):  # (a coordinate at -inf: an exact 0)
            allow[j] = want[j] * (a_L + rnd(1, z)) + _exp_allow(z) + half(want[j])
    return want, allow


def ldj_allowance(kind, x, lo=0.0, hi=0.0):
    """(want fp64, allowance) of one segment's ldj as ldj_np forms it"""
    mp = _mp()
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    want = _f(ldj_mp(kind, x, lo, hi))
    half = 0.5 * ulp(want)

    def sum_allow(terms):  # one rounding per addition, of the partial sum
        a, part = 0.0, float(terms[0]) if len(terms) else 0.0
        for v in terms[1:]:
            part += float(v)
            a += rnd(1, part)
        return a

    if kind == REAL:
        return want, 0.0
    if kind in (LOWER, UPPER):
        return want, sum_allow(x) + half
    if kind == ORDERED:
        return want, sum_allow(x[1:]) + half
    if kind == INTERVAL:
        lo, hi = _vec(lo, len(x)), _vec(hi, len(x))
        terms, a = [], 0.0
        for j in range(len(x)):
            w = hi[j] - lo[j]
            lw = float(np.log(w))
            a_lw = rnd(1, w) / w + _log_allow(w)                 # log(hi - lo): the subtraction's rounding carried by 1 / w
            t = float(np.exp(-abs(x[j])))
            l1 = float(np.log1p(t))
            a_l1 = _exp_allow(-abs(x[j])) / (1.0 + t) + lib1p([t]) * ulp(l1)
            sp_pos, sp_neg = max(x[j], 0.0) + l1, max(-x[j], 0.0) + l1  # softplus(x), softplus(-x): one addition each
            a_sp = 2 * a_l1 + rnd(1, sp_pos) + rnd(1, sp_neg)
            term = lw - sp_pos - sp_neg
            a += a_lw + a_sp + rnd(1, lw - sp_pos) + rnd(1, term)
            terms.append(term)
        return want, a + sum_allow(terms) + half
    xt = [_mpf(mp, v) for v in x] + [mp.mpf(0)]
    L, a_L = _lse_allow(mp, xt)
    K = len(xt)
    KL = K * _f(L)
    return want, sum_allow([_f(v) for v in xt]) + K * a_L + rnd(1, KL) + rnd(1, want) + half


def within(got, want, allow):
    """the criterion, elementwise: equal IEEE class where the reference is not finite, else |got - want| <= allow"""
    got, want, allow = np.broadcast_arrays(np.asarray(got, dtype=np.float64), want, allow)
    ok = np.empty(got.shape, dtype=bool)
    nan, inf = np.isnan(want), np.isinf(want)
    ok[nan] = np.isnan(got[nan])
    ok[inf] = got[inf] == want[inf]
    fin = ~nan & ~inf
    with np.errstate(invalid="ignore"):
        ok[fin] = np.abs(got[fin] - want[fin]) <= allow[fin]
    return ok


# ---------------------------------------------------------------------------------------------- specs (whole rows)
class Spec:
    """A list of (kind, n_out, lo, hi): the layout of a row, restated without aehmc_amd.transforms."""

    def __init__(self, parts):
        self.parts = [(k, int(n), lo, hi) for k, n, lo, hi in parts]
        self.d_in = sum(n - (k == SIMPLEX) for k, n, _, _ in self.parts)
        self.d_out = sum(n for _, n, _, _ in self.parts)

    def segments(self):
        a = b = 0
        for k, n, lo, hi in self.parts:
            n_in = n - (k == SIMPLEX)
            yield k, slice(a, a + n_in), slice(b, b + n), lo, hi
            a, b = a + n_in, b + n

    def theta_np(self, x):
        out = np.empty(self.d_out)
        for k, si, so, lo, hi in self.segments():
            out[so] = theta_np(k, x[si], lo, hi)
        return out

    def reference(self, x):
        """(want [d_out], allowance [d_out]) of one row"""
        want, allow = np.empty(self.d_out), np.empty(self.d_out)
        for k, si, so, lo, hi in self.segments():
            want[so], allow[so] = theta_allowance(k, x[si], lo, hi)
        return want, allow

    def model(self, logprob=None):
        from aehmc_amd import transforms as tf
        make = {REAL: lambda n, lo, hi: tf.Real(n), LOWER: lambda n, lo, hi: tf.LowerBound(lo, n),
                UPPER: lambda n, lo, hi: tf.UpperBound(hi, n), INTERVAL: lambda n, lo, hi: tf.Interval(lo, hi, n),
                ORDERED: lambda n, lo, hi: tf.Ordered(n), SIMPLEX: lambda n, lo, hi: tf.Simplex(n)}
        spec = {f"p{i}": make[k](n, lo, hi) for i, (k, n, lo, hi) in enumerate(self.parts)}
        return tf.Model(spec, logprob or (lambda **kw: 0.0))


# ---------------------------------------------------------------------------------------------- a model with known marginals
# sigma ~ Gamma(3, rate 2), rho = 2 Beta(2, 3) - 1, pi ~ Dirichlet(2, 3, 4), mu = two ordered standard normals,
# w ~ N(0, I_3): exact E[theta] and E[theta^2], in the constrained layout (sigma, rho, pi_0..2, mu_0..1, w_0..2)
EXACT_MEAN = np.array([1.5, -0.2, 2 / 9, 3 / 9, 4 / 9, -1 / np.sqrt(np.pi), 1 / np.sqrt(np.pi), 0.0, 0.0, 0.0])
EXACT_SQUARE = np.array([3.0, 0.2, 6 / 90, 12 / 90, 20 / 90, 1.0, 1.0, 1.0, 1.0, 1.0])


