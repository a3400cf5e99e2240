"""The function table of csrc/dual.cuh and of the tracer's reverse-mode rules (aehmc_amd/tracing.py: _UN_BWD, _REV_FN,
the pow adjoints): every supported function with its C++ expression, the numpy expression the tracer accepts, f and f'
as mpmath closed forms (evaluated at 50 digits, rounded once to fp64), seeded points, edge arguments with the IEEE class
expected there, and the ALLOWANCE of value and derivative.  Shared by tests/test_dual_reference_host.py (g++ build) and
tests/test_gpu_dual_reference.py (hipRTC builds on the device).

The criterion is |got - want| <= allowance(x), an absolute number per point made of n ulp(want) + a(x).  No point is
excluded.  Every allowance comes from one of three places, named in the row's comment:
  [project]    a bound the project states against numpy / scipy (dual.cuh's comments, tests/test_dual.py), plus the
               error of numpy / scipy itself at the same point, |numpy(x) - want| (triangle inequality);
  [library]    a function dual.cuh forwards to the math library: E_np(f) + 2 ulp, E_np(f) = the largest error of numpy's
               function on the same arguments (where the result is a normal number), in ulp, measured here against mpmath -- the margin the project grants
               its own log replacement over numpy.  `lib(...)` below; inside a formula the same number as a relative
               error, (E_np + 2) 2^-52 |want|;
  [roundings]  a count of IEEE operations, 2^-53 relative (0.5 ulp) each: `rnd(k, want)`.
None is taken from a build of dual.cuh.  The derivative's reference is rounded to fp64 once: half an ulp of `want` is
added to every derivative allowance for it (value allowances of [roundings] rows count it themselves)."""
import functools
import math

import numpy as np

U = 2.0 ** -53      # one rounding, relative
TINY = 5e-324       # one rounding in gradual underflow, absolute
LOG2E, LOG10E, LN2 = 1.0 / math.log(2.0), 1.0 / math.log(10.0), math.log(2.0)  # (the tracer's constants: tracing.py _ufunc)


def ulp(w):
    return np.spacing(np.abs(w))


def rnd(k, w):
    """k roundings of a result of size |w|"""
    return k * (U * np.abs(w) + TINY)


def _mp():
    import mpmath
    mpmath.mp.dps = 50
    return mpmath.mp


def _to_float(fn, x):
    try:
        v = fn(x)
        return float(v)
    except OverflowError:
        return math.copysign(math.inf, float(_mp().sign(v)))
    except (TypeError, ValueError, ZeroDivisionError):  # complex, or a pole: no finite reference (an edge states its class itself)
        return math.nan


def mp_eval(fn, xs):
    """a closed form at 50 digits over fp64 arguments, rounded once to fp64"""
    mp = _mp()
    return np.array([_to_float(fn, mp.mpf(float(x))) for x in np.asarray(xs, dtype=np.float64).ravel()])


# ---------------------------------------------------------------------------------------------- numpy's own error
def _scipy(name):
    from scipy import special
    return getattr(special, name)


_NP_LIB = {  # library function -> (numpy / scipy, mpmath)
    "exp": (np.exp, lambda mp, x: mp.exp(x)), "expm1": (np.expm1, lambda mp, x: mp.expm1(x)),
    "sqrt": (np.sqrt, lambda mp, x: mp.sqrt(x)), "sin": (np.sin, lambda mp, x: mp.sin(x)), "cos": (np.cos, lambda mp, x: mp.cos(x)),
    "tanh": (np.tanh, lambda mp, x: mp.tanh(x)), "sinh": (np.sinh, lambda mp, x: mp.sinh(x)), "cosh": (np.cosh, lambda mp, x: mp.cosh(x)),
    "atan": (np.arctan, lambda mp, x: mp.atan(x)), "log": (np.log, lambda mp, x: mp.log(x)),
    # (numpy has neither; scipy.special.erfc forms exp(-x x) itself and is 408 ulp off at |x| = 26: the C library's, through math)
    "erf": (np.vectorize(math.erf, otypes=[np.float64]), lambda mp, x: mp.erf(x)), "erfc": (np.vectorize(math.erfc, otypes=[np.float64]), lambda mp, x: mp.erfc(x)),
}
_E_NP = {}


def e_np(name, args, second=None):
    """E_np: the largest error of numpy's `name` (pow: numpy.power(args, second)) on `args`, in ulp of the rounded 50-digit value"""
    args = np.ascontiguousarray(args, dtype=np.float64)
    key = (name, args.tobytes(), None if second is None else np.asarray(second, dtype=np.float64).tobytes())
    if key not in _E_NP:
        mp = _mp()
        with np.errstate(all="ignore"):
            if name == "pow":
                sec = np.broadcast_to(np.asarray(second, dtype=np.float64), args.shape)
                got = np.power(args, sec)
                want = np.array([_to_float(lambda a: mp.power(a, mp.mpf(float(b))), mp.mpf(float(a))) for a, b in zip(args, sec)])
            else:
                f, g = _NP_LIB[name]
                got, want = f(args), mp_eval(lambda x: g(mp, x), args)
        fin = np.isfinite(want) & (np.abs(want) >= 2.2250738585072014e-308)  # (normal results: in gradual underflow an ulp is no relative error)
        _E_NP[key] = float(np.max(np.abs(got[fin] - want[fin]) / ulp(want[fin]))) if fin.any() else 0.0
    return _E_NP[key]


def lib(name, args, second=None):
    """ulp granted to a forwarded library function on these arguments: E_np + 2"""
    return e_np(name, args, second) + 2.0


# ---------------------------------------------------------------------------------------------- points
def _entire(seed):
    r = np.random.default_rng(seed)
    return np.concatenate([r.normal(0.0, 3.0, 1200), np.linspace(-30.0, 30.0, 601)])


def _octaves():  # sqrt(2) 2^k +- 1 ulp: where log_fast moves the mantissa into the next octave
    b = np.sqrt(2.0) * np.exp2(np.arange(-5, 6))
    return np.concatenate([b, np.nextafter(b, 0.0), np.nextafter(b, np.inf)])


def _positive(seed):
    r = np.random.default_rng(seed)
    return np.concatenate([np.exp(r.uniform(-20.0, 20.0, 1000)), 1.0 + r.uniform(-1e-3, 1e-3, 300), r.uniform(0.5, 2.0, 500), _octaves(),
                           [1.0, np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0)]])


def _log1p_points(seed):
    r = np.random.default_rng(seed)
    return np.concatenate([np.expm1(r.uniform(-30.0, 30.0, 800)), r.normal(0.0, 1e-3, 300), r.uniform(-0.999, 3.0, 700), _octaves() - 1.0])


def _gamma_points(seed):
    r = np.random.default_rng(seed)
    neg = -r.uniform(0.0, 6.0, 400)
    neg = neg[np.abs(neg - np.round(neg)) >= 0.1][:100]  # (the reflection's tan(pi x) loses relative accuracy next to the poles)
    return np.concatenate([np.geomspace(1e-3, 1e3, 800), r.uniform(0.0, 30.0, 1000), -np.linspace(0.1, 5.9, 30) - 0.05, neg])


def _wide(seed):
    return np.concatenate([_entire(seed), np.linspace(-700.0, 700.0, 141)])


def _nonzero(seed):
    x = _entire(seed)
    return x[x != 0.0]


# ---------------------------------------------------------------------------------------------- the rows
class Row:
    """cpp: the expression of `T q` in aehmc_logp; np: the traced numpy expression (None: no traced form); f, df: mpmath
    closed forms (mp, x); points: seed -> fp64 arguments; va, da: (x, want_value, want_derivative) -> absolute allowance;
    edges: (argument, class of the value, class of the derivative), a class one of "nan" "+inf" "-inf" "+0" "-0" "finite"
    ("finite": within the allowance of the closed form there); lib_double: the T = double instantiation is the math
    library's own function, not dual.cuh's (held to the same allowance instead of bitwise equality with the Dual)."""

    def __init__(self, name, cpp, np_fn, f, df, points, va, da, edges=(), lib_double=False):
        self.name, self.cpp, self.np, self.f, self.df, self.points_fn = name, cpp, np_fn, f, df, points
        self.va, self.da, self.edges, self.lib_double = va, da, list(edges), lib_double


def _sp(name):
    return lambda x: _scipy(name)(x)


def _softplus_np(x):
    from aehmc_amd import tracing
    return tracing.softplus(x)


def _np_err(fn, x, want):
    with np.errstate(all="ignore"):
        return np.abs(fn(x) - want)


def _lgamma_f(mp, x):
    return mp.loggamma(x) if x > 0 else mp.log(abs(mp.gamma(x)))


def _erf_da(x, v, d):
    # [roundings] c exp(-x x): x x rounds once, 2^-53 x^2 absolute in the exponent = relative in the result (first order; x^2 2^-53 < 1e-13);
    # the constant and the product one rounding each; [library] exp at -x^2
    return lib("exp", -x * x) * 2.0 * U * np.abs(d) + rnd(2.0 + x * x, d)


def _tanh_da(x, v, d):
    # [roundings] 1 - t t: t carries [library] tanh, t t twice that plus one rounding, an ABSOLUTE error since the difference is
    # taken from 1 -- (4 lib + 1) 2^-53 is what the formula can give (the truth is below that from |x| = 19 on); the difference rounds once
    return (4.0 * lib("tanh", x) + 1.0) * U * v * v + rnd(1, d)


def _logistic_va(x, v, d):
    # [project] 2e-15 relative of scipy.special.expit
    return 2e-15 * np.abs(v) + _np_err(_sp("expit"), x, v) + TINY


def _logistic_da(x, v, d):
    # [roundings] l (1 - l), l with relative error e_l (its value allowance): 1 - l has the ABSOLUTE error e_l l + 2^-53, times l -- what
    # the formula can give (at x = 38 it returns 0 for 3.1e-17); the factor l again and the product's rounding are relative
    el = _logistic_va(x, v, d) / np.maximum(np.abs(v), 1e-300)
    return (el * v + U) * v + (el + U) * np.abs(d) + TINY


def _ratio_da(x, v, d):
    # [roundings] x / (1 + x x): forward mode forms (1 - 2 x v) / (1 + x x), reverse mode 1 / y - 2 x v / y: either way two terms that
    # cancel at |x| = 1, each with at most 4 roundings -- absolute in the terms' sizes; 3 more on the result
    y = 1.0 + x * x
    return 4.0 * U * (1.0 / y + 2.0 * x * x / (y * y)) + rnd(3, d)


def _rows():
    E, P, W = _entire, _positive, _wide
    rows = [
        # ---- forwarded to the math library: [library] E_np + 2 ulp; derivatives: another library value or a roundings count
        Row("exp", "exp(q)", np.exp, lambda mp, x: mp.exp(x), lambda mp, x: mp.exp(x), E,
            lambda x, v, d: lib("exp", x) * ulp(v), lambda x, v, d: lib("exp", x) * ulp(d),  # e * 1.0: the same library value
            edges=[(710.0, "+inf", "+inf"), (-746.0, "+0", "+0")]),
        Row("expm1", "expm1(q)", np.expm1, lambda mp, x: mp.expm1(x), lambda mp, x: mp.exp(x), E,
            lambda x, v, d: lib("expm1", x) * ulp(v), lambda x, v, d: lib("exp", x) * ulp(d)),  # [library] exp
        Row("sqrt", "sqrt(q)", np.sqrt, lambda mp, x: mp.sqrt(x), lambda mp, x: 0.5 / mp.sqrt(x), P,
            lambda x, v, d: lib("sqrt", x) * ulp(v),
            lambda x, v, d: lib("sqrt", x) * 2.0 * U * np.abs(d) + rnd(1, d),  # 0.5 / s: [library] sqrt + the division
            edges=[(0.0, "+0", "+inf")]),
        Row("sin", "sin(q)", np.sin, lambda mp, x: mp.sin(x), lambda mp, x: mp.cos(x), E,
            lambda x, v, d: lib("sin", x) * ulp(v), lambda x, v, d: lib("cos", x) * ulp(d)),  # [library] cos
        Row("cos", "cos(q)", np.cos, lambda mp, x: mp.cos(x), lambda mp, x: -mp.sin(x), E,
            lambda x, v, d: lib("cos", x) * ulp(v), lambda x, v, d: lib("sin", x) * ulp(d)),  # [library] sin
        Row("tanh", "tanh(q)", np.tanh, lambda mp, x: mp.tanh(x), lambda mp, x: mp.sech(x) ** 2, E,
            lambda x, v, d: lib("tanh", x) * ulp(v), _tanh_da),
        Row("sinh", "sinh(q)", np.sinh, lambda mp, x: mp.sinh(x), lambda mp, x: mp.cosh(x), E,
            lambda x, v, d: lib("sinh", x) * ulp(v), lambda x, v, d: lib("cosh", x) * ulp(d)),  # [library] cosh
        Row("cosh", "cosh(q)", np.cosh, lambda mp, x: mp.cosh(x), lambda mp, x: mp.sinh(x), E,
            lambda x, v, d: lib("cosh", x) * ulp(v), lambda x, v, d: lib("sinh", x) * ulp(d)),  # [library] sinh
        Row("atan", "atan(q)", np.arctan, lambda mp, x: mp.atan(x), lambda mp, x: 1 / (1 + x * x), E,
            lambda x, v, d: lib("atan", x) * ulp(v), lambda x, v, d: rnd(3, d)),  # [roundings] 1 / (1 + x x): 3
        Row("erf", "erf(q)", _sp("erf"), lambda mp, x: mp.erf(x), lambda mp, x: 2 / mp.sqrt(mp.pi) * mp.exp(-x * x), E,
            lambda x, v, d: lib("erf", x) * ulp(v), _erf_da),
        Row("erfc", "erfc(q)", _sp("erfc"), lambda mp, x: mp.erfc(x), lambda mp, x: -2 / mp.sqrt(mp.pi) * mp.exp(-x * x), E,
            lambda x, v, d: lib("erfc", x) * ulp(v), _erf_da),
        Row("pow25", "pow(q, 2.5)", lambda x: x ** 2.5, lambda mp, x: mp.power(x, 2.5), lambda mp, x: 2.5 * mp.power(x, 1.5), P,
            lambda x, v, d: lib("pow", x, 2.5) * ulp(v),
            # p f / x (forward) or p pow(x, p - 1) (reverse): [library] pow + 2 roundings
            lambda x, v, d: max(lib("pow", x, 2.5), lib("pow", x, 1.5)) * 2.0 * U * np.abs(d) + rnd(2, d),
            edges=[(0.0, "+0", "+0")]),
        Row("pow4", "pow(q, 4.0)", lambda x: x ** 4.0, lambda mp, x: x ** 4, lambda mp, x: 4 * x ** 3, E,
            lambda x, v, d: lib("pow", x, 4.0) * ulp(v),
            lambda x, v, d: max(lib("pow", x, 4.0), lib("pow", x, 3.0)) * 2.0 * U * np.abs(d) + rnd(2, d),
            edges=[(-3.0, "finite", "finite"), (-0.5, "finite", "finite"), (0.0, "+0", "+0")]),
        Row("pow05", "pow(q, 0.5)", None, lambda mp, x: mp.sqrt(x), lambda mp, x: 0.5 / mp.sqrt(x), P,  # (the tracer turns x ** 0.5 into sqrt)
            lambda x, v, d: lib("pow", x, 0.5) * ulp(v),
            lambda x, v, d: lib("pow", x, 0.5) * 2.0 * U * np.abs(d) + rnd(2, d),
            edges=[(0.0, "+0", "+inf")]),
        # pow(Dual, Dual) with a constant exponent: the rule of pow(Dual, double) (what q[0] ** q[1] is in every lane not seeded at q[1])
        Row("pow_dd_x", "pow(q, T(2.5))", None, lambda mp, x: mp.power(x, 2.5), lambda mp, x: 2.5 * mp.power(x, 1.5), P,
            lambda x, v, d: lib("pow", x, 2.5) * ulp(v),
            lambda x, v, d: max(lib("pow", x, 2.5), lib("pow", x, 1.5)) * 2.0 * U * np.abs(d) + rnd(2, d),
            edges=[(0.0, "+0", "+0")]),
        Row("pow_dd_int", "pow(q, T(3.0))", None, lambda mp, x: x ** 3, lambda mp, x: 3 * x ** 2, E,
            lambda x, v, d: lib("pow", x, 3.0) * ulp(v),
            lambda x, v, d: max(lib("pow", x, 3.0), lib("pow", x, 2.0)) * 2.0 * U * np.abs(d) + rnd(2, d),
            edges=[(-2.0, "finite", "finite"), (-0.75, "finite", "finite"), (0.0, "+0", "+0")]),
        # pow(Dual, Dual) with a constant base: f (1.0 log(1.5) + q 0.0 / 1.5) = f log(1.5): [library] pow and log, 2 roundings
        Row("pow_dd_y", "pow(T(1.5), q)", None, lambda mp, x: mp.power(1.5, x), lambda mp, x: mp.power(1.5, x) * mp.log(1.5), E,
            lambda x, v, d: lib("pow", np.full_like(x, 1.5), x) * ulp(v),
            lambda x, v, d: (lib("pow", np.full_like(x, 1.5), x) + lib("log", np.array([1.5]))) * 2.0 * U * np.abs(d) + rnd(2, d)),
        # ---- the project's own functions: [project] bounds against numpy / scipy + numpy's own error at the point
        Row("log", "log(q)", np.log, lambda mp, x: mp.log(x), lambda mp, x: 1 / x, P,
            lambda x, v, d: 2.0 * ulp(v) + _np_err(np.log, x, v),  # [project] 2 ulp of numpy (dual.cuh, log_fast)
            lambda x, v, d: rnd(1, d),  # [roundings] 1 / x: 1
            edges=[(0.0, "-inf", "+inf"), (-1.0, "nan", "finite"), (5e-324, "finite", "+inf"), (1e-310, "finite", "+inf"),
                   (math.inf, "+inf", "+0"), (math.nan, "nan", "nan")], lib_double=True),
        Row("log1p", "log1p(q)", np.log1p, lambda mp, x: mp.log1p(x), lambda mp, x: 1 / (1 + x), _log1p_points,
            lambda x, v, d: 2.0 * ulp(v) + _np_err(np.log1p, x, v),  # [project] 2 ulp of numpy (dual.cuh, log1p_fast)
            lambda x, v, d: rnd(2, d),  # [roundings] 1 / (1 + x): 2
            edges=[(-1.0, "-inf", "+inf"), (-2.0, "nan", "finite"), (2.0 ** -53, "finite", "finite"), (-2.0 ** -53, "finite", "finite"),
                   (1.797e308, "finite", "finite"), (0.0, "+0", "finite"), (-0.0, "-0", "finite")], lib_double=True),
        Row("lgamma", "lgamma(q)", _sp("gammaln"), _lgamma_f, lambda mp, x: mp.digamma(x), _gamma_points,
            lambda x, v, d: 1e-14 + 4.0 * ulp(v) + _np_err(_sp("gammaln"), x, v),  # [project] 1e-14 + 4 ulp of scipy (dual.cuh, lgamma_fast)
            lambda x, v, d: 5e-15 + 5e-14 * np.abs(d) + _np_err(_sp("digamma"), x, d),  # [project] rtol 5e-14, atol 5e-15 of scipy (test_dual.py)
            edges=[(0.0, "+inf", "-inf"), (-0.5, "finite", "finite"), (-2.5, "finite", "finite"), (1.0, "finite", "finite"),
                   (2.0, "finite", "finite"), (1e-300, "finite", "finite"), (1e300, "finite", "finite"), (5e-324, "finite", "-inf")], lib_double=True),
        Row("softplus", "softplus(q)", _softplus_np, lambda mp, x: mp.log1p(mp.exp(x)), lambda mp, x: 1 / (1 + mp.exp(-x)), W,
            lambda x, v, d: 4.0 * ulp(v) + _np_err(lambda z: np.logaddexp(0.0, z), x, v),  # [project] 4 ulp of numpy.logaddexp(0, x) (dual.cuh)
            lambda x, v, d: _logistic_va(x, d, d),  # its derivative is the logistic function: [project] 2e-15 relative of expit
            edges=[(745.0, "finite", "finite"), (-745.0, "finite", "finite"), (math.inf, "+inf", "finite"), (-math.inf, "+0", "+0")]),
        Row("logistic", "logistic(q)", _sp("expit"), lambda mp, x: 1 / (1 + mp.exp(-x)),
            lambda mp, x: mp.exp(-abs(x)) / (1 + mp.exp(-abs(x))) ** 2, W, _logistic_va, _logistic_da,
            edges=[(745.0, "finite", "+0"), (-745.0, "finite", "finite"), (math.inf, "finite", "+0"), (-math.inf, "+0", "+0")]),
        # ---- plain arithmetic: [roundings]
        Row("fabs", "fabs(q)", np.abs, lambda mp, x: abs(x), lambda mp, x: mp.mpf(-1 if x < 0 else 1), E,
            lambda x, v, d: 0.0 * v, lambda x, v, d: 0.0 * d,  # exact
            edges=[(0.0, "+0", "finite"), (-0.0, "+0", "finite")]),
        Row("square", "square(q)", np.square, lambda mp, x: x * x, lambda mp, x: 2 * x, E,
            lambda x, v, d: rnd(1, v), lambda x, v, d: 0.0 * d),  # x x: the reference's rounding alone; 2 x exact
        Row("recip", "1.0 / q", lambda x: 1.0 / x, lambda mp, x: 1 / x, lambda mp, x: -1 / (x * x), _nonzero,
            lambda x, v, d: rnd(1, v), lambda x, v, d: rnd(2, d)),  # v = 1 / x, then -v / x: 2
        Row("ratio", "q / (1.0 + q * q)", lambda x: x / (1.0 + x * x), lambda mp, x: x / (1 + x * x),
            lambda mp, x: (1 - x * x) / (1 + x * x) ** 2, E, lambda x, v, d: rnd(4, v), _ratio_da),  # x x, 1 +, /: 3 and the reference's
        # ---- the tracer's derived forms (tracing.py: _ufunc), written here as it writes them
        Row("log2", f"log(q) * {LOG2E!r}", np.log2, lambda mp, x: mp.log(x) / mp.log(2), lambda mp, x: 1 / (x * mp.log(2)), P,
            lambda x, v, d: (2.0 * ulp(np.log(x)) + _np_err(np.log, x, mp_eval_log(x))) * LOG2E * (1 + 4 * U) + rnd(4, v),  # [project] log, times a constant of 2 roundings, 1 product, the reference's
            lambda x, v, d: rnd(4, d), lib_double=True),  # (1 / x) c: 2 + the constant's 2
        Row("log10", f"log(q) * {LOG10E!r}", np.log10, lambda mp, x: mp.log(x) / mp.log(10), lambda mp, x: 1 / (x * mp.log(10)), P,
            lambda x, v, d: (2.0 * ulp(np.log(x)) + _np_err(np.log, x, mp_eval_log(x))) * LOG10E * (1 + 4 * U) + rnd(4, v),
            lambda x, v, d: rnd(4, d), lib_double=True),
        Row("exp2", f"exp(q * {LN2!r})", np.exp2, lambda mp, x: mp.power(2, x), lambda mp, x: mp.power(2, x) * mp.log(2), E,
            # the argument x c carries 2 roundings (the constant, the product) of size |x| ln 2: relative in the result; [library] exp
            lambda x, v, d: lib("exp", x * LN2) * 2.0 * U * np.abs(v) + rnd(2.0 * np.abs(x) * LN2 + 1, v),
            lambda x, v, d: lib("exp", x * LN2) * 2.0 * U * np.abs(d) + rnd(2.0 * np.abs(x) * LN2 + 3, d)),  # e c: 2 more
    ]
    return {r.name: r for r in rows}


@functools.lru_cache(maxsize=None)
def _log_ref(key):
    x = np.frombuffer(key, dtype=np.float64)
    mp = _mp()
    return mp_eval(lambda z: mp.log(z), x)


def mp_eval_log(x):
    return _log_ref(np.ascontiguousarray(x, dtype=np.float64).tobytes())


ROWS = _rows()
NAMES = list(ROWS)
TRACED = [n for n in NAMES if ROWS[n].np is not None]
SEED = 20240


@functools.lru_cache(maxsize=None)
def reference(name):
    """(points, f at 50 digits, f' at 50 digits, value allowance, derivative allowance) of a row: computed once per process"""
    row, mp = ROWS[name], _mp()
    x = np.asarray(row.points_fn(SEED + NAMES.index(name)), dtype=np.float64)
    assert 0 < len(x) <= 2000
    return (x,) + reference_at(name, x)


def reference_at(name, x):
    row, mp = ROWS[name], _mp()
    x = np.asarray(x, dtype=np.float64)
    v, d = mp_eval(lambda z: row.f(mp, z), x), mp_eval(lambda z: row.df(mp, z), x)
    assert np.isfinite(v).all() and np.isfinite(d).all(), name  # (the point sets hold finite references only: the rest are edges)
    with np.errstate(all="ignore"):
        va = np.asarray(row.va(x, v, d), dtype=np.float64) + np.zeros_like(x)
        da = np.asarray(row.da(x, v, d), dtype=np.float64) + 0.5 * ulp(d)
    for a in (va, da):
        a.flags.writeable = False
    v.flags.writeable = d.flags.writeable = False
    return v, d, va, da


def classify(g):
    g = float(g)
    if g != g:
        return "nan"
    if math.isinf(g):
        return "+inf" if g > 0 else "-inf"
    if g == 0.0:
        return "-0" if math.copysign(1.0, g) < 0 else "+0"
    return "finite"


def edge_ok(name, x, got, which, signed_zero=True):
    """an edge result `got` (`which`: 0 the value, 1 the derivative) is of the class the table expects at x; a finite
    class means within the allowance of the closed form there.  signed_zero=False: the route loses the sign of a zero."""
    row, mp = ROWS[name], _mp()
    want_cls = next(e for e in row.edges if _same(e[0], x))[1 + which]
    cls = classify(got)
    if want_cls != "finite":
        if not signed_zero and want_cls in ("+0", "-0"):
            return cls in ("+0", "-0")
        return cls == want_cls
    if cls not in ("finite", "+0", "-0"):
        return False
    xs = np.array([x], dtype=np.float64)
    v, d = mp_eval(lambda z: row.f(mp, z), xs), mp_eval(lambda z: row.df(mp, z), xs)
    with np.errstate(all="ignore"):
        a = (np.asarray(row.va(xs, v, d)) + np.zeros(1)) if which == 0 else (np.asarray(row.da(xs, v, d)) + 0.5 * ulp(d))
    return bool(abs(float(got) - (v, d)[which][0]) <= a[0])


def _same(a, b):
    return (a != a and b != b) or (a == b and math.copysign(1.0, a) == math.copysign(1.0, b))


def worst(name, x, got, want, allow):
    """(largest error in ulp of the reference, its argument, largest error / allowance, largest absolute error): what the
    measured-error tables record"""
    err = np.abs(got - want)
    with np.errstate(all="ignore"):
        u, r = err / ulp(want), np.where(err == 0.0, 0.0, err / np.where(allow > 0, allow, TINY))
    bad = ~np.isfinite(got)
    u, r = np.where(bad, np.inf, u), np.where(bad, np.inf, r)
    k = int(np.argmax(u))
    return float(u[k]), float(x[k]), float(np.max(r)), float(np.max(np.where(bad, np.inf, err)))


def check(name, x, got_v, got_d, want=None, what=""):
    """every point within the allowance; returns the measured (value, derivative) `worst` records"""
    _, v, d, va, da = reference(name) if want is None else (None,) + tuple(want)
    wv, wd = worst(name, x, got_v, v, va), worst(name, x, got_d, d, da)
    assert wv[2] <= 1.0, f"{what} {name}: value off by {wv[0]:.1f} ulp at x = {wv[1]!r}, {wv[2]:.2f} of the allowance"
    assert wd[2] <= 1.0, f"{what} {name}: derivative off by {wd[0]:.1f} ulp at x = {wd[1]!r}, {wd[2]:.2f} of the allowance"
    return wv, wd


def switch_source(names=None):
    """the body of one `switch (id)` over the rows' C++ expressions of `T q`"""
    names = NAMES if names is None else names
    return "\n".join(f"    case {NAMES.index(n)}: return T({ROWS[n].cpp});" for n in names)


# ---------------------------------------------------------------------------------------------- joint wrappers
def blocks(D, names):
    """coordinates 1 .. D-1 dealt to the rows in contiguous blocks of near-equal length: [(name, lo, hi)]"""
    n, k = len(names), D - 1
    assert k >= n
    out, lo = [], 1
    for j, name in enumerate(names):
        hi = lo + k // n + (1 if j < k % n else 0)
        out.append((name, lo, hi))
        lo = hi
    return out


def wrapper(layout):
    """lambda q: sum of f(q[block]).sum() over the blocks + q[0] * q[1:].sum() -- the coupling term keeps the density
    joint (a CustomJoint with its generated adjoint program); with q[0] = 0.0 exactly it adds exact zeros"""
    def fn(q):
        tot = None
        for name, lo, hi in layout:
            t = ROWS[name].np(q[lo:hi]).sum()
            tot = t if tot is None else tot + t
        return tot + q[0] * q[1:].sum()
    return fn


def joint_positions(layout, D, C=None):
    """positions [C, D] that walk every point of every row of the layout (q[0] = 0), the references and allowances per entry"""
    need = max(-(-len(reference(n)[0]) // (hi - lo)) for n, lo, hi in layout)
    C = need if C is None else C
    q = np.zeros((C, D))
    v, d, va, da = (np.zeros((C, D)) for _ in range(4))
    for name, lo, hi in layout:
        ref = reference(name)
        idx = (np.arange(C)[:, None] * (hi - lo) + np.arange(hi - lo)[None, :]) % len(ref[0])
        q[:, lo:hi] = ref[0][idx]
        for dst, src in zip((v, d, va, da), ref[1:]):
            dst[:, lo:hi] = src[idx]
    return q, v, d, va, da


def joint_sum_allowance(v, va):
    """the value of a joint wrapper against the 50-digit sum: the terms' allowances + (n - 1) roundings of the additions,
    each at most 2^-53 sum |t| (+ the reference sum's own rounding)"""
    n = v.shape[-1]
    return va.sum(-1) + n * U * (np.abs(v) + va).sum(-1)


def joint_sum(v):
    return np.array([math.fsum(r) for r in np.atleast_2d(v)])


def joint_edges(layout, D):
    """one position per edge of the layout's rows -- the edge argument in the first coordinate of its row's block, the first
    chain's points elsewhere: (positions [n, D], [(name, argument, coordinate)])"""
    base = joint_positions(layout, D, C=1)[0][0]
    meta = [(n, e[0], lo) for n, lo, hi in layout for e in ROWS[n].edges]
    q = np.tile(base, (len(meta), 1))
    for k, (_, x, i) in enumerate(meta):
        q[k, i] = x
    return q, meta


def check_joint_edges(layout, D, meta, value, grad, what="", others=True):
    """the gradient entry of every edge is of the expected class and leaves the other entries alone; the value is of the
    edge's class where that is NaN or infinite (NaN at an infinite argument: the coupling term is 0 * inf), else within
    the allowance of the sum with the edge's own closed form in its place"""
    _, v, d, va, da = joint_positions(layout, D, C=1)
    mp = _mp()
    for (name, x, i), val, g in zip(meta, value, grad):
        if others or not math.isinf(x):  # (forward mode: the coupling term's 0 * inf is in every lane's derivative as it is in the value)
            assert edge_ok(name, x, g[i], 1), (what, name, x, "derivative", g[i])
        rest = np.delete(np.arange(1, D), i - 1)
        # (reverse mode; in forward mode every lane differentiates every term, and 0 / nan or 0 / 0 in the edge's term reaches all of them)
        assert not others or np.all(np.abs(g[rest] - d[0][rest]) <= da[0][rest]), (what, name, x, "the other entries")
        cls = next(e for e in ROWS[name].edges if _same(e[0], x))[1]
        if math.isinf(x):
            assert classify(val) == "nan", (what, name, x, "value", val)
        elif cls in ("nan", "+inf", "-inf"):
            assert classify(val) == cls, (what, name, x, "value", val)
        else:
            xs = np.array([x])
            ev, ed = mp_eval(lambda z: ROWS[name].f(mp, z), xs), mp_eval(lambda z: ROWS[name].df(mp, z), xs)
            vv, aa = v[0].copy(), va[0].copy()
            with np.errstate(all="ignore"):
                vv[i], aa[i] = ev[0], (np.asarray(ROWS[name].va(xs, ev, ed)) + np.zeros(1))[0]
            assert abs(val - joint_sum(vv[1:])[0]) <= joint_sum_allowance(vv[1:], aa[1:]), (what, name, x, "value", val)
