"""aehmc_amd/transforms.py without a GPU: the numpy restatement of tests/transforms_ref.py against mpmath at 50 digits
(theta, ldj, the Jacobian, both round trips), the traced ``Model`` against the 50-digit closed form through the C++
harness of tests/test_tracing.py, the target class it traces to, and the errors.  (The kernel and summary.run:
tests/test_gpu_transforms.py.)"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import transforms_ref as tr  # noqa: E402
from dual_ref import U, _mp  # noqa: E402
from transforms_ref import INTERVAL, LOWER, ORDERED, REAL, SIMPLEX, UPPER  # noqa: E402

from aehmc_amd import targets, tracing  # noqa: E402
from aehmc_amd import transforms as tf  # noqa: E402

# the issue's arguments, and ordinary ones
EDGES = np.array([0.0, 1e-300, -1e-300, 40.0, -40.0, 708.0, -708.0, 750.0, -750.0, 1.0, -1.0, 0.3, -2.5, 17.0, -17.0])
POINTS = np.concatenate([EDGES, np.random.default_rng(3).normal(0.0, 3.0, 40)])
# bounds of mixed sign and magnitude (lo, hi)
BOUNDS = [(0.0, 1.0), (-1.0, 1.0), (-1e10, 2e-5), (1e-12, 3e-12), (-2.5, -1.25), (0.1, 0.3), (-3e-7, 5e8)]


def segments(n_in):
    """inputs of an Ordered / Simplex segment with n_in coordinates: ordinary, wide, and the edge arguments among them"""
    r = np.random.default_rng(100 + n_in)
    out = [r.normal(0.0, 1.0, n_in), r.normal(0.0, 3.0, n_in), r.uniform(-40.0, 40.0, n_in), np.zeros(n_in),
           np.resize(EDGES[:5], n_in), np.resize([708.0, -708.0, 1.0], n_in), np.resize([-750.0, 750.0, 0.3], n_in),
           np.full(n_in, -750.0), np.full(n_in, 750.0), np.resize([-708.0, -750.0, -40.0], n_in)]
    return out


def cases():
    """(kind, x, lo, hi) over every kind"""
    out = [(REAL, POINTS, 0.0, 0.0)]
    for lo, hi in BOUNDS:
        out += [(LOWER, POINTS, lo, 0.0), (UPPER, POINTS, 0.0, hi), (INTERVAL, POINTS, lo, hi)]
    r = np.random.default_rng(9)
    lo = r.normal(0.0, 10.0, POINTS.size)
    out.append((INTERVAL, POINTS, lo, lo + np.exp(r.normal(0.0, 4.0, POINTS.size))))  # bounds as arrays
    for n in (2, 64):
        out += [(ORDERED, x, 0.0, 0.0) for x in segments(n)]
        out += [(SIMPLEX, x, 0.0, 0.0) for x in segments(n - 1)]
    return out


CASES = cases()


@pytest.mark.parametrize("i", range(len(CASES)), ids=[f"{tr.NAMES[c[0]]}-{k}" for k, c in enumerate(CASES)])
def test_restatement_against_50_digits(i):
    kind, x, lo, hi = CASES[i]
    got = tr.theta_np(kind, x, lo, hi)
    want, allow = tr.theta_allowance(kind, x, lo, hi)
    ok = tr.within(got, want, allow)
    assert ok.all(), [(j, got[j], want[j], allow[j]) for j in np.flatnonzero(~ok)[:5]]
    if kind == INTERVAL:  # never outside the interval, and exactly the bound where exp(-|x|) underflows
        lo_v, hi_v = np.broadcast_to(lo, got.shape), np.broadcast_to(hi, got.shape)
        assert np.all((got >= lo_v) & (got <= hi_v))
        assert np.array_equal(got[x >= 750.0], hi_v[x >= 750.0]) and np.array_equal(got[x <= -750.0], lo_v[x <= -750.0])
    if kind == SIMPLEX and np.isfinite(got).all():
        assert abs(got.sum() - 1.0) <= allow.sum() + len(got) * U
    if kind == ORDERED:
        fin = np.isfinite(got)
        assert np.all(np.diff(got[fin]) >= 0.0)
    if kind in (LOWER, UPPER, INTERVAL):  # a coordinate-wise kind: one ldj per coordinate
        for j in range(len(x)):
            lo_j, hi_j = (np.broadcast_to(v, x.shape)[j] for v in (lo, hi))
            w, a = tr.ldj_allowance(kind, x[j:j + 1], lo_j, hi_j)
            assert abs(tr.ldj_np(kind, x[j:j + 1], lo_j, hi_j) - w) <= a, (x[j], w, a)
    w, a = tr.ldj_allowance(kind, x, lo, hi)
    assert abs(tr.ldj_np(kind, x, lo, hi) - w) <= a, (w, a)


def test_edge_classes_of_the_restatement():
    nan, inf = np.nan, np.inf
    assert np.isnan(tr.theta_np(LOWER, [nan], 1.0)).all() and np.isnan(tr.theta_np(INTERVAL, [nan], 0.0, 1.0)).all()
    assert tr.theta_np(LOWER, [750.0, inf], 1.0).tolist() == [inf, inf] and tr.theta_np(UPPER, [750.0], 0.0, 2.0)[0] == -inf
    assert tr.theta_np(INTERVAL, [inf, -inf, 750.0, -750.0], 0.1, 0.3).tolist() == [0.3, 0.1, 0.3, 0.1]
    assert np.isnan(tr.theta_np(SIMPLEX, [0.0, inf, 1.0])).all() and np.isnan(tr.theta_np(SIMPLEX, [0.0, nan])).all()
    assert tr.theta_np(SIMPLEX, [0.0, -inf]).tolist() == [0.5, 0.0, 0.5]
    o = tr.theta_np(ORDERED, [1.0, 0.0, nan, 0.0])
    assert o[:2].tolist() == [1.0, 2.0] and np.isnan(o[2:]).all()


JAC = [(REAL, [0.3, -1.2], 0.0, 0.0), (LOWER, [0.3, -1.2], [-2.0, 5.0], 0.0), (UPPER, [0.3, 2.2], 0.0, [-2.0, 5.0]),
       (INTERVAL, [0.3, -4.2, 6.0], [-2.0, 5.0, 0.0], [-1.0, 9.5, 1e3]), (ORDERED, [0.3, -1.2, 2.0, 0.1], 0.0, 0.0),
       (SIMPLEX, [0.3, -1.2, 2.0], 0.0, 0.0), (SIMPLEX, [-3.0], 0.0, 0.0), (ORDERED, [5.0, -7.0], 0.0, 0.0)]


@pytest.mark.parametrize("kind,x,lo,hi", JAC, ids=[f"{tr.NAMES[c[0]]}{len(c[1])}" for c in JAC])
def test_ldj_is_the_log_determinant_of_the_jacobian(kind, x, lo, hi):
    """J formed by mpmath differentiation of the 50-digit theta (Simplex: its first K - 1 outputs, the last one being
    1 - their sum); mpmath's derivative is good to about half the working precision, the test asks for 1e-20."""
    mp = _mp()
    n = len(x)
    xs = [mp.mpf(v) for v in x]

    def out(i, j, t):
        return tr.theta_mp(kind, xs[:j] + [t] + xs[j + 1:], lo, hi)[i]

    J = mp.matrix(n, n)
    for i in range(n):
        for j in range(n):
            J[i, j] = mp.diff(lambda t, i=i, j=j: out(i, j, t), xs[j])
    assert abs(mp.log(abs(mp.det(J))) - tr.ldj_mp(kind, x, lo, hi)) < mp.mpf("1e-20")


# ---- round trips.  The bound is the condition number times the allowance, not a fitted number: with a_i the allowance of
# theta_i (transforms_ref.theta_allowance) and own_j what the inverse's own operations add to x_j,
#   |x'_j - x_j| <= sum_i |dx_j / dtheta_i| a_i + own_j          (unconstrain after constrain)
#   |theta'_i - theta_i| <= sum_j |dtheta_i / dx_j| own_j + a_i    (constrain after unconstrain)
# own_j: the inverse is a subtraction or a quotient (relative error <= 3 U, carried into x by the derivative of log or
# logit) and one or two logarithms (numpy's, <= 4 ulp of a value no larger than M_j); 16 U (1 + M_j + carry_j) covers it.
def inverse_jacobian_abs(kind, x, theta, lo, hi):
    """|dx_j / dtheta_i| as a matrix [n_in, n_out]"""
    n_in, n_out = len(x), len(theta)
    Ji = np.zeros((n_in, n_out))
    if kind == REAL:
        np.fill_diagonal(Ji, 1.0)
    elif kind in (LOWER, UPPER):
        np.fill_diagonal(Ji, np.exp(-x))
    elif kind == INTERVAL:
        s = 1.0 / (1.0 + np.exp(-x))
        np.fill_diagonal(Ji, 1.0 / ((np.asarray(hi) - lo) * s * (1.0 - s)))
    elif kind == ORDERED:
        Ji[0, 0] = 1.0
        for j in range(1, n_in):
            Ji[j, j] = Ji[j, j - 1] = np.exp(-x[j])
    else:
        for j in range(n_in):
            Ji[j, j], Ji[j, n_out - 1] = 1.0 / theta[j], 1.0 / theta[-1]
    return Ji


def jacobian_abs(kind, x, theta, lo, hi):
    """|dtheta_i / dx_j| [n_out, n_in]"""
    n_in, n_out = len(x), len(theta)
    J = np.zeros((n_out, n_in))
    if kind == REAL:
        np.fill_diagonal(J, 1.0)
    elif kind in (LOWER, UPPER):
        np.fill_diagonal(J, np.exp(x))
    elif kind == INTERVAL:
        s = 1.0 / (1.0 + np.exp(-x))
        np.fill_diagonal(J, (np.asarray(hi) - lo) * s * (1.0 - s))
    elif kind == ORDERED:
        J[:, 0] = 1.0
        for j in range(1, n_in):
            J[j:, j] = np.exp(x[j])
    else:
        for i in range(n_out):
            for j in range(n_in):
                J[i, j] = theta[i] * abs((i == j) - theta[j])
    return J


def own(kind, x, theta, lo, hi):
    if kind == REAL:
        return np.zeros(len(x))
    if kind in (LOWER, UPPER):
        bound = np.abs(lo if kind == LOWER else hi)
        return 16 * U * (1.0 + np.abs(x) + (np.abs(theta) + bound) * np.exp(-x))  # (theta - lo is not exact: both operands' size)
    if kind == INTERVAL:
        w = np.asarray(hi) - lo
        u = (theta - lo) / w
        return 16 * U * (1.0 + np.abs(x) + (np.abs(theta) + np.abs(lo) + np.abs(hi)) / (w * u * (1.0 - u)))
    if kind == ORDERED:
        o = np.zeros(len(x))
        o[1:] = 16 * U * (1.0 + np.abs(x[1:]) + (np.abs(theta[1:]) + np.abs(theta[:-1])) * np.exp(-x[1:]))
        return o
    return 16 * U * (1.0 + np.abs(np.log(theta[:-1])) + abs(np.log(theta[-1])))


TRIPS = ([(REAL, 5, 0.0, 0.0), (LOWER, 8, -3.0, 0.0), (LOWER, 8, 25.0, 0.0), (UPPER, 8, 0.0, 0.7), (INTERVAL, 8, -1.0, 1.0),
          (INTERVAL, 8, 0.1, 0.3), (INTERVAL, 8, -2.5, 40.0), (ORDERED, 2, 0.0, 0.0), (ORDERED, 64, 0.0, 0.0),
          (SIMPLEX, 1, 0.0, 0.0), (SIMPLEX, 5, 0.0, 0.0), (SIMPLEX, 63, 0.0, 0.0)])


@pytest.mark.parametrize("kind,n_in,lo,hi", TRIPS, ids=[f"{tr.NAMES[c[0]]}{c[1]}-{k}" for k, c in enumerate(TRIPS)])
def test_round_trips(kind, n_in, lo, hi):
    for seed in range(5):
        x = np.random.default_rng(seed).normal(0.0, 2.0, n_in)  # (well conditioned: exp(-x) and 1 / (s (1 - s)) stay below 10^4)
        theta = tr.theta_np(kind, x, lo, hi)
        _, a = tr.theta_allowance(kind, x, lo, hi)
        o = own(kind, x, theta, lo, hi)
        back = tr.inverse_np(kind, theta, lo, hi)
        bound = inverse_jacobian_abs(kind, x, theta, lo, hi) @ a + o
        assert np.all(np.abs(back - x) <= bound), (np.abs(back - x) / bound).max()
        assert bound.max() < 1e-7  # (the inputs are well conditioned -- the bound itself says so; Ordered(64): sums of hundreds over gaps of exp(-4))
        # constrain(unconstrain(theta)): theta is the exact input now, x2 carries own, the forward map its allowance
        x2 = tr.inverse_np(kind, theta, lo, hi)
        again = tr.theta_np(kind, x2, lo, hi)
        _, a2 = tr.theta_allowance(kind, x2, lo, hi)
        bound2 = jacobian_abs(kind, x2, theta, lo, hi) @ o + a2
        assert np.all(np.abs(again - theta) <= bound2), (np.abs(again - theta) / bound2).max()


def test_exact_marginals_criterion_at_this_sample_size():
    """Before the NUTS run of tests/test_gpu_transforms.py is held to it: independent numpy draws from the exact marginals, 1024 chains x 200 draws, pass
    the criterion (|z| < 4 with the standard error from the spread of the chain means) for every mean and second moment,
    and the exact values above are the right ones."""
    r = np.random.default_rng(7)
    C, N = 1024, 200
    mu = np.sort(r.normal(size=(N, C, 2)), axis=-1)
    theta = np.concatenate([r.gamma(3.0, 0.5, (N, C, 1)), 2.0 * r.beta(2.0, 3.0, (N, C, 1)) - 1.0, r.dirichlet([2.0, 3.0, 4.0], (N, C)),
                            mu, r.normal(size=(N, C, 3))], axis=-1)
    for stat, exact in ((theta, tr.EXACT_MEAN), (theta * theta, tr.EXACT_SQUARE)):
        m = stat.mean(axis=0)
        z = (m.mean(axis=0) - exact) / (m.std(axis=0, ddof=1) / np.sqrt(C))
        assert np.all(np.abs(z) < 4.0), z



# ---- the Model
A_DIR = np.array([1.0, 2.0, 3.0])


def mixed_logprob(w, sigma, ub, rho, pi, mu):
    return (-0.5 * np.sum(w * w) + np.sum(2.0 * np.log(sigma) - 2.0 * sigma) - 0.5 * ub * ub + np.log1p(rho) + 2.0 * np.log1p(-rho)
            + np.sum(A_DIR * np.log(pi)) - 0.5 * np.sum(mu * mu))


MIXED = [("w", REAL, 3, 0.0, 0.0), ("sigma", LOWER, 2, np.array([0.0, 0.5]), 0.0), ("ub", UPPER, (), 0.0, 2.0),
         ("rho", INTERVAL, (), -1.0, 1.0), ("pi", SIMPLEX, 3, 0.0, 0.0), ("mu", ORDERED, 3, 0.0, 0.0)]


def mixed_model(**kw):
    return tf.Model({"w": tf.Real(3), "sigma": tf.LowerBound(np.array([0.0, 0.5]), 2), "ub": tf.UpperBound(2.0),
                     "rho": tf.Interval(-1.0, 1.0), "pi": tf.Simplex(3), "mu": tf.Ordered(3)}, mixed_logprob, **kw)


def mixed_closed_form(q, jacobian=True):
    """(value, sum of the absolute addends) at 50 digits; q: a list of mpf"""
    mp = tr._ctx()
    a, th, ldj = 0, {}, mp.mpf(0)
    for name, kind, n, lo, hi in MIXED:
        n_in = (n if n != () else 1) - (kind == SIMPLEX)
        th[name] = tr.theta_mp(kind, q[a:a + n_in], lo, hi)
        ldj += tr.ldj_mp(kind, q[a:a + n_in], lo, hi)
        a += n_in
    terms = ([-v * v / 2 for v in th["w"]] + [2 * mp.log(s) for s in th["sigma"]] + [-2 * s for s in th["sigma"]]
             + [-th["ub"][0] ** 2 / 2, mp.log1p(th["rho"][0]), 2 * mp.log1p(-th["rho"][0])]
             + [mp.mpf(float(c)) * mp.log(p) for c, p in zip(A_DIR, th["pi"])] + [-v * v / 2 for v in th["mu"]])
    if jacobian:
        terms.append(ldj)
    return mp.fsum(terms), mp.fsum(abs(t) for t in terms) + (mp.fsum(abs(v) for v in q) if jacobian else 0)


@pytest.mark.parametrize("jacobian", [True, False], ids=["jacobian", "no_jacobian"])
def test_traced_model_value_and_gradient_against_the_closed_form(tmp_path, jacobian):
    """The model mixes all six kinds.  Allowance: the traced program forms the value from fewer than 256 operations, each
    rounded at 2^-53 relative to an intermediate no larger than A = the sum of the absolute addends (the ldj's own
    addends |q_j| included) -- 256 U A; a derivative passes through the same operations with the factor of each, at most
    twice as many roundings, against B = max(1, the largest |gradient entry|) A -- 512 U B.  Forward and reverse mode."""
    from test_tracing import run_cpp, run_cpp_reverse
    mp = _mp()
    model = mixed_model(include_jacobian=jacobian)
    assert (model.dim, model.constrained_dim) == (12, 13)
    t = tracing.trace(model, model.dim, reverse=True)
    assert not t.elementwise and t.dim == 12
    for trial in range(2):
        q = 0.7 * np.random.default_rng(trial).normal(size=model.dim)
        qm = [mp.mpf(float(v)) for v in q]
        want, A = mixed_closed_form(qm, jacobian)
        grad = [mp.diff(lambda s, j=j: mixed_closed_form(qm[:j] + [s] + qm[j + 1:], jacobian)[0], qm[j]) for j in range(model.dim)]
        want, A, grad = float(want), float(A), np.array([float(g) for g in grad])
        B = max(1.0, np.abs(grad).max()) * A
        assert abs(float(model(q)) - want) <= 256 * U * A  # (the same expression on a plain numpy vector)
        for name, (v, g) in (("forward", run_cpp(t, q, tmp_path, f"m{trial}")), ("reverse", run_cpp_reverse(t, q, tmp_path, f"m{trial}"))):
            print(name, "value error / allowance", abs(v - want) / (256 * U * A), "gradient", (np.abs(g - grad) / (512 * U * B)).max())
            assert abs(v - want) <= 256 * U * A, name
            assert np.all(np.abs(g - grad) <= 512 * U * B), name


def test_target_classes():
    """one vector parameter, a coordinate-wise transform, a density that is one sum over it: targets.Custom (every kernel
    family); a scalar parameter likewise; anything with a segment transform or several parameters: CustomJoint"""
    lo = np.arange(7.0)
    for t in (tf.Positive(7), tf.LowerBound(lo, 7), tf.UpperBound(3.0, 7), tf.Interval(lo, lo + 2.0, 7), tf.Real(7)):
        model = tf.Model({"s": t}, lambda s: np.sum(-0.5 * (s - 1.0) ** 2))
        tgt = targets.from_callable(model, 7)
        assert isinstance(tgt, targets.Custom) and tgt.dim == 7, t
        assert targets.as_target(model, 7) is targets.as_target(model, 7)  # one trace per model
    one = tf.Model({"s": tf.Positive()}, lambda s: 2.0 * np.log(s) - 2.0 * s)
    assert isinstance(targets.from_callable(one, 1), targets.Custom)
    assert isinstance(targets.from_callable(one, 1, scalar=True), targets.Custom)
    assert isinstance(targets.from_callable(mixed_model(), 12), targets.CustomJoint)
    # the fused Jacobian term: the per-coordinate expression is the density's term plus x
    src = tracing.trace(tf.Model({"s": tf.Positive(7)}, lambda s: np.sum(2.0 * np.log(s) - 2.0 * s)), 7).source
    assert "+ q)" in src and "exp(q)" in src
    q = np.random.default_rng(0).normal(size=7)
    model = tf.Model({"s": tf.Positive(7)}, lambda s: np.sum(2.0 * np.log(s) - 2.0 * s))
    assert float(model(q)) == pytest.approx(float(np.sum(2.0 * q - 2.0 * np.exp(q)) + q.sum()), rel=1e-14)


def test_layout_table_and_unconstrain():
    import torch
    model = mixed_model()
    assert model.params_map.size == 13 and model.params_map.ref_params == ("w", "sigma", "ub", "rho", "pi", "mu")
    tab = model.table
    assert tab.dtype.itemsize == 40 and len(tab) == 13
    assert tab["kind"].tolist() == [0, 0, 0, 1, 1, 2, 3, 5, 5, 5, 4, 4, 4]
    assert tab["first"].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 7, 7, 9, 9, 9] and tab["pos"].tolist() == [0] * 7 + [0, 1, 2, 0, 1, 2]
    assert tab["len"].tolist() == [1] * 7 + [3] * 6 and tab["lo"][4] == 0.5 and tab["hi"][5] == 2.0 and tab["lo"][6] == -1.0
    y = np.arange(26.0).reshape(2, 13)
    un = model.unravel(y)
    assert un["pi"].shape == (2, 3) and un["ub"].shape == (2,) and un["mu"][1].tolist() == [23.0, 24.0, 25.0]
    r = np.random.default_rng(2)
    x = r.normal(0.0, 1.5, (5, 12))
    theta = np.stack([np.concatenate([tr.theta_np(k, row[s], lo, hi) for (_, k, _, lo, hi), s in
                                      zip(MIXED, (slice(0, 3), slice(3, 5), slice(5, 6), slice(6, 7), slice(7, 9), slice(9, 12)))])
                      for row in x])
    back = model.unconstrain({k: torch.as_tensor(v) for k, v in model.unravel(theta).items()})
    assert back.dtype == torch.float64 and tuple(back.shape) == (5, 12)
    np.testing.assert_allclose(back.numpy(), x, rtol=0, atol=1e-9)  # (the bound itself: test_round_trips)
    single = model.unconstrain({k: v[0] for k, v in model.unravel(theta).items()})
    assert tuple(single.shape) == (12,) and np.array_equal(single.numpy(), back[0].numpy())


def test_errors():
    import torch
    with pytest.raises(ValueError, match=r"\[2, 64\]"):
        tf.Ordered(65)
    with pytest.raises(ValueError, match=r"\[2, 64\]"):
        tf.Simplex(65)
    with pytest.raises(ValueError, match=r"\[2, 64\]"):
        tf.Simplex(1)
    for make in (lambda: tf.Real((2, 3)), lambda: tf.Positive((2, 2)), lambda: tf.Interval(0.0, 1.0, (4, 1))):
        with pytest.raises(ValueError, match="scalar.*or a vector"):
            make()
    with pytest.raises(ValueError, match="lo >= hi"):
        tf.Interval(1.0, 1.0)
    with pytest.raises(ValueError, match="lo >= hi"):
        tf.Interval(np.array([0.0, 2.0]), np.array([1.0, 1.5]), 2)
    with pytest.raises(ValueError, match="shape"):
        tf.LowerBound(np.zeros(3), 2)
    model = mixed_model()
    good = {"w": np.zeros(3), "sigma": [0.5, 1.5], "ub": 1.0, "rho": 0.3, "pi": [0.2, 0.3, 0.5], "mu": [-1.0, 0.0, 2.0]}
    assert tuple(model.unconstrain(good).shape) == (12,)
    for name, bad in (("sigma", [0.5, 0.5]), ("ub", 2.0), ("rho", -1.0), ("rho", np.nan), ("pi", [0.2, 0.3, 0.6]),
                      ("pi", [0.7, 0.5, -0.2]), ("mu", [0.0, 0.0, 1.0])):
        with pytest.raises(ValueError, match=f"unconstrain: {name} "):
            model.unconstrain({**good, name: bad})
    with pytest.raises(ValueError, match="a value for each of"):
        model.unconstrain({"w": np.zeros(3)})
    with pytest.raises(ValueError, match="12 unconstrained coordinates"):
        model(np.zeros(10))
    with pytest.raises(ValueError, match=r"\[\.\.\., 12\]"):
        model.constrain(torch.zeros(4, 10, dtype=torch.float64))
    with pytest.raises(ValueError, match="float64"):
        model.constrain(torch.zeros(4, 12, dtype=torch.float32))
    from aehmc_amd import summary

    class Kernel:
        num_chains, batched = 4, True

        def sample(self, *a, **k):
            raise AssertionError("not reached")

    class State:
        position = torch.zeros(4, 10, dtype=torch.float64)

    with pytest.raises(ValueError, match="positions of 12 coordinates, the chains have 10"):
        summary.run(Kernel(), State(), 0.1, 1.0, 10, constrain=model)
    with pytest.raises(ValueError, match="must be a transforms.Model"):
        summary.run(Kernel(), State(), 0.1, 1.0, 10, constrain=lambda x: x)
