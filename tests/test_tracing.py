"""aehmc_amd/tracing.py: a Python ``logprob_fn`` (reference: README.md:27-36, aehmc/hmc.py:16-40) traced into the
``aehmc_logp`` template.  The emitted source is compiled as plain C++ against csrc/dual.cuh (the way tests/test_dual.py
does) and evaluated with double and with Dual: value == the Python function on plain numpy arrays, gradient == central
differences of it.  (The GPU side -- the same sources through hipRTC, whole transitions against the numpy
restatement -- is tests/test_gpu_callable.py.)"""
import os
import subprocess

import numpy as np
import pytest

from aehmc_amd import targets, tracing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = np.random.default_rng(5)
NU, SC = 3.0 + 5 * R.random(7), 0.5 + R.random(7)
LOC = np.array([0.0, 3.0])
PREC = np.linalg.inv(np.array([[1.0, 1.0], [1.0, 4.0]]))
A6 = R.normal(size=(4, 6))
Y4 = R.normal(size=4)


def student_t(q):
    return (-0.5 * (NU + 1.0) * np.log1p((q / SC) ** 2 / NU)).sum()


def mvn(y):
    return -0.5 * (y - LOC) @ (PREC @ (y - LOC))


def funnel(q):
    v, x = q[0], q[1:]
    return -v * v / 18.0 + (-0.5 * x * x * np.exp(-v) - 0.5 * v).sum()


def regression(q):  # a small linear model with a matrix captured from the closure, sigma = exp(q[-1])
    w, ls = q[:-1], q[-1]
    r = Y4 - A6[:, :5] @ w
    return -0.5 * np.sum(r * r) * np.exp(-2.0 * ls) - 4 * ls - 0.5 * np.dot(w, w) - 0.5 * ls**2


def kitchen_sink(q):
    a = np.tanh(q[0]) + np.sin(q[1]) * np.cos(q[2]) + np.sqrt(1.0 + np.square(q[3])) + np.expm1(-np.abs(q[4]))
    b = tracing.where(q[0] > 0.1, q[0] ** 3, -q[0]) + np.maximum(q[1], q[2]) + np.minimum(q[3], 0.3) + np.logaddexp(q[4], q[0])
    c = tracing.softplus(q[1]) + 2.0 ** q[2] + np.power(1.5 + q[3] ** 2, 0.3) + (1.0 / (2.0 + q[4] ** 2)) + np.mean(q) + sum(q[1:3])
    return a + b - c + (q @ q) * 0.1


def gamma_mixture(q):  # Gamma(shape = exp(q[0]), rate = exp(q[1])) observations: lgamma of a traced shape parameter
    from scipy.special import gammaln
    a, b = np.exp(q[0]), np.exp(q[1])
    x = np.exp(q[2:])
    return np.sum(a * q[1] - gammaln(a) + (a - 1.0) * q[2:] - b * x) + q[2:].sum() - 0.5 * (q[0] ** 2 + q[1] ** 2)


XL = R.normal(size=(300, 5)) / 2.0
YL = (R.random(300) < 0.5).astype(np.float64)


def logistic(q):  # a data matrix captured from the closure: z = X @ q is ONE node used twice (value and adjoint merged)
    z = XL @ q
    return (YL * z - tracing.softplus(z)).sum() - 0.5 * (q @ q) / 4.0


def bernoulli_expit(q):  # scipy.special.expit as the link function: log p = y log s + (1 - y) log(1 - s), s = expit(X q)
    from scipy.special import expit
    s = expit(XL @ q)
    return np.sum(YL * np.log(s) + (1.0 - YL) * np.log1p(-s)) - 0.5 * np.sum(q * q)


def more_functions(q):  # the later additions: arctan sinh cosh erfc log2 log10 exp2
    from scipy.special import erfc
    return (np.arctan(q[0] * q[1]) + 0.1 * np.sinh(q[2]) - 0.05 * np.cosh(q[3] - q[0]) + np.log(0.5 * erfc(q[4] * 0.7)) + np.log2(1.0 + q[1] ** 2)
            - np.log10(2.0 + q[2] ** 2) + 0.01 * np.exp2(q[3]) - 0.5 * np.sum(q * q))


def numpy_idioms(q):  # norm / clip / sign / var / std / diff / max / min / T / reshape / zeros_like / logaddexp.reduce / concatenate
    a = -np.linalg.norm(q) + np.sum(np.clip(q, -0.4, 0.6) ** 2) + np.sum(np.sign(q) * q) * 0.1 - np.var(q) - 0.3 * np.std(q[1:], ddof=1)
    b = -np.sum(np.diff(q) ** 2) + 0.2 * np.max(q) - 0.1 * q.min() + q.T @ q * 0.05 - np.sum((q.reshape(-1) - np.zeros_like(q)) ** 2) * 0.01
    c = np.logaddexp.reduce(q[:4]) - np.sum(np.concatenate([q[:2], q[4:]]) ** 2) * 0.07 + np.sum(np.stack([q[0], q[2]]) * np.array([0.3, -0.2]))
    return a + b + c


XS = R.normal(size=(50, 4))
YS = np.eye(3)[R.integers(0, 3, size=50)]


def softmax_regression(q):  # a matrix-valued parameter written as a list of its rows: W[k] = q[4 k : 4 k + 4], logits_k = X @ W[k]
    logits = [XS @ q[4 * k:4 * k + 4] for k in range(3)]
    picked = sum((YS[:, k] * logits[k]).sum() for k in range(3))
    return picked - np.sum(tracing.logsumexp(logits)) - 0.5 * np.sum(q * q) / 9.0


def shared_under_where(q):  # a shared sub-expression with a use inside a where-branch (never merged: see _RevGen.count_uses)
    u = np.exp(q[:3]) + q[3:6] ** 2
    return np.sum(tracing.where(q[:3] > 0.1, u * q[3:6], -u) + np.sin(u)) - 0.5 * np.sum(q * q)


GROUP = R.integers(0, 7, size=120)
YG = R.normal(size=120) + GROUP * 0.3


def hierarchical(q):  # random effects by group: theta[group] is a gather through a captured integer array
    mu, lt, theta = q[0], q[1], q[2:]
    tau = np.exp(lt)
    r = YG - theta[GROUP]
    return (-0.5 * mu * mu / 25.0 + lt - 0.5 * tau * tau / 4.0 - 7 * lt - 0.5 * np.sum((theta - mu) ** 2) / (tau * tau)
            - 0.5 * np.sum(r * r) + np.sum(np.tanh(q[2:][GROUP[:30]]) * YG[:30]))


def shared_in_comparison(q):  # a shared node whose other use is a comparison only (which passes no adjoint on)
    z = XL[:40] @ q
    return np.sum(tracing.where(z > 0.1, YL[:40], -YL[:40]) * 0.3 + z * z) + np.sum(tracing.where(q > 0.0, 1.0, 2.0) * q)


OBS = R.normal(size=60) * 2.0


def mixture(q):  # three-component Gaussian mixture: means q[0:3], log-scales q[3:6], unnormalised log-weights q[6:9]
    mu, ls, lw = q[0:3], q[3:6], q[6:9]
    comp = [lw[k] - ls[k] - 0.5 * ((OBS - mu[k]) * np.exp(-ls[k])) ** 2 for k in range(3)]   # per observation, component k
    return np.sum(tracing.logsumexp(comp)) - 60 * tracing.logsumexp(lw) - 0.5 * np.sum(q * q) / 9.0


# ---- reductions that are named and used again (s = (x * x).sum(); -s + 3 log s): one `sum` node with several parents.
# Each entry: the Python density and its closed form -- value and gradient over a plain list `x` of numbers of any kind,
# `m` supplying log / log1p / sqrt / exp for that kind (numpy for float64, mpmath for the 50-digit reference).
def _tot(xs):
    return sum(xs[1:], xs[0])


def sh_log_of_sum(x):
    s = (x * x).sum()
    return -s + 3 * np.log(s)


def cf_log_of_sum(x, m):
    s = _tot([v * v for v in x])
    return -s + 3 * m.log(s), [(-1 + 3 / s) * 2 * v for v in x]


def sh_sum_twice(x):
    s = (x * x).sum()
    return -(s + s)


def cf_sum_twice(x, m):
    s = _tot([v * v for v in x])
    return -(s + s), [-4 * v for v in x]


def sh_centred(x):  # a sum on the spine AND inside the body of another reduction
    s = x.sum()
    return s - ((x - s) ** 2).sum()


def cf_centred(x, m):
    s = _tot(x)
    d = [v - s for v in x]
    sd = _tot(d)
    return s - _tot([v * v for v in d]), [1 - 2 * v + 2 * sd for v in d]


def sh_where_spine(x):  # a sum on the spine AND in both branches of a where
    s = (x * x).sum()
    return tracing.where(s > 1, -s, -s * s) - s


def cf_where_spine(x, m):
    s = _tot([v * v for v in x])
    c = -2 if s > 1 else -2 * s - 1
    return (-s if s > 1 else -s * s) - s, [c * 2 * v for v in x]


def sh_var_twice(x):  # a shared value over a reduction with a hoisted sub-expression (the mean): one loop, one declaration
    v = x.var()
    return -v - np.log(v) - 0.05 * (x * x).sum()


def cf_var_twice(x, m):
    n = len(x)
    mean = _tot(x) / n
    d = [v - mean for v in x]
    var = _tot([v * v for v in d]) / n
    return -var - m.log(var) - 0.05 * _tot([v * v for v in x]), [(-1 - 1 / var) * 2 * dv / n - 0.1 * v for dv, v in zip(d, x)]


def sh_where_shared(x):  # a sum with a hoisted sub-expression swept twice in one where branch: accumulators named per sweep
    s = ((x - x[0]) ** 2).sum()
    return tracing.where(x[1] > 0.5, s * 2, s * s) - 0.5 * (x * x).sum()


def cf_where_shared(x, m):
    d = [v - x[0] for v in x]
    s = _tot([v * v for v in d])
    c = 2 if x[1] > 0.5 else 2 * s
    ds = [2 * v for v in d]
    ds[0] = -2 * _tot(d)
    return (s * 2 if x[1] > 0.5 else s * s) - 0.5 * _tot([v * v for v in x]), [c * dv - v for dv, v in zip(ds, x)]


def sh_spine_and_inner(x):
    s = (x * x).sum()
    return -s - 0.1 * ((x - 0.1 * s) ** 2).sum()


def cf_spine_and_inner(x, m):
    s = _tot([v * v for v in x])
    d = [v - 0.1 * s for v in x]
    sd = _tot(d)
    return -s - 0.1 * _tot([v * v for v in d]), [-2 * v - 0.2 * dv + 0.04 * v * sd for dv, v in zip(d, x)]


def sh_three_uses(x):
    s = (x * x).sum()
    return -s + np.log(s) - 0.1 * np.sqrt(s)


def cf_three_uses(x, m):
    s = _tot([v * v for v in x])
    return -s + m.log(s) - 0.1 * m.sqrt(s), [(-1 + 1 / s - 0.05 / m.sqrt(s)) * 2 * v for v in x]


def sh_cmp_only(x):  # the other use is a comparison, which passes no adjoint on: the sum stays fused
    s = (x * x).sum()
    return -s + tracing.where(s > 1, 1.0, 2.0) * x[0]


def cf_cmp_only(x, m):
    s = _tot([v * v for v in x])
    c = 1 if s > 1 else 2
    g = [-2 * v for v in x]
    g[0] = g[0] + c
    return -s + c * x[0], g


def sh_lets_hoisted(x):  # exp(-a) is hoisted out of the shared sum's loop: its adjoint accumulator goes with the sum
    a = x[0]
    s = ((x[1:] * np.exp(-a)) ** 2).sum()
    return -s - np.log1p(s) - 0.5 * a * a


def cf_lets_hoisted(x, m):
    a = x[0]
    u = m.exp(-a)
    s = _tot([(v * u) * (v * u) for v in x[1:]])
    f = -1 - 1 / (1 + s)
    return -s - m.log1p(s) - 0.5 * a * a, [f * (-2 * s) - a] + [f * 2 * u * u * v for v in x[1:]]


SHARED = {"shared_log_of_sum": (sh_log_of_sum, cf_log_of_sum), "shared_sum_twice": (sh_sum_twice, cf_sum_twice),
          "shared_centred": (sh_centred, cf_centred), "shared_where_spine": (sh_where_spine, cf_where_spine),
          "shared_var_twice": (sh_var_twice, cf_var_twice), "shared_where_shared": (sh_where_shared, cf_where_shared),
          "shared_spine_and_inner": (sh_spine_and_inner, cf_spine_and_inner), "shared_three_uses": (sh_three_uses, cf_three_uses),
          "shared_cmp_only": (sh_cmp_only, cf_cmp_only), "shared_lets_hoisted": (sh_lets_hoisted, cf_lets_hoisted)}


CASES = {"student_t": (student_t, 7, True), "hierarchical": (hierarchical, 9, False), "mixture": (mixture, 9, False), "shared_in_comparison": (shared_in_comparison, 5, False), "gamma": (gamma_mixture, 6, False), "logistic": (logistic, 5, False), "bernoulli_expit": (bernoulli_expit, 5, False), "more_functions": (more_functions, 5, False), "numpy_idioms": (numpy_idioms, 6, False), "softmax_regression": (softmax_regression, 12, False),
         "shared_under_where": (shared_under_where, 6, False), "mvn": (mvn, 2, False), "funnel": (funnel, 10, False),
         "regression": (regression, 6, False), "kitchen_sink": (kitchen_sink, 5, False)}
CASES.update({name: (fn, 6, False) for name, (fn, _) in SHARED.items()})


def shared_rows_in_where(q):  # a shared sum over data rows (per-lane accumulators for q through X @ q) swept twice in one where branch
    z = XL[:40] @ q
    s = (z * z).sum()
    return tracing.where(q[0] > 0.1, -s, -0.5 * s * s) - 0.5 * (q * q).sum()


CASES["shared_rows_in_where"] = (shared_rows_in_where, 5, False)

HARNESS = r"""
#include <cstdio>
#include <cmath>
#define __device__
#include "dual.cuh"
using aehmc::Dual;
%(source)s
template <class T> struct Row {
  const double *q; int seed, D;
  T operator[](int i) const;
  int size() const { return D; }
};
template <> double Row<double>::operator[](int i) const { return q[i]; }
template <> Dual Row<Dual>::operator[](int i) const { return Dual(q[i], i == seed ? 1.0 : 0.0); }
%(params)s
int main() {
  const int D = %(D)d;
  const double q[] = {%(q)s};
#if %(elem)d
  double v = 0.0;
  for (int i = 0; i < D; i++) v += aehmc_logp(q[i], (long long)i, prm);
  std::printf("%%.17g\n", v);
  for (int i = 0; i < D; i++) std::printf("%%.17g\n", aehmc_logp(Dual(q[i], 1.0), (long long)i, prm).d);
#else
  Row<double> r{q, 0, D};
  std::printf("%%.17g\n", (double)aehmc_logp(r, prm));
  for (int i = 0; i < D; i++) { Row<Dual> rd{q, i, D}; std::printf("%%.17g\n", aehmc_logp(rd, prm).d); }
#endif
  return 0;
}
"""


REV_HARNESS = r"""
#include <cstdio>
#include <cmath>
#define __device__
#define AEHMC_LANES 1
#define AEHMC_WSUM(x) (x)
#define AEHMC_ATOMIC_ADD(p, v) (*(p) += (v))
#define AEHMC_SYNC()
#include "dual.cuh"
%(source)s
%(params)s
int main() {
  const int D = %(D)d;
  const double q[] = {%(q)s};
  double g[%(D)d] = {0};
  std::printf("%%.17g\n", aehmc_logp_grad(q, g, 0, prm));
  for (int i = 0; i < D; i++) std::printf("%%.17g\n", g[i]);
  return 0;
}
"""


def params_decl(tr):
    params = "".join(f"static const double prm{k}[] = {{{', '.join(repr(float(x)) for x in p)}}};\n" for k, p in enumerate(tr.params))
    return params + "static const double *const prm[] = {" + ", ".join([f"prm{k}" for k in range(len(tr.params))] + ["nullptr"]) + "};\n"


def run_cpp_reverse(tr, q, tmp_path, name):
    """the reverse-mode program (one lane: the loops run whole, the wavefront reductions are identities)"""
    src = tmp_path / f"{name}_rev.cpp"
    src.write_text(REV_HARNESS % dict(source=tr.grad_source, params=params_decl(tr), D=len(q), q=", ".join(repr(float(x)) for x in q)))
    exe = tmp_path / f"{name}_rev"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "aehmc_amd", "csrc"), "-o", str(exe), str(src)])
    out = [float(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    return out[0], np.array(out[1:])


def run_cpp(tr, q, tmp_path, name):
    src = tmp_path / f"{name}.cpp"
    src.write_text(HARNESS % dict(source=tr.source, params=params_decl(tr), D=len(q), q=", ".join(repr(float(x)) for x in q), elem=int(tr.elementwise)))
    exe = tmp_path / name
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "aehmc_amd", "csrc"), "-o", str(exe), str(src)])
    out = [float(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    return out[0], np.array(out[1:])


@pytest.mark.parametrize("name", sorted(CASES))
def test_traced_density_and_gradient_match_the_python_function(name, tmp_path):
    fn, D, elementwise = CASES[name]
    tr = tracing.trace(fn, D)
    assert tr.elementwise == elementwise and tr.dim == D
    for trial in range(2):
        q = 0.7 * np.random.default_rng(trial).normal(size=D)
        v, g = run_cpp(tr, q, tmp_path, f"{name}{trial}")
        assert v == pytest.approx(float(fn(q)), rel=1e-13, abs=1e-13)
        h = 1e-6
        fd = np.array([(fn(q + h * np.eye(D)[i]) - fn(q - h * np.eye(D)[i])) / (2 * h) for i in range(D)])
        np.testing.assert_allclose(g, fd, rtol=2e-7, atol=2e-8)
        if not tr.elementwise:  # the reverse sweep (taken above 64 coordinates) == the forward passes
            vr, gr = run_cpp_reverse(tr, q, tmp_path, f"{name}{trial}")
            assert vr == pytest.approx(v, rel=1e-14, abs=1e-14)
            np.testing.assert_allclose(gr, g, rtol=1e-12, atol=1e-13)


def random_density(seed, D):
    """a random joint density: hyper-parameters at the head of the position, vector terms over slices of the rest, nested
    reductions, where / maximum, captured arrays"""
    r = np.random.default_rng(seed)
    n = D - 3
    w, c = r.normal(size=n), 0.5 + r.random(n)
    A = r.normal(size=(3, n)) / np.sqrt(n)
    picks = r.integers(0, 9, size=4)
    G = max(2, n // 3)
    grp = r.integers(0, G, size=2 * n)
    w2 = r.normal(size=2 * n)
    B = r.normal(size=(n, n)) / n

    def fn(q):
        a, b, s = q[0], q[1], q[2]
        x = q[3:]
        terms = [lambda: (-0.5 * (x - a) ** 2 * np.exp(-2.0 * s)).sum() - n * s,
                 lambda: -np.sum(np.log1p(np.square((x - w) / c))) * (1.0 + b * b) ** 0.5,
                 lambda: np.tanh(a) * (x[: n // 2] * x[n - n // 2:]).sum() - 0.5 * np.dot(x, x) / (1.0 + tracing.softplus(b)),
                 lambda: -0.5 * np.sum((A @ x - np.array([a, b, s])) ** 2),
                 lambda: np.sum(tracing.where(x > a, np.sin(x) * b, -np.abs(x - a))) * 0.3 - np.logaddexp(a, b),
                 lambda: -(np.maximum(x, w) * c).sum() * np.exp(-np.abs(s)) + (x[1:] - x[:-1]).mean() * np.cos(a),
                 lambda: -0.5 * np.sum((w2 - x[:G][grp] * np.exp(0.1 * b)) ** 2) / (2 * n),            # a gather (random effects by group)
                 lambda: -0.5 * np.dot(x, B @ x) * (1.0 + 0.1 * np.tanh(s)) if n > 32 else -0.5 * np.dot(x - a, B @ (x - a)),
                 lambda: np.exp(-np.sum(x * x) / n) * a - np.log1p(np.sum(np.square(x - b)) / n)]     # functions of reductions
        out = -0.5 * (a * a + b * b + s * s)
        for k in picks:
            out = out + terms[k]()
        return out

    return fn


def random_shared_density(seed, D):
    """random_density's kind, with terms that reuse one or two NAMED reductions on and off the additive spine: under a
    function, in a where branch, inside the body of another reduction, with hoisted hyper-parameters"""
    r = np.random.default_rng(1000 + seed)
    n = D - 3
    w = r.normal(size=n) / np.sqrt(n)
    A = r.normal(size=(3, n)) / np.sqrt(n)
    picks = r.integers(0, 7, size=3)
    thr = (0.2 if seed % 2 else 0.6) * n

    def fn(q):
        a, b, s = q[0], q[1], q[2]
        x = q[3:]
        r1 = (x * x).sum()
        r2 = (x * w).sum()
        terms = [lambda: -r1 + 2.0 * np.log(r1),
                 lambda: r2 - 0.5 * ((x - r2 / n) ** 2).sum(),
                 lambda: tracing.where(r1 > thr, -r1, -r1 * r1 / n) - 0.5 * r1,
                 lambda: -r1 - np.sqrt(1.0 + r1) * np.tanh(a) - np.log1p(r1 * np.exp(-2.0 * s)),
                 lambda: (lambda r3: -r3 - np.log1p(r3))(((x - a) ** 2 * np.exp(-s)).sum()),       # hoisted hyper-parameters
                 lambda: -r2 - 0.5 * np.sum((A @ x - r2) ** 2),
                 lambda: (lambda v: -v - np.log(v + 0.1))(x.var())]
        out = -0.5 * (a * a + b * b + s * s) - 0.05 * np.dot(x, x)
        for k in picks:
            out = out + terms[k]()
        return out

    return fn


def test_a_long_reduction_that_cannot_be_spread_over_the_lanes_warns():
    X = np.random.default_rng(0).normal(size=(2000, 80))   # 80 coefficients: the inner reduction exceeds the private accumulators
    with pytest.warns(UserWarning, match="runs on ONE lane"):
        tracing.trace(lambda q: -0.5 * np.sum((X @ q) ** 2) - 0.5 * (q @ q), 80)


def test_gather_index_out_of_range_is_an_indexerror():
    with pytest.raises(IndexError, match="out of range"):
        tracing.trace(lambda q: q[np.array([0, 5])].sum(), 3)


@pytest.mark.parametrize("seed", range(18))
def test_reverse_mode_equals_forward_mode_on_random_densities(seed, tmp_path):
    """forward- and reverse-mode gradients equal to 1e-12 on random densities (both compiled as plain
    C++: the Dual template against the reverse sweep), and both equal to central differences of the Python function"""
    D = [9, 17, 70][seed % 3]
    fn = random_density(seed, D)
    tr = tracing.trace(fn, D)
    assert not tr.elementwise and "aehmc_logp_grad" in tr.grad_source
    q = 0.6 * np.random.default_rng(100 + seed).normal(size=D)
    v, g = run_cpp(tr, q, tmp_path, f"rnd{seed}")
    vr, gr = run_cpp_reverse(tr, q, tmp_path, f"rnd{seed}")
    assert v == pytest.approx(float(fn(q)), rel=1e-12, abs=1e-12) and vr == pytest.approx(v, rel=1e-13, abs=1e-13)
    np.testing.assert_allclose(gr, g, rtol=1e-12, atol=1e-12)
    h = 1e-6
    fd = np.array([(fn(q + h * np.eye(D)[i]) - fn(q - h * np.eye(D)[i])) / (2 * h) for i in range(D)])
    np.testing.assert_allclose(gr, fd, rtol=5e-7, atol=5e-7)


def test_readme_function_is_the_builtin_standard_normal_expression():
    """README.md:27-36: logprob of N(0, 1) at a scalar position.  The emitted expression is, operation for operation,
    the built-in StdNormal target's (engine.cuh: u = 0.5 (q q) + log sqrt(2 pi), g = q), so the README value is
    reproduced bit for bit on the GPU (tests/test_gpu_callable.py)."""
    tr = tracing.trace(lambda y: -0.5 * y**2 - 0.5 * np.log(2 * np.pi), 1, scalar=True)
    assert tr.elementwise and tr.params == []
    assert "return T(((-0.5 * square(q)) - 0.9189385332046727));" in tr.source
    # the same function handed a vector of one entry (a [C, 1] position) takes the same form
    assert tracing.trace(lambda y: -0.5 * y**2 - 0.5 * np.log(2 * np.pi), 1).source == tr.source


def test_targets_from_callable_picks_the_target_class():
    t1 = targets.from_callable(student_t, 7)
    assert isinstance(t1, targets.Custom) and not t1.hand_gradient and len(t1.param_list) == 3 and t1.dim == 7
    t2 = targets.from_callable(mvn, 2)
    assert isinstance(t2, targets.CustomJoint) and t2.dim == 2 and "aehmc_logp" in t2.source
    assert targets.as_target(t2, 2) is t2
    assert targets.as_target(mvn, 2) is targets.as_target(mvn, 2)  # traced once per function and shape
    with pytest.raises(TypeError, match="Target or a Python function"):
        targets.as_target(3.0, 2)


@pytest.mark.parametrize("fn, match", [
    (lambda q: q.sum() if q[0] > 0 else 0.0, "control flow cannot be traced"),
    (lambda q: __import__("math").exp(q[0]), "use the numpy functions"),
    (lambda q: np.arcsinh(q).sum(), "numpy.arcsinh is not supported"),
    (lambda q: q * 2.0, "must return a scalar"),
    (lambda q: 1.0, "does not depend on the position"),
    (lambda q: q[np.array([0.5, 1.0])].sum(), "integer arrays"),
    (lambda q: (q > 0).sum(), "comparison"),
    (lambda q: np.cumsum(q)[-1], "numpy.cumsum is not supported"),
    (lambda q: (q[:2] + q).sum(), "do not broadcast"),
    (lambda q: (np.ones((2, 2, 2)) * q[0]).sum(), "dimensions are not supported"),
    (lambda q: np.max(np.concatenate([q] * 22)), "supported up to 64"),
    (lambda q: q.reshape(3, 1).sum(), "traced values are scalars and vectors"),
    (lambda q: np.stack([q, q]).sum(), "would be a matrix"),
    (lambda q: q.astype(int).sum(), "astype"),
    (lambda q: np.linalg.norm(q, ord=1), "numpy.norm is not supported"),
])
def test_untraceable_operations_raise_typeerror_at_trace_time(fn, match):
    with pytest.raises(TypeError, match=match):
        tracing.trace(fn, 3)


def test_max_over_a_long_vector_is_refused_with_its_length():
    with pytest.raises(TypeError, match="max / min over 100 traced entries"):
        tracing.trace(lambda q: np.max(q), 100)


# ------------------------------------------------------------------------------------------ shared reductions
def loops(tr):
    """how many loops the reverse-mode program runs: a sum whose backward sweep rides in its forward loop is ONE"""
    return tr.grad_source.count("for (int i")


def test_a_spine_sum_is_fused_only_when_the_spine_is_its_one_use_that_carries_an_adjoint():
    assert loops(tracing.trace(sh_cmp_only, 6)) == 1             # (the other use is a comparison: still fused)
    assert loops(tracing.trace(lambda x: -(x * x).sum(), 6)) == 1
    assert loops(tracing.trace(sh_log_of_sum, 6)) == 2           # forward loop, then ONE backward loop with the merged adjoint
    assert loops(tracing.trace(sh_three_uses, 6)) == 2
    assert loops(tracing.trace(lambda x: -(x * x).sum() + 3 * np.log((x * x).sum()), 6)) == 3  # two nodes: one fused, one not


def shared_inputs(name, D=6):
    """two positions per density, entries of one sign (no cancellation in the sums): sum x^2 ~ 2.7 and ~ 0.3 at D = 6 --
    either side of the where threshold 1 and away from it and from 0 -- and x[1] = 0.8 / <= 0.35 around its threshold 0.5"""
    r = np.random.default_rng(sum(map(ord, name)))
    big, small = 0.3 + 0.7 * r.random(D), 0.1 + 0.25 * r.random(D)
    big[1] = 0.8
    return [big, small]


def closed_form_50_digits(cf, q):
    import mpmath
    with mpmath.workdps(50):
        v, g = cf([mpmath.mpf(float(x)) for x in q], mpmath.mp)
        return v, list(g)


def closed_form_float64(cf, q):
    v, g = cf([np.float64(x) for x in q], np)
    return float(v), np.array(g, dtype=np.float64)


def float64_error_of_the_closed_forms(cases):
    """(value, gradient): the largest error of the closed forms evaluated in plain float64 against their 50-digit values,
    over `cases` = [(closed form, position)], each as a fraction of |value| / of the gradient's largest entry"""
    ev = eg = 0.0
    for cf, q in cases:
        v, g = closed_form_50_digits(cf, q)
        v64, g64 = closed_form_float64(cf, q)
        ev = max(ev, float(abs(v64 - v) / abs(v)))
        eg = max(eg, float(max(abs(a - b) for a, b in zip(g64, g)) / max(abs(b) for b in g)))
    return ev, eg


# What the generated programs may be off by: 8 x the error of the same closed form in plain float64 (they associate the
# sums differently and log_fast is good to 2 ulp; nothing larger is expected).  A density's own float64 error can be
# exactly zero (-4 x is exact), which no differently ordered program can be held to, so the figure is the largest over
# the family and both positions, as a fraction of |value| and of the gradient's largest entry.  Measured at D = 6:
# value 8.78e-16 (shared_cmp_only, second position), gradient 8.71e-16 (shared_log_of_sum, first position: -1 + 3 / s
# cancels there) -> bounds 7.0e-15 and 7.0e-15; per density the float64 gradient error runs from 0 (shared_sum_twice,
# shared_where_spine's first position) to that.  The programs: values within 8.8e-16, gradients within 2.6e-15.
ALLOWED_OVER_FLOAT64 = 8.0


@pytest.fixture(scope="module")
def float64_error():
    return float64_error_of_the_closed_forms([(cf, q) for name, (_, cf) in sorted(SHARED.items()) for q in shared_inputs(name)])


@pytest.mark.parametrize("name", sorted(SHARED))
def test_shared_reductions_against_the_closed_form_at_50_digits(name, tmp_path, float64_error):
    """Two generated programs that agree can be wrong together: value and both gradients against the closed-form
    gradient evaluated with 50 digits"""
    fn, cf = SHARED[name]
    tr = tracing.trace(fn, 6)
    ev, eg = float64_error
    print(f"float64 error of the closed forms: value {ev:.3g}, gradient {eg:.3g}")
    assert 0.0 < ev < 1e-14 and 0.0 < eg < 1e-14
    for k, q in enumerate(shared_inputs(name)):
        v50, g50 = closed_form_50_digits(cf, q)
        assert float(fn(q)) == pytest.approx(float(v50), rel=1e-13)  # (the closed form is this density's)
        gscale = max(abs(b) for b in g50)
        for mode, (v, g) in (("forward", run_cpp(tr, q, tmp_path, f"{name}{k}")), ("reverse", run_cpp_reverse(tr, q, tmp_path, f"{name}{k}"))):
            dv = float(abs(v - v50) / abs(v50))
            dg = float(max(abs(a - b) for a, b in zip(g, g50)) / gscale)
            print(f"{name}[{k}] {mode}: value off by {dv:.3g}, gradient by {dg:.3g}")
            assert dv <= ALLOWED_OVER_FLOAT64 * ev, (mode, dv)
            assert dg <= ALLOWED_OVER_FLOAT64 * eg, (mode, dg)


@pytest.mark.parametrize("D", [9, 17, 70])
@pytest.mark.parametrize("seed", range(12))
def test_reverse_mode_equals_forward_mode_on_random_densities_with_shared_reductions(seed, D, tmp_path):
    fn = random_shared_density(seed, D)
    tr = tracing.trace(fn, D)
    assert not tr.elementwise and "aehmc_logp_grad" in tr.grad_source
    q = 0.6 * np.random.default_rng(100 + seed).normal(size=D)
    v, g = run_cpp(tr, q, tmp_path, f"rsh{seed}")
    vr, gr = run_cpp_reverse(tr, q, tmp_path, f"rsh{seed}")
    assert v == pytest.approx(float(fn(q)), rel=1e-12, abs=1e-12) and vr == pytest.approx(v, rel=1e-13, abs=1e-13)
    np.testing.assert_allclose(gr, g, rtol=1e-12, atol=1e-12)
    h = 1e-6
    fd = np.array([(fn(q + h * np.eye(D)[i]) - fn(q - h * np.eye(D)[i])) / (2 * h) for i in range(D)])
    np.testing.assert_allclose(gr, fd, rtol=5e-7, atol=5e-7)


W64 = np.random.default_rng(64).normal(size=64)
GROWTH = {"logsumexp": lambda q: tracing.logsumexp(q * W64[:len(q)]) - 0.5 * (q * q).sum(),
          "max": lambda q: np.max(q * W64[:len(q)]) - 0.5 * (q * q).sum(),
          "logaddexp_reduce": lambda q: np.logaddexp.reduce(q + W64[:len(q)]) - 0.5 * (q * q).sum()}


@pytest.mark.parametrize("name", sorted(GROWTH))
def test_source_of_a_running_maximum_grows_linearly_with_its_terms(name, tmp_path):
    """logsumexp / max / logaddexp.reduce are nested where(y > m, y, m) with the running m used twice per level: written
    out as a tree the forward source doubled per term (0.8 MB at 12 terms).  At the documented limit of 64 terms it is
    at most 64 / 8 times the 8-term source (x 2: longer names), compiles, and is right."""
    fn = GROWTH[name]
    small, big = tracing.trace(fn, 8), tracing.trace(fn, 64)
    assert len(big.source) < 2 * (64 // 8) * len(small.source), (len(small.source), len(big.source))
    assert len(big.grad_source) < 2 * (64 // 8) * len(small.grad_source)
    for tr, D in ((small, 8), (big, 64)):
        q = 0.7 * np.random.default_rng(D).normal(size=D)
        v, g = run_cpp(tr, q, tmp_path, f"{name}{D}")
        vr, gr = run_cpp_reverse(tr, q, tmp_path, f"{name}{D}")
        assert v == pytest.approx(float(fn(q)), rel=1e-13, abs=1e-13) and vr == pytest.approx(v, rel=1e-14, abs=1e-14)
        h = 1e-6
        fd = np.array([(fn(q + h * np.eye(D)[i]) - fn(q - h * np.eye(D)[i])) / (2 * h) for i in range(D)])
        np.testing.assert_allclose(g, fd, rtol=2e-7, atol=2e-8)
        np.testing.assert_allclose(gr, g, rtol=1e-12, atol=1e-13)


YARG = np.random.default_rng(11).normal(size=7) + 0.5
ARGS_CASES = {"inside_a_reduction": lambda q, y: -0.5 * ((q - y.mean()) ** 2).sum() - q[0] * q[1],
              "on_the_spine": lambda q, y: y.sum() - 0.5 * ((q - y.mean()) ** 2).sum() + y.mean() * q[2] - (q * y[:5]).sum() * y.var()}


@pytest.mark.parametrize("name", sorted(ARGS_CASES))
def test_a_reduction_over_an_args_array_alone_traces_and_differentiates(name, tmp_path):
    """`args=` arrays are lifted to traced constants: y.mean() is a `sum` node that does not depend on the position
    (IndexError: it kept three arguments where every reader takes four; and its loop was dropped from the reverse program)"""
    fn = ARGS_CASES[name]
    tr = tracing.trace(fn, 5, args=(YARG,))
    assert not tr.elementwise
    q = 0.7 * np.random.default_rng(3).normal(size=5)
    v, g = run_cpp(tr, q, tmp_path, name)
    vr, gr = run_cpp_reverse(tr, q, tmp_path, name)
    assert v == pytest.approx(float(fn(q, YARG)), rel=1e-13, abs=1e-13) and vr == pytest.approx(v, rel=1e-14, abs=1e-14)
    h = 1e-6
    fd = np.array([(fn(q + h * np.eye(5)[i], YARG) - fn(q - h * np.eye(5)[i], YARG)) / (2 * h) for i in range(5)])
    np.testing.assert_allclose(g, fd, rtol=2e-7, atol=2e-8)
    np.testing.assert_allclose(gr, g, rtol=1e-12, atol=1e-13)
    if name == "inside_a_reduction":  # the closed form too: grad = -(q - mean(y)) - [q1, q0, 0, 0, 0]
        exact = -(q - YARG.mean()) - np.array([q[1], q[0], 0.0, 0.0, 0.0])
        np.testing.assert_allclose(gr, exact, rtol=1e-14, atol=1e-15)


def test_sources_of_densities_without_shared_nodes_are_what_they_were():
    """A node with one parent is emitted exactly as before shared nodes were named: sha256 of the forward template of
    the models that share nothing (funnel, mvn, more_functions, student_t) and of every model's reverse-mode program,
    taken before shared nodes were named; `source_with_named_nodes`: the forward templates of the eleven models with
    shared nodes, as they are since (tests/golden/traced_source_digests_v1.json; the code-object cache is keyed by the source)"""
    import hashlib
    import json
    with open(os.path.join(ROOT, "tests", "golden", "traced_source_digests_v1.json")) as f:
        pinned = json.load(f)
    assert sum("source" in d for d in pinned.values()) >= 3 and all(("source" in d) != ("source_with_named_nodes" in d) for d in pinned.values())
    for name, d in sorted(pinned.items()):
        fn, D, _ = CASES[name]
        tr = tracing.trace(fn, D)
        assert hashlib.sha256(tr.source.encode()).hexdigest() == d.get("source", d.get("source_with_named_nodes")), name
        if "grad_source" in d:
            assert hashlib.sha256(tr.grad_source.encode()).hexdigest() == d["grad_source"], name


# name -> the seed tests/test_gpu_callable.py hands three_way, which draws the start positions from it: seeds at which sum x^2
# is away from 1 (the where threshold) and from 3 (where shared_log_of_sum's -1 + 3 / s cancels) in every chain
DEVICE_SHARED = {"shared_log_of_sum": 4, "shared_centred": 5, "shared_where_spine": 1, "shared_var_twice": 4}


def device_positions(name, D, C=5):
    """the start positions tests/test_gpu_callable.py's three_way draws for this density"""
    q0 = 0.4 * np.random.default_rng(50 + DEVICE_SHARED[name]).normal(size=(C, D))
    if name == "shared_where_spine":  # chain 0 shrunk to sum x^2 = 0.25: the branch below the threshold runs on the device too
        q0[0] *= np.sqrt(0.25 / (q0[0] * q0[0]).sum())
    return q0


def test_device_expected_gradients_are_the_closed_forms_at_50_digits():
    """tests/golden/shared_sum_device_grad_v1.json -- what the device test compares state.potential_energy_grad with -- is
    minus the closed-form gradient at 50 digits, rounded once; and no start position sits at the where threshold"""
    import json
    with open(os.path.join(ROOT, "tests", "golden", "shared_sum_device_grad_v1.json")) as f:
        golden = json.load(f)
    assert sorted(golden) == sorted(DEVICE_SHARED)
    for name in DEVICE_SHARED:
        for D in (17, 70):
            q0 = device_positions(name, D)
            s = (q0 * q0).sum(axis=1)
            assert np.abs(s - {"shared_where_spine": 1.0, "shared_log_of_sum": 3.0}.get(name, 0.0)).min() > 0.7
            assert name != "shared_where_spine" or ((s < 1).sum() == 1 and (s > 1).sum() == 4)  # both branches
            want = np.array([[-float(x) for x in closed_form_50_digits(SHARED[name][1], q)[1]] for q in q0])
            assert np.array_equal(want, np.array(golden[name][str(D)]))
