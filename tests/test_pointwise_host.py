"""``tracing.trace_pointwise`` without a GPU: the emitted ``aehmc_pointwise_head`` / ``aehmc_pointwise`` compiled as host
C++ (the way tests/test_tracing.py compiles a density) against the Python function on plain numpy arrays and against
mpmath at 50 digits.

Allowance per entry, in the style of tests/test_transforms_host.py: N U A with U = 2^-53, N = 64 a bound on the roundings
an entry passes through -- at most 30 arithmetic operations, doubled where they sit under a square, and each call of
the math library counted as 2 (E_np + 2) roundings, E_np <= 2 ulp for exp / log and the 6 ulp tests/dual_ref.py grants
softplus -- and A the sum of the absolute addends, where a squared residual c r^2, r = sum a_k, enters as |c| (sum |a_k|)^2:
that covers both the term and the error 2 |r| delta r that cancellation in r leaves."""
import os
import subprocess

import numpy as np
import pytest

from aehmc_amd import tracing, transforms as tf
from test_tracing import params_decl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
N_ROUNDINGS = 64

HARNESS = r"""
#include <cstdio>
#include <cmath>
#define __device__
#include "dual.cuh"
%(source)s
struct Row { const double *p; double operator[](long long i) const { return p[i]; } };
%(params)s
int main() {
  const int R = %(R)d, D = %(D)d, n_out = %(n_out)d, n_head = %(n_head)d;
  static const double q[] = {%(q)s};
  double h[%(n_head)d + 1];
  for (int r = 0; r < R; r++) {
    for (int k = 0; k <= n_head; k++) h[k] = -12345.0;
    aehmc_pointwise_head(Row{q + r * D}, prm, h);
    for (long long j = 0; j < n_out; j++) std::printf("%%.17g\n", aehmc_pointwise(Row{q + r * D}, h, j, prm));
    for (int k = 0; k < n_head; k++) std::printf("%%.17g\n", h[k]);
  }
  return 0;
}
"""


def run_pointwise_cpp(tr, q, tmp_path, name):
    """(values [R, n_out], head values [R, n_head]) of the emitted source on the rows q [R, dim] (or one row [dim])"""
    q2 = np.atleast_2d(np.asarray(q, dtype=np.float64))
    assert q2.shape[1] == tr.dim
    src = tmp_path / f"{name}.cpp"
    src.write_text(HARNESS % dict(source=tr.source, params=params_decl(tr), R=q2.shape[0], D=tr.dim, n_out=tr.n_out,
                                  n_head=tr.n_head, q=", ".join(repr(float(x)) for x in q2.reshape(-1))))
    exe = tmp_path / name
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "aehmc_amd", "csrc"), "-o", str(exe), str(src)])
    out = np.array([float(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()])
    out = out.reshape(q2.shape[0], tr.n_out + tr.n_head)
    return out[:, :tr.n_out], out[:, tr.n_out:]


def _mp():
    import mpmath
    mp = mpmath.mp.clone()
    mp.dps = 50
    return mp


def _f(mp, a):
    return [mp.mpf(float(v)) for v in np.asarray(a).reshape(-1)]


_r = np.random.default_rng(11)
X = _r.normal(size=(37, 5))
Y = _r.normal(size=37)
XL = _r.normal(size=(23, 4))
YL = (_r.random(23) < 0.5).astype(np.float64)
GROUP = _r.integers(0, 4, size=19)
YG = _r.normal(size=19)
Z = _r.random((37, 4))
HALF_LOG_2PI = 0.5 * np.log(2 * np.pi)


def regression(q):
    w, sigma = q[:5], np.exp(q[5])
    return -0.5 * ((Y - X @ w) / sigma) ** 2 - np.log(sigma) - 0.5 * np.log(2 * np.pi)


def _gauss_mp(mp, y, xs, w, sigma):
    """(-0.5 ((y - x . w) / sigma)^2 - log(sigma) - 0.5 log(2 pi), A)"""
    prods = [a * b for a, b in zip(xs, w)]
    r = y - mp.fsum(prods)
    mag = abs(y) + mp.fsum(abs(p) for p in prods)
    c = mp.mpf(float(HALF_LOG_2PI))
    return -r * r / (2 * sigma * sigma) - mp.log(sigma) - c, mag * mag / (2 * sigma * sigma) + abs(mp.log(sigma)) + c


def regression_mp(mp, q):
    w, sigma = _f(mp, q[:5]), mp.mpf(float(np.exp(q[5])))  # (sigma as the program forms it: exp's own error is in N)
    return [_gauss_mp(mp, mp.mpf(float(Y[j])), _f(mp, X[j]), w, sigma) for j in range(37)]


def logistic(q):
    z = XL @ q
    return YL * z - tracing.softplus(z)


def logistic_mp(mp, q):
    w, out = _f(mp, q), []
    for j in range(23):
        prods = [a * b for a, b in zip(_f(mp, XL[j]), w)]
        z, mag = mp.fsum(prods), mp.fsum(abs(p) for p in prods)
        sp = mp.log1p(mp.exp(z))
        out.append((mp.mpf(float(YL[j])) * z - sp, 2 * mag + sp))
    return out


def gather(q):
    mu, s = q[:4], np.exp(-q[4])
    return -0.5 * ((YG - mu[GROUP]) * s) ** 2 - q[4]


def gather_mp(mp, q):
    s, out = mp.mpf(float(np.exp(-q[4]))), []
    for j in range(19):
        y, m = mp.mpf(float(YG[j])), mp.mpf(float(q[GROUP[j]]))
        out.append((-((y - m) * s) ** 2 / 2 - mp.mpf(float(q[4])), ((abs(y) + abs(m)) * s) ** 2 / 2 + abs(mp.mpf(float(q[4])))))
    return out


def unrolled(q):
    return [q[0] * q[1], np.exp(q[2]), (q * q).sum()]


def unrolled_mp(mp, q):
    v = _f(mp, q)
    vals = [v[0] * v[1], mp.exp(v[2]), mp.fsum(x * x for x in v)]
    return [(x, abs(x)) for x in vals]


def scalar(q):
    return -0.5 * (q * q).sum() - tracing.softplus(q[0])


def scalar_mp(mp, q):
    v = _f(mp, q)
    a, b = mp.fsum(x * x for x in v) / 2, mp.log1p(mp.exp(v[0]))
    return [(-a - b, a + b)]


def mixed_model():
    return tf.Model({"w": tf.Real(5), "sigma": tf.Positive(), "pi": tf.Simplex(4)},
                    lambda w, sigma, pi: -0.5 * np.sum(w * w) - sigma + np.sum(np.log(pi)))


def model_loglik(w, sigma, pi):
    return -0.5 * ((Y - X @ w) / sigma) ** 2 - np.log(sigma) - 0.5 * np.log(2 * np.pi) + Z @ np.log(pi)


def model_mp(mp, theta):
    """theta: the CONSTRAINED vector (w [5], sigma, pi [4]) the program is traced on"""
    w, sigma, logpi = _f(mp, theta[:5]), mp.mpf(float(theta[5])), [mp.log(v) for v in _f(mp, theta[6:])]
    out = []
    for j in range(37):
        v, a = _gauss_mp(mp, mp.mpf(float(Y[j])), _f(mp, X[j]), w, sigma)
        mix = [z * lp for z, lp in zip(_f(mp, Z[j]), logpi)]
        out.append((v + mp.fsum(mix), a + mp.fsum(abs(t) for t in mix)))
    return out


def model_theta(q):
    """the constrained vector of a position of mixed_model, in numpy (the operation order of csrc/constrain.cuh)"""
    xt = np.append(q[6:9], 0.0)
    m = xt.max()
    L = m + np.log(np.sum(np.exp(xt - m)))
    return np.concatenate([q[:5], [np.exp(q[5])], np.exp(xt - L)])


CASES = {"regression": (regression, 6, regression_mp, 37), "logistic": (logistic, 4, logistic_mp, 23),
         "gather": (gather, 5, gather_mp, 19), "unrolled": (unrolled, 3, unrolled_mp, 3), "scalar": (scalar, 4, scalar_mp, 1)}


def traced(name):
    fn, dim, _, _ = CASES[name]
    return tracing.trace_pointwise(fn, dim)


def allowance(ref):
    return N_ROUNDINGS * U * np.array([float(a) for _, a in ref])


def check(got, fn_value, ref, name):
    want, allow = np.array([float(v) for v, _ in ref]), allowance(ref)
    print(name, "compiled: error / allowance", (np.abs(got - want) / allow).max(), "numpy:", (np.abs(fn_value - want) / allow).max())
    assert np.all(np.abs(got - want) <= allow), name
    assert np.all(np.abs(fn_value - want) <= allow), name


@pytest.mark.parametrize("name", sorted(CASES))
def test_emitted_source_against_numpy_and_50_digits(name, tmp_path):
    fn, dim, ref, n_out = CASES[name]
    tr = traced(name)
    assert (tr.dim, tr.n_out) == (dim, n_out)
    mp = _mp()
    q = 0.7 * np.random.default_rng(5).normal(size=(2, dim))
    values, _ = run_pointwise_cpp(tr, q, tmp_path, name)
    for trial in range(2):
        check(values[trial], np.atleast_1d(np.asarray(fn(q[trial]), dtype=np.float64)), ref(mp, q[trial]), f"{name}[{trial}]")


def test_model_pointwise_on_the_constrained_scale(tmp_path):
    model = mixed_model()
    pw = model.pointwise(model_loglik)
    assert (pw.dim, pw.n_out, model.dim, model.constrained_dim) == (9, 37, 9, 10)
    tr = pw._traced
    assert tr.dim == 10 and "exp(" not in tr.source  # (no transform is evaluated in it: sigma and pi are read)
    mp = _mp()
    q = 0.7 * np.random.default_rng(6).normal(size=(2, 9))
    theta = np.stack([model_theta(row) for row in q])
    values, _ = run_pointwise_cpp(tr, theta, tmp_path, "model")
    for trial in range(2):
        un = {k: theta[trial][model._out[k]] if t.shape else theta[trial][model._out[k].start] for k, t in model.spec.items()}
        check(values[trial], model_loglik(**un), model_mp(mp, theta[trial]), f"model[{trial}]")


def test_head_holds_what_does_not_depend_on_the_entry(tmp_path):
    """sigma's terms are hoisted: computed once per row by aehmc_pointwise_head, which has no entry index to read"""
    tr = traced("regression")
    assert tr.n_head == 2
    head_src, body_src = tr.source.split("template <class V> __device__ double aehmc_pointwise(")
    assert "long long j" not in head_src and "exp(" in head_src and "log(" in head_src
    assert "exp(" not in body_src and "log(" not in body_src
    q = 0.7 * np.random.default_rng(5).normal(size=(3, 6))
    _, head = run_pointwise_cpp(tr, q, tmp_path, "head")
    np.testing.assert_array_equal(head[:, 0], np.exp(q[:, 5]))
    np.testing.assert_allclose(head[:, 1], q[:, 5], rtol=0, atol=8 * U * np.abs(q[:, 5]).max() + 8 * U)
    assert traced("logistic").n_head == 0 and traced("unrolled").n_head == 0 and traced("gather").n_head >= 1


def test_source_length():
    """a lazy vector's source does not know its length; an unrolled one grows by one case per entry"""
    def lazy(n):
        x, y = np.linspace(-1.0, 1.0, 5 * n).reshape(n, 5), np.linspace(0.0, 1.0, n)
        return tracing.trace_pointwise(lambda q: -0.5 * ((y - x @ q[:5]) / np.exp(q[5])) ** 2 - q[5], 6)
    a, b = lazy(37), lazy(370)
    assert (a.n_out, b.n_out) == (37, 370) and len(a.source) == len(b.source)

    def listed(n):
        return tracing.trace_pointwise(lambda q: [np.exp(q[k % 3]) * q[(k + 1) % 3] for k in range(n)], 3)
    l8, l16, l32 = (len(listed(n).source) for n in (8, 16, 32))
    assert l16 > l8 and abs((l32 - l16) - 2 * (l16 - l8)) <= 0.1 * (l16 - l8)


def test_what_cannot_be_traced():
    with pytest.raises(tracing.TraceError, match="comparison"):
        tracing.trace_pointwise(lambda q: q > 0.0, 3)
    with pytest.raises(tracing.TraceError, match="comparison"):
        tracing.trace_pointwise(lambda q: q[0] > 0.0, 3)
    with pytest.raises(tracing.TraceError, match="does not depend on the position"):
        tracing.trace_pointwise(lambda q: np.ones(3), 3)
    with pytest.raises(tracing.TraceError, match="does not depend on the position"):
        tracing.trace_pointwise(lambda q: 2.0 * np.arange(4.0) + 1.0, 3)
    with pytest.raises(tracing.TraceError, match="does not depend on the position"):
        tracing.trace_pointwise(lambda q: [1.0, 2.0], 3)
    with pytest.raises(tracing.TraceError, match="65 entries"):
        tracing.trace_pointwise(lambda q: [q[k % 3] * float(k) for k in range(65)], 3)
    assert tracing.trace_pointwise(lambda q: [q[k % 3] * float(k + 1) for k in range(64)], 3).n_out == 64
