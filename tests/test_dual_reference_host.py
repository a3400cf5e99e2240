"""csrc/dual.cuh and the tracer's reverse-mode rules, one function at a time, against mpmath at 50 digits: the CPU build
(g++ -O1 against glibc, as tests/test_dual.py).  The table -- expressions, closed forms, points, edges, allowances and
where each allowance comes from -- is tests/dual_ref.py; tests/test_gpu_dual_reference.py runs the same table through
the run-time compiled kernels on the device.

Forward mode: one program, `switch (id)` over the table's C++ expressions, instantiated with Dual (value and derivative)
and with double (the value must be the Dual's bit for bit, except where T = double is the math library's own log / log1p /
lgamma).  Reverse mode: the traced wrapper  sum_blocks f(q[block]).sum() + q[0] * q[1:].sum()  (joint through the coupling
term, so it comes with its generated adjoint program), compiled the way tests/test_tracing.py compiles it; with q[0] = 0.0
the gradient entry of q_i is f'(q_i) plus an exact zero."""
import math
import os
import subprocess

import numpy as np
import pytest

import dual_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FWD = r"""
#include <cstdio>
#include <cmath>
#include "dual.cuh"
using aehmc::Dual;
template <class T> T fn(int id, T q) {
  switch (id) {
%s
  }
  return q;
}
int main() {
  int id; double x;
  while (std::scanf("%%d %%lf", &id, &x) == 2) {
    const Dual r = fn(id, Dual(x, 1.0));
    const double v = fn(id, x);
    std::printf("%%a %%a %%a\n", r.v, r.d, v);
  }
  return 0;
}
"""

REV = r"""
#include <cstdio>
#include <cmath>
#define __device__
#define AEHMC_LANES 1
#define AEHMC_WSUM(x) (x)
#define AEHMC_ATOMIC_ADD(p, v) (*(p) += (v))
#define AEHMC_SYNC()
#include "dual.cuh"
%(source)s
static const double *const prm[] = {nullptr};
int main() {
  const int D = %(D)d;
  double q[%(D)d], g[%(D)d];
  for (;;) {
    for (int i = 0; i < D; i++) { if (std::scanf("%%lf", &q[i]) != 1) return 0; g[i] = 0.0; }
    std::printf("%%a", aehmc_logp_grad(q, g, 0, prm));
    for (int i = 0; i < D; i++) std::printf(" %%a", g[i]);
    std::printf("\n");
  }
}
"""


def fhex(x):
    x = float(x)
    return "nan" if x != x else ("inf" if x == math.inf else "-inf" if x == -math.inf else x.hex())


def build(tmp, name, text):
    src = tmp / f"{name}.cpp"
    src.write_text(text)
    exe = tmp / name
    # (-fno-builtin-sin / -cos: g++ would fuse the Dual's sin(x) and cos(x) into one sincos call, a different glibc function whose
    # bits differ from sin's -- the T = double instantiation could then not be compared bit for bit)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fno-builtin-sin", "-fno-builtin-cos", "-I", os.path.join(ROOT, "aehmc_amd", "csrc"),
                           "-o", str(exe), str(src)])
    return exe


def run(exe, lines, width):
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split()
    return np.array([float.fromhex(t) for t in out]).reshape(-1, width)


@pytest.fixture(scope="module")
def forward(tmp_path_factory):
    return build(tmp_path_factory.mktemp("dual_fwd"), "fwd", FWD % T.switch_source())


D_REV = 70
LAYOUT = T.blocks(D_REV, T.TRACED)


@pytest.fixture(scope="module")
def reverse(tmp_path_factory):
    from aehmc_amd import tracing
    tr = tracing.trace(T.wrapper(LAYOUT), D_REV, reverse=True)
    assert not tr.elementwise and not tr.params and "aehmc_logp_grad" in tr.grad_source
    return build(tmp_path_factory.mktemp("dual_rev"), "rev", REV % dict(source=tr.grad_source, D=D_REV))


@pytest.mark.parametrize("name", T.NAMES)
def test_forward_mode_value_and_derivative_against_50_digits(name, forward):
    x = T.reference(name)[0]
    k = T.NAMES.index(name)
    got = run(forward, [f"{k} {fhex(v)}" for v in x], 3)
    T.check(name, x, got[:, 0], got[:, 1], what="forward, CPU build:")
    if T.ROWS[name].lib_double:  # T = double is glibc's log / log1p / lgamma: the same allowance, not the same bits
        _, v, _, va, _ = T.reference(name)
        assert T.worst(name, x, got[:, 2], v, va)[2] <= 1.0
    else:
        assert np.array_equal(got[:, 2], got[:, 0])


EDGES = [(n, e[0]) for n in T.NAMES for e in T.ROWS[n].edges]


@pytest.mark.parametrize("name, x", EDGES, ids=[f"{n}@{x!r}" for n, x in EDGES])
def test_forward_mode_edges_have_the_expected_class(name, x, forward):
    got = run(forward, [f"{T.NAMES.index(name)} {fhex(x)}"], 3)[0]
    assert T.edge_ok(name, x, got[0], 0), (name, x, "value", got[0])
    assert T.edge_ok(name, x, got[1], 1), (name, x, "derivative", got[1])
    assert T.edge_ok(name, x, got[2], 0), (name, x, "T = double", got[2])


def test_reverse_mode_gradient_and_value_against_50_digits(reverse):
    q, v, d, va, da = T.joint_positions(LAYOUT, D_REV)
    got = run(reverse, [" ".join(fhex(t) for t in row) for row in q], D_REV + 1)
    assert np.array_equal(got[:, 1], np.array([sum(r[1:]) for r in q]))  # d/dq_0 = the plain sum of the points, in coordinate order
    for name, lo, hi in LAYOUT:
        sl = (slice(None), slice(lo, hi))
        w = T.worst(name, q[sl].ravel(), got[:, 1:][sl].ravel(), d[sl].ravel(), da[sl].ravel())
        assert w[2] <= 1.0, f"reverse, CPU build: {name}: derivative off by {w[0]:.1f} ulp at x = {w[1]!r}, {w[2]:.2f} of the allowance"
    err = np.abs(got[:, 0] - T.joint_sum(v[:, 1:]))
    assert np.all(err <= T.joint_sum_allowance(v[:, 1:], va[:, 1:])), err.max()


def test_reverse_mode_edges_have_the_expected_class(reverse):
    """one evaluation per edge of every traced row, the other coordinates at ordinary points"""
    q, meta = T.joint_edges(LAYOUT, D_REV)
    got = run(reverse, [" ".join(fhex(t) for t in row) for row in q], D_REV + 1)
    T.check_joint_edges(LAYOUT, D_REV, meta, got[:, 0], got[:, 1:], what="reverse, CPU build:")


def test_numpy_error_E_np_is_what_the_table_expects():
    """E_np of the forwarded functions, measured against mpmath on the table's points: at most 2 ulp for numpy and the C library (1 but for erfc); a platform where it is larger would widen the [library] allowances unnoticed"""
    for name in ("exp", "expm1", "sqrt", "sin", "cos", "tanh", "sinh", "cosh", "atan", "erf", "erfc"):
        e = T.e_np(name, T.reference(name)[0])
        print(f"E_np({name}) = {e:.2f} ulp")
        assert e <= 2.0, (name, e)
    assert T.e_np("sqrt", T.reference("sqrt")[0]) == 0.0
    assert T.e_np("pow", T.reference("pow25")[0], 2.5) <= 1.0
