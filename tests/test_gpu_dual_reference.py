"""csrc/dual.cuh and the tracer's reverse-mode rules ON THE DEVICE, one function at a time, against mpmath at 50 digits:
the table of tests/dual_ref.py (expressions, closed forms, points, edges, allowances with their sources) through the real
run-time compiled paths -- hipRTC against the device math library, where ::exp, ::log, ::lgamma, ::tan, ::erf and ::pow
are other programs than glibc's (tests/test_dual_reference_host.py checks the g++ build).  No new kernels, no new ABI.

Routes (one compile each, the function chosen by a parameter or a coordinate block):
  forward   targets.Custom, ONE source whose aehmc_logp switches on (int)prm[0][0]; one chain per point, positions
            [n, 1]: potential_energy = -f(x), potential_energy_grad = -f'(x).  prm[0][1] = 1 evaluates the T = double
            instantiation instead (the bare library function: what tells the library from dual.cuh when a row fails);
  lanes     a hand-written CustomJoint of 1 + (number of rows) coordinates, the seeded lane JointArg<Dual>;
  reverse   the traced wrapper of tests/dual_ref.py with from_callable(..., reverse=True) at D = 17 (the rows in two
            halves) and D = 70, in new_state (the generated program on a wavefront per chain), and after one HMC
            transition of step size 2^-40 with engine option joint_wg = 0 and = 2 (a workgroup per chain), checked at
            the positions the transition returns.

MEASURED ON THE DEVICE (MI355X, the run recorded in DESIGN.md section 4; largest error in ulp of the 50-digit value):
  function                        forward f          forward f'          lanes f'   reverse f' (new_state)   reverse f' (after a transition, joint_wg 0 / 2)
  exp(q)                          1 ulp (0.33)       1 ulp (0.29)        1 ulp (0.29)        1 ulp (0.29)        1 ulp (0.29) / 1 ulp (0.29)
  expm1(q)                        1 ulp (0.33)       1 ulp (0.29)        1 ulp (0.29)        1 ulp (0.29)        1 ulp (0.22) / 1 ulp (0.22)
  sqrt(q)                         0 ulp (0.00)       1 ulp (0.33)        1 ulp (0.33)        1 ulp (0.33)        1 ulp (0.24) / 1 ulp (0.24)
  sin(q)                          1 ulp (0.33)       1 ulp (0.29)        1 ulp (0.29)        1 ulp (0.29)        0 ulp (0.00) / 0 ulp (0.00)
  cos(q)                          1 ulp (0.33)       1 ulp (0.29)        1 ulp (0.29)        1 ulp (0.29)        1 ulp (0.29) / 1 ulp (0.29)
  tanh(q)                         1 ulp (0.33)       1.7e-16 abs (0.33)  1.7e-16 abs (0.33)  1.7e-16 abs (0.33)  1.3e-16 abs (0.27) / 1.3e-16 abs (0.27)
  sinh(q)                         1 ulp (0.33)       1 ulp (0.29)        1 ulp (0.29)        1 ulp (0.29)        1 ulp (0.22) / 1 ulp (0.22)
  cosh(q)                         1 ulp (0.33)       1 ulp (0.29)        1 ulp (0.29)        1 ulp (0.29)        1 ulp (0.22) / 1 ulp (0.22)
  atan(q)                         1 ulp (0.33)       2 ulp (0.60)        2 ulp (0.60)        2 ulp (0.60)        1 ulp (0.46) / 1 ulp (0.46)
  erf(q)                          1 ulp (0.33)       411 ulp (0.90)      411 ulp (0.90)      411 ulp (0.90)      9 ulp (0.54) / 9 ulp (0.54)
  erfc(q)                         2 ulp (0.50)       411 ulp (0.90)      411 ulp (0.90)      411 ulp (0.90)      14 ulp (0.64) / 14 ulp (0.64)
  pow(q, 2.5)                     1 ulp (0.33)       2 ulp (0.38)        2 ulp (0.38)        2 ulp (0.35)        2 ulp (0.18) / 2 ulp (0.18)
  pow(q, 4.0)                     1 ulp (0.33)       2 ulp (0.32)        2 ulp (0.32)        1 ulp (0.22)        1 ulp (0.21) / 1 ulp (0.21)
  pow(q, 0.5)                     1 ulp (0.33)       2 ulp (0.24)        2 ulp (0.24)        -                   - / -
  pow(q, T(2.5))                  1 ulp (0.33)       2 ulp (0.35)        2 ulp (0.35)        -                   - / -
  pow(q, T(3.0))                  1 ulp (0.33)       2 ulp (0.37)        2 ulp (0.37)        -                   - / -
  pow(T(1.5), q)                  1 ulp (0.33)       2 ulp (0.19)        2 ulp (0.19)        -                   - / -
  log(q)                          2 ulp (1.00)       0 ulp (0.00)        0 ulp (0.00)        0 ulp (0.00)        0 ulp (0.00) / 0 ulp (0.00)
  log1p(q)                        2 ulp (1.00)       1 ulp (0.67)        1 ulp (0.67)        1 ulp (0.67)        1 ulp (0.30) / 1 ulp (0.30)
  lgamma(q)                       9.1e-13 abs (0.55) 2.8e-13 abs (0.53)  2.8e-13 abs (0.53)  2.8e-13 abs (0.53)  2.3e-13 abs (0.01) / 2.3e-13 abs (0.01)
  softplus(q)                     2 ulp (0.50)       2 ulp (0.15)        2 ulp (0.15)        2 ulp (0.15)        1 ulp (0.09) / 1 ulp (0.09)
  logistic(q)                     2 ulp (0.14)       1.6e-16 abs (0.19)  1.6e-16 abs (0.19)  1.6e-16 abs (0.19)  1.1e-16 abs (0.09) / 1.1e-16 abs (0.09)
  fabs(q)                         0 ulp (0.00)       0 ulp (0.00)        0 ulp (0.00)        0 ulp (0.00)        0 ulp (0.00) / 0 ulp (0.00)
  square(q)                       0 ulp (0.00)       0 ulp (0.00)        0 ulp (0.00)        0 ulp (0.00)        0 ulp (0.00) / 0 ulp (0.00)
  1.0 / q                         0 ulp (0.00)       1 ulp (0.67)        1 ulp (0.67)        1 ulp (0.67)        1 ulp (0.43) / 1 ulp (0.43)
  q / (1.0 + q * q)               2 ulp (0.52)       2.2e-16 abs (0.40)  2.2e-16 abs (0.40)  2.2e-16 abs (0.47)  1.4e-16 abs (0.30) / 1.4e-16 abs (0.30)
  log(q) * 1.4426950408889634     2 ulp (0.34)       1 ulp (0.40)        1 ulp (0.40)        1 ulp (0.40)        1 ulp (0.28) / 1 ulp (0.28)
  log(q) * 0.43429448190325176    4 ulp (0.55)       3 ulp (0.79)        3 ulp (0.79)        2 ulp (0.57)        2 ulp (0.41) / 2 ulp (0.41)
  exp(q * 0.6931471805599453)     20 ulp (0.54)      19 ulp (0.49)       19 ulp (0.49)       19 ulp (0.49)       3 ulp (0.27) / 3 ulp (0.27)
  (in brackets: the fraction of the allowance used; abs: the largest absolute error, where the formula's error is absolute.  Worst
  arguments: erf' / erfc' 411 ulp at x = -25.8; tanh' at -25.3; logistic' at 680; digamma at 1.4643; log_fast 2 ulp at 1.0004.)
"""
import json
import math
import os

import numpy as np
import pytest

import dual_ref as T

pytestmark = pytest.mark.gpu

FN = ("template <class T> __device__ inline __attribute__((always_inline)) T aehmc_fn(int id, T q) {\n  switch (id) {\n"
      + T.switch_source() + "\n  }\n  return q;\n}\n")
FORWARD = FN + """template <class T> __device__ T aehmc_logp(T q, long long i, const double *const *prm) {
  if (prm[0][1] != 0.0) return T(aehmc_fn((int)prm[0][0], value_of(q)));  // T = double: the value alone
  return aehmc_fn((int)prm[0][0], q);
}
"""
D_LANES = 1 + len(T.NAMES)
LANES_LAYOUT = T.blocks(D_LANES, T.NAMES)
LANES = (FN + "template <class V> __device__ auto aehmc_logp(const V &q, const double *const *prm) {\n  typedef decltype(q[0]) T;\n  T lp = T(0.0), s = T(0.0);\n"
         + "".join(f"  lp += aehmc_fn<T>({T.NAMES.index(n)}, q[{lo}]);\n  s += q[{lo}];\n" for n, lo, hi in LANES_LAYOUT)
         + "  return lp + q[0] * s;\n}\n")
HALVES = (T.TRACED[:13], T.TRACED[13:])
REVERSE = {"17a": (17, T.blocks(17, HALVES[0])), "17b": (17, T.blocks(17, HALVES[1])), "70": (70, T.blocks(70, T.TRACED))}
MEASURED = {}  # (route, row) -> ((ulp, argument, error / allowance) of the value, the same of the derivative)


def dev(x):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64, device="cuda")


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    path = os.environ.get("AEHMC_DUAL_REPORT")  # (how the table above and DESIGN.md's were written)
    if path:
        with open(path, "w") as f:
            json.dump({f"{r}|{n}": v for (r, n), v in MEASURED.items()}, f, indent=1)


def forward_eval(name, x, as_double=False):
    from aehmc_amd import nuts, targets
    tgt = targets.Custom(FORWARD, params=[np.array([float(T.NAMES.index(name)), float(as_double)])], dim=1)
    st = nuts.new_state(dev(np.asarray(x, dtype=np.float64).reshape(-1, 1)), tgt)
    return -st.potential_energy.cpu().numpy().reshape(-1), -st.potential_energy_grad.cpu().numpy().reshape(-1)


@pytest.mark.parametrize("name", T.NAMES)
def test_forward_mode_on_the_device_against_50_digits(name):
    x, v, d, va, da = T.reference(name)
    got_v, got_d = forward_eval(name, x)
    dbl = forward_eval(name, x, as_double=True)[0]
    MEASURED["double", name] = (T.worst(name, x, dbl, v, va), None)
    MEASURED["forward", name] = (T.worst(name, x, got_v, v, va), T.worst(name, x, got_d, d, da))
    T.check(name, x, got_v, got_d, what="forward, device:")
    if T.ROWS[name].lib_double:
        assert MEASURED["double", name][0][2] <= 1.0, (name, MEASURED["double", name][0])
    else:
        assert np.array_equal(dbl, got_v)


@pytest.mark.parametrize("name", [n for n in T.NAMES if T.ROWS[n].edges])
def test_forward_mode_edges_on_the_device(name):
    """a row's edges in a call of their own (U = -f and the sum over the one coordinate lose the sign of a zero value)"""
    xs = np.array([e[0] for e in T.ROWS[name].edges])
    got_v, got_d = forward_eval(name, xs)
    dbl = forward_eval(name, xs, as_double=True)[0]
    for x, gv, gd, b in zip(xs, got_v, got_d, dbl):
        assert T.edge_ok(name, x, gv, 0, signed_zero=False), (name, x, "value", gv)
        assert T.edge_ok(name, x, gd, 1), (name, x, "derivative", gd)
        assert T.edge_ok(name, x, b, 0, signed_zero=False), (name, x, "T = double", b)


def check_joint(route, layout, q, v, d, va, da, value, grad):
    """gradient entries pointwise, the value against the 50-digit sum; q[:, 0] may be non-zero (after a transition): the
    coupling term then adds q_0 to every entry (one more rounding) and q_0 sum(q_i) to the value"""
    q0, bad = q[:, :1], []
    for name, lo, hi in layout:
        want = d[:, lo:hi] + q0
        allow = da[:, lo:hi] + np.where(q0 != 0.0, T.ulp(np.abs(d[:, lo:hi]) + np.abs(q0)), 0.0)
        w = T.worst(name, q[:, lo:hi].ravel(), grad[:, lo:hi].ravel(), want.ravel(), allow.ravel())
        MEASURED[route, name] = (None, w)
        if w[2] > 1.0:
            bad.append(f"{route}, device: {name}: derivative off by {w[0]:.1f} ulp at x = {w[1]!r}, {w[2]:.2f} of the allowance")
    assert not bad, "\n".join(bad)
    s = np.array([math.fsum(r[1:]) for r in q])
    np.testing.assert_allclose(grad[:, 0], s, rtol=0, atol=q.shape[1] * T.U * np.abs(q[:, 1:]).sum(1).max())
    terms = np.concatenate([v[:, 1:], q0 * s[:, None]], axis=1)
    allow = np.concatenate([va[:, 1:], 2 * T.U * np.abs(q0 * s[:, None]) + np.abs(q0) * q.shape[1] * T.U * np.abs(q[:, 1:]).sum(1, keepdims=True)], axis=1)
    err = np.abs(value - T.joint_sum(terms))
    assert np.all(err <= T.joint_sum_allowance(terms, allow)), (route, err.max())


def joint_state(tgt, q):
    from aehmc_amd import nuts
    st = nuts.new_state(dev(q), tgt)
    return -st.potential_energy.cpu().numpy(), -st.potential_energy_grad.cpu().numpy()


def test_forward_mode_in_the_lanes_against_50_digits():
    from aehmc_amd import targets
    tgt = targets.CustomJoint(LANES, D_LANES)
    q, v, d, va, da = T.joint_positions(LANES_LAYOUT, D_LANES)
    value, grad = joint_state(tgt, q)
    check_joint("lanes", LANES_LAYOUT, q, v, d, va, da, value, grad)
    eq, meta = T.joint_edges(LANES_LAYOUT, D_LANES)
    value, grad = joint_state(tgt, eq)
    T.check_joint_edges(LANES_LAYOUT, D_LANES, meta, value, grad, what="lanes, device:", others=False)


@pytest.mark.parametrize("key", sorted(REVERSE))
def test_reverse_mode_on_the_device_against_50_digits(key):
    """new_state: the generated adjoint program on a wavefront per chain; then one HMC transition (a leapfrog of step
    2^-40: the points move in their last bits and stay in their domains) on a wavefront per chain and on a workgroup
    per chain (joint_wg = 2), the state it returns checked at the positions it returns"""
    from aehmc_amd import RandomStream, hmc, targets
    from aehmc_amd.engine import get_engine
    D, layout = REVERSE[key]
    tgt = targets.from_callable(T.wrapper(layout), D, reverse=True)
    assert isinstance(tgt, targets.CustomJoint) and "aehmc_logp_grad" in tgt.source
    q, v, d, va, da = T.joint_positions(layout, D)
    value, grad = joint_state(tgt, q)
    check_joint(f"reverse {D}", layout, q, v, d, va, da, value, grad)
    eq, meta = T.joint_edges(layout, D)
    value, grad = joint_state(tgt, eq)
    T.check_joint_edges(layout, D, meta, value, grad, what=f"reverse {D}, device:")
    C = 24
    eng = get_engine()
    try:
        for wg in (0, 2):
            eng.set_option("joint_wg", wg)
            kern = hmc.new_kernel(RandomStream(seeds=range(C)), tgt)
            before = sum(eng.rtc_stats())
            info, _ = kern(hmc.new_state(dev(q[:C]), tgt), 2.0 ** -40, np.ones(D), 1)
            assert sum(eng.rtc_stats()) > before  # (each route brought a program of its own for this density: the option took)
            p = info.state.position.cpu().numpy()
            moved = (p != q[:C]).any(1)
            assert moved.sum() >= C // 2, moved.sum()
            refs = [np.zeros((C, D)) for _ in range(4)]
            for name, lo, hi in layout:
                for dst, src in zip(refs, T.reference_at(name, p[:, lo:hi].ravel())):
                    dst[:, lo:hi] = src.reshape(C, hi - lo)
            check_joint(f"reverse {D} joint_wg={wg}", layout, p, *refs, -info.state.potential_energy.cpu().numpy(),
                        -info.state.potential_energy_grad.cpu().numpy())
    finally:
        eng.set_option("joint_wg", 1)
