"""Per-transition trajectory lengths: ``kernel.sample(state, eps, imm, <lengths>, N)`` and ``summary.run`` with a list of
lengths against the loop of single transitions ``kernel(state, eps, imm, L_i)``, bit for bit, on every HMC route: the ones
whose kernels read the lengths from device memory (one launch) and the ones the engine runs as single transitions."""
import math
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_chees import ROUTES, _dev, _diag_gaussian_kernel  # noqa: E402

LENGTHS = [3, 1, 0, 7, 1, 4, 7]  # L = 1, a repeat, the maximum twice, a zero


def funnel(q):  # README: a Python logprob_fn, traced
    v, x = q[0], q[1:]
    return -v * v / 18.0 + (-0.5 * x * x * np.exp(-v) - 0.5 * v).sum()


STUDENT_T = """
  template <class T> __device__ T aehmc_logp(T q, long long i, const double *const *prm) {
    const double nu = prm[0][i];
    return -0.5 * (nu + 1.0) * log1p(q * q / nu);
  }"""


def _route(route):
    """(factory of (kernel, state), step size, metric) of one of test_gpu_chees.ROUTES, with its metric as there."""
    C, D, dense, eps = ROUTES[route]
    r = np.random.default_rng(D)
    if dense:
        A = r.normal(size=(D, D)) / (4 * math.sqrt(D))
        imm = _dev(np.eye(D) + (A + A.T) / 2)
    else:
        imm = _dev(1.0 + 0.2 * r.random(D))
    return (lambda: _diag_gaussian_kernel(C, np.linspace(1.0, 2.0, D), seed0=7)), eps, imm


def _other(name):
    """The routes beyond ROUTES: (factory, step size, metric)."""
    import aehmc_amd as aa
    from aehmc_amd import PerChain, targets
    r = np.random.default_rng(5)

    def factory(target, C, D, q0=None):
        q = r.normal(size=(C, D)) if q0 is None else q0

        def make():
            kernel = aa.hmc.new_kernel(aa.RandomStream(seeds=range(40, 40 + C)), target)
            return kernel, aa.hmc.new_state(_dev(q), target)
        return make
    if name == "fused_dense":  # shared dense metric, D <= 64: k_hmc_fused_dense
        C, D = 8, 6
        A = r.normal(size=(D, D)) / (2 * math.sqrt(D))
        return factory(targets.DiagGaussian(np.zeros(D), np.linspace(1.0, 2.0, D)), C, D), 0.9, _dev(np.eye(D) + (A + A.T) / 2)
    if name == "custom_fused":  # coordinate-wise targets.Custom: the run-time compiled k_hmc_fused
        C, D = 8, 5
        return factory(targets.Custom(STUDENT_T, params=[np.linspace(3.0, 7.0, D)]), C, D), 0.8, _dev(0.5 + r.random(D))
    if name == "traced_funnel":  # the README's funnel, D = 10: the run-time compiled k_hmc_fused_dense
        return factory(funnel, 8, 10), 0.35, 1.0
    if name == "traced_funnel_100":  # 64 < D <= 1024: the run-time compiled k_hmc_fused with the program's rows in LDS
        return factory(funnel, 8, 100, 0.3 * r.normal(size=(8, 100))), 0.12, _dev(0.5 + r.random(100))
    if name == "regression":  # k_hmc_linreg (beyond the required set: reads the lengths on the device too)
        X = r.normal(size=300)
        return factory(targets.LinearRegression(X, 3 * X + r.normal(size=300)), 8, 2, 0.3 * r.normal(size=(8, 2))), 0.04, _dev(np.array([0.7, 1.3]))
    if name == "per_chain_dense":  # k_hmc_pc_dense: a route left on single transitions inside the engine
        C, D = 5, 70
        A = r.normal(size=(C, D, D)) / (4 * math.sqrt(D))
        imm = np.eye(D)[None] + 0.5 * (A + A.transpose(0, 2, 1))
        eps = 0.5 * (0.5 + r.random(C))
        return (factory(targets.DiagGaussian(np.zeros(D), np.linspace(1.0, 2.0, D)), C, D), PerChain(_dev(eps)),
                PerChain(_dev(imm)))
    raise KeyError(name)


def _loop(make, eps, imm, lengths):
    """The reference: single transitions.  Returns (draws, acc, div, last Diagnostics, generator states)."""
    kernel, s = make()
    draws, acc, div, step, updates = [], [], [], None, None
    for L in lengths:
        step, updates = kernel(s, eps, imm, L)
        assert (step.n_leapfrog == L).all()
        s = step.state._replace(momentum=None)
        draws.append(s.position.clone())
        acc.append(step.acceptance_probability.clone())
        div.append(step.is_diverging.clone())
    (rng,) = updates.values()
    return torch.stack(draws), torch.stack(acc), torch.stack(div), step, rng.clone()


def _assert_same(make, eps, imm, lengths, mixed=False):
    want, wacc, wdiv, last, wrng = _loop(make, eps, imm, lengths)
    if mixed:  # input condition: accepted and rejected transitions both occur
        prev = torch.cat([make()[1].position[None], want[:-1]])
        moved = (want != prev).reshape(len(lengths), want.shape[1], -1).any(2)[[L > 0 for L in lengths]]
        print(f"{int(moved.sum())} of {moved.numel()} transitions accepted")
        assert bool(moved.any()) and not bool(moved.all()), "input condition: accepts and rejects both occur"
    kernel, state = make()
    draws, info, acc, div = kernel.sample(state, eps, imm, lengths, len(lengths))
    assert torch.equal(draws, want) and torch.equal(acc, wacc) and torch.equal(div, wdiv)
    assert torch.equal(info.state.position, last.state.position)
    assert torch.equal(info.state.potential_energy, last.state.potential_energy)
    assert torch.equal(info.state.potential_energy_grad, last.state.potential_energy_grad)
    assert torch.equal(info.state.momentum, last.state.momentum)
    assert torch.equal(info.acceptance_probability, last.acceptance_probability)
    assert (info.n_leapfrog == sum(lengths)).all()
    assert torch.equal(kernel._hmc["holder"]["rng"], wrng)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("route", list(ROUTES))
def test_sample_with_lengths_on_the_chees_routes(route):
    """fused 64 x 5, workgroup per chain 32 x 1100, block dense 32 x 72, lock-step 16 x 520 (single transitions inside
    the engine), each at its mixed step size."""
    make, eps, imm = _route(route)
    _assert_same(make, eps, imm, LENGTHS, mixed=True)
    assert sum(LENGTHS) == 23


@pytest.mark.timeout(180)
@pytest.mark.parametrize("name", ["fused_dense", "custom_fused", "traced_funnel", "traced_funnel_100", "regression",
                                  "per_chain_dense"])
def test_sample_with_lengths_on_the_other_routes(name):
    make, eps, imm = _other(name)
    _assert_same(make, eps, imm, LENGTHS)


@pytest.mark.timeout(120)
def test_fused_route_with_fp_contract():
    """The contracted trajectory loop is separate code with an L - 1 trip count; the reference runs in the same mode."""
    from aehmc_amd.engine import get_engine
    eng = get_engine()
    make, eps, imm = _route("fused")
    eng.set_option("fp_contract", 1)
    try:
        _assert_same(make, eps, imm, LENGTHS)
        make, eps, imm = _route("workgroup_per_chain")
        _assert_same(make, eps, imm, LENGTHS)
    finally:
        eng.set_option("fp_contract", 0)


@pytest.mark.timeout(120)
def test_wide_route_across_momentum_chunks():
    """More transitions than one chunk of drawn momenta holds (22 with the HMC workspace at this shape): the second and
    third chunk read their own slices of the lengths."""
    make, eps, imm = _route("workgroup_per_chain")
    _assert_same(make, eps, imm, (LENGTHS * 7)[:47])


@pytest.mark.timeout(120)
@pytest.mark.parametrize("route", ["fused", "block_dense", "lock_step"])
def test_constant_lengths_equal_the_int_call(route):
    make, eps, imm = _route(route)
    k1, s1 = make()
    k2, s2 = make()
    a = k1.sample(s1, eps, imm, torch.full((5,), 4, dtype=torch.int64), 5)
    b = k2.sample(s2, eps, imm, 4, 5)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    assert torch.equal(a[1].state.position, b[1].state.position) and torch.equal(a[1].state.momentum, b[1].state.momentum)
    assert torch.equal(a[1].n_leapfrog, b[1].n_leapfrog) and (a[1].n_leapfrog == 20).all()
    assert torch.equal(k1._hmc["holder"]["rng"], k2._hmc["holder"]["rng"])


def test_bad_lengths_raise_and_an_int_still_works():
    make, eps, imm = _route("fused")
    kernel, state = make()
    with pytest.raises(ValueError):
        kernel.sample(state, eps, imm, [3, 1], 3)
    with pytest.raises(ValueError):
        kernel.sample(state, eps, imm, [3, -1, 2], 3)
    with pytest.raises(ValueError):
        kernel.sample(state, eps, imm, np.array([3.5, 1.0, 2.0]), 3)
    draws, info, _, _ = kernel.sample(state, eps, imm, np.int64(3), 2)
    assert draws.shape[0] == 2 and (info.n_leapfrog == 6).all()
    draws, info, _, _ = kernel.sample(state, eps, imm, np.array([3, 0, 2]), 3)
    assert draws.shape[0] == 3 and (info.n_leapfrog == 5).all()


@pytest.mark.timeout(120)
def test_summary_run_hands_each_chunk_its_slice():
    from aehmc_amd import summary
    make, eps, imm = _route("fused")
    k1, s1 = make()
    k2, s2 = make()
    draws, info, acc, div = k1.sample(s1, eps, imm, LENGTHS, len(LENGTHS))
    s, rinfo, racc, rdiv = summary.run(k2, s2, eps, imm, len(LENGTHS), num_integration_steps=LENGTHS, chunk=3)
    assert torch.equal(racc, acc) and torch.equal(rdiv, div)
    assert torch.equal(rinfo.state.position, info.state.position)
    assert torch.equal(rinfo.state.potential_energy, info.state.potential_energy)
    assert torch.equal(rinfo.state.potential_energy_grad, info.state.potential_energy_grad)
    assert (rinfo.n_leapfrog == sum(LENGTHS)).all()
    assert torch.equal(k1._hmc["holder"]["rng"], k2._hmc["holder"]["rng"])
    assert torch.equal(s.mean, summary.summarize(draws).mean)
