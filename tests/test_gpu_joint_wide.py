"""Traced joint densities above 2048 coordinates (up to 10176) on the device: the AEHMC_T_JOINT instantiations of the
workgroup-per-chain kernels (k_nuts_wide / k_hmc_wide compiled against the traced program, the chain's position and
gradient rows in LDS) and the workgroup-per-chain evaluation kernel of new_state and the lock-step path
(k_target_joint_wg).  Oracle: the numpy restatement (oracle/np_oracle.py) driven by THE SAME Python function on plain
arrays and an analytic gradient.  Targets are shared at module scope: every distinct program is a run-time compile."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import np_oracle as no  # noqa: E402

RTOL = 1e-9


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda", dtype=torch.float64)


class NumpyTarget:
    """The numpy restatement's target from the SAME Python function (called on plain arrays) and an analytic gradient."""

    def __init__(self, fn, grad):
        self.fn, self.grad = fn, grad

    def __call__(self, q):
        q = np.asarray(q, dtype=np.float64)
        return float(-self.fn(q)), -np.asarray(self.grad(q), dtype=np.float64)


def funnel(q):
    v, x = q[0], q[1:]
    return -v * v / 18.0 + (-0.5 * x * x * np.exp(-v) - 0.5 * v).sum()


def funnel_grad(q):
    v, x = q[0], q[1:]
    g = np.empty_like(q)
    g[0] = -v / 9.0 + 0.5 * np.sum(x * x) * np.exp(-v) - 0.5 * (len(q) - 1)
    g[1:] = -x * np.exp(-v)
    return g


SCHOOLS_Y = np.array([28.0, 8.0, -3.0, 7.0, -1.0, 1.0, 18.0, 12.0])
SCHOOLS_SIGMA = np.array([15.0, 10.0, 16.0, 11.0, 9.0, 11.0, 10.0, 18.0])
J = 4998  # tiled eight schools: D = J + 2 = 5000
SY, SS = np.resize(SCHOOLS_Y, J), np.resize(SCHOOLS_SIGMA, J)


def schools(q):
    """eight schools, non-centred, tiled: q = [mu, log tau, eta_1..J]"""
    mu, lt, eta = q[0], q[1], q[2:]
    tau = np.exp(lt)
    z = (SY - (mu + tau * eta)) / SS
    return -0.5 * mu * mu / 25.0 - np.log1p(tau * tau / 25.0) + lt + (-0.5 * eta * eta - 0.5 * z * z).sum()


def schools_grad(q):
    mu, lt, eta = q[0], q[1], q[2:]
    tau = np.exp(lt)
    z = (SY - (mu + tau * eta)) / SS
    g = np.empty_like(q)
    g[0] = -mu / 25.0 + np.sum(z / SS)
    g[1] = -(2.0 * tau * tau / 25.0) / (1.0 + tau * tau / 25.0) + 1.0 + np.sum(z * tau * eta / SS)
    g[2:] = -eta + z * tau / SS
    return g


G, NOBS = 5000, 20000  # hierarchical gather model: D = G + 2 = 5002
_r = np.random.default_rng(5)
GROUP = _r.integers(0, G, size=NOBS)
YOBS = 0.4 + _r.normal(size=G)[GROUP] * 0.7 + _r.normal(size=NOBS)


def gather_model(q):
    """random intercepts: q = [mu, log sigma, a_1..a_G]; y_n ~ N(mu + a_{g(n)}, 1), a_g ~ N(0, sigma^2), mu ~ N(0, 1),
    log sigma ~ N(0, 1) -- the position gathered through a data index (reverse sweep: atomic adjoints)"""
    mu, ls, a = q[0], q[1], q[2:]
    r = YOBS - mu - a[GROUP]
    return -0.5 * mu * mu - 0.5 * ls * ls + (-0.5 * a * a * np.exp(-2.0 * ls) - ls).sum() + (-0.5 * r * r).sum()


def gather_grad(q):
    mu, ls, a = q[0], q[1], q[2:]
    r = YOBS - mu - a[GROUP]
    g = np.empty_like(q)
    g[0] = -mu + np.sum(r)
    g[1] = -ls + np.sum(a * a * np.exp(-2.0 * ls) - 1.0)
    g[2:] = -a * np.exp(-2.0 * ls) + np.bincount(GROUP, weights=r, minlength=G)
    return g


MODELS = {"funnel4096": (funnel, funnel_grad, 4096, 0.02), "funnel10000": (funnel, funnel_grad, 10000, 0.02),
          "funnel10176": (funnel, funnel_grad, 10176, 0.02),  # (the largest: 2 (D + 1) doubles of rows fill the LDS)
          "schools5000": (schools, schools_grad, 5000, 0.05), "gather5002": (gather_model, gather_grad, G + 2, 0.003)}


@functools.lru_cache(maxsize=None)
def traced(name, D=None):
    """one traced target per model and size for the whole module (each is a run-time compile)"""
    from aehmc_amd import targets
    fn, _, D0, _ = MODELS[name]
    tgt = targets.from_callable(fn, D or D0)
    assert isinstance(tgt, targets.CustomJoint) and "#define AEHMC_JOINT_GRAD 1" in tgt.source
    return tgt


@pytest.fixture
def eng():
    from aehmc_amd.engine import get_engine
    e = get_engine()
    try:
        yield e
    finally:
        e.set_option("joint_wide", 1)


def _check_step(info, c, o):
    np.testing.assert_allclose(info.state.position[c].cpu().numpy(), o.state.position, rtol=RTOL, atol=1e-11)
    np.testing.assert_allclose(info.state.potential_energy[c].item(), o.state.potential_energy, rtol=RTOL)
    np.testing.assert_allclose(info.state.potential_energy_grad[c].cpu().numpy(), o.state.potential_energy_grad,
                               rtol=RTOL, atol=1e-10)
    assert info.n_leapfrog[c].item() == o.n_leapfrog and info.num_doublings[c].item() == o.num_doublings
    assert bool(info.is_turning[c]) == bool(o.is_turning) and bool(info.is_diverging[c]) == bool(o.is_diverging)


@pytest.mark.parametrize("model", ["funnel4096", "funnel10000", "schools5000"])
def test_new_state_above_2048_coordinates(model):
    """new_state: U and the whole gradient from one sweep of the program by a workgroup (k_target_joint_wg)"""
    from aehmc_amd import nuts
    fn, grad, D, _ = MODELS[model]
    otgt = NumpyTarget(fn, grad)
    q0 = 0.3 * np.random.default_rng(D).normal(size=(3, D))
    state = nuts.new_state(dev(q0), traced(model))
    for c in range(3):
        U, g = otgt(q0[c])
        np.testing.assert_allclose(state.potential_energy[c].item(), U, rtol=1e-12)
        np.testing.assert_allclose(state.potential_energy_grad[c].cpu().numpy(), g, rtol=1e-11, atol=1e-12)


@pytest.mark.parametrize("model", ["funnel4096", "funnel10000", "funnel10176", "schools5000", "gather5002"])
def test_nuts_above_2048_coordinates_matches_numpy(model):
    """NUTS on k_nuts_wide<512, 8 | 16 | 20, true, AEHMC_T_JOINT>: 3 chains x 2 transitions, random diagonal metric"""
    from aehmc_amd import RandomStream, nuts
    fn, grad, D, eps = MODELS[model]
    otgt, tgt = NumpyTarget(fn, grad), traced(model)
    r = np.random.default_rng(D + 1)
    C, n = 3, 2
    q0 = 0.3 * r.normal(size=(C, D))
    imm = 0.5 + r.random(D)
    seeds = [1300 + c for c in range(C)]
    kern = nuts.new_kernel(RandomStream(seeds=seeds), tgt, max_num_expansions=4)
    state = nuts.new_state(dev(q0), tgt)
    okern = [no.nuts_kernel(no.RandomStream(sd), otgt, max_num_expansions=4) for sd in seeds]
    ostate = [no.new_state(q0[c].copy(), otgt) for c in range(C)]
    for _ in range(n):
        info, _ = kern(state, eps, imm)
        state = info.state._replace(momentum=None)
        for c in range(C):
            o = okern[c](ostate[c], eps, imm)
            ostate[c] = o.state._replace(momentum=None)
            _check_step(info, c, o)


def test_hmc_above_2048_coordinates_matches_numpy():
    """HMC (L = 7) on k_hmc_wide<512, 8, AEHMC_T_JOINT, false>: single calls, then sample(3) in one launch pair"""
    from aehmc_amd import RandomStream, hmc
    fn, grad, D, _ = MODELS["funnel4096"]
    otgt, tgt = NumpyTarget(fn, grad), traced("funnel4096")
    r = np.random.default_rng(17)
    C, L, eps = 3, 7, 0.05
    q0 = 0.3 * r.normal(size=(C, D))
    imm = 0.5 + r.random(D)
    seeds = [1700 + c for c in range(C)]
    kern = hmc.new_kernel(RandomStream(seeds=seeds), tgt)
    okern = [no.hmc_kernel(no.RandomStream(sd), otgt) for sd in seeds]
    ostate = [no.new_state(q0[c].copy(), otgt) for c in range(C)]
    info, _ = kern(hmc.new_state(dev(q0), tgt), eps, imm, L)
    for c in range(C):
        o = okern[c](ostate[c], eps, imm, L)
        ostate[c] = o.state._replace(momentum=None)
        np.testing.assert_allclose(info.state.position[c].cpu().numpy(), o.state.position, rtol=RTOL, atol=1e-11)
        np.testing.assert_allclose(info.state.potential_energy[c].item(), o.state.potential_energy, rtol=RTOL)
        np.testing.assert_allclose(info.state.potential_energy_grad[c].cpu().numpy(), o.state.potential_energy_grad,
                                   rtol=RTOL, atol=1e-10)
        np.testing.assert_allclose(info.acceptance_probability[c].item(), o.acceptance_probability, rtol=1e-8)
        assert bool(info.is_diverging[c]) == bool(o.is_diverging)
    samples, info = kern.sample(info.state._replace(momentum=None), eps, imm, L, 3)[:2]
    for c in range(C):
        for t in range(3):
            o = okern[c](ostate[c], eps, imm, L)
            ostate[c] = o.state._replace(momentum=None)
            np.testing.assert_allclose(samples[t, c].cpu().numpy(), o.state.position, rtol=RTOL, atol=1e-11)
        np.testing.assert_allclose(info.state.potential_energy[c].item(), ostate[c].potential_energy, rtol=RTOL)
        np.testing.assert_allclose(info.acceptance_probability[c].item(), o.acceptance_probability, rtol=1e-8)


def test_shared_dense_metric_above_2048_coordinates_on_the_lock_step_path():
    """a shared dense SPD metric, funnel at D = 3000: the lock-step path (GEMMs) with the density evaluated a workgroup per
    live chain (k_target_joint_wg behind the compaction)"""
    from aehmc_amd import RandomStream, nuts
    D = 3000
    otgt, tgt = NumpyTarget(funnel, funnel_grad), traced("funnel4096", D)
    r = np.random.default_rng(30)
    u = r.normal(size=D)
    imm = np.diag(0.6 + 0.8 * r.random(D)) + 0.3 * np.outer(u, u) / D
    imm = 0.5 * (imm + imm.T)
    C, n, eps = 3, 2, 0.02
    q0 = 0.3 * r.normal(size=(C, D))
    seeds = [3000 + c for c in range(C)]
    kern = nuts.new_kernel(RandomStream(seeds=seeds), tgt, max_num_expansions=4)
    state = nuts.new_state(dev(q0), tgt)
    okern = [no.nuts_kernel(no.RandomStream(sd), otgt, max_num_expansions=4) for sd in seeds]
    ostate = [no.new_state(q0[c].copy(), otgt) for c in range(C)]
    for _ in range(n):
        info, _ = kern(state, eps, dev(imm))
        state = info.state._replace(momentum=None)
        for c in range(C):
            o = okern[c](ostate[c], eps, imm)
            ostate[c] = o.state._replace(momentum=None)
            _check_step(info, c, o)


def _run(eng, tgt, D, opt, seeds, q0, imm, eps):
    """two NUTS transitions under option `joint_wide` = opt; also returns how many run-time compiled programs the
    transitions added to the engine (compiled or loaded from the disk cache: the route's kernel, unless the target's
    binding already brought it)"""
    from aehmc_amd import RandomStream, nuts
    eng.set_option("joint_wide", opt)
    kern = nuts.new_kernel(RandomStream(seeds=seeds), tgt, max_num_expansions=5)
    state = nuts.new_state(dev(q0), tgt)
    before = sum(eng.rtc_stats())
    out = []
    for _ in range(2):
        info, _ = kern(state, eps, imm)
        state = info.state._replace(momentum=None)
        out.append(info)
    return out, sum(eng.rtc_stats()) - before


@pytest.mark.parametrize("D,opts", [(1000, (1, 2)), (4096, (0, 1))], ids=["wide_vs_rows_1000", "wide_vs_lockstep_4096"])
def test_joint_wide_route_cross_checks(eng, D, opts):
    """the same transitions on two routes: joint_wide = 2 (the wide kernel) against the default rows kernel at D = 1000,
    the default (wide) against joint_wide = 0 (lock-step path, k_target_joint_wg) at D = 4096.  Discrete outputs
    identical, values to 1e-9 (the kinetic-energy and program sums are associated differently).  The routes differ: the
    first run's kernels came with the target's binding (k_nuts_joint_rows / k_target_joint_wg), the second one brings
    the wide kernel, a program of its own"""
    tgt = traced("funnel4096", D) if D != 4096 else traced("funnel4096")
    r = np.random.default_rng(D + 7)
    C = 6
    q0, imm, seeds = 0.3 * r.normal(size=(C, D)), 0.5 + r.random(D), [4000 + c for c in range(C)]
    a, na = _run(eng, tgt, D, opts[0], seeds, q0, imm, 0.03)
    b, nb = _run(eng, tgt, D, opts[1], seeds, q0, imm, 0.03)
    assert (na, nb) == (0, 1), (na, nb)
    for x, y in zip(a, b):
        for f in ("n_leapfrog", "num_doublings", "is_turning", "is_diverging"):
            assert getattr(x, f).cpu().tolist() == getattr(y, f).cpu().tolist(), f
        np.testing.assert_allclose(x.state.position.cpu().numpy(), y.state.position.cpu().numpy(), rtol=RTOL, atol=1e-11)
        np.testing.assert_allclose(x.state.potential_energy.cpu().numpy(), y.state.potential_energy.cpu().numpy(), rtol=RTOL)
        np.testing.assert_allclose(x.state.potential_energy_grad.cpu().numpy(), y.state.potential_energy_grad.cpu().numpy(),
                                   rtol=RTOL, atol=1e-10)
        np.testing.assert_allclose(x.acceptance_probability.cpu().numpy(), y.acceptance_probability.cpu().numpy(), rtol=1e-8)


def test_joint_wide_2_keeps_the_default_route_up_to_512_coordinates(eng):
    """joint_wide = 2 takes the wide kernel only where the engine's work rows are padded for it (D > 512): at D = 100 NUTS
    stays on its default route -- no further program, the same bits"""
    D = 100
    tgt = traced("funnel4096", D)
    r = np.random.default_rng(D + 7)
    C = 6
    q0, imm, seeds = 0.3 * r.normal(size=(C, D)), 0.5 + r.random(D), [4100 + c for c in range(C)]
    a, _ = _run(eng, tgt, D, 1, seeds, q0, imm, 0.05)
    b, nb = _run(eng, tgt, D, 2, seeds, q0, imm, 0.05)
    assert nb == 0
    for x, y in zip(a, b):
        assert torch.equal(x.state.position, y.state.position) and torch.equal(x.n_leapfrog, y.n_leapfrog)
        assert torch.equal(x.state.potential_energy_grad, y.state.potential_energy_grad)


def test_joint_wide_option_values(eng):
    from aehmc_amd.engine import EngineError
    with pytest.raises(EngineError, match="joint_wide"):
        eng.set_option("joint_wide", 3)


def test_window_adaptation_and_sample_above_2048_coordinates():
    """window_adaptation.run(150) and sample(60), 64 chains, D = 4096, the weakly coupled Gaussian of
    test_gpu_callable.py's window-adaptation test: per-chain step sizes and diagonal metrics on the wide kernel"""
    from aehmc_amd import RandomStream, nuts, window_adaptation
    C, D = 64, 4096
    sd = 0.5 + np.arange(D) % 3

    def logprob_fn(q):
        z = (q - 1.0) / sd
        return -0.5 * (z @ z) - 0.05 * np.sum(z[1:] * z[:-1])   # (weakly coupled neighbours: a joint density)

    kernel = nuts.new_kernel(RandomStream(seeds=range(C)), logprob_fn, max_num_expansions=7)
    state = nuts.new_state(dev(1.0 + 0.3 * np.random.default_rng(1).normal(size=(C, D))), logprob_fn)
    state, (step_size, imm), _ = window_adaptation.run(kernel, state, num_steps=150)
    samples, info, acc, div = kernel.sample(state, step_size, imm, 60)
    s = samples.cpu().numpy().reshape(-1, D)
    assert samples.shape == (60, C, D) and np.isfinite(s).all() and not bool(div.any())
    assert 0.6 < float(acc.mean()) < 0.98
    # (the means in units of each coordinate's scale: over 4096 coordinates the widest ones, sd = 2.5, reach 0.3 of
    #  absolute error from 64 x 60 draws; the average standardised error bounds any common bias much tighter)
    zm = (s.mean(axis=0) - 1.0) / sd
    np.testing.assert_allclose(zm, 0.0, atol=0.25)
    assert abs(zm.mean()) < 0.02, zm.mean()
    np.testing.assert_allclose(s.std(axis=0) / sd, 1.0, atol=0.2)
