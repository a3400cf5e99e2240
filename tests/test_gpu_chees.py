"""The ChEES warm-up on the GPU: aehmc_chees_update with fed inputs against the numpy restatement (tests/chees_ref.py),
the (init, update) loop and chees.run against each other and the restatement, the accept flag and the momentum sign on
the HMC routes it relies on, the adapted (T, eps) against whole reference warm-ups, and chees.sample."""
import json
import math
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chees_ref as cr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULPS = 16 * 2.0 ** -52   # "a few ulp": about ten roundings and libm calls (exp, log, pow: 1 - 2 ulp each) per scalar
SCALARS = ("log_T", "log_T_avg", "adam_m", "adam_v", "da_x", "da_x_avg", "da_g_avg", "da_mu")
SIGMA = np.linspace(1.0, 10.0, 20)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _host_state(st) -> cr.CheesState:
    h = {k: v.cpu().numpy() for k, v in st.items()}
    assert (h["step_size"] == h["step_size"][0]).all()
    return cr.CheesState(int(h["step"][0]), *(float(h[k][0]) for k in ("log_T", "log_T_avg", "adam_m", "adam_v", "h")),
                         int(h["num_steps"][0]), int(h["da_step"][0]),
                         *(float(h[k][0]) for k in ("da_x", "da_x_avg", "da_g_avg", "da_mu")), float(h["step_size"][0]))


def _close(got, want, scale, what):
    """A few ulp of the value, or of the larger operand where the value is a sum of signed terms that may cancel."""
    assert abs(got - want) <= ULPS * max(abs(want), abs(scale)) + 1e-300, (what, got, want)


def _check_scalars(got: cr.CheesState, want: cr.CheesState, before: cr.CheesState):
    """Every field of the device state against the restatement fed the device's sums.  Each scalar is a recurrence on
    its own previous value (``before``), which is therefore the operand whose ulp bounds the error when the new value
    is smaller; da_x = mu - c g_avg takes mu."""
    for name in SCALARS + ("step_size",):
        scale = before.da_mu if name == "da_x" else getattr(before, name)
        _close(getattr(got, name), getattr(want, name), scale, name)
    assert (got.step, got.da_step, got.h) == (want.step, want.da_step, want.h)
    assert got.num_steps == want.num_steps, (got, want)


def _far_from_an_integer(s: cr.CheesState):
    """The condition on the INPUT under which ceil(h T / eps) may be compared for equality."""
    r = cr.ratio(s.h, math.exp(s.log_T), s.step_size)
    return abs(r - round(r)) > 1e-6


def _metric(kind, D, r):
    if kind == "scalar":
        return 0.7
    if kind == "diag":
        return 0.5 + r.random(D)
    A = r.normal(size=(D, D)) / math.sqrt(D)
    M = A @ A.T + np.eye(D)
    return (M + M.T) / 2


@pytest.mark.timeout(60)
@pytest.mark.parametrize("kind", ["scalar", "diag", "dense"])
@pytest.mark.parametrize("C,D", [(1, 1), (3, 1), (5, 7), (64, 64), (65, 65), (130, 129), (257, 1000)])
def test_update_with_fed_inputs(C, D, kind):
    """Three updates in a row (n = 1, 2, 3; the last with is_last) with accept flags mixed, all 1, all 0.  In the mixed
    one some rejected chains carry NaN in their momentum row (and equal before / after positions, since the means run
    over all chains): nothing of those rows may reach S.  S, abar, m0, m1 against fsum values under the bound
    n 2^-52 sum|terms| with n = C (chees_ref.sums; largest |dS| / bound seen: 0.55 at C = 5, D = 7); the scalar outputs against the restatement fed
    the device's own S, A, abar to a few ulp, num_steps equal (h T / eps is checked to be away from an integer); a
    second run of each update from the same state is bit-equal."""
    from aehmc_amd.engine import get_engine
    eng = get_engine()
    r = np.random.default_rng(1000 * C + D)
    imm = _metric(kind, D, r)
    st, cst = eng.chees_alloc(C, D)
    eng.chees_init(C, 0.8, 3.0, cst)
    _check_scalars(_host_state(st), cr.init(0.8, 3.0), cr.init(0.8, 3.0))
    for k, flags in enumerate(("mixed", "ones", "zeros")):
        q0 = r.normal(size=(C, D)) * (1 + r.random(D)) + r.normal(size=D)
        q1 = q0 + r.normal(size=(C, D))
        mom = r.normal(size=(C, D))
        a = r.random(C)
        acc = {"mixed": (r.random(C) < 0.6), "ones": np.ones(C, bool), "zeros": np.zeros(C, bool)}[flags].astype(np.int32)
        if flags == "mixed":
            poisoned = np.flatnonzero(acc == 0)[::2]
            mom[poisoned] = np.nan
            q1[poisoned] = q0[poisoned]
        before = _host_state(st)
        copy = {name: t.clone() for name, t in st.items()}
        args = [_dev(q0), _dev(q1), _dev(mom)]

        def run(state):
            m = args[2]
            if kind == "dense":
                m, diag, scalar = eng.gemm_nt(m, _dev(imm)), None, 1.0
            else:
                diag, scalar = (_dev(imm), 0.0) if kind == "diag" else (None, imm)
            eng.chees_update(C, D, k == 2, 0.651, 0.025, 1000, args[0], args[1], m, diag, scalar, _dev(acc), _dev(a),
                             eng.chees_cstate(state))
        run(st)
        run(copy)
        for name in st:
            assert torch.equal(st[name], copy[name]), (flags, name)
        t = cr.sums(q0, q1, mom, imm, acc, a)
        got = st["sums"].cpu().numpy()
        S, A, abar, m0, m1 = got[0], got[1], got[2], got[3:3 + D], got[3 + D:]
        print(f"C={C} D={D} {kind} {flags}: |dS| / bound = {abs(S - t.S) / max(t.S_bound, 1e-300):.3g}, "
              f"m: {(np.abs(m1 - t.m1) / t.m1_bound).max():.3g}, abar: {abs(abar - t.abar) / t.abar_bound:.3g}")
        assert A == t.A
        assert abs(S - t.S) <= t.S_bound, (flags, S, t.S, t.S_bound)
        if flags == "zeros":
            assert S == 0.0
        assert abs(abar - t.abar) <= t.abar_bound
        assert (np.abs(m0 - t.m0) <= t.m0_bound).all() and (np.abs(m1 - t.m1) <= t.m1_bound).all()
        want = cr.update(before, k == 2, float(S), float(A), float(abar))
        assert _far_from_an_integer(want), "input condition: pick another seed"
        _check_scalars(_host_state(st), want, before)


def _chees_state(cs) -> cr.CheesState:
    """A chees.CheesState (device arrays) as the restatement's tuple of host values."""
    da = cs.da_state
    return cr.CheesState(int(cs.step), float(cs.log_trajectory_length), float(cs.log_trajectory_length_avg),
                         float(cs.adam_m), float(cs.adam_v), float(cs.halton_weight), int(cs.num_steps), int(da.step),
                         float(da.iterates), float(da.iterates_avg), float(da.gradient_avg), float(da.shrinkage_pts),
                         float(cs.step_size[0]))


def _diag_gaussian_kernel(C, sigma, seed0=0):
    import aehmc_amd as aa
    from aehmc_amd import targets
    D = len(sigma)
    target = targets.DiagGaussian(np.zeros(D), np.asarray(sigma, dtype=np.float64))
    kernel = aa.hmc.new_kernel(aa.RandomStream(seeds=range(seed0, seed0 + C)), target)
    q = np.random.default_rng(seed0).normal(size=(C, D))
    return kernel, aa.hmc.new_state(_dev(q), target)


@pytest.mark.timeout(60)
def test_loop_parity_and_run():
    """adaptation()'s (init, update) around hmc.new_kernel, C = 64, D = 5, 30 steps: at every step the WHOLE device state
    against the restatement fed the same transition outputs (num_integration_steps equal: the restatement's h T / eps
    is first checked to stay away from an integer), and chees.run bit-equal to the hand-driven loop."""
    from aehmc_amd import chees
    C, sigma, n = 64, np.linspace(1.0, 3.0, 5), 30
    imm = _dev(np.linspace(0.8, 1.6, 5))
    kernel, state0 = _diag_gaussian_kernel(C, sigma)
    init, update = chees.adaptation(n, inverse_mass_matrix=imm)
    cs, (eps, L) = init(state0)
    ref, state = cr.init(), state0
    assert L == ref.num_steps == 1
    for i in range(n):
        before, used = state.position, L
        info, _ = kernel(state, eps, imm, L)
        state = info.state._replace(momentum=None)
        accepted = (state.position != before).any(1)
        old = cs
        cs, (eps, L) = update(i, cs, before, info, accepted)
        assert int(old.step) == i + 1 and int(cs.step) == i + 2   # (states are values)
        ref = cr.update_from_arrays(ref, i == n - 1, before.cpu().numpy(), state.position.cpu().numpy(),
                                    info.state.momentum.cpu().numpy(), imm.cpu().numpy(), accepted.cpu().numpy(),
                                    info.acceptance_probability.cpu().numpy())
        assert _far_from_an_integer(ref), f"input condition at step {i}: pick another seed"
        assert (info.n_leapfrog == used).all()
        got = _chees_state(cs)
        assert (L, got.num_steps, got.step, got.da_step, got.h) == (ref.num_steps,) * 2 + (ref.step, ref.da_step, ref.h)
        for name in SCALARS + ("step_size",):   # (looser than a few ulp: the restatement runs on its own fsum sums)
            assert getattr(got, name) == pytest.approx(getattr(ref, name), rel=1e-9, abs=1e-12), (i, name)
    kernel2, state2 = _diag_gaussian_kernel(C, sigma)
    last, (step_size, imm_out, T), updates = chees.run(kernel2, state2, n, imm)
    assert imm_out is imm and len(updates) == 1
    assert step_size == float(eps.value[0]) and T == math.exp(float(cs.log_trajectory_length))
    assert torch.equal(last.position, state.position) and torch.equal(last.potential_energy, state.potential_energy)


# (C, D, dense metric, step size of the mixed transition).  The engine does not expose the route it took; each shape
# relies on these conditions of hmc_path (csrc/engine.hip) for a DiagGaussian target with the default options:
#   fused                diagonal metric, D <= 1024                      (hmc_fused_supported -> k_hmc_fused)
#   workgroup_per_chain  diagonal metric, 1024 < D <= 10176              (hmc_resident_supported -> k_hmc_wide)
#   block_dense          shared dense metric, 65 <= D <= 512             (block_dense_supported -> k_hmc_block_*)
#   lock_step            shared dense metric, D > 512: no family takes it (HMC_PATH_LOCKSTEP)
# A change of those thresholds has to move the shapes along.
ROUTES = {
    "fused": (64, 5, False, 1.5),
    "workgroup_per_chain": (32, 1100, False, 0.25),
    "block_dense": (32, 72, True, 0.55),
    "lock_step": (16, 520, True, 0.33),
}


@pytest.mark.timeout(60)
@pytest.mark.parametrize("route", list(ROUTES))
def test_accept_flag_and_momentum_sign(route):
    """What the update reads off a transition, on each HMC route ChEES may run on: ``out["flags"][0]`` is "the position
    changed" per chain (a transition with both outcomes), and for accepted chains -imm . momentum is the velocity the
    trajectory ARRIVED with: after a short trajectory (2 leapfrogs of 0.05) it points away from the start,
    <q_after - q_before, v> > 0."""
    from aehmc_amd._common import Layout, bind_target
    from aehmc_amd.engine import get_engine
    C, D, dense, eps_mixed = ROUTES[route]
    eng = get_engine()
    kernel, state = _diag_gaussian_kernel(C, np.linspace(1.0, 2.0, D), seed0=7)
    r = np.random.default_rng(D)
    if dense:
        A = r.normal(size=(D, D)) / (4 * math.sqrt(D))
        imm = _dev(np.eye(D) + (A + A.T) / 2)
    else:
        imm = _dev(1.0 + 0.2 * r.random(D))
    k = kernel._hmc
    q, U, g = bind_target(k, eng, state, Layout((C, D), True, C), False)
    eng.set_metric(imm, D)
    for eps, L, mixed in ((0.05, 2, False), (eps_mixed, 3, True)):
        before = q.clone()
        out = eng.hmc_step(k["holder"]["rng"], eps, L, k["divergence_threshold"], q, U, g)
        flag = out["flags"][0].bool()
        moved = (q != before).any(1)
        print(f"{route}: eps {eps}: {int(flag.sum())} of {C} accepted")
        assert torch.equal(flag, moved)
        if mixed:
            assert bool(flag.any()) and not bool(flag.all()), "input condition: a transition with both outcomes"
        else:
            assert int(flag.sum()) >= C // 2
            v = -(out["momentum"] @ imm) if dense else -(imm * out["momentum"])
            assert bool((((q - before) * v).sum(1)[flag] > 0).all())


@pytest.fixture(scope="module")
def stat_runs():
    """chees.run on the two statistical targets: C = 256, 800 steps, DiagGaussian sigma = linspace(1, 10, 20) with the
    identity metric and with imm = sigma (effective scales 1 ... sqrt(10)); shared by the tests below."""
    from aehmc_amd import chees
    out = {}
    for name, imm in (("identity", 1.0), ("imm_sigma", _dev(SIGMA))):
        kernel, state = _diag_gaussian_kernel(256, SIGMA, seed0=100)
        state, params, _ = chees.run(kernel, state, 800, imm)
        out[name] = (kernel, state, params)
    return out


@pytest.mark.timeout(120)   # (with the module fixture: two warm-ups of 800 steps, well under a second each)
@pytest.mark.parametrize("name", ["identity", "imm_sigma"])
def test_adapted_values_are_a_draw_from_the_reference_distribution(stat_runs, name):
    """The device's final T and eps within mean +- 5 sd of the restatement's 16 seeds (tests/golden/chees_ref_runs.json,
    whose spread of T is checked to be below 5 % on the CPU): the device run is one more draw from that distribution.
    A wrong momentum sign, a dropped Halton weight or means over accepted chains only move T by a factor or to a clamp.
    Reference, 16 seeds: identity T = 18.4 (sd 0.16), eps = 1.69; imm = sigma T = 5.53, eps = 1.55."""
    gold = np.array(json.load(open(os.path.join(ROOT, "tests", "golden", "chees_ref_runs.json")))["runs"][name])
    mean, sd = gold.mean(0), gold.std(0, ddof=1)
    _, _, (eps, _, T) = stat_runs[name]
    print(f"{name}: device T = {T:.4f}, eps = {eps:.4f}; reference T = {mean[0]:.4f} +- {sd[0]:.4f}, "
          f"eps = {mean[1]:.4f} +- {sd[1]:.4f}")
    assert abs(T - mean[0]) <= 5 * sd[0], (T, mean[0], sd[0])
    assert abs(eps - mean[1]) <= 5 * sd[1], (eps, mean[1], sd[1])


@pytest.mark.timeout(60)
def test_sample_lengths_and_draws():
    """chees.sample: transition i runs L_i = max(1, ceil(halton(first + i) T / eps)) leapfrogs; its draws are bit-equal
    to a loop of kernel calls with those lengths; ``jitter=False`` is kernel.sample at ceil(T / eps)."""
    from aehmc_amd import chees
    sigma, C, N = np.linspace(1.0, 3.0, 5), 8, 6
    eps, T, imm = 0.37, 2.9, _dev(np.linspace(0.8, 1.6, 5))
    lengths = [max(1, math.ceil(cr.halton(3 + i) * T / eps)) for i in range(N)]
    assert lengths == [chees.num_integration_steps(eps, T, 3 + i) for i in range(N)] and len(set(lengths)) > 2
    kernel, state = _diag_gaussian_kernel(C, sigma)
    draws, info, acc, div = chees.sample(kernel, state, eps, imm, T, N, first=3)
    assert draws.shape == (N, C, 5) and acc.shape == (N, C) and div.shape == (N, C) and div.dtype == torch.bool
    assert (info.n_leapfrog == lengths[-1]).all() and torch.equal(info.state.position, draws[-1])
    kernel2, s = _diag_gaussian_kernel(C, sigma)
    for i, L in enumerate(lengths):
        step, _ = kernel2(s, eps, imm, L)
        assert (step.n_leapfrog == L).all()
        s = step.state._replace(momentum=None)
        assert torch.equal(draws[i], s.position) and torch.equal(acc[i], step.acceptance_probability)
    one, info1, _, _ = chees.sample(kernel, info.state._replace(momentum=None), eps, imm, T, 1, first=3 + N)
    assert (info1.n_leapfrog == chees.num_integration_steps(eps, T, 3 + N)).all()
    kernel3, s3 = _diag_gaussian_kernel(C, sigma)
    kernel4, s4 = _diag_gaussian_kernel(C, sigma)
    fixed, info3, acc3, _ = chees.sample(kernel3, s3, eps, imm, T, N, jitter=False)
    want, info4, acc4, _ = kernel4.sample(s4, eps, imm, math.ceil(T / eps), N)
    assert torch.equal(fixed, want) and torch.equal(acc3, acc4)
    none, _, _, _ = chees.sample(kernel3, s3, eps, imm, T, 2, keep_samples=False)
    assert none is None


@pytest.mark.timeout(120)   # (the fixture again, should this test be selected alone)
@pytest.mark.parametrize("name", ["identity", "imm_sigma"])
def test_sample_after_run_recovers_the_target(stat_runs, name):
    """200 jittered draws per chain after the warm-up: the mean of every coordinate within 5 MCSE of 0 and
    R-hat < 1.05 (summary.summarize)."""
    from aehmc_amd import chees, summary
    kernel, state, (eps, imm, T) = stat_runs[name]
    draws, _, acc, _ = chees.sample(kernel, state, eps, imm, T, 200)
    s = summary.summarize(draws)
    mean, mcse, rhat, sd = (x.cpu().numpy() for x in (s.mean, s.mcse, s.rhat, s.sd))
    print(f"{name}: acceptance {float(acc.mean()):.3f}, max |mean| / mcse = {np.abs(mean / mcse).max():.2f}, "
          f"max rhat = {rhat.max():.4f}, ess min = {float(s.ess.min()):.0f}, sd / sigma = {(sd / SIGMA).round(3)}")
    assert (np.abs(mean) <= 5 * mcse).all(), (mean / mcse)
    assert (rhat < 1.05).all(), rhat
