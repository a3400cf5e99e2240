"""Generalised HMC and the MEADS warm-up on the GPU against the numpy restatement (tests/meads_ref.py): the transition with
fixed parameters bit for bit where it is elementwise, the user-defined routes, aehmc_meads_update with fed inputs,
meads.run against the hand-driven loop and the restatement, and the adapted parameters against the golden seeds."""
import functools
import json
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meads_ref as mr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = mr.PARITY


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _np(t):
    return t.detach().cpu().numpy()


def _target(t):
    from aehmc_amd import targets
    if isinstance(t, mr.StdNormal):
        return targets.StdNormal()
    if isinstance(t, mr.Isotropic):
        return targets.IsoGaussian()
    return targets.DiagGaussian(t.mu, t.sigma)


def _kernel(target, seeds, q0):
    """A GHMC kernel built FIRST from its stream (so its two sites are meads_ref.sites(seeds)) and the starting state."""
    import aehmc_amd as aa
    kernel = aa.ghmc.new_kernel(aa.RandomStream(seeds=seeds), target)
    return kernel, aa.ghmc.new_state(_dev(q0), target)


def _rel(got, want, tol, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
    assert (err <= tol).all(), (what, float(err.max()))
    return float(err.max()) if err.size else 0.0


@functools.lru_cache(maxsize=None)
def _parity_ref(name, C, D):
    return mr.parity_run(name, C, D)


@pytest.mark.timeout(60)
@pytest.mark.parametrize("name", mr.PARITY_TARGETS)
@pytest.mark.parametrize("C,D", mr.PARITY_SHAPES)
def test_transition_against_the_restatement(C, D, name):
    """12 single transitions at eps = 0.37, alpha = 0.6, delta = 0.3, s = linspace(0.8, 1.6, D): accept flags equal (the
    reference's margins are checked on the host), position, gradient and momentum bit-equal, U, slice and acceptance
    probability to 1e-12 relative, and the generator states numpy's afterwards (site #2 advanced by one double).

    The slice: ``fmod((u + 1) + delta, 2) - 1`` works on numbers of size 1 to 2, so a slice carries an ABSOLUTE error of
    some 1e-16 whatever its own size, in the restatement as on the device, and with 64 chains and 12 transitions some
    |u| is below 1e-3 in every fixture (a first draft that divided the free-running difference by |u| measured
    1.01e-12 at C = D = 64, |u| = 1.7e-4: one ulp of u + 1).  The 1e-12 RELATIVE bound is therefore asked of every
    single transition -- the device's slice against the restatement's one-step map of the device's own incoming slice,
    where the drift is the same bits on both sides and only exp(-Delta) differs.  The free-running slices are compared
    too, on the slice's own scale (|u| < 1): every transition multiplies by exp(-Delta), and Delta is a difference of
    two energies H, each a sum of D terms taken in another order on the device (lane-strided, then a butterfly) than in
    numpy (pairwise) -- up to about log2(D) + a few roundings of size H on either side.  Allowed after k transitions:
    k * 16 * 2^-52 * max H  (D = 1: 1e-14 after 12; D = 1000, H = 1400: 6e-11)."""
    t, q0, hist, (g1, g2) = _parity_ref(name, C, D)
    kernel, state = _kernel(_target(t), mr.parity_seeds(name, C, D), q0)
    s = _dev(mr.parity_scale(D))
    worst, drift, hmax, u_in = 0.0, 0.0, 1.0, None
    for k, (ch, info_ref) in enumerate(hist):
        info, updates = kernel(state, P["eps"], s, P["alpha"], P["delta"])
        state = info.state
        assert np.array_equal(_np(info.is_turning), info_ref.accepted), k
        assert np.array_equal(_np(info.is_diverging), info_ref.is_diverging), k
        for got, want, what in ((state.position, ch.q, "q"), (state.potential_energy_grad, ch.g, "g"), (state.momentum, ch.v, "v")):
            assert np.array_equal(_np(got), want), (k, what, float(np.abs(_np(got) - want).max()))
        u_dev = _np(state.slice)
        u_want = ch.u if u_in is None else mr.slice_step(u_in, info_ref, P["delta"])
        worst = max(worst, _rel(_np(state.potential_energy), ch.U, 1e-12, "U"), _rel(u_dev, u_want, 1e-12, "slice"),
                    _rel(_np(info.acceptance_probability), info_ref.acceptance_probability, 1e-12, "acceptance_probability"))
        drift = max(drift, float(np.abs(u_dev - ch.u).max()))
        hmax = max(hmax, float((np.abs(ch.U) + 0.5 * np.sum(ch.v * ch.v, axis=1)).max()))
        assert drift <= (k + 1) * 16 * 2.0 ** -52 * hmax, (k, "free-running slice", drift, hmax)
        u_in = u_dev
        assert (_np(info.n_leapfrog) == 1).all()
    print(f"{name} C={C} D={D}: largest relative error of U, slice (per transition), acceptance probability: {worst:.3g}; "
          f"free-running slice: {drift:.3g} absolute")
    (rng,) = updates.values()
    assert np.array_equal(_np(rng).view(np.uint64).reshape(C, 2, 4), mr.site_states(g1, g2))


@pytest.mark.timeout(60)
@pytest.mark.parametrize("C,D", [(3, 1), (5, 7), (65, 65), (5, 257), (4, 1024)])
def test_sample_is_the_loop_of_single_calls(C, D):
    """.sample(12) equals 12 single calls bit for bit, samples[-1] is the final position, n_leapfrog = 12, and a call
    with momentum and slice handed back (5 + 7) continues bit-equal to the one longer call."""
    name = "diag_gaussian"
    t, q0, hist, _ = _parity_ref(name, C, D)
    s = _dev(mr.parity_scale(D))
    args = (P["eps"], s, P["alpha"], P["delta"])
    seeds = mr.parity_seeds(name, C, D)
    kernel, state = _kernel(_target(t), seeds, q0)
    singles = []
    for _ in range(12):
        info, _ = kernel(state, *args)
        state = info.state
        singles.append((state.position.clone(), float(info.acceptance_probability.sum())))
    kernel, state0 = _kernel(_target(t), seeds, q0)
    samples, info, acc, div = kernel.sample(state0, *args, 12)
    assert samples.shape == (12, C, D) and acc.shape == (12, C) and div.shape == (12, C)
    for k in range(12):
        assert torch.equal(samples[k], singles[k][0]), k
    assert torch.equal(samples[-1], info.state.position) and (info.n_leapfrog == 12).all()
    for a, b in zip(info.state, state):
        assert torch.equal(a, b)
    assert np.array_equal(_np(info.state.position), hist[-1][0].q)
    kernel, state0 = _kernel(_target(t), seeds, q0)
    first, info5, _, _ = kernel.sample(state0, *args, 5)
    second, info7, _, _ = kernel.sample(info5.state, *args, 7, keep_samples=True)
    assert torch.equal(torch.cat([first, second]), samples)
    for a, b in zip(info7.state, info.state):
        assert torch.equal(a, b)


_DIAG_ELEM = '''__device__ void aehmc_custom_elem(double q, long long i, const double *const *prm, double &u, double &g) {
  const double z = (q - prm[0][i]) / prm[1][i];
  u = 0.5 * (z * z) + log(prm[1][i]) + 0.91893853320467267;
  g = z / prm[1][i];
}'''


@pytest.mark.timeout(120)
@pytest.mark.parametrize("C,D", [(5, 7), (5, 257)])
def test_custom_source_of_the_diagonal_gaussian(C, D):
    """targets.Custom with the diagonal Gaussian written by the user against the built-in target, 12 transitions: 1e-12."""
    from aehmc_amd import targets
    t, q0, _, _ = _parity_ref("diag_gaussian", C, D)
    seeds = mr.parity_seeds("diag_gaussian", C, D)
    args = (P["eps"], _dev(mr.parity_scale(D)), P["alpha"], P["delta"], 12)
    kernel, state = _kernel(_target(t), seeds, q0)
    want, winfo, wacc, _ = kernel.sample(state, *args)
    custom = targets.Custom(_DIAG_ELEM, params=[t.mu, t.sigma], dim=D)
    kernel, state = _kernel(custom, seeds, q0)
    got, ginfo, gacc, _ = kernel.sample(state, *args)
    assert torch.equal(ginfo.is_turning, winfo.is_turning)
    scale = float(want.abs().max())
    assert float((got - want).abs().max()) <= 1e-12 * scale
    _rel(_np(ginfo.state.potential_energy), _np(winfo.state.potential_energy), 1e-12, "U")
    _rel(_np(gacc), _np(wacc), 1e-12, "acceptance history")


@pytest.mark.timeout(180)
@pytest.mark.parametrize("D", mr.FUNNEL_DIMS)
def test_traced_funnel_against_the_restatement(D):
    """A Python function traced with its reverse-mode program against the restatement's analytic gradient, 6 transitions
    at eps = 0.05 with a scalar scale: 1e-9 relative (to the largest entry for the vectors)."""
    from aehmc_amd import targets
    t, q0, seeds, hist = mr.funnel_run(D)
    kernel, state = _kernel(targets.from_callable(mr.funnel_logp, D, reverse=True), seeds, q0)
    for k, (ch, info_ref) in enumerate(hist):
        info, _ = kernel(state, 0.05, 1.0, P["alpha"], P["delta"])
        state = info.state
        assert np.array_equal(_np(info.is_turning), info_ref.accepted), k
        for got, want, what in ((state.position, ch.q, "q"), (state.potential_energy_grad, ch.g, "g"), (state.momentum, ch.v, "v")):
            assert np.abs(_np(got) - want).max() <= 1e-9 * np.abs(want).max(), (k, what)
        _rel(_np(state.potential_energy), ch.U, 1e-9, "U")
        _rel(_np(state.slice), ch.u, 1e-9, "slice")
        _rel(_np(info.acceptance_probability), info_ref.acceptance_probability, 1e-9, "acceptance_probability")


@pytest.mark.timeout(120)
def test_refused_configurations():
    import aehmc_amd as aa
    from aehmc_amd import ghmc, targets
    r = np.random.default_rng(3)
    C = 3

    def call(target, D, scale=1.0):
        kernel, state = _kernel(target, range(C), r.normal(size=(C, D)))
        return kernel(state, 0.1, scale, 0.5, 0.25)

    A = r.normal(size=(4, 4))
    with pytest.raises(ValueError, match="not supported"):
        call(targets.DenseMVN(np.zeros(4), A @ A.T + np.eye(4)), 4)
    with pytest.raises(ValueError, match="not supported"):
        call(targets.LinearRegression(r.normal(size=16), r.normal(size=16)), 2)
    with pytest.raises(ValueError, match="1024"):
        call(targets.StdNormal(), 1025)
    with pytest.raises(ValueError, match="reverse-mode program"):
        call(targets.from_callable(mr.funnel_logp, 10, reverse=False), 10)
    with pytest.raises(ValueError, match="entries"):
        call(targets.StdNormal(), 4, scale=torch.ones(3, dtype=torch.float64))
    with pytest.raises(ValueError, match="PerChain"):
        call(targets.StdNormal(), 4, scale=aa.PerChain(torch.ones(C, 4, dtype=torch.float64)))
    info, _ = call(targets.StdNormal(), 4)  # and the engine is in working order afterwards
    assert isinstance(info.state, ghmc.GhmcState) and torch.isfinite(info.state.position).all()


SUMS = ("z4", "z2", "g4", "g2", "Fz", "Fg", "lam_z", "lam_g")


def _close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert (np.abs(got - want) <= 1e-9 * np.abs(want) + 1e-12).all(), (what, got, want)


@pytest.mark.timeout(60)
@pytest.mark.parametrize("C,D", [(2, 1), (3, 2), (5, 7), (64, 64), (65, 65), (130, 129), (257, 1000)])
def test_update_with_fed_inputs(C, D):
    """Two updates in a row (count 0 and 1) on random Q, G: every intermediate sum and every parameter within 1e-9
    relative + 1e-12 of the restatement (which forms the C x C matrix), a second run from the same state bit-equal; then
    the guard: two chains made identical in one coordinate leave the parameters and count one skip."""
    from aehmc_amd.engine import get_engine
    eng = get_engine()
    r = np.random.default_rng(1000 * C + D)
    st = eng.meads_alloc(D, 0.01, with_sums=True)
    ref = mr.init(D, 0.01)
    for k in range(2):
        Q = r.normal(size=(C, D)) * (0.5 + 2 * r.random(D)) + r.normal(size=D)
        G = r.normal(size=(C, D)) * (0.5 + r.random(D))
        copy = {n: t.clone() for n, t in st.items()}
        eng.meads_update(C, D, _dev(Q), _dev(G), 0.5, 1.0, st)
        eng.meads_update(C, D, _dev(Q), _dev(G), 0.5, 1.0, copy)
        for n in st:
            assert torch.equal(st[n], copy[n]), (k, n)
        want, ref = mr.statistics(Q, G), mr.update(ref, Q, G)
        sums = _np(st["sums"])
        for i, n in enumerate(SUMS):
            _close(sums[i], want[n], n)
        _close(sums[8:8 + D], want["m"], "m")
        _close(sums[8 + D:], want["sd"], "sd")
        _close(_np(st["params"]), [ref.eps, ref.alpha, ref.delta], "params")
        _close(_np(st["scale"]), ref.scale, "scale")
        assert (int(st["count"]), int(st["skipped"])) == (ref.count, ref.skipped) == (k + 1, 0)
    Q = r.normal(size=(C, D))
    Q[:, D - 1] = 1.25  # sd = 0 in the last coordinate
    before = {n: t.clone() for n, t in st.items()}
    eng.meads_update(C, D, _dev(Q), _dev(r.normal(size=(C, D))), 0.5, 1.0, st)
    assert torch.equal(st["params"], before["params"]) and torch.equal(st["scale"], before["scale"])
    assert (int(st["count"]), int(st["skipped"])) == (3, 1)
    with pytest.raises(ValueError, match="at least 2"):
        from aehmc_amd.ghmc import engine_call
        engine_call(eng.meads_update, 1, D, _dev(Q[:1]), _dev(Q[:1]), 0.5, 1.0, st)


@pytest.mark.timeout(120)
def test_run_is_the_hand_driven_loop_and_follows_the_restatement():
    """meads.run for 20 steps against the (init, update) loop around single kernel calls: bit-equal parameters, scale and
    chain state; both within 1e-9 of the restatement's parameters at every step (its margins are checked on the host:
    no accept flag can differ)."""
    from aehmc_amd import meads
    t, q0, seeds = mr.loop_start()
    n = mr.LOOP["steps"]
    rec = []
    mr.warmup(t, q0, seeds, n, record=rec)
    kernel, state = _kernel(_target(t), seeds, q0)
    init, update = meads.adaptation()
    ms, params = init(state)
    assert params[0] == 0.01 and params[2:] == (1.0, 0.5) and (params[1] == 1).all()
    ms, params = update(ms, state.position, state.potential_energy_grad)
    steps = [params]
    for _ in range(n):
        info, _ = kernel(state, *params)
        state = info.state
        ms, params = update(ms, state.position, state.potential_energy_grad)
        steps.append(params)
    for k, ((eps, scale, alpha, delta), want) in enumerate(zip(steps, rec)):
        _rel([eps, alpha, delta], [want.eps, want.alpha, want.delta], 1e-9, ("params", k))
        _rel(_np(scale), want.scale, 1e-9, ("scale", k))
    kernel2, state2 = _kernel(_target(t), seeds, q0)
    end, (eps, scale, alpha, delta), updates, ms2 = meads._run(kernel2, state2, n, 0.5, 1.0, 0.01)
    assert (eps, alpha, delta) == (steps[-1][0], steps[-1][2], steps[-1][3]) and torch.equal(scale, steps[-1][1])
    assert int(ms2.count) == int(ms.count) == n + 1 and int(ms2.skipped) == int(ms.skipped) == 0
    for a, b in zip(end, state):
        assert torch.equal(a, b)
    public = meads.run(_kernel(_target(t), seeds, q0)[0], state2, n)
    assert len(public) == 3 and public[1][0] == eps and torch.equal(public[0].position, end.position)


# ---- statistics ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stat_runs():
    """meads.run with C = 256 for 300 steps on the two golden targets, from seeds the golden file does not hold."""
    from aehmc_amd import meads
    out = {}
    for name in mr.GOLDEN_SIGMA:
        t, q0, _ = mr.golden_start(name, 99)
        kernel, state = _kernel(_target(t), [990000 + c for c in range(mr.GOLDEN["C"])], q0)
        out[name] = (kernel,) + tuple(meads.run(kernel, state, mr.GOLDEN["steps"])[:2])
    return out


@pytest.mark.timeout(120)
@pytest.mark.parametrize("name", list(mr.GOLDEN_SIGMA))
def test_adapted_parameters_lie_within_the_golden_spread(stat_runs, name):
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "meads_ref_runs.json")))[name]
    _, _, (eps, scale, alpha, delta) = stat_runs[name]
    for got, runs, what in ((eps, np.array(gold["eps"]), "eps"), (alpha, np.array(gold["alpha"]), "alpha")):
        mean, sd = runs.mean(), runs.std(ddof=1)
        print(f"{name}: {what} = {got:.4f}, golden {mean:.4f} +- {sd:.4f}")
        assert abs(got - mean) <= 5 * sd, (what, got, mean, sd)
    assert delta == alpha / 2
    worst = np.abs(np.array(gold["log_scale_ratio"])).max(axis=1)
    ratio = np.abs(np.log(_np(scale) / mr.GOLDEN_SIGMA[name])).max()
    print(f"{name}: max |log(scale / sigma)| = {ratio:.4f}, golden max {worst.max():.4f}, sd {worst.std(ddof=1):.4f}")
    assert ratio <= worst.max() + 5 * worst.std(ddof=1)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("name", list(mr.GOLDEN_SIGMA))
def test_sample_after_run_recovers_the_target(stat_runs, name):
    """200 draws per chain after the warm-up: every mean within 5 mcse_chains of 0 and R-hat < 1.05."""
    from aehmc_amd import meads, summary
    kernel, state, (eps, scale, alpha, delta) = stat_runs[name]
    draws, _, acc, _ = meads.sample(kernel, state, eps, scale, alpha, delta, 200)
    s = summary.summarize(draws)
    mean, mcse, rhat, sd = (_np(x) for x in (s.mean, s.mcse_chains, s.rhat, s.sd))
    print(f"{name}: acceptance {float(acc.mean()):.3f}, max |mean| / mcse_chains = {np.abs(mean / mcse).max():.2f}, "
          f"max rhat = {rhat.max():.4f}, sd / sigma = {(sd / mr.GOLDEN_SIGMA[name]).round(3)}")
    assert (np.abs(mean) <= 5 * mcse).all(), (mean / mcse)
    assert (rhat < 1.05).all(), rhat
