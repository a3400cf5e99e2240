"""Non-finite energies in every kernel family, against the oracle (tests/nonfinite_cases.py; the reference side is pinned
on the CPU by tests/test_nonfinite_host.py).

The reference's rules -- a NaN energy difference is -inf, the step diverges, p_accept = 0 (aehmc/hmc.py:189-195,
proposals.py:43-45); a NaN expit is 0 (proposals.py:95-97); the scan behind a first step that diverged still runs and
draws (trajectory.py:336) -- are written once for NUTS (csrc/nuts_tree.cuh) and once per HMC family, and every family
carries the values through its own reductions, LDS rows, MFMA products and slot copies.  Poisoned and healthy chains
share wavefronts, teams and workgroups here:
  1. poison by start position (1e150 scale, overflow, NaN, inf), every row of FAMILIES / RTC_FAMILIES and generalised HMC;
  2. poison in mid-tree: a density with a wall (hand-written, traced, GLM) on the run-time compiled routes;
  3. poison by per-chain step size, and divergence_threshold = inf / 1e308 with step sizes that overflow;
  4. window adaptation with one chain started at scale 1e150.
Discrete outputs and ALL generator words identical to the oracle's, reals at 1e-9 with non-finite entries of the same
class and sign, a chain the oracle leaves in place bit-equal to what went in (the NaN's payload included)."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import nonfinite_cases as nc  # noqa: E402
import rng_plant as rp  # noqa: E402
import test_gpu_rng_planted as planted  # noqa: E402
from oracle import c_oracle as co  # noqa: E402
from test_gpu_rng_planted import FAMILIES, L_HMC, LOCKSTEP, MAX_EXP, OPTION_DEFAULTS, RTC_FAMILIES, dev, eng, words  # noqa: E402,F401

TEAM_ROWS = ("resident-teams-d1", "resident-teams-d3", "resident-teams-d24", "resident-teams-d3-sample")


def chains_of(family):
    return nc.C_TEAMS if family in TEAM_ROWS else nc.C_DEFAULT


def n_sites(sampler):
    return 4 if sampler == "nuts" else 2


# ------------------------------------------------------------------ one device run, reduced to the oracle runners' dicts
def as_dict(info, rng_words, C, D, sampler, n_leapfrog=None):
    def f(t, shape):
        return t.cpu().numpy().reshape(shape)
    d = dict(position=f(info.state.position, (C, D)), potential_energy=f(info.state.potential_energy, (C,)),
             potential_energy_grad=f(info.state.potential_energy_grad, (C, D)), momentum=f(info.state.momentum, (C, D)),
             acceptance_probability=f(info.acceptance_probability, (C,)), is_diverging=f(info.is_diverging, (C,)),
             n_leapfrog=f(info.n_leapfrog, (C,)) if n_leapfrog is None else n_leapfrog,
             words=rng_words.reshape(C, n_sites(sampler), 4)[:, :, :2].copy())
    if sampler == "nuts":
        d.update(num_doublings=f(info.num_doublings, (C,)), is_turning=f(info.is_turning, (C,)))
    return d


def device_run(eng, sampler, mode, options, tgt, imm, q0, rng, eps, T, L=L_HMC, thr=1000.0, first_state=None):
    """T transitions of one route from the generator states ``rng``: (what went in, the transitions as dicts).  ``mode``
    "sample": one launch for all transitions, reported as nonfinite_cases.as_sampled lays an oracle run out."""
    from aehmc_amd import RandomStream, hmc, nuts
    C, D = q0.shape
    mod = nuts if sampler == "nuts" else hmc
    extra = () if sampler == "nuts" else (L,)
    for name, val in options.items():
        eng.set_option(name, val)
    srng = RandomStream.from_state(rng.copy())
    kernel = (nuts.new_kernel(srng, tgt, max_num_expansions=MAX_EXP, divergence_threshold=thr) if sampler == "nuts"
              else hmc.new_kernel(srng, tgt, divergence_threshold=thr))
    if first_state is not None:  # (a hand-written gradient is verified where it is first evaluated: at a finite point)
        mod.new_state(dev(first_state), tgt)
    state = mod.new_state(dev(q0), tgt)
    start = dict(position=state.position.cpu().numpy().reshape(C, D), potential_energy=state.potential_energy.cpu().numpy().reshape(C),
                 potential_energy_grad=state.potential_energy_grad.cpu().numpy().reshape(C, D))
    outs = []
    if mode == "steps":
        for _ in range(T):
            info, updates = kernel(state, eps, imm, *extra)
            outs.append(as_dict(info, words(updates[srng]), C, D, sampler))
            state = info.state._replace(momentum=None)
    else:
        samples, info, acc, div = kernel.sample(state, eps, imm, *extra, T)[:4]
        for t in range(T - 1):
            outs.append(dict(position=samples[t].cpu().numpy().reshape(C, D), acceptance_probability=acc[t].cpu().numpy().reshape(C),
                             is_diverging=div[t].cpu().numpy().reshape(C).astype(bool)))
        holder = kernel._nuts["holder"] if sampler == "nuts" else kernel._hmc["holder"]
        outs.append(as_dict(info, words(holder["rng"]), C, D, sampler))
        np.testing.assert_array_equal(nc.bits(samples[T - 1].cpu().numpy().reshape(C, D)), nc.bits(outs[-1]["position"]))
        np.testing.assert_array_equal(acc[T - 1].cpu().numpy().reshape(C), outs[-1]["acceptance_probability"])
    for name in options:
        eng.set_option(name, OPTION_DEFAULTS[name])
    return start, outs


def assert_against_oracle(start, outs, ref, sampler, mode, what):
    """the assertions of section 1 of the issue: parity with the oracle, and bit-equality of what the oracle left in place"""
    want = ref if mode == "steps" else nc.as_sampled(ref)
    nc.assert_same_run(outs, want, sampler, what)
    q_in, before = start["position"], start
    still = np.ones(q_in.shape[0], dtype=bool)
    for t, r in enumerate(ref):
        still &= nc.stayed(q_in, r["position"])  # (the oracle's own positions, from the same start)
        assert (nc.bits(outs[t]["position"])[still] == nc.bits(q_in)[still]).all(), (what, t, "a chain left in place moved")
        if "potential_energy" in outs[t]:
            for k in ("potential_energy", "potential_energy_grad"):
                assert (nc.bits(outs[t][k])[still] == nc.bits(before[k])[still]).all(), (what, t, k, "not what went in")


# ------------------------------------------------------------------ 1. poison by start position
@pytest.mark.parametrize("family", list(FAMILIES))
def test_kernel_family_with_poisoned_starts(eng, family):
    """Every kernel family, two transitions, chains c % 3 == 1 started at a poison (all five in one call) beside healthy
    N(0, 1) starts, against the C oracle on the same generator states (chain by chain where every chain has its own
    matrix).  A family that masks a reduction with 0 * x, lets a NaN row of a 16-chain product reach another row, drops the
    isnan rule of its accept step or draws another number of words behind a diverged first step fails here."""
    from aehmc_amd import PerChain
    sampler, D, mk, options, mode, _ = FAMILIES[family]
    T, C = 2, chains_of(family)
    r = np.random.default_rng(2000 + D)
    rng = co.site_states(list(range(100 + D, 100 + D + C)), n_sites(sampler))
    if mk == "linreg":
        tgt, otgt, imm, N = planted.linreg(r)
        eps = 0.3
        q0 = np.array([3.0, np.log(0.5)]) + (0.5 / np.sqrt(N)) * r.normal(size=(C, 2))
        q0, labels = nc.poison_starts(q0, nc.LINREG_POISONS, r)
    else:
        tgt, otgt, imm = planted.gaussian(D, r, dense_metric=mk == "dense", per_chain=C if mk == "per_chain" else 0)
        eps = 0.25 / D ** 0.25 if D <= 512 else 0.05 / D ** 0.25
        q0, labels = nc.poison_starts(r.normal(size=(C, D)), nc.GAUSS_POISONS, r)
        nc.assert_scale_is_order_safe(q0)
    imm_dev = PerChain(dev(imm)) if mk == "per_chain" else imm
    ref = nc.c_run(sampler, otgt, imm, rng, q0, eps, T, L=L_HMC, max_exp=MAX_EXP, per_chain_imm=mk == "per_chain")
    start, outs = device_run(eng, sampler, mode, options, tgt, imm_dev, q0, rng, eps, T)
    assert_against_oracle(start, outs, ref, sampler, mode, (family, labels))
    bad = nc.is_poisoned(C)
    assert all(r["is_diverging"][bad].all() for r in ref) and not any(r["is_diverging"][~bad].any() for r in ref)


def coupled_gaussian_target(D):
    """planted.coupled_gaussian with its gradient by hand, for np_oracle"""
    sd = 0.5 + np.arange(D) % 3
    fn = planted.coupled_gaussian(D)

    def grad(q):
        z = (q - 1.0) / sd
        g = -z
        g[1:] -= 0.05 * z[:-1]
        g[:-1] -= 0.05 * z[1:]
        return g / sd
    return fn, nc.CallableTarget(fn, grad)


def rtc_case(kind, D, r):
    from aehmc_amd import targets
    if kind.startswith("glm"):
        import test_gpu_custom_target as tct
        N = 900 if kind == "glm" else 300
        X, y, _ = tct.logistic_data(N, D, 77)
        return targets.CustomGLM(tct.LOGISTIC, X, y, params=[[2.0]]), 0.02 + 0.05 * r.random(D), 0.4, 0.3, 0.0, 0.3
    return targets.from_callable(planted.coupled_gaussian(D), D), 0.5 + r.random(D), 0.25 / D ** 0.25, 0.25 / D ** 0.25, 1.0, 1.0


@pytest.mark.parametrize("family", list(RTC_FAMILIES))
def test_runtime_compiled_family_with_poisoned_starts(eng, family):
    """The run-time compiled routes on their own targets with the same poisons, against the lock-step route of the same
    target on the same generator states (test_joint_lockstep_with_poisoned_starts_equals_np_oracle pins that one)."""
    kind, D, options = RTC_FAMILIES[family]
    T, C = 2, nc.C_DEFAULT
    r = np.random.default_rng(D + len(family))
    tgt, imm, eps_n, eps_h, centre, scale = rtc_case(kind, D, r)
    healthy = centre + scale * r.normal(size=(C, D))
    q0, labels = nc.poison_starts(healthy, nc.GAUSS_POISONS, r)
    for sampler, eps in (("nuts", eps_n), ("hmc", eps_h)):
        rng = co.site_states(list(range(300 + D, 300 + D + C)), n_sites(sampler))
        start, fast = device_run(eng, sampler, "sample", options, tgt, imm, q0, rng, eps, T, first_state=healthy)
        start_l, lock = device_run(eng, sampler, "sample", LOCKSTEP, tgt, imm, q0, rng, eps, T)
        for name in LOCKSTEP:
            eng.set_option(name, OPTION_DEFAULTS[name])
        nc.assert_same_run(fast, lock, sampler, (family, sampler, labels))
        bad = nc.is_poisoned(C)
        assert all(o["is_diverging"][bad].all() for o in lock) and not lock[-1]["is_diverging"][~bad].all()
        never_moved = bad & (np.array(labels) != "scale")  # (a non-finite H0: every delta is NaN -> -inf, hmc.py:190)
        for k in ("position", "potential_energy", "potential_energy_grad"):
            assert (nc.bits(fast[-1][k])[never_moved] == nc.bits(start[k])[never_moved]).all(), (family, sampler, k)


@pytest.mark.parametrize("sampler", ["nuts", "hmc"])
def test_joint_lockstep_with_poisoned_starts_equals_np_oracle(eng, sampler):
    """the reference of the test above: the lock-step route of the traced joint target against np_oracle on the Python
    function itself"""
    from aehmc_amd import targets
    D, T, C = 70, 2, nc.C_DEFAULT
    r = np.random.default_rng(D)
    fn, otgt = coupled_gaussian_target(D)
    imm, eps = 0.5 + r.random(D), 0.25 / D ** 0.25
    healthy = 1.0 + r.normal(size=(C, D))
    q0, labels = nc.poison_starts(healthy, nc.GAUSS_POISONS, r)
    rng = co.site_states(list(range(800, 800 + C)), n_sites(sampler))
    ref = nc.np_run(sampler, otgt, rng, q0, eps, imm, T, L=L_HMC, max_exp=MAX_EXP)
    start, outs = device_run(eng, sampler, "steps", LOCKSTEP, targets.from_callable(fn, D), imm, q0, rng, eps, T)
    for name in LOCKSTEP:
        eng.set_option(name, OPTION_DEFAULTS[name])
    assert_against_oracle(start, outs, ref, sampler, "steps", (sampler, labels))


@pytest.mark.parametrize("D", [7, 257])
def test_ghmc_with_poisoned_starts(eng, D):
    """Generalised HMC (ghmc_fused.cuh:192 holds its own copy of the isnan rule) against tests/meads_ref.py's transition,
    which restates hmc.py:190 (tests/test_nonfinite_host.py checks that it does)."""
    import aehmc_amd as aa
    import meads_ref as mr
    T, P, C = 2, mr.PARITY, nc.C_DEFAULT
    r = np.random.default_rng(D)
    t = mr.DiagGaussian(r.normal(size=D), 0.5 + r.random(D))
    q0, labels = nc.poison_starts(r.normal(size=(C, D)), nc.GAUSS_POISONS, r)
    s = mr.parity_scale(D)
    rng = co.site_states(list(range(60 + D, 60 + D + C)), 2)
    gens = [[rp.numpy_generator(rp.unpack_state(rng[c, k]), (int(rng[c, k, 2]) << 64) | int(rng[c, k, 3])) for c in range(C)]
            for k in range(2)]
    tgt = aa.targets.DiagGaussian(t.mu, t.sigma)
    kernel = aa.ghmc.new_kernel(aa.RandomStream.from_state(rng.copy()), tgt)
    state = aa.ghmc.new_state(dev(q0), tgt)
    with np.errstate(all="ignore"):
        ch = mr.start(t, q0)
    bad = nc.is_poisoned(C)
    for k in range(T):
        info, updates = kernel(state, P["eps"], dev(s), P["alpha"], P["delta"])
        state = info.state
        with np.errstate(all="ignore"):
            ch, ref = mr.transition(ch, gens[0], gens[1], t, P["eps"], P["alpha"], P["delta"], s)
        assert ref.margin[~bad].min() > 1e-9
        assert np.array_equal(info.is_turning.cpu().numpy(), ref.accepted), k
        assert np.array_equal(info.is_diverging.cpu().numpy(), ref.is_diverging), k
        assert ref.is_diverging[bad].all() and not ref.is_diverging[~bad].any()
        for name, got, want in (("q", state.position, ch.q), ("g", state.potential_energy_grad, ch.g), ("v", state.momentum, ch.v),
                                ("U", state.potential_energy, ch.U), ("p", info.acceptance_probability, ref.acceptance_probability)):
            nc.assert_reals(got.cpu().numpy(), want, atol=1e-12, what=(D, k, name))
        rejected = bad & ~ref.accepted
        assert (nc.bits(state.position.cpu().numpy())[rejected] == nc.bits(q0)[rejected]).all()
    (after,) = updates.values()
    assert np.array_equal(words(after).reshape(C, 2, 4), mr.site_states(gens[0], gens[1]))


# ------------------------------------------------------------------ 3. poison by parameter; the threshold that never fires
# name: (sampler, D, metric, engine options, "steps" | "sample"): the routes that take one step size per chain -- those of
# test_per_chain_parameters_equal_single_chain_runs (per-chain diagonal metrics beside them, as there), the rolling block
# kernel's per_chain_eps case and the per-chain dense kernels
PER_CHAIN_EPS = {
    "fused-hmc": ("hmc", 70, "per_chain_diag", {}, "steps"),
    "wide-hmc": ("hmc", 1500, "per_chain_diag", {}, "steps"),
    "resident-nuts": ("nuts", 70, "per_chain_diag", {}, "steps"),
    "wide-nuts": ("nuts", 600, "per_chain_diag", {}, "steps"),
    "linreg-nuts": ("nuts", 2, "linreg", {}, "steps"),
    "block-dense-roll-nuts-sample": ("nuts", 72, "dense", {"block_dense": 1, "block_roll": 1}, "sample"),
    "per-chain-dense-nuts": ("nuts", 65, "per_chain", {}, "steps"),
    "per-chain-dense-hmc-sample": ("hmc", 65, "per_chain", {}, "sample"),
}


@pytest.mark.parametrize("route", list(PER_CHAIN_EPS))
def test_per_chain_step_sizes_that_overflow(eng, route):
    """PerChain step sizes 1e154, 1e200, 1e308, inf and nan on the chains c % 3 == 1, the others at the route's ordinary
    step size; every chain against the C oracle run alone with its own step size."""
    from aehmc_amd import PerChain
    sampler, D, mk, options, mode = PER_CHAIN_EPS[route]
    T, C = 2, nc.C_DEFAULT
    r = np.random.default_rng(3000 + D)
    rng = co.site_states(list(range(400 + D, 400 + D + C)), n_sites(sampler))
    if mk == "linreg":
        tgt, otgt, imm1, N = planted.linreg(r)
        imm = imm1 * (0.5 + r.random((C, 2)))
        base = 0.3
        q0 = np.array([3.0, np.log(0.5)]) + (0.5 / np.sqrt(N)) * r.normal(size=(C, 2))
    else:
        tgt, otgt, imm = planted.gaussian(D, r, dense_metric=mk == "dense", per_chain=C if mk == "per_chain" else 0)
        if mk == "per_chain_diag":
            imm = 0.5 + r.random((C, D))
        base = 0.25 / D ** 0.25 if D <= 512 else 0.05 / D ** 0.25
        q0 = r.normal(size=(C, D))
    per_chain = mk != "dense"
    eps = nc.poison_step_sizes(C, base)
    ref = nc.c_run(sampler, otgt, imm, rng, q0, eps, T, L=L_HMC, max_exp=MAX_EXP, per_chain_imm=per_chain)
    start, outs = device_run(eng, sampler, mode, options, tgt, PerChain(dev(imm)) if per_chain else imm, q0, rng,
                             PerChain(dev(eps)), T)
    assert_against_oracle(start, outs, ref, sampler, mode, route)
    bad = nc.is_poisoned(C)
    assert all(r["is_diverging"][bad].all() for r in ref) and not any(r["is_diverging"][~bad].any() for r in ref)


# one row per scalar-code variant of nuts_tree.cuh: LANES (a wavefront per chain, the wide kernel, the lock-step engine) and
# the scalar form (sub-wavefront teams)
NEVER_FIRES_ROWS = ("resident-wavefront-step", "wide-nuts", "lockstep-diag-nuts", "resident-teams-d3")


@pytest.mark.parametrize("thr,eps", nc.NEVER_FIRES)
@pytest.mark.parametrize("family", NEVER_FIRES_ROWS)
def test_divergence_threshold_that_never_fires(eng, family, thr, eps):
    """divergence_threshold = inf (and 1e308) with a step size that overflows the energies: nothing diverges, and infinite
    weights pass through nuts_step_scalars, nuts_expansion_scalars and the biased draw."""
    sampler, D, mk, options, mode, _ = FAMILIES[family]
    T, C = 2, chains_of(family)
    r = np.random.default_rng(4000 + D)
    rng = co.site_states(list(range(500 + D, 500 + D + C)), 4)
    tgt, otgt, imm = planted.gaussian(D, r)
    q0 = r.normal(size=(C, D))
    ref = nc.c_run("nuts", otgt, imm, rng, q0, eps, T, max_exp=MAX_EXP, thr=thr)
    start, outs = device_run(eng, "nuts", mode, options, tgt, imm, q0, rng, eps, T, thr=thr)
    nc.assert_same_run(outs, ref if mode == "steps" else nc.as_sampled(ref), "nuts", (family, thr, eps))
    if np.isinf(thr):
        assert not any(r["is_diverging"].any() for r in ref)


# ------------------------------------------------------------------ 2. non-finite values in mid-tree: the wall
WALL_ELEMENTWISE = ("resident-teams-d3", "resident-teams-d24", "resident-teams-d3-sample", "resident-wavefront-step",
                    "resident-wavefront-sample", "fused-hmc-sample", "wide-nuts", "wide-hmc-sample", "block-dense-reg-nuts",
                    "block-dense-rows-nuts", "block-dense-reg-hmc", "block-dense-rows-hmc", "block-dense-roll-nuts-sample",
                    "lockstep-diag-nuts", "lockstep-diag-hmc", "lockstep-dense-nuts", "lockstep-dense-hmc")
WALL_T = 2


@functools.lru_cache(maxsize=None)
def wall_reference(form, size, sampler, poison):
    """np_oracle on the wall density as a callable (computed once per input: the rows of a shape share it), with the
    condition of the case asserted on the oracle's outputs alone"""
    p = nc.WALL_POISONS[poison]
    if form == "elementwise":
        C, seeds, q0, w = nc.wall_inputs(size, sampler)
        otgt, imm, eps, L = nc.Wall(w, p), nc.wall_metric(size), nc.wall_eps(size), nc.wall_length(size)
    elif form == "joint":
        C, seeds, q0, w = nc.wall_inputs(size, sampler, joint=True)
        otgt, imm, eps, L = nc.wall_joint_target(w, p), np.ones(size), nc.wall_eps(size), nc.wall_length(size)
    else:
        X, y, C, seeds, q0, imm, eps, w = nc.wall_glm_inputs(size, sampler=sampler)
        otgt, L = nc.WallGLM(X, y, w, p), nc.GLM_L
    rng = co.site_states(seeds, n_sites(sampler))
    ref = nc.np_run(sampler, otgt, rng, q0, eps, imm, WALL_T, L=L, max_exp=MAX_EXP)
    if sampler == "nuts":
        nc.assert_wall_condition(ref, C, (form, size, poison))
    else:  # (no tree: at least four diverging transitions, a third of the chains untouched)
        div = np.stack([o["is_diverging"] for o in ref])
        assert div.sum() >= 4 and 3 * (~div).all(axis=0).sum() >= C, (form, size, poison)
        if poison == "minus_inf":
            # hmc.py:189-195: delta = H0 - (-inf) = +inf is no NaN, so the reference ACCEPTS with probability 1 and flags a
            # divergence; the chain then sits at H0 = -inf, every later delta is NaN -> -inf and diverges.  Parity is the
            # contract: this is the oracle's behaviour, and the device's is compared with it below.
            with np.errstate(all="ignore"):
                hit = div[0] & np.isfinite([otgt(q)[0] for q in q0])  # (a GLM chain may START beyond the wall)
            assert hit.any() or form == "glm"  # (the short GLM trajectories end beyond the wall only where they began there)
            assert (ref[0]["acceptance_probability"][hit] == 1).all() and div[1][hit].all()
            assert np.isneginf(ref[0]["potential_energy"][hit]).all()
    return ref, rng, q0, w, imm, eps, L


def wall_params(w, poison):
    return [np.array([float(w)]), np.array([float(nc.WALL_POISONS[poison])])]


@pytest.mark.parametrize("poison", list(nc.WALL_POISONS))
@pytest.mark.parametrize("family", WALL_ELEMENTWISE)
def test_wall_in_mid_tree_on_elementwise_routes(eng, family, poison):
    """A hand-written Custom density whose potential is the poison beyond q_i >= w (w and the poison are parameters: one
    compilation per kernel family), at the shapes of FAMILIES: trajectories cross the wall in mid-tree, so the non-finite
    energy meets running sums, checkpoints and the U-turn products, not only the first step."""
    from aehmc_amd import targets
    sampler, D, mk, options, mode, _ = FAMILIES[family]
    ref, rng, q0, w, imm, eps, L = wall_reference("elementwise", D, sampler, poison)
    assert (mk == "dense") == (np.ndim(imm) == 2)
    tgt = targets.Custom(nc.WALL_SOURCE, params=wall_params(w, poison))
    start, outs = device_run(eng, sampler, mode, options, tgt, dev(imm) if mk == "dense" else imm, q0, rng, eps, WALL_T, L=L,
                             first_state=np.zeros_like(q0))
    assert_against_oracle(start, outs, ref, sampler, mode, (family, poison))


@pytest.mark.parametrize("poison", list(nc.WALL_POISONS))
@pytest.mark.parametrize("family", [f for f in RTC_FAMILIES if f.startswith("joint")])
def test_wall_in_mid_tree_on_traced_joint_routes(eng, family, poison):
    """The same wall traced from Python with tracing.where behind a weakly coupled (joint) density, through
    from_callable(..., reverse=True), on the joint routes (tests/test_nonfinite_host.py checks the emitted source on both
    sides of the wall: the poison is read from the parameter array, not folded away)."""
    from aehmc_amd import targets
    _, D, options = RTC_FAMILIES[family]
    for sampler in ("nuts", "hmc"):
        ref, rng, q0, w, imm, eps, L = wall_reference("joint", D, sampler, poison)
        tgt = targets.from_callable(nc.wall_joint_logp, D, args=tuple(wall_params(w, poison)), reverse=True)
        assert not isinstance(tgt, targets.Custom)
        start, outs = device_run(eng, sampler, "sample", options, tgt, imm, q0, rng, eps, WALL_T, L=L)
        assert_against_oracle(start, outs, ref, sampler, "sample", (family, sampler, poison))


@pytest.mark.parametrize("poison", list(nc.WALL_POISONS))
@pytest.mark.parametrize("family", [f for f in RTC_FAMILIES if f.startswith("glm")])
def test_wall_in_mid_tree_on_glm_routes(eng, family, poison):
    """A CustomGLM whose row loss is the poison beyond z > w, on both GLM routes."""
    from aehmc_amd import targets
    kind, D, options = RTC_FAMILIES[family]
    N = 900 if kind == "glm" else 300
    for sampler in ("nuts", "hmc"):
        ref, rng, q0, w, imm, eps, L = wall_reference("glm", N, sampler, poison)
        X, y = nc.wall_glm_inputs(N, sampler=sampler)[:2]
        tgt = targets.CustomGLM(nc.WALL_GLM_SOURCE, X, y, params=[[nc.GLM_TAU]] + wall_params(w, poison))
        start, outs = device_run(eng, sampler, "sample", options, tgt, imm, q0, rng, eps, WALL_T, L=L,
                                 first_state=np.zeros_like(q0))
        assert_against_oracle(start, outs, ref, sampler, "sample", (family, sampler, poison))


# ------------------------------------------------------------------ 4. warm-up with a poisoned chain
class OracleNuts:
    """kernel(state, step_size, imm) of one chain on the C oracle, for oracle/np_adaptation.run; keeps the last outputs"""

    def __init__(self, otgt, rng_c, D):
        self.otgt, self.D, self.rng, self.last = otgt, D, rng_c[None].copy(), None

    def __call__(self, state, eps, imm):
        from types import SimpleNamespace
        from oracle import np_oracle as no
        q = np.array(state.position, dtype=np.float64).reshape(1, self.D).copy()
        U = np.array([state.potential_energy], dtype=np.float64)
        g = np.array(state.potential_energy_grad, dtype=np.float64).reshape(1, self.D).copy()
        self.last = co.nuts_step(self.otgt, co.Metric(imm, self.D), self.rng, float(eps), q, U, g)
        return SimpleNamespace(state=no.IntegratorState(q[0].copy(), None, float(U[0]), g[0].copy()),
                               acceptance_probability=float(self.last["acceptance_probability"][0]))


def warmup_case(full, D, C, far_out=True):
    from aehmc_amd import targets
    r = np.random.default_rng(D + C)
    mu, sigma = r.normal(size=D), 0.5 + r.random(D)
    q0 = mu + sigma * r.normal(size=(C, D))
    far = mu + sigma * nc.scale_for(D) * r.normal(size=D)
    if far_out:
        q0[1] = far
    nc.assert_scale_is_order_safe(q0)
    return (targets.DiagGaussian(mu, sigma), co.Target(co.T_DIAG_GAUSSIAN, D, mu=mu, sigma=sigma), q0,
            co.site_states([300 + c for c in range(C)], 4))


def warmup_on_device(tgt, q0, rng, steps, full, fused):
    """(position, step sizes, metric, L^-T or sqrt of the mass, generator states) after the warm-up, then position, n_leapfrog,
    num_doublings, is_diverging, is_turning and generator states of the following transition"""
    from aehmc_amd import RandomStream, nuts, window_adaptation
    srng = RandomStream.from_state(rng.copy())
    kernel = nuts.new_kernel(srng, tgt)
    state = nuts.new_state(dev(q0), tgt)
    state, (eps, imm), upd = window_adaptation.run(kernel, state, steps, is_mass_matrix_full=full, initial_step_size=1.0, fused=fused)
    after = upd[srng].clone()
    info, upd = kernel(state, eps, imm)
    return (state.position.clone(), eps.value.clone(), imm.value.clone(), imm.sqrt_mass.clone(), after, info.state.position.clone(),
            info.n_leapfrog.clone(), info.num_doublings.clone(), info.is_diverging.clone(), info.is_turning.clone(), upd[srng].clone())


def warmup_oracle_mismatches(out, otgt, q0, rng, steps, full):
    """what of a device warm-up is not oracle/np_adaptation.py's, driven by the C oracle chain by chain: [(chain, what)]"""
    from oracle import np_adaptation as na
    from oracle import np_oracle as no
    C, D = q0.shape
    bad = []
    for c in range(C):
        ok = OracleNuts(otgt, rng[c], D)
        qc, Uc, gc = co.new_state(otgt, q0[c:c + 1].copy())
        st, (eps_o, imm_o) = na.run(ok, no.IntegratorState(qc[0], None, float(Uc[0]), gc[0]), steps, is_mass_matrix_full=full,
                                    initial_step_size=1.0)
        if not np.array_equal(words(out[4]).reshape(C, 4, 4)[c, :, :2], ok.rng[0, :, :2]):
            bad.append((c, "generator states after the warm-up"))
        ok(st, eps_o, imm_o)
        for k, name in ((6, "n_leapfrog"), (7, "num_doublings"), (8, "is_diverging"), (9, "is_turning")):
            if int(out[k].reshape(-1)[c].item()) != int(ok.last[name][0]):
                bad.append((c, name))
        if not np.array_equal(words(out[10]).reshape(C, 4, 4)[c, :, :2], ok.rng[0, :, :2]):
            bad.append((c, "generator states after the following transition"))
    return bad


ORACLE_HORIZON = 60


@pytest.mark.parametrize("full,D,C", [(False, 30, 7), (True, 6, 5)])
def test_warmup_with_one_chain_started_far_out(full, D, C):
    """window_adaptation.run (per-chain adaptation, the shapes and the 130 steps of test_fused_warmup_equals_step_by_step)
    with chain 1 started at scale 1e150: the one-launch call is bitwise the step-by-step loop.  Over the suite's horizon
    for a warm-up against the oracle -- 60 steps: the loop feeds the step size back into the trajectory, which amplifies
    last-bit differences by about 1.2 per step (test_window_adaptation_matches_oracle) -- the generator states after the
    warm-up and the discrete outputs and generator states of the following transition are those of
    oracle/np_adaptation.py driven by the C oracle: the far-out chain's acceptances of 0 shrink ITS step size and leave
    its neighbours' adaptation alone."""
    tgt, otgt, q0, rng = warmup_case(full, D, C)
    outs = [warmup_on_device(tgt, q0, rng, 130, full, fused) for fused in (True, False)]
    for k, (a, b) in enumerate(zip(*outs)):
        assert torch.equal(a, b) or (torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(), b.nan_to_num())), k
    short = warmup_on_device(tgt, q0, rng, ORACLE_HORIZON, full, True)
    assert warmup_oracle_mismatches(short, otgt, q0, rng, ORACLE_HORIZON, full) == []
