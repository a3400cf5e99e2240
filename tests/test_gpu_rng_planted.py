"""The device RNG's rare paths, reached by construction instead of by volume (tests/rng_plant.py).

PCG64's step is invertible, so a generator state can be built whose k-th raw output is any chosen word: a ziggurat tail
draw in lane 63 of `wave_normals`, a wedge test in lane 62, a uniform 16 ulps from the boundary of `binomial(1, p)`.
  a. `rng_normals` on ~270 planted streams x every request size of the table: values and stream position against numpy
     (tests/test_rng_planted_host.py proves that this table takes every branch of `wave_normals` at least 20 times);
  b. `rng_bernoulli` with the first uniform inside the guard bands of `binomial1_inversion`, where its literal
     arithmetic decides;
  c. every kernel family that draws its momentum itself -- each inlines its own copy of `wave_normals` or of
     `rng_standard_normal` -- with tail and wedge words planted in the momentum site, against the C oracle on the same
     states (run-time compiled families: against the lock-step route, which the first cases pin to the oracle).
Reference: numpy.random.Generator (PCG64, ziggurat normal, binomial(1, p)), which the reference's RandomStream
call sites execute (aehmc/metrics.py:66, trajectory.py:516, proposals.py:99,131, hmc.py:194)."""
import random

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import rng_plant as rp  # noqa: E402
import wave_normals_ref as wr  # noqa: E402
from oracle import c_oracle as co  # noqa: E402

RTOL = 1e-9
OPTION_DEFAULTS = {"resident_nuts": 2, "fused_hmc": 1, "fused_nuts": 0, "resident_min_team": 0, "block_dense": 1,
                   "block_roll": 0, "pc_dense": 1, "joint_wg": 1, "joint_resident": 1, "joint_wide": 1}


@pytest.fixture()
def eng():
    from aehmc_amd.engine import get_engine
    e = get_engine()
    try:
        yield e
    finally:
        for name, val in OPTION_DEFAULTS.items():
            e.set_option(name, val)


def dev(x, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda").to(dtype)


def words(t):
    return t.cpu().numpy().view(np.uint64)


# ------------------------------------------------------------------ a. rng_normals
def test_rng_normals_on_planted_streams(eng):
    """Every planted stream is a chain of one call; for every request size a fresh copy of the states draws n normals and
    then 64 more.  Bit-equal to numpy except where the model says the value came from the tail formula (`log1p`: 4e-16,
    the rule of test_device_rng_matches_numpy), and the generator state after each call is numpy's, both words."""
    from aehmc_amd.engine import rng_to_device
    cases = rp.normal_cases()
    C = len(cases)
    assert C == 2 * len(rp.NORMAL_POSITIONS) * rp.NORMAL_REPLICATES
    st = rp.pack_sites([[(s, inc)] for _, _, s, inc in cases])[:, 0]
    streams = [wr.Stream(rp.numpy_generator(s, inc).bit_generator.random_raw(1024)) for _, _, s, inc in cases]
    for n in rp.NORMAL_SIZES:
        rng = rng_to_device(st.copy(), "cuda")
        got, after = [], []
        for m in (n, 64):
            got.append(eng.rng_normals(rng, m).cpu().numpy())
            after.append(words(rng).copy())
        for c, (kind, k, s, inc) in enumerate(cases):
            g = rp.numpy_generator(s, inc)
            pos = 0
            for call, m in enumerate((n, 64)):
                ref = g.normal(size=m)
                _, pos, _, tails = wr.wave_normals(streams[c], m, pos)
                exact = np.ones(m, dtype=bool)
                exact[sorted(tails)] = False
                z = got[call][c]
                where = (kind, k, n, call)
                assert np.array_equal(z[exact], ref[exact]), where
                np.testing.assert_allclose(z[~exact], ref[~exact], rtol=4e-16, atol=0, err_msg=str(where))
                state = rp.generator_state(g)
                assert (int(after[call][c][0]), int(after[call][c][1])) == (state >> 64, state & rp.M64), where


# ------------------------------------------------------------------ b. rng_bernoulli
def test_rng_bernoulli_in_the_guard_bands(eng):
    """q = m 2^-53 in [0.5, 1) so that p = 1 - q and 1 - p are exact; the first uniform planted at q + j 2^-53 and at
    1 - j 2^-53 inside the 1e-12 bands (the literal branch of `binomial1_inversion`, probability 1e-12 per draw) and just
    outside them, for p (direct) and p' = q (the 1 - binomial(1 - p') route).  Every planted U is at least 16 ulps from
    the boundary: numpy's outcome is then the exact-arithmetic one after a single uniform (checked on the host), so an
    exp(log(q)) that differs by an ulp or two between the device and libm cannot change the expected result."""
    from aehmc_amd.engine import rng_to_device
    cases = rp.bernoulli_cases()
    assert len(cases) == 300 * 12 * 2
    st = rp.pack_sites([[(s, inc)] for _, s, inc, _, _ in cases])[:, 0]
    rng = rng_to_device(st.copy(), "cuda")
    p = np.array([[c[0]] for c in cases])
    b = eng.rng_bernoulli(rng, dev(p)).cpu().numpy()
    after = words(rng)
    for c, (pc, s, inc, u, m) in enumerate(cases):
        g = rp.numpy_generator(s, inc)
        assert int(b[c, 0]) == int(g.binomial(1, pc)), (pc, u, m)
        state = rp.generator_state(g)
        assert (int(after[c][0]), int(after[c][1])) == (state >> 64, state & rp.M64), (pc, u, m)


# ------------------------------------------------------------------ c. kernel families
def plant_positions(D, T):
    """stream positions of the momentum site that get a planted word: around the 64-lane round and the end of the first
    draw, and (calls of several transitions) at the start and around the round of the second one; small D: all of them"""
    want = {0, 1, 31, 61, 62, 63, 64, 65, D - 3, D - 2, D - 1}
    if T > 1:
        want |= {D, D + 1, D + 62, D + 63}
    if D <= 3:
        want |= set(range(T * D))
    return sorted(k for k in want if 0 <= k < T * D)


def planted_sites(D, T, n_sites, seed):
    """uint64 [C, n_sites, 4]: one plant per chain in site 0 (2 kinds x positions x 2 replicates), random other sites"""
    rnd = random.Random(seed)
    chains = []
    for make in (rp.tail_raw, rp.wedge_raw):
        for k in plant_positions(D, T):
            for _ in range(2):
                inc = rp.random_inc(rnd)
                sites = [(rp.plant(make(rnd), k, inc, rnd), inc)]
                sites += [(rnd.getrandbits(128), rp.random_inc(rnd)) for _ in range(n_sites - 1)]
                chains.append(sites)
    return rp.pack_sites(chains)


def gaussian(D, r, dense_metric=False, per_chain=0):
    from aehmc_amd import targets
    mu, sigma = r.normal(size=D), 0.5 + r.random(D)
    tgt, otgt = targets.DiagGaussian(mu, sigma), co.Target(co.T_DIAG_GAUSSIAN, D, mu=mu, sigma=sigma)
    if per_chain:
        A = r.normal(size=(per_chain, D, D))
        imm = A @ A.transpose(0, 2, 1) / D + 0.5 * np.eye(D)
        imm = 0.5 * (imm + imm.transpose(0, 2, 1))
    elif dense_metric:
        A = r.normal(size=(D, D))
        imm = A @ A.T / D + np.eye(D)
        imm = 0.5 * (imm + imm.T)
    else:
        imm = 0.5 + r.random(D)
    return tgt, otgt, imm


def linreg(r, N=700):
    from aehmc_amd import targets
    X = r.normal(size=N)
    y = 3 * X + 0.5 * r.normal(size=N)
    return targets.LinearRegression(X, y), co.Target(co.T_LINREG, 2, X=X, y=y), np.array([1.0 / N, 0.5 / N]), N


# name: (sampler, D, metric, engine options, "steps" | "sample", transitions).  The options select the family as
# include/aehmc_hip.h documents them (`fused_nuts` is looked at on the lock-step route only, hence `resident_nuts` = 0
# beside it); D picks the instantiation: sub-wavefront teams with several chains per wavefront (D = 1, 3, 24), a
# wavefront per chain (130), a workgroup per chain behind k_draw_momentum (700; HMC 1500), k_hmc_fused (40), the small
# dense kernels (<= 64), the block kernels (64 < D <= 512, shared dense metric), per-chain dense matrices (65).
FAMILIES = {
    "lockstep-diag-nuts": ("nuts", 70, "diag", {"resident_nuts": 0}, "steps", 2),
    "lockstep-diag-hmc": ("hmc", 70, "diag", {"fused_hmc": 0}, "steps", 2),
    "lockstep-dense-nuts": ("nuts", 72, "dense", {"block_dense": 0}, "steps", 2),
    "lockstep-dense-hmc": ("hmc", 72, "dense", {"block_dense": 0}, "steps", 2),
    "fused-nuts-wavefront": ("nuts", 70, "diag", {"resident_nuts": 0, "fused_nuts": 1}, "steps", 2),
    "resident-teams-d1": ("nuts", 1, "diag", {"resident_min_team": 1}, "steps", 3),
    "resident-teams-d3": ("nuts", 3, "diag", {"resident_min_team": 1}, "steps", 3),
    "resident-teams-d24": ("nuts", 24, "diag", {"resident_min_team": 1}, "steps", 3),
    "resident-teams-d3-sample": ("nuts", 3, "diag", {"resident_min_team": 1}, "sample", 3),
    "resident-wavefront-step": ("nuts", 130, "diag", {}, "steps", 2),
    "resident-wavefront-sample": ("nuts", 130, "diag", {}, "sample", 2),
    "wide-nuts": ("nuts", 700, "diag", {}, "steps", 2),
    "fused-hmc-sample": ("hmc", 40, "diag", {}, "sample", 3),
    "wide-hmc-sample": ("hmc", 1500, "diag", {}, "sample", 3),
    "small-dense-nuts-d7": ("nuts", 7, "dense", {}, "steps", 2),
    "small-dense-nuts-d64": ("nuts", 64, "dense", {}, "steps", 2),
    "small-dense-hmc-d7": ("hmc", 7, "dense", {}, "steps", 2),
    "small-dense-hmc-d64": ("hmc", 64, "dense", {}, "steps", 2),
    "block-dense-reg-nuts": ("nuts", 72, "dense", {"block_dense": 1}, "steps", 2),
    "block-dense-rows-nuts": ("nuts", 72, "dense", {"block_dense": 2}, "steps", 2),
    "block-dense-reg-hmc": ("hmc", 72, "dense", {"block_dense": 1}, "steps", 2),
    "block-dense-rows-hmc": ("hmc", 72, "dense", {"block_dense": 2}, "steps", 2),
    "block-dense-roll-nuts-sample": ("nuts", 72, "dense", {"block_dense": 1, "block_roll": 1}, "sample", 3),
    "per-chain-dense-nuts": ("nuts", 65, "per_chain", {}, "steps", 2),
    "per-chain-dense-hmc-sample": ("hmc", 65, "per_chain", {}, "sample", 2),
    "linreg-nuts": ("nuts", 2, "linreg", {}, "steps", 3),
    "linreg-nuts-sample": ("nuts", 2, "linreg", {}, "sample", 3),
    "linreg-hmc-sample": ("hmc", 2, "linreg", {}, "sample", 3),
}
L_HMC, MAX_EXP = 7, 6


@pytest.mark.parametrize("family", list(FAMILIES))
def test_kernel_family_with_planted_momentum_states(eng, family):
    """One transition or a few of one kernel family with tail and wedge words planted in the momentum site, the same
    [C, n_sites, 4] states on the device (RandomStream.from_state) and in the C oracle: positions, energies, gradients,
    momenta at 1e-9, every discrete output identical, ALL generator states identical afterwards (the assertions of
    tests/test_gpu_parity.py).  A call site that loses a state word in the redraw loop, calls `wave_normals` under a
    partial EXEC mask or hands the stream on at the wrong position changes the momentum or the state."""
    from aehmc_amd import PerChain, RandomStream, hmc, nuts
    sampler, D, mk, options, mode, T = FAMILIES[family]
    r = np.random.default_rng(1000 + D)
    n_sites = 4 if sampler == "nuts" else 2
    rng = planted_sites(D, T, n_sites, seed=D * 10 + T)
    C = rng.shape[0]
    assert C == 4 * len(plant_positions(D, T)) and 12 <= C <= 90
    if mk == "linreg":
        tgt, otgt, imm, N = linreg(r)
        eps = 0.3
        q0 = np.array([3.0, np.log(0.5)]) + (0.5 / np.sqrt(N)) * r.normal(size=(C, 2))
    else:
        tgt, otgt, imm = gaussian(D, r, dense_metric=mk == "dense", per_chain=C if mk == "per_chain" else 0)
        eps = 0.25 / D ** 0.25 if D <= 512 else 0.05 / D ** 0.25   # (the step sizes of the families' own parity tests)
        q0 = r.normal(size=(C, D))
    imm_dev = PerChain(dev(imm)) if mk == "per_chain" else imm
    mod = nuts if sampler == "nuts" else hmc
    extra = () if sampler == "nuts" else (L_HMC,)
    for name, val in options.items():
        eng.set_option(name, val)
    srng = RandomStream.from_state(rng.copy())
    kernel = mod.new_kernel(srng, tgt, max_num_expansions=MAX_EXP) if sampler == "nuts" else mod.new_kernel(srng, tgt)
    state = mod.new_state(dev(q0), tgt)

    # the oracle, chain by chain where every chain has its own matrix
    q, U, g = co.new_state(otgt, q0.copy())

    def oracle_step():
        if mk != "per_chain":
            metric = co.Metric(imm, D)
            return (co.nuts_step(otgt, metric, rng, eps, q, U, g, max_exp=MAX_EXP) if sampler == "nuts"
                    else co.hmc_step(otgt, metric, rng, eps, L_HMC, q, U, g))
        parts = []
        for c in range(C):
            metric = co.Metric(imm[c], D)
            qc, Uc, gc, rc = q[c:c + 1].copy(), U[c:c + 1].copy(), g[c:c + 1].copy(), rng[c:c + 1].copy()
            parts.append(co.nuts_step(otgt, metric, rc, eps, qc, Uc, gc, max_exp=MAX_EXP) if sampler == "nuts"
                         else co.hmc_step(otgt, metric, rc, eps, L_HMC, qc, Uc, gc))
            q[c], U[c], g[c], rng[c] = qc[0], Uc[0], gc[0], rc[0]
        return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}

    def check(info, res, n_leapfrog):
        np.testing.assert_allclose(info.state.position.cpu().numpy().reshape(q.shape), q, rtol=RTOL, atol=1e-12)
        np.testing.assert_allclose(info.state.potential_energy.cpu().numpy().reshape(U.shape), U, rtol=RTOL)
        np.testing.assert_allclose(info.state.potential_energy_grad.cpu().numpy().reshape(g.shape), g, rtol=RTOL, atol=1e-9)
        np.testing.assert_allclose(info.state.momentum.cpu().numpy().reshape(q.shape), res["momentum"], rtol=RTOL, atol=1e-12)
        np.testing.assert_allclose(info.acceptance_probability.cpu().numpy().reshape(-1), res["acceptance_probability"], rtol=RTOL)
        assert np.array_equal(info.is_diverging.cpu().numpy().reshape(-1), res["is_diverging"])
        assert np.array_equal(info.n_leapfrog.cpu().numpy().reshape(-1), n_leapfrog)
        if sampler == "nuts":
            assert np.array_equal(info.num_doublings.cpu().numpy().reshape(-1), res["num_doublings"])
            assert np.array_equal(info.is_turning.cpu().numpy().reshape(-1), res["is_turning"])

    if mode == "steps":
        for t in range(T):
            info, updates = kernel(state, eps, imm_dev, *extra)
            res = oracle_step()
            check(info, res, res["n_leapfrog"])
            assert np.array_equal(words(updates[srng]).reshape(rng.shape)[:, :, :2], rng[:, :, :2]), t
            state = info.state._replace(momentum=None)
    else:
        samples, info, acc, div = kernel.sample(state, eps, imm_dev, *extra, T)[:4]
        total = 0
        for t in range(T):
            res = oracle_step()
            total = total + res["n_leapfrog"]
            np.testing.assert_allclose(samples[t].cpu().numpy().reshape(q.shape), q, rtol=RTOL, atol=1e-12)
            np.testing.assert_allclose(acc[t].cpu().numpy().reshape(-1), res["acceptance_probability"], rtol=RTOL)
            assert np.array_equal(div[t].cpu().numpy().reshape(-1).astype(bool), res["is_diverging"]), t
        check(info, res, total)
        holder = kernel._nuts["holder"] if sampler == "nuts" else kernel._hmc["holder"]
        assert np.array_equal(words(holder["rng"]).reshape(rng.shape)[:, :, :2], rng[:, :, :2])
    assert not res["is_diverging"].all()  # trajectories that ran: the planted |z| of 3.7 to 5 did not blow them up


@pytest.mark.parametrize("D", [7, 257])
def test_ghmc_with_planted_momentum_states(eng, D):
    """Generalised HMC (ghmc_fused.cuh) against tests/meads_ref.py's transition with its numpy generators set to the planted
    states: two transitions, accept flags identical, reals at 1e-9, both generator states of every chain numpy's."""
    import aehmc_amd as aa
    import meads_ref as mr
    T, P = 2, mr.PARITY
    rng = planted_sites(D, T, 2, seed=D + 5)
    C = rng.shape[0]
    r = np.random.default_rng(D)
    t = mr.DiagGaussian(r.normal(size=D), 0.5 + r.random(D))
    q0, s = r.normal(size=(C, D)), mr.parity_scale(D)
    gens = [[rp.numpy_generator(rp.unpack_state(rng[c, k]), (int(rng[c, k, 2]) << 64) | int(rng[c, k, 3])) for c in range(C)]
            for k in range(2)]
    tgt = aa.targets.DiagGaussian(t.mu, t.sigma)
    kernel = aa.ghmc.new_kernel(aa.RandomStream.from_state(rng.copy()), tgt)
    state = aa.ghmc.new_state(dev(q0), tgt)
    ch = mr.start(t, q0)
    for k in range(T):
        info, updates = kernel(state, P["eps"], dev(s), P["alpha"], P["delta"])
        state = info.state
        ch, ref = mr.transition(ch, gens[0], gens[1], t, P["eps"], P["alpha"], P["delta"], s)
        assert ref.margin.min() > 1e-9  # (no accept test within rounding of flipping: fixed data, decided on the host)
        assert np.array_equal(info.is_turning.cpu().numpy(), ref.accepted), k
        assert np.array_equal(info.is_diverging.cpu().numpy(), ref.is_diverging), k
        for got, want in ((state.position, ch.q), (state.potential_energy_grad, ch.g), (state.momentum, ch.v),
                          (state.potential_energy, ch.U), (info.acceptance_probability, ref.acceptance_probability)):
            np.testing.assert_allclose(got.cpu().numpy(), want, rtol=RTOL, atol=1e-12)
    (after,) = updates.values()
    assert np.array_equal(words(after).reshape(C, 2, 4), mr.site_states(gens[0], gens[1]))


# ------------------------------------------------------------------ run-time compiled families
def coupled_gaussian(D):
    sd = 0.5 + np.arange(D) % 3

    def logprob_fn(q):
        z = (q - 1.0) / sd
        return -0.5 * (z @ z) - 0.05 * np.sum(z[1:] * z[:-1])   # (weakly coupled neighbours: a joint density)
    return logprob_fn


# name: (target, D, engine options of the route)
RTC_FAMILIES = {
    "glm-one-launch": ("glm", 10, {}),
    "glm-workgroup": ("glm-small", 10, {"joint_wg": 2}),
    "joint-rows": ("joint", 70, {"joint_resident": 0}),
    "joint-resident": ("joint", 70, {"joint_resident": 2}),
    "joint-workgroup": ("joint", 70, {"joint_wg": 2}),
    "joint-wide": ("joint", 600, {"joint_wide": 2}),
}
LOCKSTEP = {"resident_nuts": 0, "fused_hmc": 0}


@pytest.mark.parametrize("family", list(RTC_FAMILIES))
def test_runtime_compiled_family_equals_lockstep_on_planted_states(eng, family):
    """The run-time compiled kernels carry their own copy of `draw_momentum`: each route against the lock-step route of the
    same target on the same planted states (the pattern of test_custom_glm_one_launch_equals_lockstep) -- generator
    states and discrete outputs identical, reals to 1e-9; the lock-step route is pinned to the oracle above."""
    from aehmc_amd import RandomStream, hmc, nuts, targets
    kind, D, options = RTC_FAMILIES[family]
    T = 2
    r = np.random.default_rng(D + len(family))
    if kind.startswith("glm"):
        import test_gpu_custom_target as tct
        N = 900 if kind == "glm" else 300
        X, y, _ = tct.logistic_data(N, D, 77)
        tgt = targets.CustomGLM(tct.LOGISTIC, X, y, params=[[2.0]])
        imm, eps_n, eps_h = 0.02 + 0.05 * r.random(D), 0.4, 0.3
        scale = 0.3
    else:
        tgt = targets.from_callable(coupled_gaussian(D), D)
        imm, eps_n, eps_h = 0.5 + r.random(D), 0.25 / D ** 0.25, 0.25 / D ** 0.25
        scale = 1.0
    rng_n, rng_h = planted_sites(D, T, 4, seed=D + 1), planted_sites(D, T, 2, seed=D + 2)
    C = rng_n.shape[0]
    q0 = (0.0 if kind.startswith("glm") else 1.0) + scale * r.normal(size=(C, D))
    outs = {}
    for fast in (1, 0):
        for name, val in (options if fast else LOCKSTEP).items():
            eng.set_option(name, val)
        kn = nuts.new_kernel(RandomStream.from_state(rng_n.copy()), tgt, max_num_expansions=MAX_EXP)
        sn, infn = kn.sample(nuts.new_state(dev(q0), tgt), eps_n, imm, T)[:2]
        kh = hmc.new_kernel(RandomStream.from_state(rng_h.copy()), tgt)
        sh, infh, acch = kh.sample(hmc.new_state(dev(q0), tgt), eps_h, imm, L_HMC, T)[:3]
        outs[fast] = (sn, sh, acch, infn.state.momentum, infh.state.momentum, infn.n_leapfrog, infn.num_doublings,
                      infn.is_diverging, infh.is_diverging, kn._nuts["holder"]["rng"].clone(), kh._hmc["holder"]["rng"].clone())
        for name in options:
            eng.set_option(name, OPTION_DEFAULTS[name])
    for k in range(5, 11):
        assert torch.equal(outs[1][k], outs[0][k]), k
    for k in range(5):
        np.testing.assert_allclose(outs[1][k].cpu().numpy(), outs[0][k].cpu().numpy(), rtol=RTOL, atol=1e-12, err_msg=str(k))
    assert int(outs[1][5].sum()) > T * C and not bool(outs[1][7].all())
    # the momentum site moved by the momenta of T transitions at least: the planted positions were all drawn
    assert (words(outs[1][9]).reshape(rng_n.shape)[:, 0, :2] != rng_n[:, 0, :2]).any(axis=1).all()
