"""Whitened dense MVN ("dense_whiten", the default): a dense-precision Gaussian under a shared dense inverse mass matrix,
D > 512, on the lock-step path runs its leapfrogs in z = L^-1 (q - mu), r = L^T p (imm = L L^T): one product with
H = L^T P L per leapfrog instead of two.  The transition is mapped in and out on its own, so results equal the
untransformed arithmetic up to rounding: every discrete output and the RNG consumption identical, reals within 1e-9.

The matrices here are unrelated random SPD matrices and mu is non-zero, so H is far from the identity."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import c_oracle as co  # noqa: E402

RTOL = 1e-9


@pytest.fixture(scope="module")
def eng():
    from aehmc_amd.engine import get_engine
    return get_engine()


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda")


def spd(r, D):
    A = r.normal(size=(D, D))
    m = A @ A.T / D + np.eye(D)
    return 0.5 * (m + m.T)


def problem(D, seed):
    r = np.random.default_rng(seed)
    mu = r.normal(size=D)
    cov = spd(r, D)
    P = np.linalg.inv(cov)
    P = 0.5 * (P + P.T)
    imm = spd(r, D)
    return r, mu, P, imm


def new_kernel(mod, srng, tgt, max_exp=6):
    from aehmc_amd import nuts
    return mod.new_kernel(srng, tgt, max_num_expansions=max_exp) if mod is nuts else mod.new_kernel(srng, tgt)


def run(mod, tgt, imm, q0, seeds, eps, n, extra, whiten, eng, max_exp=6):
    """n consecutive transitions: their Diagnostics, then the generator states"""
    from aehmc_amd import RandomStream
    eng.set_option("dense_whiten", whiten)
    try:
        srng = RandomStream(seeds=seeds)
        kernel = new_kernel(mod, srng, tgt, max_exp)
        state = mod.new_state(dev(q0), tgt)
        infos = []
        for _ in range(n):
            info, upd = kernel(state, eps, dev(imm) if isinstance(imm, np.ndarray) else imm, *extra)
            infos.append(info)
            state = info.state._replace(momentum=None)
        return infos, upd[srng].cpu().numpy().view(np.uint64).copy()
    finally:
        eng.set_option("dense_whiten", 1)


def host(info):
    s = info.state
    out = dict(q=s.position, U=s.potential_energy, g=s.potential_energy_grad, p=s.momentum,
               acc=info.acceptance_probability, nl=info.n_leapfrog, nd=getattr(info, "num_doublings", None),
               turn=info.is_turning, div=info.is_diverging)
    return {k: v.cpu().numpy() for k, v in out.items() if v is not None}


def same_discrete(a, b, nuts=True):
    for f in ("nl", "div") + (("nd", "turn") if nuts else ()):
        assert np.array_equal(a[f], b[f]), f


def close_reals(a, q, U, g, p, acc):
    np.testing.assert_allclose(a["q"], q, rtol=RTOL, atol=1e-12)
    np.testing.assert_allclose(a["U"], U, rtol=RTOL)
    np.testing.assert_allclose(a["g"], g, rtol=RTOL, atol=1e-12)
    np.testing.assert_allclose(a["p"], p, rtol=RTOL, atol=1e-12)
    np.testing.assert_allclose(a["acc"], acc, rtol=RTOL)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("D", [700, 1500, 2048])
def test_whitened_dense_mvn_matches_oracle(eng, D):
    """NUTS (depth 6, three transitions) and HMC (L = 11) against the C oracle; the same runs with "dense_whiten" 0
    give identical discrete outputs and generator states."""
    from aehmc_amd import hmc, nuts, targets
    r, mu, P, imm = problem(D, D)
    C, eps = 4, 0.12
    seeds = [300 + c for c in range(C)]
    q0 = r.normal(size=(C, D))
    tgt = targets.DenseMVN(dev(mu), dev(P))
    otgt, metric = co.Target(co.T_DENSE_MVN, D, mu=mu, prec=P), co.Metric(imm, D)
    for mod, n, extra, nsites in ((nuts, 3, (), 4), (hmc, 1, (11,), 2)):
        is_nuts = mod is nuts
        on, rng_on = run(mod, tgt, imm, q0, seeds, eps, n, extra, 1, eng)
        off, rng_off = run(mod, tgt, imm, q0, seeds, eps, n, extra, 0, eng)
        assert np.array_equal(rng_on, rng_off)
        rng = co.site_states(seeds, nsites)
        q, U, g = co.new_state(otgt, q0.copy())
        for t in range(n):
            a, b = host(on[t]), host(off[t])
            same_discrete(a, b, is_nuts)
            if is_nuts:
                res = co.nuts_step(otgt, metric, rng, eps, q, U, g, max_exp=6, nthreads=C)
                assert np.array_equal(a["nd"], res["num_doublings"]) and np.array_equal(a["turn"], res["is_turning"])
            else:
                res = co.hmc_step(otgt, metric, rng, eps, 11, q, U, g, nthreads=C)
            assert np.array_equal(a["nl"], res["n_leapfrog"]) and np.array_equal(a["div"], res["is_diverging"])
            close_reals(a, q, U, g, res["momentum"], res["acceptance_probability"])
        assert np.array_equal(rng_on[:, :, :2], rng[:, :, :2])


@pytest.mark.timeout(600)
def test_whitened_unmoved_chains_return_their_input_bitwise(eng):
    """A chain whose returned point is its initial one -- an HMC rejection, a NUTS divergence on the first step --
    returns the caller's (q, U, g) bit for bit, not their round trip through the whitening map."""
    from aehmc_amd import hmc, nuts, targets
    D = 640
    r, mu, P, imm = problem(D, 5)
    C = 6
    seeds = [40 + c for c in range(C)]
    q0 = mu + r.normal(size=(C, D))
    tgt = targets.DenseMVN(dev(mu), dev(P))
    st = nuts.new_state(dev(q0), tgt)
    q_in, U_in, g_in = (x.cpu().numpy() for x in (st.position, st.potential_energy, st.potential_energy_grad))
    for mod, extra in ((hmc, (7,)), (nuts, ())):
        infos, _ = run(mod, tgt, imm, q0, seeds, 5.0, 1, extra, 1, eng)  # step far too large: every chain diverges
        a = host(infos[0])
        assert a["div"].all()
        assert np.array_equal(a["q"].view(np.int64), q_in.view(np.int64))
        assert np.array_equal(a["U"].view(np.int64), U_in.view(np.int64))
        assert np.array_equal(a["g"].view(np.int64), g_in.view(np.int64))


@pytest.mark.timeout(600)
def test_whitened_chains_do_not_depend_on_their_batch(eng):
    """Five of twelve chains run alone equal the same chains in the full launch, bit for bit (NUTS: chains leave the
    compacted GEMMs at different steps; HMC)."""
    from aehmc_amd import hmc, nuts, targets
    D = 1100
    r, mu, P, imm = problem(D, 11)
    C, eps = 12, 0.12
    seeds = [700 + c for c in range(C)]
    q0 = r.normal(size=(C, D))
    tgt = targets.DenseMVN(dev(mu), dev(P))
    sub = [1, 4, 5, 9, 11]
    for mod, extra in ((nuts, ()), (hmc, (9,))):
        full, rng_full = run(mod, tgt, imm, q0, seeds, eps, 2, extra, 1, eng)
        part, rng_part = run(mod, tgt, imm, q0[sub], [seeds[i] for i in sub], eps, 2, extra, 1, eng)
        assert np.array_equal(rng_full[sub], rng_part)
        for a, b in zip(full, part):
            a, b = host(a), host(b)
            for k in a:
                assert np.array_equal(a[k][sub], b[k]), k
        if mod is nuts:
            assert len(np.unique(host(full[0])["nl"])) >= 2


@pytest.mark.timeout(600)
def test_whitened_sample_equals_single_calls(eng):
    """sample(4) equals four single transitions bit for bit: every transition maps in and out on its own."""
    from aehmc_amd import RandomStream, hmc, nuts, targets
    D = 900
    r, mu, P, imm = problem(D, 3)
    C, eps = 5, 0.12
    seeds = [20 + c for c in range(C)]
    q0 = r.normal(size=(C, D))
    tgt = targets.DenseMVN(dev(mu), dev(P))
    for mod, extra in ((nuts, ()), (hmc, (9,))):
        singles, rng_s = run(mod, tgt, imm, q0, seeds, eps, 4, extra, 1, eng)
        srng = RandomStream(seeds=seeds)
        kernel = new_kernel(mod, srng, tgt)
        samples, info, acc_hist, div_hist = kernel.sample(mod.new_state(dev(q0), tgt), eps, dev(imm), *extra, 4)
        rng_m = (kernel._nuts if mod is nuts else kernel._hmc)["holder"]["rng"].cpu().numpy().view(np.uint64)
        assert np.array_equal(rng_m, rng_s)
        for t in range(4):
            assert np.array_equal(samples[t].cpu().numpy(), singles[t].state.position.cpu().numpy()), t
            assert np.array_equal(acc_hist[t].cpu().numpy(), singles[t].acceptance_probability.cpu().numpy()), t
        last = singles[-1].state
        assert np.array_equal(info.state.position.cpu().numpy(), last.position.cpu().numpy())
        assert np.array_equal(info.state.potential_energy.cpu().numpy(), last.potential_energy.cpu().numpy())
        assert np.array_equal(info.state.potential_energy_grad.cpu().numpy(), last.potential_energy_grad.cpu().numpy())


@pytest.mark.timeout(600)
def test_whitened_operator_follows_the_bound_arrays(eng):
    """The whitened operator is formed from the bound arrays and dropped on every re-binding: after an in-place edit of
    the precision or of the inverse mass matrix (the Python layer binds again: the tensor's version moved) the results
    equal those after a forced re-bind; two targets alternating on one metric give the results of fresh bindings."""
    from aehmc_amd import nuts, targets
    D = 800
    r, mu, P, imm = problem(D, 17)
    C, eps = 4, 0.12
    seeds = [60 + c for c in range(C)]
    q0 = r.normal(size=(C, D))
    Pd, immd = dev(P), dev(imm)
    tgt = targets.DenseMVN(dev(mu), Pd)

    def go(t, m, force=False):
        if force:
            eng.set_target(t, D, force=True)
            eng.set_metric(m, D, force=True)
        infos, rng = run(nuts, t, m, q0, seeds, eps, 1, (), 1, eng)
        return host(infos[0]), rng

    def same(a, b):
        assert np.array_equal(a[1], b[1])
        for k in a[0]:
            assert np.array_equal(a[0][k], b[0][k]), k

    before = go(tgt, immd)
    Pd.mul_(1.25)  # in place: the same tensor object
    edited = go(tgt, immd)
    assert not np.array_equal(edited[0]["q"], before[0]["q"])
    same(edited, go(tgt, immd, force=True))
    immd.mul_(0.8)
    edited = go(tgt, immd)
    same(edited, go(tgt, immd, force=True))

    other = targets.DenseMVN(dev(mu[::-1].copy()), dev(np.linalg.inv(spd(r, D))))
    fresh_a, fresh_b = go(tgt, immd, force=True), go(other, immd, force=True)
    for _ in range(2):
        same(go(tgt, immd), fresh_a)
        same(go(other, immd), fresh_b)


@pytest.mark.timeout(1200)
def test_whitened_c3_shape_depth10_matches_unwhitened():
    """c3 (D = 1e4 AR(1) precision, imm = Sigma, the bench's step size) with 256 chains at max_num_expansions = 10:
    whitening on and off give identical discrete outputs and generator states, reals within 1e-9."""
    from bench import build_c3

    from aehmc_amd import nuts, targets
    from aehmc_amd.engine import get_engine
    eng = get_engine()
    D, C = 10_000, 256
    eps = 0.5 * D ** -0.25
    Sigma, P = build_c3(D, torch.device("cuda"))
    tgt = targets.DenseMVN(torch.zeros(D, dtype=torch.float64, device="cuda"), P)
    seeds = [1000 + c for c in range(C)]
    q0 = np.random.default_rng(1234).standard_normal((C, D))
    on, rng_on = run(nuts, tgt, Sigma, q0, seeds, eps, 1, (), 1, eng, max_exp=10)
    off, rng_off = run(nuts, tgt, Sigma, q0, seeds, eps, 1, (), 0, eng, max_exp=10)
    assert np.array_equal(rng_on, rng_off)
    a, b = host(on[0]), host(off[0])
    same_discrete(a, b)
    assert a["nd"].max() >= 5
    close_reals(a, b["q"], b["U"], b["g"], b["p"], b["acc"])
