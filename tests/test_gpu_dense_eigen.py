"""Eigen route of the whitened dense MVN ("dense_eigen"): the whitened operator H = L^T P L is factored once per
binding, H = V diag(lam) V^T, and a NUTS transition runs in y = V^T z, s = V^T r -- a coordinate-wise Gaussian under the
identity metric, no product inside the lock-step loop.  NUTS is equivariant under the rotation, so against the oracle
and against "dense_eigen" 0 every discrete output and the generator states are identical and the reals agree within
the tolerances of tests/test_gpu_dense_whiten.py.

"dense_eigen" 2 takes the route from D = 513 on (the default, 1, from 2048 on).  Problems as in
test_gpu_dense_whiten.py and test_gpu_white_ahead.py: unrelated random SPD matrices, a non-zero mu, 6 chains; D = 513 is
the smallest whitened size, D = 700 leaves a ragged last batch in the element passes."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu

RTOL = 1e-9  # (test_gpu_dense_whiten.py: rtol 1e-9, atol 1e-12 on vectors)
C, DEPTH = 6, 6
SEEDS = [300 + c for c in range(C)]
# as test_gpu_white_ahead.py chose them for these very problems: at 0.12 the chains make 4 or 5 doublings and differ in
# depth; at 1.1 (D = 513) chains diverge in the first expansion of the first three transitions, but not all of them
EPS, EPS_DIVERGING = 0.12, 1.1


@pytest.fixture(scope="module")
def eng():
    from aehmc_amd.engine import get_engine
    e = get_engine()
    yield e
    e.set_white_basis(None)
    e.set_option("dense_eigen_solver", 1)
    e.set_option("dense_eigen", 1)


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda")


def spd(r, D):
    A = r.normal(size=(D, D))
    m = A @ A.T / D + np.eye(D)
    return 0.5 * (m + m.T)


@functools.lru_cache(maxsize=None)
def problem(D, degenerate=False):
    """mu, P, imm, q0 (test_gpu_white_ahead.problem); degenerate: imm = P^-1, so that H = I up to rounding"""
    r = np.random.default_rng(D)
    mu = r.normal(size=D)
    cov = spd(r, D)
    P = np.linalg.inv(cov)
    P = 0.5 * (P + P.T)
    imm = spd(r, D)
    return mu, P, (cov if degenerate else imm), r.normal(size=(C, D))


def host(info):
    s = info.state
    out = dict(q=s.position, U=s.potential_energy, g=s.potential_energy_grad, p=s.momentum,
               acc=info.acceptance_probability, nl=info.n_leapfrog, nd=info.num_doublings, turn=info.is_turning,
               div=info.is_diverging)
    return {k: v.cpu().numpy() for k, v in out.items()}


def run(eng, prob, eps, n, eigen, rows=None, fresh=False, want_state=None):
    """n chained kernel() calls with "dense_eigen" = eigen: their Diagnostics on the host, then the generator states.
    rows: a subset of the chains.  fresh: every call binds fresh copies of P and of imm.  want_state: the route the
    call must have taken (aehmc_white_basis_info), checked after the first call."""
    from aehmc_amd import RandomStream, nuts, targets
    mu, P, imm, q0 = prob
    rows = list(range(C)) if rows is None else rows
    eng.set_option("dense_eigen", eigen)
    try:
        srng = RandomStream(seeds=[SEEDS[i] for i in rows])
        tgt = targets.DenseMVN(dev(mu), dev(P))
        kernel = nuts.new_kernel(srng, tgt, max_num_expansions=DEPTH)
        state = nuts.new_state(dev(q0[rows]), tgt)
        immd = dev(imm)
        infos = []
        for t in range(n):
            if fresh:
                kernel._nuts["logprob_fn"] = targets.DenseMVN(dev(mu), dev(P))
                immd = dev(imm)
            info, upd = kernel(state, eps, immd)
            if t == 0 and want_state is not None:
                assert eng.white_basis_info()["state"] in want_state, eng.white_basis_info()
            infos.append(host(info))
            state = info.state._replace(momentum=None)
        return infos, upd[srng].cpu().numpy().view(np.uint64).copy()
    finally:
        eng.set_option("dense_eigen", 1)


@functools.lru_cache(maxsize=None)
def whitened(D, eps, degenerate=False):
    """three chained transitions of "dense_eigen" 0, shared by the tests that compare against them"""
    from aehmc_amd.engine import get_engine
    return run(get_engine(), problem(D, degenerate), eps, 3, 0)


def same_discrete(a, b):
    for f in ("nl", "div", "nd", "turn"):
        assert np.array_equal(a[f], b[f]), f


def close_reals(a, q, U, g, p, acc):
    np.testing.assert_allclose(a["q"], q, rtol=RTOL, atol=1e-12)
    np.testing.assert_allclose(a["U"], U, rtol=RTOL)
    np.testing.assert_allclose(a["g"], g, rtol=RTOL, atol=1e-12)
    np.testing.assert_allclose(a["p"], p, rtol=RTOL, atol=1e-12)
    np.testing.assert_allclose(a["acc"], acc, rtol=RTOL)


def same_bytes(a, b, what=""):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


def against_oracle(prob, eps, on, rng_on, D):
    from oracle import c_oracle as co
    mu, P, imm, q0 = prob
    otgt, metric = co.Target(co.T_DENSE_MVN, D, mu=mu, prec=P), co.Metric(imm, D)
    rng = co.site_states(SEEDS, 4)
    q, U, g = co.new_state(otgt, q0.copy())
    for a in on:
        res = co.nuts_step(otgt, metric, rng, eps, q, U, g, max_exp=DEPTH, nthreads=C)
        assert np.array_equal(a["nd"], res["num_doublings"]) and np.array_equal(a["turn"], res["is_turning"])
        assert np.array_equal(a["nl"], res["n_leapfrog"]) and np.array_equal(a["div"], res["is_diverging"])
        close_reals(a, q, U, g, res["momentum"], res["acceptance_probability"])
    assert np.array_equal(rng_on[:, :, :2], rng[:, :, :2])


@gpu
@pytest.mark.parametrize("D", [513, 700])
def test_eigen_route_matches_oracle(eng, D):
    """Three chained NUTS transitions at depth 6 against the C oracle, with the solver's basis; discrete outputs and
    generator states identical to "dense_eigen" 0."""
    prob = problem(D)
    on, rng_on = run(eng, prob, EPS, 3, 2, want_state=(1, 3))
    off, rng_off = whitened(D, EPS)
    assert rng_on.tobytes() == rng_off.tobytes()
    for a, b in zip(on, off):
        same_discrete(a, b)
    assert max(a["nd"].max() for a in on) >= 4
    against_oracle(prob, EPS, on, rng_on, D)


@gpu
def test_eigen_route_degenerate_spectrum(eng):
    """imm = P^-1: H = I up to rounding, every eigenvalue within rounding of 1 and the eigenvectors arbitrary -- the
    benchmark's own case.  The basis passes the acceptance check and the transitions equal the oracle's."""
    D = 513
    prob = problem(D, True)
    on, rng_on = run(eng, prob, EPS, 3, 2, want_state=(1, 3))
    off, rng_off = whitened(D, EPS, True)
    assert rng_on.tobytes() == rng_off.tobytes()
    for a, b in zip(on, off):
        same_discrete(a, b)
        close_reals(a, b["q"], b["U"], b["g"], b["p"], b["acc"])
    against_oracle(prob, EPS, on, rng_on, D)


@gpu
def test_eigen_route_diverging_chains(eng):
    """A step size at which chains diverge in the first expansion: the discrete outputs and generator states of
    "dense_eigen" 0, reals within tolerance (a chain that diverged at once returns its input)."""
    D = 513
    on, rng_on = run(eng, problem(D), EPS_DIVERGING, 3, 2, want_state=(1, 3))
    off, rng_off = whitened(D, EPS_DIVERGING)
    div = np.stack([h["div"] for h in off])
    assert div.any() and not div.all(), div
    assert rng_on.tobytes() == rng_off.tobytes()
    for a, b in zip(on, off):
        same_discrete(a, b)
        close_reals(a, b["q"], b["U"], b["g"], b["p"], b["acc"])


@gpu
def test_eigen_route_chains_do_not_depend_on_their_batch(eng):
    """Three of the six chains run alone equal the same chains in the full launch, bit for bit."""
    D, sub = 700, [1, 4, 5]
    full, rng_full = run(eng, problem(D), EPS, 2, 2, want_state=(1, 3))
    part, rng_part = run(eng, problem(D), EPS, 2, 2, rows=sub, want_state=(1, 3))
    assert rng_full[sub].tobytes() == rng_part.tobytes()
    for a, b in zip(full, part):
        same_bytes({k: v[sub] for k, v in a.items()}, b)
    assert len(np.unique(full[0]["nl"])) >= 2


@gpu
def test_eigen_route_unmoved_chains_return_their_input_bitwise(eng):
    """A chain whose returned point is its initial one (every chain diverges on its first step here) returns the
    caller's (q, U, g) bit for bit, not their round trip through the basis."""
    from aehmc_amd import nuts, targets
    D = 513
    mu, P, imm, q0 = problem(D)
    st = nuts.new_state(dev(q0), targets.DenseMVN(dev(mu), dev(P)))
    want = dict(q=st.position, U=st.potential_energy, g=st.potential_energy_grad)
    infos, _ = run(eng, problem(D), 5.0, 1, 2, want_state=(1, 3))
    assert infos[0]["div"].all()
    for k, v in want.items():
        assert infos[0][k].tobytes() == v.cpu().numpy().tobytes(), k


@gpu
def test_eigen_route_sample_and_fresh_copies_equal_single_calls(eng):
    """sample(4) equals four single calls bit for bit, and so do four calls that each bind fresh copies of the precision
    and of the inverse mass matrix: the operator formed again has the old bits, so the basis is the one kept aside
    (state 3: the solver does not run again) and the carried state counts."""
    from aehmc_amd import RandomStream, nuts, targets
    D, T = 700, 4
    mu, P, imm, q0 = problem(D)
    singles, rng_s = run(eng, problem(D), EPS, T, 2, want_state=(1, 3))
    fresh, rng_f = run(eng, problem(D), EPS, T, 2, fresh=True)
    assert eng.white_basis_info()["state"] == 3
    assert rng_f.tobytes() == rng_s.tobytes()
    for t in range(T):
        same_bytes(fresh[t], singles[t], f"fresh copies, transition {t}")
    eng.set_option("dense_eigen", 2)
    try:
        srng = RandomStream(seeds=SEEDS)
        tgt = targets.DenseMVN(dev(mu), dev(P))
        kernel = nuts.new_kernel(srng, tgt, max_num_expansions=DEPTH)
        samples, info, acc_hist, div_hist = kernel.sample(nuts.new_state(dev(q0), tgt), EPS, dev(imm), T)
        assert eng.white_basis_info()["state"] in (1, 3)
    finally:
        eng.set_option("dense_eigen", 1)
    assert kernel._nuts["holder"]["rng"].cpu().numpy().view(np.uint64).tobytes() == rng_s.tobytes()
    for t in range(T):
        assert samples[t].cpu().numpy().tobytes() == singles[t]["q"].tobytes(), t
        assert acc_hist[t].cpu().numpy().tobytes() == singles[t]["acc"].tobytes(), t
    last = host(info)
    for k in ("q", "U", "g"):
        assert last[k].tobytes() == singles[-1][k].tobytes(), k


def whitened_operator(prob):
    """H = L^T P L as the engine's arithmetic defines it, on the host (its eigenvectors are the same up to rounding)"""
    mu, P, imm, q0 = prob
    L = np.linalg.cholesky(imm)
    H = L.T @ P @ L
    return 0.5 * (H + H.T)


@gpu
def test_supplied_basis_is_checked(eng):
    """A basis from numpy's eigh gives the route (state 2) and the oracle's transitions; a deliberately non-orthogonal
    one is rejected (state -3) and the results have the bits of "dense_eigen" 0.  The measured acceptance quantities of
    LAPACK's basis are far inside the bounds."""
    D = 513
    prob = problem(D)
    lam, V = np.linalg.eigh(whitened_operator(prob))
    off, rng_off = whitened(D, EPS)
    try:
        eng.set_white_basis(dev(V), dev(lam))
        on, rng_on = run(eng, prob, EPS, 3, 2, want_state=(2,))
        info = eng.white_basis_info()
        print("numpy eigh, D = 513: orth", info["orth"], "resid", info["resid"])
        assert 0 <= info["orth"] <= 4.6e-14 and 0 <= info["resid"] <= 2.4e-14, info  # (the engine's bounds: DESIGN §3)
        assert rng_on.tobytes() == rng_off.tobytes()
        for a, b in zip(on, off):
            same_discrete(a, b)
        against_oracle(prob, EPS, on, rng_on, D)
        bad = V.copy()
        bad[:, 0] += 1e-6 * bad[:, 1]
        eng.set_white_basis(dev(bad), dev(lam))
        rej, rng_rej = run(eng, prob, EPS, 3, 2, want_state=(-3,))
        assert rng_rej.tobytes() == rng_off.tobytes()
        for a, b in zip(rej, off):
            same_bytes(a, b, "rejected basis")
    finally:
        eng.set_white_basis(None)


@gpu
def test_missing_solver_gives_the_whitened_route(eng):
    """With the solver's symbols not found (the test hook) the whitened route runs: state -1, the bits of "dense_eigen" 0."""
    D = 513
    off, rng_off = whitened(D, EPS)
    eng.set_option("dense_eigen_solver", 0)
    try:
        got, rng_got = run(eng, problem(D), EPS, 3, 2, want_state=(-1,))
    finally:
        eng.set_option("dense_eigen_solver", 1)
    assert rng_got.tobytes() == rng_off.tobytes()
    for a, b in zip(got, off):
        same_bytes(a, b, "no solver")


def test_rotated_reference_transition_equals_the_whitened_one():
    """On the CPU, with the numpy oracle at D = 64: the reference NUTS transition of the coordinate-wise Gaussian
    (Lambda, identity metric) from y0 = V^T z0 with the momentum V^T r (r: the normals the whitened transition draws),
    mapped back with V, equals the whitened transition on (H, identity metric): discrete outputs identical, reals within
    the tolerance of the GPU tests."""
    from oracle import np_oracle as npo
    D = 64
    r = np.random.default_rng(64)
    H = spd(r, D) @ np.diag(r.uniform(0.2, 3.0, size=D))
    H = 0.5 * (H + H.T) + D * 0.01 * np.eye(D)
    lam, V = np.linalg.eigh(H)

    class Eigen:  # dU/dy_i = lam_i y_i, U = 0.5 sum y_i dU/dy_i
        def __call__(self, y):
            g = lam * np.asarray(y, dtype=np.float64)
            return float(0.5 * np.dot(y, g)), g

    class Rotated:  # the momentum site: V^T r of the normals it draws
        def __init__(self, gen):
            self.gen = gen

        def normal(self, loc, scale, size):
            return V.T @ self.gen.normal(loc, scale, size=size)

    class RotatedStream(npo.RandomStream):
        first = True

        def site(self):
            gen = super().site()
            if self.first:
                self.first = False
                return Rotated(gen)
            return gen

    eps, imm = 0.3 / np.sqrt(lam.max()), np.ones(D)
    moved = 0
    for seed in range(6):
        z0 = np.random.default_rng(1000 + seed).normal(size=D)
        white_t, eigen_t = npo.DenseMVN(np.zeros(D), H), Eigen()
        a = npo.nuts_kernel(npo.RandomStream(seed), white_t, DEPTH)(npo.new_state(z0, white_t), eps, imm)
        b = npo.nuts_kernel(RotatedStream(seed), eigen_t, DEPTH)(npo.new_state(V.T @ z0, eigen_t), eps, imm)
        assert (a.num_doublings, a.is_turning, a.is_diverging, a.n_leapfrog) == \
               (b.num_doublings, b.is_turning, b.is_diverging, b.n_leapfrog)
        np.testing.assert_allclose(V @ b.state.position, a.state.position, rtol=RTOL, atol=1e-12)
        np.testing.assert_allclose(V @ b.state.momentum, a.state.momentum, rtol=RTOL, atol=1e-12)
        np.testing.assert_allclose(V @ b.state.potential_energy_grad, a.state.potential_energy_grad, rtol=RTOL, atol=1e-12)
        np.testing.assert_allclose(b.state.potential_energy, a.state.potential_energy, rtol=RTOL)
        np.testing.assert_allclose(b.acceptance_probability, a.acceptance_probability, rtol=RTOL)
        moved += a.num_doublings
    assert moved >= 12  # (the trees are real ones)
