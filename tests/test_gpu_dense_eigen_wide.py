"""Eigen route of the whitened dense MVN, loop in the workgroup-per-chain kernel ("dense_eigen_wide", the default for
512 < D <= 10176): between the boundary products one launch of k_nuts_wide's AEHMC_T_WHITE_EIGEN instantiation carries
every chain through its whole tree -- lambda where the isotropic instantiation keeps the metric, the rotated momentum
preset -- in the place of the diagonal lock-step stage.

The references are the routes that existed before it, never the new code: the lock-step eigen stage
("dense_eigen_wide" 0), the whitened route ("dense_eigen" 0) and, at D = 513 and 700, the C oracle.  Discrete outputs
and generator states are identical, reals agree within 1e-9 relative + 1e-12 absolute (tests/test_gpu_dense_eigen.py).

Shapes: one per instantiation of the kernel, the smallest that reaches it and leaves its last slot ragged --
    513, 700   <256, 4>         slots past D; at 513 one element in the third slot
    1100       <256, 8>
    2100       <512, 8>         above the default threshold of "dense_eigen" (below it the tests set "dense_eigen" 2)
    4100       <512, 16, true>  first shape with q and lambda in LDS
    8200       <512, 20, true>  the benchmark's instantiation
D = 513 / 700: the random SPD problems of test_gpu_dense_eigen.py, eps 0.12.  From 1100 on the operators are the
benchmark's AR(1) closed forms built on the device, the metric with another rho than the target's covariance (0.3
against 0.5: the eigenvalues of H lie in about [0.6, 1.6]), eps 0.15: half a period of the slowest and fastest coordinate
is 27 and 16 leapfrogs, so trees end by U-turn after 4 or 5 doublings.

Every comparison case is two runs -- depth limit 6 (chained transitions) and depth limit 3 (one transition) -- and
asserts on the REFERENCE's outputs that its chains include three with num_doublings >= 4 (they have expanded to both
sides up to probability 2^-3 each), one that ended by U-turn and one that ended at the depth limit."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu

RTOL, ATOL = 1e-9, 1e-12
C = 6
SEEDS = [300 + c for c in range(C)]
EPS, EPS_AR, EPS_DIVERGING = 0.12, 0.15, 1.1  # (0.12 and 1.1: test_gpu_dense_eigen.py, for the same problems)
DEEP, SHALLOW = 6, 3
WIDE, LOCKSTEP, WHITENED = "wide", "lockstep", "whitened"


@pytest.fixture(scope="module")
def eng():
    from aehmc_amd.engine import get_engine
    e = get_engine()
    yield e
    e.set_option("dense_eigen_wide", 1)
    e.set_option("dense_eigen", 1)


def dev(x):
    if isinstance(x, torch.Tensor):
        return x
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda")


def spd(r, D):
    A = r.normal(size=(D, D))
    m = A @ A.T / D + np.eye(D)
    return 0.5 * (m + m.T)


@functools.lru_cache(maxsize=None)
def problem(D, degenerate=False):
    """mu, P, imm, q0 of test_gpu_dense_eigen.problem (host); degenerate: imm = P^-1, so that H = I up to rounding"""
    r = np.random.default_rng(D)
    mu = r.normal(size=D)
    cov = spd(r, D)
    P = np.linalg.inv(cov)
    P = 0.5 * (P + P.T)
    imm = spd(r, D)
    return mu, P, (cov if degenerate else imm), r.normal(size=(C, D))


def ar1(D, rho):
    """Sigma_ij = rho^|i-j| s_i s_j, s_i = 1 + (i mod 3), and its tridiagonal inverse, dense, on the device (bench.py c3)"""
    i = torch.arange(D, device="cuda")
    s = (1.0 + (i % 3)).to(torch.float64)
    Sigma = s[:, None] * rho ** (i[:, None] - i[None, :]).abs().to(torch.float64) * s[None, :]
    d = torch.full((D,), (1 + rho * rho) / (1 - rho * rho), dtype=torch.float64, device="cuda")
    d[0] = d[-1] = 1.0 / (1 - rho * rho)
    off = torch.full((D - 1,), -rho / (1 - rho * rho), dtype=torch.float64, device="cuda")
    P = (torch.diag(d) + torch.diag(off, 1) + torch.diag(off, -1)) / s[:, None] / s[None, :]
    return (0.5 * (Sigma + Sigma.T)).contiguous(), (0.5 * (P + P.T)).contiguous()


@functools.lru_cache(maxsize=1)  # (one D at a time: the matrices of D = 8200 are 0.5 GB each)
def problem_ar(D):
    """target: covariance AR(1) rho 0.5 (its precision P); metric: AR(1) rho 0.3 -- a well-conditioned H = L^T P L that
    is far from the identity.  Device tensors; q0 = mu + the scales o standard normals."""
    _, P = ar1(D, 0.5)
    imm, _ = ar1(D, 0.3)
    i = torch.arange(D, device="cuda", dtype=torch.float64)
    mu = torch.sin(0.37 * i)
    gen = torch.Generator(device="cuda").manual_seed(D)
    q0 = mu + (1.0 + (i % 3)) * torch.randn((C, D), dtype=torch.float64, device="cuda", generator=gen)
    return mu, P, imm, q0


def host(info):
    s = info.state
    out = dict(q=s.position, U=s.potential_energy, g=s.potential_energy_grad, p=s.momentum,
               acc=info.acceptance_probability, nl=info.n_leapfrog, nd=info.num_doublings, turn=info.is_turning,
               div=info.is_diverging)
    return {k: v.cpu().numpy() for k, v in out.items()}


def run(eng, prob, eps, n, route, depth=DEEP, rows=None, fresh=False, need_basis=True):
    """n chained kernel() calls on `route`: their Diagnostics on the host, then the generator states.  rows: a subset
    of the chains.  fresh: every call binds fresh copies of P and of imm."""
    from aehmc_amd import RandomStream, nuts, targets
    mu, P, imm, q0 = (dev(x) for x in prob)
    D = mu.shape[0]
    rows = list(range(C)) if rows is None else rows
    eng.set_option("dense_eigen", 0 if route == WHITENED else 2 if D < 2048 else 1)
    eng.set_option("dense_eigen_wide", 1 if route == WIDE else 0)
    try:
        srng = RandomStream(seeds=[SEEDS[i] for i in rows])
        tgt = targets.DenseMVN(mu, P)
        kernel = nuts.new_kernel(srng, tgt, max_num_expansions=depth)
        state = nuts.new_state(q0[rows].contiguous(), tgt)
        immd = imm
        infos = []
        for t in range(n):
            if fresh:
                kernel._nuts["logprob_fn"] = targets.DenseMVN(mu.clone(), P.clone())
                immd = imm.clone()
            info, upd = kernel(state, eps, immd)
            if t == 0 and route != WHITENED and need_basis:
                st = eng.white_basis_info()["state"]
                if st == -1 and D >= 2048:
                    pytest.skip("no eigensolver library on this machine: the eigen route is not taken")
                assert st in (1, 3), eng.white_basis_info()
            infos.append(host(info))
            state = info.state._replace(momentum=None)
        return infos, upd[srng].cpu().numpy().view(np.uint64).copy()
    finally:
        eng.set_option("dense_eigen", 1)
        eng.set_option("dense_eigen_wide", 1)


def get_problem(D, degenerate=False):
    return problem(D, degenerate) if D < 1024 else problem_ar(D)


def both_depths(eng, D, route, degenerate=False):
    """the two runs of a comparison case: (infos, generator states) at depth limit 6 and at depth limit 3"""
    prob, eps = get_problem(D, degenerate), (EPS if D < 1024 else EPS_AR)
    n = 3 if D < 1024 else 2
    return run(eng, prob, eps, n, route, DEEP), run(eng, prob, eps, 1, route, SHALLOW)


def same_discrete(a, b):
    for f in ("nl", "div", "nd", "turn"):
        assert np.array_equal(a[f], b[f]), f


def close_reals(a, b):
    for k in ("q", "g", "p"):
        np.testing.assert_allclose(a[k], b[k], rtol=RTOL, atol=ATOL, err_msg=k)
    for k in ("U", "acc"):
        np.testing.assert_allclose(a[k], b[k], rtol=RTOL, atol=ATOL, err_msg=k)


def same_bytes(a, b, what=""):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


def covered(deep, shallow):
    """the coverage condition, on a reference's outputs"""
    nd = np.concatenate([h["nd"] for h in deep])
    assert (nd >= 4).sum() >= 3, nd
    ends = [(h, d) for hs, d in ((deep, DEEP), (shallow, SHALLOW)) for h in hs]
    assert any(((h["turn"] != 0) & (h["div"] == 0)).any() for h, d in ends), "no chain ended by U-turn"
    assert any(((h["nd"] == d) & (h["turn"] == 0) & (h["div"] == 0)).any() for h, d in ends), "no chain ended at the depth limit"


def compare(new, ref):
    for (infos_n, rng_n), (infos_r, rng_r) in zip(new, ref):
        assert rng_n.tobytes() == rng_r.tobytes()
        for a, b in zip(infos_n, infos_r):
            same_discrete(a, b)
            close_reals(a, b)


def against_oracle(prob, eps, depth, on, rng_on, D):
    from oracle import c_oracle as co
    mu, P, imm, q0 = prob
    otgt, metric = co.Target(co.T_DENSE_MVN, D, mu=mu, prec=P), co.Metric(imm, D)
    rng = co.site_states(SEEDS, 4)
    q, U, g = co.new_state(otgt, q0.copy())
    for a in on:
        res = co.nuts_step(otgt, metric, rng, eps, q, U, g, max_exp=depth, nthreads=C)
        same_discrete(a, dict(nl=res["n_leapfrog"], div=res["is_diverging"], nd=res["num_doublings"], turn=res["is_turning"]))
        close_reals(a, dict(q=q, U=U, g=g, p=res["momentum"], acc=res["acceptance_probability"]))
    assert np.array_equal(rng_on[:, :, :2], rng[:, :, :2])


@gpu
@pytest.mark.parametrize("D", [513, 700, 1100, 2100, 4100, 8200])
def test_wide_loop_matches_the_routes_before_it(eng, D):
    """The lock-step eigen stage and the whitened route (and the C oracle at D = 513, 700): discrete outputs and
    generator states identical, reals within tolerance, at depth limits 6 and 3."""
    new = both_depths(eng, D, WIDE)
    for route in (LOCKSTEP, WHITENED):
        ref = both_depths(eng, D, route)
        covered(ref[0][0], ref[1][0])
        compare(new, ref)
    if D < 1024:
        for (infos, rng), depth in zip(new, (DEEP, SHALLOW)):
            against_oracle(problem(D), EPS, depth, infos, rng, D)


@gpu
def test_wide_loop_degenerate_spectrum(eng):
    """imm = P^-1: H = I up to rounding, every eigenvalue within rounding of 1, the eigenvectors arbitrary -- the
    benchmark's own case."""
    D = 513
    new = both_depths(eng, D, WIDE, True)
    for route in (LOCKSTEP, WHITENED):
        ref = both_depths(eng, D, route, True)
        covered(ref[0][0], ref[1][0])
        compare(new, ref)
    for (infos, rng), depth in zip(new, (DEEP, SHALLOW)):
        against_oracle(problem(D, True), EPS, depth, infos, rng, D)


@gpu
def test_wide_loop_diverging_chains(eng):
    """A step size at which chains diverge in the first expansion, but not all of them (a chain that diverged at once
    returns its input)."""
    D = 513
    new = run(eng, problem(D), EPS_DIVERGING, 3, WIDE)
    for route in (LOCKSTEP, WHITENED):
        ref = run(eng, problem(D), EPS_DIVERGING, 3, route)
        div = np.stack([h["div"] for h in ref[0]])
        assert div.any() and not div.all(), div
        compare([new], [ref])


@gpu
def test_wide_loop_chains_do_not_depend_on_their_batch(eng):
    """Three of the six chains run alone equal the same chains in the full launch, bit for bit."""
    D, sub = 700, [1, 4, 5]
    full, rng_full = run(eng, problem(D), EPS, 2, WIDE)
    part, rng_part = run(eng, problem(D), EPS, 2, WIDE, rows=sub)
    assert rng_full[sub].tobytes() == rng_part.tobytes()
    for a, b in zip(full, part):
        same_bytes({k: v[sub] for k, v in a.items()}, b)
    assert len(np.unique(full[0]["nl"])) >= 2


@gpu
def test_wide_loop_unmoved_chains_return_their_input_bitwise(eng):
    """A chain whose returned point is its initial one (every chain diverges on its first step here) returns the
    caller's (q, U, g) bit for bit, not their round trip through the basis."""
    from aehmc_amd import nuts, targets
    D = 513
    mu, P, imm, q0 = problem(D)
    st = nuts.new_state(dev(q0), targets.DenseMVN(dev(mu), dev(P)))
    want = dict(q=st.position, U=st.potential_energy, g=st.potential_energy_grad)
    infos, _ = run(eng, problem(D), 5.0, 1, WIDE)
    assert infos[0]["div"].all()
    for k, v in want.items():
        assert infos[0][k].tobytes() == v.cpu().numpy().tobytes(), k


@gpu
def test_wide_loop_sample_and_fresh_copies_equal_single_calls(eng):
    """sample(4) equals four single calls bit for bit, and so do four calls that each bind fresh copies of the precision
    and of the inverse mass matrix (the carried state counts on this route as on the lock-step one)."""
    from aehmc_amd import RandomStream, nuts, targets
    D, T = 700, 4
    mu, P, imm, q0 = problem(D)
    singles, rng_s = run(eng, problem(D), EPS, T, WIDE)
    fresh, rng_f = run(eng, problem(D), EPS, T, WIDE, fresh=True)
    assert rng_f.tobytes() == rng_s.tobytes()
    for t in range(T):
        same_bytes(fresh[t], singles[t], f"fresh copies, transition {t}")
    eng.set_option("dense_eigen", 2)
    try:
        srng = RandomStream(seeds=SEEDS)
        tgt = targets.DenseMVN(dev(mu), dev(P))
        kernel = nuts.new_kernel(srng, tgt, max_num_expansions=DEEP)
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


@gpu
def test_above_the_kernels_ceiling_the_lockstep_stage_runs(eng):
    """D = 10200 > 10176: the option changes nothing -- the bits of the lock-step stage."""
    D = 10200
    prob = problem_ar(D)
    a = run(eng, prob, EPS_AR, 1, WIDE, SHALLOW)
    b = run(eng, prob, EPS_AR, 1, LOCKSTEP, SHALLOW)
    assert a[1].tobytes() == b[1].tobytes()
    same_bytes(a[0][0], b[0][0], "D = 10200")
    assert (b[0][0]["nd"] >= 1).all()
