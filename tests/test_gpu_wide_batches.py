"""k_nuts_wide's element pass in batches (csrc/nuts_wide.cuh): where q lives in LDS, the reads of a batch of BR elements are
issued together, the arithmetic follows element by element and the writes come last; a batch whose BR slots all exist
takes one uniform branch, any other keeps the guard per element.  The same order -- LDS reads of a batch, then its stores
-- in the copy on accept, where an end is parked and in the output loop.  Nothing of this may change a result.

References are routes that do not run this kernel:
    standard normal, isotropic, diagonal Gaussian   the lock-step engine ("resident_nuts" 0)
    eigen instantiation (DenseMVN, "dense_eigen" 2, a supplied basis)   the lock-step eigen stage ("dense_eigen_wide" 0)
Discrete outputs and generator states identical; reals within 1e-9 relative + 1e-12 absolute, the project's parity bound
(the order of the sums differs between the routes, the arithmetic per element does not).

Shapes: for every plan <T, R> the slot counts nslots = ceil(D / T) at which the batch logic can go wrong --
    <256, 4>        D = 513 (3 slots: a partial batch only), 1024 (4)
    <256, 8>        1025 (5: one full batch + 1), 1793 (8)
    <512, 8>        2049 (5), 3585 (8)
    <512, 16, LDS>  4097 (9), 6145 (13), 8192 (16)
    <512, 20, LDS>  8193 (17), 9217 (19), 10000 (20, all full), 10176 (20, lanes past D inside a full batch)
The two pointwise kinds run at every shape; the diagonal Gaussian (batches of 2, parameters streamed from R = 16 on) and the
eigen instantiation at the first shape of the first plan and of the two LDS plans and at the last shape.

8 chains, depth limit 6, one transition: 63 leapfrogs where no U-turn ends the tree earlier, expansions to both sides
(an end parked and fetched back) and accepted sub-trajectory proposals in every case -- asserted on the reference.

The eigen cases need a basis of H = L^T P L.  At D = 513 it is numpy's eigh of H; above, eigh would take minutes on the
host, so the problem is built from its basis instead: V = plane rotations of the coordinate pairs (2 i, 2 i + 1),
lambda spread over [0.6, 1.6], H = V diag(lambda) V^T, a diagonal-valued dense metric imm = diag(l^2) and P = diag(1 / l)
H diag(1 / l).  (The kernel under test sees lambda and the rotated momentum, never V.  A basis with two entries per
column leaves the engine's acceptance check -- max |V^T V - I| <= 4.6e-14 by a D-term GEMM -- nothing to round: dense
orthogonal bases exact to 2e-15 on the host measured 4.75e-14 there at D = 8193.)  Either way the engine checks the
supplied basis against the H it forms itself and reports state 2: the caller's basis is in use."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu

RTOL, ATOL = 1e-9, 1e-12
C, DEPTH = 8, 6
SEEDS = [4100 + c for c in range(C)]
SHAPES = [513, 1024, 1025, 1793, 2049, 3585, 4097, 6145, 8192, 8193, 9217, 10000, 10176]
FEWER = [513, 4097, 8193, 10176]


@pytest.fixture(scope="module")
def eng():
    from aehmc_amd.engine import get_engine
    e = get_engine()
    yield e
    e.set_option("resident_nuts", 2)
    e.set_option("dense_eigen", 1)
    e.set_option("dense_eigen_wide", 1)
    e.set_white_basis(None)


def dev(x):
    return x if isinstance(x, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(x), device="cuda")


def host(info, upd, srng):
    s = info.state
    out = dict(q=s.position, U=s.potential_energy, g=s.potential_energy_grad, p=s.momentum,
               acc=info.acceptance_probability, nl=info.n_leapfrog, nd=info.num_doublings, turn=info.is_turning,
               div=info.is_diverging)
    out = {k: v.cpu().numpy() for k, v in out.items()}
    out["rng"] = upd[srng].cpu().numpy().view(np.uint64).copy()
    return out


def compare(new, ref):
    # the case exercises what it is meant to, judged on the reference: trees of 3 doublings or more in half the chains (a
    # chain has then turned to both sides with probability 3 / 4), one of 4 or more, moved chains, no divergence
    assert (ref["nd"] >= 3).sum() >= C // 2 and ref["nd"].max() >= 4, ref["nd"]
    assert not ref["div"].any()
    assert (ref["acc"] > 0).all()
    for k in ("nl", "nd", "turn", "div"):
        print(k, new[k].tolist())
        assert np.array_equal(new[k], ref[k]), k
    assert new["rng"].tobytes() == ref["rng"].tobytes()
    for k in ("q", "p", "g", "U", "acc"):
        err = np.abs(new[k] - ref[k]) / (ATOL + RTOL * np.abs(ref[k]))
        print(k, "worst error / bound", float(err.max()))
        np.testing.assert_allclose(new[k], ref[k], rtol=RTOL, atol=ATOL, err_msg=k)


def pointwise_case(kind, D):
    from aehmc_amd import targets
    r = np.random.default_rng(7 * D + len(kind))
    imm = 0.5 + r.random(D)
    if kind == "std":
        tgt, q0 = targets.StdNormal(), r.normal(size=(C, D))
    elif kind == "iso":
        tgt, q0 = targets.IsoGaussian(), r.normal(size=(C, D))
    else:
        mu, sigma = r.normal(size=D), 0.5 + r.random(D)
        tgt, q0 = targets.DiagGaussian(mu, sigma), mu + sigma * r.normal(size=(C, D))
    return tgt, q0, imm


def run_pointwise(eng, kind, D, resident):
    from aehmc_amd import RandomStream, nuts
    tgt, q0, imm = pointwise_case(kind, D)
    eng.set_option("resident_nuts", 2 if resident else 0)
    try:
        srng = RandomStream(seeds=SEEDS)
        kernel = nuts.new_kernel(srng, tgt, max_num_expansions=DEPTH)
        info, upd = kernel(nuts.new_state(dev(q0), tgt), 0.4 / D ** 0.25, imm)
        return host(info, upd, srng)
    finally:
        eng.set_option("resident_nuts", 2)


def eigen_case(D):
    """mu, P, imm, q0, V, lam on the device (the module's docstring)"""
    gen = torch.Generator(device="cuda").manual_seed(D)
    i = torch.arange(D, device="cuda", dtype=torch.float64)
    l = 1.0 + 0.25 * (i % 3)
    mu = torch.sin(0.37 * i)
    q0 = mu + l * torch.randn((C, D), dtype=torch.float64, device="cuda", generator=gen)
    if D < 1024:
        r = np.random.default_rng(D)
        A = r.normal(size=(D, D))
        P = np.linalg.inv(A @ A.T / D + np.eye(D))
        P = 0.5 * (P + P.T)
        L = np.diag(l.cpu().numpy())
        H = L.T @ P @ L
        lam, V = np.linalg.eigh(0.5 * (H + H.T))
        return mu, dev(P), torch.diag(l * l).contiguous(), q0, dev(V), dev(lam)
    frac = torch.remainder(i * 0.6180339887498949, 1.0)
    lam = 0.6 + frac
    even = torch.arange(0, D - 1, 2, device="cuda")
    c, s = torch.cos(0.3 + frac[even]), torch.sin(0.3 + frac[even])
    V = torch.eye(D, dtype=torch.float64, device="cuda")
    V[even, even], V[even, even + 1], V[even + 1, even], V[even + 1, even + 1] = c, -s, s, c
    H = (V * lam) @ V.T  # (two non-zero terms per entry)
    P = 0.5 * (H + H.T) / l[:, None] / l[None, :]
    return mu, (0.5 * (P + P.T)).contiguous(), torch.diag(l * l).contiguous(), q0, V.contiguous(), lam


def run_eigen(eng, case, wide):
    from aehmc_amd import RandomStream, nuts, targets
    mu, P, imm, q0, V, lam = case
    eng.set_option("dense_eigen", 2)
    eng.set_option("dense_eigen_wide", 1 if wide else 0)
    eng.set_white_basis(V, lam)
    try:
        srng = RandomStream(seeds=SEEDS)
        tgt = targets.DenseMVN(mu, P)
        kernel = nuts.new_kernel(srng, tgt, max_num_expansions=DEPTH)
        info, upd = kernel(nuts.new_state(q0, tgt), 0.15, imm)
        assert eng.white_basis_info()["state"] == 2, eng.white_basis_info()
        return host(info, upd, srng)
    finally:
        eng.set_white_basis(None)
        eng.set_option("dense_eigen", 1)
        eng.set_option("dense_eigen_wide", 1)


@gpu
@pytest.mark.parametrize("D", SHAPES)
@pytest.mark.parametrize("kind", ["std", "iso"])
def test_pointwise_batches_match_the_lockstep_engine(eng, kind, D):
    compare(run_pointwise(eng, kind, D, True), run_pointwise(eng, kind, D, False))


@gpu
@pytest.mark.parametrize("D", FEWER)
def test_diag_gaussian_batches_match_the_lockstep_engine(eng, D):
    compare(run_pointwise(eng, "diag", D, True), run_pointwise(eng, "diag", D, False))


@gpu
@pytest.mark.parametrize("D", FEWER)
def test_eigen_batches_match_the_lockstep_stage(eng, D):
    case = eigen_case(D)
    compare(run_eigen(eng, case, True), run_eigen(eng, case, False))
