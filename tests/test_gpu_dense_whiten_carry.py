"""Whitened dense MVN, the carry ("dense_whiten_carry", the default) and the triangular hint of the chain-batched GEMM.

Carry: after a whitened transition the engine holds the returned (q, U, g) next to the whitened pair (z, H z) it came
from; a chain that enters the next whitened call with exactly that state keeps the pair, every other chain is mapped in
from q as with the option at 0.  So a carried chain's z is not rounded through q = mu + L z, z = L^-1 (q - mu): against
"dense_whiten_carry" 0 the discrete outputs and the generator states are identical and the reals agree to the
project's GPU parity tolerance (rtol 1e-9, atol 1e-12), and wherever nothing is carried the results are bitwise equal.

Hint: skipping K-tiles of exact zeros changes no bit for finite A; the profiled flop count is what a launch executes."""
import ctypes as ct

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-9, 1e-12


@pytest.fixture(scope="module")
def eng():
    from aehmc_amd.engine import get_engine
    e = get_engine()
    yield e
    e.set_option("dense_whiten_carry", 1)
    e.set_option("dense_whiten", 1)
    e.profile_enable(False)


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda")


def spd(r, D):
    A = r.normal(size=(D, D))
    m = A @ A.T / D + np.eye(D)
    return 0.5 * (m + m.T)


def problem(D, seed):
    r = np.random.default_rng(seed)
    mu = r.normal(size=D)
    P = np.linalg.inv(spd(r, D))
    return r, mu, 0.5 * (P + P.T), spd(r, D)


def host(info):
    s = info.state
    out = dict(q=s.position, U=s.potential_energy, g=s.potential_energy_grad, p=s.momentum,
               acc=info.acceptance_probability, nl=info.n_leapfrog, nd=getattr(info, "num_doublings", None),
               turn=info.is_turning, div=info.is_diverging)
    return {k: v.cpu().numpy() for k, v in out.items() if v is not None}


DISCRETE = ("nl", "nd", "turn", "div")


def bitwise(a, b, rows=slice(None)):
    for k in a:
        assert np.array_equal(a[k][rows], b[k][rows], equal_nan=True), k


class Chain:
    """One sampler on one problem: transitions one at a time, with room for something in between."""

    def __init__(self, eng, mod, tgt, imm, q0, seeds, eps, extra, carry, max_exp=5):
        from aehmc_amd import RandomStream, nuts
        self.eng, self.mod, self.imm, self.eps, self.extra, self.carry = eng, mod, imm, eps, extra, carry
        eng.set_option("dense_whiten", 1)
        eng.set_option("dense_whiten_carry", carry)
        self.srng = RandomStream(seeds=seeds)
        self.kernel = (mod.new_kernel(self.srng, tgt, max_num_expansions=max_exp) if mod is nuts
                       else mod.new_kernel(self.srng, tgt))
        self.state = mod.new_state(dev(q0), tgt)
        self.upd = None

    def step(self):
        self.eng.set_option("dense_whiten_carry", self.carry)
        info, self.upd = self.kernel(self.state, self.eps, self.imm, *self.extra)
        self.state = info.state._replace(momentum=None)
        return host(info)

    def rng(self):
        return self.upd[self.srng].cpu().numpy().view(np.uint64).copy()


def samplers():
    from aehmc_amd import hmc, nuts
    return ((nuts, ()), (hmc, (9,)))


@pytest.mark.timeout(900)
def test_carry_against_no_carry(eng):
    """NUTS and HMC, D = 700, four chained transitions: generator states and discrete outputs identical, reals within
    (1e-9, 1e-12); the first transition, where nothing is carried yet, bitwise equal."""
    from aehmc_amd import targets
    D, C, eps = 700, 6, 0.12
    r, mu, P, imm = problem(D, 21)
    q0 = r.normal(size=(C, D))
    tgt, immd = targets.DenseMVN(dev(mu), dev(P)), dev(imm)
    seeds = [900 + c for c in range(C)]
    for mod, extra in samplers():
        runs = []
        for carry in (1, 0):
            ch = Chain(eng, mod, tgt, immd, q0, seeds, eps, extra, carry)
            runs.append(([ch.step() for _ in range(4)], ch.rng()))
        (on, rng_on), (off, rng_off) = runs
        assert np.array_equal(rng_on, rng_off)
        bitwise(on[0], off[0])
        for a, b in zip(on, off):
            for k in a:
                if k in DISCRETE:
                    assert np.array_equal(a[k], b[k]), k
                else:
                    err = np.abs(a[k] - b[k]) / (ATOL + RTOL * np.abs(b[k]))
                    print(f"{mod.__name__} {k}: max error / tolerance = {err.max():.3g}")
                    np.testing.assert_allclose(a[k], b[k], rtol=RTOL, atol=ATOL, err_msg=k)


@pytest.mark.timeout(900)
def test_carry_is_taken(eng):
    """The second of two chained transitions executes exactly the two input products (z0 = L^-1 (q0 - mu), H z0 on C
    rows) fewer with the carry than without: a count of flops, not a timing.  (Six chains: the few-row kernels, which
    count 2 M N K.)"""
    from aehmc_amd import targets
    D, C, eps = 640, 6, 0.12
    r, mu, P, imm = problem(D, 22)
    q0 = r.normal(size=(C, D))
    tgt, immd = targets.DenseMVN(dev(mu), dev(P)), dev(imm)
    seeds = [910 + c for c in range(C)]
    for mod, extra in samplers():
        flops, second = {}, {}
        for carry in (1, 0):
            ch = Chain(eng, mod, tgt, immd, q0, seeds, eps, extra, carry)
            ch.step()
            eng.profile_enable(True)
            try:
                second[carry] = ch.step()
                flops[carry] = eng.profile_read()[2]
            finally:
                eng.profile_enable(False)
        for k in DISCRETE:
            if k in second[1]:
                assert np.array_equal(second[1][k], second[0][k]), k
        print(f"{mod.__name__}: flops carry 1 = {flops[1]:.0f}, carry 0 = {flops[0]:.0f}")
        assert flops[0] - flops[1] == 2 * (2.0 * C * D * D)


@pytest.mark.timeout(900)
def test_carry_edited_rows(eng):
    """Positions of some chains edited in place between two transitions (U and dU/dq re-evaluated with torch): those
    chains equal the "dense_whiten_carry" 0 run bit for bit, the others the carried run."""
    from aehmc_amd import targets
    D, C, eps = 700, 8, 0.12
    r, mu, P, imm = problem(D, 23)
    q0 = r.normal(size=(C, D))
    mud, Pd, immd = dev(mu), dev(P), dev(imm)
    tgt = targets.DenseMVN(mud, Pd)
    seeds = [920 + c for c in range(C)]
    sub, rest = [1, 2, 6], [0, 3, 4, 5, 7]
    shift = dev(r.normal(size=(len(sub), D)) * 0.1)

    def edit(ch):
        s = ch.state
        s.position[sub] += shift  # in place: the same tensors go back into the kernel
        res = s.position[sub] - mud
        g = res @ Pd
        s.potential_energy_grad[sub] = g
        s.potential_energy[sub] = 0.5 * (res * g).sum(dim=1)

    for mod, extra in samplers():
        out = {}
        for name, carry, edited in (("carried", 1, False), ("fresh", 0, True), ("mixed", 1, True)):
            ch = Chain(eng, mod, tgt, immd, q0, seeds, eps, extra, carry)
            ch.step()
            if edited:
                edit(ch)
            out[name] = ch.step()
        bitwise(out["mixed"], out["fresh"], sub)
        bitwise(out["mixed"], out["carried"], rest)


@pytest.mark.timeout(900)
def test_carry_record_is_dropped(eng):
    """Between two chained transitions: a new_state call, a call with another chain count, a new workspace,
    "dense_whiten" toggled.  Each leaves nothing to carry: the second transition equals the "dense_whiten_carry" 0 run
    bit for bit.  (A forced re-bind: test_carry_follows_content_not_arrays.)"""
    from aehmc_amd import nuts, targets
    D, C, eps = 700, 6, 0.12
    r, mu, P, imm = problem(D, 24)
    q0 = r.normal(size=(C, D))
    tgt, immd = targets.DenseMVN(dev(mu), dev(P)), dev(imm)
    seeds = [930 + c for c in range(C)]
    keep = []

    def new_state(ch):
        eng.new_state(dev(q0))

    def other_c(ch):
        Chain(eng, ch.mod, tgt, immd, q0[:4], seeds[:4], eps, ch.extra, 1).step()

    def new_workspace(ch):
        keep.append(eng._ws)  # (kept alive: the next buffer is another one)
        eng._ws = None

    def toggle(ch):
        eng.set_option("dense_whiten", 0)
        eng.set_option("dense_whiten", 1)

    for mod, extra in samplers():
        ref = Chain(eng, mod, tgt, immd, q0, seeds, eps, extra, 0)
        ref.step()
        want = ref.step()
        for between in (new_state, other_c, new_workspace, toggle):
            ch = Chain(eng, mod, tgt, immd, q0, seeds, eps, extra, 1)
            ch.step()
            between(ch)
            got = ch.step()
            for k in want:
                assert np.array_equal(got[k], want[k]), (mod.__name__, between.__name__, k)
    keep.clear()


@pytest.mark.timeout(900)
def test_carry_follows_content_not_arrays(eng):
    """Results depend on what the bound arrays hold, not on which arrays hold it: a caller who passes a fresh copy of the
    same inverse mass matrix with every call (the engine binds, and forms the operator, again each time) gets bit for
    bit what one binding gives -- the carried run.  After a forced re-bind to an edited matrix nothing is carried: the
    transition equals the "dense_whiten_carry" 0 run."""
    from aehmc_amd import targets
    D, C, eps = 700, 6, 0.12
    r, mu, P, imm = problem(D, 26)
    q0 = r.normal(size=(C, D))
    tgt, immd = targets.DenseMVN(dev(mu), dev(P)), dev(imm)
    seeds = [950 + c for c in range(C)]
    for mod, extra in samplers():
        one = Chain(eng, mod, tgt, immd, q0, seeds, eps, extra, 1)
        want = [one.step() for _ in range(3)]
        ch = Chain(eng, mod, tgt, immd.clone(), q0, seeds, eps, extra, 1)
        for t in range(3):
            ch.imm = immd.clone()
            bitwise(ch.step(), want[t])
        out = {}
        for carry in (1, 0):
            m = immd.clone()
            ch = Chain(eng, mod, tgt, m, q0, seeds, eps, extra, carry)
            ch.step()
            m.mul_(1.05)
            eng.set_target(tgt, D, force=True)
            eng.set_metric(m, D, force=True)
            out[carry] = ch.step()
        bitwise(out[1], out[0])


# ---------------------------------------------------------------------------------------- triangular hint
BN, BK = 256, 16  # tile of the kernel that honours the hint


def tri_flops(M, N, K, tri):
    """What a hinted launch of the 128 x 256 stream-K kernel executes: per column tile the K-tiles that are not wholly
    inside B's zero triangle."""
    nk = (K + BK - 1) // BK
    total = 0
    for tn in range((N + BN - 1) // BN):
        lo = min(tn * BN // BK, nk - 1) if tri == 2 else 0
        hi = min(((tn + 1) * BN + BK - 1) // BK, nk) if tri == 1 else nk
        total += min(BN, N - tn * BN) * (min(hi * BK, K) - lo * BK)
    return 2.0 * M * total


@pytest.mark.timeout(900)
@pytest.mark.parametrize("n", [2064, 4096, 10000])
def test_triangular_hint_is_bitwise_and_counted(eng, n):
    """aehmc_gemm_nt_tri against aehmc_gemm_nt: random finite A with 4096 rows, random lower / upper triangular B
    (N = K = n; 2064 is not a multiple of 256), all rows and a compacted row list.  Outputs bitwise equal; the counted
    flops are those of the executed K-tiles, fewer than 2 M N K: the kernel that honours the hint is the one that ran."""
    M = 4096
    g = torch.Generator(device="cuda").manual_seed(n)
    A = torch.randn(M, n, dtype=torch.float64, device="cuda", generator=g)
    full = torch.randn(n, n, dtype=torch.float64, device="cuda", generator=g)
    rows = torch.sort(torch.randperm(M, device="cuda", generator=g)[:2900]).values.to(torch.int32)
    idx = torch.zeros(M, dtype=torch.int32, device="cuda")
    idx[:rows.numel()] = rows
    cnt = torch.tensor([rows.numel()], dtype=torch.int32, device="cuda")
    for tri, B in ((1, torch.tril(full)), (2, torch.triu(full))):
        B = B.contiguous()
        want = eng.gemm_nt(A, B)
        for ri, nr, m in ((None, None, M), (idx, cnt, rows.numel())):
            out = {}
            for hint in (tri, 0):
                out[hint] = torch.full((M, n), -7.0, dtype=torch.float64, device="cuda")
                eng.profile_enable(True)
                try:
                    eng.gemm_nt_tri(A, B, hint, ri, nr, out=out[hint])
                    fl = eng.profile_read()[2]
                finally:
                    eng.profile_enable(False)
                expect = tri_flops(m, n, n, hint) if hint else 2.0 * m * n * n
                print(f"n = {n}, tri = {hint}, rows = {m}: flops {fl:.0f} of {2.0 * m * n * n:.0f}")
                assert fl == expect
                assert not hint or fl < 0.62 * 2.0 * m * n * n
            assert torch.equal(out[tri], out[0])
            if ri is None:
                assert torch.equal(out[tri], want)
            else:
                live = rows.long()
                assert torch.equal(out[tri][live], want[live])
                mask = torch.ones(M, dtype=torch.bool, device="cuda")
                mask[live] = False
                assert bool((out[tri][mask] == -7.0).all())
        del want, out


@pytest.mark.timeout(900)
def test_hint_needs_an_exactly_triangular_sqrt_mass(eng):
    """white_prepare gives the hint only where the bound sqrt_mass is triangular to the bit.  The engine's own factor
    is: an HMC transition at 2048 x 4096 then counts the triangular K-tiles for L^-1, L^-T and L.  The same factor with
    -0.0 below the diagonal (bound through the C ABI) is not: L^-1 and L^-T run in full, and every result is the same
    bit for bit."""
    from aehmc_amd import _lib, hmc, targets
    D, C, eps = 4096, 2048, 0.05
    r = np.random.default_rng(25)
    mu = r.normal(size=D)
    d = 1.0 + r.random(D)
    A = r.normal(size=(D, 8)) / 4
    P = np.diag(d) + A @ A.T
    B2 = r.normal(size=(D, 8)) / 4
    imm = np.diag(1.0 + r.random(D)) + B2 @ B2.T
    q0 = r.normal(size=(C, D))
    tgt, immd = targets.DenseMVN(dev(mu), dev(0.5 * (P + P.T))), dev(0.5 * (imm + imm.T))
    seeds = [940 + c for c in range(C)]
    L = 2
    full = 2.0 * C * D * D

    def one():
        ch = Chain(eng, hmc, tgt, immd, q0, seeds, eps, (L,), 0)
        eng.profile_enable(True)
        try:
            out = ch.step()
            return out, eng.profile_read()[2]
        finally:
            eng.profile_enable(False)

    eng.set_target(tgt, D, force=True)
    eng.set_metric(immd, D, force=True)
    exact, fl_exact = one()
    # z0 and H z0, L leapfrogs, the fresh gradient: full; L^-1 and L: lower triangular; L^-T: upper
    assert fl_exact == (2 + L) * full + 2 * tri_flops(C, D, D, 1) + tri_flops(C, D, D, 2)
    _, t, sm = eng._keep["metric"]
    sm2 = sm.clone()
    low = torch.tril(torch.ones(D, D, dtype=torch.bool, device="cuda"), diagonal=-1)
    assert bool((sm2[low] == 0).all())
    sm2[low] = -0.0
    c = _lib.CMetric(ndim=2, D=D, imm=t.data_ptr(), sqrt_mass=sm2.data_ptr())
    try:
        eng._check(eng.lib.aehmc_set_metric(eng.ctx, ct.byref(c)), "aehmc_set_metric")
        inexact, fl_inexact = one()
    finally:
        eng.set_metric(immd, D, force=True)
    print(f"flops: exact factor {fl_exact:.0f}, -0.0 below the diagonal {fl_inexact:.0f}")
    assert fl_inexact - fl_exact == 2 * full - tri_flops(C, D, D, 1) - tri_flops(C, D, D, 2)
    bitwise(exact, inexact)
