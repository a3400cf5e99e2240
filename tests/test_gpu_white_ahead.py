"""Whitened NUTS lock-step, "dense_whiten_ahead" (the default): the bookkeeping pass forms the chain's next half step
from the values it holds (k_step_white_ahead) instead of a second pass reading them back (k_step_white, option 0).
Same operations on the same bits in the same order, so every test compares option 1 against option 0 on the same
library byte for byte: all Diagnostics fields, the returned state, the generator states.

Problems as in test_gpu_dense_whiten.py: unrelated random SPD matrices and a non-zero mu.  D = 513 is the smallest
whitened size and leaves one lane's tail in the four-deep element pass, D = 700 a ragged last batch."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

C, DEPTH, T = 6, 6, 3
SEEDS = [300 + c for c in range(C)]
# chosen with the C oracle on the CPU (seeds 300..305, problem(D, D)): at 0.12 the chains of both sizes make 4 or 5
# doublings and differ in depth within a transition; at 1.1 (D = 513) five of six chains diverge in the first
# transition, five in the second, two in the third
EPS, EPS_DIVERGING = 0.12, 1.1


@pytest.fixture(scope="module")
def eng():
    from aehmc_amd.engine import get_engine
    e = get_engine()
    yield e
    e.set_option("dense_whiten_ahead", 1)
    e.set_option("dense_whiten", 1)


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda")


def spd(r, D):
    A = r.normal(size=(D, D))
    m = A @ A.T / D + np.eye(D)
    return 0.5 * (m + m.T)


@functools.lru_cache(maxsize=None)
def problem(D):
    r = np.random.default_rng(D)
    mu = r.normal(size=D)
    P = np.linalg.inv(spd(r, D))
    P = 0.5 * (P + P.T)
    imm = spd(r, D)
    return mu, P, imm, r.normal(size=(C, D))


def host(info):
    s = info.state
    out = dict(q=s.position, U=s.potential_energy, g=s.potential_energy_grad, p=s.momentum,
               acc=info.acceptance_probability, nl=info.n_leapfrog, nd=info.num_doublings, turn=info.is_turning,
               div=info.is_diverging)
    return {k: v.cpu().numpy() for k, v in out.items()}


def step_size(eps):
    from aehmc_amd import PerChain
    return PerChain(dev(np.asarray(eps))) if isinstance(eps, tuple) else eps


def make(eng, D, ahead, whiten):
    from aehmc_amd import RandomStream, nuts, targets
    mu, P, imm, q0 = problem(D)
    eng.set_option("dense_whiten", whiten)
    eng.set_option("dense_whiten_ahead", ahead)
    tgt = targets.DenseMVN(dev(mu), dev(P))
    srng = RandomStream(seeds=SEEDS)
    return srng, nuts.new_kernel(srng, tgt, max_num_expansions=DEPTH), nuts.new_state(dev(q0), tgt), dev(imm)


@functools.lru_cache(maxsize=None)
def single_calls(D, eps, ahead, whiten=1):
    """T chained kernel() calls: their Diagnostics on the host, then the generator states"""
    from aehmc_amd.engine import get_engine
    eng = get_engine()
    try:
        srng, kernel, state, imm = make(eng, D, ahead, whiten)
        infos = []
        for _ in range(T):
            info, upd = kernel(state, step_size(eps), imm)
            infos.append(host(info))
            state = info.state._replace(momentum=None)
        return infos, upd[srng].cpu().numpy().view(np.uint64).copy()
    finally:
        eng.set_option("dense_whiten", 1)
        eng.set_option("dense_whiten_ahead", 1)


def one_sample_call(eng, D, eps, ahead):
    try:
        srng, kernel, state, imm = make(eng, D, ahead, 1)
        samples, info, acc_hist, div_hist = kernel.sample(state, step_size(eps), imm, T)
        out = host(info)
        out.update(samples=samples.cpu().numpy(), acc_hist=acc_hist.cpu().numpy(), div_hist=div_hist.cpu().numpy())
        return out, kernel._nuts["holder"]["rng"].cpu().numpy().view(np.uint64).copy()
    finally:
        eng.set_option("dense_whiten_ahead", 1)


def same_bytes(a, b, what=""):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k)
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


@pytest.mark.parametrize("D", [513, 700])
def test_ahead_equals_second_pass_bytewise(eng, D):
    """Three chained transitions, as three kernel() calls and as sample(3) (the carry is taken in both): option 1 equals
    option 0 byte for byte.  Some chain makes >= 4 doublings and chains finish at different depths, so chains turn
    round (the fallback pass), go on in the same direction, and leave the compacted rows at different steps; with more
    than 50 direction draws a run without a change of direction has probability below 2^-50."""
    on, rng_on = single_calls(D, EPS, 1)
    off, rng_off = single_calls(D, EPS, 0)
    nd = np.stack([h["nd"] for h in off])
    assert nd.max() >= 4 and any(len(np.unique(row)) >= 2 for row in nd), nd
    assert nd.sum() > 50, nd
    assert rng_on.tobytes() == rng_off.tobytes()
    for t in range(T):
        same_bytes(on[t], off[t], f"transition {t}")
    s_on, srng_on = one_sample_call(eng, D, EPS, 1)
    s_off, srng_off = one_sample_call(eng, D, EPS, 0)
    assert srng_on.tobytes() == srng_off.tobytes() == rng_off.tobytes()
    same_bytes(s_on, s_off, "sample")
    for t in range(T):  # (and sample(3) is the three single calls)
        assert s_on["samples"][t].tobytes() == off[t]["q"].tobytes(), t


def test_ahead_diverging_chains(eng):
    """A step size at which chains diverge (the work done ahead of a chain that ends is discarded, non-finite values
    included): option 1 equals option 0 byte for byte, and the discrete outputs are those of "dense_whiten" 0."""
    D = 513
    on, rng_on = single_calls(D, EPS_DIVERGING, 1)
    off, rng_off = single_calls(D, EPS_DIVERGING, 0)
    plain, rng_plain = single_calls(D, EPS_DIVERGING, 1, 0)
    div = np.stack([h["div"] for h in off])
    assert div.any() and not div.all(), div
    assert rng_on.tobytes() == rng_off.tobytes() == rng_plain.tobytes()
    for t in range(T):
        same_bytes(on[t], off[t], f"transition {t}")
        for k in ("nl", "nd", "turn", "div"):
            assert np.array_equal(on[t][k], plain[t][k]), (t, k)


def test_ahead_per_chain_step_sizes(eng):
    """Per-chain step sizes (the whitened route takes them): option 1 equals option 0 byte for byte."""
    D = 700
    eps = tuple(0.08 + 0.03 * c for c in range(C))
    on, rng_on = single_calls(D, eps, 1)
    off, rng_off = single_calls(D, eps, 0)
    assert len(np.unique(np.stack([h["nl"] for h in off]))) >= 3
    assert rng_on.tobytes() == rng_off.tobytes()
    for t in range(T):
        same_bytes(on[t], off[t], f"transition {t}")


def test_ahead_workspace_size_unchanged(eng):
    """The half-step momentum takes a vector the whitened mode left unused: the workspace does not grow."""
    from aehmc_amd import targets
    D = 513
    mu, P, imm, _ = problem(D)
    eng.set_target(targets.DenseMVN(dev(mu), dev(P)), D)
    eng.set_metric(dev(imm), D)
    sizes = []
    for ahead in (1, 0, 1):
        eng.set_option("dense_whiten_ahead", ahead)
        sizes.append([eng.lib.aehmc_workspace_bytes(eng.ctx, c, d) for c, d in ((C, DEPTH), (4096, 10), (1, 1))])
    assert sizes[0] == sizes[1] == sizes[2] and min(sizes[0]) > 0, sizes
