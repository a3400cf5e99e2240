"""Highest-density intervals, the MCSE of quantiles and of the sd, the beta quantile and the posterior table on the
device (aehmc_amd/summary.py over csrc/posterior.cuh) against the reference of tests/posterior_ref.py."""
import ctypes as ct
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import posterior_ref as pr  # noqa: E402
import summary_ref as sr  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

RTOL = 1e-9  # the project's parity tolerance
# Exact ranks at the largest shape tested need S * err < DELTA / 2: 1e-6 / (2 * 25664) = 1.9e-11
BETA_ATOL = 1e-11
# (N, C, D, layout) of tests/test_gpu_quantiles.py: R = N C in {1, 15, 1961, 25664, 16384, 129}; D = 17 and 65 straddle
# workgroups of 16 coordinates; R = 16384 and 25664 are 4 and 7 chunks of the sort, so windows cross chunk boundaries
# and m exceeds a chunk
SHAPES = [(1, 1, 1, "N"), (5, 3, 2, "NCD"), (37, 53, 17, "NCD"), (401, 64, 100, "NCD"), (4, 4096, 1, "NC"),
          (129, 1, 65, "ND")]
HDI_PROBS = (1e-9, 0.5, 0.9, 0.94, 1.0)
MCSE_CASES = [(8, 2, 3, 0.0), (40, 8, 17, 0.5), (100, 16, 65, 0.9), (401, 64, 100, 0.3)]
MCSE_PROBS = (0.05, 0.5, 0.95)
TABLE_FIELDS = ("mean", "sd", "hdi_lower", "hdi_upper", "mcse_mean", "mcse_sd", "ess_bulk", "ess_tail", "rhat")


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def host(t):
    return t.cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def laid_out(x, N, C, D, layout):
    """x [N C, D] on the device in the layout's view, with what the calls need to read it."""
    view = {"N": (N,), "NC": (N, C), "ND": (N, D), "NCD": (N, C, D)}[layout]
    shape = {"N": (), "NC": (), "ND": (D,), "NCD": (D,)}[layout]
    return dev(x).reshape(view), shape, dict(batched=layout in ("NC", "NCD"))


@functools.lru_cache(maxsize=None)
def draws(N, C, D):
    """x [R, D]: normal draws with a location and a scale per coordinate; never written to."""
    r = np.random.default_rng(9000 + N + C + D)
    x = r.normal(size=(N * C, D)) * (0.5 + r.random(D)) + r.normal(size=D) * 3.0
    x.setflags(write=False)
    return x


def close(got, want, name=""):
    """Within RTOL relative where the reference is finite, NaN and inf where it has them."""
    assert got.shape == want.shape, name
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), name
    assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), name
    rel = np.abs(got[fin] - want[fin]) / np.where(want[fin] != 0, np.abs(want[fin]), 1.0)
    print(name, "max rel err", rel.max() if rel.size else 0.0)
    assert np.all(rel <= RTOL), (name, rel.max())


# ---- the highest-density interval ----

@pytest.mark.parametrize("N,C,D,layout", SHAPES)
def test_hdi_to_the_bit(N, C, D, layout):
    from aehmc_amd import summary
    from aehmc_amd.engine import get_engine
    x = draws(N, C, D)
    t, shape, kw = laid_out(x, N, C, D, layout)
    eng = get_engine()
    for prob in HDI_PROBS:
        lower, upper, idx = pr.hdi(x, prob)
        lo, hi = summary.hdi(t, prob, **kw)
        assert lo.shape == shape and hi.shape == shape
        assert np.array_equal(bits(host(lo)).reshape(D), bits(lower)), prob
        assert np.array_equal(bits(host(hi)).reshape(D), bits(upper)), prob
        rl, ru, ri = eng.summary_hdi(t.reshape(N * C, D), prob)
        assert np.array_equal(host(ri), idx), prob
        assert np.array_equal(bits(host(rl)), bits(lower)) and np.array_equal(bits(host(ru)), bits(upper)), prob
        if prob == 1e-9:
            assert np.all(idx == 0) and np.array_equal(bits(lower), bits(upper))


def hard_values():
    """[37 * 53, 17]: coordinate 0 constant, 1 two values, 2 the negation of 3, 4 magnitudes from 1e-310 to 1e300 with
    both signs, 5 a few +-inf, 6 zeros of both signs, 7 small integers (many tied widths), 8 a few values many times
    each; the rest as drawn."""
    R = 37 * 53
    r = np.random.default_rng(4444)
    x = r.normal(size=(R, 17))
    x[:, 0] = 2.5
    x[:, 1] = np.where(np.arange(R) % 3 == 0, -1.25, 3.0)
    r.shuffle(x[:, 1])
    x[:, 2] = -x[:, 3]
    x[:, 4] = r.choice([-1.0, 1.0], size=R) * 10.0 ** r.uniform(-310, 300, size=R)
    x[:4, 4] = [1e-310, -1e-310, 1e300, -1e300]
    x[r.choice(R, size=7, replace=False), 5] = [np.inf, np.inf, np.inf, -np.inf, -np.inf, np.inf, -np.inf]
    x[:, 6] = np.where(r.random(R) < 0.5, 0.0, -0.0)
    x[:, 7] = r.integers(0, 40, size=R)
    x[:, 8] = r.choice([-2.0, -0.0, 0.0, 1e-320, 7.0], size=R)
    return x


def test_hdi_hard_values_to_the_bit():
    from aehmc_amd.engine import get_engine
    x = hard_values()
    R = x.shape[0]
    assert np.any((np.abs(x[:, 4]) < 2.3e-308) & (x[:, 4] != 0)), "no denormal among the magnitudes"
    assert np.signbit(x[:, 6]).any() and not np.signbit(x[:, 6]).all()
    eng = get_engine()
    y = x.copy()
    y[1234, 9] = np.nan
    other = [d for d in range(17) if d != 9]
    for prob in HDI_PROBS + (0.003, 0.999):
        lower, upper, idx = pr.hdi(x, prob)
        gl, gu, gi = (host(v) for v in eng.summary_hdi(dev(x), prob))
        assert np.array_equal(gi, idx), (prob, gi, idx)
        assert np.array_equal(bits(gl), bits(lower)) and np.array_equal(bits(gu), bits(upper)), prob
        assert gl[0] == 2.5 and gu[0] == 2.5 and gi[0] == 0
        assert not np.signbit(gl[6]) and not np.signbit(gu[6]) and gl[6] == 0.0 and gu[6] == 0.0 and gi[6] == 0
        # one NaN: its coordinate is NaN, NaN, -1; every other coordinate keeps its bits
        pl, pu, pi = (host(v) for v in eng.summary_hdi(dev(y), prob))
        assert np.isnan(pl[9]) and np.isnan(pu[9]) and pi[9] == -1
        assert np.array_equal(bits(pl[other]), bits(gl[other])) and np.array_equal(bits(pu[other]), bits(gu[other]))
        assert np.array_equal(pi[other], gi[other])


def test_hdi_tile_independence_and_determinism():
    from aehmc_amd.engine import get_engine
    N, C, D = 37, 53, 17
    x = draws(N, C, D)
    S = N * C
    t = dev(x)
    eng = get_engine()
    one = int(eng.lib.aehmc_summary_rank_work(S, 1))
    assert one < int(eng.lib.aehmc_summary_rank_work(S, D))
    for prob in (0.5, 0.94):
        want = eng.summary_hdi(t, prob)
        again = eng.summary_hdi(t, prob)
        for nbytes in (one, 5 * one):
            got = eng.summary_hdi(t, prob, _work_bytes=nbytes)
            for g, a, w in zip(got, again, want):
                assert same_bits(a, w) if w.dtype == torch.float64 else torch.equal(a, w)
                assert same_bits(g, w) if w.dtype == torch.float64 else torch.equal(g, w)
    # several chunks a column and several tiles at once
    big = draws(401, 64, 100)
    tb = dev(big)
    one = int(eng.lib.aehmc_summary_rank_work(401 * 64, 1))
    lower, upper, idx = pr.hdi(big, 0.9)
    gl, gu, gi = eng.summary_hdi(tb, 0.9, _work_bytes=7 * one + 256)
    assert np.array_equal(bits(host(gl)), bits(lower)) and np.array_equal(bits(host(gu)), bits(upper))
    assert np.array_equal(host(gi), idx)


# ---- the beta quantile ----

def beta_grid():
    rows = [(p, e * prob + 1.0, e * (1.0 - prob) + 1.0) for e in 10.0 ** np.arange(0.0, 7.01, 0.5)
            for prob in (0.0, 0.01, 0.05, 0.5, 0.95, 0.99, 1.0) for p in (pr.P_LO, pr.P_HI)]
    return np.array(rows).T.copy()


def test_beta_quantile_against_scipy():
    """The bound is derived (BETA_ATOL above), not measured; observed on an MI355X: 2.14e-14."""
    from scipy.special import betaincinv
    from aehmc_amd.engine import get_engine
    p, a, b = beta_grid()
    assert p.size == 15 * 7 * 2
    want = betaincinv(a, b, p)
    got = host(get_engine().beta_quantile(dev(p), dev(a), dev(b)))
    err = np.abs(got - want)
    k = int(np.argmax(err))
    print("beta quantile: max abs err", err.max(), "at p, a, b =", p[k], a[k], b[k])
    assert np.all(np.isfinite(got)) and np.all((got > 0) & (got < 1))
    assert np.all(err <= BETA_ATOL), (err.max(), p[k], a[k], b[k])


def test_beta_quantile_outside_its_domain():
    from aehmc_amd.engine import get_engine
    nan, inf = np.nan, np.inf
    p = np.array([0.0, 1.0, -0.1, 1.1, nan, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5])
    a = np.array([2.0, 2.0, 2.0, 2.0, 2.0, 0.5, 2.0, nan, 2.0, inf, 2.0])
    b = np.array([3.0, 3.0, 3.0, 3.0, 3.0, 3.0, 0.9, 3.0, nan, 3.0, 3.0])
    got = host(get_engine().beta_quantile(dev(p), dev(a), dev(b)))
    assert np.isnan(got[:-1]).all() and 0.0 < got[-1] < 1.0


# ---- the MCSE of a quantile ----

@functools.lru_cache(maxsize=None)
def mcse_case(N, C, D, phi):
    """(x [N, C, D], the reference's dict): AR(1) draws with a location and a scale per coordinate; never written
    to."""
    rng = np.random.default_rng(7100 + N + C + D)
    loc = rng.normal(size=D) * 3.0
    scale = 0.5 + rng.random(D)
    x = sr.ar1(rng, N, C, D, phi, loc, scale)
    x.setflags(write=False)
    return x, pr.mcse_quantile(x, MCSE_PROBS)


@pytest.mark.parametrize("N,C,D,phi", MCSE_CASES)
def test_mcse_quantile(N, C, D, phi):
    from aehmc_amd import summary
    from aehmc_amd.engine import get_engine
    x, ref = mcse_case(N, C, D, phi)
    print("reference ess from", ref["ess"].min(), "to", ref["ess"].max())
    assert not ref["unsure"].any(), "a scaled beta quantile lies within 1e-6 of an integer: pick another seed"
    assert not ref["near"].any(), "a deciding pair sum of the reference lies within 1e-9 of zero: pick another seed"
    t = dev(x)
    # (i) the kernel alone, on the reference's own ess: the ranks exactly, the result to the bit
    out, ranks = get_engine().summary_quantile_mcse(t.reshape(N * C, D), list(MCSE_PROBS), dev(ref["ess"]))
    assert np.array_equal(host(ranks), ref["ranks"])
    assert np.array_equal(bits(host(out)), bits(ref["mcse"]))
    # (ii) end to end, with the ess of the device
    got = host(summary.mcse_quantile(t, MCSE_PROBS))
    close(got, ref["mcse"], "mcse_quantile")
    med = summary.mcse_median(t)
    assert med.shape == (D,) and same_bits(med, summary.mcse_quantile(t, 0.5))
    close(host(med), ref["mcse"][1], "mcse_median")


def test_mcse_quantile_layouts():
    """One chain, no coordinate axis: the shapes of `quantiles`."""
    from aehmc_amd import summary
    x, ref = mcse_case(40, 8, 17, 0.5)
    t = dev(x)
    a = summary.mcse_quantile(t[:, :, 3].contiguous(), MCSE_PROBS)
    assert a.shape == (3,)
    assert same_bits(a, summary.mcse_quantile(t, MCSE_PROBS)[:, 3])
    one = t[:, 0].contiguous()  # [N, D]: one chain
    b = summary.mcse_quantile(one, 0.5, batched=False)
    assert b.shape == (17,)
    assert same_bits(b, summary.mcse_quantile(one.reshape(40, 1, 17), 0.5))
    assert summary.mcse_quantile(one[:, 2].contiguous(), (0.5, 0.9), batched=False).shape == (2,)


def test_mcse_quantile_bad_ess_and_nan():
    from aehmc_amd.engine import get_engine
    x, ref = mcse_case(40, 8, 17, 0.5)
    S, D = 320, 17
    eng = get_engine()
    ess = ref["ess"].copy()
    ess[0, 0], ess[1, 1], ess[2, 2], ess[0, 3] = np.nan, 0.0, -1.0, np.inf
    y = x.reshape(S, D).copy()
    y[77, 5] = np.nan
    want, wranks, _ = pr.mcse_quantile_from_ess(y, MCSE_PROBS, ess)
    out, ranks = eng.summary_quantile_mcse(dev(y), list(MCSE_PROBS), dev(ess))
    out, ranks = host(out), host(ranks)
    for q, d in ((0, 0), (1, 1), (2, 2), (0, 3), (0, 5), (1, 5), (2, 5)):
        assert np.isnan(out[q, d]) and ranks[0, q, d] == -1 and ranks[1, q, d] == -1
    assert np.array_equal(bits(out), bits(want)) and np.array_equal(ranks, wranks)
    assert np.isfinite(out).sum() == 3 * D - 7
    # tile independence and determinism of the kernel
    one = int(eng.lib.aehmc_summary_rank_work(S, 1))
    for nbytes in (None, one, 5 * one):
        o2, r2 = eng.summary_quantile_mcse(dev(y), list(MCSE_PROBS), dev(ess), _work_bytes=nbytes)
        assert np.array_equal(bits(host(o2)), bits(out)) and np.array_equal(host(r2), ranks)


# ---- mcse_sd and the table ----

@pytest.mark.parametrize("N,C,D,phi", [(40, 8, 17, 0.5), (401, 64, 100, 0.3)])
def test_mcse_sd_and_table(N, C, D, phi):
    from aehmc_amd import summary
    x, _ = mcse_case(N, C, D, phi)
    ref = pr.table(x, prob=0.9)
    assert not ref["near"].any(), "a deciding pair sum of the reference lies within 1e-9 of zero: pick another seed"
    t = dev(x)
    msd = summary.mcse_sd(t)
    assert msd.shape == (D,)
    close(host(msd), ref["mcse_sd"], "mcse_sd")
    tab = summary.table(t, prob=0.9)
    assert tab._fields == TABLE_FIELDS + ("num_draws", "num_chains")
    assert (tab.num_draws, tab.num_chains) == (N, C)
    for name in TABLE_FIELDS:
        close(host(getattr(tab, name)), ref[name], name)
    # the columns that existed are those of the direct calls, the new ones those of theirs
    s, r = summary.summarize(t), summary.rank_summarize(t)
    lower, upper = summary.hdi(t, 0.9)
    for got, want in ((tab.mean, s.mean), (tab.sd, s.sd), (tab.mcse_mean, s.mcse), (tab.ess_bulk, r.ess_bulk),
                      (tab.ess_tail, r.ess_tail), (tab.rhat, r.rhat), (tab.hdi_lower, lower), (tab.hdi_upper, upper),
                      (tab.mcse_sd, msd)):
        assert same_bits(got, want)


# ---- refusals ----

def test_refusals():
    """A refused call names its entry point; the engine still answers afterwards."""
    from aehmc_amd import summary
    from aehmc_amd.engine import EngineError, get_engine
    eng = get_engine()
    x = draws(37, 53, 17)
    t = dev(x)
    S, D = t.shape
    t3 = t.reshape(37, 53, 17)
    for prob in (0.0, 1.0000001, -0.5, float("nan")):
        with pytest.raises(ValueError, match="prob"):
            summary.hdi(t3, prob)
        with pytest.raises(EngineError, match="aehmc_summary_hdi.*prob"):
            eng.summary_hdi(t, prob)
        with pytest.raises(ValueError, match="prob"):
            summary.table(t3, prob=prob)
    with pytest.raises(ValueError, match="at most 64 probs"):
        summary.mcse_quantile(t3, [i / 100.0 for i in range(65)])
    ess = torch.full((65, D), 100.0, dtype=torch.float64, device="cuda")
    with pytest.raises(EngineError, match="aehmc_summary_quantile_mcse.*at most 64"):
        eng.summary_quantile_mcse(t, [i / 100.0 for i in range(65)], ess)
    with pytest.raises(EngineError, match="aehmc_summary_quantile_mcse.*outside"):
        eng.summary_quantile_mcse(t, [0.5, 1.5], ess[:2].contiguous())
    with pytest.raises(ValueError, match="probs"):
        summary.mcse_quantile(t3, 1.5)
    # scratch: too small, misaligned
    one = int(eng.lib.aehmc_summary_rank_work(S, 1))
    with pytest.raises(EngineError, match="aehmc_summary_hdi.*one coordinate needs"):
        eng.summary_hdi(t, 0.9, _work_bytes=one - 256)
    with pytest.raises(EngineError, match="aehmc_summary_quantile_mcse.*one coordinate needs"):
        eng.summary_quantile_mcse(t, [0.5], ess[:1].contiguous(), _work_bytes=one - 256)
    work = torch.empty(one + 256, dtype=torch.uint8, device="cuda")
    lower, upper = (torch.empty(D, dtype=torch.float64, device="cuda") for _ in range(2))
    out = torch.empty(1, D, dtype=torch.float64, device="cuda")
    half = (ct.c_double * 1)(0.5)
    rc = eng.lib.aehmc_summary_hdi(eng.ctx, S, D, t.data_ptr(), 0.9, lower.data_ptr(), upper.data_ptr(), None,
                                   work.data_ptr() + 8, one, eng.stream)
    assert rc != 0
    with pytest.raises(EngineError, match="aehmc_summary_hdi.*256-byte aligned"):
        eng._check(rc, "aehmc_summary_hdi")
    rc = eng.lib.aehmc_summary_quantile_mcse(eng.ctx, S, D, 1, t.data_ptr(), half, ess.data_ptr(), out.data_ptr(), None,
                                             work.data_ptr() + 8, one, eng.stream)
    assert rc != 0
    with pytest.raises(EngineError, match="aehmc_summary_quantile_mcse.*256-byte aligned"):
        eng._check(rc, "aehmc_summary_quantile_mcse")
    # null pointers
    for args in ((None, lower.data_ptr(), upper.data_ptr()), (t.data_ptr(), None, upper.data_ptr()),
                 (t.data_ptr(), lower.data_ptr(), None)):
        rc = eng.lib.aehmc_summary_hdi(eng.ctx, S, D, args[0], 0.9, args[1], args[2], None, work.data_ptr(), one,
                                       eng.stream)
        assert rc != 0
        with pytest.raises(EngineError, match="aehmc_summary_hdi.*bad arguments"):
            eng._check(rc, "aehmc_summary_hdi")
    rc = eng.lib.aehmc_summary_hdi(eng.ctx, S, D, t.data_ptr(), 0.9, lower.data_ptr(), upper.data_ptr(), None, None, one,
                                   eng.stream)
    assert rc != 0
    for args in ((None, half, ess.data_ptr(), out.data_ptr()), (t.data_ptr(), None, ess.data_ptr(), out.data_ptr()),
                 (t.data_ptr(), half, None, out.data_ptr()), (t.data_ptr(), half, ess.data_ptr(), None)):
        rc = eng.lib.aehmc_summary_quantile_mcse(eng.ctx, S, D, 1, args[0], args[1], args[2], args[3], None,
                                                 work.data_ptr(), one, eng.stream)
        assert rc != 0
        with pytest.raises(EngineError, match="aehmc_summary_quantile_mcse.*bad arguments"):
            eng._check(rc, "aehmc_summary_quantile_mcse")
    rc = eng.lib.aehmc_beta_quantile(eng.ctx, 4, None, lower.data_ptr(), lower.data_ptr(), upper.data_ptr(), eng.stream)
    assert rc != 0
    with pytest.raises(EngineError, match="aehmc_beta_quantile.*bad arguments"):
        eng._check(rc, "aehmc_beta_quantile")
    assert eng.lib.aehmc_summary_hdi(eng.ctx, 1 << 31, D, t.data_ptr(), 0.9, lower.data_ptr(), upper.data_ptr(), None,
                                     work.data_ptr(), one, eng.stream) != 0
    # draws on the wrong device, too few draws for split chains
    cpu = torch.as_tensor(x).reshape(37, 53, 17)
    for call in (lambda: summary.hdi(cpu), lambda: summary.mcse_quantile(cpu, 0.5), lambda: summary.mcse_sd(cpu),
                 lambda: summary.table(cpu)):
        with pytest.raises(ValueError, match="must be on"):
            call()
    with pytest.raises(ValueError, match="at least 4 draws"):
        summary.mcse_quantile(t3[:3].contiguous(), 0.5)
    # the engine still answers
    lower_ref, upper_ref, _ = pr.hdi(x, 0.9)
    lo, hi = summary.hdi(t3)
    assert np.array_equal(bits(host(lo)), bits(lower_ref)) and np.array_equal(bits(host(hi)), bits(upper_ref))
