"""Pareto-smoothed importance sampling, PSIS-LOO and WAIC on the device (aehmc_amd/summary.py over csrc/psis.cuh)
against the reference of tests/psis_ref.py.

The tolerance is measured, not chosen: EPS_FACTOR times the largest difference between the fp64 and the 80-bit
long-double run of the reference over the very inputs of a test, per output (figures beside EPS_FACTOR and in DESIGN.md
section 4)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import psis_ref as ps  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

# The device may differ from the fp64 reference by this many times what the reference's own rounding moves it: its
# exp / log1p / expm1 may be a couple of ulp off where numpy's are within one, and its sums run in another order.
# Observed on the MI355X (this file, -s), device - reference against eps_ref: psislw at [25664, 17] k 8.5e-15 against
# 2.4e-14, log-weights 1.3e-14 against 2.4e-13, log_mean 8.9e-16 against 3.6e-14; loo elpd_i 3.0e-14 against 6.2e-14,
# k 1.1e-14 against 1.5e-14, elpd 5.0e-14 against 8.8e-14; the small shapes k 1.9e-15 against 3.3e-16 (a factor of 6).
EPS_FACTOR = 32
N, C, D = 401, 64, 17  # R = 25664: seven chunks of the sort and no multiple of one; D: one more than a workgroup's 16
R = N * C
REFF = (1.0, 1.0, 0.3, 0.05, 4.0)  # per column, in turn: tails of 481, 878, 2150 (thetas beyond LDS) and 241 draws


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def host(t):
    return t.cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def chain_like(r, n, repeat=0.3):
    x = r.normal(size=n)
    for i in np.flatnonzero(r.random(n) < repeat):
        if i:
            x[i] = x[i - 1]
    return x


@functools.lru_cache(maxsize=None)
def ratios():
    """x [R, 17], never written to.  0, 1: normal; 2, 3: Pareto tails of shape 0.3 and 0.7; 4, 5: chain-like, about
    30 % of the draws repeat the one before; 6: 40 integers (the largest fills the tail: nothing above the cutoff);
    7: 400 integers (mass ties, ties at the cutoff); 8: a constant; 9: some -inf; 10: a NaN; 11: a +inf; 12: all
    -inf; 13: Student t; 14: log of exponential ratios (k near 0); 15: a narrow column; 16: a wide one (k above 1)."""
    r = np.random.default_rng(31337)
    x = r.normal(size=(R, D))
    x[:, 1] *= 2.0
    x[:, 2] = -0.3 * np.log(r.random(R))
    x[:, 3] = -0.7 * np.log(r.random(R))
    x[:, 4] = chain_like(r, R)
    x[:, 5] = 3.0 * chain_like(r, R) - 40.0
    x[:, 6] = r.integers(0, 40, size=R)
    x[:, 7] = r.integers(0, 400, size=R) * 0.0625
    x[:, 8] = -3.75
    x[r.choice(R, size=200, replace=False), 9] = -np.inf
    x[12345, 10] = np.nan
    x[777, 11] = np.inf
    x[:, 12] = -np.inf
    x[:, 13] = r.standard_t(4, size=R)
    x[:, 14] = np.log(-np.log(r.random(R)))
    x[:, 15] = 1e-3 * r.normal(size=R) + 700.0
    x[:, 16] = 30.0 * r.normal(size=R)
    x.setflags(write=False)
    return x


def reff_columns(n):
    return np.array([REFF[d % len(REFF)] for d in range(n)])


@functools.lru_cache(maxsize=None)
def ratios_ref():
    x, v = ratios(), values()
    return ps.psislw(x, reff_columns(D), v), ps.psislw(x, reff_columns(D), v, dtype=np.longdouble)


@functools.lru_cache(maxsize=None)
def values():
    v = np.random.default_rng(4242).normal(size=(R, D)) * 2.0
    v.setflags(write=False)
    return v


def eps_ref(a, b):
    """The largest difference between the two runs of the reference where both are finite."""
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    fin = np.isfinite(a) & np.isfinite(b)
    return float(np.abs(a[fin] - b[fin]).max()) if fin.any() else 0.0


def check(got, ref64, refld, name):
    """The NaN / inf pattern exactly, finite values within EPS_FACTOR eps_ref; prints both figures first."""
    got, ref64 = np.asarray(got, dtype=np.float64), np.asarray(ref64, dtype=np.float64)
    assert got.shape == ref64.shape, name
    fin = np.isfinite(ref64)
    eps = eps_ref(ref64, refld)
    diff = float(np.abs(got[fin] - ref64[fin]).max()) if fin.any() and np.isfinite(got[fin]).all() else np.inf
    print(f"{name}: eps_ref {eps:.3e}, device - reference {diff:.3e}, allowed {EPS_FACTOR * eps:.3e}")
    assert np.array_equal(np.isnan(got), np.isnan(ref64)), name
    assert np.array_equal(got[~fin & ~np.isnan(ref64)], ref64[~fin & ~np.isnan(ref64)]), name
    assert diff <= EPS_FACTOR * eps, (name, diff, eps)


# ---- psislw ----

def test_psislw_against_the_reference():
    from aehmc_amd import summary
    from aehmc_amd.engine import get_engine
    x = ratios()
    ref, refld = ratios_ref()
    t = dev(x).reshape(N, C, D)
    lw, k = summary.psislw(t, dev(reff_columns(D)))
    assert lw.shape == (N, C, D) and k.shape == (D,)
    _, k2, tail, mean = get_engine().summary_psis(t.reshape(R, D), dev(reff_columns(D)), dev(values()), weights=False)
    assert same_bits(k, k2)
    print("tail_len", host(tail).tolist(), "k", host(k).tolist())
    assert np.array_equal(host(tail), ref["tail_len"])
    n = ref["tail_len"].tolist()
    assert n[:4] == [481, 481, 878, 2150] and 230 <= n[4] <= 241 and 470 <= n[5] <= 481  # (ties at the cutoff stay out)
    assert n[6] == 0 and 0 < n[7] < 878 and n[8] == 0 and n[10:13] == [-1, -1, -1]
    check(host(k), ref["k"], refld["k"], "pareto_k")
    check(host(lw).reshape(R, D), ref["lw"], refld["lw"], "log_weights")
    check(host(mean), ref["log_mean"], refld["log_mean"], "log_mean")
    # a float reff, and the default
    for reff in (1.0, 0.3):
        r64, rld = ps.psislw(x[:, :6], reff), ps.psislw(x[:, :6], reff, dtype=np.longdouble)
        lw, k = summary.psislw(t[:, :, :6].contiguous(), reff)
        check(host(k), r64["k"], rld["k"], f"pareto_k, reff {reff}")
        check(host(lw).reshape(R, 6), r64["lw"], rld["lw"], f"log_weights, reff {reff}")
    assert same_bits(summary.psislw(t[:, :, 0].contiguous())[0], summary.psislw(t[:, :, :1].contiguous())[0][:, :, 0])


def test_rows_may_come_in_any_order():
    """What comes from the sorted column keeps its bits under a permutation of the rows: pareto_k, tail_len and every
    row's log-weight.  log_mean is summed along the rows: it stays within the measured tolerance of the reference."""
    from aehmc_amd.engine import get_engine
    eng = get_engine()
    t, v, reff = dev(ratios()), dev(values()), dev(reff_columns(D))
    ref, refld = ratios_ref()
    perm = torch.randperm(R, generator=torch.Generator().manual_seed(5)).cuda()
    lw, k, tail, mean = eng.summary_psis(t, reff, v)
    plw, pk, ptail, pmean = eng.summary_psis(t[perm].contiguous(), reff, v[perm].contiguous())
    assert same_bits(k, pk) and torch.equal(tail, ptail)
    assert same_bits(lw[perm], plw)
    fin = torch.isfinite(mean)
    print("log_mean, permuted - original", float((pmean[fin] - mean[fin]).abs().max()))
    check(host(pmean), ref["log_mean"], refld["log_mean"], "log_mean of the permuted rows")


def test_runs_and_tiles_give_the_same_bits():
    from aehmc_amd.engine import get_engine
    eng = get_engine()
    t, v, reff = dev(ratios()), dev(values()), dev(reff_columns(D))
    want = eng.summary_psis(t, reff, v)
    again = eng.summary_psis(t, reff, v)
    one = int(eng.lib.aehmc_summary_rank_work(R, 1))
    narrow = eng.summary_psis(t, reff, v, _work_bytes=one)          # a tile of one coordinate
    some = eng.summary_psis(t, reff, v, _work_bytes=5 * one + 256)  # tiles of 5, 5, 5 and 2
    for got in (again, narrow, some):
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]) and torch.equal(got[2], want[2])
        assert same_bits(got[3], want[3])
    # the leave-one-out form: ratios that are the negated values, without the negated copy, weights not stored
    loo_a = eng.summary_psis((-v).contiguous(), reff, v)
    for kw in ({}, {"_work_bytes": one}):
        loo_b = eng.summary_psis(None, reff, v, weights=False, **kw)
        assert loo_b[0] is None and same_bits(loo_a[1], loo_b[1]) and torch.equal(loo_a[2], loo_b[2])
        assert same_bits(loo_a[3], loo_b[3])


# ---- loo and waic ----

@functools.lru_cache(maxsize=None)
def log_lik():
    """[401, 64, 17] on the device, from torch: observations y_i ~ N(theta, s_i) under chain-like draws of theta, the
    scales s_i from 0.6 (a narrow likelihood: k above 1) to 3 (k near 0.1)."""
    g = torch.Generator().manual_seed(99)
    theta = 0.6 * torch.randn(N, C, generator=g, dtype=torch.float64)
    stay = torch.rand(N, C, generator=g, dtype=torch.float64) < 0.3
    for i in range(1, N):  # a rejected transition repeats the chain's draw
        theta[i] = torch.where(stay[i], theta[i - 1], theta[i])
    y = 1.2 * torch.randn(D, generator=g, dtype=torch.float64)
    s = torch.linspace(0.6, 3.0, D, dtype=torch.float64)
    ll = -0.5 * ((y - theta[:, :, None]) / s) ** 2 - torch.log(s) - 0.5 * np.log(2 * np.pi)
    return ll.cuda().contiguous()


def test_loo_against_the_reference():
    from aehmc_amd import summary
    ll = log_lik()
    S = R
    reff = summary.relative_eff(ll)
    assert reff.shape == (D,) and bool(((reff > 0) & torch.isfinite(reff)).all())
    print("reff", host(reff).tolist())
    summary.loo(ll)  # (whatever the first call sets up is not counted below)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    res = summary.loo(ll)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    from aehmc_amd.engine import get_engine
    scratch = int(get_engine().lib.aehmc_summary_rank_work(S, D))
    print("peak bytes over entry", peak, "one array", S * D * 8, "sort scratch", scratch)
    assert peak < S * D * 8 + scratch
    ref = ps.loo(host(ll).reshape(S, D), host(reff))
    refld = ps.loo(host(ll).reshape(S, D), host(reff), dtype=np.longdouble)
    assert res.n_samples == S and res.n_data == D and res.k_threshold == ref["k_threshold"] == 0.7
    assert res.warning == ref["warning"] and res.warning  # (the narrow likelihoods)
    assert np.array_equal(host(res.tail_len), ref["tail_len"])
    print("k", host(res.pareto_k).tolist())
    for name, got in (("elpd_i", host(res.elpd_i)), ("pareto_k", host(res.pareto_k)), ("lppd_i", host(res.lppd_i)),
                      ("elpd", res.elpd), ("se", res.se), ("p", res.p)):
        check(got, ref[name], refld[name], "loo " + name)
    same = summary.loo(ll, reff)
    assert same_bits(same.elpd_i, res.elpd_i) and same_bits(same.pareto_k, res.pareto_k) and same.elpd == res.elpd
    # the fused path against stored weights: the same sum of S positive terms in another order; either order is
    # within S 2^-53 of the exact sum, relative
    lw, k = summary.psislw(-ll, reff)
    assert same_bits(k, res.pareto_k)
    stored = torch.logsumexp((lw + ll).reshape(S, D), dim=0)
    diff = float((stored - res.elpd_i).abs().max())
    print("fused against stored weights", diff)
    assert diff <= S * 2.0 ** -53


def test_waic_against_numpy():
    from aehmc_amd import summary
    ll = log_lik()
    res = summary.waic(ll)
    ref = ps.waic(host(ll).reshape(R, D))
    refld = ps.waic(host(ll).reshape(R, D), dtype=np.longdouble)
    for name, got in (("elpd_i", host(res.elpd_i)), ("p_i", host(res.p_i)), ("lppd_i", host(res.lppd_i)),
                      ("elpd", res.elpd), ("se", res.se), ("p", res.p)):
        check(got, ref[name], refld[name], "waic " + name)
    one = summary.waic(ll[:, 0, 0].contiguous(), batched=False)  # a single chain, a single observation
    assert one.elpd_i.shape == () and one.se == 0.0


# ---- small shapes ----

def test_small_shapes():
    """R = 1, 2, 20 (four draws above the cutoff: no fit), 21 (five: a fit), 4097 (one key more than a chunk of the
    sort), with 1 and 3 columns; eps_ref over all of them together."""
    from aehmc_amd.engine import get_engine
    eng = get_engine()
    cases, got = [], []
    for rows in (1, 2, 20, 21, 4097):
        for cols in (1, 3):
            r = np.random.default_rng(rows * 10 + cols)
            x, v = r.normal(size=(rows, cols)) * 1.5, r.normal(size=(rows, cols))
            if cols == 3:
                x[:, 1] = np.round(x[:, 1])  # ties
            cases.append((ps.psislw(x, 1.0, v), ps.psislw(x, 1.0, v, dtype=np.longdouble)))
            got.append(eng.summary_psis(dev(x), None, dev(v)))
            assert np.array_equal(host(got[-1][2]), cases[-1][0]["tail_len"]), (rows, cols)
    want = {1: 0, 2: 1, 20: 4, 21: 5}
    for (ref, _), rows in zip(cases[::2], (1, 2, 20, 21)):
        assert ref["tail_len"][0] == want[rows] and (ref["k"][0] == np.inf) == (rows < 21)
    assert host(got[0][0])[0, 0] == 0.0  # one draw: log-weight 0
    for f, i in (("k", 1), ("lw", 0), ("log_mean", 3)):
        check(np.concatenate([host(g[i]).ravel() for g in got]), np.concatenate([c[0][f].ravel() for c in cases]),
              np.concatenate([c[1][f].ravel() for c in cases]), "small shapes " + f)


# ---- refusals ----

def test_refusals():
    """A refused call names its entry point; the engine still answers afterwards."""
    from aehmc_amd import summary
    from aehmc_amd.engine import EngineError, get_engine
    eng = get_engine()
    x = ratios()[:37 * 53]
    t = dev(x)
    S, cols = t.shape
    t3 = t.reshape(37, 53, cols)
    for call in (lambda a, **kw: summary.psislw(a, **kw)[0], summary.loo, summary.waic):
        with pytest.raises(ValueError, match="float64"):
            call(t3.float())
        with pytest.raises(ValueError, match="must be on"):
            call(t3.cpu())
        with pytest.raises(ValueError, match="torch tensor"):
            call(x)
    for call in (summary.psislw, summary.loo):
        with pytest.raises(ValueError, match=r"reff must be a float or a tensor of shape \(17,\)"):
            call(t3, torch.ones(cols + 1, dtype=torch.float64, device="cuda"))
        for bad in (float("nan"), float("inf"), 0.0, -1.0):
            with pytest.raises(ValueError, match="reff must be finite and positive"):
                call(t3, bad)
        with pytest.raises(ValueError, match="reff must be on"):
            call(t3, torch.ones(cols, dtype=torch.float64))
        with pytest.raises(ValueError, match="reff must be float64"):
            call(t3, torch.ones(cols, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError, match="at least 4 draws"):
        summary.loo(t3[:3].contiguous())  # (the relative efficiency is a split-chain ESS; reff=1.0 needs none)
    assert summary.loo(t3[:3].contiguous(), 1.0).n_samples == 3 * 53
    # scratch: too small, misaligned
    one = int(eng.lib.aehmc_summary_rank_work(S, 1))
    with pytest.raises(EngineError, match="aehmc_summary_psis.*one coordinate needs"):
        eng.summary_psis(t, _work_bytes=one - 256)
    work = torch.empty(one + 256, dtype=torch.uint8, device="cuda")
    k, mean = (torch.empty(cols, dtype=torch.float64, device="cuda") for _ in range(2))

    def raw(ratios_ptr, values_ptr, k_ptr, mean_ptr, work_ptr, rows=S):
        return eng.lib.aehmc_summary_psis(eng.ctx, rows, cols, ratios_ptr, None, values_ptr, None, k_ptr, None, mean_ptr,
                                          work_ptr, one, eng.stream)

    def refused(rc, text):
        assert rc != 0
        with pytest.raises(EngineError, match="aehmc_summary_psis.*" + text):
            eng._check(rc, "aehmc_summary_psis")

    refused(raw(t.data_ptr(), None, k.data_ptr(), None, work.data_ptr() + 8), "256-byte aligned")
    refused(raw(None, None, k.data_ptr(), None, work.data_ptr()), "bad arguments")
    refused(raw(t.data_ptr(), None, None, None, work.data_ptr()), "bad arguments")
    refused(raw(t.data_ptr(), None, k.data_ptr(), None, None), "bad arguments")
    refused(raw(t.data_ptr(), t.data_ptr(), k.data_ptr(), None, work.data_ptr()), "log_values and log_mean go together")
    refused(raw(t.data_ptr(), None, k.data_ptr(), mean.data_ptr(), work.data_ptr()), "log_values and log_mean go together")
    refused(raw(t.data_ptr(), None, k.data_ptr(), None, work.data_ptr(), rows=1 << 31), "R must be below 2\\^31")
    # a reff entry that is not finite and positive is that column's NaN, not an error
    reff = torch.ones(cols, dtype=torch.float64, device="cuda")
    reff[0], reff[1], reff[2], reff[3] = 0.0, float("nan"), float("inf"), -2.0
    lw, k, tail, _ = eng.summary_psis(t, reff)
    assert bool(torch.isnan(lw[:, :4]).all()) and bool(torch.isnan(k[:4]).all()) and host(tail)[:4].tolist() == [-1] * 4
    assert bool(torch.isfinite(lw[:, 4:6]).all()) and host(tail)[4] > 4
    # the engine still answers
    ref = ps.psislw(x[:, :2])
    assert np.array_equal(host(eng.summary_psis(t[:, :2].contiguous())[2]), ref["tail_len"])
