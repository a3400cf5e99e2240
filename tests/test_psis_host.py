"""The reference of tests/psis_ref.py against what it restates, without a GPU: its tie rule against the plain argsort
version (ArviZ's psislw), the generalised-Pareto fit on ratios of known shape, PSIS-LOO against the closed form of a
normal model, and the edge cases of the definition.  The margins here are the sampling error of one fixed seed, not
device tolerances."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import psis_ref as ps  # noqa: E402


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def chain_like(R, seed, repeat=0.3):
    """[R] normal draws in which about ``repeat`` of the entries repeat the one before, as rejected transitions do."""
    r = np.random.default_rng(seed)
    x = r.normal(size=R)
    for i in np.flatnonzero(r.random(R) < repeat):
        if i:
            x[i] = x[i - 1]
    return x


@pytest.mark.parametrize("R", [21, 64, 257, 4096])
def test_tie_rule_is_the_plain_version_without_ties(R):
    r = np.random.default_rng(100 + R)
    x = np.stack([r.normal(size=R), 2.0 * r.standard_t(3, size=R), -0.7 * np.log(r.random(R))], axis=1)
    v = r.normal(size=x.shape)
    a, b = ps.psislw(x, v=v), ps.psislw(x, v=v, tie_rule=False)
    assert np.array_equal(a["tail_len"], b["tail_len"]) and np.all(a["tail_len"] > 4)
    for f in ("lw", "k", "log_mean"):
        assert np.array_equal(bits(a[f]), bits(b[f])), f


@pytest.mark.parametrize("R", [64, 257, 4096])
def test_tie_rule_keeps_the_sums_of_every_tie_order(R):
    """With ties the plain version depends on the order an argsort gives them; its sum of weights and its LOO sum do
    not, and the tie rule gives those same sums: tied draws have one v, and the rule preserves sum exp over a group."""
    r = np.random.default_rng(200 + R)
    ll = np.stack([chain_like(R, 300 + R), np.round(2.0 * chain_like(R, 301 + R)), r.integers(-30, 31, size=R) * 0.125],
                  axis=1)
    want = ps.psislw(-ll, v=ll)
    assert np.all(want["tail_len"] > 4) and np.all(np.isfinite(want["k"]))
    np.testing.assert_allclose(np.exp(want["lw"]).sum(axis=0), 1.0, rtol=0, atol=1e-13)
    seen = set()
    for trial in range(8):
        got = ps.psislw(-ll, v=ll, tie_rule=False, rng=np.random.default_rng(trial))
        seen.add(bits(got["lw"]).tobytes())
        assert np.array_equal(got["tail_len"], want["tail_len"])
        assert np.array_equal(bits(got["k"]), bits(want["k"]))  # (the fit sees the sorted tail only)
        np.testing.assert_allclose(np.exp(got["lw"]).sum(axis=0), 1.0, rtol=0, atol=1e-13)
        np.testing.assert_allclose(got["log_mean"], want["log_mean"], rtol=0, atol=1e-12)
        # a function of the multiset: sorted, the plain weights differ from the rule's only inside tie groups
        assert np.all(np.abs(np.sort(got["lw"], axis=0) - np.sort(want["lw"], axis=0)).max(axis=0) < 1.0)
    assert len(seen) > 1  # (the plain version did depend on the order)
    perm = r.permutation(R)
    again = ps.psislw(-ll[perm], v=ll[perm])
    # (numpy's pairwise sum of the normaliser follows the row order: equal to rounding, not to the bit)
    np.testing.assert_allclose(again["lw"], want["lw"][perm], rtol=0, atol=1e-13)
    assert np.array_equal(bits(again["k"]), bits(want["k"]))


@pytest.mark.parametrize("k", [0.1, 0.5, 0.9])
def test_known_pareto_shape(k):
    """Ratios u^-k, u uniform, have a Pareto tail of shape k exactly.  The estimate from the 425 tail draws has a
    standard deviation near (1 + k) / sqrt(425), 0.05 to 0.09, and the prior pulls it towards 0.5: the margin of 0.1
    holds for this seed (the estimates are 0.114, 0.515 and 0.911), not for every one."""
    u = np.random.default_rng(0).random(20000)
    r = ps.psislw((-k * np.log(u))[:, None])
    print("k", k, "estimated", r["k"][0], "tail", r["tail_len"][0])
    assert r["tail_len"][0] == ps.tail_size(20000) == 425
    assert abs(r["k"][0] - k) < 0.1


def test_loo_of_a_normal_mean_against_the_closed_form():
    """y_i ~ N(mu, 1), flat prior: mu | y ~ N(ybar, 1/n), and the leave-one-out predictive density of y_i is
    N(ybar_-i, 1 + 1/(n - 1)).  With independent exact posterior draws the importance ratios r = 1 / p(y_i | mu) have,
    for d = y_i - ybar and s2 = 1/n, E r^2 / (E r)^2 = (1 - s2) / sqrt(1 - 2 s2) exp(d^2 (1 / (1 - 2 s2) - 1 / (1 - s2)))
    (Gaussian integrals), so the log of their mean over S draws has the standard error sqrt((that - 1) / S): 0.001 to
    0.005 here.  The margin is 5 of them; PSIS only lowers the variance of the plain estimator, and its bias is far
    below that at k < 0.5."""
    n, S = 50, 8000
    r = np.random.default_rng(77)
    y = r.normal(size=n) + 0.3
    mu = y.mean() + r.normal(size=S) / np.sqrt(n)
    ll = -0.5 * (y[None, :] - mu[:, None]) ** 2 - 0.5 * np.log(2 * np.pi)
    res = ps.loo(ll)
    loo_mean = (y.sum() - y) / (n - 1)
    var = 1.0 + 1.0 / (n - 1)
    exact = -0.5 * (y - loo_mean) ** 2 / var - 0.5 * np.log(2 * np.pi * var)
    d2, s2 = (y - y.mean()) ** 2, 1.0 / n
    rel = (1 - s2) / np.sqrt(1 - 2 * s2) * np.exp(d2 * (1 / (1 - 2 * s2) - 1 / (1 - s2))) - 1
    se = np.sqrt(rel / S)
    err = np.abs(res["elpd_i"] - exact)
    print("max |elpd_i - exact|", err.max(), "max in standard errors", (err / se).max(), "se", se.min(), se.max(),
          "max k", res["pareto_k"].max())
    assert np.all(res["pareto_k"] < 0.5) and not res["warning"]
    assert np.all(err <= 5 * se)
    # (the same mu for every i: the errors may be fully correlated)
    assert abs(res["elpd"] - exact.sum()) <= 5 * np.sqrt((se ** 2).sum()) * np.sqrt(n)
    bound = 5 * np.sqrt((se ** 2).sum()) * np.sqrt(n)
    lppd = -0.5 * d2 / (1 + s2) - 0.5 * np.log(2 * np.pi * (1 + s2))  # the posterior predictive density, N(ybar, 1 + 1/n)
    p_exact = (lppd - exact).sum()
    w = ps.waic(ll)
    print("p_loo", res["p"], "exact", p_exact, "p_waic", w["p"], "elpd_loo", res["elpd"], "elpd_waic", w["elpd"])
    # one parameter; the lppd's own sampling error is below that of the LOO terms
    assert 0.8 < p_exact < 1.3 and abs(res["p"] - p_exact) <= 2 * bound
    # WAIC and LOO differ in terms of order 1 / n^2 per observation
    assert abs(w["elpd"] - res["elpd"]) <= 2 * bound and abs(w["p"] - p_exact) <= 2 * bound


def test_small_columns():
    r = np.random.default_rng(5)
    for R, n in ((1, 0), (2, 1), (20, 4)):
        x = r.normal(size=(R, 1))
        res = ps.psislw(x, v=x)
        assert res["tail_len"][0] == n and res["k"][0] == np.inf
        want = x[:, 0] - x.max()
        want = want - np.log(np.exp(want).sum())  # only normalised
        assert np.array_equal(bits(res["lw"][:, 0]), bits(want))
    assert ps.psislw(np.array([[3.0]]))["lw"][0, 0] == 0.0
    x = r.normal(size=(21, 1))
    res = ps.psislw(x)
    assert ps.tail_size(21) == 5 and res["tail_len"][0] == 5 and np.isfinite(res["k"][0])
    assert np.exp(res["lw"]).sum() == pytest.approx(1.0, abs=1e-14)


def test_degenerate_columns():
    R = 200
    r = np.random.default_rng(6)
    x = r.normal(size=(R, 6))
    x[:, 0] = 1.25                      # a constant: nothing lies above the cutoff
    x[r.choice(R, 9, replace=False), 1] = -np.inf  # weight 0
    x[17, 2] = np.nan
    x[18, 3] = np.inf
    x[:, 4] = -np.inf
    res = ps.psislw(x, v=np.zeros_like(x))
    assert res["tail_len"][0] == 0 and res["k"][0] == np.inf
    assert np.array_equal(bits(res["lw"][:, 0]), bits(np.full(R, -np.log(np.float64(R)))))
    assert res["tail_len"][1] > 4 and np.isfinite(res["k"][1])
    assert np.all(res["lw"][~np.isfinite(x[:, 1]), 1] == -np.inf) and np.isfinite(res["lw"][np.isfinite(x[:, 1]), 1]).all()
    for d in (2, 3, 4):
        assert np.isnan(res["lw"][:, d]).all() and np.isnan(res["k"][d]) and res["tail_len"][d] == -1
        assert np.isnan(res["log_mean"][d])
    assert res["tail_len"][5] > 4
    np.testing.assert_allclose(res["log_mean"][[0, 1, 5]], 0.0, atol=1e-13)  # v = 0: the log of the weights' sum


def test_reff_sets_the_tail():
    R = 4096  # 3 sqrt(R) = 192, R / 5 = 819.2
    assert ps.tail_size(R) == 192
    assert ps.tail_size(R, 0.3) == int(np.ceil(3 * np.sqrt(R / 0.3))) == 351
    assert ps.tail_size(R, 4.0) == 96
    assert ps.tail_size(R, 1e-3) == 820 and ps.tail_size(R, 1e-300) == 820  # the fifth of the draws at most
    assert ps.tail_size(1) == 0 and ps.tail_size(2) == 1 and ps.tail_size(20) == 4 and ps.tail_size(21) == 5
    x = np.random.default_rng(7).normal(size=(R, 3))
    res = ps.psislw(x, reff=np.array([0.3, 1.0, 4.0]))
    assert list(res["tail_len"]) == [351, 192, 96]
    for bad in (0.0, -1.0, np.inf, np.nan):
        res = ps.psislw(x[:, :1], reff=bad)
        assert res["tail_len"][0] == -1 and np.isnan(res["k"][0]) and np.isnan(res["lw"]).all()


def test_long_double_agrees():
    """The computation is well conditioned: fp64 and 80-bit long double agree to a few 1e-15."""
    for R in (64, 257, 4096):
        x = np.stack([chain_like(R, 900 + R), np.random.default_rng(R).normal(size=R) * 2.0], axis=1)
        a, b = ps.psislw(x), ps.psislw(x, dtype=np.longdouble)
        assert np.array_equal(a["tail_len"], b["tail_len"])
        dk = np.abs(a["k"] - b["k"]).max()
        dl = np.abs(a["lw"] - b["lw"]).max()
        print(R, "k", float(dk), "lw", float(dl))
        assert dk < 1e-13 and dl < 1e-13
