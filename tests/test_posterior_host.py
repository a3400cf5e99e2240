"""The reference of tests/posterior_ref.py against what it restates, without a GPU: the HDI against a brute force over
all windows and against the normal distribution's own interval, the MCSE of the median and of the sd against their
asymptotic values for independent normal draws.  The margins here are the sampling error of one fixed seed, not device
tolerances."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import posterior_ref as pr  # noqa: E402


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def columns(R):
    """[R, 6]: normal draws, small integers (many tied widths), two values, zeros of both signs, a few infinities,
    a constant."""
    r = np.random.default_rng(600 + R)
    x = r.normal(size=(R, 6))
    x[:, 1] = r.integers(0, 5, size=R)
    x[:, 2] = np.where(r.random(R) < 0.4, -1.25, 3.0)
    x[:, 3] = np.where(r.random(R) < 0.5, 0.0, -0.0)
    if R > 4:
        x[:2, 4], x[2, 4] = np.inf, -np.inf
    x[:, 5] = 2.5
    return x


@pytest.mark.parametrize("R", [1, 2, 7, 64, 200])
@pytest.mark.parametrize("prob", [1e-9, 0.3, 0.5, 0.9, 0.94, 1.0])
def test_hdi_against_brute_force(R, prob):
    x = columns(R)
    lower, upper, idx = pr.hdi(x, prob)
    bl, bu, bi = pr.hdi_brute(x, prob)
    assert np.array_equal(idx, bi)  # the first of equally narrow windows
    assert np.array_equal(bits(lower), bits(bl)) and np.array_equal(bits(upper), bits(bu))
    assert not np.signbit(lower[3]) and not np.signbit(upper[3])
    m = pr.hdi_width(R, prob)
    assert 0 <= m <= R - 1
    if prob == 1e-9:  # every finite width is 0: the first finite draw (inf - inf is no width)
        fin = [0, 1, 2, 3, 5]
        assert m == 0 and np.all(idx[fin] == 0) and np.array_equal(bits(lower), bits(upper))
        assert idx[4] == (1 if R > 4 else 0)


def test_hdi_tied_widths_first_index_wins():
    x = np.array([[0.0], [1.0], [2.0], [3.0], [4.0], [4.0], [7.0], [8.0]])
    lower, upper, idx = pr.hdi(x, 0.25)  # m = 2: widths 2 2 2 1 3 4
    assert (lower[0], upper[0], idx[0]) == (3.0, 4.0, 3)
    lower, upper, idx = pr.hdi(x[:5], 0.5)  # m = 2: widths 2 2 2
    assert (lower[0], upper[0], idx[0]) == (0.0, 2.0, 0)


def test_hdi_full_mass_and_one_draw():
    x = columns(64)
    lower, upper, idx = pr.hdi(x, 1.0)
    s = np.sort(x + 0.0, axis=0)
    assert np.array_equal(bits(lower), bits(s[0])) and np.array_equal(bits(upper), bits(s[-1])) and np.all(idx == 0)
    one = np.array([[1.5, -0.0, np.nan]])
    for prob in (1e-9, 0.5, 1.0):
        lower, upper, idx = pr.hdi(one, prob)
        assert np.array_equal(bits(lower[:2]), bits([1.5, 0.0])) and np.array_equal(bits(upper[:2]), bits([1.5, 0.0]))
        assert np.isnan(lower[2]) and np.isnan(upper[2]) and list(idx) == [0, 0, -1]


def test_hdi_of_normal_draws():
    x = np.random.default_rng(12).normal(size=(25664, 1))
    lower, upper, _ = pr.hdi(x, 0.9)
    print("hdi", lower[0], upper[0])
    assert abs(lower[0] + 1.645) < 0.05 and abs(upper[0] - 1.645) < 0.05


@pytest.mark.parametrize("sigma", [1.0, 0.2])
def test_mcse_of_independent_normal_draws(sigma):
    N, C, D = 500, 8, 6
    S = N * C
    x = sigma * np.random.default_rng(13).normal(size=(N, C, D))
    res = pr.mcse_quantile(x, [0.5])
    want = 1.2533 * sigma / np.sqrt(S)
    print("mcse_median", res["mcse"][0], "asymptotic", want, "ess", res["ess"][0])
    assert np.all(np.abs(res["mcse"][0] - want) <= 0.25 * want)
    assert np.all(res["ranks"][0] < res["ranks"][1]) and np.all(res["ranks"][0] >= 0) and np.all(res["ranks"][1] < S)
    msd, _ = pr.mcse_sd(x)
    want = sigma / np.sqrt(2 * S)
    print("mcse_sd", msd, "asymptotic", want)
    assert np.all(np.abs(msd - want) <= 0.25 * want)


def test_mcse_quantile_refuses_bad_ess():
    x = np.random.default_rng(14).normal(size=(400, 3))
    x[5, 2] = np.nan
    ess = np.array([[np.nan, 0.0, 50.0], [-1.0, np.inf, 50.0], [50.0, 50.0, 50.0]])
    out, ranks, _ = pr.mcse_quantile_from_ess(x, [0.05, 0.5, 0.95], ess)
    assert np.isnan(out[:2]).all() and np.isnan(out[2, 2]) and np.isfinite(out[2, :2]).all()
    assert np.all(ranks[:, :2] == -1) and np.all(ranks[:, 2, 2] == -1) and np.all(ranks[:, 2, :2] >= 0)
