"""What the rank-normalised diagnostics (aehmc_amd/summary.py over csrc/rank.cuh) promise without a GPU: the formula
of Phi^-1 that the device evaluates, restated in numpy (tests/rank_ref.py), against scipy and a 40-digit reference;
argument validation before the engine is asked for; the fields of RankSummary."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rank_ref as rr  # noqa: E402

torch = pytest.importorskip("torch")

S = 200_000
NDTRI_RTOL = 1e-13  # the formula's relative error is near 1e-16, scipy against the 40-digit reference is 2.8e-16


def grid(k):
    return (np.asarray(k, dtype=np.float64) - 0.375) / (S + 0.25)


def test_ndtri_formula_against_scipy():
    """Every argument a run of S pooled draws can produce, and the smallest and largest of any S < 2^31."""
    from scipy.special import ndtri
    for s in (S, 4, 5, 2**31 - 1):
        p = (np.arange(1, min(s, S) + 1, dtype=np.float64) - 0.375) / (s + 0.25)
        p = np.concatenate([p, (s - np.arange(0.0, min(s, 1000)) - 0.375) / (s + 0.25)])
        got, want = rr.ndtri_as241(p), ndtri(p)
        rel = np.abs(got - want) / np.where(want != 0, np.abs(want), 1.0)
        print("S", s, "max rel err against scipy", rel.max())
        assert np.all(rel <= NDTRI_RTOL)
    assert rr.ndtri_as241(np.array([0.5]))[0] == 0.0


def test_ndtri_formula_against_40_digits():
    """Both tails and the centre of the grid (k - 3/8) / (S + 1/4), S = 200 000, against sqrt(2) erfinv(2 p - 1)."""
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.dps = 40
    k = np.concatenate([np.arange(1, 121), np.arange(S // 2 - 60, S // 2 + 61), np.arange(S - 119, S + 1),
                        np.linspace(1, S, 240).astype(np.int64)])
    p = grid(k)
    got = rr.ndtri_as241(p)
    want = [mpmath.sqrt(2) * mpmath.erfinv(2 * mpmath.mpf(float(v)) - 1) for v in p]
    rel = np.array([float(abs((mpmath.mpf(float(g)) - w) / w)) for g, w in zip(got, want)])
    print("max rel err against 40 digits", rel.max())
    assert np.all(rel <= NDTRI_RTOL)


def every(names):
    from aehmc_amd import summary
    return [getattr(summary, n) for n in names]


ALL = ("ranks", "rank_normalize", "bulk_ess", "rank_rhat", "rank_summarize")
SPLIT = ("bulk_ess", "rank_rhat", "rank_summarize")
ACOV = ("bulk_ess", "rank_summarize")


def test_arguments_are_checked_before_the_engine():
    """Every refusal is a ValueError and comes before get_engine(): it is the same with and without a GPU."""
    from aehmc_amd import summary
    good = torch.zeros(8, 3, 2, dtype=torch.float64)
    for f in every(ALL):
        with pytest.raises(ValueError, match="torch tensor"):
            f(np.zeros((8, 3, 2)))
        with pytest.raises(ValueError, match="float64"):
            f(good.float())
        with pytest.raises(ValueError, match="contiguous"):
            f(good.transpose(0, 1))
        with pytest.raises(ValueError, match=r"\[N, C\] or \[N, C, D\]"):
            f(torch.zeros(8, dtype=torch.float64))
        with pytest.raises(ValueError, match=r"\[N, C\] or \[N, C, D\]"):
            f(torch.zeros(8, 3, 2, 2, dtype=torch.float64))
        with pytest.raises(ValueError, match=r"\[N\] / \[N, D\]"):
            f(good, batched=False)
        with pytest.raises(ValueError, match="at least one draw"):
            f(torch.zeros(0, 3, 2, dtype=torch.float64))
    for f in every(SPLIT):
        with pytest.raises(ValueError, match="at least 4 draws"):
            f(torch.zeros(3, 5, 2, dtype=torch.float64))
        with pytest.raises(ValueError, match="at least 4 draws"):
            f(torch.zeros(3, dtype=torch.float64), batched=False)
    long = torch.zeros(2 * summary.MAX_ACOV_ROWS, 1, dtype=torch.float64)
    for f in every(ACOV):
        with pytest.raises(ValueError, match="segment length \\+ lags"):
            f(long)
        with pytest.raises(ValueError, match="max_lag must be at least 1"):
            f(good, max_lag=0)
    with pytest.raises(ValueError, match="within \\[0, 1\\]"):
        summary.rank_summarize(good, prob=1.5)


def test_rank_summary_fields():
    from aehmc_amd import summary
    assert summary.RankSummary._fields == ("rhat", "rhat_bulk", "rhat_folded", "ess_bulk", "ess_tail", "lag_truncated",
                                           "num_draws", "num_chains")
