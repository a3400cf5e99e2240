"""The streaming WAIC fold (csrc/pointwise.cuh) as tests/waic_ref.py restates it, against exact arithmetic from the same
doubles: the allowances of waic_ref hold at part boundaries, for a column whose variance is 10^-18 of its squared mean,
for terms that underflow, and however the rows are cut into update calls; non-finite draws behave as in summary.waic."""
import numpy as np
import pytest

import waic_ref as wr

SIZES = [wr.PART - 1, wr.PART + 1, 3 * wr.PART + 5]
NAMES = ["well_scaled", "well_scaled_2", "offset_1e6", "spread_700", "inf_first", "inf_middle", "nan"]


def columns(S, seed=0):
    r = np.random.default_rng(seed)
    x = np.empty((S, len(NAMES)))
    x[:, 0] = -3.0 + 2.0 * r.normal(size=S)
    x[:, 1] = -0.5 * r.chisquare(3, size=S) - 1.2
    x[:, 2] = -1e6 + 1e-3 * r.normal(size=S)      # kappa about 10^9: a sum-of-squares formula has no digit left
    x[:, 3] = -700.0 * r.random(S)                # exp(l - max) underflows for most terms
    x[:, 4] = x[:, 0]
    x[0, 4] = -np.inf
    x[:, 5] = x[:, 1]
    x[S // 2, 5] = -np.inf
    x[:, 6] = x[:, 0]
    x[S // 3, 6] = np.nan
    return x


@pytest.fixture(scope="module")
def references():
    return {S: (columns(S), wr.exact(columns(S))) for S in SIZES}


@pytest.mark.parametrize("cut", [1, 7, None], ids=["cut1", "cut7", "whole"])
@pytest.mark.parametrize("S", SIZES)
def test_fold_against_exact_arithmetic(references, S, cut):
    x, (lppd, p, kappa) = references[S]
    f = wr.Fold(x.shape[1])
    step = S if cut is None else cut
    for r0 in range(0, S, step):
        f.update(x[r0:r0 + step])
    assert f.n == S
    got_lppd, got_p = f.result()
    tol_lppd, tol_p = wr.allowances(S, p, kappa)
    fin = slice(0, 4)
    print(f"S={S} cut={cut} lppd error / allowance", np.abs(got_lppd - lppd)[:6] / tol_lppd,
          "p error / allowance", (np.abs(got_p - p) / tol_p)[fin])
    assert np.all(np.abs(got_lppd[:6] - lppd[:6]) <= tol_lppd)
    assert np.all(np.abs(got_p[fin] - p[fin]) <= tol_p[fin])
    # non-finite draws: -inf adds nothing to the sum and makes p NaN; a NaN makes the observation NaN; neighbours untouched
    assert np.isnan(got_p[4]) and np.isnan(got_p[5]) and np.isfinite(got_lppd[4]) and np.isfinite(got_lppd[5])
    assert np.isnan(got_lppd[6]) and np.isnan(got_p[6])


def test_sum_of_squares_fails_where_the_fold_does_not(references):
    """the column at -10^6 +- 10^-3: the textbook formula is off by more than its whole value"""
    x, (_, p, kappa) = references[SIZES[-1]]
    col, S = x[:, 2], x.shape[0]
    naive = (np.sum(col * col) - S * np.mean(col) ** 2) / (S - 1)
    assert kappa[2] > 1e8 and abs(naive - p[2]) > p[2]


def test_merge_is_the_part_merge(references):
    """two accumulators merged in order: within the same allowances, and exactly the fold when the first holds whole parts"""
    S = SIZES[-1]
    x, (lppd, p, kappa) = references[S]
    whole = wr.Fold(x.shape[1]).update(x)
    cutat = 3 * wr.PART
    a, b = wr.Fold(x.shape[1]).update(x[:cutat]), wr.Fold(x.shape[1]).update(x[cutat:])
    a.merge(b)
    for u, v in zip(a.state, whole.state):  # (the tail is one part: merging it is what the fold did)
        assert np.array_equal(u, v, equal_nan=True)
    a, b = wr.Fold(x.shape[1]).update(x[:100]), wr.Fold(x.shape[1]).update(x[100:])
    got_lppd, got_p = a.merge(b).result()
    tol_lppd, tol_p = wr.allowances(S, p, kappa)
    assert np.all(np.abs(got_lppd[:4] - lppd[:4]) <= tol_lppd) and np.all(np.abs(got_p[:4] - p[:4]) <= tol_p[:4])


def test_one_draw_and_all_minus_infinity():
    f = wr.Fold(2).update(np.array([[-1.5, -np.inf]]))
    lppd, p = f.result()
    assert lppd[0] == -1.5 and lppd[1] == -np.inf and np.isnan(p).all()  # (one draw: 0 / 0, as torch.var gives)
