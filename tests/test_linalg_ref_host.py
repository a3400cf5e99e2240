"""Host-side checks of the extended-precision factorisation reference (tests/linalg_ref.py): against 50-digit
arithmetic, against the defining identity, and of the fp64 yardstick that sets the device's error bound."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import linalg_ref as lr  # noqa: E402

LD = np.longdouble


def test_longdouble_has_a_64_bit_mantissa():
    assert np.finfo(LD).nmant >= 63, "linalg_ref needs an extended-precision longdouble"


def _mp_chol_inv_t(m):
    """L^-T of m in 50-digit arithmetic, from the definitions (element by element)."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    D = m.shape[0]
    a = [[mp.mpf(float(m[i, j])) for j in range(D)] for i in range(D)]
    L = [[mp.mpf(0)] * D for _ in range(D)]
    for i in range(D):
        for j in range(i + 1):
            s = a[i][j] - sum(L[i][k] * L[j][k] for k in range(j))
            L[i][j] = mp.sqrt(s) if i == j else s / L[j][j]
    X = [[mp.mpf(0)] * D for _ in range(D)]
    for c in range(D):
        for i in range(c, D):
            s = (mp.mpf(1) if i == c else mp.mpf(0)) - sum(L[i][j] * X[j][c] for j in range(c, i))
            X[i][c] = s / L[i][i]
    return L, [[X[j][i] for j in range(D)] for i in range(D)]


def _rowwise_err_mp(got, ref, D):
    mp = pytest.importorskip("mpmath")
    return max(max(abs(mp.mpf(got[i, j].astype(str)) - ref[i][j]) for j in range(D)) / max(abs(ref[i][j]) for j in range(D))
               for i in range(D))


@pytest.mark.parametrize("kind", lr.FAMILIES)
@pytest.mark.parametrize("D", [1, 2, 5, 12])
def test_helper_against_mpmath(kind, D):
    """chol_inv_t against 50 digits, 1e-17 relative per row (longdouble: u = 5.4e-20; an fp64 helper would give 1e-16,
    and a longdouble factorisation WITHOUT the helper's refinement 1e-13 on `graded`: cond x 2^-64)."""
    mp = pytest.importorskip("mpmath")
    m = lr.family(kind, D)
    L, S = lr.chol_inv_t(m)
    Lm, Sm = _mp_chol_inv_t(m)
    eL, eS = _rowwise_err_mp(L, Lm, D), _rowwise_err_mp(S, Sm, D)
    print(f"{kind} D = {D}: L {float(eL):.3e}, L^-T {float(eS):.3e}")
    assert np.array_equal(np.triu(L, 1), np.zeros((D, D))) and np.array_equal(np.tril(S, -1), np.zeros((D, D)))
    assert eL <= mp.mpf("1e-17") and eS <= mp.mpf("1e-17"), (kind, D, float(eL), float(eS))


def test_helper_at_condition_1e12():
    """The refinement repeats until its second-order term is below rounding: four more orders of conditioning."""
    D = 8
    q, _ = np.linalg.qr(np.random.default_rng(3).normal(size=(D, D)))
    m = (q * np.logspace(0, -12, D)) @ q.T
    m = 0.5 * (m + m.T)
    L, S = lr.chol_inv_t(m)
    Lm, Sm = _mp_chol_inv_t(m)
    assert _rowwise_err_mp(L, Lm, D) <= 1e-17 and _rowwise_err_mp(S, Sm, D) <= 1e-17


@pytest.mark.parametrize("kind", lr.FAMILIES)
def test_factor_whitens_its_matrix(kind):
    """S^T a S = I in longdouble at D = 130, to 8 D u cond(a) with u = 2^-64: the factor's backward error D u |L||L^T|
    seen through S.  cond is 1e8 for `graded` and at most 9 for `well` (eigenvalues of A A^T / D lie in [0, 4], + 0.5);
    the identity is invariant under the scaling of `scaled`, which therefore has `well`'s bound (4.5e-15 would already
    fail an fp64 factor: D 2^-53 = 1.4e-14)."""
    D = 130
    m, S, _ = lr.reference(kind, D)
    R = S.T @ m.astype(LD) @ S - np.eye(D, dtype=LD)
    tol = 8 * D * 2.0 ** -64 * (1e8 if kind == "graded" else 9.0)
    print(f"{kind}: |S^T a S - I| = {float(np.abs(R).max()):.3e}, bound {tol:.3e}")
    assert np.abs(R).max() < tol


def test_only_the_lower_triangle_is_read():
    m = lr.family("well", 12).copy()
    _, S = lr.chol_inv_t(m)
    m[np.triu_indices(12, 1)] = np.nan
    _, S2 = lr.chol_inv_t(m)
    assert np.array_equal(S, S2)


def test_not_positive_definite_is_reported():
    m = lr.family("well", 5).copy()
    m[3, 3] = -1.0
    with pytest.raises(np.linalg.LinAlgError, match=r"pivot 4\)"):
        lr.chol_inv_t(m)


@pytest.mark.parametrize("kind", lr.FAMILIES)
@pytest.mark.parametrize("D", [64, 129, 194])
def test_yardstick_error_band(kind, D):
    """The fp64 LAPACK factor against the helper: a row-wise error in (0, 1e-8) -- not zero (the helper is not fp64 in
    disguise), not large (the two factor the same matrix the same way)."""
    _, _, y = lr.reference(kind, D)
    print(f"yardstick {kind} D = {D}: {y:.3e}  (bound for the device: {lr.bound(D, y):.3e})")
    assert 0.0 < y < 1e-8
