"""The shared dense-metric factor (dense_sqrt_mass in csrc/engine.hip: 64-wide blocked Cholesky, blocked triangular
inverse, transpose; O(D^3) in the fp64 MFMA GEMM, modes C -= A B^T and C = -A B^T included) against the
extended-precision reference of tests/linalg_ref.py, through the raw aehmc_metric_sqrt ABI (engine.set_metric rejects
asymmetric input and caches).  Sizes are the smallest that take each route of the factorisation:

  D <= 64         one block, no GEMM
  65              one row below the block, odd D: every product on the scalar-load 128 x 128 kernel
  66              two rows, even D: the in-place panel product on gemm_nt_f64_kernel<true> (kept off the tail kernels:
                  launch_gemm_nt_f64's in_place), the inverse's T^T on tail <4,3> with N = 2
  128, 130, 192   panels of M = 64 / 66, 2 / 128, 64 rows; the inverse's few-row products on the tail kernels
  193             three blocks with every product on the scalar-load kernels
  194             M = 130: the panel product on the small tiles with N = 64
  257, 320, 449   several row tiles in the C -= A B^T update (M = 385: 4 x 4 tiles), several block columns in the inverse

Error measure and bound: linalg_ref.rowwise_err / linalg_ref.bound -- 8 x max(the row-wise error of LAPACK's fp64
factor of the same matrix, sqrt(D) 2^-53).  A structural mistake (stale tile, dropped K remainder, wrong row stride)
shows at 1e-6 or worse."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import linalg_ref as lr  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 66, 127, 128, 129, 130, 192, 193, 194, 257, 320, 449]


@pytest.fixture(scope="module")
def eng():
    from aehmc_amd.engine import get_engine
    return get_engine()


def dev(x):
    return torch.as_tensor(np.array(x, dtype=np.float64), device="cuda")


def bits(t):
    return t.contiguous().view(torch.int64)


def factor(eng, m):
    """aehmc_metric_sqrt of the host matrix m into a NaN-filled output."""
    D = m.shape[0]
    imm = dev(m)
    out = torch.full((D, D), float("nan"), dtype=torch.float64, device="cuda")
    eng._check(eng.lib.aehmc_metric_sqrt(eng.ctx, 2, D, imm.data_ptr(), out.data_ptr(), eng.stream), "aehmc_metric_sqrt")
    return out


def check_factor(S_dev, kind, D, what=""):
    """Every element written, triangular to the bit, row-wise error within the bound; returns error / yardstick."""
    _, S_ref, yard = lr.reference(kind, D)
    S = S_dev.cpu().numpy()
    assert not np.isnan(S).any(), "elements of the output were not written (or are NaN)"
    assert not S.view(np.int64)[np.tril_indices(D, -1)].any(), "the strict lower triangle is not all-zero bits"
    err = float(lr.rowwise_err(S, S_ref).max())
    floor = max(yard, np.sqrt(D) * 2.0 ** -53)
    print(f"factor {what}{kind} D = {D}: row-wise error {err:.3e}, yardstick {yard:.3e}, ratio {err / floor:.3f} (may be 8)")
    assert err <= lr.bound(D, yard), (kind, D, err, yard)
    return err / floor


@pytest.mark.parametrize("D", SIZES)
@pytest.mark.parametrize("kind", lr.FAMILIES)
def test_factor_against_reference(eng, kind, D):
    m, _, _ = lr.reference(kind, D)
    S = factor(eng, m)
    check_factor(S, kind, D)
    assert torch.equal(bits(S), bits(factor(eng, m))), "a second call gave other bits"


@pytest.mark.parametrize("D", [194, 449])
@pytest.mark.parametrize("kind", lr.FAMILIES)
def test_gemm_route_options_keep_the_bits(eng, kind, D):
    """Every GEMM variant sums the same k-chain: the factor does not depend on which one a product is sent to."""
    m, _, _ = lr.reference(kind, D)
    base = factor(eng, m)
    check_factor(base, kind, D, "(default options) ")
    try:
        for small in range(5):
            for sk in range(3):
                eng.set_option("gemm_small_tiles", small)
                eng.set_option("streamk", sk)
                assert torch.equal(bits(factor(eng, m)), bits(base)), f"gemm_small_tiles {small}, streamk {sk}"
    finally:
        eng.set_option("gemm_small_tiles", 1)
        eng.set_option("streamk", 2)


@pytest.mark.parametrize("D", [66, 194, 257])
def test_only_the_lower_triangle_is_read(eng, D):
    """dense_cholesky: "the upper one keeps the input"; the reference factors one triangle (metrics.py:56)."""
    m, _, _ = lr.reference("well", D)
    poisoned = m.copy()
    poisoned[np.triu_indices(D, 1)] = np.nan
    S = factor(eng, poisoned)
    check_factor(S, "well", D, "(NaN above the diagonal) ")
    assert torch.equal(bits(S), bits(factor(eng, m)))


def _failing(D, p, seed=0):
    """a = L L^T of a known lower-triangular L with a diagonal >= 1, a[p, p] lowered by 2 L[p, p]^2: the pivots before p
    are untouched and pivot p is -L[p, p]^2 <= -1 up to rounding, the first to fail."""
    r = np.random.default_rng([seed, D, p])
    L = np.tril(r.normal(size=(D, D)), -1) / np.sqrt(D) + np.diag(1.0 + r.random(D))
    a = L @ L.T
    a = 0.5 * (a + a.T)
    a[p, p] -= 2.0 * L[p, p] ** 2
    return a


def _valid_factor_through_set_metric(eng, D):
    m, _, _ = lr.reference("well", D)
    eng.set_metric(m, D, force=True)
    check_factor(eng._keep["metric"][2], "well", D, "(set_metric after a failure) ")


@pytest.mark.parametrize("D,p", [(200, 0), (200, 63), (200, 64), (200, 65), (200, 191), (200, 199), (64, 63)])
def test_failed_pivot_is_reported(eng, D, p):
    from aehmc_amd.engine import EngineError
    with pytest.raises(EngineError, match=rf"not positive definite \(pivot {p + 1}\)"):
        factor(eng, _failing(D, p))
    _valid_factor_through_set_metric(eng, 194)


def test_nan_on_the_diagonal_is_a_failed_pivot(eng):
    from aehmc_amd.engine import EngineError
    m = lr.reference("well", 194)[0].copy()
    m[70, 70] = np.nan
    with pytest.raises(EngineError, match=r"not positive definite \(pivot 71\)"):
        factor(eng, m)
    _valid_factor_through_set_metric(eng, 194)
