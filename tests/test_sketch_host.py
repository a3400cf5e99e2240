"""The numpy restatement of the streaming quantile sketch (tests/sketch_ref.py) pinned on the CPU: the slot it selects
holds the exact order statistic, a resolved estimate lies within one bin width of numpy.quantile, the default grid
resolves the central 90 % of normal draws -- what tests/test_gpu_sketch.py relies on --, and the library exports the two
entry points."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sketch_ref as sk  # noqa: E402

EPS = np.finfo(np.float64).eps


def heavy(kind):
    """[37 * 53, 17] draws with tails the default grid does not hold: Student-t with 3 and 1.5 degrees of freedom,
    log-normal."""
    r = np.random.default_rng(1500)
    R, D = 37 * 53, 17
    if kind == "t3":
        return r.standard_t(3.0, size=(R, D))
    if kind == "t1.5":
        return r.standard_t(1.5, size=(R, D)) * (0.5 + r.random(D)) + r.normal(size=D)
    return np.exp(r.normal(size=(R, D)) * 1.5)


def cases():
    for N, C, D in sk.SHAPES:
        yield f"normal-{N}-{C}-{D}", sk.draws(N, C, D)
    for kind in ("t3", "t1.5", "lognormal"):
        yield kind, heavy(kind)


CASES = dict(cases())


@pytest.mark.parametrize("B", sk.BINS)
@pytest.mark.parametrize("name", list(CASES))
def test_selected_slot_holds_the_order_statistic_and_the_bound_holds(name, B):
    """The slot selected for rank k = floor(p (R - 1)) is the slot of np.sort(x)[k] (binning is monotone); where
    resolved, |estimate - np.quantile| <= width + 4 eps max(|lo|, |hi|) (both neighbouring order statistics lie in the
    slots the two positions lie in, and the interpolation between the positions weighs them as the exact rule weighs the
    order statistics; the rounding of lo + width * c is a few eps of the grid's largest edge)."""
    x = CASES[name]
    R, D = x.shape
    lo, hi = sk.fit_grid(x)
    cnt = sk.counts(x, lo, hi, B)
    assert cnt.sum(axis=1).tolist() == [R] * D
    est, res, slot_k = sk.quantiles(cnt, lo, hi, B, sk.PROBS)
    s = np.sort(x, axis=0)
    for i, p in enumerate(sk.PROBS):
        k = int(math.floor(p * (R - 1)))
        assert np.array_equal(slot_k[i], sk.slots(s[k], lo, hi, B)), (name, B, p)
    width, _ = sk.widths(lo, hi, B)
    err = np.abs(est - np.quantile(x, sk.PROBS, axis=0))
    bound = width + 4 * EPS * np.maximum(np.abs(lo), np.abs(hi))
    print(name, B, "resolved", res.mean(), "worst error / width where resolved",
          np.max(np.where(res, err / width, 0.0)))
    assert np.all(err[res] <= np.broadcast_to(bound, err.shape)[res])
    assert res.any()


@pytest.mark.parametrize("N,C,D", sk.SHAPES)
def test_default_grid_resolves_the_central_mass_of_normal_draws(N, C, D):
    x = sk.draws(N, C, D)
    lo, hi = sk.fit_grid(x)
    assert np.all(np.isfinite(lo) & np.isfinite(hi) & (lo < hi))
    probs = [p for p in sk.PROBS if 0.05 <= p <= 0.95]
    for B in sk.BINS:
        _, res, _ = sk.quantiles(sk.counts(x, lo, hi, B), lo, hi, B, probs)
        assert res.all(), (B, np.argwhere(~res))


def test_edge_values_and_the_nan_slot():
    """grid (0, 64) in 64 bins: width 1, everything exact."""
    B = 64
    v = np.array([float(i) for i in range(64)] + [64.0, np.inf, -0.0, -1e-300, -np.inf, np.nan])
    got = sk.slots(v[:, None], np.zeros(1), np.full(1, 64.0), B)[:, 0]
    assert got.tolist() == list(range(1, 65)) + [65, 65, 1, 0, 0, 66]
    cnt = sk.counts(np.stack([v, np.arange(70.0) % 64], axis=1), np.zeros(2), np.full(2, 64.0), B)
    est, res, _ = sk.quantiles(cnt, np.zeros(2), np.full(2, 64.0), B, (0.25, 0.5))
    assert np.isnan(est[:, 0]).all() and not res[:, 0].any()
    assert np.isfinite(est[:, 1]).all() and res[:, 1].all()


def test_library_exports_the_sketch_entry_points():
    from aehmc_amd import _lib
    lib = _lib.load()
    for name in ("aehmc_summary_sketch_update", "aehmc_summary_sketch_quantiles"):
        assert name in _lib.SYMBOLS
        assert getattr(lib, name) is not None
