"""Host-side checks of the quantiles: the numpy restatement (tests/quantile_ref.py) against numpy.quantile to the bit,
the new names and C-ABI symbols, and the Python layer's argument validation, which runs before anything touches the
device."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import quantile_ref as qr  # noqa: E402

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("aehmc_summary_quantile_work", "aehmc_summary_order_stats", "aehmc_summary_quantiles")
PROBS = (0.0, 0.05, 1.0 / 3.0, 0.5, 0.95, 1.0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("R", [1, 2, 3, 7, 1961])
def test_restatement_is_numpy_quantile_to_the_bit(R):
    """default_rng(500 + R), columns of different location and scale, and one of small integers (ties)."""
    r = np.random.default_rng(500 + R)
    x = r.normal(size=(R, 6)) * np.array([1.0, 1e-3, 1e6, 1.0, 3.0, 1.0]) + np.array([0.0, 5.0, -7e6, 1e3, 0.0, 0.0])
    x[:, 5] = r.integers(-3, 4, size=R)
    got = qr.quantiles(x, PROBS)
    want = np.quantile(x, PROBS, axis=0)
    assert got.shape == want.shape == (len(PROBS), 6)
    assert np.array_equal(bits(got), bits(want))
    ranks = sorted({0, R // 2, R - 1})
    assert np.array_equal(bits(qr.order_statistics(x, ranks)), bits(np.sort(x, axis=0)[ranks]))


def test_restatement_is_nan_where_numpy_quantile_is():
    x = np.random.default_rng(77).normal(size=(50, 4))
    x[17, 2] = np.nan
    got = qr.quantiles(x, PROBS)
    with np.errstate(invalid="ignore"):
        want = np.quantile(x, PROBS, axis=0)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got[:, 2]).all() and not np.isnan(got[:, 0]).any()
    keep = [0, 1, 3]
    assert np.array_equal(bits(got[:, keep]), bits(want[:, keep]))
    assert np.isnan(qr.order_statistics(x, [0, 49])[:, 2]).all()


def test_restatement_tail_ess_on_iid_draws():
    """iid draws: both indicators are iid Bernoulli, so the tail ESS is about N C (band of test_summary_host's
    phi = 0 case, widened to 0.8 ... 1.2 for a 5 % indicator of 16 x 400 draws)."""
    x = np.random.default_rng(5).standard_normal((400, 16, 3))
    ess, near, trunc = qr.tail_ess(x)
    assert not near.any() and not trunc.any()
    assert np.all((ess > 0.8 * 6400) & (ess < 1.2 * 6400)), ess


def test_new_names_are_exported():
    from aehmc_amd import summary
    for name in ("quantiles", "median", "interval", "order_statistics", "tail_ess"):
        assert callable(getattr(summary, name)), name
    assert summary.Summary._fields == ("mean", "sd", "rhat", "ess", "mcse", "ess_chains", "mcse_chains",
                                       "lag_truncated", "num_draws", "num_chains")


def test_library_exports_the_quantile_symbols():
    from aehmc_amd import _lib
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
    assert lib.aehmc_summary_quantile_work(1000, 100, 3) > 0
    assert lib.aehmc_summary_quantile_work(1 << 20, 5, 8) == lib.aehmc_summary_quantile_work(7, 5, 8)
    assert lib.aehmc_summary_quantile_work(0, 100, 3) == 0 and lib.aehmc_summary_quantile_work(10, 100, 65) == 0


def test_lib_declares_the_header_argument_counts():
    from aehmc_amd import _lib, summary
    hdr = open(os.path.join(ROOT, "include", "aehmc_hip.h")).read()
    limit = int(re.search(r"#define AEHMC_SUMMARY_QUANTILE_MAX (\d+)", hdr).group(1))
    assert limit == summary.MAX_QUANTILES >= 32
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW_SYMBOLS:
        m = re.search(rf"\bint(?:64_t)?\s+{name}\s*\(([^)]*)\)\s*;", hdr)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SYMBOLS[name][1]), name


def test_validation_precedes_the_device(monkeypatch):
    """Bad samples, probs or ranks raise ValueError without the engine being asked for at all."""
    from aehmc_amd import summary

    def no_device(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")

    monkeypatch.setattr(summary, "get_engine", no_device)
    ok = torch.zeros(8, 3, 2, dtype=torch.float64)
    calls = {"quantiles": lambda x, **kw: summary.quantiles(x, 0.5, **kw), "median": summary.median,
             "interval": summary.interval, "order_statistics": lambda x, **kw: summary.order_statistics(x, [0], **kw),
             "tail_ess": summary.tail_ess}
    for name, call in calls.items():
        with pytest.raises(ValueError, match="float64"):
            call(ok.to(torch.float32))
        with pytest.raises(ValueError, match="contiguous"):
            call(ok.transpose(1, 2))
        with pytest.raises(ValueError, match="torch tensor"):
            call(ok.numpy())
        for bad, batched in ((torch.zeros(8, dtype=torch.float64), True),
                             (torch.zeros(8, 2, 2, 2, dtype=torch.float64), True), (ok, False)):
            with pytest.raises(ValueError, match="samples must be"):
                call(bad, batched=batched)
        with pytest.raises(ValueError, match="at least one draw"):
            call(torch.zeros(0, 3, 2, dtype=torch.float64))
    for bad in (-0.1, 1.5, float("nan"), float("inf"), (0.5, 2.0), (), [0.1] * (summary.MAX_QUANTILES + 1), "a", None,
                (0.5, None)):
        with pytest.raises(ValueError, match="probs"):
            summary.quantiles(ok, bad)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="probs"):
            summary.interval(ok, bad)
        with pytest.raises(ValueError, match="probs"):
            summary.tail_ess(ok, prob=bad)
    for bad in ((), (-1,), (24,), (0, 24), (0.5,), [0] * (summary.MAX_QUANTILES + 1), 3, ("a",)):
        with pytest.raises(ValueError, match="ranks"):
            summary.order_statistics(ok, bad)
    with pytest.raises(ValueError, match="at least 4 draws"):
        summary.tail_ess(ok[:3].contiguous())
    with pytest.raises(ValueError, match="max_lag"):
        summary.tail_ess(ok, max_lag=0)
    long_run = torch.zeros(2 * summary.MAX_ACOV_ROWS, 1, dtype=torch.float64)
    with pytest.raises(ValueError, match=rf"{summary.MAX_ACOV_ROWS}.*max_lag"):
        summary.tail_ess(long_run)


def test_valid_call_without_gpu_raises_engine_error(monkeypatch):
    """No CPU fallback: where torch sees no GPU (here: told so), every new entry point raises EngineError."""
    from aehmc_amd import summary
    from aehmc_amd.engine import EngineError
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    x = torch.zeros(8, 3, 2, dtype=torch.float64)
    with pytest.raises(EngineError):
        summary.quantiles(x, (0.05, 0.95))
    with pytest.raises(EngineError):
        summary.median(x)
    with pytest.raises(EngineError):
        summary.interval(x)
    with pytest.raises(EngineError):
        summary.order_statistics(x, [0, 23])
    with pytest.raises(EngineError):
        summary.tail_ess(x)
