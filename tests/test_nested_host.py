"""Host-side checks of the nested R-hat: the numpy restatement (tests/nested_ref.py) against closed forms, the Python
layer's argument validation, which runs before anything touches the device, and the exports."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import nested_ref as nr  # noqa: E402

torch = pytest.importorskip("torch")


@pytest.mark.parametrize("N,C,D", [(2, 2, 1), (4, 2, 3), (7, 13, 5), (50, 64, 4)])
def test_one_chain_per_superchain_is_the_classical_rhat_plus_one_over_n(N, C, D):
    """M = 1: between is the variance of the chain means and within the mean of the chains' variances, so
    nested_rhat^2 - rhat^2 = 1 + B/W - ((n - 1) / n + B/W) = 1 / n for the unsplit classical rhat."""
    x = nr.draws(5 + N + C, N, C, 1, D, offset=3.0)
    got = nr.nested_rhat(x, C)["nested_rhat"] ** 2 - nr.classical_rhat(x) ** 2
    print("max |nested^2 - rhat^2 - 1/n|", np.max(np.abs(got - 1.0 / N)))
    assert np.all(np.abs(got - 1.0 / N) <= 1e-12)


def test_copies_constants_and_windows():
    """Superchains that are exact copies of each other: between = 0 and nested_rhat = 1.0 exactly.  Constant input:
    NaN.  Chains constant inside superchains that differ: +inf.  A trace over windows is the restatement of each
    window on its own, and a window of one draw has no variance along the chain."""
    r = np.random.default_rng(2)
    one = r.standard_normal((6, 1, 5, 3)) + 100.0
    x = np.broadcast_to(one, (6, 4, 5, 3)).reshape(6, 20, 3)
    for window in (None, 1, 2, 3):
        res = nr.nested_rhat(x, 4, window)
        assert np.all(res["between"] == 0.0) and np.all(res["within"] > 0.0)
        assert np.all(res["nested_rhat"] == 1.0) and np.all(res["mcse_superchains"] == 0.0)
    const = np.full((4, 6, 2), 7.25)
    res = nr.nested_rhat(const, 3)
    assert np.isnan(res["nested_rhat"]).all() and np.all(res["between"] == 0.0) and np.all(res["within"] == 0.0)
    steps = np.broadcast_to(np.arange(3.0).reshape(1, 3, 1, 1), (4, 3, 2, 2)).reshape(4, 6, 2)
    res = nr.nested_rhat(steps, 3, 2)
    assert np.all(np.isposinf(res["nested_rhat"])) and np.all(res["between"] == 1.0)
    y = nr.draws(3, 6, 3, 4, 2)
    tr = nr.nested_rhat(y, 3, 2)
    assert tr["nested_rhat"].shape == (3, 2)
    for i in range(3):
        one_window = nr.nested_rhat(y[2 * i:2 * i + 2], 3)
        for f in nr.FIELDS:
            assert np.array_equal(tr[f][i], one_window[f])
    a = y[:1].reshape(3, 4, 2)  # one draw: within is the spread of the chains about their superchain's mean alone
    want = (((a - a.mean(axis=1, keepdims=True)) ** 2).sum(axis=1) / 3).mean(axis=0)
    np.testing.assert_allclose(nr.nested_rhat(y[:1], 3)["within"], want, rtol=1e-12)


def test_well_mixed_and_stuck_superchains():
    """Independent draws: B/W is about 1 / (M n) and nested_rhat - 1 about half of it.  Superchains that sit ten
    within-sd apart: about 10."""
    r = np.random.default_rng(8)
    K, M, n, D = 8, 64, 4, 5
    x = r.standard_normal((n, K * M, D))
    res = nr.nested_rhat(x, K)
    assert np.all(res["nested_rhat"] < np.sqrt(1 + 10 / (M * n)))
    np.testing.assert_allclose(res["within"], 1.0 + 1.0 / n, rtol=0.1)  # (the chains' variance + that of their means)
    stuck = x * 1.0 + 10.0 * r.standard_normal((1, K, 1, D)).repeat(M, axis=2).reshape(1, K * M, D)
    assert np.all(nr.nested_rhat(stuck, K)["nested_rhat"] > 2.0)


def test_names_are_exported():
    from aehmc_amd import _lib, summary
    assert summary.NestedRhat._fields == ("nested_rhat", "between", "within", "mean", "mcse_superchains", "num_draws",
                                          "num_chains", "num_superchains", "window")
    for name in ("nested_rhat", "NestedAccumulator", "superchain_positions"):
        assert callable(getattr(summary, name))
    assert "aehmc_nested_update" in _lib.SYMBOLS
    assert getattr(_lib.load(), "aehmc_nested_update") is not None


def test_superchain_positions():
    from aehmc_amd import summary
    starts = torch.arange(6.0, dtype=torch.float64).reshape(3, 2)
    q0 = summary.superchain_positions(starts, chains_per_superchain=4)
    assert q0.shape == (12, 2) and q0.is_contiguous()
    for c in range(12):
        assert torch.equal(q0[c], starts[c // 4])
    assert torch.equal(summary.superchain_positions(starts[:, 0].contiguous(), 2), torch.tensor([0.0, 0.0, 2.0, 2.0, 4.0, 4.0],
                                                                                               dtype=torch.float64))
    assert torch.equal(summary.superchain_positions(starts, 1), starts)
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="chains_per_superchain"):
            summary.superchain_positions(starts, bad)
    with pytest.raises(ValueError, match="starts must be"):
        summary.superchain_positions(torch.zeros(2, 2, 2, dtype=torch.float64), 2)
    with pytest.raises(ValueError, match="torch tensor"):
        summary.superchain_positions(starts.numpy(), 2)


def test_validation_precedes_the_device(monkeypatch):
    """Bad arguments raise ValueError without the engine being asked for at all."""
    from aehmc_amd import summary

    def no_device(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")

    monkeypatch.setattr(summary, "get_engine", no_device)
    ok = torch.zeros(8, 6, 2, dtype=torch.float64)
    for K in (1, 0, -2):
        with pytest.raises(ValueError, match="num_superchains must be at least 2"):
            summary.nested_rhat(ok, K)
    with pytest.raises(ValueError, match="do not divide"):
        summary.nested_rhat(ok, 4)
    with pytest.raises(ValueError, match="do not divide"):  # one chain cannot hold two superchains
        summary.nested_rhat(ok[:, 0].contiguous(), 2, batched=False)
    with pytest.raises(ValueError, match="window must be at least 1"):
        summary.nested_rhat(ok, 3, window=0)
    with pytest.raises(ValueError, match="multiple of window"):
        summary.nested_rhat(ok, 3, window=3)
    with pytest.raises(ValueError, match="window must be an integer"):
        summary.nested_rhat(ok, 3, window=2.0)
    with pytest.raises(ValueError, match="nothing to estimate inside"):
        summary.nested_rhat(ok, 6, window=1)
    with pytest.raises(ValueError, match="nothing to estimate inside"):
        summary.nested_rhat(ok[:1].contiguous(), 6)
    with pytest.raises(ValueError, match="nothing to estimate inside"):
        summary.NestedAccumulator(8, 6, (2,), 6, window=1)
    with pytest.raises(ValueError, match="float64"):
        summary.nested_rhat(ok.to(torch.float32), 3)
    with pytest.raises(ValueError, match="contiguous"):
        summary.nested_rhat(ok.transpose(1, 2), 3)
    with pytest.raises(ValueError, match="torch tensor"):
        summary.nested_rhat(ok.numpy(), 3)
    for bad in (torch.zeros(8, dtype=torch.float64), torch.zeros(8, 2, 2, 2, dtype=torch.float64)):
        with pytest.raises(ValueError, match="samples must be"):
            summary.nested_rhat(bad, 2)
    with pytest.raises(ValueError, match="at least 1 draw"):
        summary.NestedAccumulator(0, 6, (2,), 3)
    with pytest.raises(ValueError, match="scalar or a vector"):
        summary.NestedAccumulator(8, 6, (2, 2), 3)
    with pytest.raises(ValueError, match="num_superchains must be an integer"):
        summary.NestedAccumulator(8, 6, (2,), 3.0)

    class K:
        num_chains, batched = 6, True

        @staticmethod
        def sample(*a, **k):
            raise AssertionError("sampled before the arguments were checked")

    state = type("S", (), {"position": torch.zeros(6, 2, dtype=torch.float64)})()
    with pytest.raises(ValueError, match="nested must be a NestedAccumulator"):
        summary.run(K, state, 0.1, 1.0, 10, nested=object())


class _Engine:
    """Stands in for the device where only the bookkeeping of an accumulator is looked at."""
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def nested_update(self, x, t0, num_draws, window, chains_per_superchain, mean, m2, out):
        self.calls.append((tuple(x.shape), t0, num_draws, window, chains_per_superchain))


def test_accumulator_bookkeeping(monkeypatch):
    """Wrong layout or device, more draws than announced and an early result() are ValueErrors; the engine sees the
    draws' place in the run and the window length (all draws with window=None)."""
    from aehmc_amd import summary
    eng = _Engine()
    monkeypatch.setattr(summary, "get_engine", lambda: eng)
    acc = summary.NestedAccumulator(8, 6, (2,), 3, window=4)
    assert (acc.num_superchains, acc.chains_per_superchain, acc.window) == (3, 2, 4)
    assert acc.mean.shape == (6, 2) and acc.m2.shape == (6, 2) and acc.out.shape == (2, 5, 2)
    x = torch.zeros(8, 6, 2, dtype=torch.float64)
    with pytest.raises(ValueError, match="chunk must be"):
        acc.update(x[:, :5].contiguous())
    with pytest.raises(ValueError, match="chunk must be"):
        acc.update(torch.zeros(3, 6, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="float64"):
        acc.update(x.to(torch.float32))
    with pytest.raises(ValueError, match="must be on"):
        acc.update(x.to("meta"))
    acc.update(x[:3])
    with pytest.raises(ValueError, match="3 of 8 draws folded"):
        acc.result()
    with pytest.raises(ValueError, match="exceed"):
        acc.update(x[:6])
    res = acc.update(x[3:]).result()
    assert eng.calls == [((3, 6, 2), 0, 8, 4, 2), ((5, 6, 2), 3, 8, 4, 2)]
    assert res.nested_rhat.shape == (2, 2) and res.mean.shape == (2, 2)
    assert (res.num_draws, res.num_chains, res.num_superchains, res.window) == (8, 6, 3, 4)
    whole = summary.NestedAccumulator(8, 6, (), 2)
    res = whole.update(torch.zeros(8, 6, dtype=torch.float64)).result()
    assert eng.calls[-1] == ((8, 6, 1), 0, 8, 8, 3) and res.nested_rhat.shape == () and res.window is None

    class K:
        num_chains, batched = 6, True

        @staticmethod
        def sample(*a, **k):
            raise AssertionError("sampled before the arguments were checked")

    state = type("S", (), {"position": torch.zeros(6, 2, dtype=torch.float64)})()
    with pytest.raises(ValueError, match="nested must be a NestedAccumulator of 6 chains"):
        summary.run(K, state, 0.1, 1.0, 10, nested=summary.NestedAccumulator(10, 6, (3,), 3))
    with pytest.raises(ValueError, match="more exceed"):
        summary.run(K, state, 0.1, 1.0, 10, nested=acc)


def test_valid_call_without_gpu_raises_engine_error(monkeypatch):
    """No CPU fallback: where torch sees no GPU (here: told so), the entry points raise EngineError."""
    from aehmc_amd import summary
    from aehmc_amd.engine import EngineError
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    x = torch.zeros(1, 4, 2, dtype=torch.float64)
    with pytest.raises(EngineError):
        summary.nested_rhat(x, 2)
    with pytest.raises(EngineError):
        summary.nested_rhat(x, 2, window=1)
    with pytest.raises(EngineError):
        summary.NestedAccumulator(1, 4, (2,), 2)
