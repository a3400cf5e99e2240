"""Host-side checks of the posterior summaries: the numpy restatement (tests/summary_ref.py) against closed forms, and
the Python layer's argument validation, which runs before anything touches the device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import summary_ref as sr  # noqa: E402

torch = pytest.importorskip("torch")

# ESS / theory of the restatement on stationary AR(1) series, theory = N C (1 - phi) / (1 + phi); see
# test_restatement_against_ar1_closed_form for where the numbers come from
ESS_BAND = {0.0: (0.92, 1.12), 0.5: (0.92, 1.12), 0.9: (0.54, 1.28)}
# mcse / mcse_chains at 1024 split chains of 200 draws with little autocorrelation, for 100 coordinates at once
MCSE_RATIO_BAND = (0.886, 1.124)
AR1_SEED = 1000


@pytest.mark.parametrize("N,C", [(400, 512), (1000, 64)])
@pytest.mark.parametrize("phi", [0.0, 0.5, 0.9])
def test_restatement_against_ar1_closed_form(N, C, phi):
    """ESS of the restatement over N C (1 - phi) / (1 + phi) on AR(1) series [N, C, 4] (marginal N(2, 3^2)) drawn with
    numpy default_rng(1000) -- the committed seed -- at (N, C) = (400, 512) and (1000, 64).

    Observed on that seed, all 4 coordinates, both shapes: phi = 0: 0.989 ... 1.010; phi = 0.5: 0.989 ... 1.049;
    phi = 0.9: 0.751 ... 1.068.  Spread over the 20 seeds 1000 ... 1019 (standard deviation of the ratio, the larger of
    the two shapes): 0.007, 0.022, 0.070.  The band is the observed range of phi in {0, 0.5} (0.989 ... 1.049) and of
    phi = 0.9, each widened by three of those standard deviations (0.067 and 0.21).

    phi = 0.9 at N = 400 is the truncated case: segments of 200 draws whose chain means are removed leave
    rho_k > 0 at every lag (the bias of the centred autocovariance shrinks with (n - k) / n while W's does not), so the
    pair sums are positive to the last lag, tau is over-estimated (ratio ~0.8) and lag_truncated says so."""
    x = sr.ar1(np.random.default_rng(AR1_SEED), N, C, 4, phi, loc=2.0, scale=3.0)
    r = sr.summarize(x)
    ratio = r["ess"] / (N * C * (1 - phi) / (1 + phi))
    print("ess / theory", ratio, "mcse / mcse_chains", r["mcse"] / r["mcse_chains"], "rhat", r["rhat"])
    lo, hi = ESS_BAND[phi]
    assert np.all((ratio > lo) & (ratio < hi)), ratio
    assert np.all(r["lag_truncated"] == (phi == 0.9 and N == 400))
    assert not r["near"].any()
    assert np.all(np.abs(r["rhat"] - 1) < 0.06)
    np.testing.assert_allclose(r["sd"], 3.0, rtol=0.05)
    assert np.all(np.abs(r["mean"] - 2.0) < 5 * r["mcse"])


def test_restatement_on_iid_draws_and_mcse_agreement():
    """iid N(0, 1) draws [400, 512, 4] from default_rng(7): ESS / (N C) observed 1.003 ... 1.016 (band of phi = 0), and
    the two standard errors agree.

    mcse / mcse_chains at this shape (1024 split chains of 200 draws): observed 0.977 ... 1.033 on the committed AR(1)
    seed for phi in {0, 0.5} and 0.991 ... 1.005 here; standard deviation over the seeds 1000 ... 1019: 0.018 (it is the
    noise of a variance estimated from 1024 chain means, sqrt(2 / 1023) / 2 = 0.022, not of ess).  MCSE_RATIO_BAND is
    that range widened by five standard deviations (0.0905), because the GPU test holds all 100 coordinates of its
    target to it at once: 100 two-sided tails at 5 sd are 6e-5."""
    x = np.random.default_rng(7).standard_normal((400, 512, 4))
    r = sr.summarize(x)
    ratio = r["ess"] / (400 * 512)
    print("ess / (N C)", ratio, "mcse / mcse_chains", r["mcse"] / r["mcse_chains"])
    assert np.all((ratio > ESS_BAND[0.0][0]) & (ratio < ESS_BAND[0.0][1]))
    q = r["mcse"] / r["mcse_chains"]
    assert np.all((q > MCSE_RATIO_BAND[0]) & (q < MCSE_RATIO_BAND[1]))
    np.testing.assert_allclose(r["ess_chains"], r["sd"] ** 2 / r["mcse_chains"] ** 2, rtol=1e-12)
    assert not r["lag_truncated"].any()


def test_restatement_split_and_degenerate_cases():
    """Odd N: the middle draw belongs to neither half.  Two groups of chains with different means: rhat well above 1.
    A coordinate that never moved: rhat = ess = NaN, mcse = 0."""
    x = np.random.default_rng(3).standard_normal((5, 3, 2))
    z = sr.split_chains(x)
    assert z.shape == (2, 6, 2) and np.array_equal(z[:, :3], x[:2]) and np.array_equal(z[:, 3:], x[3:])
    y = np.random.default_rng(4).standard_normal((100, 8, 2))
    y[:, :4, 0] += 5.0
    y[:, :, 1] = 3.0
    r = sr.summarize(y)
    assert r["rhat"][0] > 2.0 and r["ess"][0] < 20
    assert np.isnan(r["rhat"][1]) and np.isnan(r["ess"][1]) and r["mcse"][1] == 0.0 and r["sd"][1] == 0.0


def test_summary_module_is_exported():
    import aehmc_amd
    from aehmc_amd import summary
    assert aehmc_amd.summary is summary and "summary" in aehmc_amd.__all__
    assert summary.Summary._fields == ("mean", "sd", "rhat", "ess", "mcse", "ess_chains", "mcse_chains",
                                       "lag_truncated", "num_draws", "num_chains")
    for name in ("summarize", "Accumulator", "run", "rhat", "ess", "mcse"):
        assert callable(getattr(summary, name))


def test_validation_precedes_the_device(monkeypatch):
    """Bad arguments raise ValueError without the engine being asked for at all."""
    from aehmc_amd import summary

    def no_device(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")

    monkeypatch.setattr(summary, "get_engine", no_device)
    ok = torch.zeros(8, 3, 2, dtype=torch.float64)
    with pytest.raises(ValueError, match="at least 4 draws"):
        summary.summarize(ok[:3].contiguous())
    with pytest.raises(ValueError, match="at least 2 draws"):
        summary.summarize(ok[:1].contiguous(), split=False)
    with pytest.raises(ValueError, match="float64"):
        summary.summarize(ok.to(torch.float32))
    with pytest.raises(ValueError, match="contiguous"):
        summary.summarize(ok.transpose(1, 2))
    with pytest.raises(ValueError, match="torch tensor"):
        summary.summarize(ok.numpy())
    for bad, batched in ((torch.zeros(8, dtype=torch.float64), True), (torch.zeros(8, 2, 2, 2, dtype=torch.float64), True),
                         (ok, False)):
        with pytest.raises(ValueError, match="samples must be"):
            summary.summarize(bad, batched=batched)
    with pytest.raises(ValueError, match="max_lag"):
        summary.summarize(ok, max_lag=0)
    # above the autocovariance kernel's limit: the message names it and points to max_lag
    long_run = torch.zeros(2 * summary.MAX_ACOV_ROWS, 1, dtype=torch.float64)
    with pytest.raises(ValueError, match=rf"{summary.MAX_ACOV_ROWS}.*max_lag"):
        summary.summarize(long_run)
    with pytest.raises(ValueError, match="at least 4 draws"):
        summary.Accumulator(3, 2, (5,))
    with pytest.raises(ValueError, match="scalar or a vector"):
        summary.Accumulator(10, 2, (5, 5))

    class K:
        _hmc = {}
        num_chains, batched = 3, True

        @staticmethod
        def sample(*a, **k):
            raise AssertionError("sampled before the arguments were checked")

    state = type("S", (), {"position": torch.zeros(3, 2, dtype=torch.float64)})()
    with pytest.raises(ValueError, match="num_integration_steps"):
        summary.run(K, state, 0.1, 1.0, 10)
    with pytest.raises(ValueError, match="chunk"):
        summary.run(K, state, 0.1, 1.0, 10, num_integration_steps=3, chunk=0)
    with pytest.raises(ValueError, match="at least 4 draws"):
        summary.run(K, state, 0.1, 1.0, 3, num_integration_steps=3)


def test_valid_call_without_gpu_raises_engine_error(monkeypatch):
    """No CPU fallback: where torch sees no GPU (here: told so), every entry point raises EngineError, as
    hmc.new_state does."""
    from aehmc_amd import summary
    from aehmc_amd.engine import EngineError
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    x = torch.zeros(8, 3, 2, dtype=torch.float64)
    with pytest.raises(EngineError):
        summary.summarize(x)
    with pytest.raises(EngineError):
        summary.rhat(x)
    with pytest.raises(EngineError):
        summary.Accumulator(8, 3, (2,))
