"""Streaming ESS / MCSE on the device (summary.Accumulator / summary.run with max_lag, over aehmc_summary_lag_update of
csrc/summary.cuh) against the numpy restatement of tests/summary_ref.py and the stored-draw path, their determinism
under any chunking, and runs the stored-draw path cannot hold."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import summary_ref as sr  # noqa: E402
import summary_stream_ref as ssr  # noqa: E402

torch = pytest.importorskip("torch")
from test_gpu_summary import RTOL, against_restatement, dev, same_bits, series  # noqa: E402

pytestmark = pytest.mark.gpu

FIELDS = ("mean", "sd", "rhat", "ess", "mcse", "ess_chains", "mcse_chains", "lag_truncated")
STREAMING = ("mean", "sd", "rhat", "ess_chains", "mcse_chains")


def stream(x, split, L, chunk, shape=None):
    """Summary of the device tensor x [N, C, ...] fed to an Accumulator in chunks of `chunk` draws"""
    from aehmc_amd import summary
    N, C = x.shape[:2]
    acc = summary.Accumulator(N, C, tuple(x.shape[2:]) if shape is None else shape, split=split, max_lag=L)
    for lo in range(0, N, chunk):
        acc.update(x[lo:lo + chunk])
    return acc.result()


def close(got, want, name):
    g, w = got.cpu().numpy(), want.cpu().numpy()
    assert np.array_equal(np.isnan(g), np.isnan(w)), name
    fin = np.isfinite(w)
    rel = np.abs(g[fin] - w[fin]) / np.where(w[fin] != 0, np.abs(w[fin]), 1.0)
    print(name, "max rel diff", rel.max() if rel.size else 0.0)
    assert np.all(rel <= RTOL), (name, rel.max())


# the last two: more lags than one pass of the fold covers (144), whole chains and split ones with a chunk across the
# split point; seeds checked for `near` like the others
@pytest.mark.parametrize("N,C,D,split,L,seed", ssr.CASES + [(400, 3, 17, False, 150, 11), (700, 2, 5, True, 300, 12)])
def test_stream_against_restatement(N, C, D, split, L, seed):
    x = series(seed, N, C, D)
    s = stream(dev(x), split, L, 37)
    assert (s.num_draws, s.num_chains) == (N, C)
    against_restatement(s, sr.summarize(x, split=split, max_lag=L), (D,))


def test_stream_scalar_positions():
    N, C, D, split, L, seed = ssr.CASES[2]
    x = series(seed, N, C, D)
    s = stream(dev(x).reshape(N, C), split, L, 37)
    against_restatement(s, sr.summarize(x, split=split, max_lag=L), ())


@pytest.mark.parametrize("N,C,D,split,L,seed", ssr.CASES[:3])
def test_stream_against_stored_draws(N, C, D, split, L, seed):
    from aehmc_amd import summary
    x = dev(series(seed, N, C, D))
    got, want = stream(x, split, L, 37), summary.summarize(x, split=split, max_lag=L)
    close(got.ess, want.ess, "ess")
    close(got.mcse, want.mcse, "mcse")
    assert torch.equal(got.lag_truncated, want.lag_truncated)
    for f in STREAMING:
        assert same_bits(getattr(got, f), getattr(want, f)), f


def test_chunking_changes_nothing():
    """Chunks of 1, K - 2, K - 1, K, 37 and N draws, K - 1 = 40 the ring's length: shorter than the ring, as long, longer,
    the split point (draws 200 | 201) inside a chunk -- every field has the same bits, and so has a second run."""
    N, C, D, split, L, seed = ssr.CASES[0]
    x = dev(series(seed, N, C, D))
    K = min(L + 1, N // 2)
    runs = [stream(x, split, L, chunk) for chunk in (1, K - 2, K - 1, K, 37, N, 37)]
    for r in runs[1:]:
        for f in FIELDS:
            assert same_bits(getattr(r, f), getattr(runs[0], f)), f


def test_large_offset():
    N, C, D, split, L, seed = ssr.OFFSET_CASE
    x = series(seed, N, C, D) + ssr.OFFSET
    against_restatement(stream(dev(x), split, L, 37), sr.summarize(x, split=split, max_lag=L), (D,))


def test_not_converged_and_never_moving():
    x = series(21, 200, 16, 5)
    x[:, :8, 0] += 4.0   # two groups of chains with different means
    x[:, :, 3] = 1.25    # a coordinate that never moved
    x[:, :, 4] = np.arange(16)[None, :]  # stuck chains, each somewhere else
    ref = sr.summarize(x, max_lag=20)
    s = stream(dev(x), True, 20, 37)
    against_restatement(s, ref, (5,))
    assert float(s.rhat[0]) > 2.0
    assert torch.isnan(s.ess[3]) and float(s.mcse[3]) == 0.0 and float(s.sd[3]) == 0.0
    assert np.isfinite(ref["ess"][4]) and ref["sd"][4] > 0  # (the stuck chains: compared above like every coordinate)


def test_beyond_the_stored_draw_limit():
    """20 000 draws: segments of 10 000, which summarize cannot hold at any max_lag."""
    from aehmc_amd import summary
    N, C = 20_000, 4
    x = sr.ar1(np.random.default_rng(32), N, C, 3, np.array([0.0, 0.9, 0.9]))
    with pytest.raises(ValueError, match=rf"{summary.MAX_ACOV_ROWS}"):
        summary.summarize(dev(x), max_lag=50)
    ref = sr.summarize(x, max_lag=50)
    s = stream(dev(x), True, 50, 4096)
    against_restatement(s, ref, (3,))
    assert np.array_equal(s.lag_truncated.cpu().numpy(), ref["lag_truncated"])


def _run_against_sample(make_kernel, state, args, N, L, extra=()):
    """summary.run(chunk=37, max_lag=L) against kernel.sample(N) + summarize(max_lag=L) on a twin kernel."""
    from aehmc_amd import summary
    k1, k2, k3 = make_kernel(), make_kernel(), make_kernel()
    kw = {} if not extra else {"num_integration_steps": extra[0]}
    samples, info, acc, div = k1.sample(state, *args, *extra, N)
    want = summary.summarize(samples, max_lag=L)
    got, info2, acc2, div2 = summary.run(k2, state, *args, N, chunk=37, max_lag=L, **kw)
    close(got.ess, want.ess, "ess")
    close(got.mcse, want.mcse, "mcse")
    assert torch.equal(got.lag_truncated, want.lag_truncated)
    for f in STREAMING:
        assert same_bits(getattr(got, f), getattr(want, f)), f
    for f in ("position", "potential_energy", "potential_energy_grad", "momentum"):
        assert same_bits(getattr(info2.state, f), getattr(info.state, f)), f
    assert same_bits(info2.acceptance_probability, info.acceptance_probability)
    assert torch.equal(info2.is_diverging, info.is_diverging) and torch.equal(info2.n_leapfrog, info.n_leapfrog)
    assert same_bits(acc2, acc) and torch.equal(div2, div)
    h1 = getattr(k1, "_nuts", None) or k1._hmc
    h2 = getattr(k2, "_nuts", None) or k2._hmc
    assert torch.equal(h1["holder"]["rng"], h2["holder"]["rng"])
    plain = summary.run(k3, state, *args, N, chunk=37, **kw)[0]
    assert plain.ess is None and plain.mcse is None and plain.lag_truncated is None
    for f in STREAMING:
        assert same_bits(getattr(plain, f), getattr(got, f)), f


def test_run_with_max_lag_nuts():
    from aehmc_amd import RandomStream, nuts, targets
    r = np.random.default_rng(41)
    C, D = 64, 10
    mu, sigma = r.normal(size=D) * 2.0, 0.5 + r.random(D)
    tgt = targets.DiagGaussian(mu, sigma)
    state = nuts.new_state(dev(mu + sigma * r.normal(size=(C, D))), tgt)
    _run_against_sample(lambda: nuts.new_kernel(RandomStream(seeds=[50_000 + c for c in range(C)]), tgt), state,
                        (0.3, sigma**2), 100, 20)


def test_run_with_max_lag_hmc():
    from aehmc_amd import RandomStream, hmc, targets
    r = np.random.default_rng(42)
    C, D = 64, 10
    tgt = targets.DiagGaussian(r.normal(size=D), 0.5 + r.random(D))
    state = hmc.new_state(dev(r.normal(size=(C, D))), tgt)
    _run_against_sample(lambda: hmc.new_kernel(RandomStream(seeds=list(range(C))), tgt), state,
                        (0.2, 0.5 + r.random(D)), 100, 20, extra=(8,))


def test_errors():
    from aehmc_amd import summary
    with pytest.raises(ValueError, match="max_lag"):
        summary.Accumulator(100, 4, (3,), max_lag=0)
    acc = summary.Accumulator(100, 4, (3,), max_lag=5)
    acc.update(dev(series(1, 60, 4, 3)))
    with pytest.raises(ValueError, match="60 of 100"):
        acc.result()
