"""Posterior summaries on the device (aehmc_amd/summary.py over csrc/summary.cuh) against the numpy restatement of
tests/summary_ref.py, their determinism, and summary.run against sample + summarize."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import summary_ref as sr  # noqa: E402
from test_summary_host import MCSE_RATIO_BAND  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

RTOL = 1e-9  # the project's parity tolerance
REALS = ("sd", "rhat", "ess", "mcse", "ess_chains", "mcse_chains")


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int64) if a.dtype == torch.float64 else a,
                                                                     b.contiguous().view(torch.int64) if b.dtype == torch.float64 else b)


def against_restatement(s, ref, shape):
    """mean within RTOL of the coordinate's sd, every other real within RTOL relative (NaN and inf where the
    restatement has them), lag_truncated equal -- on every coordinate."""
    assert not ref["near"].any(), "a deciding pair sum of the restatement lies within 1e-9 of zero: pick another seed"
    sd = ref["sd"].reshape(shape)
    got = s.mean.cpu().numpy()
    assert got.shape == shape
    err = np.abs(got - ref["mean"].reshape(shape))
    print("mean: max |err| / sd", np.max(err / np.where(sd > 0, sd, 1.0)))
    assert np.all(err <= RTOL * sd + (sd == 0) * RTOL * np.abs(ref["mean"].reshape(shape)))
    for name in REALS:
        got, want = getattr(s, name).cpu().numpy(), ref[name].reshape(shape)
        assert got.shape == shape
        fin = np.isfinite(want)
        assert np.array_equal(np.isnan(got), np.isnan(want)), name
        assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), name
        rel = np.abs(got[fin] - want[fin]) / np.where(want[fin] != 0, np.abs(want[fin]), 1.0)
        print(name, "max rel err", rel.max() if rel.size else 0.0)
        assert np.all(rel <= RTOL), (name, rel.max())
    assert np.array_equal(s.lag_truncated.cpu().numpy(), ref["lag_truncated"].reshape(shape))


def series(seed, N, C, D):
    """AR(1) draws with a correlation, a location and a scale per coordinate, and a small offset per chain."""
    r = np.random.default_rng(seed)
    phi = r.uniform(-0.3, 0.8, size=D)
    x = sr.ar1(r, N, C, D, phi, loc=r.normal(size=D) * 3.0, scale=0.5 + r.random(D))
    return x + 0.05 * r.normal(size=(1, C, D))


# (N, C, D, split, layout): D in {1, 2, 63, 64, 65, 100, 1000}, C in {1, 3, 64, 4096}, N in {4, 5, 401, 1000}
CASES = [(4, 1, 1, True, "N"), (5, 3, 2, True, "NCD"), (401, 64, 63, True, "NCD"), (401, 64, 64, False, "NCD"),
         (401, 3, 65, True, "NCD"), (1000, 64, 100, True, "NCD"), (1000, 3, 1000, False, "NCD"),
         (401, 4096, 2, True, "NCD"), (5, 4096, 1, True, "NC"), (1000, 1, 100, False, "ND"), (4, 64, 100, False, "NCD"),
         (401, 1, 1, True, "NC"), (5, 64, 1000, True, "NCD")]


@pytest.mark.parametrize("N,C,D,split,layout", CASES)
def test_kernels_against_restatement(N, C, D, split, layout):
    from aehmc_amd import summary
    x = series(100 + N + C + D, N, C, D)
    ref = sr.summarize(x, split=split)
    shape = {"N": (), "NC": (), "ND": (D,), "NCD": (D,)}[layout]
    view = {"N": (N,), "NC": (N, C), "ND": (N, D), "NCD": (N, C, D)}[layout]
    s = summary.summarize(dev(x).reshape(view), batched=layout in ("NC", "NCD"), split=split)
    assert (s.num_draws, s.num_chains) == (N, C)
    against_restatement(s, ref, shape)
    assert same_bits(summary.rhat(dev(x).reshape(view), batched=layout in ("NC", "NCD"), split=split), s.rhat)


@pytest.mark.parametrize("N,C,D,split", [(401, 5, 70, True), (100, 64, 3, False), (75, 130, 1, True)])
def test_chunking_changes_nothing(N, C, D, split):
    """An Accumulator fed chunks of 1, 37 and N draws: bit-equal moments and Summary fields; they are summarize()'s
    too, and two identical summarize() calls are bit-equal in every field."""
    from aehmc_amd import summary
    x = dev(series(7 + N, N, C, D))
    runs = []
    for chunk in (1, 37, N):
        acc = summary.Accumulator(N, C, (D,), split=split)
        for lo in range(0, N, chunk):
            acc.update(x[lo:lo + chunk])
        runs.append((acc.mean.clone(), acc.m2.clone(), acc.result()))
    a, b = summary.summarize(x, split=split), summary.summarize(x, split=split)
    for f in summary.Summary._fields[:8]:
        assert same_bits(getattr(a, f), getattr(b, f)), f
    for mean, m2, res in runs:
        assert same_bits(mean, runs[0][0]) and same_bits(m2, runs[0][1])
        assert res.ess is None and res.mcse is None and res.lag_truncated is None
        for f in ("mean", "sd", "rhat", "ess_chains", "mcse_chains"):
            assert same_bits(getattr(res, f), getattr(a, f)), f
    with pytest.raises(ValueError, match="exceed"):
        acc.update(x[:1])
    with pytest.raises(ValueError, match="chunk must be"):
        summary.Accumulator(N, C, (D,)).update(x[:, :C - 1].contiguous())


def _equal_runs(make_kernel, state, args, N, extra=()):
    """summary.run(chunk=37 or less) against kernel.sample(N) + summarize on a second kernel with the same seeds."""
    from aehmc_amd import summary
    k1, k2 = make_kernel(), make_kernel()
    kw = {} if not extra else {"num_integration_steps": extra[0]}
    samples, info, acc, div = k1.sample(state, *args, *extra, N)
    want = summary.summarize(samples)
    got, info2, acc2, div2 = summary.run(k2, state, *args, N, chunk=min(37, N - 2), **kw)
    for f in ("mean", "sd", "rhat", "ess_chains", "mcse_chains"):
        assert same_bits(getattr(got, f), getattr(want, f)), f
    assert got.ess is None and (got.num_draws, got.num_chains) == (want.num_draws, want.num_chains)
    for f in ("position", "potential_energy", "potential_energy_grad", "momentum"):
        assert same_bits(getattr(info2.state, f), getattr(info.state, f)), f
    assert same_bits(info2.acceptance_probability, info.acceptance_probability)
    assert torch.equal(info2.is_diverging, info.is_diverging) and torch.equal(info2.n_leapfrog, info.n_leapfrog)
    assert same_bits(acc2, acc) and torch.equal(div2, div)
    h1 = getattr(k1, "_nuts", None) or k1._hmc
    h2 = getattr(k2, "_nuts", None) or k2._hmc
    assert torch.equal(h1["holder"]["rng"], h2["holder"]["rng"])
    return samples, want


@pytest.fixture(scope="module")
def diag_gaussian_run():
    """NUTS on N(mu, diag sigma^2), D = 100, 512 chains started from exact draws, 400 transitions."""
    from aehmc_amd import RandomStream, nuts, targets
    r = np.random.default_rng(11)
    C, D, N = 512, 100, 400
    mu, sigma = r.normal(size=D) * 2.0, 0.5 + r.random(D)
    tgt = targets.DiagGaussian(mu, sigma)
    state = nuts.new_state(dev(mu + sigma * r.normal(size=(C, D))), tgt)
    samples, want = _equal_runs(lambda: nuts.new_kernel(RandomStream(seeds=[30_000 + c for c in range(C)]), tgt),
                                state, (0.3, sigma**2), N)
    return mu, samples, want


def test_run_equals_sample_then_summarize_nuts(diag_gaussian_run):
    mu, samples, want = diag_gaussian_run
    against_restatement(want, sr.summarize(samples.cpu().numpy()), (100,))


def test_run_equals_sample_then_summarize_hmc():
    from aehmc_amd import RandomStream, hmc, targets
    r = np.random.default_rng(12)
    C, D = 64, 10
    tgt = targets.DiagGaussian(r.normal(size=D), 0.5 + r.random(D))
    state = hmc.new_state(dev(r.normal(size=(C, D))), tgt)
    _equal_runs(lambda: hmc.new_kernel(RandomStream(seeds=list(range(C))), tgt), state, (0.2, 0.5 + r.random(D)), 100,
                extra=(8,))


def test_run_leaves_the_whitened_carry_alone():
    """Dense-precision Gaussian under a shared dense metric at D = 520 (whitened leapfrogs, state carried from call to
    call): the chunks of summary.run, with the summary kernels between them, give the bits of one sample() call."""
    from aehmc_amd import RandomStream, nuts, targets
    r = np.random.default_rng(13)
    C, D = 8, 520
    A, B = r.normal(size=(D, D)), r.normal(size=(D, D))
    prec, imm = A @ A.T / D + np.eye(D), B @ B.T / D + np.eye(D)
    prec, imm = 0.5 * (prec + prec.T), 0.5 * (imm + imm.T)
    tgt = targets.DenseMVN(r.normal(size=D), prec)
    state = nuts.new_state(dev(r.normal(size=(C, D))), tgt)
    _equal_runs(lambda: nuts.new_kernel(RandomStream(seeds=list(range(C))), tgt, max_num_expansions=3), state,
                (0.1, dev(imm)), 7)


def test_statistics_of_the_diag_gaussian_run(diag_gaussian_run):
    """|mean - mu| / mcse_chains < 4 on every coordinate (the form and threshold of test_nuts_mcse_matches_oracle), and
    the two standard errors agree within the band of tests/test_summary_host.py."""
    mu, _, s = diag_gaussian_run
    z = (s.mean.cpu().numpy() - mu) / s.mcse_chains.cpu().numpy()
    q = (s.mcse / s.mcse_chains).cpu().numpy()
    print("max |z|", np.abs(z).max(), "mcse / mcse_chains", q.min(), q.max(), "rhat max", float(s.rhat.max()),
          "ess min / max", float(s.ess.min()), float(s.ess.max()))
    assert np.all(np.abs(z) < 4.0), z
    assert np.all((q > MCSE_RATIO_BAND[0]) & (q < MCSE_RATIO_BAND[1])), (q.min(), q.max())


def test_not_converged_and_never_moving():
    from aehmc_amd import summary
    x = series(21, 200, 16, 5)
    x[:, :8, 0] += 4.0   # two groups of chains with different means
    x[:, :, 3] = 1.25    # a coordinate that never moved
    x[:, :, 4] = np.arange(16)[None, :]  # stuck chains, each somewhere else
    ref = sr.summarize(x)
    s = summary.summarize(dev(x))
    against_restatement(s, ref, (5,))
    assert float(s.rhat[0]) > 2.0
    assert torch.isnan(s.rhat[3]) and torch.isnan(s.ess[3]) and float(s.mcse[3]) == 0.0 and float(s.sd[3]) == 0.0
    acc = summary.Accumulator(200, 16, (5,)).update(dev(x)).result()
    assert torch.isnan(acc.rhat[3]) and torch.isnan(acc.ess_chains[3]) and float(acc.mcse_chains[3]) == 0.0


def test_autocovariance_limit_and_max_lag():
    from aehmc_amd import summary
    N, C = 10_000, 4
    r = np.random.default_rng(31)
    x = sr.ar1(r, N, C, 3, np.array([0.0, 0.9, 0.9]))
    with pytest.raises(ValueError, match=rf"{summary.MAX_ACOV_ROWS}.*max_lag"):
        summary.summarize(dev(x))
    s = summary.summarize(dev(x), max_lag=20)
    ref = sr.summarize(x, max_lag=20)
    against_restatement(s, ref, (3,))
    assert s.lag_truncated.cpu().tolist() == [False, True, True]
    # every lag of the longest segment that fits: 4096 draws per split chain
    y = series(32, 8192, 2, 2)
    against_restatement(summary.summarize(dev(y)), sr.summarize(y), (2,))
