"""Nested R-hat on the device (aehmc_amd/summary.py over csrc/nested.cuh) against the numpy restatement of
tests/nested_ref.py, its independence of the chunking, the identity with the classical R-hat, degenerate and non-finite
input, summary.run(nested=...) against sample + nested_rhat, and a run started as superchains far from the target."""
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import nested_ref as nr  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

RTOL = 1e-9  # the project's parity tolerance (tests/test_gpu_summary.py)
TENSORS = nr.FIELDS


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == torch.float64 and torch.equal(a.contiguous().view(torch.int64),
                                                                                      b.contiguous().view(torch.int64))


def against_restatement(got, ref, shape):
    """between, within, nested_rhat and mcse_superchains within RTOL relative, mean within RTOL sqrt(within + between),
    NaN and inf exactly where the restatement has them -- on every coordinate and window."""
    scale = np.sqrt(ref["within"] + ref["between"]).reshape(shape)
    mean = got.mean.cpu().numpy()
    assert mean.shape == shape
    err = np.abs(mean - ref["mean"].reshape(shape))
    print("mean: max |err| / sqrt(within + between)", np.max(err / np.where(scale > 0, scale, 1.0)))
    fin = np.isfinite(scale)
    assert np.all(err[fin] <= RTOL * scale[fin])
    for name in ("between", "within", "nested_rhat", "mcse_superchains"):
        g, want = getattr(got, name).cpu().numpy(), ref[name].reshape(shape)
        assert g.shape == shape, name
        fin = np.isfinite(want)
        assert np.array_equal(np.isnan(g), np.isnan(want)), name
        assert np.array_equal(g[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), name
        rel = np.abs(g[fin] - want[fin]) / np.where(want[fin] != 0, np.abs(want[fin]), 1.0)
        print(name, "max rel err", rel.max() if rel.size else 0.0)
        assert np.all(rel <= RTOL), (name, rel.max())


# (N, K, M, D, window): each the smallest shape that reaches one edge of the kernel
SHAPES = [(1, 2, 2, 1, 1),       # smallest case
          (4, 2, 1, 3, None),    # M = 1
          (5, 3, 5, 7, 1),       # odd sizes
          (12, 4, 16, 65, 3),    # D crosses the 16-coordinate blocks (and 64), one coordinate in the last
          (8, 5, 13, 130, 4),    # K is not a multiple of the 16 lanes per coordinate; 8 chains side by side + 5 single
          (6, 64, 4, 2, 2),      # narrow D (128 lanes per coordinate), fewer superchains than lanes
          (6, 300, 2, 1, 3),     # more superchains than the 256 lanes of a coordinate
          (2, 2, 300, 5, 2)]     # long superchains


def case(N, K, M, D, window):
    x = nr.draws(10 + N + K + M + D, N, K, M, D)
    return x, nr.nested_rhat(x, K, window)


@pytest.mark.parametrize("N,K,M,D,window", SHAPES)
def test_kernels_against_restatement(N, K, M, D, window):
    from aehmc_amd import summary
    x, ref = case(N, K, M, D, window)
    shape = (D,) if window is None else (N // window, D)
    got = summary.nested_rhat(dev(x), num_superchains=K, window=window)
    assert (got.num_draws, got.num_chains, got.num_superchains, got.window) == (N, K * M, K, window)
    against_restatement(got, ref, shape)
    again = summary.nested_rhat(dev(x), K, window=window)
    for f in TENSORS:
        assert same_bits(getattr(got, f), getattr(again, f)), f


@pytest.mark.parametrize("N,K,M,window", [(1, 2, 2, 1), (6, 300, 2, 3), (4, 3, 5, None)])
def test_scalar_chains_and_the_batched_flag(N, K, M, window):
    """[N, C] draws of scalar chains give fields without a coordinate axis; batched=False is one chain, which cannot
    hold two superchains."""
    from aehmc_amd import summary
    x, ref = case(N, K, M, 1, window)
    shape = () if window is None else (N // window,)
    got = summary.nested_rhat(dev(x[:, :, 0]), K, window=window, batched=True)
    against_restatement(got, ref, shape)
    with_axis = summary.nested_rhat(dev(x), K, window=window)
    for f in TENSORS:
        assert same_bits(getattr(got, f), getattr(with_axis, f).reshape(shape)), f
    with pytest.raises(ValueError, match="do not divide"):
        summary.nested_rhat(dev(x[:, :, 0]), K, window=window, batched=False)


@pytest.mark.parametrize("N,K,M,D,window", [SHAPES[3], SHAPES[4]])
def test_chunking_changes_nothing(N, K, M, D, window):
    """The draws whole, one at a time, in chunks of window - 1 and of window + 1 (cuts inside windows, chunks that end
    several windows): every output is bit-equal, and so is the carried state of the chains where it is still in use."""
    from aehmc_amd import summary
    x = dev(case(N, K, M, D, window)[0])
    runs = []
    for chunk in (N, 1, window - 1, window + 1):
        acc = summary.NestedAccumulator(N, K * M, (D,), K, window=window)
        for lo in range(0, N, chunk):
            acc.update(x[lo:lo + chunk])
        runs.append(acc.result())
    for res in runs[1:]:
        for f in TENSORS:
            assert same_bits(getattr(res, f), getattr(runs[0], f)), f
    # half a window folded: the carried moments do not depend on how it arrived
    half = []
    for chunk in (window - 1, 1):
        acc = summary.NestedAccumulator(N, K * M, (D,), K, window=window)
        for lo in range(0, window + window - 1, chunk):
            acc.update(x[lo:min(lo + chunk, 2 * window - 1)])
        half.append((acc.mean.clone(), acc.m2.clone(), acc.out[0].clone()))
    for a, b in zip(*half):
        assert same_bits(a, b)
    with pytest.raises(ValueError, match="exceed"):
        acc.update(x)


@pytest.mark.parametrize("N,C,D", [(4, 2, 3), (9, 33, 70)])
def test_one_chain_per_superchain_against_the_classical_rhat(N, C, D):
    """M = 1, one window: nested_rhat^2 - rhat^2 = 1 / N for summarize's unsplit rhat.  Each square is held to RTOL
    relative by its own parity test, so their difference is held to RTOL (nested_rhat^2 + rhat^2)."""
    from aehmc_amd import summary
    x = dev(nr.draws(40 + N + C, N, C, 1, D))
    nested = summary.nested_rhat(x, C).nested_rhat ** 2
    classical = summary.summarize(x, split=False).rhat ** 2
    err = (nested - classical - 1.0 / N).abs()
    print("max |nested^2 - rhat^2 - 1/N|", err.max().item(), "squares up to", nested.max().item())
    assert bool((err <= RTOL * (nested + classical)).all())


def test_degenerate_and_non_finite_input():
    """One coordinate each: all draws constant -> NaN; chains constant inside superchains that differ -> +inf; equal
    superchain means with spread -> exactly 1.0; one NaN draw -> that coordinate and window NaN, everything else
    bit-equal to the run without it -- fed whole and one draw at a time."""
    from aehmc_amd import summary
    N, K, M, D, w = 6, 3, 4, 6, 2
    x = nr.draws(77, N, K, M, D, offset=100.0).reshape(N, K, M, D)
    x[..., 1] = 7.25
    x[..., 2] = np.arange(K).reshape(1, K, 1) * 1.5 - 100.0
    x[..., 3] = x[:, :1, :, 3]  # the superchains are copies of the first
    x = x.reshape(N, K * M, D)
    clean = summary.nested_rhat(dev(x), K, window=w)
    r = clean.nested_rhat.cpu().numpy()
    assert np.isnan(r[:, 1]).all() and np.all(clean.between.cpu().numpy()[:, 1] == 0.0)
    assert np.all(np.isposinf(r[:, 2])) and np.all(clean.within.cpu().numpy()[:, 2] == 0.0)
    assert np.all(r[:, 3] == 1.0) and np.all(clean.between.cpu().numpy()[:, 3] == 0.0)
    assert np.all(clean.within.cpu().numpy()[:, 3] > 0.0) and np.all(clean.mcse_superchains.cpu().numpy()[:, 3] == 0.0)
    assert np.isfinite(r[:, [0, 4, 5]]).all()
    # (not coordinate 3: the restatement's mean of K equal means need not be that mean to the last bit)
    cols = [0, 1, 2, 4, 5]
    against_restatement(types.SimpleNamespace(**{f: getattr(clean, f)[:, cols] for f in TENSORS}),
                        nr.nested_rhat(x[:, :, cols], K, w), (N // w, len(cols)))
    bad = x.copy()
    bad[2, 5, 4] = np.nan  # first draw of window 1, chain 5, coordinate 4
    xb = dev(bad)
    for chunk in (N, 1):
        acc = summary.NestedAccumulator(N, K * M, (D,), K, window=w)
        for lo in range(0, N, chunk):
            acc.update(xb[lo:lo + chunk])
        res = acc.result()
        hit = torch.zeros(N // w, D, dtype=torch.bool, device="cuda")
        hit[1, 4] = True
        for f in TENSORS:
            got, want = getattr(res, f), getattr(clean, f)
            assert bool(torch.isnan(got[hit]).all()), f
            assert same_bits(got[~hit], want[~hit]), f


def _superchain_run(seed, K, M, D, spread):
    """A DiagGaussian target, its scales, and K M chains started as K superchains `spread` standard deviations out."""
    from aehmc_amd import nuts, summary, targets
    r = np.random.default_rng(seed)
    mu, sigma = r.normal(size=D) * 2.0, 0.5 + r.random(D)
    starts = mu + spread * sigma * r.normal(size=(K, D))
    tgt = targets.DiagGaussian(mu, sigma)
    q0 = summary.superchain_positions(dev(starts), chains_per_superchain=M)
    assert q0.shape == (K * M, D)
    return tgt, sigma, nuts.new_state(q0, tgt)


def test_run_feeds_the_accumulator():
    """summary.run(nested=acc) against kernel.sample + nested_rhat on the stored draws, kernels of the same seeds: the
    nested results are bit-equal, and what run returns is bit-equal to a run without the sink."""
    from aehmc_amd import RandomStream, nuts, summary
    K, M, D, N, w = 4, 4, 3, 12, 3
    tgt, sigma, state = _superchain_run(5, K, M, D, 3.0)
    k1, k2, k3 = (nuts.new_kernel(RandomStream(seeds=[40_000 + c for c in range(K * M)]), tgt) for _ in range(3))
    samples, *_ = k1.sample(state, 0.3, sigma**2, N)
    want = summary.nested_rhat(samples, K, window=w)
    acc = summary.NestedAccumulator(N, K * M, (D,), K, window=w)
    with_sink = summary.run(k2, state, 0.3, sigma**2, N, chunk=5, nested=acc)
    without = summary.run(k3, state, 0.3, sigma**2, N, chunk=5)
    got = acc.result()
    for f in TENSORS:
        assert same_bits(getattr(got, f), getattr(want, f)), f
    assert bool(torch.isfinite(got.nested_rhat).all())
    for f in ("mean", "sd", "rhat", "ess_chains", "mcse_chains"):
        assert same_bits(getattr(with_sink[0], f), getattr(without[0], f)), f
    for f in ("position", "potential_energy", "potential_energy_grad"):
        assert same_bits(getattr(with_sink[1].state, f), getattr(without[1].state, f)), f
    assert torch.equal(with_sink[1].n_leapfrog, without[1].n_leapfrog)
    assert same_bits(with_sink[2], without[2]) and torch.equal(with_sink[3], without[3])
    with pytest.raises(ValueError, match="more exceed"):
        summary.run(k3, state, 0.3, sigma**2, N, nested=acc)


def test_trace_shows_when_the_warmup_was_long_enough():
    """K = 8 superchains of M = 64 chains on a 5-dimensional DiagGaussian, started with superchain_positions from points
    drawn at 10 standard deviations; NUTS with a small step budget (8 leapfrogs of 0.08 in the target's own scales),
    traced in windows of 4 transitions.  First window: the superchain means still sit near their starts, ten within-sd
    apart, nested_rhat > 2 in every coordinate.  Last window: nested_rhat < sqrt(1 + 10 / (M window)) = 1.0193, ten times
    the between / within of independent draws.

    80 transitions, not 40: with this budget a transition keeps about 0.9 of a chain's distance to the mode, and the
    restated sampler (oracle/c_oracle.py, seeds 0 ... 2 of this set-up) gave 2.8 ... 4.3 for the smallest first-window
    value and at most 1.013 over the last three windows at 80 transitions; at 40 transitions with a budget large enough
    to arrive (8 leapfrogs of 0.1) the first window fell to 2.03 on one seed.  The bounds are the issue's."""
    from aehmc_amd import RandomStream, nuts, summary
    K, M, D, N, w = 8, 64, 5, 80, 4
    tgt, sigma, state = _superchain_run(0, K, M, D, 10.0)
    kernel = nuts.new_kernel(RandomStream(seeds=[70_000 + c for c in range(K * M)]), tgt, max_num_expansions=3)
    acc = summary.NestedAccumulator(N, K * M, (D,), K, window=w)
    summary.run(kernel, state, 0.08, sigma**2, N, nested=acc)
    tr = acc.result().nested_rhat
    assert tr.shape == (N // w, D)
    print("first window", tr[0].cpu().numpy(), "last window", tr[-1].cpu().numpy(),
          "largest per window", tr.max(dim=1).values.cpu().numpy())
    assert bool((tr[0] > 2.0).all())
    assert bool((tr[-1] < np.sqrt(1.0 + 10.0 / (M * w))).all())
