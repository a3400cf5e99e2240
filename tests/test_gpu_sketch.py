"""The streaming quantile sketch on the device (summary.QuantileSketch and summary.run(sketch=...) over csrc/sketch.cuh)
against the numpy restatement of tests/sketch_ref.py, which tests/test_sketch_host.py pins on the CPU."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sketch_ref as sk  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

RTOL = 1e-9  # the project's parity tolerance


def dev(a):
    return torch.as_tensor(np.array(a, dtype=np.float64), device="cuda")  # (a copy: the shared draws are read-only)


def host(t):
    return t.cpu().numpy()


def same_bits(a, b):
    return torch.equal(a.view(torch.int64), b.view(torch.int64))


@functools.lru_cache(maxsize=None)
def narrow_grid(N, C, D):
    """An explicit grid that leaves draws on both sides: one unit below to one and a half above the column means."""
    m = sk.draws(N, C, D).mean(axis=0)
    return m - 1.0, m + 1.5


@functools.lru_cache(maxsize=None)
def reference(N, C, D, B, fitted):
    """(lo, hi, counts, estimate, resolved) of the restatement; computed once, never written to."""
    x = sk.draws(N, C, D)
    lo, hi = sk.fit_grid(x) if fitted else narrow_grid(N, C, D)
    cnt = sk.counts(x, lo, hi, B)
    est, res, _ = sk.quantiles(cnt, lo, hi, B, sk.PROBS)
    for a in (lo, hi, cnt, est, res):
        a.setflags(write=False)
    return lo, hi, cnt, est, res


def folded(N, C, D, B, fitted):
    from aehmc_amd import summary
    x = dev(sk.draws(N, C, D)).reshape(N, C, D)
    grid = None if fitted else tuple(dev(v) for v in narrow_grid(N, C, D))
    return summary.QuantileSketch(C, (D,), bins=B, grid=grid).update(x), x


@pytest.mark.parametrize("fitted", [False, True], ids=["explicit", "fitted"])
@pytest.mark.parametrize("B", sk.BINS)
@pytest.mark.parametrize("N,C,D", sk.SHAPES)
def test_counts_and_quantiles_against_restatement(N, C, D, B, fitted):
    """counts to the bit (and the fitted edges); estimates to RTOL and `resolved` equal; a resolved estimate within
    `bound` of the exact quantile of the same stored draws; median and interval are rows of quantiles."""
    from aehmc_amd import summary
    lo, hi, cnt, est, res = reference(N, C, D, B, fitted)
    s, x = folded(N, C, D, B, fitted)
    assert np.array_equal(host(s.lo).view(np.int64), lo.view(np.int64))
    assert np.array_equal(host(s.hi).view(np.int64), hi.view(np.int64))
    assert s.counts.dtype == torch.int64 and tuple(s.counts.shape) == (D, B + 3)
    assert torch.equal(s.counts.cpu(), torch.from_numpy(cnt.copy()))
    assert s.num_draws == N * C
    got, ok = s.quantiles(sk.PROBS), s.resolved(sk.PROBS)
    assert tuple(got.shape) == tuple(ok.shape) == (len(sk.PROBS), D) and ok.dtype == torch.bool
    assert np.array_equal(host(ok), res)
    np.testing.assert_allclose(host(got), est, rtol=RTOL, atol=0.0, equal_nan=True)
    bound = host(s.bound)
    assert np.array_equal(bound, (hi - lo) / B)
    exact = host(summary.quantiles(x, sk.PROBS))
    err = np.abs(host(got) - exact)
    print("resolved", res.mean(), "worst error / bound where resolved", np.max(np.where(res, err / bound, 0.0)))
    assert np.all(err[res] <= np.broadcast_to(bound, err.shape)[res])
    if fitted:
        inner = [i for i, p in enumerate(sk.PROBS) if 0.05 <= p <= 0.95]
        assert res[inner].all()
    assert same_bits(s.median(), got[4])
    one = s.quantiles(0.25)
    assert tuple(one.shape) == (D,) and same_bits(one, got[2]) and tuple(s.resolved(0.25).shape) == (D,)
    lower, upper = s.interval(0.9)
    pair = s.quantiles(((1.0 - 0.9) / 2.0, (1.0 + 0.9) / 2.0))
    assert same_bits(lower, pair[0]) and same_bits(upper, pair[1]) and same_bits(upper, got[5])


def test_scalar_positions_and_one_chain_without_its_axis():
    from aehmc_amd import summary
    x = dev(sk.draws(4, 4096, 1))
    s = summary.QuantileSketch(4096, ()).update(x.reshape(4, 4096))
    assert torch.equal(s.counts.cpu(), torch.from_numpy(reference(4, 4096, 1, 2048, True)[2].copy()))
    assert tuple(s.quantiles(sk.PROBS).shape) == (len(sk.PROBS),) and tuple(s.median().shape) == ()
    assert tuple(s.bound.shape) == () and tuple(s.resolved(0.5).shape) == ()
    y = dev(sk.draws(129, 1, 65))
    s = summary.QuantileSketch(1, (65,), bins=4096).update(y.reshape(129, 65))
    assert torch.equal(s.counts.cpu(), torch.from_numpy(reference(129, 1, 65, 4096, True)[2].copy()))


def test_chunking_changes_nothing():
    from aehmc_amd import summary
    N, C, D = 37, 53, 17
    x = dev(sk.draws(N, C, D)).reshape(N, C, D)
    lo, hi = (dev(v) for v in sk.fit_grid(sk.draws(N, C, D)))
    whole = summary.QuantileSketch(C, (D,), grid=(lo, hi)).update(x)
    want = whole.quantiles(sk.PROBS)
    for cuts in ([1] * N, [5, 1, 31]):
        s = summary.QuantileSketch(C, (D,), grid=(lo, hi))
        t = 0
        for n in cuts:
            s.update(x[t:t + n])
            t += n
        assert t == N and torch.equal(s.counts, whole.counts)
        assert same_bits(s.quantiles(sk.PROBS), want)


def test_edge_values():
    """grid (0, 64) in 64 bins: width 1, everything exact."""
    from aehmc_amd import summary
    B = 64
    v = np.array([float(i) for i in range(64)] + [64.0, np.inf, -0.0, -1e-300, -np.inf, np.nan])
    x = np.stack([v, np.arange(70.0) % 64], axis=1)
    s = summary.QuantileSketch(1, (2,), bins=B, grid=(0.0, 64.0)).update(dev(x))
    cnt = host(s.counts)
    want0 = np.ones(B + 3, dtype=np.int64)
    want0[0] = 2    # -1e-300, -inf
    want0[1] = 2    # 0.0, -0.0
    want0[65] = 2   # 64.0, +inf
    want0[66] = 1   # NaN
    want1 = np.zeros(B + 3, dtype=np.int64)
    want1[1:65] = 1
    want1[1:7] = 2
    assert cnt[0].tolist() == want0.tolist() and cnt[1].tolist() == want1.tolist()
    assert np.array_equal(cnt, sk.counts(x, np.zeros(2), np.full(2, 64.0), B))
    q, ok = host(s.quantiles((0.25, 0.5))), host(s.resolved((0.25, 0.5)))
    assert np.isnan(q[:, 0]).all() and not ok[:, 0].any()
    est, res, _ = sk.quantiles(cnt, np.zeros(2), np.full(2, 64.0), B, (0.25, 0.5))
    assert ok[:, 1].all() and res[:, 1].all()
    np.testing.assert_allclose(q[:, 1], est[:, 1], rtol=RTOL, atol=0.0)
    assert host(s.bound).tolist() == [1.0, 1.0]


def test_counters_carry_into_the_upper_word():
    from aehmc_amd import summary
    s = summary.QuantileSketch(1, (2,), bins=64, grid=(0.0, 64.0))
    s.counts[0, 6] += 2**32 - 5
    s.update(dev(np.full((10, 2), 5.5)))
    assert int(s.counts[0, 6].item()) == 2**32 + 5 and int(s.counts[1, 6].item()) == 10
    assert int(s.counts.sum().item()) == 2**32 + 15 and s.num_draws == 2**32 + 5


def test_merge():
    from aehmc_amd import summary
    N, C, D = 37, 53, 17
    x = dev(sk.draws(N, C, D)).reshape(N, C, D)
    lo, hi = (dev(v) for v in sk.fit_grid(sk.draws(N, C, D)))
    whole = summary.QuantileSketch(C, (D,), grid=(lo, hi)).update(x)
    a = summary.QuantileSketch(C, (D,), grid=(lo, hi)).update(x[:18])
    b = summary.QuantileSketch(C, (D,), grid=(lo, hi)).update(x[18:])
    assert a.merge(b) is a and torch.equal(a.counts, whole.counts)
    assert same_bits(a.quantiles(sk.PROBS), whole.quantiles(sk.PROBS))
    moved = summary.QuantileSketch(C, (D,), grid=(lo, torch.nextafter(hi, hi + 1.0))).update(x[:2])
    with pytest.raises(ValueError, match="bit-equal"):
        a.merge(moved)
    with pytest.raises(ValueError, match="do not merge"):
        a.merge(summary.QuantileSketch(C, (D,), bins=1024, grid=(lo, hi)))
    with pytest.raises(ValueError, match="need their grid"):
        a.merge(summary.QuantileSketch(C, (D,)))
    assert torch.equal(a.counts, whole.counts)


def test_run_feeds_the_sketch_and_changes_nothing_else():
    """summary.run(chunk=7, sketch=sk) on NUTS, N(mu, diag sigma^2), 64 chains, D = 17, 40 draws: everything returned,
    the chain states and the generator states have the bits of a twin run without the sketch; the sketch holds the counts
    of the stored draws of a third twin's kernel.sample on the same grid."""
    from aehmc_amd import RandomStream, nuts, summary, targets
    r = np.random.default_rng(77)
    C, D, N = 64, 17, 40
    mu, sigma = r.normal(size=D) * 2.0, 0.5 + r.random(D)
    tgt = targets.DiagGaussian(mu, sigma)
    state = nuts.new_state(dev(mu + sigma * r.normal(size=(C, D))), tgt)
    k1, k2, k3 = (nuts.new_kernel(RandomStream(seeds=[70_000 + c for c in range(C)]), tgt) for _ in range(3))
    args = (0.3, sigma**2)
    s = summary.QuantileSketch(C, (D,))
    got, info, acc, div = summary.run(k1, state, *args, N, chunk=7, sketch=s)
    want, info2, acc2, div2 = summary.run(k2, state, *args, N, chunk=7)
    for f in want._fields:
        a, b = getattr(got, f), getattr(want, f)
        assert same_bits(a, b) if isinstance(b, torch.Tensor) else a == b, f
    for f in ("position", "potential_energy", "potential_energy_grad", "momentum"):
        assert same_bits(getattr(info.state, f), getattr(info2.state, f)), f
    assert same_bits(info.acceptance_probability, info2.acceptance_probability)
    assert torch.equal(info.is_diverging, info2.is_diverging) and torch.equal(info.n_leapfrog, info2.n_leapfrog)
    assert same_bits(acc, acc2) and torch.equal(div, div2)
    assert torch.equal(k1._nuts["holder"]["rng"], k2._nuts["holder"]["rng"])
    samples = k3.sample(state, *args, N)[0]
    stored = summary.QuantileSketch(C, (D,), grid=(s.lo, s.hi)).update(samples)
    assert s.num_draws == N * C and torch.equal(s.counts, stored.counts)
    lo, hi = sk.fit_grid(host(samples[:7]).reshape(7 * C, D))
    assert np.array_equal(host(s.lo).view(np.int64), lo.view(np.int64))
    assert np.array_equal(host(s.hi).view(np.int64), hi.view(np.int64))
    with pytest.raises(ValueError, match="sketch must be"):
        summary.run(k1, state, *args, N, sketch=summary.QuantileSketch(C, (D + 1,)))


def test_errors_before_any_launch():
    from aehmc_amd import summary
    C, D = 3, 2
    for bins in (0, 32, 100, 8192, 2047, 2.5):
        with pytest.raises(ValueError, match="bins must be"):
            summary.QuantileSketch(C, (D,), bins=bins)
    for grid in ((1.0, 1.0), (2.0, 1.0), (0.0, float("inf")), (float("nan"), 1.0), (float("-inf"), 0.0),
                 (dev([0.0, 1.0]), dev([1.0, 1.0]))):
        with pytest.raises(ValueError, match="finite edges with lo < hi"):
            summary.QuantileSketch(C, (D,), grid=grid)
    with pytest.raises(ValueError, match="grid lo must be"):
        summary.QuantileSketch(C, (D,), grid=(dev([0.0, 1.0, 2.0]), 5.0))
    with pytest.raises(ValueError, match="pair"):
        summary.QuantileSketch(C, (D,), grid=1.0)
    with pytest.raises(ValueError, match="span must be"):
        summary.QuantileSketch(C, (D,), span=0.0)
    s = summary.QuantileSketch(C, (D,), grid=(-4.0, 4.0))
    x = dev(np.random.default_rng(5).normal(size=(5, C, D)))
    with pytest.raises(ValueError, match="chunk must be"):
        s.update(x[:, :C - 1].contiguous())
    with pytest.raises(ValueError, match="float64"):
        s.update(x.float())
    with pytest.raises(ValueError, match="must be on"):
        s.update(x.cpu())
    with pytest.raises(ValueError, match="no draw"):
        s.quantiles(0.5)
    with pytest.raises(ValueError, match="no draw"):
        s.resolved(0.5)
    assert int(s.counts.sum().item()) == 0
    s.update(x)
    with pytest.raises(ValueError, match="before the first update"):
        s.fit(x)
    for probs in (1.5, (), float("nan")):
        with pytest.raises(ValueError, match="probs"):
            s.quantiles(probs)
    fitted = summary.QuantileSketch(C, (D,)).fit(x)
    assert int(fitted.counts.sum().item()) == 0 and fitted.lo is not None
    lo, hi = sk.fit_grid(host(x).reshape(5 * C, D))
    assert np.array_equal(host(fitted.lo).view(np.int64), lo.view(np.int64))
    assert np.array_equal(host(fitted.hi).view(np.int64), hi.view(np.int64))
