"""Order statistics, quantiles, intervals and tail ESS on the device (aehmc_amd/summary.py over csrc/quantile.cuh)
against np.sort, numpy.quantile and the numpy restatement of tests/quantile_ref.py."""
import functools
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import quantile_ref as qr  # noqa: E402
import summary_ref as sr  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

RTOL = 1e-9  # the project's parity tolerance
EPS = np.finfo(np.float64).eps
PROBS = (0.0, 0.05, 0.25, 1.0 / 3.0, 0.5, 0.95, 1.0)
# (N, C, D, layout): R = N C in {1, 15, 1961, 25664, 16384, 129}; D = 17 and 65 straddle tiles of 16 coordinates
SHAPES = [(1, 1, 1, "N"), (5, 3, 2, "NCD"), (37, 53, 17, "NCD"), (401, 64, 100, "NCD"), (4, 4096, 1, "NC"),
          (129, 1, 65, "ND")]


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def host(t):
    return t.cpu().numpy()


def laid_out(x, N, C, D, layout):
    """x [N C, D] on the device in the layout's view, with what the calls need to read it."""
    view = {"N": (N,), "NC": (N, C), "ND": (N, D), "NCD": (N, C, D)}[layout]
    shape = {"N": (), "NC": (), "ND": (D,), "NCD": (D,)}[layout]
    return dev(x).reshape(view), shape, dict(batched=layout in ("NC", "NCD"))


@functools.lru_cache(maxsize=None)
def draws(N, C, D):
    """(x [R, D], np.sort(x, 0)): normal draws with a location and a scale per coordinate; never written to."""
    r = np.random.default_rng(9000 + N + C + D)
    x = r.normal(size=(N * C, D)) * (0.5 + r.random(D)) + r.normal(size=D) * 3.0
    s = np.sort(x, axis=0)
    x.setflags(write=False)
    s.setflags(write=False)
    return x, s


def ranks_of(R):
    if R <= 15:
        return list(range(R))
    r = np.random.default_rng(R)
    return [0, 1, R // 2, R - 2, R - 1] + [int(v) for v in r.integers(0, R, size=9)]


@pytest.mark.parametrize("N,C,D,layout", SHAPES)
def test_selection_to_the_bit(N, C, D, layout):
    from aehmc_amd import summary
    x, s = draws(N, C, D)
    ranks = ranks_of(N * C)
    t, shape, kw = laid_out(x, N, C, D, layout)
    got = host(summary.order_statistics(t, ranks, **kw))
    assert got.shape == (len(ranks),) + shape
    assert np.array_equal(bits(got).reshape(len(ranks), D), bits(s[ranks]))


def hard_values():
    """[37 * 53, 17]: coordinate 0 all equal, 1 two values in equal numbers (R is odd: one more of the first), 2 the
    negation of 3, 4 magnitudes from 1e-310 to 1e300 with both signs, 5 a few +-inf, 6 zeros of both signs, 7 the
    integers 0 ... R - 1 shuffled; the rest as drawn."""
    R = 37 * 53
    r = np.random.default_rng(4242)
    x = r.normal(size=(R, 17))
    x[:, 0] = 2.5
    x[:, 1] = np.where(np.arange(R) % 2 == 0, -1.25, 3.0)
    r.shuffle(x[:, 1])
    x[:, 2] = -x[:, 3]
    x[:, 4] = r.choice([-1.0, 1.0], size=R) * 10.0 ** r.uniform(-310, 300, size=R)
    x[:4, 4] = [1e-310, -1e-310, 1e300, -1e300]
    x[r.choice(R, size=7, replace=False), 5] = [np.inf, np.inf, np.inf, -np.inf, -np.inf, np.inf, -np.inf]
    x[:, 6] = np.where(r.random(R) < 0.5, 0.0, -0.0)
    x[:, 7] = r.permutation(R)
    return x


def test_hard_values_to_the_bit():
    from aehmc_amd import summary
    x = hard_values()
    R = x.shape[0]
    assert np.any((np.abs(x[:, 4]) < 2.3e-308) & (x[:, 4] != 0)), "no denormal among the magnitudes"
    s = np.sort(x, axis=0)
    ranks = ranks_of(R)
    got = host(summary.order_statistics(dev(x).reshape(37, 53, 17), ranks))
    other = [d for d in range(17) if d != 6]
    assert np.array_equal(bits(got[:, other]), bits(s[ranks][:, other]))
    assert np.all(got[:, 6] == s[ranks, 6])  # zeros of both signs: equal as values (np.sort leaves their order open)
    assert np.array_equal(got[:, 7], np.asarray(ranks, dtype=np.float64))
    # every rank of the shuffled integers is its own answer, 64 ranks a call
    every = np.arange(R)
    for lo in range(0, R, 640):
        part = [int(v) for v in every[lo:lo + 640:10]]
        assert np.array_equal(host(summary.order_statistics(dev(x[:, 7]), part, batched=False)),
                              np.asarray(part, dtype=np.float64))


def test_nan_poisons_its_coordinate_only():
    from aehmc_amd import summary
    x, _ = draws(37, 53, 17)
    y = x.copy()
    y[1234, 3] = np.nan
    ranks = ranks_of(37 * 53)
    clean_r, clean_q = (host(f) for f in (summary.order_statistics(dev(x).reshape(37, 53, 17), ranks),
                                          summary.quantiles(dev(x).reshape(37, 53, 17), PROBS)))
    got_r = host(summary.order_statistics(dev(y).reshape(37, 53, 17), ranks))
    got_q = host(summary.quantiles(dev(y).reshape(37, 53, 17), PROBS))
    other = [d for d in range(17) if d != 3]
    assert np.isnan(got_r[:, 3]).all() and np.isnan(got_q[:, 3]).all()
    assert np.array_equal(bits(got_r[:, other]), bits(clean_r[:, other]))
    assert np.array_equal(bits(got_q[:, other]), bits(clean_q[:, other]))
    assert np.array_equal(bits(got_q[:, other]), bits(qr.quantiles(y, PROBS)[:, other]))


@pytest.mark.parametrize("N,C,D,layout", SHAPES)
def test_quantiles(N, C, D, layout):
    """Bit-equal to the restatement; within 4 eps max(|a|, |b|) of numpy.quantile (one multiply and one add on
    operands no larger than the two order statistics a, b); median is the row of 0.5; interval(0.9) is the pair of
    quantiles at (1 - 0.9) / 2 and (1 + 0.9) / 2 as floating point has them -- the latter is 0.95 itself, the former is
    one ulp below 0.05 --; a scalar probs drops the leading axis."""
    from aehmc_amd import summary
    x, s = draws(N, C, D)
    R = N * C
    t, shape, kw = laid_out(x, N, C, D, layout)
    got = host(summary.quantiles(t, PROBS, **kw))
    assert got.shape == (len(PROBS),) + shape
    got2 = got.reshape(len(PROBS), D)
    assert np.array_equal(bits(got2), bits(qr.quantiles(x, PROBS)))
    want = np.quantile(x, PROBS, axis=0)
    lo = np.array([int(math.floor(p * (R - 1))) for p in PROBS])
    bound = 4 * EPS * np.maximum(np.abs(s[lo]), np.abs(s[np.minimum(lo + 1, R - 1)]))
    err = np.abs(got2 - want)
    print("max err / bound against numpy.quantile", np.max(err / bound))
    assert np.all(err <= bound)
    med = summary.median(t, **kw)
    assert tuple(med.shape) == shape and np.array_equal(bits(host(med)).ravel(), bits(got2[4]))
    one = summary.quantiles(t, 0.25, **kw)
    assert tuple(one.shape) == shape and np.array_equal(bits(host(one)).ravel(), bits(got2[2]))
    ends = ((1.0 - 0.9) / 2.0, (1.0 + 0.9) / 2.0)
    lower, upper = summary.interval(t, 0.9, **kw)
    assert tuple(lower.shape) == tuple(upper.shape) == shape
    pair = host(summary.quantiles(t, ends, **kw)).reshape(2, D)
    assert np.array_equal(bits(pair), bits(qr.quantiles(x, ends)))
    assert np.array_equal(bits(host(lower)).ravel(), bits(pair[0]))
    assert np.array_equal(bits(host(upper)).ravel(), bits(pair[1]))
    assert ends[1] == 0.95 and np.array_equal(bits(pair[1]), bits(got2[5]))


def test_determinism_and_sweeps():
    """Two calls give the same bits; twenty probs (more than one sweep's worth of ranks) give the bits of the same
    probs asked for one at a time."""
    from aehmc_amd import summary
    x, _ = draws(37, 53, 17)
    t = dev(x).reshape(37, 53, 17)
    probs = [float(p) for p in np.random.default_rng(20).random(20)]
    a, b = summary.quantiles(t, probs), summary.quantiles(t, probs)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    singles = torch.stack([summary.quantiles(t, p) for p in probs])
    assert torch.equal(a.view(torch.int64), singles.view(torch.int64))
    assert np.array_equal(bits(host(a)), bits(qr.quantiles(x, probs)))
    ranks = ranks_of(37 * 53)
    r1, r2 = summary.order_statistics(t, ranks), summary.order_statistics(t, ranks)
    assert torch.equal(r1.view(torch.int64), r2.view(torch.int64))


@pytest.mark.parametrize("seed,N,C,D", [(11, 200, 16, 5), (12, 101, 7, 3), (13, 400, 64, 17)])
def test_tail_ess_against_restatement(seed, N, C, D):
    from aehmc_amd import summary
    r = np.random.default_rng(seed)
    phi = r.uniform(-0.3, 0.8, D)
    loc = r.normal(size=D) * 3
    scale = 0.5 + r.random(D)
    x = sr.ar1(r, N, C, D, phi, loc=loc, scale=scale)
    want, near, _ = qr.tail_ess(x)
    assert not near.any(), "a deciding pair sum of the restatement lies within 1e-9 of zero: pick another seed"
    got = host(summary.tail_ess(dev(x)))
    assert got.shape == (D,)
    rel = np.abs(got - want) / np.abs(want)
    print("tail ess", got, "max rel err", rel.max())
    assert np.all(rel <= RTOL)


def test_end_to_end_interval_of_a_gaussian():
    """NUTS on N(mu, diag sigma^2), D = 4, 256 chains, step size 0.5, unit metric, 200 draws after 50 discarded: each
    end of interval(0.9) lies within five standard errors of a sample quantile, 5 sd sqrt(p (1 - p) / ess_tail) /
    phi(1.645) with p = 0.05, of mu -+ 1.645 sigma."""
    from aehmc_amd import RandomStream, nuts, summary, targets
    r = np.random.default_rng(21)
    C, D = 256, 4
    mu, sigma = r.normal(size=D) * 2.0, 0.5 + r.random(D)
    tgt = targets.DiagGaussian(mu, sigma)
    kernel = nuts.new_kernel(RandomStream(seeds=[50_000 + c for c in range(C)]), tgt)
    state = nuts.new_state(dev(mu + sigma * r.normal(size=(C, D))), tgt)
    imm = np.ones(D)
    _, info, _, _ = kernel.sample(state, 0.5, imm, 50)
    samples, _, _, _ = kernel.sample(info.state._replace(momentum=None), 0.5, imm, 200)
    assert tuple(samples.shape) == (200, C, D)
    ess_tail = host(summary.tail_ess(samples))
    assert np.all(np.isfinite(ess_tail) & (ess_tail > 0)), ess_tail
    sd = host(summary.summarize(samples).sd)
    lower, upper = (host(v) for v in summary.interval(samples, 0.9))
    dens = math.exp(-0.5 * 1.645**2) / math.sqrt(2.0 * math.pi)
    tol = 5.0 * sd * np.sqrt(0.05 * 0.95 / ess_tail) / dens
    print("tail ess", ess_tail, "lower err / tol", (lower - (mu - 1.645 * sigma)) / tol, "upper err / tol",
          (upper - (mu + 1.645 * sigma)) / tol)
    assert np.all(np.abs(lower - (mu - 1.645 * sigma)) <= tol)
    assert np.all(np.abs(upper - (mu + 1.645 * sigma)) <= tol)
