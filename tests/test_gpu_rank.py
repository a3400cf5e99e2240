"""Average ranks, normal scores and the rank-normalised diagnostics on the device (aehmc_amd/summary.py over
csrc/rank.cuh) against the reference pipeline of tests/rank_ref.py (scipy's rankdata and ndtri, numpy's median, the
numpy restatement of the estimators)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rank_ref as rr  # noqa: E402
import summary_ref as sr  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

RTOL = 1e-9  # the project's parity tolerance
# (N, C, D, layout): S = N C in {4, 15, 1961, 129, 32768, 25664, 262144}.  The scatter's workgroup takes a chunk of
# 4096 keys of a column in rounds of 1024: S = 1961 is the first with two rounds, (8, 4096, 1) the first with several
# chunks (8) a column; D = 17 and 33 are one past tiles of 16 coordinates.
SHAPES = [(4, 1, 1, "N"), (5, 3, 2, "NCD"), (37, 53, 17, "NCD"), (129, 1, 65, "ND"), (8, 4096, 1, "NC"),
          (401, 64, 33, "NCD"), (64, 4096, 3, "NCD")]
ESTIMATOR_SHAPES = [(5, 3, 2), (37, 53, 17), (401, 64, 33), (129, 1, 65), (1000, 3, 16), (64, 4096, 3)]
REALS = ("rhat", "rhat_bulk", "rhat_folded", "ess_bulk", "ess_tail")


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def host(t):
    return t.cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def laid_out(x, N, C, D, layout):
    """x [N C, D] on the device in the layout's view, with what the calls need to read it."""
    view = {"N": (N,), "NC": (N, C), "ND": (N, D), "NCD": (N, C, D)}[layout]
    return dev(x).reshape(view), view, dict(batched=layout in ("NC", "NCD"))


@functools.lru_cache(maxsize=None)
def draws(N, C, D):
    """(x [S, D], its ranks, its normal scores by the reference): normal draws with a location and a scale per
    coordinate; never written to."""
    r = np.random.default_rng(9100 + N + C + D)
    x = r.normal(size=(N * C, D)) * (0.5 + r.random(D)) + r.normal(size=D) * 3.0
    rk = rr.ranks(x)
    z = rr.scores(rk)
    for a in (x, rk, z):
        a.setflags(write=False)
    return x, rk, z


def close(got, want):
    rel = np.abs(got - want) / np.where(want != 0, np.abs(want), 1.0)
    print("max rel err", rel.max())
    return np.all(rel <= RTOL)


@pytest.mark.parametrize("N,C,D,layout", SHAPES)
def test_ranks_to_the_bit(N, C, D, layout):
    from aehmc_amd import summary
    x, rk, _ = draws(N, C, D)
    t, view, kw = laid_out(x, N, C, D, layout)
    got = host(summary.ranks(t, **kw))
    assert got.shape == view
    assert np.array_equal(bits(got).reshape(N * C, D), bits(rk))


def hard_values():
    """[37 * 53, 17]: coordinate 0 all equal, 1 two values in unequal numbers, 2 the negation of 3, 4 magnitudes from
    1e-310 to 1e300 with both signs, 5 a few +-inf, 6 zeros of both signs, 7 the integers 0 ... S - 1 shuffled, 8 a few
    values many times each; the rest as drawn."""
    S = 37 * 53
    r = np.random.default_rng(4343)
    x = r.normal(size=(S, 17))
    x[:, 0] = 2.5
    x[:, 1] = np.where(np.arange(S) % 3 == 0, -1.25, 3.0)
    r.shuffle(x[:, 1])
    x[:, 2] = -x[:, 3]
    x[:, 4] = r.choice([-1.0, 1.0], size=S) * 10.0 ** r.uniform(-310, 300, size=S)
    x[:4, 4] = [1e-310, -1e-310, 1e300, -1e300]
    x[r.choice(S, size=7, replace=False), 5] = [np.inf, np.inf, np.inf, -np.inf, -np.inf, np.inf, -np.inf]
    x[:, 6] = np.where(r.random(S) < 0.5, 0.0, -0.0)
    x[:, 7] = r.permutation(S)
    x[:, 8] = r.choice([-2.0, -0.0, 0.0, 1e-320, 7.0], size=S)
    return x


def test_hard_values_to_the_bit():
    from aehmc_amd import summary
    x = hard_values()
    S = x.shape[0]
    assert np.any((np.abs(x[:, 4]) < 2.3e-308) & (x[:, 4] != 0)), "no denormal among the magnitudes"
    assert np.signbit(x[:, 6]).any() and not np.signbit(x[:, 6]).all()
    want = rr.ranks(x)
    got = host(summary.ranks(dev(x).reshape(37, 53, 17))).reshape(S, 17)
    assert np.array_equal(bits(got), bits(want))
    assert np.all(got[:, 0] == (S + 1) / 2) and np.all(got[:, 6] == (S + 1) / 2)
    assert np.array_equal(got[:, 7], x[:, 7] + 1.0)
    assert np.array_equal(got[:, 2], S + 1 - got[:, 3])
    # one NaN: its coordinate is all NaN, every other coordinate keeps its bits
    y = x.copy()
    y[1234, 9] = np.nan
    for mode in (summary.ranks, summary.rank_normalize):
        clean, poisoned = (host(mode(dev(v).reshape(37, 53, 17))).reshape(S, 17) for v in (x, y))
        other = [d for d in range(17) if d != 9]
        assert np.isnan(poisoned[:, 9]).all()
        assert np.array_equal(bits(poisoned[:, other]), bits(clean[:, other]))


@pytest.mark.parametrize("N,C,D,layout", SHAPES)
def test_normal_scores(N, C, D, layout):
    from aehmc_amd import summary
    x, rk, z = draws(N, C, D)
    S = N * C
    t, view, kw = laid_out(x, N, C, D, layout)
    got = host(summary.rank_normalize(t, **kw))
    assert got.shape == view
    got = got.reshape(S, D)
    assert close(got, z)
    if S % 2:
        assert np.all(got[rk == (S + 1) / 2] == 0.0) and np.sum(rk == (S + 1) / 2) == D
    # the draws are tie-free: the scores of the negated draws are the negated scores
    assert np.all(np.diff(np.sort(x, axis=0), axis=0) > 0)
    neg = host(summary.rank_normalize(-t, **kw)).reshape(S, D)
    assert close(neg, -got)


@pytest.mark.parametrize("N,C,D,layout", [(5, 3, 2, "NCD"), (37, 53, 17, "NCD"), (129, 1, 65, "ND"),
                                          (8, 4096, 1, "NC")])
def test_fold(N, C, D, layout):
    """The ranks of the draws folded about the median that the device computes are the reference's ranks of
    |x - numpy's median|, to the bit; odd and even S."""
    from aehmc_amd import summary
    x, _, _ = draws(N, C, D)
    t, view, kw = laid_out(x, N, C, D, layout)
    got = host(summary._rank(t, kw["batched"], 0, True))
    assert got.shape == view
    assert np.array_equal(bits(got).reshape(N * C, D), bits(rr.ranks(rr.fold(x))))


def against_reference(s, ref, shape):
    """Reals within RTOL relative (NaN and inf where the reference has them), lag_truncated equal."""
    assert not ref["near"].any() and not ref["near_folded"].any() and not ref["near_tail"].any(), \
        "a deciding pair sum of the reference lies within 1e-9 of zero: pick another seed"
    for name in REALS:
        got, want = host(getattr(s, name)), ref[name].reshape(shape)
        assert got.shape == shape
        fin = np.isfinite(want)
        assert np.array_equal(np.isnan(got), np.isnan(want)), name
        assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), name
        rel = np.abs(got[fin] - want[fin]) / np.where(want[fin] != 0, np.abs(want[fin]), 1.0)
        print(name, "max rel err", rel.max() if rel.size else 0.0)
        assert np.all(rel <= RTOL), (name, rel.max())
    assert np.array_equal(host(s.lag_truncated), ref["lag_truncated"].reshape(shape))


def series(seed, N, C, D):
    """The AR(1) generator of tests/test_gpu_summary.py: a correlation, a location and a scale per coordinate, a small
    offset per chain."""
    r = np.random.default_rng(seed)
    phi = r.uniform(-0.3, 0.8, size=D)
    x = sr.ar1(r, N, C, D, phi, loc=r.normal(size=D) * 3.0, scale=0.5 + r.random(D))
    return x + 0.05 * r.normal(size=(1, C, D))


@pytest.mark.parametrize("N,C,D", ESTIMATOR_SHAPES)
def test_estimators_against_reference(N, C, D):
    from aehmc_amd import summary
    x = series(7000 + N + C + D, N, C, D)
    ref = rr.rank_summarize(x)
    s = summary.rank_summarize(dev(x))
    assert (s.num_draws, s.num_chains) == (N, C)
    against_reference(s, ref, (D,))


def test_scale_mismatch_is_seen():
    """8 chains of 200 normal draws, the odd chains at three times the scale: the classical split R-hat says converged,
    the rank-normalised one of the folded draws does not."""
    from aehmc_amd import summary
    x = np.random.default_rng(31).normal(size=(200, 8, 4))
    x[:, 1::2] *= 3.0
    ref = rr.rank_summarize(x)
    t = dev(x)
    s = summary.rank_summarize(t)
    against_reference(s, ref, (4,))
    classical = host(summary.summarize(t).rhat)
    print("classical", classical, "bulk", host(s.rhat_bulk), "folded", host(s.rhat_folded))
    assert np.all(classical < 1.01)
    assert np.all(host(s.rhat_folded) > 1.1)
    assert same_bits(s.rhat, s.rhat_folded)


def test_determinism_and_independence_of_arrival_order():
    from aehmc_amd import summary
    from aehmc_amd.engine import get_engine
    x, rk, _ = draws(37, 53, 17)
    S = 37 * 53
    t = dev(x).reshape(37, 53, 17)
    a, b = summary.ranks(t), summary.ranks(t)
    assert same_bits(a, b)
    za, zb = summary.rank_normalize(t), summary.rank_normalize(t)
    assert same_bits(za, zb)
    # permuted rows: permuted ranks
    perm = np.random.default_rng(5).permutation(S)
    p = summary.ranks(dev(x[perm]), batched=False)
    assert np.array_equal(bits(host(p)), bits(rk[perm]))
    # a monotone map of tie-free draws keeps every rank
    y = np.exp(x)
    assert np.all(np.diff(np.sort(y, axis=0), axis=0) > 0)
    assert same_bits(summary.ranks(dev(y).reshape(37, 53, 17)), a)
    # the least scratch (one coordinate a tile) and an odd tile of 5 coordinates: the bits of the default call
    eng = get_engine()
    flat = t.reshape(S, 17)
    one = int(eng.lib.aehmc_summary_rank_work(S, 1))
    assert one < int(eng.lib.aehmc_summary_rank_work(S, 17))
    for nbytes in (one, 5 * one):
        for mode, want in ((0, a), (1, za)):
            assert same_bits(eng.summary_rank(flat, None, mode, _work_bytes=nbytes).reshape(37, 53, 17), want)
    big, brk, _ = draws(64, 4096, 3)
    tb = dev(big)
    one = int(eng.lib.aehmc_summary_rank_work(64 * 4096, 1))
    got = eng.summary_rank(tb, None, 0, _work_bytes=2 * one + 256)
    assert np.array_equal(bits(host(got)), bits(brk))


def test_composition():
    from aehmc_amd import summary
    t = dev(series(77, 101, 7, 5))
    s = summary.rank_summarize(t)
    assert same_bits(summary.bulk_ess(t), summary.summarize(summary.rank_normalize(t)).ess)
    assert same_bits(s.ess_bulk, summary.bulk_ess(t))
    assert same_bits(summary.rank_rhat(t), s.rhat)
    assert same_bits(s.ess_tail, summary.tail_ess(t))
    assert same_bits(s.rhat_bulk, summary.rhat(summary.rank_normalize(t)))
    assert same_bits(s.rhat_folded, summary.rhat(summary.rank_normalize(t, fold=True)))
    assert same_bits(s.rhat, torch.maximum(s.rhat_bulk, s.rhat_folded))


def test_abi_errors():
    """A refused call names its entry point and writes nothing."""
    from aehmc_amd import summary
    from aehmc_amd.engine import EngineError, get_engine
    eng = get_engine()
    x, rk, _ = draws(37, 53, 17)
    t = dev(x)
    S, D = t.shape
    one = int(eng.lib.aehmc_summary_rank_work(S, 1))
    with pytest.raises(EngineError, match="aehmc_summary_rank.*one coordinate needs"):
        eng.summary_rank(t, None, 0, _work_bytes=one - 256)
    for mode in (-1, 2):
        with pytest.raises(EngineError, match="aehmc_summary_rank.*mode"):
            eng.summary_rank(t, None, mode)
    work = torch.empty(one, dtype=torch.uint8, device="cuda")
    rc = eng.lib.aehmc_summary_rank(eng.ctx, S, D, t.data_ptr(), None, 0, None, work.data_ptr(), work.numel(),
                                    eng.stream)
    assert rc != 0
    with pytest.raises(EngineError, match="aehmc_summary_rank.*bad arguments"):
        eng._check(rc, "aehmc_summary_rank")
    assert eng.lib.aehmc_summary_rank_work(0, 3) == 0 and eng.lib.aehmc_summary_rank_work(1 << 31, 3) == 0
    assert np.array_equal(bits(host(summary.ranks(t, batched=False))), bits(rk))  # the engine still answers
