"""Posterior summaries on the device: per-coordinate mean, sd, split R-hat, effective sample size and Monte-Carlo
standard error of what ``kernel.sample`` draws (``aehmc_summary_update`` / ``_autocov`` / ``_lag_update`` / ``_final``,
csrc/summary.cuh).

The reference leaves this to arviz on the host (tests/test_hmc.py:158-167: ``arviz.ess``, then ``std / sqrt(ess)``).
Here the draws stay where they are, and a run whose draws cannot be stored at all (4096 chains x 10^4 coordinates are
328 MB per draw) is summarised while it is sampled: ``run``.

Two families of estimators per coordinate, with n draws per (split) chain and m (split) chains:

- across chains -- ``rhat``, ``ess_chains``, ``mcse_chains``: W is the mean of the chains' variances, B/n the variance
  of the chains' means, var+ = W (n - 1) / n + B/n; rhat = sqrt(var+ / W), mcse_chains = sqrt((B/n) / m) (the spread of
  independent chain means: exact whatever the autocorrelation, and sharp with many chains), ess_chains = var+ /
  mcse_chains^2.  They need running moments only, so they stream.
- along chains -- ``ess``, ``mcse``, ``lag_truncated``: Stan's estimator from the chain-averaged autocovariance with
  Geyer's initial positive, initial monotone sequence.  ``summarize`` computes it from the stored draws.  With
  ``max_lag`` given, ``Accumulator`` and ``run`` stream it too: lagged products of the draws, shifted by the chain's
  first draw, over a ring of the last ``max_lag`` draws, centred when a segment ends -- the quantity of
  ``summarize(samples, max_lag=...)`` to rounding, for a run of any length.

Next to them, from the stored draws and with the chains pooled: exact ``quantiles`` (numpy's default "linear" rule),
``median``, equal-tailed ``interval``, the raw ``order_statistics`` (a radix select per coordinate, csrc/quantile.cuh:
no sort) and Stan's ``tail_ess``.

And the rank-normalised diagnostics of Vehtari, Gelman, Simpson, Carpenter and Buerkner (2021), which see what the
classical ``rhat`` cannot -- chains that agree in location but not in scale, targets without a variance: ``ranks``
(average ranks of the pooled draws, a segmented radix sort per coordinate, csrc/rank.cuh), ``rank_normalize`` (their
normal scores z = Phi^-1((r - 3/8) / (S + 1/4))), ``bulk_ess`` and ``rank_rhat``, and ``rank_summarize`` for all of
them at once.  The kernels produce ranks and scores only; every estimator after that is ``summarize`` run on z.

From the same sorted columns, the columns of an ArviZ-style table that were still missing: ``hdi`` (the narrowest window
of consecutive order statistics), ``mcse_quantile`` / ``mcse_median`` (two order statistics per coordinate, at ranks
that a beta quantile of the coordinate's own ESS gives; csrc/posterior.cuh), ``mcse_sd``, and ``table`` for the
``az.summary`` columns at once.

And for comparing models, from the pointwise log-likelihood of the stored draws (one observation is one "coordinate"):
``psislw`` (Pareto-smoothed importance weights and the Pareto shape k per observation, csrc/psis.cuh, again on the
sorted columns), ``loo`` (PSIS-LOO: the weights are used where they are formed and never stored), ``relative_eff`` and
``waic``.  The array itself comes from the model: ``Pointwise`` (``transforms.Model.pointwise``) is a traced vector
function of the position, evaluated by one kernel (csrc/pointwise.cuh), and ``WaicAccumulator`` folds it -- or stored
blocks -- into WAIC without the array ever existing; ``run(..., waic=acc)`` does so while it samples.

Without the stored draws: ``QuantileSketch``, a fixed-grid histogram per coordinate that ``run`` can feed next to its
``Accumulator`` (csrc/sketch.cuh) -- ``quantiles``, ``median`` and ``interval`` of the pooled draws to within one bin
width, with ``resolved`` to say where that bound holds.

For many chains that each run for a short time -- the regime of the pooled warm-up, ChEES and MEADS, where the
estimators above have too few draws per chain --: ``nested_rhat`` / ``NestedAccumulator`` (the nested R-hat of Margossian,
Hoffman, Sountsov, Riou-Durand, Vehtari and Gelman; csrc/nested.cuh).  The chains are started as superchains that share a
point (``superchain_positions``), the spread of the superchain means is compared with the spread inside superchains, for
any number of draws from one, per window of draws if asked; ``run(..., nested=acc)`` feeds one while it samples.

fp64, deterministic: two calls on the same draws, and any chunking of them, give the same bits.  No CPU fallback."""
from __future__ import annotations

import math
import operator
from typing import NamedTuple, Optional

import torch

from ._common import trajectory_lengths
from .engine import get_engine

# aehmc_hip.h: AEHMC_SUMMARY_MAX_ROWS -- the autocovariance kernel keeps a coordinate's centred series (one segment)
# and as many zeros as there are lags in LDS
MAX_ACOV_ROWS = 8192
# summary.run(chunk=None): the draw buffer of a chunk stays under this many bytes (at least one draw)
CHUNK_BYTES = 1 << 30
# aehmc_hip.h: AEHMC_SUMMARY_QUANTILE_MAX -- ranks of one order_statistics call, probabilities of one quantiles call
MAX_QUANTILES = 64


class Summary(NamedTuple):
    """Per-coordinate device tensors shaped like one chain's position, plus the run's size.  ``ess``, ``mcse`` and
    ``lag_truncated`` (bool: the autocorrelation pairs were still positive at the last lag, so ``ess`` is an
    over-estimate -- raise ``max_lag`` or run longer) are None in streaming mode unless ``max_lag`` is given."""
    mean: torch.Tensor
    sd: torch.Tensor
    rhat: torch.Tensor
    ess: Optional[torch.Tensor]
    mcse: Optional[torch.Tensor]
    ess_chains: torch.Tensor
    mcse_chains: torch.Tensor
    lag_truncated: Optional[torch.Tensor]
    num_draws: int
    num_chains: int


def _check_run(num_draws, num_chains, shape, split):
    num_draws, num_chains, shape = int(num_draws), int(num_chains), tuple(int(s) for s in shape)
    if len(shape) > 1:
        raise ValueError(f"a chain's position must be a scalar or a vector, got shape {shape}")
    if num_chains < 1 or (len(shape) == 1 and shape[0] < 1):
        raise ValueError("num_chains and the position's length must be positive")
    if split and num_draws < 4:
        raise ValueError(f"split chains need at least 4 draws, got {num_draws}")
    if not split and num_draws < 2:
        raise ValueError(f"a summary needs at least 2 draws, got {num_draws}")
    return num_draws, num_chains, shape


def _check_draws(x, what):
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"{what} must be a torch tensor (what kernel.sample returns), got {type(x).__name__}")
    if x.dtype != torch.float64:
        raise ValueError(f"{what} must be float64, got {x.dtype}")
    if not x.is_contiguous():
        raise ValueError(f"{what} must be contiguous")


def _chunk_rows(eng, chunk, num_chains, shape, what):
    """chunk [T, num_chains, *shape] (one chain: the chain axis may be missing), checked, as [T, C, D]."""
    _check_draws(chunk, what)
    T = chunk.shape[0] if chunk.ndim else 0
    tails = [(num_chains,) + shape] + ([shape] if num_chains == 1 else [])  # (one chain: no axis)
    if T < 1 or tuple(chunk.shape[1:]) not in tails:
        raise ValueError(f"{what} must be [T, {num_chains}" + "".join(f", {s}" for s in shape) +
                         f"], got {tuple(chunk.shape)}")
    if chunk.device != eng.device:
        raise ValueError(f"{what} must be on {eng.device}, it is on {chunk.device}")
    return chunk.reshape(T, num_chains, shape[0] if shape else 1)


class Accumulator:
    """Streaming moments of a run of ``num_draws`` draws of ``num_chains`` chains whose position has shape ``shape``
    (``()`` or ``(D,)``): ``update(chunk)`` folds the next draws, in order, ``result()`` gives the ``Summary`` once all
    have arrived.  Where the chunks are cut, a chunk of one draw included, does not change a bit.

    ``max_lag=None``: moments only, ``ess`` / ``mcse`` / ``lag_truncated`` are None.  ``max_lag=L``: they are Stan's ESS
    from lags 0 ... L of the chain-averaged autocovariance (K = min(L + 1, segment length) lags), streamed as lagged
    products over a ring of the last K - 1 draws.  That costs memory: a ring and a head of K - 1 draws each, and the
    products of groups of 4 chains (2 above 48 lags), K / 4 (K / 2) draws more -- about 2.25 (K - 1) draws in all;
    ``max_lag=32`` at 4096 chains x 10^4 coordinates is about 24 GB."""

    def __init__(self, num_draws: int, num_chains: int, shape, split: bool = True, max_lag: Optional[int] = None):
        self.num_draws, self.num_chains, self.shape = _check_run(num_draws, num_chains, shape, split)
        self.split = bool(split)
        self.D = self.shape[0] if self.shape else 1
        if max_lag is not None and int(max_lag) < 1:
            raise ValueError("max_lag must be at least 1")
        self._eng = get_engine()
        S = 2 if self.split else 1
        C, D, dev = self.num_chains, self.D, self._eng.device
        self.mean = torch.zeros(S, C, D, dtype=torch.float64, device=dev)
        self.m2 = torch.zeros_like(self.mean)
        self.seen = 0
        self.lags = None if max_lag is None else min(int(max_lag) + 1, self.num_draws // S)
        if self.lags is not None:
            K = self.lags
            self._group = self._eng.summary_lag_group(K)  # chains whose products are summed before they are stored
            self._shift, self._sums = (torch.zeros(C, D, dtype=torch.float64, device=dev) for _ in range(2))
            self._ring, self._head = (torch.zeros(K - 1, C, D, dtype=torch.float64, device=dev) for _ in range(2))
            self._prod = torch.zeros(-(-C // self._group), K, D, dtype=torch.float64, device=dev)
            self._acov = torch.zeros(K, D, dtype=torch.float64, device=dev)

    def _rows(self, chunk, what="chunk"):
        return _chunk_rows(self._eng, chunk, self.num_chains, self.shape, what)

    def update(self, chunk):
        return self._fold(self._rows(chunk))

    def _fold(self, x):  # x: [T, C, D]
        if self.seen + x.shape[0] > self.num_draws:
            raise ValueError(f"{self.seen} draws folded, {x.shape[0]} more exceed the run's {self.num_draws}")
        self._eng.summary_update(x, self.seen, self.num_draws, self.mean.shape[0], self.mean, self.m2)
        if self.lags is not None:
            self._eng.summary_lag_update(x, self.seen, self.num_draws, self.mean.shape[0], self.lags, self._shift,
                                         self._sums, self._ring, self._head, self._prod, self._acov)
        self.seen += x.shape[0]
        return self

    def result(self, _acov=None) -> Summary:
        if self.seen != self.num_draws:
            raise ValueError(f"{self.seen} of {self.num_draws} draws folded")
        if _acov is None and self.lags is not None:
            _acov = self._acov
        out, trunc = self._eng.summary_final(self.num_draws, self.mean.shape[0], self.mean, self.m2, _acov)
        f = [out[i].reshape(self.shape) for i in range(7)]
        have = _acov is not None
        return Summary(mean=f[0], sd=f[1], rhat=f[2], ess=f[3] if have else None, mcse=f[4] if have else None,
                       ess_chains=f[5], mcse_chains=f[6],
                       lag_truncated=trunc.bool().reshape(self.shape) if have else None,
                       num_draws=self.num_draws, num_chains=self.num_chains)


def _check_acov_length(N, split, max_lag):
    """The number of lags K of ``summarize`` at N draws, or its ValueError where the autocovariance kernel cannot hold
    them."""
    n = N // 2 if split else N
    if max_lag is not None and int(max_lag) < 1:
        raise ValueError("max_lag must be at least 1")
    K = n if max_lag is None else min(int(max_lag) + 1, n)
    if n + K > MAX_ACOV_ROWS:
        fits = (f"max_lag <= {MAX_ACOV_ROWS - n - 1} fits at this length" if n <= MAX_ACOV_ROWS - 2 else
                f"no max_lag fits segments above {MAX_ACOV_ROWS - 2} draws")
        raise ValueError(f"the autocovariance kernel holds segment length + lags <= {MAX_ACOV_ROWS}: {N} draws give "
                         f"segments of {n} draws with {K} lags ({fits}); summary.Accumulator gives the cross-chain "
                         "estimators at any length")
    return K


def summarize(samples, *, batched: bool = True, split: bool = True, max_lag: Optional[int] = None) -> Summary:
    """Summary of stored draws ``samples`` [N, ...] as ``kernel.sample`` returns them: [N, C] or [N, C, D] with
    ``batched`` (a leading chain axis, the default), [N] or [N, D] for one chain.  ``split``: every chain counts as
    two, its first and its last N // 2 draws (arviz's and Stan's split R-hat / ESS).  ``max_lag``: the autocorrelation
    sum uses lags 0 ... max_lag (default: every lag of a segment); segment length + lags may not exceed
    ``MAX_ACOV_ROWS``."""
    _check_draws(samples, "samples")
    lo = 2 if batched else 1
    if samples.ndim not in (lo, lo + 1):
        raise ValueError(f"samples must be [N, C] or [N, C, D] (batched) or [N] / [N, D], got {tuple(samples.shape)}")
    N = samples.shape[0]
    C = samples.shape[1] if batched else 1
    shape = tuple(samples.shape[lo:])
    N, C, shape = _check_run(N, C, shape, split)
    K = _check_acov_length(N, split, max_lag)
    acc = Accumulator(N, C, shape, split)  # (moments only: the autocovariance comes from the stored draws)
    x = acc._rows(samples, "samples")
    acc._fold(x)
    acov = acc._eng.summary_autocov(x, 2 if split else 1, K, acc.mean)
    return acc.result(acov)


def rhat(samples, **kw):
    return summarize(samples, **kw).rhat


def ess(samples, **kw):
    return summarize(samples, **kw).ess


def mcse(samples, **kw):
    return summarize(samples, **kw).mcse


def _pooled(samples, batched):
    """samples as ``summarize`` takes them -> (the draws of all chains as rows [R, D], a coordinate's shape)."""
    _check_draws(samples, "samples")
    lo = 2 if batched else 1
    if samples.ndim not in (lo, lo + 1):
        raise ValueError(f"samples must be [N, C] or [N, C, D] (batched) or [N] / [N, D], got {tuple(samples.shape)}")
    shape = tuple(samples.shape[lo:])
    R = samples.shape[0] * (samples.shape[1] if batched else 1)
    D = shape[0] if shape else 1
    if R < 1 or D < 1:
        raise ValueError(f"samples must hold at least one draw of at least one coordinate, got {tuple(samples.shape)}")
    if R >= 1 << 31:
        raise ValueError(f"the selection counts in 32 bits: {R} pooled draws are not below 2^31")
    return samples.reshape(R, D), shape


def _check_probs(probs):
    scalar = isinstance(probs, (int, float)) and not isinstance(probs, bool)
    try:
        p = [float(probs)] if scalar else [float(v) for v in probs]
    except (TypeError, ValueError):
        raise ValueError(f"probs must be a float or a sequence of floats, got {probs!r}") from None
    if not p:
        raise ValueError("probs must not be empty")
    if len(p) > MAX_QUANTILES:
        raise ValueError(f"at most {MAX_QUANTILES} probs a call, got {len(p)}")
    for v in p:
        if not (math.isfinite(v) and 0.0 <= v <= 1.0):
            raise ValueError(f"probs must be finite and within [0, 1], got {v}")
    return p, scalar


def _on_device(eng, x):
    if x.device != eng.device:
        raise ValueError(f"samples must be on {eng.device}, they are on {x.device}")


def quantiles(samples, probs, *, batched: bool = True):
    """Quantiles of stored draws at ``probs`` (a float or a sequence of floats in [0, 1]), per coordinate, the chains
    pooled as the mean and sd of ``Summary`` are: a device tensor [Q, *shape], or ``shape`` for a scalar ``probs``.
    ``samples`` as ``summarize`` takes them.  Exact: numpy's default "linear" rule (R type 7) between the two
    neighbouring order statistics, which a radix select finds without sorting; a coordinate with a NaN gives NaN."""
    x, shape = _pooled(samples, batched)
    p, scalar = _check_probs(probs)
    eng = get_engine()
    _on_device(eng, x)
    out = eng.summary_quantiles(x, p)
    return out[0].reshape(shape) if scalar else out.reshape((len(p),) + shape)


def median(samples, **kw):
    return quantiles(samples, 0.5, **kw)


def interval(samples, prob: float = 0.9, **kw):
    """``(lower, upper)``: the equal-tailed interval of mass ``prob``, the quantiles at (1 - prob) / 2 and
    (1 + prob) / 2."""
    (prob,), _ = _check_probs(prob)
    q = quantiles(samples, ((1.0 - prob) / 2.0, (1.0 + prob) / 2.0), **kw)
    return q[0], q[1]


def order_statistics(samples, ranks, *, batched: bool = True):
    """The ``ranks``-th smallest (0-based ints, any order) of the pooled draws of every coordinate: [M, *shape], the
    bits of ``sort(draws)[ranks]``."""
    x, shape = _pooled(samples, batched)
    try:
        r = [operator.index(v) for v in ranks]
    except TypeError:
        raise ValueError(f"ranks must be a sequence of integers, got {ranks!r}") from None
    if not r:
        raise ValueError("ranks must not be empty")
    if len(r) > MAX_QUANTILES:
        raise ValueError(f"at most {MAX_QUANTILES} ranks a call, got {len(r)}")
    for v in r:
        if not 0 <= v < x.shape[0]:
            raise ValueError(f"ranks must be within [0, {x.shape[0]}), got {v}")
    eng = get_engine()
    _on_device(eng, x)
    return eng.summary_order_stats(x, r).reshape((len(r),) + shape)


def tail_ess(samples, *, batched: bool = True, prob: float = 0.05, max_lag: Optional[int] = None):
    """Stan's tail ESS: the smaller of the split-chain ``ess`` of the indicators ``x <= q`` at the ``prob`` and the
    ``1 - prob`` quantile of the pooled draws.  Allocates one indicator array the size of ``samples`` at a time.
    ``summarize``'s length limit (``MAX_ACOV_ROWS``) applies."""
    _pooled(samples, batched)
    (prob,), _ = _check_probs(prob)
    lo = 2 if batched else 1
    _check_run(samples.shape[0], samples.shape[1] if batched else 1, samples.shape[lo:], True)
    _check_acov_length(samples.shape[0], True, max_lag)
    view = (2,) + (1,) * (lo - 1) + tuple(samples.shape[lo:])  # (a coordinate's quantile against all its draws)
    q = quantiles(samples, (prob, 1.0 - prob), batched=batched).reshape(view)
    out = None
    for i in range(2):
        e = summarize((samples <= q[i]).to(torch.float64), batched=batched, split=True, max_lag=max_lag).ess
        out = e if out is None else torch.minimum(out, e)
    return out


class RankSummary(NamedTuple):
    """Rank-normalised diagnostics per coordinate (device tensors shaped like one chain's position): ``rhat`` is the
    larger of ``rhat_bulk`` (split R-hat of the normal scores of the draws) and ``rhat_folded`` (of the normal scores of
    the draws folded about their median, which sees a difference in scale); ``ess_bulk`` is the split-chain ``ess`` of
    the normal scores, ``lag_truncated`` belongs to it; ``ess_tail`` is ``tail_ess``."""
    rhat: torch.Tensor
    rhat_bulk: torch.Tensor
    rhat_folded: torch.Tensor
    ess_bulk: torch.Tensor
    ess_tail: torch.Tensor
    lag_truncated: torch.Tensor
    num_draws: int
    num_chains: int


def _rank(samples, batched, mode, fold):
    """ranks (mode 0) or normal scores (mode 1) of the pooled draws, or with ``fold`` of the draws folded about the
    pooled median -- which is computed on the device and handed to the kernel: no folded copy of the draws is made."""
    x, _ = _pooled(samples, batched)
    eng = get_engine()
    _on_device(eng, x)
    center = eng.summary_quantiles(x, [0.5]).reshape(-1) if fold else None
    return eng.summary_rank(x, center, mode).reshape(samples.shape)


def ranks(samples, *, batched: bool = True):
    """Average ranks of stored draws, per coordinate and with the chains pooled: a tensor shaped like ``samples`` whose
    entry is ``#{y < x} + (#{y == x} + 1) / 2`` over the S pooled draws y of the coordinate (1-based; ties share the
    mean of their places: the bits of ``scipy.stats.rankdata(method="average")``).  ``samples`` as ``summarize`` takes
    them.  Values compare as IEEE values (-0.0 and +0.0 tie); a coordinate with a NaN gives NaN for all its draws."""
    return _rank(samples, batched, 0, False)


def rank_normalize(samples, *, batched: bool = True, fold: bool = False):
    """The normal scores ``z = Phi^-1((r - 3/8) / (S + 1/4))`` of the ranks r of ``ranks``, shaped like ``samples``.
    ``fold``: of the ranks of ``|x - median|`` instead, the median that of the coordinate's pooled draws (``median``)."""
    return _rank(samples, batched, 1, bool(fold))


def _check_rank_run(samples, batched, max_lag=None, acov=True):
    """The argument checks of the rank-normalised split estimators, all before any work is done."""
    _pooled(samples, batched)
    lo = 2 if batched else 1
    _check_run(samples.shape[0], samples.shape[1] if batched else 1, samples.shape[lo:], True)
    if acov:
        _check_acov_length(samples.shape[0], True, max_lag)


def bulk_ess(samples, *, batched: bool = True, max_lag: Optional[int] = None):
    """Bulk ESS: the split-chain ``ess`` of the normal scores of the draws.  Allocates one array the size of
    ``samples``.  ``summarize``'s length limit (``MAX_ACOV_ROWS``) applies."""
    _check_rank_run(samples, batched, max_lag)
    return summarize(rank_normalize(samples, batched=batched), batched=batched, max_lag=max_lag).ess


def _split_rhat(z, batched):
    """``summarize(z).rhat`` from the moments alone (the same kernels, the same bits; no autocovariance, no limit on
    the length)."""
    lo = 2 if batched else 1
    acc = Accumulator(z.shape[0], z.shape[1] if batched else 1, tuple(z.shape[lo:]), True)
    acc._fold(acc._rows(z, "samples"))
    return acc.result().rhat


def rank_rhat(samples, *, batched: bool = True):
    """Rank-normalised split R-hat, ``rank_summarize(samples).rhat``: the larger of the split ``rhat`` of the normal
    scores of the draws and of the draws folded about their median.  One array the size of ``samples`` at a time."""
    _check_rank_run(samples, batched, acov=False)
    out = _split_rhat(rank_normalize(samples, batched=batched), batched)
    return torch.maximum(out, _split_rhat(rank_normalize(samples, batched=batched, fold=True), batched))


def rank_summarize(samples, *, batched: bool = True, max_lag: Optional[int] = None, prob: float = 0.05) -> RankSummary:
    """``RankSummary`` of stored draws ``samples`` as ``summarize`` takes them.  ``max_lag`` as in ``summarize``, for
    ``ess_bulk`` and ``ess_tail``; ``prob`` as in ``tail_ess``.  Holds one array of normal scores the size of
    ``samples`` at a time: the bulk estimators come first, and their array is released before that of the folded draws
    is made (``tail_ess`` then allocates its indicators, again one array at a time).  ``summarize``'s length limit
    (``MAX_ACOV_ROWS``) applies and is checked before any work is done."""
    _check_rank_run(samples, batched, max_lag)
    (prob,), _ = _check_probs(prob)
    z = rank_normalize(samples, batched=batched)
    bulk = summarize(z, batched=batched, max_lag=max_lag)
    del z
    folded = _split_rhat(rank_normalize(samples, batched=batched, fold=True), batched)
    return RankSummary(rhat=torch.maximum(bulk.rhat, folded), rhat_bulk=bulk.rhat, rhat_folded=folded,
                       ess_bulk=bulk.ess, ess_tail=tail_ess(samples, batched=batched, prob=prob, max_lag=max_lag),
                       lag_truncated=bulk.lag_truncated, num_draws=bulk.num_draws, num_chains=bulk.num_chains)


def _check_hdi_prob(prob):
    if not isinstance(prob, (int, float)) or isinstance(prob, bool):
        raise ValueError(f"prob must be a float, got {prob!r}")
    prob = float(prob)
    if not (math.isfinite(prob) and 0.0 < prob <= 1.0):
        raise ValueError(f"prob must be finite and within (0, 1], got {prob}")
    return prob


def hdi(samples, prob: float = 0.9, *, batched: bool = True):
    """``(lower, upper)``: the highest-density interval of mass ``prob`` in (0, 1] of stored draws, per coordinate and
    with the chains pooled, each shaped like one chain's position.  ``samples`` as ``summarize`` takes them.  Of the
    windows of m + 1 consecutive order statistics, m = min(floor(prob S), S - 1) over the S pooled draws, the narrowest,
    and of equally narrow ones the first: ArviZ's unimodal ``hdi`` (the ``hdi_3%`` / ``hdi_97%`` columns of
    ``az.summary`` at prob = 0.94), exact, from the sorted columns of csrc/rank.cuh.  ``prob = 1`` gives (min, max);
    zeros of both signs come back as +0.0; a coordinate with a NaN gives NaN."""
    x, shape = _pooled(samples, batched)
    prob = _check_hdi_prob(prob)
    eng = get_engine()
    _on_device(eng, x)
    lower, upper, _ = eng.summary_hdi(x, prob)
    return lower.reshape(shape), upper.reshape(shape)


def mcse_quantile(samples, probs, *, batched: bool = True, max_lag: Optional[int] = None):
    """Monte-Carlo standard error of ``quantiles(samples, probs)``: [Q, *shape], or ``shape`` for a scalar ``probs``
    (``posterior::mcse_quantile``, ArviZ's ``mcse(method="quantile")``).  Per probability p the split-chain ``ess`` e of
    the indicator ``x <= quantile(x, p)`` (what ``tail_ess`` forms per tail; ``max_lag`` and the length limit as in
    ``summarize``), then half the distance between the order statistics at the 0.1586553 and the 0.8413447 quantile of
    Beta(e p + 1, e (1 - p) + 1), scaled to the S pooled draws.  One indicator array the size of ``samples`` at a time,
    one kernel call for all probabilities.  A coordinate with a NaN, or whose indicator has no ESS, gives NaN."""
    x, shape = _pooled(samples, batched)
    p, scalar = _check_probs(probs)
    lo = 2 if batched else 1
    _check_run(samples.shape[0], samples.shape[1] if batched else 1, samples.shape[lo:], True)
    _check_acov_length(samples.shape[0], True, max_lag)
    eng = get_engine()
    _on_device(eng, x)
    view = (len(p),) + (1,) * (lo - 1) + tuple(samples.shape[lo:])  # (a coordinate's quantile against all its draws)
    q = eng.summary_quantiles(x, p).reshape(view)
    e = torch.stack([summarize((samples <= q[i]).to(torch.float64), batched=batched, split=True, max_lag=max_lag)
                     .ess.reshape(-1) for i in range(len(p))])
    out, _ = eng.summary_quantile_mcse(x, p, e)
    return out[0].reshape(shape) if scalar else out.reshape((len(p),) + shape)


def mcse_median(samples, **kw):
    return mcse_quantile(samples, 0.5, **kw)


def mcse_sd(samples, *, batched: bool = True, max_lag: Optional[int] = None):
    """Monte-Carlo standard error of the standard deviation (``posterior::mcse_sd``), shaped like one chain's position:
    with c = x - the pooled mean, e the split-chain ``ess`` of c^2, Evar = mean(c^2) and
    varvar = (mean(c^4) - Evar^2) / e, ``sqrt(varvar / Evar / 4)``.  Allocates two arrays the size of ``samples``.
    ``summarize``'s length limit (``MAX_ACOV_ROWS``) applies."""
    _check_rank_run(samples, batched, max_lag)
    _on_device(get_engine(), samples)
    pool = tuple(range(2 if batched else 1))
    c = samples - samples.mean(dim=pool, keepdim=True)
    c2 = c * c
    del c
    e = summarize(c2, batched=batched, split=True, max_lag=max_lag).ess
    evar = c2.mean(dim=pool)
    varvar = ((c2 * c2).mean(dim=pool) - evar * evar) / e
    return torch.sqrt(varvar / evar / 4.0)


class PosteriorTable(NamedTuple):
    """The columns of ``az.summary`` per coordinate (device tensors shaped like one chain's position): ``mean``, ``sd``
    and ``mcse_mean`` are ``summarize``'s mean, sd and mcse; ``hdi_lower`` / ``hdi_upper`` are ``hdi`` at the table's
    ``prob``; ``mcse_sd``; ``ess_bulk``, ``ess_tail`` and ``rhat`` are ``rank_summarize``'s."""
    mean: torch.Tensor
    sd: torch.Tensor
    hdi_lower: torch.Tensor
    hdi_upper: torch.Tensor
    mcse_mean: torch.Tensor
    mcse_sd: torch.Tensor
    ess_bulk: torch.Tensor
    ess_tail: torch.Tensor
    rhat: torch.Tensor
    num_draws: int
    num_chains: int


def table(samples, prob: float = 0.9, *, batched: bool = True, max_lag: Optional[int] = None) -> PosteriorTable:
    """``PosteriorTable`` of stored draws ``samples`` as ``summarize`` takes them: ``summarize``, ``rank_summarize``,
    ``hdi(prob)`` and ``mcse_sd`` one after the other, every argument checked before any work is done.  Each of them
    that sorts does its own sort."""
    _check_rank_run(samples, batched, max_lag)
    prob = _check_hdi_prob(prob)
    s = summarize(samples, batched=batched, max_lag=max_lag)
    r = rank_summarize(samples, batched=batched, max_lag=max_lag)
    lower, upper = hdi(samples, prob, batched=batched)
    return PosteriorTable(mean=s.mean, sd=s.sd, hdi_lower=lower, hdi_upper=upper, mcse_mean=s.mcse,
                          mcse_sd=mcse_sd(samples, batched=batched, max_lag=max_lag), ess_bulk=r.ess_bulk,
                          ess_tail=r.ess_tail, rhat=r.rhat, num_draws=s.num_draws, num_chains=s.num_chains)


# loo / waic / relative_eff: what torch forms on the way (exp of a block of columns, its log-sum-exp) stays under this
# many bytes, at least one column
MODEL_BLOCK_BYTES = 128 << 20


def _column_blocks(S, D):
    step = max(1, MODEL_BLOCK_BYTES // (8 * S))
    return [(d0, min(d0 + step, D)) for d0 in range(0, D, step)]


def _reff_columns(reff, shape, D, eng):
    """``reff`` -- a float, or a device tensor shaped like one chain's position -- as a device tensor [D], or None
    for 1."""
    if isinstance(reff, torch.Tensor):
        if tuple(reff.shape) != shape:
            raise ValueError(f"reff must be a float or a tensor of shape {shape}, got shape {tuple(reff.shape)}")
        if reff.dtype != torch.float64:
            raise ValueError(f"reff must be float64, got {reff.dtype}")
        if reff.device != eng.device:
            raise ValueError(f"reff must be on {eng.device}, it is on {reff.device}")
        return reff.reshape(D).contiguous()
    if not isinstance(reff, (int, float)) or isinstance(reff, bool):
        raise ValueError(f"reff must be a float or a tensor, got {reff!r}")
    reff = float(reff)
    if not (math.isfinite(reff) and reff > 0.0):
        raise ValueError(f"reff must be finite and positive, got {reff}")
    return None if reff == 1.0 else torch.full((D,), reff, dtype=torch.float64, device=eng.device)


def psislw(log_ratios, reff=1.0, *, batched: bool = True):
    """``(log_weights, pareto_k)``: Pareto-smoothed importance sampling (Vehtari, Simpson, Gelman, Yao & Gabry; ArviZ's
    ``psislw``) of stored log importance ratios, per coordinate and with the chains pooled.  ``log_ratios`` as
    ``summarize`` takes its draws -- one observation, or whatever else the ratios belong to, is one trailing
    "coordinate"; ``log_weights`` is shaped like it and sums to 1 after ``exp`` over the pooled draws of a coordinate,
    ``pareto_k`` like one chain's position.  ``reff``: the relative efficiency of the draws, a float or a device tensor
    shaped like one chain's position; the tail holds ``ceil(min(S / 5, 3 sqrt(S / reff)))`` of the S pooled draws at
    most.  The largest draws above the cutoff (strictly: ties at the cutoff stay out) are replaced by the expected
    order statistics of the generalised Pareto distribution fitted to them (Zhang & Stephens' estimator with ArviZ's
    priors), tied draws sharing the mean weight of their places, so that the weights do not depend on the order of the
    draws.  ``pareto_k`` is +inf where fewer than 5 draws lie above the cutoff (nothing is smoothed) and NaN where the
    fit fails; a coordinate with a NaN, a +inf, nothing but -inf, or a ``reff`` that is not finite and positive is NaN
    throughout.  csrc/psis.cuh, on the sorted columns of csrc/rank.cuh."""
    x, shape = _pooled(log_ratios, batched)
    eng = get_engine()
    _on_device(eng, x)
    lw, k, _, _ = eng.summary_psis(x, _reff_columns(reff, shape, x.shape[1], eng))
    return lw.reshape(log_ratios.shape), k.reshape(shape)


def relative_eff(log_lik, *, batched: bool = True, max_lag: Optional[int] = None):
    """The relative efficiency that ``loo`` hands to the smoothing, shaped like one chain's position: per observation
    ``summarize(exp(log_lik - max)).ess / S`` over the S pooled draws (R ``loo``'s ``relative_eff`` of the
    likelihood), and 1 where that is not finite and positive.  ``max_lag`` and the length limit as in ``summarize``."""
    x, shape = _pooled(log_lik, batched)
    _check_rank_run(log_lik, batched, max_lag)
    _on_device(get_engine(), x)
    S, D = x.shape
    pool = tuple(range(2 if batched else 1))
    out = []
    for d0, d1 in _column_blocks(S, D) if shape else [(0, 1)]:
        blk = log_lik[..., d0:d1] if shape else log_lik
        e = torch.exp(blk - blk.amax(dim=pool, keepdim=True)).contiguous()
        out.append(summarize(e, batched=batched, max_lag=max_lag).ess.reshape(-1) / S)
    r = torch.cat(out)
    return torch.where(torch.isfinite(r) & (r > 0), r, torch.ones_like(r)).reshape(shape)


def _pooled_lppd(x):
    """log mean_s exp(x) per column of x [S, D], a block of columns at a time."""
    S, D = x.shape
    return torch.cat([torch.logsumexp(x[:, d0:d1], dim=0) for d0, d1 in _column_blocks(S, D)]) - math.log(S)


class LooResult(NamedTuple):
    """PSIS-LOO of a model.  ``elpd``, ``se`` and ``p`` are floats: the expected log pointwise predictive density, its
    standard error ``sqrt(n_data var(elpd_i))`` and the effective number of parameters ``sum(lppd_i - elpd_i)``.
    ``elpd_i``, ``pareto_k``, ``lppd_i`` and ``tail_len`` (int64: the draws that were smoothed, -1 for an observation
    that is NaN) are device tensors shaped like one chain's position.  ``warning``: some ``pareto_k`` lies above
    ``k_threshold = min(1 - 1 / log10(S), 0.7)``, the estimate of that observation is unreliable."""
    elpd: float
    se: float
    p: float
    elpd_i: torch.Tensor
    pareto_k: torch.Tensor
    lppd_i: torch.Tensor
    tail_len: torch.Tensor
    k_threshold: float
    warning: bool
    n_samples: int
    n_data: int


def loo(log_lik, reff=None, *, batched: bool = True, max_lag: Optional[int] = None) -> LooResult:
    """Leave-one-out cross-validation by Pareto-smoothed importance sampling (``az.loo``, R's ``loo``) from the
    pointwise log-likelihood ``log_lik``, laid out as ``summarize`` takes its draws: one observation is one trailing
    "coordinate", [N, C, n_data] with ``batched``.  Per observation the log ratios are ``-log_lik``, smoothed as in
    ``psislw``, and ``elpd_i = log sum_s w_s exp(log_lik_s)``; the weights are never stored and no negated copy of
    ``log_lik`` is made: besides the sort's scratch the call allocates a few blocks of ``MODEL_BLOCK_BYTES`` at most
    (torch's temporaries for ``relative_eff`` and ``lppd_i``), nothing the size of ``log_lik``.
    ``reff``: as in ``psislw``, or None for ``relative_eff(log_lik)`` (``max_lag`` goes there, and ``summarize``'s
    length limit applies; pass ``reff=1.0`` for independent draws).  ``lppd_i = log mean_s exp(log_lik_s)``."""
    x, shape = _pooled(log_lik, batched)
    eng = get_engine()
    _on_device(eng, x)
    S, D = x.shape
    if reff is None:
        r = relative_eff(log_lik, batched=batched, max_lag=max_lag).reshape(D)
    else:
        r = _reff_columns(reff, shape, D, eng)
    _, k, tail, elpd_i = eng.summary_psis(None, r, x, weights=False)
    lppd_i = _pooled_lppd(x)
    threshold = min(1.0 - 1.0 / math.log10(S), 0.7) if S > 1 else -math.inf
    return LooResult(elpd=elpd_i.sum().item(), se=math.sqrt(D * torch.var(elpd_i, unbiased=False).item()),
                     p=(lppd_i - elpd_i).sum().item(), elpd_i=elpd_i.reshape(shape), pareto_k=k.reshape(shape),
                     lppd_i=lppd_i.reshape(shape), tail_len=tail.reshape(shape), k_threshold=threshold,
                     warning=bool((k > threshold).any().item()), n_samples=S, n_data=D)


class WaicResult(NamedTuple):
    """The widely applicable information criterion on the elpd scale: ``elpd_i = lppd_i - p_i``, ``elpd`` and ``p``
    their sums (floats), ``se = sqrt(n_data var(elpd_i))``; the per-observation tensors are shaped like one chain's
    position."""
    elpd: float
    se: float
    p: float
    elpd_i: torch.Tensor
    p_i: torch.Tensor
    lppd_i: torch.Tensor


def waic(log_lik, *, batched: bool = True) -> WaicResult:
    """WAIC from the pointwise log-likelihood ``log_lik`` as ``loo`` takes it: ``lppd_i = log mean_s exp(log_lik_s)``
    and ``p_i`` the sample variance (divisor S - 1) of ``log_lik`` over the S pooled draws.  torch reductions, a block
    of ``MODEL_BLOCK_BYTES`` at a time."""
    x, shape = _pooled(log_lik, batched)
    _on_device(get_engine(), x)
    S, D = x.shape
    lppd_i = _pooled_lppd(x)
    p_i = torch.cat([torch.var(x[:, d0:d1], dim=0, unbiased=True) for d0, d1 in _column_blocks(S, D)])
    elpd_i = lppd_i - p_i
    return WaicResult(elpd=elpd_i.sum().item(), se=math.sqrt(D * torch.var(elpd_i, unbiased=False).item()),
                      p=p_i.sum().item(), elpd_i=elpd_i.reshape(shape), p_i=p_i.reshape(shape),
                      lppd_i=lppd_i.reshape(shape))


# csrc/pointwise.cuh: PW_PART -- a WAIC fold cuts its rows into parts of this many; blocks of rows that are multiples of it
# fold to the bits of one call
WAIC_PART = 256


class Pointwise:
    """A vector function of one chain's position, ``fn(q, *args)`` -> ``n_out`` entries (a pointwise log-likelihood: one
    entry per observation), traced once (``tracing.trace_pointwise``: what a traced ``logprob_fn`` may do, with a vector
    result) and compiled with hipRTC on first use.  ``pw(samples)``: a contiguous float64 device tensor [..., dim] ->
    [..., n_out], one kernel that writes nothing but its result (csrc/pointwise.cuh).  ``transforms.Model.pointwise``
    builds one on the constrained scale of a model."""

    def __init__(self, fn, dim, args=(), *, _model=None):
        from . import tracing
        self.dim = int(dim)
        self._model = _model
        if _model is not None and _model.dim != self.dim:
            raise ValueError(f"the model has {_model.dim} coordinates, not {self.dim}")
        self._traced = tracing.trace_pointwise(fn, self.dim if _model is None else _model.constrained_dim, args=args)
        self.n_out = self._traced.n_out

    def _check(self, samples, what):
        _check_draws(samples, what)
        if samples.ndim < 1 or samples.shape[-1] != self.dim:
            raise ValueError(f"{what} must be [..., {self.dim}], got {tuple(samples.shape)}")
        eng = get_engine()
        _on_device(eng, samples)
        return eng, samples.reshape(-1, self.dim)

    def _block_rows(self):
        """rows of a constrained block: under MODEL_BLOCK_BYTES, a multiple of WAIC_PART (the folds of consecutive blocks
        are then the fold of all their rows, bit for bit)"""
        return max(WAIC_PART, MODEL_BLOCK_BYTES // (8 * self._model.constrained_dim) // WAIC_PART * WAIC_PART)

    def _blocks(self, eng, x, buf=None):
        """(r0, r1, the rows the program reads) over x [R, dim]: x itself, or its constrained blocks in one reused buffer"""
        R = x.shape[0]
        if self._model is None:
            yield 0, R, x
            return
        step, cd = self._block_rows(), self._model.constrained_dim
        if buf is None:
            buf = torch.empty(min(step, R) * cd, dtype=torch.float64, device=eng.device)
        for r0 in range(0, R, step):
            r1 = min(r0 + step, R)
            yield r0, r1, self._model._constrain_rows(eng, x[r0:r1], buf[:(r1 - r0) * cd].view(r1 - r0, cd))

    def __call__(self, samples):
        eng, x = self._check(samples, "samples")
        out = torch.empty(x.shape[0], self.n_out, dtype=torch.float64, device=eng.device)
        eng.set_pointwise(self, self._traced)
        for r0, r1, rows in self._blocks(eng, x):
            eng.pointwise_eval(rows, out[r0:r1])
        return out.reshape(tuple(samples.shape[:-1]) + (self.n_out,))

    def _fold(self, eng, x, acc, constrained=None, buf=None):
        """fold the rows x [R, dim] into ``acc``; ``constrained``: the same rows on the model's constrained scale, where
        the caller has them already"""
        eng.set_pointwise(self, self._traced)
        for r0, r1, rows in ([(0, x.shape[0], constrained)] if constrained is not None else self._blocks(eng, x, buf)):
            eng.pointwise_waic_fold(rows, acc.state, acc.n_samples)
            acc.n_samples += r1 - r0


class WaicAccumulator:
    """Streaming WAIC: per observation a running log-sum-exp and a running variance of the pointwise log-likelihood, so
    that a run whose log-likelihood array cannot be stored (4096 chains x 10^4 observations: 328 MB per draw) still gets
    a model-comparison number.  ``WaicAccumulator(pw)`` with a ``Pointwise``: ``update(draws)`` folds positions
    [T, C, dim] or [R, dim] through it without forming their log-likelihood.  ``WaicAccumulator(n_obs)``:
    ``update_log_lik(x)`` folds stored blocks [..., n_obs] (it works on either).  ``result()``: the ``WaicResult`` of
    ``waic`` on all folded draws, to rounding; ``n_samples``: how many there are.  ``state`` [4, n_obs] holds the running
    maximum, sum of exp, mean and sum of squared deviations (csrc/pointwise.cuh has the arithmetic).  Rows are folded
    in parts of ``WAIC_PART``, cut per call: equal calls give equal bits, another cut of the same draws the same result
    to rounding.  PSIS-LOO does not stream: it needs every draw of an observation."""

    def __init__(self, pw_or_n_obs):
        if isinstance(pw_or_n_obs, Pointwise):
            self.pointwise, self.n_obs = pw_or_n_obs, pw_or_n_obs.n_out
        else:
            try:
                self.pointwise, self.n_obs = None, operator.index(pw_or_n_obs)
            except TypeError:
                raise ValueError(f"WaicAccumulator takes a Pointwise or a number of observations, got {pw_or_n_obs!r}") from None
            if self.n_obs < 1:
                raise ValueError("the number of observations must be positive")
        self._eng = get_engine()
        self.state = torch.zeros(4, self.n_obs, dtype=torch.float64, device=self._eng.device)
        self.state[0] = -math.inf
        self.n_samples = 0

    def update(self, draws):
        if self.pointwise is None:
            raise ValueError("this accumulator was built from a number of observations: it folds stored blocks "
                             "(update_log_lik); build it from a Pointwise to fold positions")
        eng, x = self.pointwise._check(draws, "draws")
        self.pointwise._fold(eng, x, self)
        return self

    def update_log_lik(self, x):
        _check_draws(x, "x")
        if x.ndim < 1 or x.shape[-1] != self.n_obs:
            raise ValueError(f"x must be [..., {self.n_obs}], got {tuple(x.shape)}")
        _on_device(self._eng, x)
        rows = x.reshape(-1, self.n_obs)
        self._eng.waic_fold(rows, self.state, self.n_samples)
        self.n_samples += rows.shape[0]
        return self

    def merge(self, other):
        """Add the draws of ``other`` BEHIND this accumulator's (ordered: as if ``other``'s draws had been one more
        part of a fold)."""
        if not isinstance(other, WaicAccumulator) or other.n_obs != self.n_obs or other is self:
            raise ValueError(f"merge takes another WaicAccumulator of {self.n_obs} observations")
        if other.n_samples:
            self._eng.waic_merge(self.state, self.n_samples, other.state, other.n_samples)
            self.n_samples += other.n_samples
        return self

    def result(self) -> WaicResult:
        if self.n_samples < 1:
            raise ValueError("no draw has been folded yet")
        lppd_i, p_i = self._eng.waic_final(self.state, self.n_samples)
        elpd_i = lppd_i - p_i
        return WaicResult(elpd=elpd_i.sum().item(), se=math.sqrt(self.n_obs * torch.var(elpd_i, unbiased=False).item()),
                          p=p_i.sum().item(), elpd_i=elpd_i, p_i=p_i, lppd_i=lppd_i)


# aehmc_hip.h: AEHMC_SUMMARY_SKETCH_MIN_BINS / _MAX_BINS -- the grids of QuantileSketch (a power of two in between)
MIN_SKETCH_BINS, MAX_SKETCH_BINS = 64, 4096


def _grid_edge(v, shape, D, what):
    """An edge of a QuantileSketch grid -- a float or a [*shape] tensor -- as a host fp64 tensor [D]."""
    if isinstance(v, torch.Tensor):
        if tuple(v.shape) != shape:
            raise ValueError(f"grid {what} must be a float or a tensor of shape {shape}, got shape {tuple(v.shape)}")
        return v.detach().to(device="cpu", dtype=torch.float64).reshape(D).clone()
    if isinstance(v, (int, float)) and not isinstance(v, bool):
        return torch.full((D,), float(v), dtype=torch.float64)
    raise ValueError(f"grid {what} must be a float or a tensor of shape {shape}, got {type(v).__name__}")


class QuantileSketch:
    """Streaming quantiles of draws that are not kept: a fixed-grid histogram per coordinate, the chains pooled
    (``aehmc_summary_sketch_update`` / ``_sketch_quantiles``, csrc/sketch.cuh).  ``update(chunk)`` folds draws
    [T, num_chains, *shape] -- the chunks ``Accumulator.update`` takes, in any order --, ``quantiles`` / ``median`` /
    ``interval`` answer at any time after the first.  ``summary.run(..., sketch=sk)`` feeds one while it samples.

    Coordinate d has ``bins`` (a power of two in [64, 4096]) equal bins between ``lo[d]`` and ``hi[d]``, one counter
    below, one above and one for NaN: ``counts`` [D, bins + 3], int64, is the whole state.  An estimate interpolates
    inside the bin that holds the rank; where ``resolved(probs)`` is True -- both neighbouring ranks in interior bins,
    no NaN counted -- it lies within ``bound`` (the bin width, [*shape]) of the exact quantile of the pooled draws.  Where
    it is False the estimate lies outside the grid and carries no bound (NaN where a NaN was counted, as ``quantiles``
    of stored draws gives).  Counts are integers: any chunking of the same draws gives the same bits.

    The grid: ``grid=(lo, hi)``, floats or [*shape] tensors with finite ``lo < hi``; or ``fit(samples)`` on stored
    draws; or, by default, fitted to the FIRST chunk folded: with its exact quartiles q25, q50, q75 and
    scale = (q75 - q25) / 1.349 (1 where that is 0 or not finite), lo, hi = q50 -+ span * scale.  That assumes chains
    which are warmed up when the first chunk is drawn, as ``summary.run`` expects; it is ``resolved`` that says
    otherwise -- then pass ``grid`` or more ``span``.  ``span=8`` with 2048 bins is a bin of 1 / 128 of a standard
    deviation for a normal coordinate."""

    def __init__(self, num_chains: int, shape, *, bins: int = 2048, span: float = 8.0, grid=None):
        self.num_chains, self.shape = int(num_chains), tuple(int(v) for v in shape)
        if len(self.shape) > 1:
            raise ValueError(f"a chain's position must be a scalar or a vector, got shape {self.shape}")
        if self.num_chains < 1 or (self.shape and self.shape[0] < 1):
            raise ValueError("num_chains and the position's length must be positive")
        try:
            self.bins = operator.index(bins)
        except TypeError:
            raise ValueError(f"bins must be an integer, got {bins!r}") from None
        if not MIN_SKETCH_BINS <= self.bins <= MAX_SKETCH_BINS or self.bins & (self.bins - 1):
            raise ValueError(f"bins must be a power of two in [{MIN_SKETCH_BINS}, {MAX_SKETCH_BINS}], got {bins}")
        self.span = float(span)
        if not (math.isfinite(self.span) and self.span > 0.0):
            raise ValueError(f"span must be positive and finite, got {span}")
        self.D = self.shape[0] if self.shape else 1
        self._lo = self._hi = self._width = self._inv = None
        if grid is not None:
            try:
                lo, hi = grid
            except (TypeError, ValueError):
                raise ValueError("grid must be a pair (lo, hi)") from None
            lo, hi = _grid_edge(lo, self.shape, self.D, "lo"), _grid_edge(hi, self.shape, self.D, "hi")
            if not bool((torch.isfinite(lo) & torch.isfinite(hi) & (lo < hi)).all()):
                raise ValueError("grid needs finite edges with lo < hi in every coordinate")
        self._eng = get_engine()
        self.counts = torch.zeros(self.D, self.bins + 3, dtype=torch.int64, device=self._eng.device)
        self._started = False
        if grid is not None:
            self._set_grid(lo, hi)

    def _set_grid(self, lo, hi):
        """lo, hi: host fp64 [D].  width and 1 / width are computed here, once, and the kernels read them."""
        width = (hi - lo) / float(self.bins)
        inv = 1.0 / width
        self._lo, self._hi, self._width, self._inv = (t.to(self._eng.device) for t in (lo, hi, width, inv))

    def _fit(self, x):  # x: [T, C, D]
        rows = x.reshape(-1, self.D)
        if rows.shape[0] >= 1 << 31:
            raise ValueError(f"the selection counts in 32 bits: {rows.shape[0]} pooled draws are not below 2^31")
        q = self._eng.summary_quantiles(rows, [0.25, 0.5, 0.75]).cpu()
        scale = (q[2] - q[0]) / 1.349
        scale = torch.where(torch.isfinite(scale) & (scale != 0.0), scale, torch.ones_like(scale))
        reach = self.span * scale
        self._set_grid(q[1] - reach, q[1] + reach)

    def fit(self, samples):
        """Set the grid from stored draws [T, num_chains, *shape] (their quartiles, as the default does with the first
        chunk) without counting them; before any ``update``."""
        if self._started:
            raise ValueError("fit comes before the first update: the counts belong to the grid they were made on")
        self._fit(_chunk_rows(self._eng, samples, self.num_chains, self.shape, "samples"))
        return self

    def update(self, chunk):
        x = _chunk_rows(self._eng, chunk, self.num_chains, self.shape, "chunk")
        if x.shape[0] * x.shape[1] >= 1 << 31:
            raise ValueError(f"a call counts in 32 bits: {x.shape[0] * x.shape[1]} pooled draws are not below 2^31")
        if self._lo is None:
            self._fit(x)
        self._eng.summary_sketch_update(x, self.bins, self._lo, self._inv, self.counts)
        self._started = True
        return self

    def merge(self, other):
        """Add the counts of ``other``, a sketch of other draws on the SAME grid (``bins`` and the bits of both edges)."""
        if not isinstance(other, QuantileSketch):
            raise ValueError(f"merge takes a QuantileSketch, got {type(other).__name__}")
        if other.bins != self.bins or other.shape != self.shape:
            raise ValueError(f"sketches of {self.bins} bins and shape {self.shape} and of {other.bins} bins and shape "
                             f"{other.shape} do not merge")
        if self._lo is None or other._lo is None:
            raise ValueError("both sketches need their grid before they merge (grid=, fit or a first update)")
        for mine, theirs in ((self._lo, other._lo), (self._hi, other._hi)):
            if not torch.equal(mine.view(torch.int64), theirs.view(torch.int64)):
                raise ValueError("sketches merge on one grid only: lo and hi must be bit-equal")
        self.counts += other.counts
        self._started = self._started or other._started
        return self

    def _query(self, probs):
        p, scalar = _check_probs(probs)
        if not self._started:
            raise ValueError("the sketch has counted no draw yet")
        est, res = self._eng.summary_sketch_quantiles(self.counts, self.bins, self._lo, self._width, p)
        view = self.shape if scalar else (len(p),) + self.shape
        return est.reshape(view), res.bool().reshape(view)

    def quantiles(self, probs):
        """Estimates at ``probs`` (a float or a sequence of floats in [0, 1]): [Q, *shape], or ``shape`` for a float."""
        return self._query(probs)[0]

    def resolved(self, probs):
        """bool, shaped like ``quantiles(probs)``: the estimate lies within ``bound`` of the exact quantile."""
        return self._query(probs)[1]

    def median(self):
        return self.quantiles(0.5)

    def interval(self, prob: float = 0.9):
        """``(lower, upper)``: the estimates at (1 - prob) / 2 and (1 + prob) / 2."""
        (prob,), _ = _check_probs(prob)
        q = self.quantiles(((1.0 - prob) / 2.0, (1.0 + prob) / 2.0))
        return q[0], q[1]

    @property
    def lo(self):
        return None if self._lo is None else self._lo.reshape(self.shape)

    @property
    def hi(self):
        return None if self._hi is None else self._hi.reshape(self.shape)

    @property
    def bound(self):
        """The bin width [*shape]: the error bound of a resolved estimate (None until the grid is set)."""
        return None if self._width is None else self._width.reshape(self.shape)

    @property
    def num_draws(self):
        """Pooled draws counted so far, NaN included (read from the counters)."""
        return int(self.counts[0].sum().item())


class NestedRhat(NamedTuple):
    """Nested R-hat per coordinate (device tensors shaped like one chain's position; with ``window=w`` each has a
    leading axis of ``num_draws // w`` windows): ``between`` is the variance of the superchain means, ``within`` the
    mean over superchains of (the variance of the chain means inside the superchain + the mean of the chains' own
    variances over the window), ``nested_rhat = sqrt(1 + between / within)``; ``mean`` is the mean of the superchain
    means and ``mcse_superchains = sqrt(between / num_superchains)`` its standard error from independent superchains
    (no autocorrelation estimate).  ``within = between = 0`` gives NaN, ``within = 0 < between`` +inf,
    ``between = 0 < within`` exactly 1."""
    nested_rhat: torch.Tensor
    between: torch.Tensor
    within: torch.Tensor
    mean: torch.Tensor
    mcse_superchains: torch.Tensor
    num_draws: int
    num_chains: int
    num_superchains: int
    window: Optional[int]


def superchain_positions(starts, chains_per_superchain: int):
    """Initial positions of ``K * chains_per_superchain`` chains in K superchains: ``starts`` [K, D] or [K], every row
    repeated ``chains_per_superchain`` times in place -- chain c starts at ``starts[c // chains_per_superchain]``, the
    contiguous grouping ``nested_rhat`` assumes (and ``parallel.shard_chains`` keeps whole when K divides by the world
    size)."""
    if not isinstance(starts, torch.Tensor):
        raise ValueError(f"starts must be a torch tensor [K, D] or [K], got {type(starts).__name__}")
    if starts.ndim not in (1, 2) or starts.shape[0] < 1:
        raise ValueError(f"starts must be [K, D] or [K], got {tuple(starts.shape)}")
    try:
        M = operator.index(chains_per_superchain)
    except TypeError:
        raise ValueError(f"chains_per_superchain must be an integer, got {chains_per_superchain!r}") from None
    if M < 1:
        raise ValueError("chains_per_superchain must be at least 1")
    return starts.repeat_interleave(M, dim=0).contiguous()


def _check_nested(num_draws, num_chains, shape, num_superchains, window):
    """(num_draws, num_chains, shape, K, M, window or None) of a nested R-hat run, or its ValueError."""
    num_draws, num_chains, shape = int(num_draws), int(num_chains), tuple(int(s) for s in shape)
    if len(shape) > 1:
        raise ValueError(f"a chain's position must be a scalar or a vector, got shape {shape}")
    if num_chains < 1 or (len(shape) == 1 and shape[0] < 1):
        raise ValueError("num_chains and the position's length must be positive")
    if num_draws < 1:
        raise ValueError(f"nested R-hat needs at least 1 draw, got {num_draws}")
    try:
        K = operator.index(num_superchains)
    except TypeError:
        raise ValueError(f"num_superchains must be an integer, got {num_superchains!r}") from None
    if K < 2:
        raise ValueError(f"nested R-hat compares superchains: num_superchains must be at least 2, got {K}")
    if num_chains % K:
        raise ValueError(f"{num_chains} chains do not divide into {K} superchains of equal size")
    M = num_chains // K
    if window is not None:
        try:
            window = operator.index(window)
        except TypeError:
            raise ValueError(f"window must be an integer or None, got {window!r}") from None
        if window < 1:
            raise ValueError(f"window must be at least 1, got {window}")
        if num_draws % window:
            raise ValueError(f"num_draws must be a multiple of window: {num_draws} draws, windows of {window}")
    if M == 1 and (num_draws if window is None else window) == 1:
        raise ValueError("a window of one draw with one chain per superchain leaves nothing to estimate inside a "
                         "superchain: take more chains per superchain or a longer window")
    return num_draws, num_chains, shape, K, M, window


class NestedAccumulator:
    """Streaming nested R-hat (Margossian et al.) of a run of ``num_draws`` draws of ``num_chains`` chains whose
    position has shape ``shape``: the chains are ``num_superchains`` superchains of consecutive chains that share a
    starting point (``superchain_positions``).  ``update(chunk)`` folds the next draws [T, num_chains, *shape], in order,
    ``result()`` gives the ``NestedRhat`` once all have arrived.  ``window=None``: one window of all draws, fields shaped
    like a position; ``window=w`` (``num_draws % w == 0``): one row per window of w draws, a trace that shows when the
    chains forgot their starting points.  Any number of draws from 1.  The state is the chains' running moments of the
    window in progress (``mean``, ``m2`` [num_chains, D]) and the rows written so far (``out`` [windows, 5, D]);
    at most two kernel launches per ``update`` whatever the chunk holds, and where the chunks are cut, inside a window or
    one draw at a time, does not change a bit (``aehmc_nested_update``, csrc/nested.cuh)."""

    def __init__(self, num_draws: int, num_chains: int, shape, num_superchains: int, window: Optional[int] = None):
        (self.num_draws, self.num_chains, self.shape, self.num_superchains, self.chains_per_superchain,
         self.window) = _check_nested(num_draws, num_chains, shape, num_superchains, window)
        self.D = self.shape[0] if self.shape else 1
        self._w = self.num_draws if self.window is None else self.window
        self._eng = get_engine()
        dev = self._eng.device
        self.mean = torch.zeros(self.num_chains, self.D, dtype=torch.float64, device=dev)
        self.m2 = torch.zeros_like(self.mean)
        self.out = torch.zeros(self.num_draws // self._w, 5, self.D, dtype=torch.float64, device=dev)
        self.seen = 0

    def update(self, chunk):
        return self._fold(_chunk_rows(self._eng, chunk, self.num_chains, self.shape, "chunk"))

    def _fold(self, x):  # x: [T, C, D]
        if self.seen + x.shape[0] > self.num_draws:
            raise ValueError(f"{self.seen} draws folded, {x.shape[0]} more exceed the run's {self.num_draws}")
        self._eng.nested_update(x, self.seen, self.num_draws, self._w, self.chains_per_superchain, self.mean, self.m2,
                                self.out)
        self.seen += x.shape[0]
        return self

    def result(self) -> NestedRhat:
        if self.seen != self.num_draws:
            raise ValueError(f"{self.seen} of {self.num_draws} draws folded")
        view = self.shape if self.window is None else (self.out.shape[0],) + self.shape
        f = [self.out[:, i].reshape(view) for i in range(5)]
        return NestedRhat(nested_rhat=f[0], between=f[1], within=f[2], mean=f[3], mcse_superchains=f[4],
                          num_draws=self.num_draws, num_chains=self.num_chains, num_superchains=self.num_superchains,
                          window=self.window)


def nested_rhat(samples, num_superchains: int, *, window: Optional[int] = None, batched: bool = True) -> NestedRhat:
    """``NestedRhat`` of stored draws ``samples`` as ``summarize`` takes them ([N, C] or [N, C, D] with ``batched``),
    the C chains in ``num_superchains`` superchains of consecutive chains.  ``window`` as in ``NestedAccumulator``.  One
    chain (``batched=False``) cannot hold two superchains and is refused."""
    _check_draws(samples, "samples")
    lo = 2 if batched else 1
    if samples.ndim not in (lo, lo + 1):
        raise ValueError(f"samples must be [N, C] or [N, C, D] (batched) or [N] / [N, D], got {tuple(samples.shape)}")
    C = samples.shape[1] if batched else 1
    acc = NestedAccumulator(samples.shape[0], C, tuple(samples.shape[lo:]), num_superchains, window)
    return acc.update(samples).result()


def run(kernel, state, step_size, inverse_mass_matrix, num_samples: int, *, num_integration_steps=None,
        chunk: Optional[int] = None, max_lag: Optional[int] = None, sketch: Optional[QuantileSketch] = None,
        constrain=None, waic: Optional[WaicAccumulator] = None, nested: Optional[NestedAccumulator] = None):
    """Sample ``num_samples`` transitions per chain and summarise them without keeping them: ``kernel.sample`` is
    driven in chunks of ``chunk`` draws into one reused buffer and every chunk is folded into an ``Accumulator``.
    Returns ``(Summary, Diagnostics of the last transition, acceptance history, divergence history)`` -- what
    ``kernel.sample`` returns with the summary in place of the draws (``n_leapfrog`` is the total of the run).  The
    chain states, the generator states and the histories are those of one ``kernel.sample`` call.

    ``max_lag=None``: the Summary's ``ess`` / ``mcse`` / ``lag_truncated`` are None, its cross-chain estimators are
    what many chains are judged by.  ``max_lag=L``: they are those of ``summarize(samples, max_lag=L)`` to rounding,
    from a ring of the last draws instead of all of them -- about 2.25 L draws of extra memory (see ``Accumulator``;
    ``max_lag=32`` at 4096 chains x 10^4 coordinates is about 24 GB).

    ``sketch``: a ``QuantileSketch`` of the run's chains and position shape; every chunk is folded into it too, so that
    median and intervals are there when the run ends (``sketch.quantiles`` / ``interval`` / ``resolved``).  What is
    returned does not change.

    ``constrain``: a ``transforms.Model`` of the position's length; every chunk is mapped to the constrained scale
    (``aehmc_constrain``, one pass into a second reused buffer) before it is folded, so the Summary and the sketch are
    those of the model's parameters, shaped ``(model.constrained_dim,)`` -- the mean of sigma, not of log sigma.  The
    two buffers together stay under ``CHUNK_BYTES``; the chain state that is returned stays unconstrained.

    ``waic``: a ``WaicAccumulator`` built from a ``Pointwise`` of the position's length; every chunk's positions are
    folded into it too (the log-likelihood is evaluated inside the fold and never stored), so ``waic.result()`` is there
    when the run ends.  What is returned does not change.  A ``Pointwise`` of ``constrain``'s own model reads the
    constrained buffer of the run; any other model-bound one maps into a buffer of its own, which counts towards
    ``CHUNK_BYTES``.

    ``nested``: a ``NestedAccumulator`` of the run's chains and position shape (the constrained one with ``constrain``)
    that still expects at least ``num_samples`` draws; every chunk is folded into it too, so the nested R-hat of chains
    started with ``superchain_positions`` -- or its trace over windows -- is there when the run ends
    (``nested.result()`` once all its draws have arrived).  What is returned does not change.

    An HMC kernel needs ``num_integration_steps`` (as in ``window_adaptation.run``): an int, or one length per
    transition (a sequence of ``num_samples`` entries, as ``kernel.sample`` takes it -- the jittered lengths of
    ``chees.trajectory_lengths`` for a run too large to store); every chunk gets its slice.  ``chunk=None``: the largest
    chunk whose buffer stays under ``CHUNK_BYTES`` (1 GiB), at least one draw."""
    is_hmc = getattr(kernel, "_hmc", None) is not None
    if is_hmc and num_integration_steps is None:
        raise ValueError("summary.run with an HMC kernel needs num_integration_steps")
    if not hasattr(kernel, "sample"):
        raise ValueError("summary.run needs a kernel of hmc.new_kernel / nuts.new_kernel (with .sample)")
    lengths = None if num_integration_steps is None else trajectory_lengths(num_integration_steps, num_samples)
    extra = () if num_integration_steps is None or lengths is not None else (int(num_integration_steps),)
    pos = state.position
    pshape = tuple(pos.shape) if hasattr(pos, "shape") else ()
    batched = bool(getattr(kernel, "batched", len(pshape) == 2))
    C = int(getattr(kernel, "num_chains", None) or (pshape[0] if batched else 1))
    if batched and (len(pshape) < 1 or pshape[0] != C):
        raise ValueError(f"position must have leading dimension {C}, got shape {pshape}")
    shape = pshape[1:] if batched else pshape
    N = int(num_samples)
    if chunk is not None and int(chunk) < 1:
        raise ValueError("chunk must be at least 1")
    D_in = shape[0] if shape else 1
    if constrain is not None:
        if not (hasattr(constrain, "_constrain_rows") and hasattr(constrain, "constrained_dim")):
            raise ValueError(f"constrain must be a transforms.Model, got {type(constrain).__name__}")
        if constrain.dim != D_in:
            raise ValueError(f"constrain maps positions of {constrain.dim} coordinates, the chains have {D_in}")
    if waic is not None:
        if not isinstance(waic, WaicAccumulator) or waic.pointwise is None:
            raise ValueError("waic must be a WaicAccumulator built from a Pointwise")
        if waic.pointwise.dim != D_in:
            raise ValueError(f"waic folds positions of {waic.pointwise.dim} coordinates, the chains have {D_in}")
    oshape = shape if constrain is None else (int(constrain.constrained_dim),)
    if nested is not None:
        if not (isinstance(nested, NestedAccumulator) and nested.num_chains == C and nested.shape == tuple(oshape)):
            raise ValueError(f"nested must be a NestedAccumulator of {C} chains and shape {tuple(oshape)}")
        if nested.seen + N > nested.num_draws:
            raise ValueError(f"nested has folded {nested.seen} of its {nested.num_draws} draws, {N} more exceed them")
    acc = Accumulator(N, C, oshape, max_lag=max_lag)
    if sketch is not None and not (isinstance(sketch, QuantileSketch) and sketch.num_chains == C
                                   and sketch.shape == acc.shape):
        raise ValueError(f"sketch must be a QuantileSketch of {C} chains and shape {acc.shape}")
    per_draw = C * (D_in if constrain is None else D_in + acc.D) * 8
    wmodel = None if waic is None else waic.pointwise._model
    own = wmodel is not None and wmodel is not constrain  # (the fold maps the rows itself, into a buffer of its own)
    if own:
        per_draw += C * wmodel.constrained_dim * 8
    chunk = min(N, int(chunk) if chunk is not None else max(1, CHUNK_BYTES // per_draw))
    dev = acc._eng.device
    buf = torch.empty(chunk * C * D_in, dtype=torch.float64, device=dev)
    cbuf = None if constrain is None else torch.empty(chunk * C * acc.D, dtype=torch.float64, device=dev)
    wbuf = None
    if own:
        wbuf = torch.empty(min(chunk * C, waic.pointwise._block_rows()) * wmodel.constrained_dim, dtype=torch.float64, device=dev)
    acc_hist = div_hist = info = total = None
    done = 0
    while done < N:
        T = min(chunk, N - done)
        if lengths is not None:
            extra = (lengths[done:done + T],)
        samples, info, a, d = kernel.sample(state, step_size, inverse_mass_matrix, *extra, T, into=buf)
        positions = samples.reshape(T * C, D_in)
        if constrain is not None:
            samples = constrain._constrain_rows(acc._eng, positions, cbuf[:T * C * acc.D].view(T * C, acc.D))
        if waic is not None:
            waic.pointwise._fold(acc._eng, positions, waic, samples if wmodel is not None and wmodel is constrain else None,
                                 wbuf)
        acc.update(samples.reshape((T, C) + oshape))
        if sketch is not None:
            sketch.update(samples.reshape((T, C) + oshape))
        if nested is not None:
            nested.update(samples.reshape((T, C) + oshape))
        if acc_hist is None:
            acc_hist = torch.empty((N,) + tuple(a.shape[1:]), dtype=a.dtype, device=a.device)
            div_hist = torch.empty((N,) + tuple(d.shape[1:]), dtype=d.dtype, device=d.device)
        acc_hist[done:done + T], div_hist[done:done + T] = a, d
        total = info.n_leapfrog if total is None else total + info.n_leapfrog
        state = info.state._replace(momentum=None)
        done += T
    return acc.result(), info._replace(n_leapfrog=total), acc_hist, div_hist
