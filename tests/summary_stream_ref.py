"""numpy restatement of the streaming autocovariance (include/aehmc_hip.h, aehmc_summary_lag_update), written from its
formula: lagged products of draws shifted by the segment's first draw, over a ring of the last K - 1 of them, centred
when the segment ends.  Imports nothing from aehmc_amd, and no torch.

A segment of n draws x_0 ... x_{n-1} of one chain, a = x_0, y_t = x_t - a, K lags:
  R(k) = sum_{t >= k} y_t y_{t-k},  Y = sum y_t,  head = y_0 ... y_{K-2},  ring = the last K - 1 of the y seen so far;
at the segment's end, with ybar = Y / n and first_k / last_k the sums of the first / last k shifted draws,
  n acov(k) = R(k) - ybar (2 Y - first_k - last_k) + (n - k) ybar^2."""
import numpy as np

import summary_ref as sr


def series(seed, N, C, D):
    """AR(1) draws with a correlation, a location and a scale per coordinate, and a small offset per chain: the
    series of tests/test_gpu_summary.py, draw for draw, for tests that must run without torch."""
    r = np.random.default_rng(seed)
    phi = r.uniform(-0.3, 0.8, size=D)
    x = sr.ar1(r, N, C, D, phi, loc=r.normal(size=D) * 3.0, scale=0.5 + r.random(D))
    return x + 0.05 * r.normal(size=(1, C, D))


class StreamingAutocov:
    """update(chunk [T, C, D]) folds the next draws of a run of N; result() is acov [K, D], the mean over the split
    chains, once all have arrived.  Segment 1 reuses the state of segment 0; an odd run's middle draw is skipped."""

    def __init__(self, N, C, D, split, max_lag):
        self.N, self.C, self.D, self.S = N, C, D, 2 if split else 1
        self.n = N // self.S
        self.K = min(int(max_lag) + 1, self.n)
        K = self.K
        self.shift, self.sums = np.zeros((C, D)), np.zeros((C, D))
        self.ring, self.head = np.zeros((K - 1, C, D)), np.zeros((K - 1, C, D))
        self.prod = np.zeros((K, C, D))
        self.acov = np.zeros((K, D))
        self.seen = 0

    def update(self, chunk):
        N, n, K = self.N, self.n, self.K
        for row in np.asarray(chunk, dtype=np.float64):
            t = self.seen
            self.seen += 1
            if self.S == 1 or t < n:
                p = t
            elif t >= N - n:
                p = t - (N - n)
            else:
                continue  # the middle draw of an odd run
            if p == 0:
                self.shift[...] = row
                self.sums[...] = 0.0
                self.prod[...] = 0.0
            y = row - self.shift
            self.prod[0] += y * y
            for k in range(1, min(K - 1, p) + 1):
                self.prod[k] += y * self.ring[(p - k) % (K - 1)]
            self.sums += y
            if p < K - 1:
                self.head[p] = y
            self.ring[p % (K - 1)] = y
            if p == n - 1:
                self._end_segment()
        return self

    def _end_segment(self):
        n, K = self.n, self.K
        ybar = self.sums / n
        first = last = 0.0
        for k in range(K):
            if k:
                first = first + self.head[k - 1]
                last = last + self.ring[(n - k) % (K - 1)]
            chains = self.prod[k] - ybar * (2.0 * self.sums - first - last) + (n - k) * ybar * ybar
            self.acov[k] += chains.sum(axis=0) / n

    def result(self):
        assert self.seen == self.N
        return self.acov / (self.S * self.C)


def autocovariance(x, split, max_lag, chunk):
    """acov [K, D] of x [N, C, D] streamed in chunks of `chunk` draws"""
    N, C, D = x.shape
    s = StreamingAutocov(N, C, D, split, max_lag)
    for lo in range(0, N, chunk):
        s.update(x[lo:lo + chunk])
    return s.result()


# (N, C, D, split, max_lag, seed of series): shapes whose restatement has no deciding pair sum within
# 1e-9 of zero.  odd N with the middle draw skipped; whole chains; K at the segment length; a small run; max_lag = 1 with
# D just past a 64 block; 64 lags unsplit; the smallest run; max_lag above the segment length (K clipped to n)
CASES = [(401, 5, 70, True, 40, 408), (100, 64, 3, False, 10, 107), (75, 130, 1, True, 36, 82), (9, 3, 2, True, 3, 5),
         (8, 2, 65, True, 1, 6), (1000, 3, 64, False, 63, 9), (4, 1, 1, True, 1, 3), (5, 3, 2, True, 5, 4)]
# the same series 1e4 away from zero: products of unshifted draws would lose seven digits here
OFFSET_CASE, OFFSET = (2000, 4, 3, True, 20, 77), 1e4
