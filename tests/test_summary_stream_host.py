"""Host-side check of the streaming autocovariance's algebra: the numpy restatement of the ring / head / shift form
(tests/summary_stream_ref.py) against the plain definition (tests/summary_ref.autocovariance), for several chunkings."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import summary_ref as sr  # noqa: E402
import summary_stream_ref as ssr  # noqa: E402

series = ssr.series

TOL = 1e-12  # of W, the mean within-chain variance: fp64 sums of at most 2000 products of O(sd) terms


@pytest.mark.parametrize("N,C,D,split,L,seed,offset",
                         [c + (0.0,) for c in ssr.CASES] + [ssr.OFFSET_CASE + (ssr.OFFSET,)])
def test_streamed_autocovariance_is_the_definition(N, C, D, split, L, seed, offset):
    x = series(seed, N, C, D) + offset
    z = sr.split_chains(x, split)
    K = min(L + 1, z.shape[0])
    want = sr.autocovariance(z, K)
    W = z.var(axis=0, ddof=1).mean(axis=0)
    got = {chunk: ssr.autocovariance(x, split, L, chunk) for chunk in (1, 37, N)}
    for chunk, a in got.items():
        assert a.shape == (K, D)
        err = np.max(np.abs(a - want) / W)
        print("chunk", chunk, "max |acov err| / W", err)
        assert err <= TOL
        assert np.array_equal(a, got[1])  # the restatement folds draw by draw: the chunking cannot matter


def test_a_chain_that_never_moves_gives_exact_zeros():
    x = series(21, 200, 16, 5)
    x[:, :, 3] = 1.25
    x[:, :, 4] = np.arange(16)[None, :]
    a = ssr.autocovariance(x, True, 20, 37)
    assert np.all(a[:, 3:] == 0.0)
