"""The fp64 MFMA GEMM (csrc/gemm_f64.cuh) on VIEWS into larger buffers, through the raw aehmc_gemm_nt /
aehmc_gemm_nt_tri ABI: leading dimensions larger than the operands, bases in the middle of a buffer, rows of very
different scale, and where a NaN or an infinity may travel -- one case per kernel route of launch_gemm_nt_f64, at the
smallest shape that takes it.  (The dense-metric factorisation is the only caller that passes lda > K, ldc > N and
offset bases; its modes C -= A B^T and C = -A B^T have no ABI of their own and are covered by
tests/test_gpu_dense_factor.py.)

The route of every case is derived from the dispatcher's conditions (`vec` = lda, ldb even and A, B 16-byte aligned;
Tm = ceil(M / 128), Tn = ceil(N / 128), total = Tm Tn; the stream-K grids of a 256-CU device are 512 (two workgroups
per CU) and 256 (one)), not from what the kernels return.  A run with bases one double into their buffers or with odd
lda / ldb has vec = false: M <= 128 and the forced-tiled cases then take gemm_nt_f64_kernel<false>, the small-tile cases
gemm_nt_f64_small_kernel<.., false>, the stream-K cases gemm_nt_f64_kernel<false> -- every variant sums the same
k-chain, so the bits must not change.

Per case:
  strides and guards   lda = K + 6, ldb = K + 10, ldc = N + 3 (odd on purpose) and N + 4, M + 2 rows of C; NaN in the pad
                       columns of A and B, a sentinel bit pattern in the pad columns and extra rows of C (and in the rows a
                       compacted row list leaves out).  The result is bitwise the product of contiguous copies, every
                       sentinel survives.
  offset bases         A and B one double into their buffers (8-byte aligned only); odd lda and ldb: the same bits.
  accuracy             against the longdouble product of the same operands, componentwise
                       |err| <= gamma_K (|A| |B|^T), gamma_K = K u / (1 - K u), u = 2^-53: it holds for ANY summation order,
                       with or without fused multiply-adds, so it needs no measurement.  Also with the rows of A and B
                       scaled by 10^U(-8, 8).  (|A| |B|^T is formed in fp64: a sum of non-negative terms, good to 1e-13.
                       Above 6e8 multiply-adds -- the 4096 x 2048 x 2048 products alone -- the
                       longdouble product is formed for 6e8 / (N K) = 143 rows -- the first, the
                       last and a random draw of the others; every row is still compared bitwise with the contiguous
                       product.)
  non-finite values    one NaN at A[m*, k*], one +inf at B[n*, k']; m* and n* in the last (partial) tile, and m* = 0 (the
                       tail kernel loads row 0 for its padding rows).  Outside row m* and column n* the output is bit-equal
                       to the clean run, inside it is non-finite.  With a triangular hint the header's rule applies: the NaN
                       reaches the 256-wide column tiles whose executed K range holds k*, the others keep the clean bits."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LD = np.longdouble
SENT = 0x7FF85A5A12345678  # a NaN with a payload no arithmetic produces
U = 2.0 ** -53
LD_MACS = 6e8
TRI_BN = 256  # column-tile width of the kernel that honours the hint (gemm_nt_f64_streamk_kernel<true, 8>)


@pytest.fixture(scope="module")
def eng():
    from aehmc_amd.engine import get_engine
    return get_engine()


def case(M, N, K, route, small=1, streamk=2, tri=0, rows=0):
    return pytest.param(M, N, K, small, streamk, tri, rows, id=f"{M}x{N}x{K}-{route}")


CASES = []
# mode 0, vec, M <= 128: the tail kernels -- M <= 16 <1,6>, <= 32 <2,4>, <= 64 <4,3>, else <8,2> (K even: lda, ldb even)
for _M, _t in ((1, "tail16"), (16, "tail16"), (17, "tail24"), (33, "tail43"), (65, "tail82"), (128, "tail82")):
    for _N, _K in ((16, 16), (50, 38), (64, 64)):
        CASES.append(case(_M, _N, _K, _t))
# M > 128, N <= 2048, K >= 2, total < 256, gemm_small_tiles 3 / 2 / 4: 64 x 128, 64 x 64, 32 x 64 tiles; K even: <.., true>
for _M, _N, _K in ((129, 65, 66), (333, 200, 78)):
    for _s, _t in ((3, "small64x128"), (2, "small64x64"), (4, "small32x64")):
        CASES.append(case(_M, _N, _K, _t, small=_s))
# gemm_small_tiles 0 and streamk 0 (no GemmStreamK): gemm_nt_f64_kernel<vec>; K = 333: lda = 339 is odd, <false> throughout
CASES.append(case(130, 257, 50, "tiled128-vec", small=0, streamk=0))
CASES.append(case(517, 129, 333, "tiled128-scalar", small=0, streamk=0))
# N = 8000 > 2048: no small tiles.  streamk 2: K % 16 == 0, Tm ceil(N / 256) = 9 x 32 = 288 >= 256: <true, 8>, hybrid
# schedule (288 tiles x 4 K-tiles cut into ranges of 5: tiles are handed between neighbours).  streamk 1: total =
# 9 x 63 = 567 >= 512: <true, 4>, ranges of 5 again
CASES.append(case(1100, 8000, 64, "streamk-wide", streamk=2))
CASES.append(case(1100, 8000, 64, "streamk-128", streamk=1))
# gemm_small_tiles 0, streamk 2: 3 x 4 = 12 wide tiles < 256, M > 128, K % 16 == 0: <true, 4, true> (pipelined 128 x 128)
CASES.append(case(300, 1000, 64, "streamk-pipe128", small=0, streamk=2))
# total = 32 x 16 = 512 (no small tiles), Tm ceil(N / 256) = 32 x 8 = 256 >= 256: <true, 8, true, tri>; 4000 of 4096 rows
CASES.append(case(4096, 2048, 2048, "tri-lower", tri=1, rows=4000))
CASES.append(case(4096, 2048, 2048, "tri-upper", tri=2, rows=4000))


def bits(t):
    return t.contiguous().view(torch.int64)


def embed(x, ld, off):
    """x [R, K] as a view with row stride ld that starts `off` doubles into a NaN-filled buffer -> (buffer, address)."""
    R, K = x.shape
    buf = torch.full((off + R * ld,), float("nan"), dtype=torch.float64, device="cuda")
    buf[off:].view(R, ld)[:, :K] = x
    return buf, buf.data_ptr() + 8 * off


def product(eng, A, B, pad=(0, 0, 0), off=0, tri=0, rows=None):
    """A B^T of the device matrices A [M, K], B [N, K] with lda = K + pad[0], ldb = K + pad[1], ldc = N + pad[2] and
    M + 2 rows of C (no extra rows when unpadded); checks the sentinels and returns C [M, N] (sentinel bits in the rows a
    row list leaves out)."""
    (M, K), N = A.shape, B.shape[0]
    lda, ldb, ldc = K + pad[0], K + pad[1], N + pad[2]
    Mc = M + (2 if pad[2] else 0)
    bufA, pA = embed(A, lda, off)
    bufB, pB = embed(B, ldb, off)
    C = torch.full((Mc, ldc), SENT, dtype=torch.int64, device="cuda")
    if tri == 0 and rows is None:
        rc = eng.lib.aehmc_gemm_nt(eng.ctx, M, N, K, pA, lda, pB, ldb, C.data_ptr(), ldc, eng.stream)
    else:
        ri, nr = (rows[0].data_ptr(), rows[1].data_ptr()) if rows is not None else (None, None)
        rc = eng.lib.aehmc_gemm_nt_tri(eng.ctx, M, N, K, pA, lda, pB, ldb, C.data_ptr(), ldc, tri, ri, nr, eng.stream)
    eng._check(rc, "aehmc_gemm_nt")
    untouched = torch.ones((Mc, ldc), dtype=torch.bool, device="cuda")
    if rows is None:
        untouched[:M, :N] = False
    else:
        untouched[rows[2], :N] = False
    assert bool((C[untouched] == SENT).all()), f"C was written outside its {M} x {N} elements (pad {pad}, offset {off})"
    assert bool((C[~untouched] != SENT).all()), "elements of C were not written"
    del bufA, bufB
    return C[:M, :N].contiguous().view(torch.float64)


def check_accuracy(C, A, B, written, what):
    """|C - A B^T| <= gamma_K |A| |B|^T against the longdouble product, on the rows `written` (a sample of them above
    LD_MACS multiply-adds)."""
    (M, K), N = A.shape, B.shape[0]
    rows = np.asarray(written)
    cap = max(4, int(LD_MACS // (N * K)))
    if len(rows) > cap:
        pick = np.random.default_rng(K).choice(rows[2:-2], size=cap - 4, replace=False)
        rows = np.concatenate([rows[:2], np.sort(pick), rows[-2:]])
    a, b = A.cpu().numpy()[rows], B.cpu().numpy()
    ref = a.astype(LD) @ b.astype(LD).T
    err = np.abs(C.cpu().numpy()[rows].astype(LD) - ref)
    gamma = K * U / (1 - K * U)
    bound = gamma * (np.abs(a) @ np.abs(b).T)
    worst = float((err / np.maximum(bound, np.finfo(np.float64).tiny)).max())
    print(f"{what}: largest |err| / (gamma_K |A||B|^T) = {worst:.4f} over {len(rows)} rows")
    assert (err <= bound).all(), what


@pytest.mark.parametrize("M,N,K,small,streamk,tri,n_rows", CASES)
def test_gemm_on_views(eng, M, N, K, small, streamk, tri, n_rows):
    r = np.random.default_rng([M, N, K, tri])
    A_h, B_h = r.normal(size=(M, K)), r.normal(size=(N, K))
    if tri:  # 1: B[n, k] == 0 for k > n;  2: for k < n
        B_h = np.tril(B_h) if tri == 1 else np.triu(B_h)
    A, B = torch.as_tensor(A_h, device="cuda"), torch.as_tensor(B_h, device="cuda")
    rows, written = None, np.arange(M)
    if n_rows:  # a compacted row list: n_rows distinct rows in random order
        written = r.permutation(M)[:n_rows]
        rows = (torch.as_tensor(written.astype(np.int32), device="cuda"),
                torch.as_tensor(np.array([n_rows], dtype=np.int32), device="cuda"), torch.as_tensor(written, device="cuda"))
    PAD = (6, 10, 3)
    try:
        eng.set_option("gemm_small_tiles", small)
        eng.set_option("streamk", streamk)
        run = lambda a, b, **kw: product(eng, a, b, tri=tri, rows=rows, **kw)  # noqa: E731
        # ---- strides and guards, offset bases
        flat = run(A, B)
        clean = run(A, B, pad=PAD)
        assert torch.equal(bits(clean), bits(flat)), "lda = K + 6, ldb = K + 10, ldc = N + 3"
        assert torch.equal(bits(run(A, B, pad=(6, 10, 4))), bits(flat)), "ldc = N + 4"
        assert torch.equal(bits(run(A, B, pad=PAD, off=1)), bits(flat)), "A and B one double into their buffers"
        assert torch.equal(bits(run(A, B, pad=(7, 11, 3))), bits(flat)), "odd lda and ldb"
        # ---- accuracy, also with rows of very different scale
        check_accuracy(clean, A, B, written, "N(0, 1) operands")
        sA = torch.as_tensor(10.0 ** r.uniform(-8, 8, size=(M, 1)), device="cuda")
        sB = torch.as_tensor(10.0 ** r.uniform(-8, 8, size=(N, 1)), device="cuda")
        As, Bs = A * sA, B * sB
        mixed = run(As, Bs, pad=PAD)
        assert torch.equal(bits(mixed), bits(run(As, Bs))), "mixed scales: strided against contiguous"
        assert torch.equal(bits(run(As, Bs, pad=(7, 11, 4), off=1)), bits(mixed)), "mixed scales: odd strides, offset bases"
        check_accuracy(mixed, As, Bs, written, "rows scaled by 10^U(-8, 8)")
        # ---- where a non-finite value may go
        ks = 1000 if tri else K - 1                            # tri: splits the column tiles into reached / not reached
        ns, kp = N - 1, (K - 1 if tri == 2 else K // 2)       # (tri: the infinity lies inside B's non-zero triangle)
        cols = torch.arange(N, device="cuda")
        if tri == 1:    # column tile tn runs k < (tn + 1) TRI_BN
            reached = (cols // TRI_BN + 1) * TRI_BN > ks
        elif tri == 2:  # column tile tn runs k >= tn TRI_BN
            reached = (cols // TRI_BN) * TRI_BN <= ks
        else:
            reached = torch.ones(N, dtype=torch.bool, device="cuda")
        live = torch.zeros(M, dtype=torch.bool, device="cuda")
        live[torch.as_tensor(written, device="cuda")] = True
        for ms in sorted({int(written[-1]), int(written[0])}):  # the last (partial) row tile, and the first row
            An, Bn = A.clone(), B.clone()
            An[ms, ks] = float("nan")
            Bn[ns, kp] = float("inf")
            out = run(An, Bn, pad=PAD)
            hit = torch.zeros((M, N), dtype=torch.bool, device="cuda")
            hit[ms, reached] = True
            hit[:, ns] = True
            hit &= live[:, None]
            same = bits(out) == bits(clean)
            assert bool(same[~hit].all()), f"a non-finite value left row {ms} / column {ns}"
            assert bool((~torch.isfinite(out[hit])).all()), f"finite elements in row {ms} / column {ns}"
    finally:
        eng.set_option("gemm_small_tiles", 1)
        eng.set_option("streamk", 2)
