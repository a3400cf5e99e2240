"""Extended-precision restatement of the dense-metric factorisation (metrics.py:56-58: L = cholesky(imm),
mass_matrix_sqrt = L^-T), written from the definitions in numpy.longdouble (64-bit mantissa on x86-64: u = 2^-64 against
fp64's 2^-53).  Imports nothing from aehmc_amd.

chol_inv_t(a) -> (L, L^-T): a row-by-row Cholesky of the LOWER triangle of a (the upper one is never read), then
forward substitution for L^-1, both then refined on residuals formed without rounding, so that the result is good to
longdouble's rounding whatever the condition number.  family(): the three kinds of test matrix; rowwise_err(): the
row-scaled error measure; yardstick(): the same operation by LAPACK in fp64, whose own error against chol_inv_t sets what a device factor may
have."""
import numpy as np

LD = np.longdouble
FAMILIES = ("well", "graded", "scaled")


def _factor_plain(a):
    """(L, L^-1) in plain longdouble: row-by-row Cholesky of the lower triangle, then forward substitution."""
    D = a.shape[0]
    L = np.zeros((D, D), dtype=LD)
    for i in range(D):
        for j in range(i):  # L[i, j] = (a[i, j] - sum_k<j L[i, k] L[j, k]) / L[j, j]
            L[i, j] = (a[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
        d = a[i, i] - L[i, :i] @ L[i, :i]
        if not d > 0:
            raise np.linalg.LinAlgError(f"not positive definite (pivot {i + 1})")
        L[i, i] = np.sqrt(d)
    X = np.zeros((D, D), dtype=LD)  # L X = I, row by row: X[i, :] = (e_i - L[i, :i] X[:i, :]) / L[i, i]
    for i in range(D):
        r = -(L[i, :i] @ X[:i, :i + 1]) if i else np.zeros(1, dtype=LD)
        r[i] += LD(1)
        X[i, :i + 1] = r / L[i, i]
    return L, X


def _residual(C, A, B, slices=5):
    """C - A B^T [n, m] for longdouble A [n, K], B [m, K], C, to ~2^-100 of rowmax|A| rowmax|B| per element, however much
    cancels.  Every row is scaled by a power of two below 1 and cut into `slices` integer pieces of b bits with
    2 b + log2 K <= 53, so that the fp64 product of two pieces is exact; the pieces' products are taken off C from the
    largest down with the rounding error of every subtraction carried along (two-sum)."""
    K = A.shape[1]
    b = (53 - int(np.ceil(np.log2(max(K, 2))))) // 2

    def cut(M):
        _, e = np.frexp(np.abs(M).max(axis=1))
        Y, out = np.ldexp(M, -e[:, None]), []
        for _ in range(slices):
            Y = np.ldexp(Y, b)
            T = np.trunc(Y)
            out.append(T.astype(np.float64))
            Y = Y - T
        return e, out

    ea, sa = cut(A)
    eb, sb = cut(B)
    hi = np.ldexp(np.asarray(C, dtype=LD), -(ea[:, None] + eb[None, :]))
    lo = np.zeros_like(hi)
    for w in range(slices):  # weight 2^-(b (w + 2)): the pairs s + t = w (those beyond lie below the last piece's cut)
        for s in range(w + 1):
            t = np.ldexp((sa[s] @ sb[w - s].T).astype(LD), -b * (w + 2))
            x = hi - t
            z = x - hi
            lo += (hi - (x - z)) + (-t - z)
            hi = x
    return np.ldexp(hi + lo, ea[:, None] + eb[None, :])


def _f64_product(A, B):
    """A B in fp64, as longdouble: for CORRECTIONS, which are needed to a few digits only."""
    return (np.asarray(A, dtype=np.float64) @ np.asarray(B, dtype=np.float64)).astype(LD)


def chol_inv_t(a):
    """(L, L^-T) of the symmetric positive definite a [D, D], both longdouble; reads a[i, j] for j <= i only.

    The plain longdouble factor has a forward error of the order cond(a) 2^-64 (1e-13 for the `graded` family: its
    pivots are differences that cancel seven digits).  Refinement takes that out: with the residual R = a - L L^T formed
    without rounding (_residual), a = L (I + F) L^T for F = L^-1 R L^-T, which is tiny, and the Cholesky factor of
    I + F is I + Phi(F) up to F^2, Phi = strict lower triangle + half the diagonal: L <- L + L Phi, L^-1 <- L^-1 - Phi L^-1,
    repeated until F^2 is below longdouble's rounding (once, up to a condition number of ~1e10).  The inverse then gets
    one Newton step X <- X + X (I - L X), again on an unrounded residual.  What is left is the rounding of the results."""
    a = np.asarray(a, dtype=LD)
    D = a.shape[0]
    a = np.tril(a) + np.tril(a, -1).T
    L, X = _factor_plain(a)
    for _ in range(4):
        F = _f64_product(_f64_product(X, _residual(a, L, L)), X.T)
        Phi = np.tril(0.5 * (F + F.T), -1) + 0.5 * np.diag(np.diag(F))
        L, X = L + np.tril(_f64_product(L, Phi)), X - np.tril(_f64_product(Phi, X))
        if D * float(np.abs(F).max()) ** 2 < 2.0 ** -66:
            break
    X = X + np.tril(_f64_product(X, _residual(np.eye(D, dtype=LD), L, X.T.copy())))
    return L, X.T.copy()


def family(kind, D, seed=0):
    """A symmetric positive definite fp64 matrix [D, D] of one of FAMILIES, from a seeded generator.
    well: A A^T / D + 0.5 I;  graded: Q diag(logspace(0, -8, D)) Q^T (condition number 1e8);
    scaled: `well`, then m * s s^T with s = 10^U(-4, 4) (nominal condition number ~1e16; Cholesky is scale-invariant)."""
    r = np.random.default_rng([seed, D, FAMILIES.index(kind)])
    if kind == "graded":
        q, _ = np.linalg.qr(r.normal(size=(D, D)))
        m = (q * np.logspace(0, -8, D)) @ q.T
    else:
        A = r.normal(size=(D, D))
        m = A @ A.T / D + 0.5 * np.eye(D)
        if kind == "scaled":
            s = 10.0 ** r.uniform(-4, 4, size=D)
            m = m * np.outer(s, s)
    return 0.5 * (m + m.T)


def rowwise_err(S, S_ref):
    """[D]: max_j |S - S_ref|[i, j] / max_j |S_ref[i, j]|, in longdouble (the rows of L^-T of a `scaled` matrix differ
    by many orders of magnitude: an error small against the whole matrix may be all of a small row)."""
    S_ref = np.asarray(S_ref, dtype=LD)
    d = np.abs(np.asarray(S, dtype=LD) - S_ref).max(axis=1)
    return d / np.abs(S_ref).max(axis=1)


def yardstick(m):
    """L^-T by the reference's own operation in fp64: solve_triangular(cholesky(m), I, lower=True, trans=1)."""
    from scipy.linalg import solve_triangular
    return solve_triangular(np.linalg.cholesky(m), np.eye(m.shape[0]), lower=True, trans=1)


def bound(D, yard_err):
    """What a device factor may have, row-wise: 8 x max(the yardstick's own error, sqrt(D) 2^-53)."""
    return 8.0 * max(float(yard_err), float(np.sqrt(D)) * 2.0 ** -53)


_CACHE = {}


def reference(kind, D, seed=0):
    """(m, S_ref, yardstick's largest row-wise error) of family(kind, D, seed); computed once per process, the arrays
    read-only."""
    key = (kind, D, seed)
    if key not in _CACHE:
        m = family(kind, D, seed)
        _, S = chol_inv_t(m)
        y = float(rowwise_err(yardstick(m), S).max())
        m.setflags(write=False)
        S.setflags(write=False)
        _CACHE[key] = (m, S, y)
    return _CACHE[key]
