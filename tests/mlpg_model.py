"""
numpy model of the MLPG kernels (magphase_amd/csrc/magphase_mlpg.hip), one function per kernel:

    dense_system / solve_dense   k_mlpg_solve: the dense W_k, A = sum_k W_k^T P_k W_k and b = sum_k W_k^T P_k mu_k of ONE
                                 system (one utterance, one dimension) in float64 or longdouble, and c = A^-1 b
    apply                        k_mlpg_apply: the stencil y_k = [P_k] W_k x
    backward                     the backward formulas z = A^-1 g, dL/dmu_k = P_k W_k z
    ldl_emulation                the kernel's banded LDL^T in float64 and in the kernel's operation order (without its
                                 fused multiply-adds: numpy has none, every a*b+c below rounds twice)

A system's operands: mu [F x K] (column k = stream k), var [F x K] (a global variance broadcast to F rows), windows
[n_win x 3] taps (w[-1], w[0], w[+1]); stream 0 is static.
"""
import numpy as np

U = 2.0 ** -53
SOLVE_BACKWARD_BOUND = 16 * U    # eta: <= 7 rounded terms per band entry + the bandwidth-2 factorisation + two substitutions
APPLY_BOUND = 4 * U              # one product, two fused multiply-adds, one division
WINDOWS = ((-0.5, 0.0, 0.5), (1.0, -2.0, 1.0))


def taps(windows, dtype=np.float64):
    """[K x 3] taps, stream 0 = (0, 1, 0)."""
    return np.vstack([[0.0, 1.0, 0.0], np.asarray(windows, dtype=np.float64).reshape(-1, 3)]).astype(dtype)


def dense_w(F, w, dtype=np.float64):
    """W[t, t + j] = w[j + 1] for 0 <= t + j < F: taps outside the utterance are dropped."""
    W = np.zeros((F, F), dtype=dtype)
    for t in range(F):
        for j in (-1, 0, 1):
            if 0 <= t + j < F:
                W[t, t + j] = w[j + 1]
    return W


def dense_system(mu, var, windows=WINDOWS, dtype=np.float64):
    """(A [F x F], b [F], [W_k], [p_k]) of one system in `dtype`; mu may be None (A only, b = None)."""
    var = np.asarray(var, dtype=dtype)
    F, K = var.shape
    tp = taps(windows, dtype)
    assert tp.shape[0] == K
    A = np.zeros((F, F), dtype=dtype)
    b = None if mu is None else np.zeros(F, dtype=dtype)
    Ws, ps = [], []
    for k in range(K):
        W = dense_w(F, tp[k], dtype)
        p = np.ones(F, dtype=dtype) / var[:, k]
        A += W.T @ (p[:, None] * W)
        if mu is not None:
            b += W.T @ (p * np.asarray(mu, dtype=dtype)[:, k])
        Ws.append(W)
        ps.append(p)
    return A, b, Ws, ps


def gauss_solve(A, b):
    """A^-1 b by elimination without pivoting in A's own dtype (A is symmetric positive definite; longdouble has no LAPACK)."""
    A = A.copy()
    x = b.copy()
    n = len(x)
    for i in range(n):
        for r in range(i + 1, min(i + 3, n)):   # bandwidth 2
            m = A[r, i] / A[i, i]
            A[r, i:min(i + 3, n)] -= m * A[i, i:min(i + 3, n)]
            x[r] -= m * x[i]
    for i in range(n - 1, -1, -1):
        x[i] = (x[i] - A[i, i + 1:min(i + 3, n)] @ x[i + 1:min(i + 3, n)]) / A[i, i]
    return x


def solve_dense(mu, var, windows=WINDOWS, dtype=np.float64):
    A, b, _, _ = dense_system(mu, var, windows, dtype)
    return np.linalg.solve(A, b) if dtype == np.float64 else gauss_solve(A, b)


def apply(x, var, windows=WINDOWS, dtype=np.float64):
    """y [F x K] = [P_k] W_k x of one column x [F]; var: [F x K] or None."""
    x = np.asarray(x, dtype=dtype)
    F = len(x)
    tp = taps(windows, dtype)
    y = np.zeros((F, tp.shape[0]), dtype=dtype)
    for k in range(tp.shape[0]):
        y[:, k] = dense_w(F, tp[k], dtype) @ x
        if var is not None:
            y[:, k] = y[:, k] / np.asarray(var, dtype=dtype)[:, k]
    return y


def apply_abs_terms(x, var, windows=WINDOWS):
    """sum_j |w_k[j] x[t + j]| [/ var]: what the stencil's rounding error is relative to."""
    tpa = np.abs(np.asarray(windows, dtype=np.float64).reshape(-1, 3))
    v = None if var is None else np.abs(np.asarray(var, dtype=np.float64))
    return apply(np.abs(np.asarray(x, dtype=np.float64)), v, tpa)


def backward(g, var, windows=WINDOWS, dtype=np.float64):
    """dL/dmu [F x K] for g = dL/dc [F]: z = A^-1 g, dL/dmu_k = P_k W_k z."""
    A, _, Ws, ps = dense_system(None, var, windows, dtype)
    g = np.asarray(g, dtype=dtype)
    z = np.linalg.solve(A, g) if dtype == np.float64 else gauss_solve(A, g)
    return np.stack([p * (W @ z) for W, p in zip(Ws, ps)], axis=1)


def ldl_emulation(mu, var, windows=WINDOWS):
    """k_mlpg_solve on one system, float64, the kernel's order of operations (see the module docstring for the one
    difference).  -> c [F]."""
    mu = np.asarray(mu, dtype=np.float64)
    var = np.asarray(var, dtype=np.float64)
    F, K = var.shape
    w = taps(windows)
    aa = np.stack([w[:, 2] * w[:, 2], w[:, 1] * w[:, 1], w[:, 0] * w[:, 0]], axis=1)
    e0, e1, ff = w[:, 1] * w[:, 2], w[:, 0] * w[:, 1], w[:, 0] * w[:, 2]
    p = np.zeros((F + 3, K))      # rows -1 .. F + 1 at index i + 1: zero outside the utterance
    q = np.zeros((F + 3, K))
    p[1:F + 1] = 1.0 / var
    q[1:F + 1] = p[1:F + 1] * mu
    l1s, l2s, z = np.zeros(F), np.zeros(F), np.zeros(F)
    d1 = d2 = 1.0
    l1p = y1 = y2 = e_1 = f1 = f2 = 0.0
    for i in range(F):
        a = e = f = r = 0.0
        for k in range(K):
            for j in range(3):
                a = a + aa[k, j] * p[i + j, k]
                r = r + w[k, 2 - j] * q[i + j, k]
            e = e + e0[k] * p[i + 1, k]
            e = e + e1[k] * p[i + 2, k]
            f = f + ff[k] * p[i + 2, k]
        l2 = f2 / d2
        v = e_1 - f2 * l1p
        l1 = v / d1
        dd = (a - l1 * v) - l2 * f2
        y = (r - l1 * y1) - l2 * y2
        l1s[i], l2s[i], z[i] = l1, l2, y / dd
        d2, d1, l1p, y2, y1, f2, f1, e_1 = d1, dd, l1, y1, y, f1, f, e
    c = np.zeros(F)
    c1 = c2 = 0.0
    for i in range(F - 1, -1, -1):
        m1 = l1s[i + 1] if i + 1 < F else 0.0
        m2 = l2s[i + 2] if i + 2 < F else 0.0
        c[i] = (z[i] - m1 * c1) - m2 * c2
        c2, c1 = c1, c[i]
    return c


# ---------------------------------------------------------------------------------------------------------------------
# The same system as its three bands, for MANY systems at once (the GPU tests hold every system of a batch to the bounds;
# dense longdouble products of 257 x 257 matrices per system would take minutes).  mu, var: [F x K x S], S systems.
# tests/test_mlpg_host.py holds the bands to dense_system.
# ---------------------------------------------------------------------------------------------------------------------
def band_system(mu, var, windows=WINDOWS, dtype=np.longdouble):
    """(a, e, f, b) [F x S]: a = diag A, e[i] = A[i, i + 1] (row F - 1 zero), f[i] = A[i, i + 2] (rows >= F - 2 zero),
    b = the right-hand side (None when mu is None)."""
    var = np.asarray(var, dtype=dtype)
    F, K, S = var.shape
    w = taps(windows, dtype)
    pp = np.zeros((F + 2, K, S), dtype=dtype)     # row i + 1 = frame i; zero outside the utterance
    pp[1:F + 1] = np.ones((), dtype=dtype) / var
    a, e, f = (np.zeros((F, S), dtype=dtype) for _ in range(3))
    b = None
    if mu is not None:
        qq = np.zeros_like(pp)
        qq[1:F + 1] = pp[1:F + 1] * np.asarray(mu, dtype=dtype)
        b = np.zeros((F, S), dtype=dtype)
    for k in range(K):
        a += w[k, 2] * w[k, 2] * pp[0:F, k] + w[k, 1] * w[k, 1] * pp[1:F + 1, k] + w[k, 0] * w[k, 0] * pp[2:F + 2, k]
        e += w[k, 1] * w[k, 2] * pp[1:F + 1, k] + w[k, 0] * w[k, 1] * pp[2:F + 2, k]
        f += w[k, 0] * w[k, 2] * pp[2:F + 2, k]
        if mu is not None:
            b += w[k, 2] * qq[0:F, k] + w[k, 1] * qq[1:F + 1, k] + w[k, 0] * qq[2:F + 2, k]
    e[F - 1:] = 0
    f[max(F - 2, 0):] = 0
    return a, e, f, b


def band_matvec(a, e, f, c):
    y = a * c
    y[:-1] += e[:-1] * c[1:]
    y[1:] += e[:-1] * c[:-1]
    y[:-2] += f[:-2] * c[2:]
    y[2:] += f[:-2] * c[:-2]
    return y


def band_solve(a, e, f, b):
    """A^-1 b by LDL^T in the operands' dtype, every system at once."""
    F = a.shape[0]
    d, l1, l2, y = (np.zeros_like(a) for _ in range(4))
    for i in range(F):
        if i >= 2:
            l2[i] = f[i - 2] / d[i - 2]
        if i >= 1:
            v = e[i - 1] - (f[i - 2] * l1[i - 1] if i >= 2 else 0)
            l1[i] = v / d[i - 1]
        d[i] = a[i] - (l1[i] * l1[i] * d[i - 1] if i >= 1 else 0) - (l2[i] * l2[i] * d[i - 2] if i >= 2 else 0)
        y[i] = b[i] - (l1[i] * y[i - 1] if i >= 1 else 0) - (l2[i] * y[i - 2] if i >= 2 else 0)
    c = y / d
    for i in range(F - 2, -1, -1):
        c[i] -= l1[i + 1] * c[i + 1] + (l2[i + 2] * c[i + 2] if i + 2 < F else 0)
    return c


def band_dense(a, e, f):
    """[S x F x F] float64."""
    F, S = a.shape
    A = np.zeros((S, F, F))
    i = np.arange(F)
    A[:, i, i] = a.T.astype(np.float64)
    if F > 1:
        A[:, i[:-1], i[1:]] = A[:, i[1:], i[:-1]] = e[:-1].T.astype(np.float64)
    if F > 2:
        A[:, i[:-2], i[2:]] = A[:, i[2:], i[:-2]] = f[:-2].T.astype(np.float64)
    return A


def band_errors(c, mu, var, windows=WINDOWS, rhs=None):
    """Per system (arrays [S]): eta / SOLVE_BACKWARD_BOUND, forward error / (2 kappa_inf 16 u), kappa_inf -- for a computed
    c [F x S]; A and b in longdouble from the operands as given, kappa_inf from the dense float64 A; the reference solution
    is the longdouble LDL^T.  rhs [F x S]: the right-hand side itself instead of mu (the backward pass' solve)."""
    L = np.longdouble
    a, e, f, b = band_system(mu if rhs is None else None, var, windows, L)
    if rhs is not None:
        b = np.asarray(rhs, dtype=L)
    cl = np.asarray(c, dtype=L)
    na = np.abs(a) + np.abs(e) + np.abs(f)
    na[1:] += np.abs(e[:-1])
    na[2:] += np.abs(f[:-2])
    norm_a = np.max(na, axis=0).astype(np.float64)
    den = norm_a * np.max(np.abs(cl), axis=0).astype(np.float64) + np.max(np.abs(b), axis=0).astype(np.float64)
    res = np.max(np.abs(b - band_matvec(a, e, f, cl)), axis=0).astype(np.float64)
    eta = np.where(den > 0, res / np.where(den > 0, den, 1.0), 0.0)
    ref = band_solve(a, e, f, b)
    inv = np.linalg.inv(band_dense(a, e, f))
    kappa = norm_a * np.max(np.sum(np.abs(inv), axis=2), axis=1)
    nref = np.max(np.abs(ref), axis=0).astype(np.float64)
    fwd = np.max(np.abs(cl - ref), axis=0).astype(np.float64) / np.where(nref > 0, nref, 1.0)
    return eta / SOLVE_BACKWARD_BOUND, fwd / (2.0 * kappa * SOLVE_BACKWARD_BOUND), kappa, ref


def errors(c, mu, var, windows=WINDOWS, rhs=None):
    """band_errors for one system (c [F], mu / var [F x K]) -> (eta fraction, forward fraction, kappa)."""
    eta, fwd, kappa, _ = band_errors(np.asarray(c)[:, None], None if mu is None else np.asarray(mu)[:, :, None],
                                     np.asarray(var)[:, :, None], windows, None if rhs is None else np.asarray(rhs)[:, None])
    return float(eta[0]), float(fwd[0]), float(kappa[0])
