"""
Model of the MLPG variance gradients and the trajectory likelihood (k_mlpg_var_bwd, k_mlpg_nll, k_mlpg_nll_bwd; DESIGN.md
section 3.3n, "variances"), on top of tests/mlpg_model.py (mm).

Dense, ONE system (mu, var [F x K], x, g [F]):
    nll_dense            NLL through slogdet and a dense solve (float64)
    nll_longdouble       the same in longdouble (dense LDL^T: numpy has no longdouble LAPACK)
    torch_grads          gradients of NLL and of a loss <g, c> by torch autograd in float64 on the dense model
    dense_inverse        A^-1 in longdouble, for the band of Z
    var_grad_closed, nll_grads_closed     the closed forms of the issue on dense matrices, any dtype
    recursion_emulation  the kernel's LDL^T and its reverse recursion for the band of Z, float64, the kernel's order (without
                         its fused multiply-adds)
Banded, MANY systems at once (mu, var [F x K x S], x, g [F x S]; what the GPU tests hold every system to):
    band_model           c, z, NLL, its gradients, the variance gradient of <g, c>, the band of Z and kappa_inf, in longdouble
tests/test_mlpg_variance_host.py holds band_model to the dense forms.
"""
import numpy as np

import mlpg_model as mm

U = mm.U
LOG_2PI = np.log(2 * np.pi)


# ----------------------------------------------------------------------------------------------------------------- dense
def nll_dense(mu, var, x, windows=mm.WINDOWS):
    A, b, _, _ = mm.dense_system(mu, var, windows)
    c = np.linalg.solve(A, b)
    e = np.asarray(x, dtype=np.float64) - c
    sign, logdet = np.linalg.slogdet(A)
    assert sign > 0
    return 0.5 * e @ A @ e - 0.5 * logdet + 0.5 * len(e) * LOG_2PI


def ldl_dense(A):
    """(L unit lower, d) with A = L diag(d) L^T, in A's dtype."""
    n = A.shape[0]
    L = np.eye(n, dtype=A.dtype)
    d = np.zeros(n, dtype=A.dtype)
    for i in range(n):
        d[i] = A[i, i] - np.sum(L[i, :i] ** 2 * d[:i])
        for r in range(i + 1, n):
            L[r, i] = (A[r, i] - np.sum(L[r, :i] * L[i, :i] * d[:i])) / d[i]
    return L, d


def nll_longdouble(mu, var, x, windows=mm.WINDOWS):
    Ld = np.longdouble
    A, b, _, _ = mm.dense_system(mu, var, windows, Ld)
    c = mm.gauss_solve(A, b)
    e = np.asarray(x, dtype=Ld) - c
    _, d = ldl_dense(A)
    return Ld(0.5) * (e @ A @ e) - Ld(0.5) * np.sum(np.log(d)) + Ld(0.5) * len(e) * np.log(2 * np.pi * np.ones((), Ld))


def dense_inverse(A):
    """A^-1 in A's dtype, column by column (banded elimination without pivoting)."""
    n = A.shape[0]
    eye = np.eye(n, dtype=A.dtype)
    return np.stack([mm.gauss_solve(A, eye[:, j]) for j in range(n)], axis=1)


def _torch_system(mu, var, windows):
    import torch

    F, K = np.asarray(var).shape
    tp = mm.taps(windows)
    Ws = [torch.from_numpy(mm.dense_w(F, tp[k])) for k in range(K)]
    mu_t = torch.tensor(np.asarray(mu, dtype=np.float64), requires_grad=True)
    var_t = torch.tensor(np.asarray(var, dtype=np.float64), requires_grad=True)
    A = sum(W.T @ torch.diag(1.0 / var_t[:, k]) @ W for k, W in enumerate(Ws))
    b = sum(W.T @ (mu_t[:, k] / var_t[:, k]) for k, W in enumerate(Ws))
    return mu_t, var_t, A, torch.linalg.solve(A, b)


def torch_grads(mu, var, x=None, g=None, windows=mm.WINDOWS):
    """torch autograd, float64, dense.  x given: (NLL, dNLL/dmu, dNLL/dvar); g given: (c, d<g,c>/dmu, d<g,c>/dvar)."""
    import torch

    mu_t, var_t, A, c = _torch_system(mu, var, windows)
    if x is not None:
        e = torch.from_numpy(np.asarray(x, dtype=np.float64)) - c
        val = 0.5 * e @ A @ e - 0.5 * torch.linalg.slogdet(A)[1] + 0.5 * len(e) * LOG_2PI
        loss = val
    else:
        val = c
        loss = torch.from_numpy(np.asarray(g, dtype=np.float64)) @ c
    loss.backward()
    return val.detach().numpy(), mu_t.grad.numpy(), var_t.grad.numpy()


def torch_mvn_nll(mu, var, x, windows=mm.WINDOWS):
    """-log N(x; c, A^-1) by torch.distributions.MultivariateNormal(precision_matrix=A)."""
    import torch

    A, b, _, _ = mm.dense_system(mu, var, windows)
    c = np.linalg.solve(A, b)
    dist = torch.distributions.MultivariateNormal(torch.from_numpy(c), precision_matrix=torch.from_numpy(A))
    return -float(dist.log_prob(torch.from_numpy(np.asarray(x, dtype=np.float64))))


def var_grad_closed(mu, var, g, windows=mm.WINDOWS, dtype=np.float64):
    """A of the issue: d<g,c>/dvar_k[t] = -p_k[t]^2 (W_k z)[t] (mu_k[t] - (W_k c)[t]), z = A^-1 g.  -> [F x K]."""
    A, b, Ws, ps = mm.dense_system(mu, var, windows, dtype)
    solve = np.linalg.solve if dtype == np.float64 else mm.gauss_solve
    c, z = solve(A, b), solve(A, np.asarray(g, dtype=dtype))
    mu = np.asarray(mu, dtype=dtype)
    return np.stack([-p * p * (W @ z) * (mu[:, k] - W @ c) for k, (W, p) in enumerate(zip(Ws, ps))], axis=1)


def nll_grads_closed(mu, var, x, windows=mm.WINDOWS, dtype=np.float64):
    """B of the issue -> (dNLL/dmu, dNLL/dvar) [F x K], s_k from the dense inverse."""
    A, b, Ws, ps = mm.dense_system(mu, var, windows, dtype)
    c = (np.linalg.solve if dtype == np.float64 else mm.gauss_solve)(A, b)
    Z = np.linalg.inv(A) if dtype == np.float64 else dense_inverse(A)
    e = np.asarray(x, dtype=dtype) - c
    mu = np.asarray(mu, dtype=dtype)
    half = np.ones((), dtype) / 2
    gm, gv = [], []
    for k, (W, p) in enumerate(zip(Ws, ps)):
        we, s = W @ e, np.diag(W @ Z @ W.T)
        gm.append(-p * we)
        gv.append(-p * p * (half * we * we - we * (mu[:, k] - W @ c) - half * s))
    return np.stack(gm, axis=1), np.stack(gv, axis=1)


def recursion_emulation(var, windows=mm.WINDOWS):
    """The forward LDL^T sweep of k_mlpg_nll_bwd and its reverse recursion on one system, float64, the kernel's order.
    -> (d [F], Z band [F x 3]: Z[i, i], Z[i, i + 1], Z[i, i + 2] (zero past F), s [F x K]: (W_k Z W_k^T)[t, t])."""
    var = np.asarray(var, dtype=np.float64)
    F, K = var.shape
    w = mm.taps(windows)
    aa = np.stack([w[:, 2] * w[:, 2], w[:, 1] * w[:, 1], w[:, 0] * w[:, 0]], axis=1)
    e0, e1, ff = w[:, 1] * w[:, 2], w[:, 0] * w[:, 1], w[:, 0] * w[:, 2]
    p = np.zeros((F + 3, K))
    p[1:F + 1] = 1.0 / var
    l1s, l2s, dinv, ds = np.zeros(F), np.zeros(F), np.zeros(F), np.zeros(F)
    d1 = d2 = 1.0
    l1p = e_1 = f1 = f2 = 0.0
    for i in range(F):
        a = e = f = 0.0
        for k in range(K):
            for j in range(3):
                a = a + aa[k, j] * p[i + j, k]
            e = e + e0[k] * p[i + 1, k]
            e = e + e1[k] * p[i + 2, k]
            f = f + ff[k] * p[i + 2, k]
        l2 = f2 / d2
        v = e_1 - f2 * l1p
        l1 = v / d1
        dd = (a - l1 * v) - l2 * f2
        l1s[i], l2s[i], dinv[i], ds[i] = l1, l2, 1.0 / dd, dd
        d2, d1, l1p, f2, f1, e_1 = d1, dd, l1, f1, f, e
    Z = np.zeros((F, 3))
    s = np.zeros((F, K))
    z11 = z12 = z22 = 0.0
    for i in range(F - 1, -2, -1):
        m1 = l1s[i + 1] if 0 <= i and i + 1 < F else 0.0
        m2 = l2s[i + 2] if 0 <= i and i + 2 < F else 0.0
        di = dinv[i] if i >= 0 else 0.0
        z01 = -m1 * z11 - m2 * z12
        z02 = -m1 * z12 - m2 * z22
        z00 = (di - m1 * z01) - m2 * z02
        if i >= 0:
            Z[i] = z00, z01, z02
        t = i + 1
        if t < F:
            for k in range(K):
                diag = (aa[k, 0] * z22 + aa[k, 1] * z11) + aa[k, 2] * z00
                offd = (e1[k] * z01 + ff[k] * z02) + e0[k] * z12
                s[t, k] = diag + 2.0 * offd
        z22, z12, z11 = z11, z01, z00
    return ds, Z, s


# ------------------------------------------------------------------------------------------------- banded, many systems
def _stencil(w, x):
    """(W x)[t] = w[0] x[t - 1] + w[1] x[t] + w[2] x[t + 1], taps outside dropped; x [F x S]."""
    y = w[1] * x
    y[1:] += w[0] * x[:-1]
    y[:-1] += w[2] * x[1:]
    return y


def band_model(mu, var, x=None, g=None, go=None, windows=mm.WINDOWS, dtype=np.longdouble, c=None):
    """Every system of one utterance at once.  mu, var: [F x K x S]; x (static target), g (dL/dc): [F x S] or None; go: [S]
    upstream gradient of the NLL (default 1); c [F x S]: the trajectory as a kernel received it, in place of the model's own
    (the likelihood kernels take c from a preceding solve).  -> dict of arrays in `dtype`:
        c [F x S]; kappa [S] (float64, of the dense float64 A); Z [F x 3 x S] (Z[i,i], Z[i,i+1], Z[i,i+2]); s [F x K x S]
        x given: nll [S], nll_g_mean, nll_g_var [F x K x S] (times go)
        g given: z [F x S], traj_g_var [F x K x S]"""
    var = np.asarray(var, dtype=dtype)
    mu = np.asarray(mu, dtype=dtype)
    F, K, S = var.shape
    w = mm.taps(windows, dtype)
    one, half = np.ones((), dtype), np.ones((), dtype) / 2
    pk = one / var
    a, e, f, b = mm.band_system(mu, var, windows, dtype)
    # LDL^T (as mm.band_solve), the pivots kept
    d, l1, l2 = (np.zeros_like(a) for _ in range(3))
    for i in range(F):
        if i >= 2:
            l2[i] = f[i - 2] / d[i - 2]
        if i >= 1:
            l1[i] = (e[i - 1] - (f[i - 2] * l1[i - 1] if i >= 2 else 0)) / d[i - 1]
        d[i] = a[i] - (l1[i] * l1[i] * d[i - 1] if i >= 1 else 0) - (l2[i] * l2[i] * d[i - 2] if i >= 2 else 0)
    out = {"c": mm.band_solve(a, e, f, b) if c is None else np.asarray(c, dtype=dtype), "d": d}
    c = out["c"]
    # the band of Z = A^-1
    Z = np.zeros((F + 2, 3, S), dtype=dtype)
    for i in range(F - 1, -1, -1):
        m1 = l1[i + 1] if i + 1 < F else 0
        m2 = l2[i + 2] if i + 2 < F else 0
        Z[i, 1] = -m1 * Z[i + 1, 0] - m2 * Z[i + 1, 1]
        Z[i, 2] = -m1 * Z[i + 1, 1] - m2 * Z[i + 2, 0]
        Z[i, 0] = one / d[i] - m1 * Z[i, 1] - m2 * Z[i, 2]
    out["Z"] = Z[:F]
    Zp = np.zeros((F + 3, 3, S), dtype=dtype)      # row t + 1 = Z row t; rows -1, F, F + 1 zero
    Zp[1:F + 1] = Z[:F]
    s = np.zeros((F, K, S), dtype=dtype)
    for k in range(K):
        wm, w0, wp = w[k]
        s[:, k] = wm * wm * Zp[0:F, 0] + w0 * w0 * Zp[1:F + 1, 0] + wp * wp * Zp[2:F + 2, 0] \
            + 2 * (wm * w0 * Zp[0:F, 1] + wm * wp * Zp[0:F, 2] + w0 * wp * Zp[1:F + 1, 1])
    # taps whose frame lies outside the utterance are dropped: Z rows there are zero already, but Z[F-1, 1..2] and Z[F-2, 2]
    # are zero by construction as well (m1, m2 = 0 multiply zeros)
    out["s"] = s
    inv = np.linalg.inv(mm.band_dense(a, e, f))
    na = np.abs(a) + np.abs(e) + np.abs(f)
    na[1:] += np.abs(e[:-1])
    na[2:] += np.abs(f[:-2])
    out["kappa"] = np.max(na, axis=0).astype(np.float64) * np.max(np.sum(np.abs(inv), axis=2), axis=1)
    if x is not None:
        ev = np.asarray(x, dtype=dtype) - c
        gof = np.ones(S, dtype=dtype) if go is None else np.asarray(go, dtype=dtype)
        quad = np.zeros(S, dtype=dtype)
        gm, gv = np.zeros_like(var), np.zeros_like(var)
        for k in range(K):
            we, wc = _stencil(w[k], ev), _stencil(w[k], c)
            quad += np.sum(pk[:, k] * we * we, axis=0)
            gm[:, k] = -gof * pk[:, k] * we
            gv[:, k] = -gof * pk[:, k] ** 2 * (half * we * we - we * (mu[:, k] - wc) - half * s[:, k])
        out["nll"] = half * quad - half * np.sum(np.log(d), axis=0) + half * F * np.log(2 * np.pi * one)
        out["nll_g_mean"], out["nll_g_var"] = gm, gv
    if g is not None:
        z = mm.band_solve(a, e, f, np.asarray(g, dtype=dtype))
        tv = np.zeros_like(var)
        for k in range(K):
            tv[:, k] = -pk[:, k] ** 2 * _stencil(w[k], z) * (mu[:, k] - _stencil(w[k], c))
        out["z"], out["traj_g_var"] = z, tv
    return out


def var_bwd_entry_model(z, c, mu, var, windows=mm.WINDOWS, dtype=np.longdouble):
    """k_mlpg_var_bwd on the operands as it receives them (z, c [F x S]; mu, var [F x K x S]) -> (model [F x K x S] in dtype,
    allowance [F x K x S] float64).  The allowance: with Sz = sum_j |w_k[j] z[t + j]|, Sc likewise, the stencils carry at
    most mm.APPLY_BOUND Sz and mm.APPLY_BOUND Sc; mu - W_k c one more rounding, p^2 three (a division, two products), the
    two outer products two: |error| <= p^2 Sz (|mu| + Sc) (2 mm.APPLY_BOUND + 6 u)."""
    zl, cl = np.asarray(z, dtype=dtype), np.asarray(c, dtype=dtype)
    mu, var = np.asarray(mu, dtype=dtype), np.asarray(var, dtype=dtype)
    w = mm.taps(windows, dtype)
    K = var.shape[1]
    ref, allow = np.zeros_like(var), np.zeros(var.shape)
    for k in range(K):
        p = np.ones((), dtype) / var[:, k]
        ref[:, k] = -p * p * _stencil(w[k], zl) * (mu[:, k] - _stencil(w[k], cl))
        sz, sc = _stencil(np.abs(w[k]), np.abs(zl)), _stencil(np.abs(w[k]), np.abs(cl))
        allow[:, k] = (p * p * sz * (np.abs(mu[:, k]) + sc)).astype(np.float64) * (2 * mm.APPLY_BOUND + 6 * U)
    return ref, allow
