"""
float64 model of the minimum-phase stage (la.build_min_phase_from_mag_spec, k_min_phase), of its adjoint (k_min_phase_bwd,
DESIGN.md section 3.3o) and of the magnitude-only synthesis built on them, for tests/test_min_phase_autograd_host.py and
tests/test_gpu_min_phase_autograd.py.  Needs neither a GPU nor the library.

N = fft_len, M = N / 2, H = M + 1.  phi = T L with L = ln m:
  c[n]   = (1/N) [L[0] + (-1)^n L[M] + 2 sum_{k=1..M-1} L[k] cos(2 pi k n / N)]
  phi[k] = -2 sum_{n=1..M-1} c[n] sin(2 pi k n / N),  phi[0] = phi[M] = 0
"""
import numpy as np
import torch

import compressed_synthesis_autograd_model as cs_model

MAGIC = -1.0e10    # the protected logarithm's value where m <= 0 (libaudio.py:241-248)


def fold_weights(N):
    M = N // 2
    w = np.zeros(N)
    w[0] = w[M] = 1.0
    w[1:M] = 2.0
    return w


def protected_log(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m > 0, np.log(np.where(m > 0, m, 1.0)), MAGIC)


def T_apply(L):
    """phi = T L, rows of [.. x H] float64, by np.fft (the reference's own route: irfft, causal fold, fft)."""
    L = np.asarray(L, dtype=np.float64)
    N = 2 * (L.shape[-1] - 1)
    c = np.fft.irfft(L, n=N, axis=-1)
    phi = np.fft.rfft(c * fold_weights(N), axis=-1).imag
    phi[..., 0] = phi[..., -1] = 0.0
    return phi


def Tt_apply(g_phi):
    """g_L = T^t g_phi, rows of [.. x H] float64, as the issue states it:
    s[n] = sum_{k=1..M-1} g_phi[k] sin(2 pi k n / N); g_c = -w s; g_L[k] = (e[k] / N) sum_n g_c[n] cos(2 pi k n / N)."""
    g = np.array(g_phi, dtype=np.float64)
    N = 2 * (g.shape[-1] - 1)
    g[..., 0] = g[..., -1] = 0.0
    # irfft of the Hermitian spectrum i g: x[n] = -(2 / N) s[n]
    s = -0.5 * N * np.fft.irfft(1j * g, n=N, axis=-1)
    g_c = -fold_weights(N) * s
    e = np.full(g.shape[-1], 2.0)
    e[0] = e[-1] = 1.0
    return np.fft.rfft(g_c, axis=-1).real * (e / N)


def T_dense(N):
    """T as a dense [H x H] matrix from the defining sums (no FFT)."""
    M, H = N // 2, N // 2 + 1
    n = np.arange(N)
    k = np.arange(H)
    C = np.cos(2 * np.pi * np.outer(n, k) / N)          # [N x H]
    e = np.full(H, 2.0)
    e[0] = e[-1] = 1.0
    c_of_L = C * (e / N)[None, :]                        # c = c_of_L @ L
    S = np.sin(2 * np.pi * np.outer(k, n[1:M]) / N)      # [H x (M - 1)]
    T = -2.0 * S @ c_of_L[1:M]
    T[0] = T[-1] = 0.0
    return T


def min_phase_rows(m):
    """(m, cos phi, sin phi) of magnitude rows [F x H], float64: what k_min_phase writes."""
    phi = T_apply(protected_log(m))
    return np.asarray(m, dtype=np.float64), np.cos(phi), np.sin(phi)


def backward_rows(m, c, s, g_m, g_a, g_b, n_phase=None):
    """What k_min_phase_bwd computes from the forward's rows (m, c = cos phi, s = sin phi) and the gradients with respect
    to them (None: zero); columns of g_a / g_b from n_phase on count as zero."""
    m, c, s = (np.asarray(x, dtype=np.float64) for x in (m, c, s))
    H = m.shape[-1]
    n_phase = H if n_phase is None else int(n_phase)
    z = np.zeros_like(m)
    ga = z if g_a is None else np.asarray(g_a, dtype=np.float64)
    gb = z if g_b is None else np.asarray(g_b, dtype=np.float64)
    g_phi = np.zeros_like(m)
    g_phi[..., :n_phase] = gb[..., :n_phase] * c[..., :n_phase] - ga[..., :n_phase] * s[..., :n_phase]
    g_L = Tt_apply(g_phi)
    out = (z if g_m is None else np.asarray(g_m, dtype=np.float64)).copy()
    pos = m > 0
    out[pos] += g_L[pos] / m[pos]
    return out


def chain_loss(m, w_m, w_a, w_b):
    """A scalar loss of the forward's three rows: sum(w_m m + w_a cos phi + w_b sin phi)."""
    mm, c, s = min_phase_rows(m)
    return float(np.sum(w_m * mm + w_a * c + w_b * s))


def T_torch(L):
    """phi = T L in torch float64 (differentiable): the FFT restatement."""
    N = 2 * (L.shape[-1] - 1)
    c = torch.fft.irfft(L.to(torch.complex128), n=N, dim=-1)
    S = torch.fft.rfft(c * torch.from_numpy(fold_weights(N)), dim=-1)
    keep = torch.ones(L.shape[-1], dtype=torch.float64)
    keep[0] = keep[-1] = 0.0
    return S.imag * keep


def rel_err_rows(got, ref):
    """max over rows of max |got - ref| / max |ref| of the row; no row or bin left out."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape
    scale = np.max(np.abs(ref), axis=-1, keepdims=True)
    scale = np.where(scale > 0, scale, 1.0)
    return float(np.max(np.abs(got - ref) / scale)) if ref.size else 0.0


# ----------------------------------------------------------------------------------------------------------------------
# the magnitude-only synthesis: tests/compressed_synthesis_autograd_model.py with the min-phase stage put in front
# ----------------------------------------------------------------------------------------------------------------------
def forward_torch(a_mag, tab, cst, ns, inv_gain, phase="min_phase", b_out_hpf=True):
    """One utterance: the magnitude rows (torch float64) -> the waveform [out_len] (differentiable).  The phase of the
    periodic component is the minimum phase of the frame's magnitude ('min_phase') or zero ('zero')."""
    N, H = cst["N"], cst["H"]
    W = torch.from_numpy(cs_model._lerp_matrix(tab))
    m = W @ torch.exp(a_mag @ torch.from_numpy(cst["u_mag"]))
    P, A = (torch.from_numpy(x) for x in cs_model._curves(tab, cst))
    if phase == "min_phase":
        phi = T_torch(torch.log(m))
        u = torch.complex(torch.cos(phi), torch.sin(phi))
    else:
        u = torch.complex(torch.ones_like(m), torch.zeros_like(m))
    T = P * u + A * torch.from_numpy(ns * inv_gain[:, None])
    S = m * T
    n2 = S.real * S.real + S.imag * S.imag
    mod = torch.where(n2 == 0, torch.zeros_like(n2), torch.sqrt(torch.where(n2 == 0, torch.ones_like(n2), n2)))
    ends = torch.zeros(H, dtype=torch.bool)
    ends[0] = ends[-1] = True
    S = torch.complex(torch.where(ends, mod, S.real), torch.where(ends, torch.zeros_like(n2), S.imag))
    frm = torch.fft.fftshift(torch.fft.irfft(S, n=N, dim=1), dim=1) * torch.from_numpy(cs_model.anti_ringing_windows(tab, N))
    out_len = tab["out_len"]
    y = torch.zeros(out_len, dtype=torch.float64)
    for i in range(frm.shape[0]):
        t0 = int(tab["rel"][i]) - tab["start"]
        lo, hi = max(0, -t0), min(N, out_len - t0)
        if hi > lo:
            y[t0 + lo:t0 + hi] = y[t0 + lo:t0 + hi] + frm[i, lo:hi]
    return cs_model._Hpf.apply(y, cst["fs"]) if b_out_hpf else y


def grads_autograd(a_mag, gy, tab, cst, ns, inv_gain, phase="min_phase", b_out_hpf=True):
    t = torch.tensor(np.asarray(a_mag, dtype=np.float64), requires_grad=True)
    y = forward_torch(t, tab, cst, ns, inv_gain, phase, b_out_hpf)
    y.backward(torch.tensor(np.asarray(gy, dtype=np.float64)))
    return t.grad.numpy()
