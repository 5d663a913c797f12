"""
float64 model of the lossless synthesis and of its backward pass, for
tests/test_lossless_autograd_host.py and tests/test_gpu_lossless_autograd.py.  Needs neither a GPU nor the library.

forward_torch is the reference's forward (magphase.py:1759-1776, libaudio.py:369-388, ola :34-62) restated in plain torch
float64, so that torch's autograd gives the gradients; grads_closed is the closed form the HIP kernel implements, in numpy.
"""
import numpy as np
import torch

from magphase_amd import hostmath as hm


def v_pm_of(v_f0, fs):
    """Pitch marks of synthesis_from_lossless (magphase.py:1771-1772): float cumsum, then truncation."""
    return np.cumsum(hm.f0_to_shift(np.asarray(v_f0, dtype=np.float64), fs)).astype(int)


def forward_torch(mag, real, imag, v_pm, fft_len):
    """One utterance: mag / real / imag torch float64 [F x H] -> y [out_len] (differentiable).
    The divisor |p| is replaced by 1 where p == 0 BEFORE the square root, so autograd sees no sqrt'(0)."""
    N = int(fft_len)
    H = N // 2 + 1
    s = real * real + imag * imag
    den = torch.sqrt(torch.where(s == 0, torch.ones_like(s), s))
    keep = torch.ones(H, dtype=mag.dtype)
    keep[0] = keep[-1] = 0.0                      # Im X dropped at bins 0 and N/2
    X = torch.complex(mag * real / den, mag * imag / den * keep)
    frm = torch.fft.fftshift(torch.fft.irfft(X, n=N, dim=1), dim=1)
    rel, start, out_len = hm.ola_plan(v_pm, N)
    y = torch.zeros(out_len, dtype=mag.dtype)
    for i in range(frm.shape[0]):
        t0 = int(rel[i]) - start                  # output index of sample 0 of frame i
        lo, hi = max(0, -t0), min(N, out_len - t0)
        if hi > lo:
            y[t0 + lo:t0 + hi] = y[t0 + lo:t0 + hi] + frm[i, lo:hi]
    return y


def grads_autograd(mag, real, imag, gy, v_pm, fft_len):
    """(d mag, d real, d imag) float64 numpy of sum(gy * forward) by torch autograd."""
    t = [torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=True) for a in (mag, real, imag)]
    y = forward_torch(t[0], t[1], t[2], v_pm, fft_len)
    if not y.requires_grad:      # no frame reaches the kept output (ola_plan's negative-start case): y is constant
        return tuple(np.zeros(x.shape) for x in t)
    y.backward(torch.tensor(np.asarray(gy, dtype=np.float64)))
    return tuple(x.grad.numpy() for x in t)


def grads_closed(mag, real, imag, gy, v_pm, fft_len):
    """The closed form, numpy float64: per frame gather -> ifftshift -> FFT -> (c_k / N) -> pointwise epilogue."""
    N = int(fft_len)
    H = N // 2 + 1
    mag, real, imag = (np.asarray(a, dtype=np.float64) for a in (mag, real, imag))
    gy = np.asarray(gy, dtype=np.float64)
    rel, start, out_len = hm.ola_plan(v_pm, N)
    F = mag.shape[0]
    g = np.zeros((F, N))
    for i in range(F):
        t0 = int(rel[i]) - start
        lo, hi = max(0, -t0), min(N, out_len - t0)
        if hi > lo:
            g[i, lo:hi] = gy[t0 + lo:t0 + hi]
    G = np.fft.fft(np.fft.ifftshift(g, axes=1), axis=1)[:, :H]
    c = np.full(H, 2.0)
    c[0] = c[-1] = 1.0
    gX = G * (c / N)
    gX[:, 0] = gX[:, 0].real
    gX[:, -1] = gX[:, -1].real
    return epilogue(mag, real, imag, gX)


def epilogue(mag, real, imag, gX):
    """d = Re(conj(u) gX); d mag = d, d p = (mag / den)(gX - u d); den = |p|, 1 where p == 0."""
    absp = np.sqrt(real * real + imag * imag)
    den = np.where(absp == 0, 1.0, absp)
    ur, ui = real / den, imag / den
    d = ur * gX.real + ui * gX.imag
    return d, mag / den * (gX.real - ur * d), mag / den * (gX.imag - ui * d)


def lerp_matrix(row0, row1, rowt, n_rows):
    """Dense [frames x n_rows] matrix of out[f] = (1 - t_f) rows[row0_f] + t_f rows[row1_f]."""
    row0, row1 = np.asarray(row0, dtype=np.int64), np.asarray(row1, dtype=np.int64)
    rowt = np.asarray(rowt, dtype=np.float64)
    W = np.zeros((row0.size, int(n_rows)))
    f = np.arange(row0.size)
    np.add.at(W, (f, row0), 1.0 - rowt)
    np.add.at(W, (f, row1), rowt)
    return W


def lerp_adjoint_by_table(table, rowt, gv):
    """What k_rows_lerp_adjoint computes from hostmath.lerp_adjoint_table's ranges: per row the union of the two frame
    ranges in ascending order, weight 1 - t / t / exactly 1 for a frame in both."""
    rowt = np.asarray(rowt, dtype=np.float64)
    out = np.zeros((table.shape[0], gv.shape[1]))
    for r, (a0, a1, b0, b1) in enumerate(np.asarray(table).tolist()):
        for f in sorted(set(range(a0, a1)) | set(range(b0, b1))):
            in_a, in_b = a0 <= f < a1, b0 <= f < b1
            w = 1.0 if (in_a and in_b) else ((1.0 - rowt[f]) if in_a else rowt[f])
            out[r] += w * gv[f]
    return out


def const_rate_grads(rows, gy_list, plan_rows, v_pm_list, frame_off, fft_len):
    """Gradients with respect to the constant-rate rows of a batch: rows = (mag, real, imag) float64 [R x H] (the batch's
    rows, concatenated), plan_rows = (row0, row1, rowt) the plan's host tables (global row indices), utterance k's frames
    are frame_off[k] .. frame_off[k + 1] with pitch marks v_pm_list[k] and upstream gradient gy_list[k]."""
    W = torch.tensor(lerp_matrix(plan_rows[0], plan_rows[1], plan_rows[2], rows[0].shape[0]))
    t = [torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=True) for a in rows]
    var = [W @ x for x in t]
    loss = 0.0
    for k, v_pm in enumerate(v_pm_list):
        a, b = int(frame_off[k]), int(frame_off[k + 1])
        y = forward_torch(var[0][a:b], var[1][a:b], var[2][a:b], v_pm, fft_len)
        loss = loss + (y * torch.tensor(np.asarray(gy_list[k], dtype=np.float64))).sum()
    if not (torch.is_tensor(loss) and loss.requires_grad):
        return tuple(np.zeros(x.shape) for x in t)
    loss.backward()
    return tuple(x.grad.numpy() for x in t)


def rel_err(got, ref):
    """max |got - ref| / max |ref| over a whole matrix (no element left out); the plain max |got - ref| where the
    reference is all zero."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape
    if ref.size == 0:
        return 0.0
    scale = np.max(np.abs(ref))
    return float(np.max(np.abs(got - ref)) / (scale if scale > 0 else 1.0))
