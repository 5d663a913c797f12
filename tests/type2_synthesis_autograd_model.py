"""
float64 model of the type-2 synthesis from compressed features (Type2SynthesisPlan.run() and the elliptic output filter)
and of its backward pass, for tests/test_type2_synthesis_autograd_host.py and
tests/test_gpu_type2_synthesis_autograd.py.  Needs neither a GPU nor the library.

forward_torch restates the forward (magphase.py:1452-1606) in plain torch float64 from the frame tables of one utterance,
so that torch's autograd gives the gradients; grads_closed is the closed form the HIP kernels implement, in numpy.  The
frame tables are type2_synthesis_model's (the oracle's arithmetic); the pieces type 2 shares with type 1 -- the row
interpolation, the noise frames' spectra, the anti-ringing windows, the overlap-add's frame placement -- are
compressed_synthesis_autograd_model's.  What is type 2's own is spelled out here: the phase unwarp matrix, the plain
crossfade curves and the hf_slope line, one rms gain per utterance (held constant: it does not depend on the features),
signed real DC / Nyquist bins, the elliptic high-pass.
"""
import numpy as np
import torch
from scipy import signal

import compressed_synthesis_autograd_model as base
import type2_synthesis_model as t2
from magphase_amd import hostmath as hm

rel_err, lf0_track, features = base.rel_err, base.lf0_track, base.features


# ----------------------------------------------------------------------------------------------------------------------
# tables and constants
# ----------------------------------------------------------------------------------------------------------------------
def tables(v_lf0, fs, fft_len, const_rate_ms=-1.0, b_voi_ap_win=True):
    """The frame tables of one utterance, in compressed_synthesis_autograd_model.tables' layout."""
    N = int(fft_len)
    lf0 = np.atleast_1d(np.asarray(v_lf0, dtype=np.float64))
    n_rows = lf0.shape[0]
    v_shift, v_pm, v_voi, v_locs, ns_len = t2.frame_tables(lf0, fs, const_rate_ms)
    if v_locs is not None:
        lo, hi, t, _ = hm.const_to_variable_rows(np.exp(lf0) > 0.0, v_locs, const_rate_ms, fs)
    else:
        lo = hi = np.arange(n_rows)
        t = np.zeros(n_rows)
    n = v_pm.size
    _, lft, rgt = hm.frame_bounds(v_pm, ns_len)
    se = np.r_[v_shift[0], v_shift, v_shift[-1], v_shift[-1]]
    rel, start, out_len = hm.ola_plan(v_pm, N)
    return dict(n_rows=n_rows, n_frames=n, v_shift=v_shift, v_pm=v_pm, ns_len=ns_len, nleft=np.asarray(lft, dtype=int),
                nright=np.asarray(rgt, dtype=int), voiced=np.asarray(v_voi, dtype=bool),
                wtype=np.asarray(v_voi, dtype=bool) & bool(b_voi_ap_win), row0=np.asarray(lo, dtype=int),
                row1=np.asarray(hi, dtype=int), rowt=np.asarray(t, dtype=np.float64), win_l=se[:n] + se[1:n + 1],
                win_r=se[2:n + 2] + se[3:n + 3], rel=np.asarray(rel, dtype=int), start=int(start), out_len=int(out_len))


def constants(fs, fft_len, mag_dim, phase_dim, hf_slope_coeff=1.0):
    """The unwarp matrices and per-bin curves of the plan, float64."""
    N = int(fft_len)
    H = N // 2 + 1
    alpha = hm.define_alpha(fs)
    per_v, ap_v, ap_u = (np.asarray(c, dtype=np.float64) for c in hm.type2_synthesis_bin_curves(fs, N, hf_slope_coeff))
    return dict(fs=fs, N=N, H=H, u_mag=np.asarray(hm.unwarp_matrix(mag_dim, H, alpha), dtype=np.float64),
                u_ph=np.asarray(hm.type2_phase_unwarp_matrix(phase_dim, mag_dim, H, alpha), dtype=np.float64),
                per_v=per_v, ap_v=ap_v, ap_u=ap_u)


def noise_spectra(v_noise, tab, fft_len):
    """Ns [F x H] complex and the per-frame 1 / rms_noise: one gain per utterance, the rms of |Ns| over all frames and
    bins (magphase.py:1538-1541)."""
    ns = base.noise_spectra(v_noise, tab, fft_len)[0]
    rms = float(np.sqrt(np.mean(np.abs(ns) ** 2)))
    return ns, np.full(tab["n_frames"], 1.0 / rms)


def hpf_coefficients(fs):
    return signal.ellip(4, 0.5, 80, 60 / (fs / 2.0), btype="highpass")     # magphase.py:1599-1604


def hpf(x, fs):
    b, a = hpf_coefficients(fs)
    return signal.lfilter(b, a, np.asarray(x, dtype=np.float64))


def hpf_adjoint(g, fs):
    """The adjoint of a causal LTI filter from a zero state: the same filter run backwards in time."""
    return hpf(np.asarray(g, dtype=np.float64)[::-1], fs)[::-1].copy()


class _Hpf(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, fs):
        ctx.fs = fs
        return torch.from_numpy(hpf(y.detach().numpy(), fs))

    @staticmethod
    def backward(ctx, g):
        return torch.from_numpy(hpf_adjoint(g.numpy(), ctx.fs)), None


# ----------------------------------------------------------------------------------------------------------------------
# forward
# ----------------------------------------------------------------------------------------------------------------------
def spectrum_torch(a_mag, a_real, a_imag, tab, cst, ns, inv_gain):
    """(m, a, b, T, S): the frames' features and spectra [F x H], differentiable.  The divisor that can be zero is replaced
    by 1 BEFORE the square root (magphase.py:1560-1563), so autograd sees no sqrt'(0).  Bins 0 and N/2 keep Re S."""
    W = torch.from_numpy(base._lerp_matrix(tab))
    u_mag, u_ph = torch.from_numpy(cst["u_mag"]), torch.from_numpy(cst["u_ph"])
    m = W @ torch.exp(a_mag @ u_mag)
    a, b = (W @ a_real) @ u_ph, (W @ a_imag) @ u_ph
    P, A = (torch.from_numpy(x) for x in base._curves(tab, cst))
    s = a * a + b * b
    den = torch.sqrt(torch.where(s == 0, torch.ones_like(s), s))
    noise = torch.from_numpy(ns * inv_gain[:, None])
    T = torch.complex(P * a / den, P * b / den) + A * noise
    S = m * T
    ends = torch.zeros(cst["H"], dtype=torch.bool)
    ends[0] = ends[-1] = True
    S = torch.complex(S.real, torch.where(ends, torch.zeros_like(S.imag), S.imag))
    return m, a, b, T, S


def forward_torch(a_mag, a_real, a_imag, tab, cst, ns, inv_gain, return_pre=False):
    """One utterance: the coefficient rows (torch float64) -> the waveform [out_len] (differentiable)."""
    N = cst["N"]
    S = spectrum_torch(a_mag, a_real, a_imag, tab, cst, ns, inv_gain)[4]
    frm = torch.fft.fftshift(torch.fft.irfft(S, n=N, dim=1), dim=1) * torch.from_numpy(base.anti_ringing_windows(tab, N))
    out_len = tab["out_len"]
    y = torch.zeros(out_len, dtype=torch.float64)
    for i in range(frm.shape[0]):
        t0 = int(tab["rel"][i]) - tab["start"]
        lo, hi = max(0, -t0), min(N, out_len - t0)
        if hi > lo:
            y[t0 + lo:t0 + hi] = y[t0 + lo:t0 + hi] + frm[i, lo:hi]
    return y if return_pre else _Hpf.apply(y, cst["fs"])


def grads_autograd(a_mag, a_real, a_imag, gy, tab, cst, ns, inv_gain):
    t = [torch.tensor(np.asarray(x, dtype=np.float64), requires_grad=True) for x in (a_mag, a_real, a_imag)]
    y = forward_torch(t[0], t[1], t[2], tab, cst, ns, inv_gain)
    y.backward(torch.tensor(np.asarray(gy, dtype=np.float64)))
    return tuple(x.grad.numpy() if x.grad is not None else np.zeros(x.shape) for x in t)


# ----------------------------------------------------------------------------------------------------------------------
# the closed form
# ----------------------------------------------------------------------------------------------------------------------
def frame_grads_closed(m, a, b, P, A_ig_ns, gwin, fft_len):
    """What k_synth_comp_bwd<P, T2 = true> computes: compressed_synthesis_autograd_model.frame_grads_closed with the
    type-2 ends -- S_0 <- Re S_0, S_{N/2} <- Re S_{N/2} is linear, so the real end-bin gradient passes straight through,
    gS_end = (Re gS, 0), with no projection on S / |S|."""
    N = int(fft_len)
    H = N // 2 + 1
    G = np.fft.fft(np.fft.ifftshift(gwin, axes=1), axis=1)[:, :H]
    c = np.full(H, 2.0)
    c[0] = c[-1] = 1.0
    gS = G * (c / N)
    for k in (0, H - 1):
        gS[:, k] = gS[:, k].real
    absp = np.sqrt(a * a + b * b)
    den = np.where(absp == 0, 1.0, absp)
    u = (a + 1j * b) / den
    T = P * u + A_ig_ns
    gm = (np.conj(T) * gS).real
    d = (np.conj(u) * gS).real
    gp = (m * P / den) * (gS - u * d)
    return gm, gp.real, gp.imag


def grads_closed(a_mag, a_real, a_imag, gy, tab, cst, ns, inv_gain):
    """The closed form of the whole backward pass, numpy float64."""
    a_mag, a_real, a_imag = (np.asarray(x, dtype=np.float64) for x in (a_mag, a_real, a_imag))
    N = cst["N"]
    g = hpf_adjoint(np.asarray(gy, dtype=np.float64), cst["fs"])
    W = base._lerp_matrix(tab)
    E = np.exp(a_mag @ cst["u_mag"])
    m = W @ E
    a, b = (W @ a_real) @ cst["u_ph"], (W @ a_imag) @ cst["u_ph"]
    P, A = base._curves(tab, cst)
    gwin = base.frame_windows(g, tab, N) * base.anti_ringing_windows(tab, N)
    gm, ga, gb = frame_grads_closed(m, a, b, P, A * ns * inv_gain[:, None], gwin, N)
    gE = W.T @ gm
    return (E * gE) @ cst["u_mag"].T, W.T @ (ga @ cst["u_ph"].T), W.T @ (gb @ cst["u_ph"].T)
