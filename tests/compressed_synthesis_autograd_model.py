"""
float64 model of the compressed synthesis (type 1, per_phase_type='magphase', no post-filter) and of its backward pass
(DESIGN.md section 3.3k), for tests/test_compressed_synthesis_autograd_host.py and
tests/test_gpu_compressed_synthesis_autograd.py.  Needs neither a GPU nor the library.

forward_torch restates the forward (magphase.py:825-997) in plain torch float64 from the frame tables of one utterance,
so that torch's autograd gives the gradients; grads_closed is the closed form the HIP kernels implement, in numpy.
"""
import numpy as np
import torch
from scipy import signal

from magphase_amd import hostmath as hm


# ----------------------------------------------------------------------------------------------------------------------
# tables and constants
# ----------------------------------------------------------------------------------------------------------------------
def tables(v_lf0, fs, fft_len, b_const_rate=False, b_voi_ap_win=True):
    """The frame tables of one utterance: hostplan.plan_synthesis_numpy's arithmetic with the literal scipy scan."""
    N = int(fft_len)
    lf0 = np.atleast_1d(np.asarray(v_lf0, dtype=np.float64))
    n_rows = lf0.shape[0]
    v_f0 = np.exp(lf0)
    v_voi = v_f0 > 1.0
    v_shift = hm.f0_to_shift(v_f0, fs)
    if b_const_rate:
        v_shift, v_locs = hm._const_to_variable_scan_scipy(v_shift, 5.0, fs)
        lo, hi, t, v_voi = hm.const_to_variable_rows(v_voi, v_locs, 5.0, fs)
    else:
        lo = hi = np.arange(n_rows)
        t = np.zeros(n_rows)
    v_shift = v_shift.astype(int)
    v_pm = np.cumsum(v_shift)
    n = v_pm.size
    ns_len = int(v_pm[-1] + (v_pm[-1] - v_pm[-2]))
    _, lft, rgt = hm.frame_bounds(v_pm, ns_len)
    se = np.r_[v_shift[0], v_shift, v_shift[-1], v_shift[-1]]
    rel, start, out_len = hm.ola_plan(v_pm, N)
    return dict(n_rows=n_rows, n_frames=n, v_shift=v_shift, v_pm=v_pm, ns_len=ns_len, nleft=np.asarray(lft, dtype=int),
                nright=np.asarray(rgt, dtype=int), voiced=np.asarray(v_voi, dtype=bool),
                wtype=np.asarray(v_voi, dtype=bool) & bool(b_voi_ap_win), row0=np.asarray(lo, dtype=int),
                row1=np.asarray(hi, dtype=int), rowt=np.asarray(t, dtype=np.float64), win_l=se[:n] + se[1:n + 1],
                win_r=se[2:n + 2] + se[3:n + 3], rel=np.asarray(rel, dtype=int), start=int(start), out_len=int(out_len))


def constants(fs, fft_len, mag_dim, phase_dim, alpha_phase=None, b_fbank_mel=False):
    """The unwarp matrices and per-bin curves of the plan, float64."""
    N = int(fft_len)
    H = N // 2 + 1
    alpha = hm.define_alpha(fs)
    u_mag = (hm.unwarp_fbank_matrix if b_fbank_mel else hm.unwarp_matrix)(mag_dim, H, alpha)
    u_ph = hm.phase_unwarp_matrix(phase_dim, N, fs, alpha if alpha_phase is None else alpha_phase)
    per_v, ap_v, ap_u = (np.asarray(c, dtype=np.float64) for c in hm.synthesis_bin_curves(fs, N))
    return dict(fs=fs, N=N, H=H, u_mag=np.asarray(u_mag, dtype=np.float64), u_ph=np.asarray(u_ph, dtype=np.float64),
                per_v=per_v, ap_v=ap_v, ap_u=ap_u)


def _half_windows(left, right, wtype):
    """libaudio.py:70-84: rising half of win(1 + 2 left), falling half of win(1 + 2 right) without its first sample."""
    win = (lambda n_: np.bartlett(n_) ** 2.5) if wtype else np.hanning
    wl = win(1 + 2 * left)[:left + 1]
    wr = win(1 + 2 * right)[:right + 1][::-1]
    return np.concatenate((wl, wr[1:]))


def noise_spectra(v_noise, tab, fft_len):
    """Ns [F x H] complex (FFT of the windowed frames, epoch at index 0) and the per-frame 1 / gain (magphase.py:883-906)."""
    N = int(fft_len)
    H = N // 2 + 1
    v_noise = np.asarray(v_noise, dtype=np.float64)
    assert v_noise.size == tab["ns_len"]
    F = tab["n_frames"]
    m = np.zeros((F, N))
    pm_plus = np.hstack((0, tab["v_pm"], tab["ns_len"] - 1))
    for i in range(F):
        seg = v_noise[pm_plus[i]:pm_plus[i + 2] + 1] * _half_windows(int(tab["nleft"][i]), int(tab["nright"][i]),
                                                                     bool(tab["wtype"][i]))
        start = N // 2 - int(tab["v_shift"][i])
        m[i, start:start + seg.size] = seg
    ns = np.fft.fft(np.fft.fftshift(m, axes=1), axis=1)[:, :H]
    inv = np.ones(F)
    v = tab["voiced"]
    for cls in (v, ~v):
        if np.any(cls):
            a = np.abs(ns[cls][:, 1:-1])
            with np.errstate(divide="ignore"):
                lg = np.where(a == 0, -1.0e10, np.log(np.where(a == 0, 1.0, a)))
            inv[cls] = 1.0 / np.sqrt(np.exp(np.mean(lg ** 2)))
    return ns, inv


def anti_ringing_windows(tab, fft_len):
    """[F x N]: the centred asymmetric Hann of magphase.py:969-973, zero outside its support."""
    N = int(fft_len)
    w = np.zeros((tab["n_frames"], N))
    for i in range(tab["n_frames"]):
        wl, wr = int(tab["win_l"][i]), int(tab["win_r"][i])
        w[i, N // 2 - wl:N // 2 + wr + 1] = _half_windows(wl, wr, False)
    return w


def hpf_coefficients(fs):
    return signal.butter(4, 40 / (fs / 2.0), btype="highpass")


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


def _lerp_matrix(tab):
    W = np.zeros((tab["n_frames"], tab["n_rows"]))
    f = np.arange(tab["n_frames"])
    np.add.at(W, (f, tab["row0"]), 1.0 - tab["rowt"])
    np.add.at(W, (f, tab["row1"]), tab["rowt"])
    return W


def _curves(tab, cst):
    v = tab["voiced"][:, None]
    P = np.where(v, cst["per_v"][None, :], 0.0)
    A = np.where(v, cst["ap_v"][None, :], cst["ap_u"][None, :])
    return P, A


# ----------------------------------------------------------------------------------------------------------------------
# forward
# ----------------------------------------------------------------------------------------------------------------------
def spectrum_torch(a_mag, a_real, a_imag, tab, cst, ns, inv_gain):
    """(m, a, b, T, S): the frames' features and spectra [F x H], differentiable.  The two divisors that can be zero are
    replaced by 1 BEFORE the square root, so autograd sees no sqrt'(0)."""
    W = torch.from_numpy(_lerp_matrix(tab))
    u_mag, u_ph = torch.from_numpy(cst["u_mag"]), torch.from_numpy(cst["u_ph"])
    m = W @ torch.exp(a_mag @ u_mag)
    a, b = (W @ a_real) @ u_ph, (W @ a_imag) @ u_ph
    P, A = (torch.from_numpy(x) for x in _curves(tab, cst))
    s = a * a + b * b
    den = torch.sqrt(torch.where(s == 0, torch.ones_like(s), s))
    noise = torch.from_numpy(ns * inv_gain[:, None])
    T = torch.complex(P * a / den, P * b / den) + A * noise
    S = m * T
    n2 = S.real * S.real + S.imag * S.imag
    mod = torch.where(n2 == 0, torch.zeros_like(n2), torch.sqrt(torch.where(n2 == 0, torch.ones_like(n2), n2)))
    ends = torch.zeros(cst["H"], dtype=torch.bool)
    ends[0] = ends[-1] = True
    S = torch.complex(torch.where(ends, mod, S.real), torch.where(ends, torch.zeros_like(n2), S.imag))
    return m, a, b, T, S


def forward_torch(a_mag, a_real, a_imag, tab, cst, ns, inv_gain, b_out_hpf=True, return_pre=False):
    """One utterance: the coefficient rows (torch float64) -> the waveform [out_len] (differentiable)."""
    N = cst["N"]
    S = spectrum_torch(a_mag, a_real, a_imag, tab, cst, ns, inv_gain)[4]
    frm = torch.fft.fftshift(torch.fft.irfft(S, n=N, dim=1), dim=1) * torch.from_numpy(anti_ringing_windows(tab, N))
    out_len = tab["out_len"]
    y = torch.zeros(out_len, dtype=torch.float64)
    for i in range(frm.shape[0]):
        t0 = int(tab["rel"][i]) - tab["start"]
        lo, hi = max(0, -t0), min(N, out_len - t0)
        if hi > lo:
            y[t0 + lo:t0 + hi] = y[t0 + lo:t0 + hi] + frm[i, lo:hi]
    if return_pre:
        return y
    return _Hpf.apply(y, cst["fs"]) if b_out_hpf else y


def grads_autograd(a_mag, a_real, a_imag, gy, tab, cst, ns, inv_gain, b_out_hpf=True):
    t = [torch.tensor(np.asarray(x, dtype=np.float64), requires_grad=True) for x in (a_mag, a_real, a_imag)]
    y = forward_torch(t[0], t[1], t[2], tab, cst, ns, inv_gain, b_out_hpf)
    y.backward(torch.tensor(np.asarray(gy, dtype=np.float64)))
    return tuple(x.grad.numpy() if x.grad is not None else np.zeros(x.shape) for x in t)


# ----------------------------------------------------------------------------------------------------------------------
# the closed form
# ----------------------------------------------------------------------------------------------------------------------
def frame_windows(g, tab, fft_len):
    """[F x N]: the gradient samples under every frame (zero where the forward dropped the frame's samples)."""
    N = int(fft_len)
    out = np.zeros((tab["n_frames"], N))
    for i in range(tab["n_frames"]):
        t0 = int(tab["rel"][i]) - tab["start"]
        lo, hi = max(0, -t0), min(N, tab["out_len"] - t0)
        if hi > lo:
            out[i, lo:hi] = g[t0 + lo:t0 + hi]
    return out


def frame_grads_closed(m, a, b, P, A_ig_ns, gwin, fft_len):
    """What k_synth_comp_bwd computes: m, a, b, P [F x H] the frames' features and periodic curve (0 where there is no
    periodic component), A_ig_ns = A ig Ns [F x H] complex, gwin [F x N] the windowed gradient samples -> (grad m, grad a,
    grad b) [F x H]."""
    N = int(fft_len)
    H = N // 2 + 1
    G = np.fft.fft(np.fft.ifftshift(gwin, axes=1), axis=1)[:, :H]
    c = np.full(H, 2.0)
    c[0] = c[-1] = 1.0
    gS = G * (c / N)
    absp = np.sqrt(a * a + b * b)
    den = np.where(absp == 0, 1.0, absp)
    u = (a + 1j * b) / den
    T = P * u + A_ig_ns
    S = m * T
    for k in (0, H - 1):
        mod = np.abs(S[:, k])
        dirn = np.where(mod == 0, 0.0, S[:, k] / np.where(mod == 0, 1.0, mod))
        gS[:, k] = gS[:, k].real * dirn
    gm = (np.conj(T) * gS).real
    d = (np.conj(u) * gS).real
    gp = (m * P / den) * (gS - u * d)
    return gm, gp.real, gp.imag


def grads_closed(a_mag, a_real, a_imag, gy, tab, cst, ns, inv_gain, b_out_hpf=True):
    """The closed form of the whole backward pass, numpy float64."""
    a_mag, a_real, a_imag = (np.asarray(x, dtype=np.float64) for x in (a_mag, a_real, a_imag))
    N = cst["N"]
    g = np.asarray(gy, dtype=np.float64)
    if b_out_hpf:
        g = hpf_adjoint(g, cst["fs"])
    W = _lerp_matrix(tab)
    E = np.exp(a_mag @ cst["u_mag"])
    m = W @ E
    a, b = (W @ a_real) @ cst["u_ph"], (W @ a_imag) @ cst["u_ph"]
    P, A = _curves(tab, cst)
    gwin = frame_windows(g, tab, N) * anti_ringing_windows(tab, N)
    gm, ga, gb = frame_grads_closed(m, a, b, P, A * ns * inv_gain[:, None], gwin, N)
    gE = W.T @ gm
    return (E * gE) @ cst["u_mag"].T, W.T @ (ga @ cst["u_ph"].T), W.T @ (gb @ cst["u_ph"].T)


def rel_err(got, ref):
    """max |got - ref| / max |ref| over a whole matrix (no element left out); the plain max |got - ref| where the
    reference is all zero."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape
    if ref.size == 0:
        return 0.0
    scale = np.max(np.abs(ref))
    return float(np.max(np.abs(got - ref)) / (scale if scale > 0 else 1.0))


# ----------------------------------------------------------------------------------------------------------------------
# test material
# ----------------------------------------------------------------------------------------------------------------------
def lf0_track(rng, n_rows, kind, fs):
    """n_rows of log f0 on the 5 ms grid: 'voiced', 'unvoiced' (f0 = 0: lf0 = -1e10) or 'mixed' (stretches of both)."""
    f0 = rng.uniform(110.0, 260.0) * np.exp(0.1 * np.cumsum(rng.randn(n_rows)) / np.sqrt(n_rows))
    if kind == "unvoiced":
        voi = np.zeros(n_rows, dtype=bool)
    elif kind == "voiced":
        voi = np.ones(n_rows, dtype=bool)
    else:
        voi = (np.arange(n_rows) // max(n_rows // 5, 1)) % 2 == 0
    return np.where(voi, np.log(f0), -1.0e10)


def features(rng, n_rows, mag_dim, phase_dim):
    """Plausible coefficient rows: a smooth log-mel magnitude of moderate level, phase coefficients in [-1, 1]."""
    a_mag = -3.0 + 0.8 * rng.randn(n_rows, mag_dim) * np.linspace(1.0, 0.3, mag_dim)[None, :]
    a_real = np.clip(0.5 * rng.randn(n_rows, phase_dim), -1.0, 1.0)
    a_imag = np.clip(0.5 * rng.randn(n_rows, phase_dim), -1.0, 1.0)
    return a_mag, a_real, a_imag
