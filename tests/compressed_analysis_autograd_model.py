"""
float64 model of the compressed analysis and of its backward pass, for
tests/test_compressed_analysis_autograd_host.py and tests/test_gpu_compressed_analysis_autograd.py.  Needs neither a GPU
nor the library.

forward_torch is lossless_analysis_autograd_model.forward_torch followed by the two mel warps as magphase_warp.hip
computes them (hostmath.warp_matrix in float64, the constant-rate tables of hostmath.var_to_const_rate_batch, the phase
product formed per variable-rate row and interpolated afterwards, voicing mask and clip), so that torch's autograd gives
the gradients; grads_closed is the closed form the HIP kernels implement, in numpy, from given lossless rows.
"""
import numpy as np
import torch

import lossless_analysis_autograd_model as lossless
from magphase_amd import hostmath as hm

FS = lossless.FS
EPS = 1.0e-8        # the floor of mcep -e
TIE = 1.0e-3        # |pre-clip value| within this of 1: the float32 forward may land on the other side of the clip

rel_err = lossless.rel_err
tone_and_noise = lossless.tone_and_noise


def warps(fft_len, fs=FS, mag_dim=60, phase_dim=45, alpha_phase=None):
    """(Wm [mag_dim x H], Wp [phase_dim x H]) float64, as CompressedAnalysisPlan builds them."""
    H = int(fft_len) // 2 + 1
    alpha = hm.define_alpha(fs)
    a_ph = alpha if alpha_phase is None else alpha_phase
    cf, _ = hm.define_crossfade_params(fs)
    k_full = hm.get_num_full_mel_coeffs_from_num_phase_coeffs(cf, phase_dim, a_ph, fs)
    return (np.array(hm.warp_matrix(mag_dim, H, alpha), dtype=np.float64),
            np.array(hm.warp_matrix(k_full, H, a_ph, nrows=phase_dim), dtype=np.float64))


def tables(v_pm_sec, v_voi, n_smpls, b_const_rate, fs=FS):
    """The tables of one utterance: frames (pm, left, right), the rows an output frame interpolates from (row0, row1,
    rowt; identity at the variable rate) and the voicing of the output frames."""
    pm, left, right, voi = lossless.frames_of(v_pm_sec, v_voi, n_smpls, fs)
    f0 = hm.shift_to_f0(left, voi, fs)
    if b_const_rate:
        row0, row1, rowt, f0_out, _off = hm.var_to_const_rate_batch([left], [f0], [0], fs, 5.0)
        f0 = f0_out[0]
    else:
        row0 = row1 = np.arange(pm.size, dtype=np.int64)
        rowt = np.zeros(pm.size)
    return {"pm": pm, "left": left, "right": right, "row0": np.asarray(row0), "row1": np.asarray(row1),
            "rowt": np.asarray(rowt, dtype=np.float64), "voi": np.asarray(f0) > 0}


def _lerp_t(x, tab):
    t = torch.from_numpy(tab["rowt"])[:, None]
    return (1.0 - t) * x[torch.from_numpy(tab["row0"])] + t * x[torch.from_numpy(tab["row1"])]


def warp_torch(mag, real, imag, tab, wm, wp):
    """The two warps on lossless rows (torch float64, differentiable) -> (M, R, I, pre-clip R, pre-clip I)."""
    wm_t, wp_t = torch.from_numpy(wm), torch.from_numpy(wp)
    magc = _lerp_t(mag, tab)
    m = torch.log(magc * magc + EPS) @ wm_t.T
    voi = torch.from_numpy(tab["voi"])[:, None]
    outs, pres = [], []
    for x in (real, imag):
        pre = _lerp_t((2.0 * x + EPS * torch.exp(-2.0 * x)) @ wp_t.T, tab)
        pres.append(pre)
        outs.append(torch.where(voi, torch.clamp(pre, -1.0, 1.0), torch.zeros_like(pre)))
    return m, outs[0], outs[1], pres[0], pres[1]


def forward_torch(sig, tab, fft_len, wm, wp):
    mag, real, imag = lossless.forward_torch(sig, tab["pm"], tab["left"], tab["right"], fft_len)
    return warp_torch(mag, real, imag, tab, wm, wp)


def forward_numpy(sig, tab, fft_len, wm, wp):
    with torch.no_grad():
        return tuple(t.numpy() for t in forward_torch(torch.as_tensor(np.asarray(sig, dtype=np.float64)), tab, fft_len,
                                                      wm, wp))


def tie_mask(pre_r, pre_i, tab):
    """(bool [F x phase_dim]) x 2: voiced elements whose float64 pre-clip magnitude lies within TIE of 1 -- the upstream
    test gradient is set to zero there, for the device and the model alike."""
    voi = tab["voi"][:, None]
    return tuple(voi & (np.abs(np.abs(np.asarray(p)) - 1.0) < TIE) for p in (pre_r, pre_i))


def grads_autograd(sig, grads, tab, fft_len, wm, wp):
    """d sig float64 numpy of sum_k sum(grads[k] * forward[k]) by torch autograd; grads[k] None: output k not used."""
    x = torch.tensor(np.asarray(sig, dtype=np.float64), requires_grad=True)
    out = forward_torch(x, tab, fft_len, wm, wp)[:3]
    loss = sum((o * torch.as_tensor(np.asarray(g, dtype=np.float64))).sum() for o, g in zip(out, grads) if g is not None)
    if not (torch.is_tensor(loss) and loss.requires_grad):
        return np.zeros(x.shape)
    loss.backward()
    return x.grad.numpy()


def lerp_adjoint(g, tab, n_rows):
    """The adjoint of out[f] = (1 - t_f) x[row0_f] + t_f x[row1_f] applied to g [F x W] -> [n_rows x W]."""
    g = np.asarray(g, dtype=np.float64)
    out = np.zeros((int(n_rows), g.shape[1]))
    t = tab["rowt"][:, None]
    np.add.at(out, tab["row0"], (1.0 - t) * g)
    np.add.at(out, tab["row1"], t * g)
    return out


def lerp_adjoint_by_table(g, ranges, rowt):
    """What k_rows_lerp_adjoint computes from hostmath.lerp_adjoint_table's ranges, at any width."""
    g = np.asarray(g, dtype=np.float64)
    out = np.zeros((ranges.shape[0], g.shape[1]))
    for r, (a0, a1, b0, b1) in enumerate(np.asarray(ranges).tolist()):
        for f in sorted(set(range(a0, a1)) | set(range(b0, b1))):
            in_a, in_b = a0 <= f < a1, b0 <= f < b1
            out[r] += (1.0 if in_a and in_b else (1.0 - rowt[f] if in_a else rowt[f])) * g[f]
    return out


def warp_grads_closed(mag, real, imag, out_r, out_i, grads, tab, wm, wp):
    """Section 2 of the design in numpy float64: the gradients with respect to the lossless rows (g_mag, g_real, g_imag;
    None where nothing arrives) from the rows, the forward's phase OUTPUTS (the mask is read from them) and the upstream
    gradients (gM, gR, gI), any of them None."""
    mag, real, imag = (np.asarray(a, dtype=np.float64) for a in (mag, real, imag))
    n_rows = mag.shape[0]
    t = tab["rowt"][:, None]
    g_m, g_r, g_i = grads
    res = [None, None, None]
    if g_m is not None:
        magc = (1.0 - t) * mag[tab["row0"]] + t * mag[tab["row1"]]
        res[0] = lerp_adjoint(2.0 * magc / (magc * magc + EPS) * (np.asarray(g_m, dtype=np.float64) @ wm), tab, n_rows)
    for k, (g, out, x) in enumerate(((g_r, out_r, real), (g_i, out_i, imag)), start=1):
        if g is None:
            continue
        m = tab["voi"][:, None] & (np.abs(np.asarray(out, dtype=np.float64)) < 1.0)
        h = lerp_adjoint(np.where(m, np.asarray(g, dtype=np.float64), 0.0), tab, n_rows)
        res[k] = (2.0 - 2.0 * EPS * np.exp(-2.0 * x)) * (h @ wp)
    return tuple(res)


def grads_closed(mag, real, imag, out_r, out_i, grads, tab, n_smpls, fft_len, wm, wp):
    """d sig float64 numpy: warp_grads_closed, then the closed form of the lossless analysis' backward pass."""
    g = warp_grads_closed(mag, real, imag, out_r, out_i, grads, tab, wm, wp)
    return lossless.grads_closed(mag, real, imag, g, tab["pm"], tab["left"], tab["right"], n_smpls, fft_len)


def utterance(rng, n_frames, spacings, fs=FS):
    """One utterance of n_frames epochs whose spacings are drawn from `spacings` = [(samples, voiced)]: (a tone plus white
    noise at -10 dB in float32, v_pm_sec, v_voi)."""
    pick = [spacings[i] for i in rng.randint(len(spacings), size=n_frames)]
    pm = np.cumsum([s for s, _v in pick])
    n = int(np.ceil(pm[-1] + pick[-1][0])) + 2
    return (tone_and_noise(rng, n, fs=fs).astype(np.float32), pm / fs, np.asarray([1.0 if v else 0.0 for _s, v in pick]))


MIX = [(FS / 55.0, True), (FS / 400.0, True), (0.005 * FS, False)]


def batch_utts(fft_len):
    """The gradient tests' batch for fft_len: three utterances of 2, 37 and 70 frames, with 55 Hz, 400 Hz and unvoiced
    5 ms spacing mixed."""
    rng = np.random.RandomState(int(fft_len) + 1)
    return [utterance(rng, n, MIX) for n in (2, 37, 70)]
