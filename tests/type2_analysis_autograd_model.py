"""
float64 torch model of the type-2 analysis chain and of its gradient, for
tests/test_type2_analysis_autograd_host.py and tests/test_gpu_type2_analysis_autograd.py.  Needs neither a GPU nor the
library.

The chain: the one-period frames (phase rows) and the two-period frames (magnitude rows) of the same epochs through
lossless_analysis_autograd_model.forward_torch, the true envelope of the two-period magnitudes at 600 coefficients with
forced pass counts and optionally GIVEN decisions (true_envelope_autograd_model.envelope_torch: the device's own, so that a
gradient is compared as the adjoint of the passes the device ran), then -- for the compressed form -- the two mel warps and
the row interpolation of compressed_analysis_autograd_model.warp_torch on the type-2 row tables.  Row 0 of every utterance
is computed and dropped by the caller, as the product does.
"""
import numpy as np
import torch

import compressed_analysis_autograd_model as cmodel
import lossless_analysis_autograd_model as lossless
import true_envelope_autograd_model as tam
from magphase_amd import hostmath as hm

ENV_NCOEFFS = 600


def batch_tables(utts):
    """utts = [(v_sig, fs, v_pm_sec, v_voi)] -> the batch's frame tables over the concatenated signal: pos, left, right (one
    period), left2, right2 (two periods), frame_off [n_utts + 1], smpl_off [n_utts + 1]."""
    pos, left, right, l2, r2, fo, so = [], [], [], [], [], [0], [0]
    for v_sig, fs, v_pm_sec, v_voi in utts:
        n = int(np.shape(v_sig)[0])
        pm, lf, rg, _voi = lossless.frames_of(v_pm_sec, v_voi, n, fs)
        a, b = hm.two_period_frame_bounds(pm, n)
        pos.append(np.asarray(pm, dtype=np.int64) + so[-1])
        left.append(lf), right.append(rg), l2.append(a), r2.append(b)
        fo.append(fo[-1] + len(pm)), so.append(so[-1] + n)
    cat = lambda v: np.concatenate(v).astype(np.int64)   # noqa: E731
    return {"pos": cat(pos), "left": cat(left), "right": cat(right), "left2": cat(l2), "right2": cat(r2),
            "frame_off": np.asarray(fo), "smpl_off": np.asarray(so)}


def out_rows(tab):
    """The rows the product returns: every row but row 0 of each utterance."""
    fo = tab["frame_off"]
    return np.concatenate([np.arange(min(a + 1, b), b) for a, b in zip(fo[:-1], fo[1:])] or [np.zeros(0, np.int64)])


def forward_torch(sig, tab, fft_len, iters, decisions=None):
    """sig: float64 tensor, the batch's samples end to end -> (env, real, imag [F x H], decisions used, margins)."""
    _m1, real, imag = lossless.forward_torch(sig, tab["pos"], tab["left"], tab["right"], fft_len)
    mag2, _r2, _i2 = lossless.forward_torch(sig, tab["pos"], tab["left2"], tab["right2"], fft_len)
    env, used, margin = tam.envelope_torch(mag2, "abs", ENV_NCOEFFS, iters, decisions)
    return env, real, imag, used, margin


def compressed_torch(sig, tab, rows_tab, fft_len, iters, decisions, wm, wp, b_norm_mag=False):
    """The compressed form: rows_tab = {"row0", "row1", "rowt", "voi"} of the output frames over the F rows.  -> (m_mag_mel_log,
    m_real_mel, m_imag_mel, pre-clip real, pre-clip imag)."""
    env, real, imag, _used, _margin = forward_torch(sig, tab, fft_len, iters, decisions)
    m, r, i, pre_r, pre_i = cmodel.warp_torch(env, real, imag, rows_tab, wm, wp)
    if b_norm_mag:   # magphase.py:3178-3182
        mean = m[:, 1:].mean(dim=1)
        m = torch.cat((mean[:, None], m[:, 1:] - mean[:, None]), dim=1)
    return m, r, i, pre_r, pre_i


def grads_of(sig, outs_fn, grads):
    """d sig float64 numpy of sum_k sum(grads[k] * outs_fn(x)[k]); grads[k] None: output k not used."""
    x = torch.tensor(np.asarray(sig, dtype=np.float64), requires_grad=True)
    outs = outs_fn(x)
    loss = sum((o * torch.as_tensor(np.asarray(g, dtype=np.float64))).sum() for o, g in zip(outs, grads) if g is not None)
    loss.backward()
    return x.grad.numpy()


def utterance(rng, fs, fft_len, n_voiced, n_unvoiced, gap=True):
    """A synthetic utterance (float32 tone plus noise, v_pm_sec, v_voi): a voiced stretch at ~145 Hz, an unvoiced one at
    5 ms, and (gap) three unvoiced epochs so far apart that their two-period frames exceed fft_len, then voiced again."""
    t0 = fs / 145.0
    spac = [t0 * (1.0 + 0.03 * rng.randn()) for _ in range(n_voiced)]
    voi = [1.0] * n_voiced
    spac += [0.005 * fs] * n_unvoiced
    voi += [0.0] * n_unvoiced
    if gap:
        spac += [0.4 * fft_len] * 3
        voi += [0.0] * 3
    spac += [t0] * 4
    voi += [1.0] * 4
    pm = np.cumsum(spac)
    n = int(np.ceil(pm[-1] + t0)) + 2
    return lossless.tone_and_noise(rng, n, f0=145.0, fs=fs).astype(np.float32), pm / fs, np.asarray(voi)
