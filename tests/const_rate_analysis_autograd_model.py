"""
float64 model of the constant-rate lossless analysis and of its backward pass (the CR arm), for
tests/test_const_rate_analysis_autograd_host.py and tests/test_gpu_const_rate_analysis_autograd.py.  Needs neither a GPU
nor the library.

The forward is the analysis of tests/lossless_analysis_autograd_model.py followed by out[c] = (1 - t_c) rows[row0_c] +
t_c rows[row1_c] with the tables of hostmath.var_to_const_rate_batch, in plain torch float64, so that torch's autograd
gives the gradients; grads_closed is the closed form the HIP kernels implement: the interpolation's adjoint onto the
variable-rate rows (lerp_adjoint: hostmath.lerp_adjoint_table's ranges walked as the kernels walk them), then the lossless
analysis' closed form.
"""
import numpy as np
import torch

import lossless_analysis_autograd_model as base
from magphase_amd import hostmath as hm

rel_err = base.rel_err


def frames_and_tables(v_pm_sec, v_voi, n_smpls, fs, const_rate_ms):
    """One utterance: ((pm, left, right), (row0, row1, t), v_f0_c) -- the frame table as LosslessAnalysisPlan builds it and
    the row tables / constant-rate f0 of hostmath.var_to_const_rate_batch (rows counted from the utterance's first frame).
    """
    pm, left, right, voi = base.frames_of(v_pm_sec, v_voi, n_smpls, fs)
    f0 = hm.shift_to_f0(left, voi, fs)
    row0, row1, t, f0_c, off = hm.var_to_const_rate_batch([left], [f0], [0], fs, const_rate_ms)
    assert off.tolist() == [0, row0.size] and f0_c[0].size == row0.size
    return (pm, left, right), (row0, row1, t), f0_c[0]


def lerp_torch(rows, tabs):
    """rows [F x H] (torch float64) -> [F_c x H]."""
    row0, row1, t = tabs
    if np.size(row0) == 0:
        return rows.new_zeros((0, rows.shape[1]))
    r0, r1 = torch.from_numpy(np.asarray(row0, dtype=np.int64)), torch.from_numpy(np.asarray(row1, dtype=np.int64))
    w = torch.from_numpy(np.asarray(t, dtype=np.float64))[:, None]
    return (1.0 - w) * rows[r0] + w * rows[r1]


def forward_torch(sig, frames, tabs, fft_len):
    """One utterance: sig torch float64 [n] -> (mag, real, imag) [F_c x H] at the constant rate (differentiable)."""
    return tuple(lerp_torch(x, tabs) for x in base.forward_torch(sig, frames[0], frames[1], frames[2], fft_len))


def forward_numpy(sig, frames, tabs, fft_len):
    with torch.no_grad():
        return tuple(x.numpy() for x in forward_torch(torch.as_tensor(np.asarray(sig, dtype=np.float64)), frames, tabs,
                                                      fft_len))


def grads_autograd(sig, grads, frames, tabs, fft_len):
    """d sig float64 numpy of sum_k sum(grads[k] * forward[k]) by torch autograd; grads[k] None: output k not used."""
    x = torch.tensor(np.asarray(sig, dtype=np.float64), requires_grad=True)
    out = forward_torch(x, frames, tabs, fft_len)
    loss = sum((o * torch.as_tensor(np.asarray(g, dtype=np.float64))).sum() for o, g in zip(out, grads) if g is not None)
    if not (torch.is_tensor(loss) and loss.requires_grad):
        return np.zeros(x.shape)
    loss.backward()
    return x.grad.numpy()


def lerp_matrix(tabs, n_var):
    """The interpolation as a dense [F_c x n_var] float64 matrix (row c: 1 - t_c at row0_c plus t_c at row1_c)."""
    row0, row1, t = (np.asarray(x) for x in tabs)
    A = np.zeros((row0.size, int(n_var)))
    c = np.arange(row0.size)
    np.add.at(A, (c, row0), 1.0 - t)
    np.add.at(A, (c, row1), t)
    return A


def lerp_adjoint(g, ranges, t, dtype=np.float64):
    """What the kernels compute from hostmath.lerp_adjoint_table's ranges [n_var x 4]: per variable frame the union of the
    two constant-rate row ranges in ascending order, weight 1 in both, 1 - t in the first only, t in the second only.
    g: [F_c x H] or None -> [n_var x H] or None."""
    if g is None:
        return None
    g, t = np.asarray(g, dtype=dtype), np.asarray(t, dtype=dtype)
    out = np.zeros((ranges.shape[0], g.shape[1]), dtype=dtype)
    for f, (a0, a1, b0, b1) in enumerate(np.asarray(ranges).tolist()):
        for c in sorted(set(range(a0, a1)) | set(range(b0, b1))):
            in_a, in_b = a0 <= c < a1, b0 <= c < b1
            w = dtype(1.0) if in_a and in_b else (dtype(1.0) - t[c] if in_a else t[c])
            out[f] += w * g[c]
    return out


def grads_closed(mag, real, imag, grads, frames, tabs, n_smpls, fft_len):
    """The closed form, numpy float64, from the VARIABLE-rate rows mag / real / imag [F x H] of the forward and the
    gradients of the constant-rate rows."""
    n_var = int(np.shape(mag)[0])
    ranges = hm.lerp_adjoint_table(tabs[0], tabs[1], tabs[2], n_var)
    g_var = tuple(lerp_adjoint(g, ranges, tabs[2]) for g in grads)
    return base.grads_closed(mag, real, imag, g_var, frames[0], frames[1], frames[2], n_smpls, fft_len)
