"""
Float64 numpy restatement of the type-2 analysis pieces (magphase.py:2793-2866, :182-263), written from the reference's
text, for the CPU and GPU tests: the two-period magnitude frames (the even and odd epoch subsets of windowing), the
one-period phase frames, the per-frame gain and the float shifts.  No envelope here: tests/true_envelope_model.py.
"""
import numpy as np

from magphase_amd import hostmath as hm


def hann_win(left, right):
    """la.gen_non_symmetric_win(left, right, np.hanning) (libaudio.py:70-84)."""
    return np.hstack((np.hanning(1 + 2 * left)[:left + 1], np.flipud(np.hanning(1 + 2 * right)[:right + 1])[1:]))


def subset_bounds(pm, n):
    """windowing (magphase.py:77-98) of the even and the odd epoch subsets, rows interleaved back: (left, right)."""
    left, right = np.zeros(pm.size, dtype=np.int64), np.zeros(pm.size, dtype=np.int64)
    for par in (0, 1):
        idx = np.arange(par, pm.size, 2)
        ext = np.hstack((0, pm[idx], n - 1))
        left[idx] = ext[1:-1] - ext[:-2]
        right[idx] = ext[2:] - ext[1:-1]
    return left, right


def fft_input(v_sig, p, left, right, N):
    """The windowed frame, zero-padded or truncated to N, rotated by left (magphase.py:295-319 / :213-233)."""
    frm = v_sig[p - left:p + right + 1] * hann_win(left, right)
    c = np.zeros(N)
    c[:min(frm.size, N)] = frm[:N]
    return np.hstack((c[left:], c[:left])), frm


def gain(v_sig, p, left, right, voiced, N):
    """magphase.py:236-242."""
    c, frm = fft_input(v_sig, p, left, right, N)
    return np.max(np.abs(c[:N // 2 + 1])) if voiced else np.std(frm)


def analysis(v_sig, fs, v_pm_sec, v_voi, N):
    """-> dict: mag2 / mag1 (|X| of the two- / one-period frames), real, imag, f0, shift, gain; row 0 dropped as the reference
    does.  n_warn: the frames longer than N, row 0 included -- one warning each in the reference (two- and one-period)."""
    v_sig = np.asarray(v_sig, dtype=np.float64)
    n = v_sig.size
    pm_sec, voi = hm.clean_epochs(v_pm_sec, v_voi, check_len_smpls=n, fs=fs)
    pm_smpls = pm_sec * fs
    pm, left, right = hm.frame_bounds(pm_smpls, n)
    l2, r2 = subset_bounds(pm, n)
    H = N // 2 + 1
    X1 = np.array([np.fft.fft(fft_input(v_sig, p, a, b, N)[0])[:H] for p, a, b in zip(pm, left, right)])
    X2 = np.array([np.fft.fft(fft_input(v_sig, p, a, b, N)[0])[:H] for p, a, b in zip(pm, l2, r2)])
    mag1 = np.abs(X1)
    div = np.where(mag1 == 0.0, 1.0, mag1)
    real, imag = np.where(mag1 == 0.0, 0.0, X1.real / div), np.where(mag1 == 0.0, 0.0, X1.imag / div)
    g = np.array([gain(v_sig, p, a, b, v == 1, N) for p, a, b, v in zip(pm, left, right, voi)])
    with np.errstate(divide="ignore", invalid="ignore"):
        f0 = voi * fs / left.astype(np.float64)
    return {"mag2": np.abs(X2)[1:], "mag1": mag1[1:], "real": real[1:], "imag": imag[1:], "f0": f0[1:],
            "shift": np.diff(np.hstack((0, pm_smpls[1:]))), "gain": g[1:], "pm": pm, "left2": l2, "right2": r2,
            "n_warn": int(np.sum(l2 + r2 + 1 > N) + np.sum(left + right + 1 > N))}
