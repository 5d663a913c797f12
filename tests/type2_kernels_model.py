"""
References of the three type-2 kernels of magphase_type2.hip (k_frame_gain, k_noise_power, k_noise_rms) for the CPU and
GPU tests, numpy only, together with the frame shapes, signals and buffer layout those tests share.

  frame_gain_ref   magphase.py:227-249 restated literally (window, pad or truncate, hstack rotation, max over the first
                   N/2 + 1 samples or np.std of the unpadded frame), evaluated in np.longdouble.
  noise_power_ref  sum_{k <= N/2} |rfft(frame placed as la.frm_list_to_matrix + fftshift places it)|^2, through
                   np.fft.rfft -- NOT through the three-sum identity the kernel uses.  The reference's placement exists
                   for left <= N/2 and right <= N/2 - 1 only; elsewhere it raises, and `extended=True` gives the
                   extension DESIGN.md section 3.3f states: the first N samples of the windowed frame.
  noise_rms_ref    sqrt(sum of an utterance's frame powers / (frames * (N/2 + 1))), NaN for an utterance without frames.
"""
import math

import numpy as np

FFT_LENS = (1024, 2048, 4096)
SIGNALS = ("uniform", "dc", "alternating", "zeros")
BASE_SHAPES = [(0, 0), (0, 1), (1, 0), (1, 1), (31, 32), (63, 63), (63, 64), (64, 64), (100, 3), (3, 100)]
EPS = 2.0 ** -53


def half_windows(L, R, win=np.hanning):
    """The rising half of win(2L + 1) and the falling half of win(2R + 1) around one centre sample: L + R + 1 values."""
    return np.hstack((win(2 * L + 1)[:L + 1], win(2 * R + 1)[R:][1:]))


def voi_noise_window(n):
    return np.bartlett(n) ** 2.5


def frame_gain_ref(sig, pos, L, R, voiced, N):
    w = half_windows(L, R)
    frm = np.asarray(sig[pos - L:pos + R + 1], dtype=np.longdouble) * w.astype(np.longdouble)
    assert frm.size == L + R + 1
    if not voiced:
        return np.std(frm)
    c = np.zeros(N, dtype=np.longdouble)
    if frm.size <= N:
        c[:frm.size] = frm
    else:
        c[:] = frm[:N]
    c = np.hstack((c[L:], c[:L]))
    return np.max(np.abs(c[:N // 2 + 1]))


def noise_in_domain(L, R, N):
    """Where la.frm_list_to_matrix can place the frame (its epoch on index N/2)."""
    return L <= N // 2 and R <= N // 2 - 1


def noise_frame(noise, pos, L, R, wtype):
    w = half_windows(L, R, voi_noise_window if wtype else np.hanning)
    return np.asarray(noise[pos - L:pos + R + 1], dtype=np.float64) * w


def noise_power_ref(noise, pos, L, R, wtype, N, extended=False):
    frm = noise_frame(noise, pos, L, R, wtype)
    m = np.zeros(N)
    if extended:
        n = min(frm.size, N)
        m[:n] = frm[:n]
    else:
        start = N // 2 - L
        if start < 0 or start + frm.size > N:
            raise ValueError("negative dimensions are not allowed")
        m[start:start + frm.size] = frm
        m = np.fft.fftshift(m)
    X = np.fft.rfft(m)
    assert X.size == N // 2 + 1
    return float(np.sum(X.real ** 2 + X.imag ** 2))


def noise_rms_ref(power, utt_frame_off, N):
    out = []
    for a, b in zip(utt_frame_off[:-1], utt_frame_off[1:]):
        a, b = int(a), int(b)
        out.append(math.sqrt(math.fsum(power[a:b]) / ((b - a) * (N // 2 + 1))) if b > a else float("nan"))
    return np.asarray(out, dtype=np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# what the CPU and GPU tests share: shapes, layout, signals
# ---------------------------------------------------------------------------------------------------------------------
def shapes(N, gain=False):
    """(L, R) of the directed frames: N - 1, N, N + 1 and more samples around the FFT length; for the gain also left >= N
    (no rotation) and frames far longer than N on either side (truncation, the wrap of the rotated index)."""
    s = BASE_SHAPES + [(N // 2 - 1, N // 2 - 1), (N // 2 - 1, N // 2), (N // 2, N // 2)]
    # (N/2, N/2) loses one sample to the truncation, and that sample's window value is 0: only a frame that is longer
    # still shows whether the kernels stop at N samples
    s = s + [(N // 2 + 9, N // 2), (N // 2, N // 2 + 9), (100, N)]
    if gain:
        s = s + [(N - 1, 5), (N, 5), (N + 7, 40), (5, N + 7)]
    return s


def frame_table(N, n_frames, gain, seed=0):
    """-> (left, right, flag, parity): every directed shape at an even and at an odd buffer offset, each with flag 1 and
    0 (voiced / unvoiced, or the bartlett**2.5 / Hann window), then small frames (L, R <= 70) up to n_frames."""
    rows = [(L, R, f, p) for (L, R) in shapes(N, gain) for f in (1, 0) for p in (0, 1)]
    assert n_frames >= len(rows)
    rs = np.random.RandomState(seed)
    n_pad = n_frames - len(rows)
    pad = np.stack((rs.randint(0, 71, n_pad), rs.randint(0, 71, n_pad), rs.randint(0, 2, n_pad), rs.randint(0, 2, n_pad)), 1)
    t = np.concatenate((np.asarray(rows, dtype=np.int64).reshape(-1, 4), pad.astype(np.int64)))
    return t[:, 0].copy(), t[:, 1].copy(), t[:, 2].copy(), t[:, 3].copy()


def layout(left, right, parity):
    """Frames side by side in one buffer, frame f's first sample at an offset of parity[f]: (pos, buffer length)."""
    pos = np.zeros(left.size, dtype=np.int64)
    cur = 0
    for f in range(left.size):
        cur += int((cur & 1) != int(parity[f]))
        pos[f] = cur + left[f]
        cur += left[f] + right[f] + 1
    return pos, int(cur)


def make_signal(kind, n, seed=1):
    """float32-exact samples as float64: the device and the reference read the same numbers."""
    rs = np.random.RandomState(seed)
    if kind == "uniform":
        x = rs.uniform(-1, 1, n)
    elif kind == "dc":
        x = rs.uniform(0, 1, n)
    elif kind == "alternating":
        x = rs.uniform(0.5, 1, n) * (1 - 2 * (np.arange(n) & 1))
    elif kind == "zeros":
        x = np.zeros(n)
    else:
        raise ValueError(kind)
    return x.astype(np.float32).astype(np.float64)


def noise_power_bound(N):
    """First-order error of sequentially summing <= N non-negative float64 terms, with a factor for the window and the
    final combination; the cancelling sums are bounded against the first term by (sum |x|)^2 <= N sum x^2."""
    return 4.0 * N * EPS
