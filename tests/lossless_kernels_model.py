"""numpy models of the six kernels of the lossless path that have a C entry of their own (mpx_analysis_frames,
mpx_synthesis_lossless_frames, mpx_ola_gather, mpx_ola_fixup / _width, mpx_rows_lerp, mpx_rows_lerp_adjoint), written from
the header's text and the oracle's functions, not from the kernels.  tests/test_lossless_kernels_host.py holds every one of
them to oracle.magphase_oracle; tests/test_gpu_lossless_kernels.py holds the kernels to them.

Two of the models are float32 on purpose: the overlap-add gather and the fix-up perform a fixed sequence of float32
additions, so the device's result can be asked for bit for bit."""
import numpy as np

from oracle import magphase_oracle as orc

U = 2.0 ** -24          # the unit of every derived float32 bound

# numpy record layout of the C struct mpx_ola_run (include/magphase_hip.h): 56 bytes
OLA_RUN_DTYPE = np.dtype([("frame_begin", "<i4"), ("frame_end", "<i4"), ("x0", "<i4"), ("head_end", "<i4"),
                          ("out_lo", "<i4"), ("out_hi", "<i4"), ("flush_end", "<i4"), ("fix_lo", "<i4"),
                          ("fix_hi", "<i4"), ("pad", "<i4"), ("out_base", "<i8"), ("strip_off", "<i8")])


def frame_len(L, R, N):
    return min(int(L) + int(R) + 1, int(N))


def analysis_frame(sig, pos, L, R, N):
    """One frame of mpx_analysis_frames in float64: (mag, real, imag [N/2 + 1], l1).  The frame is sig[pos - L .. pos + R]
    under the oracle's half windows, truncated or zero-padded to N, rotated left by L (by 0 when L >= N: python slicing),
    np.fft.fft, bins 0 .. N/2, compute_lossless_feats' zero rule.  l1 = sum |w x| over the samples that enter the
    transform.  Only sig[pos - L : pos - L + len] is read, len = min(L + R + 1, N)."""
    pos, L, R, N = int(pos), int(L), int(R), int(N)
    n = frame_len(L, R, N)
    w = orc.half_windows(L, R)[:n]
    seg = np.asarray(sig[pos - L:pos - L + n], dtype=np.float64) * w
    row = np.zeros(N)
    row[:n] = seg
    s = L if L < N else 0
    row = np.concatenate((row[s:], row[:s]))
    X = np.fft.fft(row)[:N // 2 + 1]
    mag, real, imag, _ = orc.compute_lossless_feats(X[None, :], np.ones(1), np.zeros(1), 1.0)
    return mag[0], real[0], imag[0], float(np.sum(np.abs(seg)))


def synthesis_frame(mag, real, imag, N):
    """The per-frame part of oracle.synthesis_from_lossless for rows [F x N/2 + 1] -> frames float64 [F x N], epoch at
    N/2: unit phasor (|real + j imag| == 0 -> divided by 1, so such a bin is 0), Hermitian extension with the imaginary
    parts of bins 0 and N/2 dropped, ifft().real, fftshift."""
    mag, real, imag = [np.atleast_2d(np.asarray(x, dtype=np.float64)) for x in (mag, real, imag)]
    assert mag.shape[1] == N // 2 + 1
    ph = real + 1j * imag
    den = np.absolute(ph)
    den[den == 0.0] = 1.0
    full = orc.hermitian_full_spectrum(mag * ph / den)
    return np.fft.fftshift(np.fft.ifft(full).real, axes=1)


def synthesis_bound_term(mag, N):
    """sum_k c_k mag_k / N per frame, c_k = 1 at bins 0 and N/2 and 2 elsewhere: the largest a sample of the frame can be."""
    mag = np.atleast_2d(np.asarray(mag, dtype=np.float64))
    c = np.full(N // 2 + 1, 2.0)
    c[0] = c[-1] = 1.0
    return np.abs(mag) @ c / N


def ola_gather(frames, utt_frame_off, pm_rel, out_start, out_off, N, dtype=np.float32):
    """out[out_off[u] + t] = sum over the frames i of utterance u, ascending, of frames[i][t + out_start[u] - pm_rel[i]]
    where that index is in [0, N).  dtype float32: the additions one by one in float32 from 0.0, the kernel's own sequence;
    float64 for the comparison with the oracle."""
    frames = np.asarray(frames)
    out = np.zeros(int(out_off[-1]), dtype=dtype)
    for u in range(len(out_off) - 1):
        o0, n = int(out_off[u]), int(out_off[u + 1] - out_off[u])
        for i in range(int(utt_frame_off[u]), int(utt_frame_off[u + 1])):
            t0 = int(pm_rel[i]) - int(out_start[u])          # output index of the frame's sample 0
            lo, hi = max(t0, 0), min(t0 + N, n)
            if hi > lo:
                out[o0 + lo:o0 + hi] = out[o0 + lo:o0 + hi] + frames[i, lo - t0:hi - t0].astype(dtype)
    return out


def fixup_covered(run, max_width=None):
    """Elements [lo, hi) of a run that mpx_ola_fixup (max_width None) / mpx_ola_fixup_width complete: the launch covers whole
    1024-element blocks from fix_lo rounded down to 64, ceil(max_width / 1024) of them."""
    lo, hi = int(run["fix_lo"]), int(run["fix_hi"])
    if max_width is not None:
        hi = min(hi, (lo & ~63) + 1024 * ((int(max_width) + 1023) // 1024))
    return lo, max(hi, lo)


def ola_fixup(pcm, runs, strips, max_width=None):
    """float32: pcm[out_base + e] += strips[strip_off + e] for fix_lo <= e < fix_hi of every run (one float32 addition per
    element; the ranges of different runs do not meet in pcm)."""
    out = np.array(pcm, dtype=np.float32, copy=True)
    strips = np.asarray(strips, dtype=np.float32)
    for run in runs:
        lo, hi = fixup_covered(run, max_width)
        b, s = int(run["out_base"]), int(run["strip_off"])
        assert b + lo >= 0 or hi == lo
        out[b + lo:b + hi] = out[b + lo:b + hi] + strips[s + lo:s + hi]
    return out


def fixup_width(runs):
    """The widest fix_hi - (fix_lo & ~63) of a run table (0 for an empty one): mpx_ola_fixup_width's max_width."""
    return max([0] + [int(r["fix_hi"]) - (int(r["fix_lo"]) & ~63) for r in runs if r["fix_hi"] > r["fix_lo"]])


def rows_lerp(src, row0, row1, t):
    """float64 (1 - t) src[row0] + t src[row1] per output row, and the per-element term |b - a| t + |y| whose 2^-24-fold
    bounds fma(b - a, t, a) in float32 (the difference and the fused multiply-add round once each)."""
    src = np.asarray(src, dtype=np.float64)
    t = np.asarray(t, dtype=np.float64).reshape(-1, 1)
    a, b = src[np.asarray(row0, dtype=np.int64)], src[np.asarray(row1, dtype=np.int64)]
    y = (1.0 - t) * a + t * b
    return y, np.abs(b - a) * np.abs(t) + np.abs(y)


def rows_lerp_adjoint(g, ranges, t, n_rows):
    """float64 dst[r] = sum over the frames f of [a0, a1) of (1 - t_f) g[f] + sum over [b0, b1) of t_f g[f]; a frame of both
    ranges weighs exactly 1.  Returns (dst, sum |w g|, the number of terms) per element / per row."""
    g = np.asarray(g, dtype=np.float64)
    t = np.asarray(t, dtype=np.float64)
    ranges = np.asarray(ranges).reshape(-1, 4)
    dst, mag = np.zeros((n_rows, g.shape[1])), np.zeros((n_rows, g.shape[1]))
    count = np.zeros(n_rows, dtype=np.int64)
    for r in range(n_rows):
        a0, a1, b0, b1 = [int(v) for v in ranges[r]]
        in_a, in_b = set(range(a0, a1)), set(range(b0, b1))
        for f in sorted(in_a | in_b):
            w = 1.0 if (f in in_a and f in in_b) else (1.0 - t[f] if f in in_a else t[f])
            dst[r] += w * g[f]
            mag[r] += np.abs(w * g[f])
            count[r] += 1
    return dst, mag, count
