"""numpy float64 model of the three backward entries of magphase_grad.hip (mpx_synthesis_lossless_backward,
mpx_analysis_lossless_backward, mpx_analysis_lossless_const_rate_backward), written from the header's text
(include/magphase_hip.h), not from the kernels.  It takes the entries' own TABLES, not plans, so that the GPU tests can
choose every argument themselves -- tables no planner builds included.  tests/test_lossless_backward_kernels_host.py holds
it to the autograd models (torch float64 autograd); tests/test_gpu_lossless_backward_kernels.py holds the kernels to it.

Two parts are float32 on purpose, so that the device's result can be asked for bit for bit: the gather of the analysis
backward (a fixed sequence of float32 additions) and the constant-rate gradient row (a fixed sequence of float32 fused
multiply-adds).  The feature row of a frame with row tables is the forward's float32 fma(x1 - x0, t, x0), emulated exactly
(fma32): what the epilogue divides by is the length of THAT phasor, which can be far shorter than either row's."""
import numpy as np

from lossless_analysis_autograd_model import window

U = 2.0 ** -24          # the unit of every derived float32 bound
TINY = np.float32(1.0e-37)


def fma32(a, b, c):
    """float32 fma(a, b, c), correctly rounded: the product of two float32 is exact in float64; the sum is rounded to odd
    (TwoSum tells whether it was exact), and 53 >= 24 + 2 bits then make the final rounding to float32 the only one."""
    a, b, c = np.broadcast_arrays(*[np.asarray(x, dtype=np.float32).astype(np.float64) for x in (a, b, c)])
    p = a * b
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.ascontiguousarray(p + c)
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def lerp32(x, row0, row1, rowt):
    """Rows [F x H] float32 of fma(x[row1] - x[row0], t, x[row0]): a float32 subtraction, then the fused multiply-add."""
    x = np.asarray(x, dtype=np.float32)
    x0, x1 = x[np.asarray(row0, dtype=np.int64)], x[np.asarray(row1, dtype=np.int64)]
    with np.errstate(invalid="ignore"):
        return fma32(x1 - x0, np.asarray(rowt, dtype=np.float32).reshape(-1, 1), x0)


# ===================================================================================== mpx_synthesis_lossless_backward
def clamp_window(pos, lo, hi, N, total):
    """[lo, hi) of a frame clamped to [0, N] and to the buffer [0, total): -> (lo, hi), (0, 0) when nothing is left."""
    lo_c = max(int(lo), 0, -int(pos))
    hi_c = min(int(hi), int(N), int(total) - int(pos))
    return (lo_c, hi_c) if hi_c > lo_c else (0, 0)


def synth_windows(gy, pos, lo, hi, N):
    """float64 [F x N]: sample n of frame f is gy[pos[f] + n] for lo <= n < hi (clamped), zero elsewhere."""
    gy = np.asarray(gy, dtype=np.float64)
    w = np.zeros((len(pos), int(N)))
    for f in range(len(pos)):
        a, b = clamp_window(pos[f], lo[f], hi[f], N, gy.size)
        if b > a:
            w[f, a:b] = gy[int(pos[f]) + a:int(pos[f]) + b]
    return w


def ck(N):
    c = np.full(N // 2 + 1, 2.0)
    c[0] = c[-1] = 1.0
    return c


def synth_gx(win, N):
    """gX [F x N/2 + 1] complex of the windows: G = fft(ifftshift(window)), gX_k = c_k G_k / N, the imaginary parts of bins
    0 and N/2 dropped."""
    G = np.fft.fft(np.fft.ifftshift(np.asarray(win, dtype=np.float64), axes=1), axis=1)[:, :N // 2 + 1]
    gX = G * (ck(N) / N)
    gX[:, 0] = gX[:, 0].real
    gX[:, -1] = gX[:, -1].real
    return gX


def synth_rows(mag, real, imag, F, row0=None, row1=None, rowt=None):
    """The feature rows the F frames see, float64 [F x H] each: row f, or with row tables the float32 interpolation."""
    if row0 is None:
        return tuple(np.asarray(x, dtype=np.float32)[:F].astype(np.float64) for x in (mag, real, imag))
    return tuple(lerp32(x, row0, row1, rowt).astype(np.float64) for x in (mag, real, imag))


def synth_epilogue(m, a, b, gX):
    """u = (a + jb) / den, den = |a + jb| (1 where that is 0), d = Re(conj(u) gX):
    grad_mag = d, grad_real = (mag / den)(Re gX - Re u d), grad_imag = (mag / den)(Im gX - Im u d).  -> (three rows, den)"""
    absp = np.hypot(a, b)
    den = np.where(absp == 0, 1.0, absp)
    ur, ui = a / den, b / den
    d = ur * gX.real + ui * gX.imag
    return (d, m / den * (gX.real - ur * d), m / den * (gX.imag - ui * d)), den


def synth_backward_parts(gy, pos, lo, hi, mag, real, imag, N, row0=None, row1=None, rowt=None):
    """Everything the GPU test needs of one launch: dict(rows = (grad_mag, grad_real, grad_imag) [F x H], gX, l1 = the
    frames' ||window||_1, m / a / b = the feature rows the frames saw, den)."""
    win = synth_windows(gy, pos, lo, hi, N)
    gX = synth_gx(win, N)
    m, a, b = synth_rows(mag, real, imag, len(pos), row0, row1, rowt)
    rows, den = synth_epilogue(m, a, b, gX)
    return dict(rows=rows, gX=gX, l1=np.sum(np.abs(win), axis=1), m=m, a=a, b=b, den=den)


def synth_backward_rows(gy, pos, lo, hi, mag, real, imag, N, row0=None, row1=None, rowt=None):
    """(grad_mag, grad_real, grad_imag), float64 [F x H] each."""
    return synth_backward_parts(gy, pos, lo, hi, mag, real, imag, N, row0, row1, rowt)["rows"]


# ====================================================================================== mpx_analysis_lossless_backward
def frame_len(L, R, N):
    return min(int(L) + int(R) + 1, int(N))


def analysis_gx(mag, real, imag, gm, gr, gi):
    """gX = grad_mag (real + j imag) + ((grad_real + j grad_imag) - (real + j imag) d) / mag, d = real grad_real + imag
    grad_imag; 0 where mag * mag < 1e-37 in float32.  A None stream counts as zeros.  -> (gX complex, live)"""
    with np.errstate(over="ignore", under="ignore"):
        m32 = np.asarray(mag, dtype=np.float32)
        live = m32 * m32 >= TINY
    mag, a, b = (np.asarray(x, dtype=np.float64) for x in (mag, real, imag))
    gm, gr, gi = (np.zeros(mag.shape) if g is None else np.asarray(g, dtype=np.float64) for g in (gm, gr, gi))
    inv = np.where(live, 1.0 / np.where(live, mag, 1.0), 0.0)
    gmm = np.where(live, gm, 0.0)
    d = a * gr + b * gi
    return (gmm * a + (gr - a * d) * inv) + 1j * (gmm * b + (gi - b * d) * inv), live


def half_spectrum(gX):
    """Y_k = gX_k / 2 for 0 < k < N/2, Y_0 = Re gX_0, Y_{N/2} = Re gX_{N/2}."""
    Y = 0.5 * np.asarray(gX, dtype=np.complex128)
    Y[:, 0] = gX[:, 0].real
    Y[:, -1] = gX[:, -1].real
    return Y


def frames_of_gx(gX, left, right, N):
    """b = N irfft_N(Y); gfrm[k] = b[(k - rot) mod N] w(k) for 0 <= k < len -> list of F float64 arrays."""
    b = N * np.fft.irfft(half_spectrum(gX), n=N, axis=1)
    out = []
    for f, (L, R) in enumerate(zip(np.asarray(left).tolist(), np.asarray(right).tolist())):
        n = frame_len(L, R, N)
        rot = L if L < N else 0
        out.append(b[f, (np.arange(n) - rot) % N] * window(L, R, n))
    return out


def analysis_backward_frames(mag, real, imag, gm, gr, gi, left, right, N):
    """The header's gfrm: per frame its len = min(L + R + 1, N) samples, float64."""
    return frames_of_gx(analysis_gx(mag, real, imag, gm, gr, gi)[0], left, right, N)


def analysis_bound_terms(mag, real, imag, gm, gr, gi, N, eg=None):
    """Per frame (sum_k c_k |Y_k|, PW): the norm the transform's rounding is proportional to, and the float32 rounding of
    the pointwise step carried to a sample, PW = sum_k c_k (E_r + E_i)_k (E_i = 0 at bins 0 and N/2) with, per component x
    of (real, imag) and its gradient gx, D = |real grad_real| + |imag grad_imag|, sc the factor of Y:
        E_x = u sc (2 |grad_mag x| + (5 |gx| + 8 |x| D) / mag)
    (grad_mag x: the product and the final sum, 2; (gx - x d) / mag: the difference, the product with the reciprocal, the
    reciprocal itself 2, the final sum: 5; x d: its product 1 and d's three roundings <= 2 D: 3 |x| D, and |gx - x d| <=
    |gx| + |x| D).  eg = (e_m, e_r, e_i): absolute errors the gradient rows already carry (the constant-rate arm's sums),
    passed through the same linear map."""
    gX, live = analysis_gx(mag, real, imag, gm, gr, gi)
    Y = half_spectrum(gX)
    c = ck(N)
    mag, a, b = (np.asarray(x, dtype=np.float64) for x in (mag, real, imag))
    gm, gr, gi = (np.zeros(mag.shape) if g is None else np.abs(np.asarray(g, dtype=np.float64)) for g in (gm, gr, gi))
    inv = np.where(live, 1.0 / np.where(live, mag, 1.0), 0.0)
    gmm = np.where(live, gm, 0.0)
    a, b = np.abs(a), np.abs(b)
    D = a * gr + b * gi
    e_r = U * (2 * gmm * a + (5 * gr + 8 * a * D) * inv)
    e_i = U * (2 * gmm * b + (5 * gi + 8 * b * D) * inv)
    if eg is not None:
        em, er, ei = (np.zeros(mag.shape) if x is None else np.asarray(x, dtype=np.float64) for x in eg)
        De = a * er + b * ei
        e_r = e_r + np.where(live, em, 0.0) * a + (er + a * De) * inv
        e_i = e_i + np.where(live, em, 0.0) * b + (ei + b * De) * inv
    e_i[:, 0] = e_i[:, -1] = 0.0
    sc = c / 2
    sc[0] = sc[-1] = 1.0
    return np.abs(Y) @ c, ((e_r + e_i) * sc) @ c


def gather(frames_scratch, pos, left, scratch_off, total, dtype=np.float32):
    """grad_sig[t] = sum over the frames f, ascending, that cover t of scratch[scratch_off[f] + t - (pos[f] - left[f])];
    frame f covers scratch_off[f + 1] - scratch_off[f] samples from pos[f] - left[f], and a frame whose slot does not lie
    within the scratch adds nothing.  dtype float32: the additions one by one in float32 from 0.0 -- fed the device's own
    scratch, the device's exact sum."""
    scratch = np.asarray(frames_scratch)
    off = np.asarray(scratch_off, dtype=np.int64)
    out = np.zeros(int(total), dtype=dtype)
    for f in range(off.size - 1):
        start, o, n = int(pos[f]) - int(left[f]), int(off[f]), int(off[f + 1] - off[f])
        if n <= 0 or o < 0 or o + n > scratch.size:
            continue
        lo, hi = max(start, 0), min(start + n, int(total))
        if hi > lo:
            out[lo:hi] = out[lo:hi] + scratch[o + lo - start:o + hi - start].astype(dtype)
    return out


# =========================================================================== mpx_analysis_lossless_const_rate_backward
def clamp_ranges(ranges, n_crows):
    return np.clip(np.asarray(ranges, dtype=np.int64).reshape(-1, 4), 0, int(n_crows)).astype(np.int32)


def cr_gradient_rows(g, ranges, rowt, n_crows, dtype=np.float64):
    """Frame f's gradient row [F x H] from the constant-rate rows g [n_crows x H]: ranges (a0, a1, b0, b1) per frame,
    clamped to [0, n_crows]; c ascending over the union of [a0, a1) and [b0, b1); weight 1 in both, 1 - rowt[c] in the first
    only, rowt[c] in the second only; acc = fma(w, g[c], acc) from 0 (float32: that very sequence, correctly rounded).
    g None -> None."""
    if g is None:
        return None
    g = np.asarray(g, dtype=dtype)
    t = np.asarray(rowt, dtype=dtype)
    rng = clamp_ranges(ranges, n_crows)
    out = np.zeros((rng.shape[0], g.shape[1]), dtype=dtype)
    for f, (a0, a1, b0, b1) in enumerate(rng.tolist()):
        for c in sorted(set(range(a0, a1)) | set(range(b0, b1))):
            in_a, in_b = a0 <= c < a1, b0 <= c < b1
            w = dtype(1.0) if (in_a and in_b) else (dtype(1.0) - t[c] if in_a else t[c])
            out[f] = fma32(w, g[c], out[f]) if dtype == np.float32 else out[f] + w * g[c]
    return out


def cr_gradient_rows_error(g, ranges, rowt, n_crows):
    """(n + 2) u sum |w g| per element: the bound of the row sums' float32 rounding (n terms: n fused multiply-adds, 1 - t,
    w g), as tests/test_gpu_lossless_kernels.py derives it for mpx_rows_lerp_adjoint."""
    if g is None:
        return None
    g = np.abs(np.asarray(g, dtype=np.float64))
    t = np.asarray(rowt, dtype=np.float64)
    rng = clamp_ranges(ranges, n_crows)
    out = np.zeros((rng.shape[0], g.shape[1]))
    for f, (a0, a1, b0, b1) in enumerate(rng.tolist()):
        cs = sorted(set(range(a0, a1)) | set(range(b0, b1)))
        for c in cs:
            in_a, in_b = a0 <= c < a1, b0 <= c < b1
            out[f] += (1.0 if (in_a and in_b) else abs(1.0 - t[c] if in_a else t[c])) * g[c]
        out[f] *= (len(cs) + 2) * U
    return out
