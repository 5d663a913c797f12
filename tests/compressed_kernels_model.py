"""
References of the forward kernels of the compressed path for the CPU and GPU tests, numpy only, float64 / longdouble:
one function per kernel, taking the float32 arrays the kernel reads, together with the operands, tables and shapes the
two test files share (tests/test_compressed_kernels_host.py checks the references and the decision margins of every
operand set; tests/test_gpu_compressed_kernels.py compares the kernels with them).

  unwarp_ref            k_mel_unwarp_mfma / k_mel_unwarp_tiled: A @ U in longdouble, exp for the magnitude job, the
                        constant -> variable rate interpolation as the device defines it (linear jobs: on the coefficient
                        rows; exp job: on the exponentials).
  warp_ref              k_mel_warp_mfma: prologue(x) @ W^T with the four prologue / epilogue modes documented above
                        warp_prologue in magphase_warp.hip; the interpolated row is formed before the prologue.
  warp_phase_rows_ref   k_warp_phase_rows: row interpolation of the variable-rate warp outputs, mode-1 mask and clip.
  min_phase_ref         k_min_phase: la.build_min_phase_from_mag_spec restated (float64, np.fft), the phase only;
                        min_phase_dft_ref is the same by longdouble cosine / sine matrices (N = 1024).
  noise_stats_ref       k_noise_stats: sum_{k=1}^{N/2-1} (ln|Ns_k|)^2 of the windowed, zero-padded noise frame.
  noise_gains_ref       k_noise_gains: sqrt(exp(mean)) per utterance and class, NaN for an empty class, 1/g per frame.
  post_filter_ref       k_post_filter: centred moving average, enhancement, end bins copied.
"""
import math

import numpy as np

from type2_kernels_model import BASE_SHAPES, layout, noise_frame

LD = np.longdouble
U24 = 2.0 ** -24           # unit round-off of float32
MAGIC = -1.0e10            # la.log's value at 0 (libaudio.py:241-248)
EXP_FLOOR = -745.13321     # ln of the smallest float64: below it the reference's exp underflows (mode 2)
SENTINEL = -7.25
FFT_LENS = (1024, 2048, 4096)


def f32(x):
    """float32-exact values as float64: the device and the reference read the same numbers."""
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def lerp(a, b, t):
    """a + (b - a) t: exact at t == 0; at t == 1 it returns b wherever b - a is exact in the working precision."""
    return a + (b - a) * t


def lerp_f32(a, b, t):
    """fmaf(b - a, t, a) as the device evaluates it: the float32 difference, then one rounding of the fma (the product of
    two 24-bit factors is exact in longdouble and the sum keeps 64 bits before the one rounding to float32)."""
    a, b, t = (np.asarray(v, dtype=np.float32) for v in (a, b, t))
    d = (b - a).astype(np.float32)
    return (d.astype(LD) * t.astype(LD) + a.astype(LD)).astype(np.float32)


def _col(t):
    return np.asarray(t, dtype=np.float32).astype(LD)[:, None]


# ---------------------------------------------------------------------------------------------------------------------
# mel unwarp
# ---------------------------------------------------------------------------------------------------------------------
def unwarp_ref(A, U, op, row0=None, row1=None, rowt=None):
    """-> (values, absdot), longdouble.  A [rows x K], U [K x H] float32; op 1 applies exp.  With row tables output row f
    is, for a linear job, lerp(A[r0], A[r1]) @ U and, for the exp job, lerp(exp(A[r0] @ U), exp(A[r1] @ U)).
    absdot = |A| @ |U| of the (interpolated: (|A[r0]| (1 - t) + |A[r1]| t)) coefficient rows."""
    A, U = np.asarray(A).astype(LD), np.asarray(U).astype(LD)   # float32 from the GPU tests; widened as they are
    aU = np.abs(U)
    if row0 is None:
        v = A @ U
        return (np.exp(v) if op else v), np.abs(A) @ aU
    r0, r1, t = np.asarray(row0), np.asarray(row1), _col(rowt)
    absdot = (np.abs(A[r0]) * (1 - t) + np.abs(A[r1]) * t) @ aU
    if op:
        return lerp(np.exp(A[r0] @ U), np.exp(A[r1] @ U), t), absdot
    return lerp(A[r0], A[r1], t) @ U, absdot


# ---------------------------------------------------------------------------------------------------------------------
# mel warp
# ---------------------------------------------------------------------------------------------------------------------
def warp_prologue_ref(mode, x):
    x = np.asarray(x, dtype=LD)
    if mode == 0:
        return np.log(x * x + LD(1.0e-8))
    if mode in (1, 3):
        return np.log(np.exp(2 * x) + LD(1.0e-8))
    if mode == 2:
        out = np.full(x.shape, LD(MAGIC))
        pos = x > 0
        out[pos] = np.log(x[pos])
        return out
    raise ValueError(mode)


def warp_ref(x, W, mode, voi=None, row0=None, row1=None, rowt=None):
    """-> (values [F x nout], absdot), longdouble.  x [rows x H], W [nout x H] float32.  out = post(pre(x~) @ W^T), x~ the
    row itself or lerp(x[r0], x[r1], t), formed BEFORE the prologue.  Epilogue of mode 1: +0 for voi == 0, else
    clip(y voi, -1, 1); of mode 2: MAGIC below EXP_FLOOR; modes 0 and 3: none."""
    x, W = np.asarray(x), np.asarray(W).astype(LD)
    if row0 is not None:
        # the operand IS the float32 value fmaf(x[r1] - x[r0], t, x[r0]) (the backward pass differentiates the same one):
        # between unrelated rows the float32 difference cancels, which is the operand's rounding and not the product's;
        # test_compressed_kernels_host.py holds lerp_f32 to the exact lerp within one rounding of each step
        x = lerp_f32(x[np.asarray(row0)], x[np.asarray(row1)], np.asarray(rowt, dtype=np.float32)[:, None])
    p = warp_prologue_ref(mode, x.astype(LD))
    y = p @ W.T
    absdot = np.abs(p) @ np.abs(W).T
    if mode == 1 and voi is not None:
        y = mask_clip(y, voi)
    elif mode == 2:
        y = np.where(y < LD(EXP_FLOOR), LD(MAGIC), y)
    return y, absdot


def mask_clip(y, voi):
    v = np.asarray(voi, dtype=np.float32).astype(LD)[:, None]
    return np.where(v == 0, LD(0.0), np.clip(y * v, -1, 1))


def warp_phase_rows_ref(tr, ti, row0, row1, rowt, voi):
    """-> (out_real, out_imag): clip(voi lerp(tmp[r0], tmp[r1], t)), +0 where voi == 0 (rows of tmp that only unvoiced
    frames name are not read: they may hold anything)."""
    r0, r1, t = np.asarray(row0), np.asarray(row1), _col(rowt)
    live = np.asarray(voi) != 0
    out = []
    for m in (tr, ti):
        m = np.asarray(m).astype(LD)
        y = np.zeros((r0.size, m.shape[1]), dtype=LD)
        y[live] = lerp(m[r0[live]], m[r1[live]], t[live])
        out.append(mask_clip(y, voi))
    return out[0], out[1]


# ---------------------------------------------------------------------------------------------------------------------
# minimum phase
# ---------------------------------------------------------------------------------------------------------------------
def _log_protected(m):
    out = np.full(m.shape, MAGIC, dtype=m.dtype)
    out[m > 0] = np.log(m[m > 0])
    return out


def min_phase_ref(mag_rows, N):
    """The phase of la.build_min_phase_from_mag_spec (libaudio.py:920-934), float64: protected log, even extension,
    irfft, fold (c[1 .. N/2 - 1] *= 2, c[N/2 + 1 ..] = 0), fft, imaginary part.  -> phi [rows x N/2 + 1]; the unit phasor
    the kernel writes is (cos phi, sin phi)."""
    m = np.asarray(mag_rows).astype(np.float64)
    half = N // 2 + 1
    assert m.shape[1] == half
    c = np.fft.irfft(_log_protected(m), n=N, axis=1)
    c[:, 1:half - 1] *= 2.0
    c[:, half:] = 0.0
    return np.fft.fft(c, axis=1)[:, :half].imag


def min_phase_dft_ref(mag_rows, N=1024):
    """The same by matrices in longdouble (no FFT): c[n] = (1/N) sum_k w_k ln m_k cos(2 pi k n / N), w_0 = w_{N/2} = 1,
    else 2; phi[k] = -sum_n fold(c)[n] sin(2 pi k n / N).  The angles are reduced exactly (k n mod N) before the cosine."""
    m = np.asarray(mag_rows).astype(LD)
    half = N // 2 + 1
    idx = np.outer(np.arange(half), np.arange(half)) % N
    ang = idx.astype(LD) * (2 * np.arccos(LD(-1.0))) / N   # pi in longdouble, not float64's
    w = np.full(half, LD(2.0))
    w[0] = w[-1] = 1
    c = (_log_protected(m) * w) @ np.cos(ang) / N
    c[:, 1:half - 1] *= 2
    return -(c @ np.sin(ang))


def allpole_spectrum(poles, N, gain=1.0):
    """|1 / A(e^{jw})| and its minimum phase -angle(A) on the N/2 + 1 bins, A(z) = prod (1 - p z^-1), |p| < 1 (poles
    given with their conjugates).  The cepstrum of 1/A decays as |p|^n / n: with |p| <= 0.9 what aliases at N >= 1024 is
    below 1e-24, so the sampled cepstrum's fold gives this phase."""
    w = 2 * np.pi * np.arange(N // 2 + 1) / N
    a = np.ones(w.size, dtype=complex)
    for p in poles:
        a = a * (1 - p * np.exp(-1j * w))
    return gain / np.abs(a), -np.unwrap(np.angle(a))


def hilbert_noise_bound(N):
    """What one float32 rounding of every magnitude (|d ln m| <= 2^-24) can move the minimum phase by: the discrete
    Hilbert transform's infinity norm is below (2 / pi) (ln N + 1) < ln N + 2."""
    return U24 * (math.log(N) + 2.0)


def phasor_angle_error(re, im, phi):
    """Angle (radians) of the device phasor relative to the reference angle phi, in (-pi, pi]."""
    re, im = np.asarray(re, dtype=np.float64), np.asarray(im, dtype=np.float64)
    c, s = np.cos(phi), np.sin(phi)
    return np.arctan2(im * c - re * s, re * c + im * s)


# ---------------------------------------------------------------------------------------------------------------------
# noise statistic and gains
# ---------------------------------------------------------------------------------------------------------------------
def noise_spectrum_ref(noise, pos, L, R, wtype, N):
    frm = noise_frame(noise, pos, L, R, wtype)
    assert frm.size <= N
    return np.fft.rfft(frm, n=N)


def noise_stats_ref(noise, pos, L, R, wtype, N):
    """sum_{k=1}^{N/2-1} (ln|Ns_k|)^2, float64; the frame and its window from type2_kernels_model.noise_frame, placed at
    index 0 (|Ns| does not depend on the placement).  An exact zero takes the protected log."""
    X = noise_spectrum_ref(noise, pos, L, R, wtype, N)
    a = np.abs(X[1:N // 2])
    return float(np.sum(_log_protected(a) ** 2))


def noise_gains_ref(sums, voiced, utt_frame_off, bins):
    """-> (gains [n_utts x 2] float64: voiced, unvoiced; NaN for an empty class, inv_gain [frames] float64)."""
    sums = np.asarray(sums).astype(np.float64)
    voiced = np.asarray(voiced) != 0
    off = [int(o) for o in utt_frame_off]
    gains = np.full((len(off) - 1, 2), np.nan)
    inv = np.zeros(sums.size)
    for u, (a, b) in enumerate(zip(off[:-1], off[1:])):
        for c, sel in enumerate((voiced[a:b], ~voiced[a:b])):
            n = int(np.sum(sel))
            if n:
                gains[u, c] = math.sqrt(math.exp(math.fsum(sums[a:b][sel]) / (n * float(bins))))
        inv[a:b] = 1.0 / np.where(voiced[a:b], gains[u, 0], gains[u, 1])
    return gains, inv


# ---------------------------------------------------------------------------------------------------------------------
# post-filter
# ---------------------------------------------------------------------------------------------------------------------
def post_filter_ref(x, half_len, nx0, nx1, tilt):
    """magphase.py:2300-2378 on [F x D] rows, float64: ave[b] = mean of x[b - h .. b + h] for nx0 <= b <= nx1 (h =
    half_len[b - nx0]), the boundary averages repeated outside; y = (x - ave) tilt + ave; bins 0 and D - 1 copied.
    -> (y, absterm) with absterm = sum |x| over the window + |x_b| |tilt_b|, the scale of the bound."""
    x = np.asarray(x, dtype=np.float64)
    tilt = np.asarray(tilt, dtype=np.float64)
    F, D = x.shape
    ave = np.zeros((F, D))
    win = np.zeros((F, D))
    for b in range(D):
        bc = min(max(b, nx0), nx1)
        h = int(half_len[bc - nx0])
        assert bc - h >= 0 and bc + h < D
        ave[:, b] = np.mean(x[:, bc - h:bc + h + 1], axis=1)
        win[:, b] = np.sum(np.abs(x[:, bc - h:bc + h + 1]), axis=1)
    y = (x - ave) * tilt[None, :] + ave
    y[:, 0] = x[:, 0]
    y[:, -1] = x[:, -1]
    return y, win + np.abs(x) * np.abs(tilt)[None, :]


def post_filter_bound_h(half_len, nx0, nx1, D):
    b = np.minimum(np.maximum(np.arange(D), nx0), nx1)
    return np.asarray(half_len)[b - nx0]


# ---------------------------------------------------------------------------------------------------------------------
# what the CPU and GPU tests share: operands, tables, shapes
# ---------------------------------------------------------------------------------------------------------------------
def distinct(rs, shape, lo, hi, signed=True):
    """Random float32 values with lo <= |v| < hi, all different: a mis-indexed element shows as an O(1) error."""
    n = int(np.prod(shape))
    v = rs.uniform(lo, hi, n)
    if signed:
        v = v * np.where(rs.randint(0, 2, n) == 1, 1.0, -1.0)
    v = v.astype(np.float32)
    for _ in range(20):   # float32 collisions of a large draw: drawn again (same sign)
        dup = np.ones(n, dtype=bool)
        dup[np.unique(v, return_index=True)[1]] = False
        if not np.any(dup):
            break
        v[dup] = (np.sign(v[dup]) * rs.uniform(lo, hi, int(np.sum(dup)))).astype(np.float32)
    assert np.unique(v).size == n, "operands must be distinct"
    return v.reshape(shape)


# ---- unwarp ---------------------------------------------------------------------------------------------------------
ONEHOT_K = (1, 2, 3, 4, 5, 7, 8, 44, 45, 46, 47, 48, 61, 62, 63, 64)
ONEHOT_H, ONEHOT_F = 513, 70
# (F, H, k_mag, k_phase): every F and H of the issue, k_mag != k_phase, one H = 2049 case
UNWARP_RANDOM = [(1, 40, 64, 1), (31, 64, 1, 64), (32, 65, 60, 45), (33, 513, 24, 16), (127, 1025, 45, 10),
                 (129, 2049, 60, 45), (129, 40, 7, 62)]


def unwarp_operands(F_rows, H, k_mag, k_phase, seed):
    """Coefficient rows with 0.5 <= |a| < 1 (two rows' entries are within a factor of two: the float32 lerp of
    the linear jobs then rounds at the scale of absdot, see test_gpu_compressed_kernels.py), matrices with distinct
    entries scaled so that |A| @ |U| <= 8 -- the exponent range of real log-mel magnitudes."""
    rs = np.random.RandomState(seed)
    out = {}
    for name, K in (("real", k_phase), ("imag", k_phase)):
        out["a_" + name] = distinct(rs, (F_rows, K), 0.5, 1.0)
    # the magnitude rows are neighbours in time: within 5 % of one base row, so that the float32 lerp of two rows'
    # exponentials (the exp job with row tables, fmaf(e1 - e0, t, e0)) rounds at the scale of its result
    base = distinct(rs, (1, k_mag), 0.55, 0.95).astype(np.float64)
    a = (base * (1.0 + 0.05 * rs.uniform(-1, 1, (F_rows, k_mag)))).astype(np.float32)
    assert np.unique(a).size > 0.99 * a.size
    out["a_mag"] = a
    for name, K in (("mag", k_mag), ("phase", k_phase)):
        out["u_" + name] = (distinct(rs, (K, H), 0.05, 1.0) * np.float32(min(1.0, 8.0 / K))).astype(np.float32)
    return out


def onehot_unwarp_operands(K, H=ONEHOT_H, F=ONEHOT_F, seed=0):
    rs = np.random.RandomState(1000 + K + seed)
    A = np.zeros((F, K), dtype=np.float32)
    A[np.arange(F), np.arange(F) % K] = 1.0
    return A, distinct(rs, (K, H), 0.05, 1.0)


def row_tables(n_rows, n_frames, seed, kind="random"):
    """Sorted row0 in [0, n_rows), row1 in {row0, row0 + 1} (<= n_rows - 1), rowt in {0, 1, random}: what the constant ->
    variable rate scan yields.  kind 'identity': row0 = row1 = f, rowt = 0."""
    if kind == "identity":
        r = np.arange(n_frames, dtype=np.int32)
        assert n_frames == n_rows
        return r, r.copy(), np.zeros(n_frames, dtype=np.float32)
    rs = np.random.RandomState(seed)
    row0 = np.sort(rs.randint(0, n_rows, n_frames)).astype(np.int32)
    row1 = np.minimum(row0 + rs.randint(0, 2, n_frames), n_rows - 1).astype(np.int32)
    pick = rs.randint(0, 3, n_frames)
    rowt = np.where(pick == 0, 0.0, np.where(pick == 1, 1.0, rs.uniform(0.05, 0.95, n_frames))).astype(np.float32)
    return row0, row1, rowt


def tile_first_of(row0, n_rows):
    """The plan's table (plans.py, CompressedSynthesisPlan): first frame of every 31-row tile of the coefficient matrix."""
    return np.searchsorted(row0, 31 * np.arange((n_rows + 30) // 31 + 1), side="left").astype(np.int32)


def tiled_row_tables(n_rows, seed):
    """Row tables for the tiled form at n_rows: the second 31-row tile (where there is one) owns no frame, the first owns
    more than 64 (130) when n_rows >= 32 and exactly 65 otherwise, the others three frames per two rows."""
    rs = np.random.RandomState(seed)
    rows = []
    n_tiles = (n_rows + 30) // 31
    for T in range(n_tiles):
        lo, hi = 31 * T, min(31 * T + 31, n_rows)
        if T == 1 and n_tiles > 2:
            continue
        n = (130 if n_rows >= 32 else 65) if T == 0 else int(1.5 * (hi - lo))
        rows.append(np.sort(rs.randint(lo, hi, n)))
    row0 = np.concatenate(rows).astype(np.int32)
    row1 = np.minimum(row0 + rs.randint(0, 2, row0.size), n_rows - 1).astype(np.int32)
    pick = rs.randint(0, 3, row0.size)
    rowt = np.where(pick == 0, 0.0, np.where(pick == 1, 1.0, rs.uniform(0.05, 0.95, row0.size))).astype(np.float32)
    return row0, row1, rowt


TILED_N_ROWS = (1, 31, 32, 62, 63, 100)
PHASE_BINS = (0, 1, 63, 64, 65, 512, 513)   # and H itself


# ---- warp -----------------------------------------------------------------------------------------------------------
WARP_ONEHOT_BINS = (0, 3, 4, 15, 16, 63, 64, 65)   # and Hfull - 1, Hfull, H - 1
# (F, H, mag_dim, phase_dim)
WARP_SHAPES = [(1, 40, 1, 15), (63, 64, 16, 17), (64, 65, 17, 1), (65, 100, 45, 60), (130, 513, 60, 45),
               (65, 2049, 64, 16), (130, 100, 15, 64)]
MAG_LO, MAG_HI = 1.0e-6, 10.0


def warp_onehot_matrix(nout, H, seed):
    """W[i] = e_{k_i}, k_i drawn from the chunk, swizzle and tail edges (every edge bin is used when nout allows)."""
    hfull = H & ~63
    edges = sorted({k for k in WARP_ONEHOT_BINS + (hfull - 1, hfull, H - 1) if 0 <= k < H})
    rs = np.random.RandomState(seed)
    ks = np.asarray(edges)[rs.permutation(len(edges))][:nout] if nout <= len(edges) else \
        np.concatenate((edges, rs.randint(0, H, nout - len(edges))))
    W = np.zeros((nout, H), dtype=np.float32)
    W[np.arange(nout), ks] = 1.0
    return W, ks


def warp_operands(rows, H, seed):
    """mag log-uniform over [1e-6, 10], real / imag uniform in [-1, 1], distinct."""
    rs = np.random.RandomState(seed)
    mag = np.exp(rs.uniform(np.log(MAG_LO * 1.0001), np.log(MAG_HI), (rows, H))).astype(np.float32)
    assert np.unique(mag).size > 0.999 * mag.size
    return mag, distinct(rs, (rows, H), 0.0, 1.0), distinct(rs, (rows, H), 0.0, 1.0)


def warp_matrices(mag_dim, phase_dim, H, seed, scale=None):
    """Dense W with distinct entries.  The phase matrix is scaled so that the mode-1 outputs stay inside the clip
    (|y| <= 2 sum |W| < 0.9): the clip has its own directed rows."""
    rs = np.random.RandomState(seed)
    w_mag = distinct(rs, (mag_dim, H), 0.05, 1.0) * np.float32(1.0 / H)
    w_ph = distinct(rs, (phase_dim, H), 0.05, 1.0) * np.float32((scale or 0.4) / H)
    return w_mag.astype(np.float32), w_ph.astype(np.float32)


def voicing(F, seed, tile=64, dead_tile=None):
    """float32 voicing flags, about a third unvoiced; dead_tile: that whole `tile`-frame tile unvoiced."""
    v = (np.random.RandomState(seed).uniform(0, 1, F) > 0.33).astype(np.float32)
    if F > 1:
        v[0], v[-1] = 1.0, 0.0
    if dead_tile is not None:
        v[tile * dead_tile:tile * (dead_tile + 1)] = 0.0
    return v


PHASE_ROWS_SIZES = [(1, 1), (5, 51), (16, 16), (257, 1)]   # n_frames x phase_dim = 1, 255, 256, 257


# ---- min phase ------------------------------------------------------------------------------------------------------
MIN_PHASE_POLES = [(0.9 * np.exp(0.3j), 0.8 * np.exp(1.1j)), (0.7 * np.exp(2.0j),), (0.85 * np.exp(0.05j), 0.5 * np.exp(2.9j), 0.6)]


def _with_conj(ps):
    out = []
    for p in ps:
        out += [p] if np.imag(p) == 0 else [p, np.conj(p)]
    return out


def min_phase_rows(N, seed=0):
    """-> (mag float32 [rows x H], kinds, closed: {row: phi} for the rows whose minimum phase is known in closed form).
    Flat rows, all-pole envelopes, random spectra over 60 dB, single-bin peaks; about 70 rows."""
    H = N // 2 + 1
    rs = np.random.RandomState(seed + N)
    rows, kinds, closed = [], [], {}
    for g in (1.0, 0.01, 37.5):
        closed[len(rows)] = np.zeros(H)
        rows.append(np.full(H, g))
        kinds.append("flat")
    for i, ps in enumerate(MIN_PHASE_POLES):
        for g in (1.0, 0.05):
            m, phi = allpole_spectrum(_with_conj(ps), N, g)
            closed[len(rows)] = phi
            rows.append(m)
            kinds.append("allpole")
    for k in (0, 1, 7, H // 2, H - 2, H - 1):
        m = np.ones(H)
        m[k] = 500.0
        rows.append(m)
        kinds.append("peak")
    while len(rows) < 70:
        rows.append(10.0 ** rs.uniform(-3.0, 0.0, H))
        kinds.append("random")
    return np.asarray(rows).astype(np.float32), kinds, closed


def min_phase_row_tables(n_rows, seed=0):
    """Frames: the identity over every row, then row0 != row1 at rowt in {0, 1, 0.37}."""
    rs = np.random.RandomState(seed)
    r0 = list(range(n_rows))
    r1 = list(range(n_rows))
    t = [0.0] * n_rows
    for w in (0.0, 1.0, 0.37):
        for _ in range(6):
            a, b = rs.choice(n_rows, 2, replace=False)
            r0.append(int(a))
            r1.append(int(b))
            t.append(w)
    return np.asarray(r0, dtype=np.int32), np.asarray(r1, dtype=np.int32), np.asarray(t, dtype=np.float32)


# ---- noise ----------------------------------------------------------------------------------------------------------
def noise_shapes(N):
    """(L, R) within the transform (L + R + 1 <= N): the type-2 tests' base shapes, the longest frames of the reference's
    domain, and lengths around the 1024-sample staging tile."""
    s = BASE_SHAPES + [(N // 2 - 1, N // 2 - 1), (N // 2, N // 2 - 1)]
    s += [(L, R) for (L, R) in [(511, 511), (511, 512), (512, 512), (1000, 900), (300, 1500)] if L + R + 1 <= N and (L, R) not in s]
    return s


def noise_frame_table(N, n_frames, seed=0):
    """(left, right, wtype, pos, total): every shape with both windows at an even and an odd offset, then small frames."""
    rows = [(L, R, w, p) for (L, R) in noise_shapes(N) for w in (1, 0) for p in (0, 1)]
    assert n_frames >= len(rows)
    rs = np.random.RandomState(seed)
    n_pad = n_frames - len(rows)
    pad = np.stack((rs.randint(2, 71, n_pad), rs.randint(2, 71, n_pad), rs.randint(0, 2, n_pad), rs.randint(0, 2, n_pad)), 1)
    t = np.concatenate((np.asarray(rows, dtype=np.int64).reshape(-1, 4), pad.astype(np.int64)))
    left, right, wtype, parity = (t[:, i].copy() for i in range(4))
    pos, total = layout(left, right, parity)
    return left, right, wtype, pos, total


def noise_signal(n, seed=1):
    """Samples with 0.05 <= |x| < 0.6.  A frame of one effective sample (L, R <= 1) has the flat spectrum |x|: with |x| near 1
    every ln|Ns| is near 0 and the RELATIVE error of sum (ln|Ns|)^2 is unbounded (its condition number is
    2 sum |ln| / sum ln^2); test_compressed_kernels_host.py holds that number below NOISE_COND_MAX for every frame."""
    rs = np.random.RandomState(seed)
    return f32(rs.uniform(0.05, 0.6, n) * np.where(rs.randint(0, 2, n) == 1, 1.0, -1.0))


NOISE_COND_MAX = 8.0


def noise_condition(noise, pos, L, R, wtype, N):
    """d(sum ln^2 |Ns|) / sum ln^2 |Ns| per relative perturbation of the |Ns|: 2 sum |ln|Ns|| / sum ln^2 |Ns|."""
    a = np.log(np.abs(noise_spectrum_ref(noise, pos, L, R, wtype, N)[1:N // 2]))
    return float(2 * np.sum(np.abs(a)) / np.sum(a * a))


NOISE_FRAMES = 150
GAIN_UTT_LENS = (1, 2, 255, 256, 257, 600)
GAIN_PATTERNS = ("voiced", "unvoiced", "alternating")


def gains_case(N, pattern, seed=0):
    """float32 sums as k_noise_stats gives them for N-point frames (about (N/2 - 1) (ln|Ns|)^2, ln|Ns| ~ 1 .. 3),
    the voicing pattern, the ragged utterances."""
    off = np.concatenate(([0], np.cumsum(GAIN_UTT_LENS))).astype(np.int32)
    total = int(off[-1])
    rs = np.random.RandomState(seed + N)
    sums = ((N // 2 - 1) * rs.uniform(1.0, 9.0, total)).astype(np.float32)
    voiced = {"voiced": np.ones(total), "unvoiced": np.zeros(total), "alternating": np.arange(total) & 1}[pattern]
    return sums, voiced.astype(np.int32), off


# ---- post-filter ----------------------------------------------------------------------------------------------------
POST_DIMS = (3, 24, 60, 64, 85, 128, 256)


def post_filter_frames(D):
    rows = 256 // D
    return sorted({1, max(rows - 1, 1), rows, rows + 1, 100})


def post_filter_synth_tables(D, seed=0):
    """half_len / nx0 / nx1 / tilt for a D the reference has no defaults for: a window that touches bin 0 (nx0 - h == 0)
    and one that touches bin D - 1 (nx1 + h == D - 1), random half lengths that stay inside the row in between."""
    rs = np.random.RandomState(seed + D)
    h0, h1 = min(5, (D - 1) // 2), min(3, (D - 1) // 2)
    nx0, nx1 = h0, D - 1 - h1
    if nx0 > nx1:
        nx0 = nx1 = D // 2
        h0 = h1 = min(nx0, D - 1 - nx0)
    n = nx1 - nx0 + 1
    b = nx0 + np.arange(n)
    cap = np.minimum(np.minimum(b, D - 1 - b), 6)
    half = np.minimum(rs.randint(0, 7, n), cap)
    half[0], half[-1] = h0, min(h1, cap[-1]) if n > 1 else h0
    assert np.all(b - half >= 0) and np.all(b + half <= D - 1) and b[0] - half[0] == 0 and b[-1] + half[-1] == D - 1
    return int(nx0), int(nx1), half.astype(np.int32), np.linspace(1.8, 2.0, D).astype(np.float32)


def post_filter_input(F, D, seed=0):
    """Log-mel magnitudes: distinct values in [-12, 2]."""
    # (x - 5 is exact in float32 for |x| < 7 up to the ulp of 8: distinct values stay distinct or collide harmlessly)
    rs = np.random.RandomState(seed + 7 * D + F)
    return distinct(rs, (F, D), 0.0, 7.0) - np.float32(5.0)


# ---- directed cases of the warp and noise tests -------------------------------------------------------------------
def epilogue_case():
    """F 130 x H 100 (one whole chunk and a 36-bin tail), 17 phase outputs: rows that clip at +1 and at -1 by >= 0.1, rows
    inside, unvoiced rows, and the whole second 64-frame tile unvoiced with NaN operand rows."""
    F, H, pd = 130, 100, 17
    rs = np.random.RandomState(4)
    kind = np.arange(F) % 5
    real = distinct(rs, (F, H), 0.0, 0.5)
    real[kind == 0] = rs.uniform(0.85, 0.95, (int(np.sum(kind == 0)), H))
    real[kind == 1] = -rs.uniform(0.85, 0.95, (int(np.sum(kind == 1)), H))
    imag = -np.roll(real, 1, axis=0)   # row f: minus row f - 1 of real (clips at the other end)
    voi = np.ones(F, dtype=np.float32)
    voi[kind == 4] = 0.0
    voi[64:128] = 0.0
    real_dev, imag_dev = real.copy(), imag.copy()
    real_dev[64:128] = np.nan
    imag_dev[64:128] = np.nan
    w_ph = (distinct(rs, (pd, H), 0.6, 1.0, signed=False) / np.float32(H)).astype(np.float32)
    mag = warp_operands(F, H, seed=8)[0]
    w_mag = warp_matrices(5, pd, H, seed=8)[0]
    return F, H, pd, mag, real, imag, real_dev, imag_dev, voi, w_mag, w_ph, (kind, np.roll(kind, 1))


def mode2_case():
    """Filter-bank magnitudes (mode 2), F 65 x H 100 -> 16 bands: exact zeros at (3, 70), (64, 70) and (10, 3); through a
    positive W every sum of those three rows lies far below EXP_FLOOR."""
    F, H, md = 65, 100, 16
    mag, real, imag = warp_operands(F, H, seed=12)
    zero_rows, zero_bin = [3, 64], 70
    mag[zero_rows, zero_bin] = 0.0
    mag[10, 3] = 0.0
    w_fb = (distinct(np.random.RandomState(2), (md, H), 0.05, 1.0, signed=False) / np.float32(H)).astype(np.float32)
    w_ph = warp_matrices(md, 15, H, seed=3)[1]
    return F, H, md, mag, real, imag, zero_rows, zero_bin, w_fb, w_ph, voicing(F, seed=1)


def rows_case(F, n_var, H, seed):
    """Row tables of the variable -> constant rate form, voicing, and the rows in use; with n_var >= 128 no voiced frame
    names a row of the second 64-row tile (it is not computed)."""
    rows = row_tables(n_var, F, seed=seed)
    voi = voicing(F, seed=seed + 1)
    if F == 1:
        voi[:] = 1.0
    if n_var >= 128:
        dead = ((rows[0] >= 64) & (rows[0] < 128)) | ((rows[1] >= 64) & (rows[1] < 128))
        voi[dead] = 0.0
    in_use = np.zeros(n_var, dtype=np.float32)
    in_use[rows[0][voi != 0]] = 1.0
    in_use[rows[1][voi != 0]] = 1.0
    return rows, voi, in_use


def phase_rows_case(F, pd, seed):
    """tmp rows in three classes (inside the clip, above +1.15, below -1.15); a frame interpolates within one class, so every
    output is inside (-0.85, 0.85) or clips by more than 0.1."""
    n_var = 12
    rs = np.random.RandomState(seed)
    cls = np.arange(n_var) % 3
    tmp = []
    for _ in range(2):
        m = distinct(rs, (n_var, pd), 0.05, 0.85)
        m[cls == 1] = rs.uniform(1.15, 1.5, (4, pd))
        m[cls == 2] = -rs.uniform(1.15, 1.5, (4, pd))
        tmp.append(m.astype(np.float32))
    row0 = rs.randint(0, n_var, F).astype(np.int32)
    row1 = ((row0 + 3 * rs.randint(0, 2, F)) % n_var).astype(np.int32)
    pick = rs.randint(0, 3, F)
    rowt = np.where(pick == 0, 0.0, np.where(pick == 1, 1.0, rs.uniform(0.05, 0.95, F))).astype(np.float32)
    voi = (rs.uniform(0, 1, F) > 0.3).astype(np.float32)
    voi[0] = 1.0
    return tmp, row0, row1, rowt, voi


DELTA_AMP = 0.5


def noise_case(N):
    """The frame table, the signal, and two directed frames appended: all zeros (L = R = 50), and one nonzero sample at
    the epoch (a flat spectrum of DELTA_AMP)."""
    left, right, wtype, pos, total = noise_frame_table(N, NOISE_FRAMES)
    x = noise_signal(total)
    x = np.concatenate((x, np.zeros(101), np.zeros(81)))
    left, right = np.append(left, [50, 40]), np.append(right, [50, 40])
    wtype, pos = np.append(wtype, [1, 0]), np.append(pos, [total + 50, total + 101 + 40])
    x[total + 101 + 40] = DELTA_AMP
    return left, right, wtype, pos, x
