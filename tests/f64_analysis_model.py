"""numpy models of the float64 analysis front end (magphase_f64.hip: mpx_analysis_frames_f64, mpx_analysis_frames_f64w,
mpx_analysis_compressed_fused), written from the header's text and the oracle's functions, not from the kernels, with the
geometries, signals and tables that tests/test_f64_analysis_host.py (CPU) and tests/test_gpu_f64_analysis_kernels.py share.

  frame model   lossless_kernels_model.analysis_frame: the oracle's half_windows, np.fft, compute_lossless_feats and
                l1 = sum |w x|; here also sum |x| over the samples that enter the transform (the scale of a weight error).
  fused model   the frame model's float64 rows, then compressed_kernels_model.warp_ref with the fused kernel's prologues
                (magnitudes: mode 0, ln(|X|^2 + 1e-8), or with mag_fbank mode 2, ln|X| with -1e10 at 0 and below the exp
                floor; both phase streams: mode 1 with its mask / clip).  Batches above BLAS_ROWS frames take the same
                prologue and epilogues around a float64 product (see fused_model).
  dft_ld        the direct DFT in longdouble: what the frame model's own transform error is measured against.
"""
import functools

import numpy as np

import compressed_kernels_model as ckm
import lossless_kernels_model as lk
from magphase_amd import hostmath as hm
from oracle import magphase_oracle as orc

LD = np.longdouble
U53 = 2.0 ** -53
FFT_LENS = (1024, 2048, 4096)
ONE_HOT_AT = ("0", "1", "L-1", "L", "L+1", "len-1")
# |np.fft - longdouble DFT| of the frame model's rows at fft_len 1024, in units of 2^-53 ||w x||_1: measured 5.13 on the
# one-hot rows of tests/test_f64_analysis_host.py::test_frame_models_own_transform_error and 2.26 on its noise rows
# (numpy's pocketfft).  The GPU test's bound carries MODEL_ERR_UNITS for it, scaled by log2 N / 10 at the longer transforms
# (the error of an FFT grows with its number of levels).
MODEL_ERR_UNITS = 8.0


def cap_doubles(N):
    """Doubles of a wave's LDS window region: a window of L + R + 2 weights above it takes several passes."""
    return 29 * N // 128


def base_geometries(N):
    """The 117 (L, R) of tests/test_gpu_lossless_kernels.py: L == 0, one- and two-tile frames, truncation at N, L >= N."""
    out = []
    for L in sorted({0, 1, 2, 63, 64, 65, N // 4, N // 2 - 1, N // 2, N // 2 + 1, N - 2, N - 1, N, N + 1, N + 200}):
        Rs = {0, 1, 64, N // 2} | {t - L - 1 for t in (N // 2, N // 2 + 1, N - 1, N, N + 1, N + 300)}
        out += [(L, R) for R in sorted(r for r in Rs if r >= 0)]
    return out


def pass_geometries(N):
    """L + R around one, two and three fills of the window region, each with L == 0, L in between and R == 0."""
    c = cap_doubles(N)
    out = []
    for lr in (c - 3, c - 2, c - 1, c, 2 * c - 2, 2 * c - 1, 2 * c, 3 * c - 1):
        out += [(L, lr - L) for L in (0, lr // 3, lr)]
    return out


def cap_geometries():
    """Half lengths at the edge of the host table (hostmath.HANN_TABLE_CAP): the longer one decides the path."""
    out = []
    for h in (hm.HANN_TABLE_CAP - 1, hm.HANN_TABLE_CAP, hm.HANN_TABLE_CAP + 1):
        out += [(h, 10), (10, h), (h, h)]
    return out


def geometries(N):
    return base_geometries(N) + pass_geometries(N) + cap_geometries()


def window_passes(L, R, N):
    return -(-(L + R + 2) // cap_doubles(N))


def frame_signals(L, R, N, rng):
    """[(kind, samples float32 [len])] of one geometry, as tests/test_gpu_lossless_kernels.py: noise below 0.6, one sample of
    0.75 at offset 0, 1, L - 1, L, L + 1, len - 1 (a sample two names mean is taken once, under the first), DC, the
    alternation, zeros."""
    n = lk.frame_len(L, R, N)
    sigs = [("noise", rng.uniform(-0.6, 0.6, n))]
    seen = set()
    for name, k in zip(ONE_HOT_AT, (0, 1, L - 1, L, L + 1, n - 1)):
        if 0 <= k < n and k not in seen:
            seen.add(k)
            x = np.zeros(n)
            x[k] = 0.75
            sigs.append(("onehot:" + name, x))
    sigs += [("dc", np.full(n, 0.5)), ("alt", np.where(np.arange(n) % 2, -1.0, 1.0)), ("zero", np.zeros(n))]
    return [(kind, x.astype(np.float32)) for kind, x in sigs]


def layout_frames(frames):
    """[(L, R, samples)] -> (sig float32, pos int64, left int32, right int32): every frame in a segment of its own, NaN in
    between and in front."""
    segs, pos, left, right = [np.full(7, np.nan, np.float32)], [], [], []
    at = 7
    for L, R, x in frames:
        pos.append(at + L), left.append(L), right.append(R)
        segs += [x, np.full(5, np.nan, np.float32)]
        at += x.size + 5
    return np.concatenate(segs), np.array(pos, np.int64), np.array(left, np.int32), np.array(right, np.int32)


def model_rows(sig, pos, left, right, N):
    """-> (mag, real, imag [F x N/2 + 1], l1 [F], sum |x| [F]) of the frame model, float64."""
    sig64 = np.asarray(sig, dtype=np.float64)
    rows = [lk.analysis_frame(sig64, p, L, R, N) for p, L, R in zip(pos, left, right)]
    sx = np.array([np.sum(np.abs(sig64[int(p) - int(L):int(p) - int(L) + lk.frame_len(L, R, N)]))
                   for p, L, R in zip(pos, left, right)])
    return tuple(np.array([r[i] for r in rows]) for i in range(4)) + (sx,)


@functools.lru_cache(maxsize=None)
def analysis_case(N):
    """Every geometry x every signal of fft_len N: the tables of ONE launch and the model's rows (computed once, shared)."""
    rng = np.random.default_rng(N + 64)
    frames, kinds = [], []
    for L, R in geometries(N):
        for kind, x in frame_signals(L, R, N, rng):
            frames.append((L, R, x))
            kinds.append(kind)
    sig, pos, left, right = layout_frames(frames)
    return dict(sig=sig, pos=pos, left=left, right=right, kinds=np.array(kinds), model=model_rows(sig, pos, left, right, N))


def count_case(F, seed):
    """F short frames (L, R <= 40; every 7th L == 0, every 11th R == 0) at random places of one signal, overlapping freely;
    samples no frame covers are NaN."""
    rng = np.random.default_rng(seed)
    left = rng.integers(1, 41, F).astype(np.int32)
    right = rng.integers(1, 41, F).astype(np.int32)
    left[::7], right[::11] = 0, 0
    n = 4096
    pos = rng.integers(50, n - 50, F).astype(np.int64)
    sig = rng.uniform(-0.6, 0.6, n).astype(np.float32)
    cover = np.zeros(n, dtype=bool)
    for p, L, R in zip(pos, left, right):
        cover[p - L:p + R + 1] = True
    sig[~cover] = np.nan
    return sig, pos, left, right


@functools.lru_cache(maxsize=4)
def count_model(N, F):
    """count_case(F, 1000 + F) and the frame model's rows at fft_len N (computed once; both window paths share them)."""
    tabs = count_case(F, 1000 + F)
    return tabs, model_rows(*tabs, N)


def analytic_frames(left, right, table):
    """Frames whose window is evaluated on the device: every frame without the table, a half above its cap with it."""
    left, right = np.asarray(left), np.asarray(right)
    if not table:
        return np.ones(left.shape, dtype=bool)
    return (left > hm.HANN_TABLE_CAP) | (right > hm.HANN_TABLE_CAP)


def dft_ld(row):
    """Bins 0 .. N/2 of the DFT of a real row by longdouble cosine / sine matrices, the angles reduced exactly."""
    row = np.asarray(row).astype(LD)
    N = row.size
    idx = np.outer(np.arange(N // 2 + 1), np.arange(N)) % N
    ang = idx.astype(LD) * (2 * np.arccos(LD(-1.0))) / N
    return np.cos(ang) @ row, -(np.sin(ang) @ row)


def transform_input(sig, pos, L, R, N):
    """The windowed, padded, rotated row that the frame model hands to np.fft (float64)."""
    n = lk.frame_len(L, R, N)
    seg = np.asarray(sig[pos - L:pos - L + n], dtype=np.float64) * orc.half_windows(L, R)[:n]
    row = np.zeros(N)
    row[:n] = seg
    s = L if L < N else 0
    return np.concatenate((row[s:], row[:s]))


# ------------------------------------------------------------------------------------------------------ fused analysis
FUSED_DIMS = ((1, 1), (3, 1), (16, 16), (17, 17), (33, 32), (60, 10), (60, 45), (64, 48))
FUSED_COUNTS = (1, 7, 8, 9, 16, 17)


def fused_geometries(N):
    """42 geometries of the families of geometries(N) (not all of them members of it): several passes, two tiles, truncation, L == 0, L >= N and halves above the table's cap."""
    c, cap = cap_doubles(N), hm.HANN_TABLE_CAP
    g = [(0, 0), (0, 1), (1, 0), (0, 64), (2, 1), (63, 64), (64, 0), (65, 64), (N // 4, N // 4), (N // 4, 0),
         (0, c - 2), (c - 2, 0), (0, c - 1), (c // 3, c - 1 - c // 3), (c, 0), (0, 2 * c - 2), (2 * c - 1, 0),
         ((2 * c) // 3, 2 * c - (2 * c) // 3), (0, 3 * c - 1), (c, 2 * c - 1),
         (N // 2 - 1, 0), (N // 2, 64), (N // 2 + 1, N // 2), (0, N // 2), (1, N // 2 - 1), (N // 4, N // 2),
         (N - 2, 1), (N - 1, 0), (N - 1, 64), (N, 0), (N, 64), (N + 1, 1), (N + 200, 64), (N + 200, N // 2),
         (N // 2, N // 2 + 300), (64, N + 235), (0, N + 299),
         (cap - 1, 10), (10, cap), (cap + 1, 10), (10, cap + 1), (cap + 1, cap + 1)]
    return g


BLAS_ROWS = 256      # batches above it: the product of fused_model in float64 (BLAS) instead of longdouble


def fused_model(rows, w_mag, w_ph, voi, mag_fbank):
    """-> ((mag, real, imag) [F x dim], (absdot_mag, absdot_real, absdot_imag), (absdot1_...)) from the frame model's rows
    (mag, real, imag float64 [F x H]); absdot = |pre(x)| @ |W|^T, absdot1 = max(|pre(x)|, 1) @ |W|^T.  Up to BLAS_ROWS frames
    the values and absdot are compressed_kernels_model.warp_ref's (longdouble).  A larger batch takes the same prologue
    (warp_prologue_ref, longdouble) and epilogues (mask_clip, the -1e10 floor) around a float64 product: a longdouble
    product of 2 051 x 2 049 x 150 takes 5 s, and float64 adds at most H 2^-53 = 2.3e-13 of absdot, 1e-7 of the bound the GPU
    test holds (tests/test_f64_analysis_host.py compares the two forms)."""
    mag, real, imag = rows[:3]
    jobs = ((mag, w_mag, 2 if mag_fbank else 0), (real, w_ph, 1), (imag, w_ph, 1))
    ys, ads, ad1s = [], [], []
    for x, w, mode in jobs:
        p = ckm.warp_prologue_ref(mode, np.asarray(x).astype(LD))
        aw = np.abs(np.asarray(w, dtype=np.float64)).T
        ad1s.append(np.maximum(np.abs(p), 1).astype(np.float64) @ aw)
        if len(x) <= BLAS_ROWS:
            y, ad = ckm.warp_ref(x, w, mode, voi=voi if mode == 1 else None)
        else:
            y = (p.astype(np.float64) @ np.asarray(w, dtype=np.float64).T).astype(LD)
            ad = np.abs(p).astype(np.float64) @ aw
            if mode == 1:
                y = ckm.mask_clip(y, voi)
            elif mode == 2:
                y = np.where(y < LD(ckm.EXP_FLOOR), LD(ckm.MAGIC), y)
        ys.append(y)
        ads.append(ad)
    return tuple(ys), tuple(ads), tuple(ad1s)
