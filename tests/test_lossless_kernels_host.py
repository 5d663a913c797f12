"""CPU: the numpy models of tests/lossless_kernels_model.py against oracle.magphase_oracle -- the oracle stays the authority,
the models only restate it per frame / per row so that the GPU tests can choose every argument themselves -- and every
argument check of the six C entries (they return before any launch, so no device is needed)."""
import ctypes
import os
import warnings

import numpy as np
import pytest

import lossless_kernels_model as lk
from _tol import within
from magphase_amd import _lib
from magphase_amd import hostmath as hm
from oracle import magphase_oracle as orc


# ------------------------------------------------------------------------------------------------ models vs the oracle
def test_analysis_frame_equals_the_oracle_row_for_row(golden_dir):
    g = np.load(os.path.join(golden_dir, "g1_index.npz"))
    rng = np.random.RandomState(5)
    seen_l0 = seen_long = False
    for i in range(int(g["ncases"])):
        n = int(g["c%d_n" % i])
        fs = 16000 if i == 1 else 48000
        N = orc.define_fft_len(fs)
        x = rng.uniform(-0.5, 0.5, n)
        pm_sec = g["c%d_pm" % i] / fs
        voi = np.ones(len(pm_sec))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            o = orc.analysis_lossless_from_epochs(x, fs, pm_sec, voi)
        pm_c, _ = orc.clean_epochs(pm_sec, voi, check_len_smpls=n, fs=fs)
        pm_plus, left, right, lens = orc.frame_bounds(pm_c * fs, n)
        assert np.array_equal(left, o[5]) and o[0].shape == (left.size, N // 2 + 1)
        seen_l0 |= bool(np.any(left == 0))
        seen_long |= bool(np.any(lens > N))
        for f in range(left.size):
            mag, real, imag, l1 = lk.analysis_frame(x, pm_plus[f + 1], left[f], right[f], N)
            X, Xo = mag * (real + 1j * imag), o[0][f] * (o[1][f] + 1j * o[2][f])
            within(np.max(np.abs(X - Xo)) / max(l1, 1e-300), 1e-13, "LK_HOST_ANA_MODEL_VS_ORACLE")
            within(np.max(np.abs(mag - o[0][f])) / max(l1, 1e-300), 1e-13, "LK_HOST_ANA_MODEL_VS_ORACLE")
            assert np.array_equal(mag == 0, o[0][f] == 0)
    assert seen_l0 and seen_long       # the golden cases hold L == 0 and frames longer than fft_len


def test_analysis_frame_reads_its_extent_only_and_honours_the_zero_rule():
    N = 1024
    for L, R in ((0, 0), (0, 5), (5, 0), (N + 200, 64), (N // 2, N // 2 + 300)):
        n = lk.frame_len(L, R, N)
        sig = np.full(L + R + 50, np.nan)
        sig[7:7 + n] = np.random.default_rng(L + R).uniform(-0.6, 0.6, n)
        mag, real, imag, l1 = lk.analysis_frame(sig, 7 + L, L, R, N)
        assert np.all(np.isfinite(mag)) and np.all(np.isfinite(real)) and l1 > 0
        sig[7:7 + n] = 0.0
        mag, real, imag, l1 = lk.analysis_frame(sig, 7 + L, L, R, N)
        assert not mag.any() and not real.any() and not imag.any() and l1 == 0


@pytest.mark.parametrize("first_f0", (200.0, 0.0, 20.0), ids=("voiced", "unvoiced", "first_epoch_beyond_half_N"))
def test_synthesis_frame_then_gather_equals_the_oracle(first_f0):
    fs, N, F = 16000, 1024, 40
    rng = np.random.default_rng(int(first_f0))
    H = N // 2 + 1
    mag = np.exp(0.5 * rng.normal(size=(F, H)))
    real, imag = rng.normal(size=(F, H)), rng.normal(size=(F, H))
    real[3, 5:9] = imag[3, 5:9] = 0.0
    v_f0 = rng.uniform(80.0, 400.0, F)
    v_f0[10:14] = 0.0
    v_f0[0] = first_f0
    ref = orc.synthesis_from_lossless(mag, real, imag, v_f0, fs)
    v_pm = orc.shift_to_pm(orc.f0_to_shift(v_f0, fs))
    pm_rel, start, out_len = hm.ola_plan(v_pm, N)
    assert (first_f0 == 20.0) == (N // 2 - int(v_pm[0]) < 0) and out_len == len(ref)
    frames = lk.synthesis_frame(mag, real, imag, N)
    out = lk.ola_gather(frames, [0, F], pm_rel, [start], [0, out_len], N, dtype=np.float64)
    # (a negative slice start keeps the buffer's last pm_0 - N/2 samples, which no frame reaches: the oracle returns zeros)
    assert bool(ref.any()) == (first_f0 != 20.0) and out.shape == ref.shape
    within(np.max(np.abs(out - ref)) / np.max(np.abs(frames)), 1e-13, "LK_HOST_SYN_MODEL_VS_ORACLE")
    within(np.max(np.abs(frames), axis=1).max() / lk.synthesis_bound_term(mag, N).max(), 1.0, "LK_HOST_SYN_TERM_BOUNDS_FRAME")


def test_float32_gather_is_the_sequential_sum():
    N = 1024
    rng = np.random.default_rng(1)
    frames = rng.normal(size=(5, N)).astype(np.float32)
    pm_rel = np.array([0, 3, 3, 900, 2500])
    out = lk.ola_gather(frames, [0, 5], pm_rel, [-4], [0, 3000], N)
    assert out.dtype == np.float32
    for t in (0, 3, 4, 7, 500, 1023 + 4, 1027 + 4, 2000, 2999):
        acc = np.float32(0.0)
        for i in range(5):
            off = t - 4 - pm_rel[i]
            if 0 <= off < N:
                acc = np.float32(acc + frames[i, off])
        assert out[t] == acc, t
    assert out[2000] == 0.0            # the gap between frames 3 and 4


def test_rows_lerp_equals_the_oracles_two_interpolations():
    rng = np.random.default_rng(2)
    fs, rate = 16000, 5.0
    # constant -> variable rate
    data = rng.normal(size=(50, 7))
    step = fs * rate / 1000
    locs = np.sort(rng.uniform(step, 50 * step, 120))
    locs[0], locs[-1] = step, 50 * step
    lo, hi, t, _ = hm.const_to_variable_rows(np.ones(50, dtype=bool), locs, rate, fs)
    y, _ = lk.rows_lerp(data, lo, hi, t)
    ref = orc.interp_from_const_to_variable_rate(data, locs, rate, fs)
    within(np.max(np.abs(y - ref)), 1e-13, "LK_HOST_LERP_MODEL_VS_ORACLE")
    # variable -> constant rate, first epoch above and at 0
    for first in (37.0, 0.0):
        pm = np.concatenate(([first], first + np.cumsum(rng.integers(40, 200, 60)))).astype(np.float64)
        data = rng.normal(size=(pm.size, 5))
        lo, hi, t = hm.var_to_const_rate_table(pm, rate, fs)
        y, _ = lk.rows_lerp(data, lo, hi, t)
        ref = orc.interp_from_variable_to_const_frm_rate(data, pm, rate, fs)
        within(np.max(np.abs(y - ref)), 1e-13, "LK_HOST_LERP_MODEL_VS_ORACLE")


def hand_ranges():
    """(ranges int32 [9 x 4], n_frames): a only, b only, a and b meeting in one frame, a and b apart with a gap, neither,
    300 frames into one row, an empty range given as a1 < a0, both ranges the same frames, neither again."""
    r = np.array([[0, 3, 0, 0], [0, 0, 3, 5], [5, 8, 7, 9], [9, 11, 14, 16], [16, 16, 16, 16], [20, 320, 16, 20],
                  [7, 3, 320, 322], [322, 325, 322, 325], [0, 0, 0, 0]], dtype=np.int32)
    return r, 325


def test_rows_lerp_adjoint_is_the_transpose_of_rows_lerp():
    rng = np.random.default_rng(3)
    # tables of a 2x time-stretch: every constant-rate row feeds about four frames
    fs, rate, n_rows = 16000, 5.0, 30
    step = fs * rate / 1000
    locs = np.linspace(step, n_rows * step, 2 * n_rows + 1)
    lo, hi, t, _ = hm.const_to_variable_rows(np.ones(n_rows, dtype=bool), locs, rate, fs)
    t = t.astype(np.float32).astype(np.float64)
    x, g = rng.normal(size=(n_rows, 6)), rng.normal(size=(lo.size, 6))
    y, _ = lk.rows_lerp(x, lo, hi, t)
    back, mag, count = lk.rows_lerp_adjoint(g, hm.lerp_adjoint_table(lo, hi, t, n_rows), t, n_rows)
    within(abs(np.sum(y * g) - np.sum(x * back)) / np.sum(np.abs(y * g)), 1e-12, "LK_HOST_ADJOINT_DUALITY")
    assert count.sum() >= lo.size and np.all(mag >= np.abs(back) - 1e-12)
    # by hand, row0 == row1 frames included: the forward of the same table
    row0 = np.array([0, 0, 1, 1, 1, 2, 2, 4, 4, 4])
    row1 = np.array([0, 1, 1, 1, 2, 2, 4, 4, 4, 4])
    t = np.array([0.5, 0.25, 0.75, 0.0, 1.0, 0.125, 0.5, 0.3, 0.0, 1.0]).astype(np.float32).astype(np.float64)
    x, g = rng.normal(size=(5, 4)), rng.normal(size=(10, 4))
    y, _ = lk.rows_lerp(x, row0, row1, t)
    ranges = hm.lerp_adjoint_table(row0, row1, t, 5)
    assert np.array_equal(ranges[3], [7, 7, 6, 6])                       # a row no frame reads
    back, _, count = lk.rows_lerp_adjoint(g, ranges, t, 5)
    within(abs(np.sum(y * g) - np.sum(x * back)) / np.sum(np.abs(y * g)), 1e-12, "LK_HOST_ADJOINT_DUALITY")
    assert not back[3].any() and count[3] == 0 and count[0] == 2 and count[1] == 4
    r, nf = hand_ranges()
    back, _, count = lk.rows_lerp_adjoint(np.ones((nf, 1)), r, np.full(nf, 0.25), len(r))
    assert np.array_equal(count, [3, 2, 4, 4, 0, 304, 2, 3, 0])
    assert np.allclose(back[:, 0], [2.25, 0.5, 0.75 * 2 + 1 + 0.25, 2 * 0.75 + 2 * 0.25, 0, 300 * 0.75 + 1, 0.5, 3, 0])


def test_fixup_model_and_run_record():
    assert lk.OLA_RUN_DTYPE.itemsize == 56 and lk.OLA_RUN_DTYPE == hm.OLA_RUN_DTYPE
    runs = np.zeros(3, dtype=lk.OLA_RUN_DTYPE)
    runs["fix_lo"], runs["fix_hi"] = [1, 70, 5], [4, 70, 2000]
    runs["out_base"], runs["strip_off"] = [-1, 50, 100], [0, 10, 20]
    pcm, strips = np.arange(3000, dtype=np.float32), np.ones(3000, dtype=np.float32)
    out = lk.ola_fixup(pcm, runs, strips)
    assert np.array_equal(np.flatnonzero(out != pcm), np.r_[0:3, 105:2100])
    assert lk.fixup_width(runs) == 2000 and np.array_equal(lk.ola_fixup(pcm, runs, strips, 2000), out)
    assert np.array_equal(np.flatnonzero(lk.ola_fixup(pcm, runs, strips, 1024) != pcm), np.r_[0:3, 105:1124])
    assert np.array_equal(lk.ola_fixup(pcm, runs, strips, 0), pcm)


# ------------------------------------------------------------------------------------------------ argument checks
def test_c_entries_argument_errors_without_gpu():
    lib = _lib.load()
    one = ctypes.c_void_p(8)   # a non-null pointer that is never followed: every call below returns before a launch

    def failed(rc, name, word):
        err = lib.mpx_last_error()
        assert rc == -1 and name in err and word in err, (rc, name, word, err)

    def ana(N=1024, n=3, ld=513, p=one):
        return lib.mpx_analysis_frames(None, N, p, one, one, one, one, n, one, one, one, ld)

    def syn(N=1024, n=3, ld=513, p=one):
        return lib.mpx_synthesis_lossless_frames(None, N, one, one, one, p, n, one, ld)

    for fn, name in ((ana, b"mpx_analysis_frames"), (syn, b"mpx_synthesis_lossless_frames")):
        failed(fn(N=1000), name, b"fft_len")
        failed(fn(n=-1), name, b"negative")
        failed(fn(ld=512), name, b"ld <")
        failed(fn(p=None), name, b"null")
        assert fn(n=0) == 0 and fn(n=0, p=None) == 0           # no frame: no launch, no error
    failed(ana(N=2048, ld=1024), b"mpx_analysis_frames", b"ld <")

    def gather(N=1024, n_utts=2, max_len=100, p=one):
        return lib.mpx_ola_gather(None, N, one, n_utts, one, p, one, one, max_len, one)

    failed(gather(N=512), b"mpx_ola_gather", b"fft_len")
    failed(gather(n_utts=-1), b"mpx_ola_gather", b"negative")
    failed(gather(max_len=-1), b"mpx_ola_gather", b"negative")
    failed(gather(p=None), b"mpx_ola_gather", b"null")
    failed(gather(n_utts=65536), b"mpx_ola_gather", b"65535")
    assert gather(n_utts=0) == 0 and gather(max_len=0, p=None) == 0

    def fix(N=1024, n=2, p=one):
        return lib.mpx_ola_fixup(None, N, p, n, one, one)

    def fixw(N=1024, n=2, p=one, w=64):
        return lib.mpx_ola_fixup_width(None, N, p, n, one, one, w)

    for fn, name in ((fix, b"mpx_ola_fixup"), (fixw, b"mpx_ola_fixup_width")):
        failed(fn(N=4097), name, b"fft_len")
        failed(fn(n=-1), name, b"negative")
        failed(fn(p=None), name, b"null")
        failed(fn(n=2 ** 30), name, b"too many")
        assert fn(n=0, p=None) == 0
    failed(fixw(w=-1), b"mpx_ola_fixup_width", b"width")
    failed(fixw(w=1024 + 128), b"mpx_ola_fixup_width", b"width")
    failed(fixw(N=4096, w=4096 + 128), b"mpx_ola_fixup_width", b"width")
    assert fixw(w=0, p=None) == 0                              # nothing to fix: no launch

    def lerp(H=5, ld_s=5, ld_d=5, n=3, p=one):
        return lib.mpx_rows_lerp(None, H, one, one, one, ld_s, one, p, one, n, one, one, one, ld_d)

    failed(lerp(H=0), b"mpx_rows_lerp", b"n_bins")
    failed(lerp(n=-1), b"mpx_rows_lerp", b"n_out")
    failed(lerp(ld_s=4), b"mpx_rows_lerp", b"pitch")
    failed(lerp(ld_d=4), b"mpx_rows_lerp", b"pitch")
    failed(lerp(p=None), b"mpx_rows_lerp", b"null")
    failed(lerp(n=4 * 2147483647 + 1), b"mpx_rows_lerp", b"too many")
    assert lerp(n=0, p=None) == 0

    def adj(H=5, ld_s=5, ld_d=5, n=3, rng=one, src=(one, one, one), dst=(one, one, one)):
        return lib.mpx_rows_lerp_adjoint(None, H, src[0], src[1], src[2], ld_s, rng, one, n, dst[0], dst[1], dst[2], ld_d)

    name = b"mpx_rows_lerp_adjoint"
    failed(adj(H=0), name, b"n_bins")
    failed(adj(n=-1), name, b"n_rows")
    failed(adj(ld_s=4), name, b"pitch")
    failed(adj(ld_d=4), name, b"pitch")
    failed(adj(rng=None), name, b"null")
    for s in range(3):                                         # a stream asked for without its source
        src = [one, one, one]
        src[s] = None
        failed(adj(src=tuple(src)), name, b"null")
        dst = [None, None, None]
        dst[s] = one
        assert adj(src=tuple(src), dst=(None, None, None)) == 0
        failed(adj(src=tuple(src), dst=tuple(dst)), name, b"null")
    failed(adj(n=4 * 2147483647 + 1), name, b"too many")
    assert adj(n=0, rng=None) == 0 and adj(dst=(None, None, None), rng=None) == 0
