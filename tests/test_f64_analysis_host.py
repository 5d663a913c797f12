"""CPU: the models of tests/f64_analysis_model.py -- the frame model against the oracle, its own transform error against a
longdouble DFT (the figure that enters the bound of tests/test_gpu_f64_analysis_kernels.py), the conditions under which
that file compares real / imag alone on EVERY bin of the noise and one-hot rows -- and every argument check of
mpx_analysis_frames_f64w and mpx_analysis_compressed_fused (they return before any launch, so no device is needed)."""
import ctypes
import os
import warnings

import numpy as np
import pytest

import compressed_kernels_model as ckm
import f64_analysis_model as fm
import lossless_kernels_model as lk
from _tol import within
from magphase_amd import _lib
from magphase_amd import hostmath as hm
from oracle import magphase_oracle as orc


def test_frame_model_equals_the_oracle_row_for_row(golden_dir):
    g = np.load(os.path.join(golden_dir, "g1_index.npz"))
    rng = np.random.RandomState(7)
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
        mag, real, imag, l1, sx = fm.model_rows(x, pm_plus[1:1 + left.size], left, right, N)
        X, Xo = mag * (real + 1j * imag), o[0] * (o[1] + 1j * o[2])
        scale = np.maximum(l1, 1e-300)[:, None]
        within(np.max(np.abs(X - Xo) / scale), 1e-13, "F64_HOST_MODEL_VS_ORACLE")
        within(np.max(np.abs(mag - o[0]) / scale), 1e-13, "F64_HOST_MODEL_VS_ORACLE")
        assert np.array_equal(mag == 0, o[0] == 0) and np.all(sx >= l1)


def test_frame_models_own_transform_error():
    """np.fft against the direct longdouble DFT at fft_len 1024 on noise rows (short, two-tile, truncated, L >= N) and one-hot
    rows, in units of 2^-53 l1."""
    N, rng = 1024, np.random.default_rng(11)
    worst = {"noise": 0.0, "onehot": 0.0}
    for L, R in ((0, 0), (3, 5), (64, 63), (N // 4, N // 4), (N // 2, N // 2 - 1), (N // 2 + 1, N // 2), (N + 200, 64)):
        n = lk.frame_len(L, R, N)
        rows = [("noise", rng.uniform(-0.6, 0.6, n))]
        for k in (1, n // 2, n - 2):
            if 0 <= k < n:
                x = np.zeros(n)
                x[k] = 0.75
                rows.append(("onehot", x))
        for kind, x in rows:
            row = fm.transform_input(x.astype(np.float32), L, L, R, N)
            l1 = np.sum(np.abs(row))
            if l1 == 0:
                continue
            re, im = fm.dft_ld(row)
            X = np.fft.fft(row)[:N // 2 + 1]
            err = float(np.max(np.sqrt((X.real - re) ** 2 + (X.imag - im) ** 2)) / (fm.U53 * l1))
            worst[kind] = max(worst[kind], err)
    print("frame model against the longdouble DFT, N = 1024: noise rows %.2f, one-hot rows %.2f x 2^-53 l1"
          % (worst["noise"], worst["onehot"]))
    if np.finfo(np.longdouble).eps < 2.0 ** -60:       # (a platform whose longdouble is float64 measures nothing)
        within(max(worst.values()), fm.MODEL_ERR_UNITS, "F64_HOST_MODEL_TRANSFORM_ERROR_UNITS")


@pytest.mark.parametrize("N", fm.FFT_LENS)
def test_noise_and_one_hot_rows_have_no_bin_below_the_phasor_threshold(N):
    """tests/test_gpu_f64_analysis_kernels.py compares real / imag alone where |X_model| >= 2^-20 l1 and asserts that this
    is EVERY bin of the noise and one-hot rows: so it must be, on the model alone.  (One-hot rows: every bin is l1.)"""
    c = fm.analysis_case(N)
    mag, _, _, l1, sx = c["model"]
    assert len(fm.base_geometries(N)) == 117 and len(fm.geometries(N)) == 117 + 24 + 9
    live = l1 > 0
    noise = (c["kinds"] == "noise")
    assert noise.sum() == len(fm.geometries(N)) and np.all(live[noise])
    smallest = float(np.min(mag[noise] / l1[noise, None]))
    print("N = %d: smallest noise bin 2^%.1f of l1" % (N, np.log2(smallest)))
    assert smallest >= 2.0 ** -20
    hot = np.array([k.startswith("onehot") for k in c["kinds"]]) & live
    assert hot.sum() > 300
    within(np.max(np.abs(mag[hot] / l1[hot, None] - 1.0)), 1e-12, "F64_HOST_ONE_HOT_MODEL_IS_FLAT")
    # a one-hot row whose model is exactly zero: the sample lies under a window weight of exactly 0
    dead = np.array([k.startswith("onehot") for k in c["kinds"]]) & ~live
    assert dead.sum() > 50 and not mag[dead].any() and np.all(sx[dead] == 0.75)
    zero = c["kinds"] == "zero"
    assert not mag[zero].any() and not sx[zero].any()


def test_geometries_reach_every_path():
    for N in fm.FFT_LENS:
        g = fm.geometries(N)
        passes = {fm.window_passes(L, R, N) for L, R in g}
        assert {1, 2, 3} <= passes
        c = fm.cap_doubles(N)
        assert (0, c - 2) in g and fm.window_passes(0, c - 2, N) == 1 and fm.window_passes(0, c - 1, N) == 2
        assert fm.window_passes(0, 2 * c - 2, N) == 2 and fm.window_passes(2 * c - 1, 0, N) == 3
        assert any(lk.frame_len(L, R, N) > N // 2 for L, R in g) and any(L + R + 1 > N for L, R in g)
        assert any(L >= N for L, R in g) and any(L == 0 for L, R in g)
        tab = fm.analytic_frames([a for a, _ in g], [b for _, b in g], True)
        assert tab.sum() >= (3 if N == 1024 else 5) and (~tab).sum() >= 80
    for N in (2048, 4096):
        g = fm.fused_geometries(N)
        assert 35 <= len(g) <= 45 and len(set(g)) == len(g)
        assert any(fm.window_passes(L, R, N) >= 3 for L, R in g) and any(L + R + 1 > N for L, R in g)
        assert any(L >= N for L, R in g) and any(L == 0 for L, R in g) and any(max(L, R) > hm.HANN_TABLE_CAP for L, R in g)
        assert any(N // 2 < L + R + 1 <= N for L, R in g)


def test_fused_model_masks_and_floors():
    N, H = 2048, 1025
    rng = np.random.default_rng(3)
    sig, pos, left, right = fm.layout_frames([(5, 6, rng.uniform(-0.6, 0.6, 12).astype(np.float32)),
                                              (4, 4, np.zeros(9, np.float32)),
                                              (0, 3, rng.uniform(-0.6, 0.6, 4).astype(np.float32))])
    rows = fm.model_rows(sig, pos, left, right, N)
    w_mag, w_ph = ckm.warp_matrices(3, 2, H, seed=5)
    voi = np.array([1.0, 1.0, 0.0], np.float32)
    (ym, yr, yi), absdot, absdot1 = fm.fused_model(rows, w_mag, w_ph, voi, 0)
    assert np.allclose(np.asarray(ym[1], float), np.log(1e-8) * w_mag.sum(axis=1).astype(float), rtol=1e-6)
    assert not yr[2].any() and not yi[2].any() and yr[0].any()
    assert all(np.all(b >= np.asarray(a, dtype=np.float64) * (1 - 1e-12)) for a, b in zip(absdot, absdot1))
    (ym2, _, _), _, _ = fm.fused_model(rows, np.abs(w_mag), w_ph, voi, 1)
    assert np.all(ym2[1] == -1.0e10) and np.all(ym2[0] > -745.0)


def test_fused_model_of_a_large_batch_equals_warp_ref(monkeypatch):
    """Above BLAS_ROWS frames the fused model's product runs in float64: the same values to 1e-12 of |pre| @ |W|^T, the same
    masks and floors."""
    N, H = 2048, 1025
    tabs = fm.count_case(40, 3)
    frames = fm.layout_frames([(4, 4, np.zeros(9, np.float32))])
    rows = tuple(np.concatenate((a, b)) for a, b in zip(fm.model_rows(*tabs, N), fm.model_rows(*frames, N)))
    w_mag, w_ph = ckm.warp_matrices(17, 33, H, seed=6)
    voi = ckm.voicing(41, seed=2)
    for fbank in (0, 1):
        wm = np.abs(w_mag) if fbank else w_mag
        ref = fm.fused_model(rows, wm, w_ph, voi, fbank)
        monkeypatch.setattr(fm, "BLAS_ROWS", 8)
        got = fm.fused_model(rows, wm, w_ph, voi, fbank)
        monkeypatch.undo()
        for k in range(3):
            floor = np.asarray(ref[0][k] == fm.LD(ckm.MAGIC))
            assert np.array_equal(np.asarray(got[0][k] == fm.LD(ckm.MAGIC)), floor) and floor.any() == (k == 0 and fbank == 1)
            assert np.array_equal(np.asarray(got[0][k] == 0), np.asarray(ref[0][k] == 0))
            err = np.abs(got[0][k] - ref[0][k])[~floor] / np.asarray(ref[1][k])[~floor]
            within(float(np.max(err)), 1e-12, "F64_HOST_FUSED_MODEL_BLAS_VS_LONGDOUBLE")
            within(float(np.max(np.abs(got[1][k] / ref[1][k] - 1))), 1e-12, "F64_HOST_FUSED_MODEL_BLAS_VS_LONGDOUBLE")


@pytest.mark.parametrize("N", fm.FFT_LENS)
def test_short_noise_frames_have_no_bin_below_the_phasor_threshold(N):
    """The frame-count and queue cases of the GPU test are noise rows too: 1, 7, 8, 9 frames and 8 x 256 x 2 + 3 (the
    MI355X's 256 CUs; the GPU test asserts the share on the device's own count as well)."""
    for F in (1, 7, 8, 9, 8 * 256 * 2 + 3, 8 * 256 + 3):
        _, (mag, _, _, l1, _) = fm.count_model(N, F)
        assert np.all(l1 > 0) and float(np.min(mag / l1[:, None])) >= 2.0 ** -20


# ------------------------------------------------------------------------------------------------ argument checks
def test_c_entries_argument_errors_without_gpu():
    lib = _lib.load()
    one = ctypes.c_void_p(8)   # a non-null pointer that is never followed: every call below returns before a launch

    def failed(rc, name, word):
        err = lib.mpx_last_error()
        assert rc == -1 and name in err and word in err, (rc, name, word, err)

    def ana(N=1024, n=3, ld=513, p=one, tab=one, cap=5):
        return lib.mpx_analysis_frames_f64w(None, N, p, one, one, one, one, n, one, one, one, ld, None, tab, cap)

    name = b"mpx_analysis_frames_f64"
    failed(ana(N=1000), name, b"fft_len")
    failed(ana(n=-1), name, b"negative n_frames")
    failed(ana(ld=512), name, b"ld <")
    failed(ana(N=4096, ld=2048), name, b"ld <")
    failed(ana(cap=-1), b"mpx_analysis_frames_f64w", b"win_cap")
    failed(ana(p=None), name, b"null")
    assert ana(n=0) == 0 and ana(n=0, p=None) == 0 and ana(n=0, tab=None, cap=-1) == 0
    assert lib.mpx_analysis_frames_f64(None, 1024, None, one, one, one, one, 0, one, one, one, 513, None) == 0
    failed(lib.mpx_analysis_frames_f64(None, 1024, None, one, one, one, one, 2, one, one, one, 513, None), name, b"null")

    def fused(N=2048, n=3, md=60, pd=45, p=one, tab=one, cap=5, out=one):
        return lib.mpx_analysis_compressed_fused(None, N, one, one, one, one, one, n, tab, cap, p, one, md, pd, one, 0,
                                                 one, one, out)

    name = b"mpx_analysis_compressed_fused"
    failed(fused(N=1024), name, b"fft_len")
    failed(fused(N=1000), name, b"fft_len")
    failed(fused(n=-1), name, b"negative n_frames")
    for md, pd in ((0, 10), (65, 10), (60, 0), (60, 49)):
        failed(fused(md=md, pd=pd), name, b"mag_dim")
    failed(fused(cap=-1), name, b"win_cap")
    failed(fused(p=None), name, b"null")
    failed(fused(out=None), name, b"null")
    assert fused(n=0) == 0 and fused(n=0, p=None) == 0 and fused(N=4096, n=0, md=64, pd=48, tab=None, cap=0) == 0
