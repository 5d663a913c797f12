"""
CPU: the references of the compressed-path kernel tests (tests/compressed_kernels_model.py) against what the rest of the
suite already trusts -- the oracle's sp_mel_unwarp / sp_mel_warp route with the real hostmath tables, its
build_min_phase_from_mag_spec, the reference's own post-filter outputs in g5_generation_hvd704.npz, the oracle's noise
gains on that utterance -- and the decision margins of every operand set tests/test_gpu_compressed_kernels.py launches:
no magnitude at the protected log's decision, no warp output near the clip or the exp floor unless it is built to lie
far beyond, no noise bin near zero except in the one frame of zeros.  These checks guard the references; the kernels are
compared with them in the GPU file only.
"""
import warnings

import numpy as np
import pytest

import compressed_kernels_model as ckm
from magphase_amd import hostmath as hm
from oracle import magphase_oracle as orc

LD = ckm.LD


def _rel_to(diff, scale):
    return float(np.max(np.abs(diff) / scale))


# ---------------------------------------------------------------------------------------------------------------------
# the references against the oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs,mag_dim,phase_dim", [(48000, 60, 45), (16000, 24, 10)])
def test_unwarp_ref_equals_the_oracle_unwarp(fs, mag_dim, phase_dim):
    alpha, N = hm.define_alpha(fs), hm.define_fft_len(fs)
    H = N // 2 + 1
    rs = np.random.RandomState(fs)
    a = rs.uniform(-1, 1, (6, mag_dim))
    u = hm.unwarp_matrix(mag_dim, H, alpha)
    ref, absdot = ckm.unwarp_ref(a, u, 0)
    want = orc.sp_mel_unwarp(a, H, alpha=alpha, in_type="log")
    assert _rel_to(ref - want, absdot) <= 1e-12
    ref_e, _ = ckm.unwarp_ref(a, u, 1)
    assert _rel_to(ref_e / np.exp(want) - 1, np.maximum(absdot, 1)) <= 1e-12
    re, im = rs.uniform(-1, 1, (6, phase_dim)), rs.uniform(-1, 1, (6, phase_dim))
    up = hm.phase_unwarp_matrix(phase_dim, N, fs, alpha)
    w_re, w_im = orc.phase_uncompress_type1_mcep(re, im, alpha, N, fs)
    for x, want in ((re, w_re), (im, w_im)):
        ref, absdot = ckm.unwarp_ref(x, up, 0)
        assert ref.shape == want.shape and _rel_to(ref - want, absdot) <= 1e-12
    # with row tables: the oracle's interpolation of the unwarped rows
    r0, r1, t = np.array([0, 0, 2, 4]), np.array([1, 0, 3, 5]), np.array([0.25, 0.0, 1.0, 0.5], dtype=np.float32)
    full = np.exp(orc.sp_mel_unwarp(a, H, alpha=alpha, in_type="log"))
    ref, _ = ckm.unwarp_ref(a, u, 1, r0, r1, t)
    want = full[r0] + (full[r1] - full[r0]) * t[:, None]
    assert _rel_to(ref / want - 1, 1.0) <= 1e-11
    ref, absdot = ckm.unwarp_ref(re, up, 0, r0, r1, t)
    want = w_re[r0] + (w_re[r1] - w_re[r0]) * t[:, None]
    assert _rel_to(ref - want, absdot + 1e-300) <= 1e-12 or _rel_to(ref - want, np.max(absdot)) <= 1e-12


def _oracle_warp_route(x, nout, alpha, in_type):
    """orc.sp_mel_warp's route (sptk_mcep, then the alpha = 0 cosine matrix) without the float32 files it passes its input and
    its cepstra through: the operands here are float32 values already, and the map is compared at 1e-12."""
    a = float("%1.2f" % alpha)
    p = x * x if in_type == 3 else np.exp(x) ** 2
    logp = np.log(p + 1.0e-8)
    half = x.shape[1] - 1
    c = np.fft.ifft(orc.add_hermitian_half_real(logp)).real[:, :half + 1].copy()
    c[:, 0] /= 2.0
    c[:, half] /= 2.0
    return orc.mcep_to_sp_cosmat(orc.freqt(c, nout - 1, a), nout, alpha=0.0, out_type="log")


@pytest.mark.parametrize("fs,mag_dim,phase_dim", [(48000, 60, 45), (16000, 24, 10)])
def test_warp_ref_equals_the_oracle_warp(fs, mag_dim, phase_dim):
    alpha, N = hm.define_alpha(fs), hm.define_fft_len(fs)
    H = N // 2 + 1
    mag, real, _ = ckm.warp_operands(4, H, seed=fs)
    for x, mode, in_type, nout, nrows in ((mag, 0, 3, mag_dim, None), (real, 3, 2, mag_dim, phase_dim)):
        w = hm.warp_matrix(nout, H, alpha, nrows=nrows)
        ref, absdot = ckm.warp_ref(x.astype(np.float64), w, mode)
        want = _oracle_warp_route(x.astype(np.float64), nout, alpha, in_type)[:, :w.shape[0]]
        assert ref.shape == want.shape and _rel_to(ref - want, absdot) <= 1e-12
    # the oracle's own function, float32 files included, agrees at their precision
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        own = np.log(orc.sp_mel_warp(mag.astype(np.float64), mag_dim, alpha=alpha, in_type=3))
    ref, absdot = ckm.warp_ref(mag, hm.warp_matrix(mag_dim, H, alpha), 0)
    assert _rel_to(ref - own, absdot) <= 1e-6
    # epilogues
    y, _ = ckm.warp_ref(real, hm.warp_matrix(mag_dim, H, alpha, nrows=phase_dim), 1, np.array([1, 0, 1, 0], dtype=np.float32))
    assert np.all(y[[1, 3]] == 0) and not np.any(np.signbit(y[[1, 3]])) and np.all(np.abs(y) <= 1)


def test_warp_ref_modes_and_epilogues_on_hand_made_values():
    x = np.array([[0.0, 1.0, 2.0, 1e-3]], dtype=np.float32)
    w = np.eye(4, dtype=np.float32)
    y0, a0 = ckm.warp_ref(x, w, 0)
    assert np.allclose(np.asarray(y0[0], dtype=np.float64), np.log(x[0].astype(np.float64) ** 2 + 1e-8), rtol=1e-14, atol=1e-15)
    assert np.array_equal(a0, np.abs(y0))
    y2, _ = ckm.warp_ref(x, w, 2)
    assert y2[0, 0] == ckm.MAGIC and y2[0, 1] == 0.0 and abs(float(y2[0, 2]) - np.log(2.0)) < 1e-15
    y2, _ = ckm.warp_ref(x, np.full((1, 4), 1e-7, dtype=np.float32), 2)   # -1e10 * 1e-7 = -1000 < -745.13
    assert y2[0, 0] == ckm.MAGIC
    y1, _ = ckm.warp_ref(np.array([[0.9, -0.9, 0.1, 0.0]], dtype=np.float32), w, 1, np.ones(1, dtype=np.float32))
    assert y1[0, 0] == 1 and y1[0, 1] == -1
    assert abs(float(y1[0, 2]) - np.log(np.exp(2.0 * np.float64(np.float32(0.1))) + 1e-8)) < 1e-12
    y3, _ = ckm.warp_ref(np.array([[0.9, -0.9, 0.1, 0.0]], dtype=np.float32), w, 3)
    assert y3[0, 0] > 1.7 and y3[0, 1] < -1.7
    # the interpolated row is formed before the prologue, with the device's float32 fmaf
    xr = np.array([[1.0, 2.0, 3.0, 4.0], [3.0, 2.0, 1.0, 8.0]], dtype=np.float32)
    yi, _ = ckm.warp_ref(xr, w, 0, None, [0], [1], [0.5])
    assert np.allclose(np.asarray(yi[0], dtype=np.float64), np.log(np.array([2.0, 2.0, 2.0, 6.0]) ** 2 + 1e-8), rtol=1e-15)


def test_phase_rows_ref_interpolates_masks_and_clips():
    tr = np.array([[0.5, -2.0], [0.7, -3.0], [np.nan, np.nan]], dtype=np.float32)
    out_r, out_i = ckm.warp_phase_rows_ref(tr, -tr, [0, 0, 2], [1, 0, 2], [0.5, 0.0, 0.3], [1.0, 1.0, 0.0])
    assert abs(float(out_r[0, 0]) - (0.5 + (np.float64(np.float32(0.7)) - 0.5) * 0.5)) < 1e-15
    assert out_r[0, 1] == -1 and out_i[0, 1] == 1
    assert out_r[1, 0] == 0.5 and np.all(out_r[2] == 0) and np.all(out_i[2] == 0) and not np.any(np.signbit(out_r[2]))


@pytest.mark.parametrize("N", ckm.FFT_LENS)
def test_min_phase_ref_equals_the_oracle_and_the_closed_form(N):
    mag, kinds, closed = ckm.min_phase_rows(N)
    assert set(kinds) == {"flat", "allpole", "peak", "random"} and mag.shape == (70, N // 2 + 1)
    phi = ckm.min_phase_ref(mag, N)
    want = orc.build_min_phase_from_mag_spec(mag.astype(np.float64))
    got = mag.astype(np.float64) * np.exp(1j * phi)
    assert _rel_to(got - want, np.abs(want)) <= 1e-12 * max(1.0, float(np.max(np.abs(phi))))
    assert np.all(phi[:, 0] == 0) and np.max(np.abs(phi[:, -1])) < 1e-12
    for f, ph in closed.items():   # the float32 rounding of the magnitudes is all that separates the two
        d = ckm.phasor_angle_error(np.cos(phi[f]), np.sin(phi[f]), ph)
        assert np.max(np.abs(d)) <= ckm.hilbert_noise_bound(N), (f, kinds[f])
    assert len(closed) == 9


def test_min_phase_float64_model_against_the_longdouble_dft():
    """The float64 FFT form is what judges the kernel (tolerances of 1e-6 .. 1e-5 rad): its own distance from the
    longdouble matrix form at N = 1024 is more than a thousand times finer."""
    mag, kinds, _ = ckm.min_phase_rows(1024)
    rows = [kinds.index(k) for k in ("flat", "allpole", "peak", "random")] + [69]
    d = float(np.max(np.abs(ckm.min_phase_ref(mag[rows], 1024) - ckm.min_phase_dft_ref(mag[rows], 1024).astype(np.float64))))
    print("min_phase_ref (float64 FFT) vs longdouble DFT, N = 1024: %.3g rad" % d)
    assert d <= 1e-12


def test_post_filter_ref_equals_the_reference_outputs(golden_dir):
    g = np.load(golden_dir + "/g5_generation_hvd704.npz")
    mm = g["in_mag"].reshape(-1, 60).astype(np.float64)
    for fs, key in ((48000, "pf48"), (16000, "pf16")):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            nx0, nx1, half, tilt = hm.post_filter_tables(60, fs)
        y, absterm = ckm.post_filter_ref(mm, half, nx0, nx1, tilt)
        assert np.max(np.abs(y - g[key])) <= 1e-12
        assert np.all(absterm >= np.abs(mm) * np.abs(tilt)[None, :])
    for D in ckm.POST_DIMS:   # the synthetic tables: windows inside the row, touching both ends
        nx0, nx1, half, tilt = ckm.post_filter_synth_tables(D)
        b = nx0 + np.arange(half.size)
        assert half.size == nx1 - nx0 + 1 and np.min(b - half) == 0 and np.max(b + half) == D - 1
        assert 1 in ckm.post_filter_frames(D) and 100 in ckm.post_filter_frames(D) and 256 // D + 1 in ckm.post_filter_frames(D)
    assert [256 // D for D in ckm.POST_DIMS] == [85, 10, 4, 4, 3, 2, 1]


def test_noise_refs_chained_equal_the_oracle_gains(golden_dir):
    g = np.load(golden_dir + "/g5_generation_hvd704.npz")
    mm = g["in_mag"].reshape(-1, 60).astype(np.float64)
    rr = g["in_real"].reshape(-1, 45).astype(np.float64)
    ii = g["in_imag"].reshape(-1, 45).astype(np.float64)
    np.random.seed(11)
    _, dbg = orc.synthesis_from_compressed(mm, rr, ii, g["in_lf0"].astype(np.float64), 48000, return_debug=True)
    np.random.seed(11)
    noise = np.random.uniform(-1, 1, dbg["ns_len"])
    N = 4096
    _, left, right, _ = orc.frame_bounds(dbg["v_pm"], dbg["ns_len"])
    voi = np.asarray(dbg["v_voi"], dtype=bool)
    sums = np.array([ckm.noise_stats_ref(noise, int(p), int(a), int(b), bool(v), N)
                     for p, a, b, v in zip(dbg["v_pm"], left, right, voi)])
    gains, inv = ckm.noise_gains_ref(sums, voi, [0, sums.size], N // 2 - 1)
    assert np.any(voi) and np.any(~voi)
    assert abs(gains[0, 0] / dbg["g_voi"] - 1) <= 1e-12 and abs(gains[0, 1] / dbg["g_unv"] - 1) <= 1e-12
    assert np.allclose(inv, np.where(voi, 1 / dbg["g_voi"], 1 / dbg["g_unv"]), rtol=1e-12, atol=0)
    # an empty class
    gains, inv = ckm.noise_gains_ref([4.0, 8.0, 2.0], [1, 1, 0], [0, 2, 3], 2)
    assert gains[0, 0] == np.sqrt(np.exp(3.0)) and np.isnan(gains[0, 1])
    assert np.isnan(gains[1, 0]) and gains[1, 1] == np.sqrt(np.exp(1.0))
    assert np.all(np.isfinite(inv)) and inv[2] == 1 / np.sqrt(np.exp(1.0))


# ---------------------------------------------------------------------------------------------------------------------
# bit-exact properties of the references
# ---------------------------------------------------------------------------------------------------------------------
def test_one_hot_operands_and_the_lerp_ends_are_exact():
    for K in ckm.ONEHOT_K:
        a, u = ckm.onehot_unwarp_operands(K)
        ref, absdot = ckm.unwarp_ref(a, u, 0)
        assert np.array_equal(ref, u[np.arange(ckm.ONEHOT_F) % K].astype(LD)) and np.array_equal(absdot, np.abs(ref))
    assert (ckm.ONEHOT_H, ckm.ONEHOT_F) == (513, 70) and ckm.ONEHOT_F - 64 == 6 and ckm.ONEHOT_H - 512 == 1
    ops = ckm.unwarp_operands(40, 65, 45, 24, seed=1)
    a = ops["a_real"]
    r0, r1 = np.arange(39), np.arange(1, 40)
    for t, want in ((0.0, a[r0]), (1.0, a[r1])):
        tt = np.full(39, t, dtype=np.float32)
        assert np.array_equal(ckm.lerp(a[r0].astype(LD), a[r1].astype(LD), LD(t)), want.astype(LD))
        ref, _ = ckm.unwarp_ref(a, ops["u_phase"], 0, r0, r1, tt)
        assert np.array_equal(ref, ckm.unwarp_ref(want, ops["u_phase"], 0)[0])
        ref, _ = ckm.unwarp_ref(ops["a_mag"], ops["u_mag"], 1, r0, r1, tt)
        end = ckm.unwarp_ref(ops["a_mag"][r0 if t == 0 else r1], ops["u_mag"], 1)[0]
        # (e0 + (e1 - e0) rounds twice in longdouble at t == 1: the exponentials are no float32 values)
        assert np.array_equal(ref, end) if t == 0 else np.max(np.abs(ref / end - 1)) <= 2.0 ** -60
        assert np.array_equal(ckm.lerp_f32(a[r0], a[r1], tt[:, None]) if t == 0 else want, want)
    # the float32 fmaf against the exact lerp: the rounded difference and one rounding of the result
    rs = np.random.RandomState(0)
    x0, x1 = ckm.warp_operands(50, 64, seed=3)[0], ckm.warp_operands(50, 64, seed=4)[0]
    t = rs.uniform(0, 1, (50, 1)).astype(np.float32)
    t[:5], t[5:10] = 0.0, 1.0
    got = ckm.lerp_f32(x0, x1, t).astype(LD)
    exact = ckm.lerp(x0.astype(LD), x1.astype(LD), t.astype(LD))
    assert np.all(np.abs(got - exact) <= ckm.U24 * (np.abs(x1.astype(LD) - x0) * t + np.abs(exact)) * (1 + 1e-6))
    assert np.array_equal(got[:5], x0[:5].astype(LD))


def test_one_hot_warp_matrices_name_every_chunk_and_tail_edge():
    seen = {}
    for F, H, md, pd in ckm.WARP_SHAPES:
        for nout, seed in ((md, 1), (pd, 2)):
            w, ks = ckm.warp_onehot_matrix(nout, H, seed)
            assert np.array_equal(np.sum(w != 0, axis=1), np.ones(nout)) and np.all(w[np.arange(nout), ks] == 1)
            seen.setdefault(H, set()).update(int(k) for k in ks)
    for H, ks in seen.items():
        hfull = H & ~63
        assert ks >= {k for k in ckm.WARP_ONEHOT_BINS + (hfull - 1, hfull, H - 1) if 0 <= k < H} or H in (40, 64, 65)
    assert {s[1] for s in ckm.WARP_SHAPES} == {40, 64, 65, 100, 513, 2049}
    assert {s[0] for s in ckm.WARP_SHAPES} == {1, 63, 64, 65, 130}
    assert {d for s in ckm.WARP_SHAPES for d in s[2:]} == {1, 15, 16, 17, 45, 60, 64}
    assert all(s[2] != s[3] for s in ckm.WARP_SHAPES) and sum(s[1] == 2049 for s in ckm.WARP_SHAPES) == 1


# ---------------------------------------------------------------------------------------------------------------------
# decision margins of the operand sets the GPU tests launch
# ---------------------------------------------------------------------------------------------------------------------
def _far_from_clip(y, voi=None):
    y = np.abs(np.asarray(y, dtype=np.float64))
    if voi is not None:
        y = y[np.asarray(voi) != 0]
    return np.all((y <= 1 - 1e-4) | (y >= 1.1))


@pytest.mark.parametrize("F,H,mag_dim,phase_dim", ckm.WARP_SHAPES)
def test_margins_of_the_warp_operands(F, H, mag_dim, phase_dim):
    if H == 2049:
        F = 8          # the same generator and matrices: a few rows show the margins of the large case
    n_in = F + 7
    mag, real, imag = ckm.warp_operands(n_in, H, seed=F + H + 1)
    assert np.min(mag) >= ckm.MAG_LO and np.max(mag) <= ckm.MAG_HI and np.max(np.abs(real)) < 1 and np.max(np.abs(imag)) < 1
    assert np.min(mag) < 1e-5 and np.max(mag) > 1.0
    w_mag, w_ph = ckm.warp_matrices(mag_dim, phase_dim, H, seed=F)
    rows = ckm.row_tables(n_in, F, seed=H)
    for tab in ((None, None, None), rows):
        for x in (real, imag):
            y, _ = ckm.warp_ref(x, w_ph, 3, None, *tab)
            assert np.max(np.abs(y)) <= 1 - 1e-4
        y, _ = ckm.warp_ref(mag, w_mag, 2, None, *tab)
        assert np.min(y) >= ckm.EXP_FLOOR + 1
    # the one-hot form: a quarter of the phase prologue stays inside the clip
    assert np.max(np.abs(ckm.warp_prologue_ref(1, real))) * 0.25 <= 1 - 1e-4


def test_margins_of_the_directed_warp_cases():
    F, H, pd, mag, real, imag, real_dev, imag_dev, voi, w_mag, w_ph, kind = ckm.epilogue_case()
    assert np.all(voi[64:128] == 0) and np.all(np.isnan(real_dev[64:128])) and H & ~63 == 64
    for x, kk in ((real, kind[0]), (imag, kind[1])):
        y, _ = ckm.warp_ref(x, w_ph, 3)
        live = voi != 0
        assert np.all(np.abs(y[live & (kk <= 1)]) >= 1.1) and np.all(np.abs(y[live & (kk > 1)]) <= 1 - 1e-4)
        assert np.any(y[live] >= 1.1) and np.any(y[live] <= -1.1)
    F, H, md, mag, real, imag, zero_rows, zero_bin, w_fb, w_ph, voi = ckm.mode2_case()
    y = ckm.warp_prologue_ref(2, mag) @ w_fb.astype(LD).T
    floored = np.zeros(F, dtype=bool)
    floored[zero_rows + [10]] = True
    assert np.all(y[floored] < -1e6) and np.all(y[~floored] >= ckm.EXP_FLOOR + 1) and zero_bin >= (H & ~63)
    assert np.all(mag[mag != 0] >= ckm.MAG_LO) and np.sum(mag == 0) == 3
    for F, n_var, H in ((130, 70, 100), (65, 150, 65), (65, 150, 513), (1, 3, 40)):
        rows, voi, in_use = ckm.rows_case(F, n_var, H, seed=F)
        mag, real, imag = ckm.warp_operands(n_var, H, seed=F + n_var)
        w_mag, w_ph = ckm.warp_matrices(24, 45, H, seed=n_var)
        assert np.any(voi != 0) and np.all(in_use[rows[0][voi != 0]] == 1) and np.all(in_use[rows[1][voi != 0]] == 1)
        if n_var >= 128:
            assert np.all(in_use[64:128] == 0) and np.any(in_use[:64] == 1) and np.any(in_use[128:] == 1)
        for x in (real, imag):
            y, _ = ckm.warp_ref(x, w_ph, 3)
            assert np.max(np.abs(y)) <= 1 - 1e-4
        assert np.min(ckm.warp_ref(mag, w_mag, 2, None, *rows)[0]) >= ckm.EXP_FLOOR + 1
    for F, pd in ckm.PHASE_ROWS_SIZES:
        tmp, row0, row1, rowt, voi = ckm.phase_rows_case(F, pd, seed=F + pd)
        t = rowt.astype(np.float64)[:, None]
        for m in tmp:
            y = m[row0].astype(np.float64) + (m[row1].astype(np.float64) - m[row0]) * t
            assert _far_from_clip(y, voi)
    assert [F * pd for F, pd in ckm.PHASE_ROWS_SIZES] == [1, 255, 256, 257]


def test_margins_of_the_unwarp_operands_and_tables():
    for F, H, km, kp in ckm.UNWARP_RANDOM:
        ops = ckm.unwarp_operands(min(F, 9), H, km, kp, seed=F + H)
        for a, u in ((ops["a_mag"], ops["u_mag"]), (ops["a_real"], ops["u_phase"])):
            assert np.min(np.abs(a)) >= 0.5 and np.max(np.abs(a)) < 1.0 and np.min(np.abs(u)) > 0
            assert np.max(np.abs(a).astype(np.float64) @ np.abs(u).astype(np.float64)) <= 8.0
        assert km != kp
    assert {s[0] for s in ckm.UNWARP_RANDOM} == {1, 31, 32, 33, 127, 129}
    assert {s[1] for s in ckm.UNWARP_RANDOM} == {40, 64, 65, 513, 1025, 2049}
    assert (64, 1) in {s[2:] for s in ckm.UNWARP_RANDOM} and (1, 64) in {s[2:] for s in ckm.UNWARP_RANDOM}
    assert sum(s[1] == 2049 for s in ckm.UNWARP_RANDOM) == 1
    assert {2 * ((K + 3) // 4) for K in ckm.ONEHOT_K} >= {2, 4, 12 * 2, 32} and any(K % 2 for K in ckm.ONEHOT_K)
    for n_rows in ckm.TILED_N_ROWS:
        row0, row1, rowt = ckm.tiled_row_tables(n_rows, seed=n_rows)
        assert np.all(np.diff(row0) >= 0) and np.all((row1 - row0 >= 0) & (row1 - row0 <= 1)) and row1.max() <= n_rows - 1
        tf = ckm.tile_first_of(row0, n_rows)
        assert tf.size == (n_rows + 30) // 31 + 1 and tf[0] == 0 and tf[-1] == row0.size <= 200
        for T in range(tf.size - 1):   # a frame's two rows lie in the 32 rows its tile holds
            f = slice(tf[T], tf[T + 1])
            assert np.all(row0[f] >= 31 * T) and np.all(row1[f] <= 31 * T + 31)
    counts = {n: np.diff(ckm.tile_first_of(ckm.tiled_row_tables(n, seed=n)[0], n)) for n in ckm.TILED_N_ROWS}
    assert counts[100][1] == 0 and counts[100][0] > 65 and counts[31][0] == 65 and counts[1][0] == 65


@pytest.mark.parametrize("N", ckm.FFT_LENS)
def test_margins_of_the_min_phase_and_noise_inputs(N):
    mag, kinds, closed = ckm.min_phase_rows(N)
    assert np.all(np.min(mag, axis=1) > 1e-3 * np.max(mag, axis=1)), "no magnitude within 1e-3 (relative) of 0"
    r0, r1, t = ckm.min_phase_row_tables(mag.shape[0])
    assert np.all(ckm.lerp_f32(mag[r0], mag[r1], t[:, None]) > 0)
    assert np.sum(r0 != r1) == 18 and [round(float(v), 2) for v in np.unique(t[r0 != r1])] == [0.0, 0.37, 1.0]
    left, right, wtype, pos, x = ckm.noise_case(N)
    F = left.size
    assert F == ckm.NOISE_FRAMES + 2 and np.all(left + right + 1 <= N) and np.min(pos - left) >= 0 and np.max(pos + right) < x.size
    assert {(int(a), int(b)) for a, b in zip(left, right)} >= set(ckm.noise_shapes(N))
    assert set(wtype[:4 * len(ckm.noise_shapes(N))]) == {0, 1}
    if N == 4096:
        assert np.sum(left + right + 1 > 1024) >= 8 and {(511, 511), (511, 512), (512, 512)} <= set(ckm.noise_shapes(N))
    for f in range(F):
        X = ckm.noise_spectrum_ref(x, int(pos[f]), int(left[f]), int(right[f]), int(wtype[f]), N)[1:N // 2]
        p = X.real ** 2 + X.imag ** 2
        if f == F - 2:
            assert np.all(p == 0)          # the one directed frame of zeros
            assert abs(ckm.noise_stats_ref(x, int(pos[f]), 50, 50, 1, N) / ((N // 2 - 1) * 1.0e20) - 1) <= 1e-15
        else:
            assert np.min(p) >= 1e-30, f
            assert ckm.noise_condition(x, int(pos[f]), int(left[f]), int(right[f]), int(wtype[f]), N) <= ckm.NOISE_COND_MAX, f
    flat = ckm.noise_stats_ref(x, int(pos[F - 1]), 40, 40, 0, N)
    assert abs(flat / ((N // 2 - 1) * np.log(ckm.DELTA_AMP) ** 2) - 1) <= 1e-13
    for pattern in ckm.GAIN_PATTERNS:
        sums, voiced, off = ckm.gains_case(N, pattern)
        assert list(np.diff(off)) == [1, 2, 255, 256, 257, 600] and sums.dtype == np.float32
        gains, inv = ckm.noise_gains_ref(sums, voiced, off, N // 2 - 1)
        assert np.all(np.isfinite(inv)) and np.any(np.isnan(gains))
