"""GPU: the type-2 analysis (analysis_lossless_type2 / analysis_compressed_type2: k_analysis_f64 over the one- and
two-period frame tables, k_frame_gain, k_true_envelope at 600 coefficients, the mel warp) against the reference's golden
(tests/golden/g16_type2.npz) and the float64 model (tests/type2_model.py).  Tolerances are <= 3 x the worst case
measured on the MI355X (tests/_tol.py records it)."""
import os
import warnings

import numpy as np
import pytest

import type2_model as t2m
from _tol import note, within
from magphase_amd import hostmath as hm
from magphase_amd import libaudio as la
from magphase_amd import libutils as lu
from magphase_amd import magphase as mp
from magphase_amd import synthetic as syn

pytestmark = pytest.mark.gpu

T2_PHASE_TOL = 9e-8     # |d real|, |d imag| per bin (float64 transform: float32 rounding only; measured 3.0e-8)
T2_GAIN_TOL = 6e-16     # relative gain error: float64 window and accumulation on the exact samples (measured 2.2e-16)
T2_ENV_TOL = 3e-4       # dB, any stored bin, rows whose pass count equals the reference's (measured 1.0e-4)
T2_ITERS_GAP = 3        # passes per frame apart from the reference's, at most
T2_MAG_TOL = 2e-5       # compressed log-mel magnitude, natural log units (measured 1.4e-5; test_gpu_compressed's WARP_TOL)
T2_PH_COMP_TOL = 2.6e-6  # compressed phase (measured 8.9e-7, as test_gpu_compressed's WARP_PHASE_TOL measures)
T2_LGAIN_TOL = 9e-6     # log gain; b_norm_mag: the row mean of the log-mel magnitudes (measured 3.2e-6)


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(golden_dir + "/g16_type2.npz")


def _utt(g, tag):
    return (syn.pcm_to_float(g[tag + "_pcm"]), int(g[tag + "_fs"]), g[tag + "_pm_sec"], g[tag + "_voi"])


def _phase_check(real, imag, r_real, r_imag, r_mag, peak=None):
    """|d real|, |d imag| per bin, on bins above 1e-5 of the frame peak (all-zero frames: none): the float64 transform
    leaves the float32 rounding of the phasor (and of the golden's stored values)."""
    peak = np.max(r_mag, axis=1, keepdims=True) if peak is None else peak.copy()
    peak[peak == 0] = 1.0
    big = r_mag > 1e-5 * peak
    within(np.max(np.abs(real - r_real)[big]), T2_PHASE_TOL, "T2_PHASE_TOL")
    within(np.max(np.abs(imag - r_imag)[big]), T2_PHASE_TOL, "T2_PHASE_TOL")


def _lossless(u, **kw):
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        r = mp.analysis_lossless_type2_batch([u], return_iters=True, **kw)[0]
    return r, len(w)


def test_lossless_type2_against_golden_and_model(g):
    n_diff = n_all = 0
    for tag in g["tags"]:
        tag = str(tag)
        u = _utt(g, tag)
        step = int(g[tag + "_step"])
        (env, real, imag, f0, fs, shift, gain, it), n_warn = _lossless(u)
        assert fs == u[1] and n_warn == int(g[tag + "_n_warn"])
        np.testing.assert_array_equal(f0, g[tag + "_f0"])
        np.testing.assert_array_equal(shift, g[tag + "_shift"])
        assert shift.dtype == np.float64 and gain.dtype == np.float64
        m = t2m.analysis(*u, hm.define_fft_len(u[1]))
        _phase_check(real, imag, m["real"], m["imag"], m["mag1"])
        _phase_check(real[:, ::step], imag[:, ::step], g[tag + "_real"], g[tag + "_imag"], m["mag1"][:, ::step],
                     peak=np.max(m["mag1"], axis=1, keepdims=True))
        ref_g = g[tag + "_gain"]
        zero = ref_g == 0.0
        np.testing.assert_array_equal(gain[zero], 0.0)
        within(np.max(np.abs(gain[~zero] / ref_g[~zero] - 1.0)), T2_GAIN_TOL, "T2_GAIN_TOL")
        within(np.max(np.abs(gain[~zero] / m["gain"][~zero] - 1.0)), T2_GAIN_TOL, "T2_GAIN_TOL")
        ref_it = g[tag + "_passes"]
        assert np.all(np.abs(it.astype(int) - ref_it) <= T2_ITERS_GAP)
        with np.errstate(divide="ignore", invalid="ignore"):
            db = 20.0 * np.log10(env[:, ::step])
        ref = g[tag + "_env_db"].astype(np.float64)
        nan_ref = np.isnan(ref).all(axis=1)
        np.testing.assert_array_equal(np.isnan(env).all(axis=1), nan_ref)
        same = (it == ref_it) & ~nan_ref
        n_diff += int(np.sum(it[~nan_ref] != ref_it[~nan_ref]))
        n_all += int(np.sum(~nan_ref))
        within(np.max(np.abs(db[same] - ref[same])), T2_ENV_TOL, "T2_ENV_TOL")
    note("type2:envelope_pass_count_differs", n_diff / n_all)
    assert n_diff / n_all <= 0.05


def test_lossless_type2_batch_equals_single_calls(g):
    utts = [_utt(g, str(t)) for t in g["tags"] if int(g[str(t) + "_fs"]) == 48000]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        batch = mp.analysis_lossless_type2_batch(utts)
        single = [mp.analysis_lossless_type2_batch([u])[0] for u in utts]
        dev = mp.analysis_lossless_type2_batch(utts, return_device=True)
    for b, s, d in zip(batch, single, dev):
        for x, y in zip(b, s):
            np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(d[0].cpu().numpy().astype(np.float64), b[0])
        np.testing.assert_array_equal(d[6].cpu().numpy(), b[6])


@pytest.mark.parametrize("tag", ["48k_b", "16k_b"])
def test_compressed_type2_against_golden(g, tag):
    u = _utt(g, tag)
    for k, (rate, norm) in enumerate(g["comp_cases"]):
        key = "%s_c%d" % (tag, k)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            r = mp.analysis_compressed_type2_batch([u], mag_dim=60, phase_dim=45, b_norm_mag=bool(norm),
                                                   const_rate_ms=float(rate))[0]
        assert len(r) == 8 and r[5] == u[1] and r[6] == int(g[key + "_fft_len"])
        assert r[0].shape == g[key + "_mag"].shape and r[1].shape == g[key + "_real"].shape
        np.testing.assert_array_equal(r[3], g[key + "_lf0"])
        np.testing.assert_array_equal(r[4], g[key + "_shift"])
        within(np.max(np.abs(r[0] - g[key + "_mag"])), T2_MAG_TOL, "T2_MAG_TOL")
        within(np.max(np.abs(r[1] - g[key + "_real"])), T2_PH_COMP_TOL, "T2_PH_COMP_TOL")
        within(np.max(np.abs(r[2] - g[key + "_imag"])), T2_PH_COMP_TOL, "T2_PH_COMP_TOL")
        within(np.max(np.abs(r[7] - g[key + "_lgain"])), T2_LGAIN_TOL, "T2_LGAIN_TOL")


def test_file_products(g, tmp_path):
    u = _utt(g, "16k_b")
    wav = str(tmp_path / "t2.wav")
    la.write_audio_file(wav, u[0], u[1], norm=None)
    mp.set_epoch_provider(lambda f: (u[2], u[3]))
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            r = mp.analysis_lossless_type2(wav)
            assert mp.analysis_lossless_type2(wav, out_dir=str(tmp_path)) is None
            c = mp.analysis_compressed_type2(wav, const_rate_ms=5.0)
            d_var, d_cr = tmp_path / "var", tmp_path / "cr"
            d_var.mkdir(), d_cr.mkdir()
            assert mp.analysis_compressed_type2(wav, out_dir=str(d_var)) is None
            assert mp.analysis_compressed_type2(wav, out_dir=str(d_cr), const_rate_ms=5.0) is None
    finally:
        mp.set_epoch_provider(None)
    assert len(r) == 7 and len(c) == 8
    H = r[0].shape[1]
    np.testing.assert_array_equal(lu.read_binfile(str(tmp_path / "t2.mag"), dim=H), r[0].astype(np.float32))
    np.testing.assert_array_equal(lu.read_binfile(str(tmp_path / "t2.shift"), dim=1).ravel(), r[5].astype(np.float32))
    assert sorted(os.listdir(str(tmp_path))) == ["cr", "t2.f0", "t2.imag", "t2.mag", "t2.real", "t2.shift", "t2.wav",
                                                 "var"]
    assert sorted(os.listdir(str(d_var))) == ["t2.imag", "t2.lf0", "t2.mag", "t2.real", "t2.shift"]
    assert sorted(os.listdir(str(d_cr))) == ["t2.imag", "t2.lf0", "t2.mag", "t2.real"]
    np.testing.assert_array_equal(lu.read_binfile(str(d_cr / "t2.mag"), dim=60), c[0].astype(np.float32))
