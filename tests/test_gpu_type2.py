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


# ---------------------------------------------------------------------------------------------------------------------
# synthetic utterances against the float64 model: fft_len 1024, mixed sample rates, over-long frames, silence
# ---------------------------------------------------------------------------------------------------------------------
def _synthetic(u, fs, dur_s=0.4):
    pcm, pm, voi = syn.make_utterance(u, dur_s=dur_s, fs=fs)
    return (syn.pcm_to_float(pcm), fs, pm, voi)


def _sparse_epochs(u, fs, N, dur_s):
    """A synthetic signal with epochs N/2 + 40 samples apart, voiced and unvoiced in turn: every one-period frame is
    longer than N (the gain kernel's truncation branch, and past the first N/2 frames' left its wrap of the index)."""
    x = _synthetic(u, fs, dur_s)[0]
    pm = np.arange(1, int(x.size // (N // 2 + 40))) * (N // 2 + 40) / float(fs)
    return (x, fs, np.round(pm, 6), (np.arange(pm.size) % 2).astype(np.float64))


def _silent(fs, dur_s=0.2):
    x, _, pm, voi = _synthetic(7, fs, dur_s)
    return (np.zeros_like(x), fs, pm, voi)


def _check_against_model(r, u, N):
    env, real, imag, f0, fs, shift, gain = r[:7]
    m = t2m.analysis(*u, N)
    assert fs == u[1] and env.shape == m["mag2"].shape and real.shape == m["real"].shape
    np.testing.assert_array_equal(f0, m["f0"])
    np.testing.assert_array_equal(shift, m["shift"])
    zero = m["gain"] == 0.0
    np.testing.assert_array_equal(gain[zero], 0.0)
    if not zero.all():
        within(np.max(np.abs(gain[~zero] / m["gain"][~zero] - 1.0)), T2_GAIN_TOL, "T2_GAIN_TOL")
    nan_ref = (m["mag2"] == 0.0).any(axis=1)   # a magnitude row with a zero bin: an all-NaN envelope row
    np.testing.assert_array_equal(np.isnan(env).all(axis=1), nan_ref)
    np.testing.assert_array_equal(np.isnan(env).any(axis=1), nan_ref)
    if np.max(m["mag1"]) > 0.0:
        _phase_check(real, imag, m["real"], m["imag"], m["mag1"])
    else:   # silence: the phasor of a zero bin is 0 (the reference divides by 1 there)
        within(np.max(np.abs(real - m["real"])), T2_PHASE_TOL, "T2_PHASE_TOL")
        within(np.max(np.abs(imag - m["imag"])), T2_PHASE_TOL, "T2_PHASE_TOL")
    return m


def _batch_with_warnings(utts, **kw):
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        r = mp.analysis_lossless_type2_batch(utts, **kw)
    return r, len(w)


def test_lossless_type2_8k_fft_1024_against_model():
    utts = [_synthetic(21, 8000), _synthetic(22, 8000), _sparse_epochs(23, 8000, 1024, 1.0), _silent(8000)]
    assert hm.define_fft_len(8000) == 1024
    n_model = 0
    for u in utts:
        (r,), n_warn = _batch_with_warnings([u])
        m = _check_against_model(r, u, 1024)
        assert n_warn == m["n_warn"]
        n_model += m["n_warn"]
    batch, n_warn = _batch_with_warnings(utts)
    assert n_warn == n_model and n_model >= 10
    for r, u in zip(batch, utts):
        m = _check_against_model(r, u, 1024)
    assert np.all(batch[3][6] == 0.0) and np.isnan(batch[3][0]).all()
    one = _batch_with_warnings([utts[2]])[0][0]
    for x, y in zip(one, batch[2]):
        np.testing.assert_array_equal(x, y)


def test_lossless_type2_batch_of_mixed_sample_rates_against_model():
    N = 2048
    utts = [_synthetic(31, 48000), _synthetic(32, 16000), _synthetic(33, 8000), _sparse_epochs(34, 16000, N, 1.2),
            _silent(48000), _synthetic(35, 8000, 0.25)]
    batch, n_warn = _batch_with_warnings(utts, fft_len=N)
    n_model = 0
    for r, u in zip(batch, utts):
        n_model += _check_against_model(r, u, N)["n_warn"]
    assert n_warn == n_model
    assert np.all(batch[4][6] == 0.0) and np.isnan(batch[4][0]).all()
