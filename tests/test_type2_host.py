"""CPU: the host side of the type-2 analysis (analysis_lossless_type2 / analysis_compressed_type2) -- frame tables and
shifts against the reference's golden (tests/golden/g16_type2.npz) and the float64 model (tests/type2_model.py), the
model itself against the golden, argument errors, and the names through the src/ shim."""
import numpy as np
import pytest

import true_envelope_model as tem
import type2_model as t2m
from magphase_amd import hostmath as hm
from magphase_amd import synthetic as syn


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(golden_dir + "/g16_type2.npz")


def _inputs(g, tag):
    return syn.pcm_to_float(g[tag + "_pcm"]), int(g[tag + "_fs"]), g[tag + "_pm_sec"], g[tag + "_voi"]


def test_two_period_bounds_equal_the_reference_subset_windowing():
    rng = np.random.RandomState(16)
    for F in (1, 2, 3, 4, 7, 30, 31):
        pm = np.cumsum(rng.randint(40, 400, size=F)).astype(np.int64)
        n = int(pm[-1]) + int(rng.randint(2, 500))
        l2, r2 = hm.two_period_frame_bounds(pm, n)
        lm, rm = t2m.subset_bounds(pm, n)
        np.testing.assert_array_equal(l2, lm)
        np.testing.assert_array_equal(r2, rm)


def test_shift_and_f0_tables_against_golden(g):
    for tag in g["tags"]:
        tag = str(tag)
        v_sig, fs, pm_sec, voi = _inputs(g, tag)
        pm_c, _ = hm.clean_epochs(pm_sec, voi, check_len_smpls=v_sig.size, fs=fs)
        np.testing.assert_array_equal(hm.type2_shift(pm_c * fs), g[tag + "_shift"])
        m = t2m.analysis(v_sig, fs, pm_sec, voi, hm.define_fft_len(fs))
        np.testing.assert_array_equal(m["shift"], g[tag + "_shift"])
        np.testing.assert_array_equal(m["f0"], g[tag + "_f0"])


def test_golden_covers_the_edge_cases(g):
    for tag in ("48k_a", "16k_a"):
        v_sig, fs, pm_sec, voi = _inputs(g, tag)
        N = hm.define_fft_len(fs)
        m = t2m.analysis(v_sig, fs, pm_sec, voi, N)
        assert m["pm"][0] > N                                   # first epoch later than fft_len samples
        assert np.any(m["left2"] + m["right2"] + 1 > N)          # a two-period frame longer than fft_len
        assert np.any(m["left2"] >= N)                          # ... one left unrotated
        assert np.any(g[tag + "_gain"] == 0.0)                   # all-zero stretch
        assert np.isnan(g[tag + "_env_db"]).all(axis=1).any()
        assert int(g[tag + "_n_warn"]) > 0
    sizes = [g[str(t) + "_pm_sec"].size % 2 for t in g["tags"]]
    assert 0 in sizes and 1 in sizes                            # odd and even epoch counts


def test_model_against_golden(g):
    for tag in g["tags"]:
        tag = str(tag)
        v_sig, fs, pm_sec, voi = _inputs(g, tag)
        N = hm.define_fft_len(fs)
        step = int(g[tag + "_step"])
        m = t2m.analysis(v_sig, fs, pm_sec, voi, N)
        ref_g = g[tag + "_gain"]
        np.testing.assert_allclose(m["gain"], ref_g, rtol=1e-12, atol=0)
        np.testing.assert_allclose(m["real"][:, ::step], g[tag + "_real"], rtol=0, atol=1e-6)
        np.testing.assert_allclose(m["imag"][:, ::step], g[tag + "_imag"], rtol=0, atol=1e-6)
        env, it = tem.true_envelope(m["mag2"], "abs", 600, 0.1)
        np.testing.assert_array_equal(it, g[tag + "_passes"])
        with np.errstate(divide="ignore", invalid="ignore"):
            db = 20.0 * np.log10(env[:, ::step])
        ref = g[tag + "_env_db"].astype(np.float64)
        np.testing.assert_array_equal(np.isnan(db), np.isnan(ref))
        ok = ~np.isnan(ref)
        assert np.max(np.abs(db[ok] - ref[ok])) < 1e-4


def test_argument_errors_on_the_host():
    from magphase_amd import magphase as mp
    pcm, pm, voi = syn.make_utterance(1, dur_s=0.3, fs=16000)
    u = (syn.pcm_to_float(pcm), 16000, pm, voi)
    for bad in (float("nan"), float("inf"), "5", None, True):
        with pytest.raises(ValueError):
            mp.analysis_compressed_type2_batch([u], const_rate_ms=bad)
    with pytest.raises(ValueError):
        mp.analysis_lossless_type2_batch([u], fft_len=1000)
    with pytest.raises(ValueError):
        mp.analysis_lossless_type2_batch([(u[0], 16000, pm, voi[:-1])])
    with pytest.raises(ValueError):
        mp.analysis_lossless_type2_batch([(u[0][None, :], 16000, pm, voi)])
    with pytest.raises(ValueError):
        mp.analysis_lossless_type2_batch([u, (u[0], 48000, pm, voi)])
    with pytest.raises(ValueError):
        mp.analysis_compressed_type2_batch([(u[0], 8000, pm, voi)])   # no warp alpha at 8 kHz
    assert mp.analysis_lossless_type2_batch([]) == [] and mp.analysis_compressed_type2_batch([]) == []


def test_names_through_the_src_shim():
    import importlib
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "src"))
    try:
        src_mp = importlib.import_module("magphase")
    finally:
        sys.path.pop(0)
    for n in ("analysis_lossless_type2", "analysis_compressed_type2", "analysis_lossless_type2_batch",
              "analysis_compressed_type2_batch"):
        assert callable(getattr(src_mp, n)), n
