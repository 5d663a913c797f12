"""CPU tests of griffin_lim's host side: API presence, argument checks (no device touched), the plan tables, the fold of
the initial phase into the lossless synthesis' inputs, the fp64 model against the reference's golden, the C ABI's checks."""
import ctypes
import os
import sys

import numpy as np
import pytest

import griffin_lim_model as glm
from magphase_amd import _lib, hostmath as hm
from magphase_amd import magphase as mp
from oracle import magphase_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "g13_griffin_lim.npz")
SEED = 1313


def _golden():
    return np.load(GOLD)


def _ndarray_init(shape, fs):   # tools/gen_golden_griffin_lim.py:ndarray_init
    return 2 * np.pi * (np.random.RandomState(SEED + fs).rand(*shape) - 0.5)


def test_api_exists_in_package_and_src_shim():
    assert callable(mp.griffin_lim) and callable(mp.griffin_lim_batch)
    sys.path.insert(0, os.path.join(ROOT, "src"))
    try:
        import magphase as shim
    finally:
        sys.path.pop(0)
    assert shim.griffin_lim is mp.griffin_lim and shim.griffin_lim_batch is mp.griffin_lim_batch


def _mag(F=6, H=1025):
    return np.abs(np.random.RandomState(3).randn(F, H)) + 0.1


@pytest.mark.parametrize("case", ["domain_first", "domain_rest", "domain_lone", "negative", "length", "zero_frames",
                                  "niters0", "niters_float", "init_str", "init_shape", "win", "fft_len", "mixed_N"])
def test_value_errors_before_any_device_call(case, monkeypatch):
    def no_engine(*a, **k):
        raise AssertionError("device touched")

    monkeypatch.setattr(mp, "get_engine", no_engine)
    m = _mag()
    sh = np.full(6, 200.0)
    kw = {}
    args = (m, sh)
    if case == "domain_first":
        sh[0] = 1025
    elif case == "domain_rest":
        sh[3] = 1024
    elif case == "domain_lone":
        args = (m[:1], np.array([1024.0]))
    elif case == "negative":
        sh[2] = -1
    elif case == "length":
        args = (m, sh[:5])
    elif case == "zero_frames":
        args = (m[:0], sh[:0])
    elif case == "niters0":
        kw["niters"] = 0
    elif case == "niters_float":
        kw["niters"] = 2.5
    elif case == "init_str":
        kw["phase_init"] = "min"
    elif case == "init_shape":
        kw["phase_init"] = np.zeros((6, 1024))
    elif case == "win":
        kw["win_func"] = np.hamming
    elif case == "fft_len":
        args = (_mag(H=1000), sh)
    if case == "mixed_N":
        with pytest.raises(ValueError):
            mp.griffin_lim_batch([(m, sh), (_mag(H=513), sh)], niters=2)
        return
    state = np.random.get_state()[2]
    with pytest.raises(ValueError):
        mp.griffin_lim(*args, niters=kw.pop("niters", 2), **kw)
    assert np.random.get_state()[2] == state   # nothing drawn


def test_domain_edges_are_accepted():
    v, N = hm.griffin_lim_shifts(_mag(), [1024, 1023, 0, 1023, 3, 1022.6])
    assert N == 2048 and v.tolist() == [1024, 1023, 0, 1023, 3, 1023]
    assert hm.griffin_lim_shifts(_mag()[:1], [1023.4])[0].tolist() == [1023]


def test_plan_tables_match_windowing_and_ola_bookkeeping():
    rng = np.random.RandomState(7)
    utts = []
    for fs, n in ((16000, 9), (48000, 7), (16000, 1), (48000, 12)):
        N = 4096 if fs == 48000 else 2048
        utts.append((N, np.r_[rng.randint(0, N // 2 + 1), rng.randint(0, N // 2, n - 1)].astype(np.int64)))
    for N in (2048, 4096):
        shifts = [s for n, s in utts if n == N]
        r = hm.griffin_lim_plan(shifts, N)
        for u, s in enumerate(shifts):
            v_pm = np.cumsum(s)
            frames = np.random.RandomState(u).randn(s.size, N)
            v_sig = orc.ola(frames, v_pm)
            assert r["out_len"][u] == v_sig.size
            a, b = r["frame_off"][u], r["frame_off"][u + 1]
            pm_plus, left, right, _ = orc.frame_bounds(v_pm, v_sig.size)
            np.testing.assert_array_equal(r["frame_pos"][a:b], pm_plus[1:-1] + r["out_off"][u])
            np.testing.assert_array_equal(r["frame_left"][a:b], left)
            np.testing.assert_array_equal(r["frame_right"][a:b], right)
            rel, start, out_len = hm.ola_plan(v_pm, N)
            np.testing.assert_array_equal(r["pm_rel"][u], rel)
            # out[t] = sum frame_i[t + start - rel_i] with start = N/2 - pm_0: frame i's centre N/2 lands on t = pm_i, so
            # the frame tables of the next analysis index this output directly
            assert r["out_start"][u] == start == N // 2 - v_pm[0]
            np.testing.assert_array_equal(rel - start + N // 2, v_pm)
            # and the model's own analysis of the model's signal cuts the frames these tables describe
            fr = orc.windowing(v_sig, v_pm)[0]
            for f in range(s.size):
                p0 = r["frame_pos"][a + f] - r["out_off"][u]
                assert fr[f].size == r["frame_left"][a + f] + r["frame_right"][a + f] + 1
                seg = v_sig[p0 - r["frame_left"][a + f]:p0 + r["frame_right"][a + f] + 1]
                np.testing.assert_allclose(fr[f], seg * orc.half_windows(r["frame_left"][a + f], r["frame_right"][a + f]))
        assert r["out_off"][-1] == sum(r["out_len"])


def _synth_model(mag, re, im):
    """fp64 model of the existing lossless synthesis: fftshift(ifft(hermitian(mag . phasor / |phasor|)))."""
    ph = re + 1j * im
    a = np.abs(ph)
    a[a == 0] = 1.0
    return np.fft.fftshift(np.fft.ifft(orc.hermitian_full_spectrum(mag * ph / a)).real, axes=1)


@pytest.mark.parametrize("init", ["random", "linear", "min_phase", "ndarray"])
def test_initial_fold_equals_first_synthesis_frames(init):
    rng = np.random.RandomState(11)
    F, H = 5, 1025
    N = 2 * (H - 1)
    m = np.abs(rng.randn(F, H)) + 0.01
    m[1] = 0.0
    arg = rng.uniform(-np.pi, np.pi, (F, H)) if init == "ndarray" else init
    np.random.seed(5)
    ph_full = glm.initial_phase(m, arg.copy() if init == "ndarray" else arg)
    ref = np.fft.ifft(orc.add_hermitian_half_real(m) * np.exp(1j * ph_full)).real
    np.random.seed(5)
    if init == "min_phase":   # the device computes these phasors (mpx_min_phase); the host folds their angles
        ph, full = np.angle(orc.build_min_phase_from_mag_spec(m)), False
    else:
        ph, full = hm.griffin_lim_initial_phase(arg, m)
    mag, re, im = hm.griffin_lim_fold(m, ph, full)
    got = _synth_model(mag, re, im)
    assert np.max(np.abs(got - ref)) <= 1e-12


def test_initial_phase_mutates_caller_array_like_reference():
    g = _golden()
    F, H = g["16k_mag"].shape
    init = _ndarray_init((F, H), 16000)
    out, full = hm.griffin_lim_initial_phase(init, g["16k_mag"])
    assert not full and out is init
    np.testing.assert_array_equal(init, g["16k_ndarray_1_init_after"])


def _circ(a, b, w):
    d = np.angle(np.exp(1j * (np.asarray(a, np.float64) - np.asarray(b, np.float64))))
    return float(np.sum(w * np.abs(d)) / np.sum(w))


def test_fp64_model_equals_reference_golden():
    g = _golden()
    for key in g["cases"]:
        key = str(key)
        tag, rest = key.split("_", 1)
        init_name, niters = rest.rsplit("_", 1)
        fs = 16000 if tag == "16k" else 48000
        m, sh = g[tag + "_mag"], g[tag + "_shift"]
        np.random.seed(SEED)
        arg = _ndarray_init(m.shape, fs) if init_name == "ndarray" else init_name
        v_sig, ph = glm.griffin_lim(m, sh, arg, int(niters))
        ref = g[key + "_sig"]
        assert v_sig.shape == ref.shape, key
        assert np.max(np.abs(v_sig - ref)) <= 1e-10 * np.max(np.abs(ref)), key
        if key + "_phase" in g.files:
            # float32-stored phase: weighted by the magnitude the phase multiplies (ill-conditioned bins weigh little)
            assert _circ(ph, g[key + "_phase"], m) <= 1e-6, key
        if init_name == "random":
            assert np.random.get_state()[2] == int(g[key + "_rng_pos"]), key


def test_cabi_argument_errors():
    lib = _lib.load()
    args = [None, 4096, None, None, None, None, None, 5, None, None, 1, None, None, 1, None, None, None, None, 2049]
    a = list(args)
    a[1] = 1000
    assert lib.mpx_griffin_lim_ola(*a) == -1 and b"fft_len" in lib.mpx_last_error()
    a = list(args)
    a[18] = 2048
    assert lib.mpx_griffin_lim_ola(*a) == -1 and b"ld" in lib.mpx_last_error()
    a = list(args)
    a[7] = -1
    assert lib.mpx_griffin_lim_ola(*a) == -1 and b"negative" in lib.mpx_last_error()
    assert lib.mpx_griffin_lim_ola(*args) == -1 and b"null" in lib.mpx_last_error()
    buf = (ctypes.c_float * 4)()
    p = ctypes.addressof(buf)
    a = [None, 4096] + [p] * 16 + [2049]
    a[7], a[10], a[13] = 5, 1, 1
    a[15] = None   # phase_out may be null
    a[17] = a[3]   # sig_out == sig_in
    assert lib.mpx_griffin_lim_ola(*a) == -1 and b"different" in lib.mpx_last_error()
    a = list(args)
    a[7] = 0
    assert lib.mpx_griffin_lim_ola(*a) == 0
