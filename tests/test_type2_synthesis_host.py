"""
CPU: the host side of synthesis_from_compressed_type2 -- the numpy model (tests/type2_synthesis_model.py) against the
real reference's signals and rms_noise (tests/golden/g17_type2_synthesis.npz), the transform-free rms identity, the
host tables of the device path against the model's direct computation, the elliptic output filter's sections and
blocked scan, the public functions' argument checks and the C entries' argument errors.
"""
import os

import numpy as np
import pytest
from scipy import signal

import type2_synthesis_model as t2s
from magphase_amd import _lib
from magphase_amd import engine as eng
from magphase_amd import hostmath as hm
from magphase_amd import magphase as mp

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# As tests/test_oracle_vs_golden.py's WAVE_TOL, for the reason given there: bit-identical on the machine that wrote the
# golden; elsewhere other BLAS / FFT kernels change last bits that exp(), the gain and the recursive filter amplify.
WAVE_TOL = 1e-6
golden, case_inputs, n_cases = t2s.golden, t2s.case_inputs, t2s.n_cases


def test_golden_has_every_case_the_feature_was_specified_with():
    g17, _ = golden()
    names = [str(n) for n in g17["names"]]
    assert names == ["48k_var", "48k_5ms", "48k_4ms", "16k_var", "16k_5ms", "16k_4ms", "16k_hf2", "16k_nowin",
                     "16k_n4096", "16k_n1024"]
    assert len(set(int(s) for s in g17["seeds"])) == len(names)
    assert str(g17["norm_mag_equals"]) == "16k_var"
    for n in names:
        nv, nf = int(g17[n + "_nvoi"]), int(g17[n + "_nfrm"])
        assert nv >= 10 and nf - nv >= 10


def test_model_against_reference_signals_and_rms():
    g17, g16 = golden()
    for i in range(n_cases(g17)):
        name, feats, fs, kw, seed = case_inputs(g17, g16, i)
        np.random.seed(seed)
        sig, dbg = t2s.synthesis(*feats, fs, **kw)
        ref = g17[name + "_sig"]
        assert sig.shape == ref.shape, name
        d = np.max(np.abs(sig - ref)) / np.max(np.abs(ref))
        rel_forms = abs(dbg["rms_spec"] - dbg["rms_ident"]) / dbg["rms_spec"]
        rel_gold = abs(dbg["rms_spec"] - float(g17[name + "_rms"])) / float(g17[name + "_rms"])
        print("%s: |d|/peak %.3g, rms forms %.3g, rms vs golden %.3g" % (name, d, rel_forms, rel_gold))
        assert d <= WAVE_TOL, name
        assert rel_forms <= 1e-13, name
        assert rel_gold <= 1e-10, name
        assert dbg["nfrms"] == int(g17[name + "_nfrm"]) and int(dbg["v_voi"].sum()) == int(g17[name + "_nvoi"]), name


@pytest.mark.parametrize("fs,N,hf", [(48000, 4096, 1.0), (16000, 2048, 2.0), (16000, 1024, 0.5), (48000, 2048, 1.0)])
def test_bin_curves_against_model(fs, N, hf):
    got = hm.type2_synthesis_bin_curves(fs, N, hf)
    want = t2s.bin_curves(fs, N, hf)
    for a, b in zip(got, want):
        assert a.shape == (N // 2 + 1,) and a.dtype == np.float64
        assert np.max(np.abs(a - b)) <= 1e-12
    per_v, ap_v, _ = got
    # what the kernel's n_per promise rests on: zero from the crossfade's upper edge on / below its lower edge
    n_per = eng._first_all_zero_from(per_v.astype(np.float32))
    assert np.all(per_v[n_per:] == 0) and per_v[n_per - 1] > 0
    assert n_per == eng._first_all_zero_from(np.asarray(hm.synthesis_bin_curves(fs, N)[0], dtype=np.float32))
    lo = int(np.flatnonzero(ap_v)[0])
    assert np.all(ap_v[:lo] == 0) and np.all(per_v[:lo] == 1)


@pytest.mark.parametrize("phase_dim,mag_dim", [(45, 60), (10, 60), (60, 60), (70, 60), (1, 4)])
def test_phase_unwarp_matrix_against_model(phase_dim, mag_dim):
    H, alpha = 1025, hm.define_alpha(16000)
    u = hm.type2_phase_unwarp_matrix(phase_dim, mag_dim, H, alpha)
    assert u.shape == (phase_dim, H)
    assert np.max(np.abs(u - t2s.phase_unwarp_matrix(phase_dim, mag_dim, H, alpha))) <= 1e-12
    x = np.random.RandomState(3).randn(7, phase_dim)
    want = t2s.phase_unwarp(x, x, mag_dim, H, alpha)[0]
    assert np.max(np.abs(x @ u - want)) <= 1e-12 * max(1.0, np.max(np.abs(want)))


def _blockwise(x, sos, pm, g, block):
    """The blocked scan of mpx_output_hpf on the host, float64: per section, every block from a zero state, the block
    end states chained with A^block, the free response G[n] . z_start added."""
    y = np.asarray(x, dtype=np.float64)
    for sec in range(2):
        b0, b1, b2, a0, a1, a2 = sos[sec]
        b0, b1, b2, a1, a2 = b0 / a0, b1 / a0, b2 / a0, a1 / a0, a2 / a0
        out = np.zeros_like(y)
        z_start = np.zeros(2)
        pmat = pm[sec].reshape(2, 2)
        for s in range(0, y.size, block):
            z0 = z1 = 0.0
            blk = y[s:s + block]
            for n, xv in enumerate(blk):
                yv = b0 * xv + z0
                z0 = b1 * xv + z1 - a1 * yv
                z1 = b2 * xv - a2 * yv
                out[s + n] = yv + g[sec, n] @ z_start
            z_start = pmat @ z_start + np.array([z0, z1])
        y = out
    return y


def test_hpf_tables_designs():
    block = 256
    for fs in (16000, 48000):
        sos, pm, g = hm.hpf_tables(fs, block, "ellip60")
        want = signal.ellip(4, 0.5, 80, 60 / (fs / 2.0), btype="highpass", output="sos")
        assert np.array_equal(sos, want)
        x = np.random.RandomState(fs).uniform(-1, 1, 5 * block + 77)
        y = _blockwise(x, sos, pm, g, block)
        ref = signal.sosfilt(sos, x)
        peak = np.max(np.abs(ref))
        assert np.max(np.abs(y - ref)) <= 1e-9 * peak
        b, a = signal.ellip(4, 0.5, 80, 60 / (fs / 2.0), btype="highpass")
        print("ellip60 @ %d Hz: cascade vs direct-form lfilter %.3g of peak, largest table entry %.3g"
              % (fs, np.max(np.abs(y - signal.lfilter(b, a, x))) / peak, max(np.max(np.abs(pm)), np.max(np.abs(g)))))
        # the default design's tables are today's
        d0, d1 = hm.hpf_tables(fs, block), hm.hpf_tables(fs, block, "butter40")
        bsos = np.ascontiguousarray(signal.butter(4, 40 / (fs / 2.0), btype="highpass", output="sos"))
        assert np.array_equal(d0[0], bsos)
        for t0, t1 in zip(d0, d1):
            assert np.array_equal(t0, t1)
    with pytest.raises(ValueError):
        hm.hpf_tables(48000, block, "cheby")


def test_numpy_planner_tables_equal_the_model():
    g17, g16 = golden()
    for i in range(n_cases(g17)):
        name, feats, fs, kw, _ = case_inputs(g17, g16, i)
        N = kw["fft_len"] or hm.define_fft_len(fs)
        rate = kw["const_rate_ms"]
        r = eng.plan_synthesis_numpy([feats[3]], fs, N, rate > 0, kw["b_voi_ap_win"],
                                     const_rate_ms=rate if rate > 0 else 5.0, type2=True)
        v_shift, v_pm, v_voi, v_locs, ns_len = t2s.frame_tables(feats[3], fs, rate)
        assert np.array_equal(r["v_shift"], v_shift) and np.array_equal(r["v_pm"], v_pm), name
        assert np.array_equal(r["voiced"].astype(bool), v_voi) and int(r["ns_len"][0]) == ns_len, name
        assert np.array_equal(r["wtype"].astype(bool), v_voi & kw["b_voi_ap_win"]), name
    # the defaults are the type-1 planner's: same tables with and without the new arguments
    lf0 = np.asarray(g16["16k_b_c2_lf0"], dtype=np.float64)
    a = eng.plan_synthesis_numpy([lf0], 16000, 2048, True, True)
    b = eng.plan_synthesis_numpy([lf0], 16000, 2048, True, True, const_rate_ms=5.0, type2=False)
    assert all(np.array_equal(a[k], b[k]) for k in a)


def test_type2_grid_voicing_counts_f0_above_zero():
    # lf0 = 0 (f0 = 1 Hz) is unvoiced for type 1 (f0 > 1) and would be voiced on the type-2 grid (f0 > 0, :1511); its
    # shift of fs samples is longer than any frame, so the planner refuses it -- as the reference's arithmetic does
    lf0 = np.r_[np.full(30, np.log(100.0)), 0.0, np.full(30, np.log(100.0))]
    with pytest.raises(ValueError):
        eng.plan_synthesis_numpy([lf0], 16000, 2048, True, True, const_rate_ms=5.0, type2=True)


def _utt(rows=20, mag_dim=60, phase_dim=45, lf0=None):
    rs = np.random.RandomState(0)
    return (rs.randn(rows, mag_dim), rs.randn(rows, phase_dim), rs.randn(rows, phase_dim),
            np.full(rows, np.log(120.0)) if lf0 is None else lf0)


def test_argument_checks_raise_before_any_device_work():
    good = _utt()
    assert mp.synthesis_from_compressed_type2_batch([], 48000) == []
    bad = [
        (good[0][0], good[1], good[2], good[3]),                       # mag not 2-D
        (good[0], good[1][:-1], good[2], good[3]),                     # row counts differ
        (good[0], good[1], good[2], good[3][:-1]),                     # len(v_lf0) differs
        (good[0], good[1], good[2][:, :-1], good[3]),                  # real / imag widths differ
        _utt(rows=1),                                                  # fewer than two synthesis frames
        _utt(lf0=np.r_[np.full(19, np.log(120.0)), np.nan]),           # non-finite lf0
        _utt(lf0=np.r_[np.full(19, np.log(120.0)), -np.inf]),
    ]
    for u in bad:
        with pytest.raises(ValueError, match=r"utts\[1\]"):
            mp.synthesis_from_compressed_type2_batch([good, u], 48000)
    with pytest.raises(ValueError, match="fft_len"):
        mp.synthesis_from_compressed_type2_batch([good], 48000, fft_len=512)
    with pytest.raises(ValueError, match="const_rate_ms"):
        mp.synthesis_from_compressed_type2_batch([good], 48000, const_rate_ms=float("nan"))
    with pytest.raises(ValueError, match="const_rate_ms"):
        mp.synthesis_from_compressed_type2(*good, 48000, const_rate_ms="5")
    with pytest.raises(ValueError, match="hf_slope_coeff"):
        mp.synthesis_from_compressed_type2(*good, 48000, hf_slope_coeff=float("inf"))


def test_signature_is_the_references():
    import inspect

    sig = inspect.signature(mp.synthesis_from_compressed_type2)
    assert list(sig.parameters) == ["m_mag_mel_log", "m_real_mel", "m_imag_mel", "v_lf0", "fs", "fft_len",
                                    "hf_slope_coeff", "b_voi_ap_win", "b_norm_mag", "v_lgain", "const_rate_ms"]
    d = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(fft_len=None, hf_slope_coeff=1.0, b_voi_ap_win=True, b_norm_mag=False, v_lgain=None,
                     const_rate_ms=-1.0)
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "_shim_magphase", os.path.join(os.path.dirname(GOLDEN), os.pardir, "src", "magphase.py"))
    shim = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(shim)
    assert shim.synthesis_from_compressed_type2 is mp.synthesis_from_compressed_type2


def test_c_entries_argument_errors_without_gpu():
    lib = _lib.load()
    rc = lib.mpx_noise_power(None, 1234, None, None, None, None, None, 5, None)
    assert rc == -1 and b"fft_len" in lib.mpx_last_error()
    rc = lib.mpx_noise_power(None, 2048, None, None, None, None, None, 5, None)
    assert rc == -1 and b"null" in lib.mpx_last_error()
    assert lib.mpx_noise_power(None, 2048, None, None, None, None, None, 0, None) == 0
    rc = lib.mpx_noise_rms(None, 1000, None, None, 3, None, None)
    assert rc == -1 and b"fft_len" in lib.mpx_last_error()
    rc = lib.mpx_noise_rms(None, 4096, None, None, 3, None, None)
    assert rc == -1 and b"null" in lib.mpx_last_error()
    assert lib.mpx_noise_rms(None, 4096, None, None, 0, None, None) == 0
    args = [None] * 19 + [None, 7, None, None, 7, None, None, 2112, 0]
    rc = lib.mpx_synthesis_compressed_type2_ola(None, 1234, None, *args)
    assert rc == -1 and b"fft_len" in lib.mpx_last_error() and b"type2" in lib.mpx_last_error()
    rc = lib.mpx_synthesis_compressed_type2_ola(None, 4096, None, *args)
    assert rc == -1 and b"null" in lib.mpx_last_error()
    args[20] = 0   # n_runs == 0 (no frames): nothing to do
    assert lib.mpx_synthesis_compressed_type2_ola(None, 4096, None, *args) == 0
    # the type-1 entry's messages still carry its own name
    rc = lib.mpx_synthesis_compressed_ola(None, 1234, None, *args)
    assert rc == -1 and lib.mpx_last_error().startswith(b"mpx_synthesis_compressed_ola: fft_len")
