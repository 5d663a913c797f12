"""CPU: host side of the constant-rate lossless analysis / synthesis (no GPU).

The scan with an explicit capacity (mpx_host_const_to_var_scan_cap) against the reference-capped native scan and the
scipy model; the synthesis plan's scan, row tables, voicing and f0 against the reference composition
(tests/const_rate_lossless_model.py), including an utterance past the reference's 2n-slot cap; the analysis f0 against
oracle.to_const_rate; the model against the reference's own output (golden G14); argument errors before any device
call; the new C-ABI symbols declared, bound and documented."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import const_rate_lossless_model as model  # noqa: E402

from magphase_amd import _lib, engine as eng, hostmath as hm  # noqa: E402
from magphase_amd import magphase as mp  # noqa: E402
from magphase_amd import synthetic as syn  # noqa: E402
from oracle import magphase_oracle as orc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g14_const_rate_lossless.npz")
NEW_SYMBOLS = ("mpx_synthesis_lossless_ola_lerp", "mpx_rows_lerp", "mpx_host_const_to_var_scan_cap")


def _f0_track(n, lo, hi, seed, unvoiced=0.2):
    rng = np.random.RandomState(seed)
    f0 = lo + (hi - lo) * (0.5 + 0.5 * np.sin(np.linspace(0, 3, n) + rng.rand()))
    f0[rng.rand(n) < unvoiced] = 0.0
    return f0


def _const_rate_feats(u, fs, cr, dur=0.4):
    pcm, pm_sec, voi = syn.make_utterance(u, dur_s=dur, fs=fs)
    o = orc.analysis_lossless_from_epochs(syn.pcm_to_float(pcm), fs, pm_sec, voi)
    return orc.to_const_rate(o[0], o[1], o[2], o[3], o[5], fs, cr)


@pytest.mark.parametrize("fs,cr,lo,hi", [(16000, 5.0, 70, 180), (48000, 5.0, 90, 300), (48000, 2.5, 100, 380),
                                         (16000, 10.0, 60, 190), (22050, 7.5, 80, 250)])
def test_capacity_scan_equals_the_reference_scan_below_its_cap(fs, cr, lo, hi):
    for seed in range(6):
        n = 20 + 37 * seed
        shift_c = hm.f0_to_shift(_f0_track(n, lo, hi, seed), fs)
        ref = eng._const_to_variable_scan(shift_c, cr, fs)          # mpx_host_const_to_var_scan (2n slots)
        assert ref[0].size < 2 * n, "case chosen below the cap"
        new = eng.const_to_variable_scan_uncapped(shift_c, cr, fs)
        assert np.array_equal(new[0], ref[0]) and np.array_equal(new[1], ref[1])
        lit = model.scan(shift_c, cr, fs)                            # one scipy interp1d call per step
        assert np.array_equal(new[0], lit[0]) and np.array_equal(new[1], lit[1])


def test_capacity_scan_runs_past_the_reference_cap():
    fs, cr, n = 48000, 10.0, 40
    shift_c = hm.f0_to_shift(np.full(n, 260.0), fs)   # 2.6 frames per constant-rate frame
    capped = eng._const_to_variable_scan(shift_c, cr, fs)
    lit_capped = model.scan(shift_c, cr, fs, capped=True)
    assert capped[0].size == 2 * n and capped[0][0] == 0.0 and capped[1][0] == 0.0   # the head lost, slot 0 left at 0
    assert np.array_equal(capped[0], lit_capped[0])
    new = eng.const_to_variable_scan_uncapped(shift_c, cr, fs)
    lit = model.scan(shift_c, cr, fs)
    assert np.array_equal(new[0], lit[0]) and np.array_equal(new[1], lit[1])
    assert new[0].size > 2 * n and new[1][0] - new[0][0] < fs * cr / 1000   # to the start of the grid
    # the tail (what the reference keeps past slot 0) is the same scan
    assert np.array_equal(new[0][-(2 * n - 1):], capped[0][1:]) and np.array_equal(new[1][-(2 * n - 1):], capped[1][1:])


def test_capacity_scan_native_errors():
    lib = _lib.load()
    c = np.array([240.0, 480.0, 720.0])
    v = np.array([100.0, 100.0, 100.0])
    out = np.empty(4)
    assert lib.mpx_host_const_to_var_scan_cap(c.ctypes.data, v.ctypes.data, 3, out.ctypes.data, out.ctypes.data, 0) == -1
    o1, o2 = np.empty(2), np.empty(2)
    assert lib.mpx_host_const_to_var_scan_cap(c.ctypes.data, v.ctypes.data, 3, o1.ctypes.data, o2.ctypes.data, 2) == -2
    assert eng.const_to_variable_scan_uncapped(np.zeros(0), 5.0, 16000)[0].size == 0
    s, l_ = eng.const_to_variable_scan_uncapped(np.array([90.0]), 5.0, 16000)
    assert np.array_equal(s, [90.0]) and np.array_equal(l_, [80.0])


@pytest.mark.parametrize("u,fs,cr_a,cr_s", [(7, 16000, 5.0, 5.0), (6, 48000, 5.0, 10.0), (1, 16000, 2.5, 2.5),
                                             (3, 48000, 5.0, 10.0), (7, 48000, 2.5, 7.5)])
def test_synthesis_tables_against_the_composition(u, fs, cr_a, cr_s):
    """Scan, voicing and f0 exact; the row tables are scipy's bracketing and reproduce its interpolation."""
    mag_c, real_c, imag_c, f0_c = _const_rate_feats(u, fs, cr_a)
    r = eng.plan_const_rate_synthesis([f0_c], [fs], cr_s)
    _, v_shift, v_locs, v_f0, rows = model.synthesis(mag_c, real_c, imag_c, f0_c, fs, cr_s)
    assert r["live"] == [0]
    assert np.array_equal(r["v_shift"][0], v_shift) and np.array_equal(r["v_locs"][0], v_locs)
    assert np.array_equal(r["v_f0"][0], v_f0)
    centres = (fs * cr_s / 1000) * np.arange(1, f0_c.size + 1)
    idx = np.clip(np.searchsorted(centres, v_locs), 1, f0_c.size - 1)
    assert np.array_equal(r["row0"], idx - 1) and np.array_equal(r["row1"], idx)
    assert np.all((r["rowt"] >= 0) & (r["rowt"] <= 1))
    for m_c, m_v in zip((mag_c, real_c, imag_c), rows):
        t = r["rowt"][:, None]
        lerp = (1 - t) * m_c[r["row0"]] + t * m_c[r["row1"]]
        assert np.max(np.abs(lerp - m_v)) <= 1e-12 * max(1.0, np.max(np.abs(m_v)))


def test_synthesis_tables_past_the_reference_cap():
    """Pitch-shifted x 1.5 and stretched to 10 ms: the reference's scan would lose the head; ours covers the grid."""
    fs, cr = 48000, 10.0
    mag_c, real_c, imag_c, f0_c = _const_rate_feats(3, fs, 5.0)
    f0_c = f0_c * 1.5
    assert model.cap_hit(f0_c, cr, fs)
    r = eng.plan_const_rate_synthesis([f0_c], [fs], cr)
    _, v_shift, v_locs, v_f0, _ = model.synthesis(mag_c, real_c, imag_c, f0_c, fs, cr)
    assert np.array_equal(r["v_shift"][0], v_shift) and np.array_equal(r["v_f0"][0], v_f0)
    assert v_shift.size > 2 * f0_c.size - 1


def test_synthesis_tables_batch_offsets_and_empty_utterances():
    fs = 16000
    a = _const_rate_feats(7, fs, 5.0)[3]
    b = _const_rate_feats(2, fs, 5.0)[3]
    r = eng.plan_const_rate_synthesis([a, np.zeros(0), b, np.array([150.0])], [fs] * 4, 5.0)
    assert r["live"] == [0, 2, 3] and r["n_rows"] == [a.size, 0, b.size, 1]
    ra = eng.plan_const_rate_synthesis([a], [fs], 5.0)
    rb = eng.plan_const_rate_synthesis([b], [fs], 5.0)
    na, nb = ra["row0"].size, rb["row0"].size
    assert np.array_equal(r["row0"][:na], ra["row0"]) and np.array_equal(r["row0"][na:na + nb], rb["row0"] + a.size)
    assert np.array_equal(r["row1"][na + nb:], [a.size + b.size])   # the single row
    assert np.array_equal(r["v_f0"][1], rb["v_f0"][0])   # (lists over the live utterances)


@pytest.mark.parametrize("fs,cr", [(16000, 5.0), (48000, 5.0), (16000, 2.5), (48000, 2.5)])
def test_analysis_f0_and_tables_against_to_const_rate(fs, cr):
    pcm, pm_sec, voi = syn.make_utterance(7, dur_s=0.4, fs=fs)
    o = orc.analysis_lossless_from_epochs(syn.pcm_to_float(pcm), fs, pm_sec, voi)
    ref = orc.to_const_rate(o[0], o[1], o[2], o[3], o[5], fs, cr)
    v_pm = np.cumsum(o[5])
    assert np.array_equal(eng._const_rate_f0_voi(o[3], v_pm, fs, cr), ref[3])
    lo, hi, t = hm.var_to_const_rate_table(v_pm, cr, fs)
    lerp = (1 - t[:, None]) * o[0][lo] + t[:, None] * o[0][hi]
    assert lerp.shape == ref[0].shape and np.max(np.abs(lerp - ref[0])) <= 1e-12 * np.max(ref[0])


def test_model_matches_the_reference_golden():
    """The composition model equals the reference's own synthesis (golden G14): on the oracle's rows of the stored
    utterances, which equal the reference's stored columns (model.golden_rows checks them)."""
    g = np.load(GOLDEN)
    for tag in g["tags"]:
        tag = str(tag)
        fs = int(g[tag + "_fs"])
        rows = model.golden_rows(g, tag)
        for rate in g[tag + "_rates"]:
            key = "%s_syn%g" % (tag, rate)
            v_syn, v_shift, v_locs, _, _ = model.synthesis(*rows, fs, float(rate))
            assert np.array_equal(v_shift, g[key + "_shift"]) and np.array_equal(v_locs, g[key + "_locs"])
            assert v_syn.size == g[key].size
            assert np.max(np.abs(v_syn - g[key])) <= 1e-9 * np.max(np.abs(g[key]))


def test_batch_tables_against_the_reference_golden():
    """hostmath.var_to_const_rate_batch (the three constant-rate analysis plans' tables) on golden G14's utterances as
    one batch: f0 is the reference's, exactly; the rows, offset by each utterance's base, interpolate the oracle's
    variable-rate rows to the reference's stored columns (the bound of model.golden_rows)."""
    g = np.load(GOLDEN)
    tags, cr, step = [str(t) for t in g["tags"]], float(g["const_rate_ms"]), int(g["col_step"])
    fs_list = [int(g[t + "_fs"]) for t in tags]
    o = [orc.analysis_lossless_from_epochs(syn.pcm_to_float(g[t + "_pcm"]), fs, g[t + "_pm_sec"], g[t + "_voi"])
         for t, fs in zip(tags, fs_list)]
    bases = np.concatenate(([0], np.cumsum([x[0].shape[0] for x in o])))
    row0, row1, rowt, f0, out_off = hm.var_to_const_rate_batch([x[5] for x in o], [x[3] for x in o], bases[:-1], fs_list, cr)
    assert row0.dtype == row1.dtype == out_off.dtype == np.int64 and rowt.dtype == np.float64
    assert np.array_equal(out_off, np.concatenate(([0], np.cumsum([g[t + "_f0"].size for t in tags]))))
    for u, t in enumerate(tags):
        a, b = int(out_off[u]), int(out_off[u + 1])
        assert np.array_equal(f0[u], g[t + "_f0"])
        lo, hi, w = hm.var_to_const_rate_table(np.cumsum(o[u][5]), cr, fs_list[u])
        assert np.array_equal(row0[a:b], lo + bases[u]) and np.array_equal(row1[a:b], hi + bases[u])
        assert np.array_equal(rowt[a:b], w)
        mag = o[u][0][:, ::step]
        lerp = (1 - w[:, None]) * mag[row0[a:b] - bases[u]] + w[:, None] * mag[row1[a:b] - bases[u]]
        pk = np.max((1 - w[:, None]) * o[u][0][lo] + w[:, None] * o[u][0][hi], axis=1, keepdims=True)
        assert np.max(np.abs(lerp - g[t + "_mag"]) / pk) <= 1e-6
    one = hm.var_to_const_rate_batch([o[0][5]], [o[0][3]], [0], fs_list[0], cr)   # one rate for the batch: a scalar fs
    assert np.array_equal(one[0], row0[:int(out_off[1])]) and np.array_equal(one[3][0], f0[0])
    empty = hm.var_to_const_rate_batch([], [], [], 16000, cr)
    assert empty[0].size == 0 and empty[3] == [] and np.array_equal(empty[4], [0])


def test_argument_errors_before_any_device_call():
    pcm, pm_sec, voi = syn.make_utterance(1, dur_s=0.2, fs=16000)
    utt = (syn.pcm_to_float(pcm), 16000, pm_sec, voi)
    for bad in (0.0, -5.0, float("nan"), float("inf"), "5"):
        with pytest.raises(ValueError):
            mp.analysis_lossless_const_rate_batch([utt], const_rate_ms=bad)
        with pytest.raises(ValueError):
            mp.synthesis_from_lossless_const_rate_batch([(np.ones((3, 513)),) * 3 + (np.zeros(3), 16000)],
                                                        const_rate_ms=bad)
    m = np.ones((4, 513))
    with pytest.raises(ValueError, match="rows"):   # f0 / row count mismatch
        mp.synthesis_from_lossless_const_rate(m, m, m, np.zeros(5), 16000)
    with pytest.raises(ValueError):                 # mag / real / imag of different shapes
        mp.synthesis_from_lossless_const_rate(m, m[:3], m, np.zeros(4), 16000)
    with pytest.raises(ValueError, match="bin count"):
        mp.synthesis_from_lossless_const_rate_batch([(m, m, m, np.zeros(4), 16000),
                                                     (np.ones((4, 2049)),) * 3 + (np.zeros(4), 48000)])
    with pytest.raises(ValueError):                 # not 1024 / 2048 / 4096 points
        mp.synthesis_from_lossless_const_rate(np.ones((4, 100)), np.ones((4, 100)), np.ones((4, 100)), np.zeros(4), 16000)
    with pytest.raises(ValueError, match="v_f0"):   # negative / non-finite f0
        mp.synthesis_from_lossless_const_rate(m, m, m, np.array([100.0, -1.0, 0.0, 0.0]), 16000)
    with pytest.raises(ValueError, match="v_f0"):
        mp.synthesis_from_lossless_const_rate(m, m, m, np.array([100.0, np.nan, 0.0, 0.0]), 16000)
    assert mp.analysis_lossless_const_rate_batch([]) == [] and mp.synthesis_from_lossless_const_rate_batch([]) == []


def test_new_symbols_declared_bound_and_documented():
    hdr = open(os.path.join(ROOT, "include", "magphase_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert s + "(" in hdr and s in _lib.SYMBOLS and s in doc, s
        assert getattr(lib, s).argtypes, s
    for name in ("analysis_lossless_const_rate_batch", "analysis_lossless_const_rate",
                 "synthesis_from_lossless_const_rate_batch", "synthesis_from_lossless_const_rate"):
        assert callable(getattr(mp, name))
    sys.path.insert(0, os.path.join(ROOT, "src"))
    try:
        import magphase as shim
        assert shim.synthesis_from_lossless_const_rate_batch is mp.synthesis_from_lossless_const_rate_batch
    finally:
        sys.path.remove(os.path.join(ROOT, "src"))
