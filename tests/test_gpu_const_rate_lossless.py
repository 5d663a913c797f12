"""GPU: lossless features on a constant frame rate -- analysis_lossless_const_rate_batch (k_analysis -> k_rows_lerp) and
synthesis_from_lossless_const_rate_batch (the LERP arm of k_synth_ola_pair; the staged form k_rows_lerp ->
k_synth_ola_pair as the cross-check) against the reference's golden (tests/golden/g14_const_rate_lossless.npz), the
oracle (oracle.to_const_rate) and the fp64 composition model (tests/const_rate_lossless_model.py).

Tolerances are <= 3 x the worst case measured on the MI355X (tests/_tol.py records it).  No frame is left out; real /
imag are compared on the bins test_gpu_lossless.py compares them on (above 1e-5 of the frame peak), in both source rows
of a constant-rate row, with that file's bound interpolated between the two rows."""
import os

import numpy as np
import pytest

import const_rate_lossless_model as model
from _tol import within
from magphase_amd import hostmath as hm
from magphase_amd import synthetic as syn
from oracle import magphase_oracle as orc

pytestmark = pytest.mark.gpu

CR_MAG_TOL = 1.2e-6      # |d mag_c| / ((1-t) peak_r0 + t peak_r1); measured 4.1e-7
CR_REAL_IMAG_TOL = 3e-7  # (|d real_c| - 2e-7) / ((1-t) peak_r0/|X_r0| + t peak_r1/|X_r1|); measured 1.0e-7
CR_PCM_TOL = 1e-6        # synthesis from given rows, / signal peak (test_gpu_lossless.py's PCM_TOL); measured 4.0e-7
CR_RT_TOL = 1.8e-6       # analysis -> synthesis, / signal peak; measured 6.3e-7
CR_MAG_GOLDEN_TOL = 8e-7  # the same at the golden's stored bins, vs the reference's rows; measured 2.6e-7
CR_PCM_GOLDEN_TOL = 8.5e-7  # synthesis from the golden utterance's rows vs the reference's signal, / peak; measured 2.8e-7
CR_ROWS_TOL = 4e-7       # device-interpolated variable-rate rows vs the fp64 composition's, / the stream's peak
# The fused LERP arm and the staged form run the same float32 operations on the same rows: equal, sample for sample.


def _mp():
    from magphase_amd import magphase as mp
    return mp


def _golden(golden_dir):
    return np.load(os.path.join(golden_dir, "g14_const_rate_lossless.npz"))


def _utt(u, fs, dur):
    pcm, pm_sec, voi = syn.make_utterance(u, dur_s=dur, fs=fs)
    return (syn.pcm_to_float(pcm), fs, pm_sec, voi)


def _check_rows(got, utt, cr, fft_len=None, label=""):
    """got: (mag, real, imag, f0) constant-rate rows against oracle.to_const_rate of the oracle's analysis."""
    x, fs, pm_sec, voi = utt
    o = orc.analysis_lossless_from_epochs(x, fs, pm_sec, voi, fft_len)
    ref = orc.to_const_rate(o[0], o[1], o[2], o[3], o[5], fs, cr)
    assert np.array_equal(np.asarray(got[3]), ref[3])
    m, re, im = [np.asarray(g, dtype=np.float64) for g in got[:3]]
    assert m.shape == ref[0].shape
    if m.shape[0] == 0:
        return
    lo, hi, t = hm.var_to_const_rate_table(np.cumsum(o[5]), cr, fs)
    t = t[:, None]
    pk = np.max(o[0], axis=1, keepdims=True)
    pk[pk == 0] = 1.0
    den = (1 - t) * pk[lo] + t * pk[hi]
    within(np.max(np.abs(m - ref[0]) / den), CR_MAG_TOL, "CR_MAG_TOL" + label)
    big = (o[0][lo] > 1e-5 * pk[lo]) & (o[0][hi] > 1e-5 * pk[hi])
    amp = ((1 - t) * pk[lo] / np.maximum(o[0][lo], 1e-300) + t * pk[hi] / np.maximum(o[0][hi], 1e-300))[big]
    within(np.max((np.abs(re - ref[1])[big] - 2e-7) / amp), CR_REAL_IMAG_TOL, "CR_REAL_IMAG_TOL" + label)
    within(np.max((np.abs(im - ref[2])[big] - 2e-7) / amp), CR_REAL_IMAG_TOL, "CR_REAL_IMAG_TOL" + label)


def _pcm_err(v, r):
    assert len(v) == len(r)
    return np.max(np.abs(np.asarray(v) - r)) / max(np.max(np.abs(r)), 1e-30)


# ------------------------------------------------------------------------------------------------- analysis
def test_analysis_against_golden(golden_dir):
    g = _golden(golden_dir)
    cr = float(g["const_rate_ms"])
    for tag in g["tags"]:
        tag = str(tag)
        fs = int(g[tag + "_fs"])
        utt = (syn.pcm_to_float(g[tag + "_pcm"]), fs, g[tag + "_pm_sec"], g[tag + "_voi"])
        a = _mp().analysis_lossless_const_rate_batch([utt], const_rate_ms=cr)[0]
        assert a[4] == fs and np.array_equal(a[3], g[tag + "_f0"])
        full = model.golden_rows(g, tag)   # every bin; the golden keeps every col_step-th (the reference's values)
        assert a[0].shape == full[0].shape
        ref_mag = g[tag + "_mag"].astype(np.float64)
        pk = np.max(full[0], axis=1, keepdims=True)
        within(np.max(np.abs(a[0][:, ::int(g["col_step"])] - ref_mag) / pk), CR_MAG_GOLDEN_TOL, "CR_MAG_GOLDEN_TOL")
        _check_rows(a[:4], utt, cr)


@pytest.mark.parametrize("cr", [5.0, 2.5])
def test_analysis_mixed_batch_against_oracle(cr):
    utts = [_utt(7, 16000, 0.5), _utt(6, 48000, 0.4), _utt(2, 16000, 0.3), _utt(3, 48000, 0.7)]
    out = _mp().analysis_lossless_const_rate_batch(utts, fft_len=4096, const_rate_ms=cr)
    for a, u in zip(out, utts):
        assert a[4] == u[1]
        _check_rows(a[:4], u, cr, fft_len=4096)


def test_analysis_return_device_equals_host():
    utts = [_utt(7, 48000, 0.4), _utt(1, 48000, 0.3)]
    h = _mp().analysis_lossless_const_rate_batch(utts, const_rate_ms=5.0)
    d = _mp().analysis_lossless_const_rate_batch(utts, const_rate_ms=5.0, return_device=True)
    for a, b in zip(h, d):
        for k in range(3):
            assert np.array_equal(a[k], b[k].cpu().numpy().astype(np.float64))
        assert np.array_equal(a[3], b[3])


def test_analysis_zero_and_single_frame_and_unvoiced():
    fs = 16000   # 5 ms = 80 samples: the grid is arange(80, pm[-1], 80)
    x = np.random.RandomState(3).uniform(-0.3, 0.3, 400)
    zero = (x, fs, np.array([30, 60]) / fs, np.array([1.0, 1.0]))
    one = (x, fs, np.array([40, 90, 150]) / fs, np.array([1.0, 1.0, 1.0]))
    a0, a1 = _mp().analysis_lossless_const_rate_batch([zero, one], const_rate_ms=5.0)
    H = hm.define_fft_len(fs) // 2 + 1
    assert a0[0].shape == (0, H) and a0[3].size == 0
    assert a1[0].shape == (1, H)
    _check_rows(a1[:4], one, 5.0)
    with pytest.raises(IndexError):   # no voiced frame: what analysis_compressed_batch(b_const_rate=True) raises
        _mp().analysis_lossless_const_rate_batch([_utt(4, 16000, 0.3)])


# ------------------------------------------------------------------------------------------------- synthesis
def test_synthesis_against_golden_and_composition(golden_dir):
    g = _golden(golden_dir)
    for tag in g["tags"]:
        tag = str(tag)
        fs = int(g[tag + "_fs"])
        feats = model.golden_rows(g, tag)[:3]   # the oracle's rows of the stored utterance (= the reference's)
        for rate in g[tag + "_rates"]:
            key = "%s_syn%g" % (tag, rate)
            v = _mp().synthesis_from_lossless_const_rate(*feats, g[tag + "_f0"], fs, const_rate_ms=float(rate))
            within(_pcm_err(v, g[key]), CR_PCM_GOLDEN_TOL, "CR_PCM_GOLDEN_TOL")
            r = model.synthesis(*feats, g[tag + "_f0"], fs, float(rate))[0]
            within(_pcm_err(v, r), CR_PCM_TOL, "CR_PCM_TOL:model")


def test_fused_arm_equals_staged_form():
    from magphase_amd import engine as eng
    e = eng.get_engine()
    for fs, N, us in ((48000, 4096, (6, 7, 3)), (16000, 1024, (2, 7)), (16000, 2048, (1,))):
        utts = [_utt(u, fs, 0.6) for u in us]
        a = _mp().analysis_lossless_const_rate_batch(utts, fft_len=N, const_rate_ms=5.0, return_device=True)
        f0 = [x[3] for x in a]
        plan = eng.LosslessConstRateSynthesisPlan(e, f0, [fs] * len(a), N, const_rate_ms=5.0)
        cat = _mp()._feats_cat_device(e, a, N // 2 + 1)
        fused = e.to_host_f64(plan.run(*cat))
        staged = e.to_host_f64(plan.run_staged(*cat))
        assert np.array_equal(fused, staged)
        # and the staged rows are the composition's rows (float32)
        rows = e.rows_lerp(cat, plan.rows, plan.total_frames)
        o = plan.out_off_host
        for k, u in enumerate(plan.live):
            r = model.synthesis(*[x.cpu().numpy().astype(np.float64) for x in a[u][:3]], a[u][3], fs, 5.0)
            within(_pcm_err(fused[o[u]:o[u + 1]], r[0]), CR_PCM_TOL, "CR_PCM_TOL:model")
        assert rows[0].shape[0] == plan.total_frames


def test_time_stretch():
    """Analysis at 5 ms, synthesis at 10 ms: twice as long; the uncapped composition's length, frame positions and rows,
    and its samples on the rows the device interpolated.

    Against the fp64 composition's own samples one frame of (48 kHz, utterance 6) differs by 2.7e-4 of the peak: a DC or
    Nyquist phasor (real = +-1, imag = 0) interpolated between rows of opposite sign at t ~ 0.5 is ~0, and its sign --
    hence X = mag * sign -- depends on the last bit of t (float32 on the device).  The composition is discontinuous
    there; the samples are therefore compared on the device's float32 rows, the rows against the fp64 ones."""
    from magphase_amd import engine as eng
    e = eng.get_engine()
    for fs, u in ((48000, 6), (16000, 7), (48000, 3)):
        utt = _utt(u, fs, 0.6)
        a = _mp().analysis_lossless_const_rate_batch([utt], const_rate_ms=5.0)[0]
        v = _mp().synthesis_from_lossless_const_rate(*a, const_rate_ms=10.0)
        r_syn, r_shift, r_locs, r_f0, r_rows = model.synthesis(*a[:4], fs, 10.0)
        assert len(v) == len(r_syn)
        N = 2 * (a[0].shape[1] - 1)
        plan = eng.LosslessConstRateSynthesisPlan(e, [a[3]], [fs], N, const_rate_ms=10.0)
        assert np.array_equal(plan.v_locs[0], r_locs) and np.array_equal(plan.v_f0[0], r_f0)
        cat = _mp()._feats_cat_device(e, [a], N // 2 + 1)
        rows = [x.cpu().numpy().astype(np.float64) for x in e.rows_lerp(cat, plan.rows, plan.total_frames)]
        for x, y in zip(rows, r_rows):
            within(np.max(np.abs(x - y)) / np.max(np.abs(y)), CR_ROWS_TOL, "CR_ROWS_TOL")
        within(_pcm_err(v, orc.synthesis_from_lossless(rows[0], rows[1], rows[2], r_f0, fs)), CR_PCM_TOL,
               "CR_PCM_TOL:stretch")
        n_in = len(utt[0])
        assert abs(len(v) - 2 * n_in) <= 2 * (fs * 10.0 / 1000) + 2 * hm.define_fft_len(fs), (len(v), n_in)


def test_pitch_shift():
    """f0 x 1.5: the composition's frame positions, the length within one constant-rate step."""
    from magphase_amd import engine as eng
    for fs, u in ((48000, 6), (16000, 7)):
        a = _mp().analysis_lossless_const_rate_batch([_utt(u, fs, 0.6)], const_rate_ms=5.0)[0]
        f0 = a[3] * 1.5
        v0 = _mp().synthesis_from_lossless_const_rate(*a, const_rate_ms=5.0)
        v = _mp().synthesis_from_lossless_const_rate(a[0], a[1], a[2], f0, fs, const_rate_ms=5.0)
        r = model.synthesis(a[0], a[1], a[2], f0, fs, 5.0)
        host = eng.plan_const_rate_synthesis([f0], [fs], 5.0)
        assert np.array_equal(host["v_locs"][0], r[2]) and np.array_equal(host["v_shift"][0], r[1])
        within(_pcm_err(v, r[0]), CR_PCM_TOL, "CR_PCM_TOL:pitch")
        assert abs(len(v) - len(v0)) <= fs * 5.0 / 1000


@pytest.mark.parametrize("cr", [5.0, 2.5])
def test_round_trip_against_the_oracle_composition(cr):
    for fs, u in ((48000, 7), (16000, 6)):
        utt = _utt(u, fs, 0.5)
        a = _mp().analysis_lossless_const_rate_batch([utt], const_rate_ms=cr)[0]
        v = _mp().synthesis_from_lossless_const_rate(*a, const_rate_ms=cr)
        o = orc.analysis_lossless_from_epochs(*utt)
        c = orc.to_const_rate(o[0], o[1], o[2], o[3], o[5], fs, cr)
        r = model.synthesis(*c, fs, cr)[0]
        within(_pcm_err(v, r), CR_RT_TOL, "CR_RT_TOL")


def test_batch_of_different_lengths_and_rates():
    """One call: utterances of different lengths, 16 and 48 kHz (4096-point features), an empty and a one-row one."""
    utts = [_utt(7, 48000, 0.7), _utt(2, 16000, 0.25), _utt(6, 48000, 0.35), _utt(1, 16000, 0.9)]
    a = _mp().analysis_lossless_const_rate_batch(utts, fft_len=4096, const_rate_ms=5.0)
    feats = [x[:5] for x in a]
    feats.insert(2, (np.zeros((0, 2049)),) * 3 + (np.zeros(0), 48000))
    feats.append((a[0][0][:1], a[0][1][:1], a[0][2][:1], a[0][3][:1], 48000))
    batch = _mp().synthesis_from_lossless_const_rate_batch(feats, const_rate_ms=5.0)
    assert batch[2].size == 0
    for f, v in zip(feats, batch):
        one = _mp().synthesis_from_lossless_const_rate(*f, const_rate_ms=5.0) if f[3].size else np.zeros(0)
        r = model.synthesis(*[np.asarray(x, dtype=np.float64) for x in f[:4]], f[4], 5.0)[0]
        assert len(v) == len(one) == len(r)
        if len(r):
            within(_pcm_err(v, r), CR_PCM_TOL, "CR_PCM_TOL:batch")
            within(_pcm_err(one, r), CR_PCM_TOL, "CR_PCM_TOL:batch")


def test_return_device_synthesis():
    a = _mp().analysis_lossless_const_rate_batch([_utt(6, 48000, 0.4)], const_rate_ms=5.0, return_device=True)[0]
    d = _mp().synthesis_from_lossless_const_rate_batch([a[:5]], return_device=True)[0]
    h = _mp().synthesis_from_lossless_const_rate_batch([a[:5]])[0]
    assert np.array_equal(d.cpu().numpy().astype(np.float64), h)
