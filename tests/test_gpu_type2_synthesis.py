"""GPU: synthesis_from_compressed_type2 (mpx_mel_unwarp_rows with the type-2 phase matrix, k_noise_power + k_noise_rms,
the type-2 arm of k_synth_comp_pair, k_ola_fixup, the elliptic output high-pass) against the reference's golden signals
(tests/golden/g17_type2_synthesis.npz, inputs from g16_type2.npz) and the float64 model (tests/type2_synthesis_model.py).
No frame, sample or utterance is left out of any comparison.

Wherever the model is used, the device signal is compared twice: before the output filter (plan.run(), float32, against
the model's v_pre_hpf: the high-pass has 80 dB of stop band and would hide an error at DC and the low bins, where type 2
differs from type 1) and after it; and every utterance's device rms against the model's, in batches too.

T2S_PCM_TOL and T2S_RMS_TOL are <= 3 x the worst case measured on the MI355X over every comparison of this file
(tests/_tol.py records it; profiles/r13_type2_chain_tolerance_report.json): measured 4.5e-7 of the signal's peak (229
comparisons, before and after the filter) and 5.1e-10 relative (118 comparisons).  Their ceilings, from which on a
difference is a bug to find and not a number to loosen, are 2e-6 (type 1's COMP_PCM_TOL, whose chain this is with a
float64 gain) and 1e-6.
"""
import os

import numpy as np
import pytest

import type2_synthesis_model as t2s
from _tol import note, within
from magphase_amd import hostmath as hm
from magphase_amd import libaudio as la
from magphase_amd import magphase as mp

pytestmark = pytest.mark.gpu
golden, case_inputs, n_cases = t2s.golden, t2s.case_inputs, t2s.n_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T2S_PCM_TOL = 1.3e-6  # |d| / peak of the signal, before and after the output filter (measured 4.5e-7)
T2S_RMS_TOL = 1.5e-9  # relative: float64 sums over float32 noise samples (measured 5.1e-10)
UNV_LF0 = -1.0e10     # la.f0_to_lf0 of an unvoiced frame


def _engine():
    from magphase_amd.engine import get_engine
    return get_engine()


def _rel(sig, ref):
    assert sig.shape == ref.shape
    return np.max(np.abs(sig - ref)) / np.max(np.abs(ref))


def _f32_noise(seed, n):
    """Uniform noise that float32 holds exactly: the device and the float64 model then read the same samples."""
    return np.random.RandomState(seed).uniform(-1, 1, n).astype(np.float32).astype(np.float64)


def _check_against_model(utts, fs, noise, kw, independence=True):
    """One batch: every utterance's pre-filter signal (plan.run()), filtered signal and rms against the float64 model fed
    with the same noise; the public batch call gives the plan's filtered signal bit for bit and, with `independence`, each
    utterance alone gives what it gives in the batch.  Returns the public call's signals."""
    from magphase_amd.engine import Type2SynthesisPlan
    e = _engine()
    plan = Type2SynthesisPlan(e, utts, fs, noise=noise, **kw)
    pre_dev = plan.run()
    assert str(pre_dev.dtype) == "torch.float32"
    post = e.output_hpf(pre_dev, plan.out_off_host, fs, design="ellip60").cpu().numpy()
    pre = pre_dev.cpu().numpy().astype(np.float64)
    rms, off = plan.rms, plan.out_off_host
    batch = mp.synthesis_from_compressed_type2_batch(utts, fs, noise=noise, **kw)
    assert len(batch) == len(utts) == len(rms)
    for u, x in enumerate(utts):
        ref, dbg = t2s.synthesis(*x, fs, v_noise=noise[u], **kw)
        a, b = int(off[u]), int(off[u + 1])
        d_pre, d_post = _rel(pre[a:b], dbg["v_pre_hpf"]), _rel(batch[u], ref)
        r = abs(rms[u] / dbg["rms_spec"] - 1.0)
        print("utt %d (%d frames, %d voiced): pre-filter %.3g, filtered %.3g, rms %.3g"
              % (u, dbg["nfrms"], int(dbg["v_voi"].sum()), d_pre, d_post, r))
        within(d_pre, T2S_PCM_TOL, "T2S_PCM_TOL")
        within(d_post, T2S_PCM_TOL, "T2S_PCM_TOL")
        within(r, T2S_RMS_TOL, "T2S_RMS_TOL")
        assert np.array_equal(post[a:b], batch[u])
        if independence:
            one = mp.synthesis_from_compressed_type2_batch([x], fs, noise=[noise[u]], **kw)[0]
            assert np.array_equal(one, batch[u]), "utterance %d depends on its batch" % u
    return batch


def test_golden_cases_single_utterance_call():
    from magphase_amd.engine import Type2SynthesisPlan
    g17, g16 = golden()
    note("T2S_excluded", 0)
    for i in range(n_cases(g17)):
        name, feats, fs, kw, seed = case_inputs(g17, g16, i)
        ref = g17[name + "_sig"]
        np.random.seed(seed)
        sig = mp.synthesis_from_compressed_type2(*feats, fs, **kw)
        assert sig.dtype == np.float64 and sig.shape == ref.shape, name
        d = _rel(sig, ref)
        np.random.seed(seed)
        plan = Type2SynthesisPlan(_engine(), [feats], fs, **kw)
        plan.run()
        assert plan.total_frames == int(g17[name + "_nfrm"]) and int(plan.voiced_host.sum()) == int(g17[name + "_nvoi"])
        r = abs(plan.rms[0] / float(g17[name + "_rms"]) - 1.0)
        print("%s: |d|/peak %.3g, rms rel %.3g" % (name, d, r))
        within(d, T2S_PCM_TOL, "T2S_PCM_TOL")
        within(r, T2S_RMS_TOL, "T2S_RMS_TOL")


def test_dead_arguments_are_ignored_as_in_the_reference():
    g17, g16 = golden()
    names = [str(n) for n in g17["names"]]
    i = names.index(str(g17["norm_mag_equals"]))
    name, feats, fs, kw, seed = case_inputs(g17, g16, i)
    np.random.seed(seed)
    a = mp.synthesis_from_compressed_type2(*feats, fs, **kw)
    np.random.seed(seed)
    b = mp.synthesis_from_compressed_type2(*feats, fs, b_norm_mag=True, v_lgain=np.asarray(g16["16k_b_c1_lgain"]), **kw)
    assert np.array_equal(a, b)
    within(_rel(b, g17[name + "_sig"]), T2S_PCM_TOL, "T2S_PCM_TOL")


def _synthetic_utts(g16):
    """The 16 kHz variable-rate rows with synthetic lf0 tracks: a 60 Hz voice, a 400 Hz voice (each with an unvoiced
    stretch in the middle) and an all-unvoiced utterance."""
    mag, real, imag = (np.asarray(g16["16k_b_c0_" + n], dtype=np.float64) for n in ("mag", "real", "imag"))
    n = mag.shape[0]
    out = []
    for f0 in (60.0, 400.0, None):
        lf0 = np.full(n, UNV_LF0)
        if f0 is not None:
            lf0[:n // 3] = np.log(f0)
            lf0[n // 2:] = np.log(f0 * 1.1)
        out.append((mag, real, imag, lf0))
    return out


def test_batch_against_model_and_batch_independence():
    g17, g16 = golden()
    fs = 16000
    rows = [case_inputs(g17, g16, i) for i in range(n_cases(g17))]
    # the rows of every 16 kHz case (variable rate, 5 ms grid, 4 ms grid), all read at the variable rate here: one call
    # has one rate; each case's own rate and arguments follow below
    utts = [r[1] for r in rows if r[0] in ("16k_var", "16k_5ms", "16k_4ms")]
    utts += _synthetic_utts(g16)
    noise = [_f32_noise(100 + u, t2s.frame_tables(x[3], fs, -1.0)[4]) for u, x in enumerate(utts)]
    _check_against_model(utts, fs, noise, {})
    # the constant-rate 16 kHz cases as batches of their own, and each with the other arguments of its golden case
    for name, feats, fs_, kw, _ in rows:
        if not name.startswith("16k"):
            continue
        ns = _f32_noise(7, t2s.frame_tables(feats[3], fs_, kw["const_rate_ms"])[4])
        got = _check_against_model([feats, feats], fs_, [ns, ns], kw, independence=False)
        assert np.array_equal(got[0], got[1]), name


def _lf0_track(n, f0):
    """_synthetic_utts' track: voiced, an unvoiced stretch, voiced again 10 % higher; f0 None: all unvoiced."""
    lf0 = np.full(n, UNV_LF0)
    if f0 is not None:
        lf0[:n // 3] = np.log(f0)
        lf0[n // 2:] = np.log(f0 * 1.1)
    return lf0


def _rows_for(f0, fs, rate, n_max, max_s=0.4):
    """The longest such track of at most n_max rows whose frames span at most max_s seconds."""
    if rate > 0.0:
        return _lf0_track(min(n_max, int(max_s * 1000.0 / rate)), f0)
    for n in range(n_max, 5, -1):
        lf0 = _lf0_track(n, f0)
        if t2s.frame_tables(lf0, fs, -1.0)[1][-1] <= max_s * fs:
            return lf0
    raise AssertionError("no track of six rows fits")


def _two_frame_rows(lf0, fs, rate):
    """(first row, rows) of the shortest run of rows around the middle that gives exactly two synthesis frames."""
    for k in range(2, 12):
        for a in range(lf0.size // 2 - 1, lf0.size // 2 + 8):
            try:
                if t2s.frame_tables(lf0[a:a + k], fs, rate)[0].size == 2:
                    return a, k
            except IndexError:   # a single frame: the model (and the reference) index v_pm[-2]
                pass
    raise AssertionError("no run of rows gives two frames")


def _utts_48k(g16, rate, low_f0):
    """Six short utterances on the 48 kHz golden rows of the case with this rate: the rows with their own lf0 (all of
    them, and their second half), a low and a 400 Hz synthetic voice, an all-unvoiced one and one of two frames."""
    key = "48k_b_c%d_" % t2s.RATE_CASE[rate]
    mag, real, imag, lf0 = (np.asarray(g16[key + n], dtype=np.float64) for n in ("mag", "real", "imag", "lf0"))
    n_all = mag.shape[0]
    a2, k2 = _two_frame_rows(lf0, 48000, rate)
    utts = []
    for a, track in ((0, lf0[:len(_rows_for(None, 48000, rate, n_all))]), (n_all // 2 - 8, lf0[n_all // 2 - 8:]),
                     (0, _rows_for(low_f0, 48000, rate, n_all)), (3, _rows_for(400.0, 48000, rate, n_all - 3)),
                     (0, _rows_for(None, 48000, rate, n_all)), (a2, lf0[a2:a2 + k2])):
        b = a + len(track)
        utts.append((mag[a:b], real[a:b], imag[a:b], np.array(track)))
    assert t2s.frame_tables(utts[-1][3], 48000, rate)[0].size == 2
    return utts


@pytest.mark.parametrize("win", [True, False])
@pytest.mark.parametrize("hf", [1.0, 1.7])
@pytest.mark.parametrize("rate", [-1.0, 5.0, 4.0])
def test_48k_batch_against_model(rate, hf, win):
    _, g16 = golden()
    fs = 48000
    utts = _utts_48k(g16, rate, 55.0)
    noise = [_f32_noise(200 + u, t2s.frame_tables(x[3], fs, rate)[4]) for u, x in enumerate(utts)]
    _check_against_model(utts, fs, noise, dict(const_rate_ms=rate, hf_slope_coeff=hf, b_voi_ap_win=win))


def test_48k_batch_at_fft_len_2048_against_model():
    # (two periods of a frame's neighbours have to fit fft_len / 2: the low voice is 110 Hz here)
    _, g16 = golden()
    fs = 48000
    utts = _utts_48k(g16, 5.0, 110.0)
    noise = [_f32_noise(300 + u, t2s.frame_tables(x[3], fs, 5.0)[4]) for u, x in enumerate(utts)]
    _check_against_model(utts, fs, noise, dict(const_rate_ms=5.0, fft_len=2048))


@pytest.mark.parametrize("real_value", [-1.0, 0.0])
def test_directed_sign_of_the_real_dc_and_nyquist_bins(real_value):
    """A flat magnitude with the phase coefficients real = -1, imag = 0: every periodic bin is -|X|, so a DC or Nyquist
    bin assembled from the modulus instead of the signed real part (type 1's rule) changes the pre-filter signal by about
    2 / (periodic bins) of its peak.  real = imag = 0: the periodic part vanishes (the protection of magphase.py:1561)."""
    fs, n, mag_dim, phase_dim = 16000, 40, 60, 45
    mag = np.full((n, mag_dim), -3.0)
    real, imag = np.full((n, phase_dim), real_value), np.zeros((n, phase_dim))
    utts = [(mag, real, imag, lf0) for lf0 in (np.full(n, np.log(120.0)), np.full(n, UNV_LF0), _lf0_track(n, 120.0))]
    noise = [_f32_noise(400 + u, t2s.frame_tables(x[3], fs, -1.0)[4]) for u, x in enumerate(utts)]
    _check_against_model(utts, fs, noise, {})


@pytest.mark.parametrize("rate", [5.0, 4.0, -1.0])
def test_frame_tables_equal_the_models(rate):
    from magphase_amd.engine import Type2SynthesisPlan
    g17, g16 = golden()
    for utt, fs in (("48k_b", 48000), ("16k_b", 16000)):
        key = "%s_c%d" % (utt, {-1.0: 0, 5.0: 2, 4.0: 4}[rate])
        feats = tuple(np.asarray(g16[key + "_" + n], dtype=np.float64) for n in ("mag", "real", "imag", "lf0"))
        v_shift, v_pm, v_voi, _, ns_len = t2s.frame_tables(feats[3], fs, rate)
        plan = Type2SynthesisPlan(_engine(), [feats, feats], fs, const_rate_ms=rate, noise_mode="device")
        for u in range(2):
            assert np.array_equal(plan.v_shift[u], v_shift) and np.array_equal(plan.v_pm[u], v_pm)
            assert np.array_equal(plan.v_voi[u], v_voi) and plan.ns_len[u] == ns_len


def test_device_noise_is_reproducible_and_matches_the_model_fed_with_it():
    from magphase_amd.engine import Type2SynthesisPlan
    g17, g16 = golden()
    fs = 16000
    utts = [case_inputs(g17, g16, i)[1] for i in (3,)] + _synthetic_utts(g16)
    seeds = [11, 12, 13, 14]
    a = mp.synthesis_from_compressed_type2_batch(utts, fs, noise_mode="device", noise_seeds=seeds)
    b = mp.synthesis_from_compressed_type2_batch(utts, fs, noise_mode="device", noise_seeds=seeds)
    plan = Type2SynthesisPlan(_engine(), utts, fs, noise_mode="device", noise_seeds=seeds)
    ns = plan.noise.cpu().numpy().astype(np.float64)
    off = plan.noise_off_host
    pre, out_off = plan.run().cpu().numpy().astype(np.float64), plan.out_off_host
    for u, x in enumerate(utts):
        assert np.all(np.isfinite(a[u])) and np.array_equal(a[u], b[u])
        v = ns[int(off[u]):int(off[u + 1])]
        assert v.size == plan.ns_len[u] and np.all(np.abs(v) <= 1.0)
        ref, dbg = t2s.synthesis(*x, fs, v_noise=v)
        within(_rel(a[u], ref), T2S_PCM_TOL, "T2S_PCM_TOL")
        within(_rel(pre[int(out_off[u]):int(out_off[u + 1])], dbg["v_pre_hpf"]), T2S_PCM_TOL, "T2S_PCM_TOL")
        within(abs(plan.rms[u] / dbg["rms_spec"] - 1.0), T2S_RMS_TOL, "T2S_RMS_TOL")


def test_pcm16_equals_the_host_wav_conversion(tmp_path):
    import wave
    g17, g16 = golden()
    _, feats, fs, kw, seed = case_inputs(g17, g16, 0)
    np.random.seed(seed)
    sig = mp.synthesis_from_compressed_type2_batch([feats], fs, **kw)[0]
    np.random.seed(seed)
    pcm = mp.synthesis_from_compressed_type2_batch([feats], fs, pcm16_norm=0.98, **kw)[0]
    path = str(tmp_path / "t2s.wav")
    la.write_audio_file(path, sig, fs, norm=0.98)
    with wave.open(path, "rb") as w:
        ref = np.frombuffer(w.readframes(w.getnframes()), dtype=np.int16)
    assert pcm.dtype == np.int16 and np.array_equal(pcm, ref)


def _third_octave_lsd(x, y, fs):
    """Log-spectral distance (dB, rms over bands) of the 1/3-octave band energies of two signals, 100 Hz .. fs/2.5."""
    n = min(x.size, y.size)
    fx, fy = np.abs(np.fft.rfft(x[:n])) ** 2, np.abs(np.fft.rfft(y[:n])) ** 2
    f = np.fft.rfftfreq(n, 1.0 / fs)
    d = []
    fc = 100.0
    while fc * 2 ** (1 / 6.0) < fs / 2.5:
        band = (f >= fc / 2 ** (1 / 6.0)) & (f < fc * 2 ** (1 / 6.0))
        d.append(10 * np.log10(np.sum(fx[band]) / np.sum(fy[band])))
        fc *= 2 ** (1 / 3.0)
    return float(np.sqrt(np.mean(np.square(d))))


@pytest.mark.parametrize("rate", [-1.0, 5.0])
def test_round_trip_on_a_bundled_recording(rate):
    wav = os.path.join(ROOT, "demos", "data_48k", "wavs_nat", "hvd_593.wav")
    v_sig, fs = la.read_audio_file(wav)
    mp.use_builtin_epoch_tracker()
    try:
        r = mp.analysis_compressed_type2(wav, const_rate_ms=rate)
    finally:
        mp.set_epoch_provider(None)
    np.random.seed(1)
    y = mp.synthesis_from_compressed_type2(r[0], r[1], r[2], r[3], fs, const_rate_ms=rate)
    np.random.seed(1)   # v_noise=None: the model draws the same stream where the reference draws it
    ref, _ = t2s.synthesis(r[0], r[1], r[2], r[3], fs, const_rate_ms=rate, v_noise=None)
    within(_rel(y, ref), T2S_PCM_TOL, "T2S_PCM_TOL")
    assert abs(y.size - v_sig.size) <= hm.define_fft_len(fs), (y.size, v_sig.size)
    lsd = _third_octave_lsd(y, v_sig, fs)
    note("T2S_roundtrip_lsd_db_rate_%g" % rate, round(lsd, 3))
    assert np.isfinite(lsd)


def test_type1_and_type2_plans_leave_nothing_behind_for_each_other():
    from magphase_amd.engine import CompressedSynthesisPlan, Type2SynthesisPlan
    g17, g16 = golden()
    _, feats, fs, _, _ = case_inputs(g17, g16, 0)
    e = _engine()
    ns = [_f32_noise(3, t2s.frame_tables(feats[3], fs, -1.0)[4])]
    p1 = CompressedSynthesisPlan(e, [feats], fs, noise=ns)
    p2 = Type2SynthesisPlan(e, [feats], fs, noise=ns)
    a1 = p1.run().cpu().numpy().copy()
    a2 = p2.run().cpu().numpy().copy()
    b1 = p1.run().cpu().numpy().copy()
    b2 = p2.run().cpu().numpy().copy()
    assert np.array_equal(a1, b1) and np.array_equal(a2, b2)
    assert not np.array_equal(a1, a2)
    assert p1.per_v.data_ptr() != p2.per_v.data_ptr() and p1.u_phase.data_ptr() != p2.u_phase.data_ptr()
    assert p1._buffers()["inv_gain"].data_ptr() != p2._buffers()["inv_gain"].data_ptr()
    # and a fresh type-1 plan built after the type-2 one computes what the first did
    c1 = CompressedSynthesisPlan(e, [feats], fs, noise=ns).run().cpu().numpy()
    assert np.array_equal(a1, c1)
