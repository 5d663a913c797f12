"""GPU: synthesis_from_compressed_type2 (mpx_mel_unwarp_rows with the type-2 phase matrix, k_noise_power + k_noise_rms,
the type-2 arm of k_synth_comp_pair, k_ola_fixup, the elliptic output high-pass) against the reference's golden signals
(tests/golden/g17_type2_synthesis.npz, inputs from g16_type2.npz) and the float64 model (tests/type2_synthesis_model.py).
No frame, sample or utterance is left out of any comparison.

T2S_PCM_TOL and T2S_RMS_TOL are NOT yet three times a measured worst case: no MI355X run of this file exists.  They are
the bounds from which on a difference counts as a finding (the signal: type 1's COMP_PCM_TOL, whose chain this is with
a float64 gain; the rms: 1e-6 relative, four orders above what float64 sums over float32 samples should leave).  The
first green run has to tighten them to <= 3 x the figures of the session's tolerance report (tests/_tol.py) and note those here.
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
T2S_PCM_TOL = 2e-6    # |d| / peak of the signal: type 1's chain with a float64 gain (COMP_PCM_TOL's value); not measured yet
T2S_RMS_TOL = 1e-6    # relative: float64 sums over float32 noise samples; not measured yet
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
    batch = mp.synthesis_from_compressed_type2_batch(utts, fs, noise=noise)
    assert len(batch) == len(utts)
    for u, x in enumerate(utts):
        ref, dbg = t2s.synthesis(*x, fs, v_noise=noise[u])
        within(_rel(batch[u], ref), T2S_PCM_TOL, "T2S_PCM_TOL")
        one = mp.synthesis_from_compressed_type2_batch([x], fs, noise=[noise[u]])[0]
        assert np.array_equal(one, batch[u]), "utterance %d depends on its batch" % u
    # the constant-rate 16 kHz cases as batches of their own, and each with the other arguments of its golden case
    for name, feats, fs_, kw, _ in rows:
        if not name.startswith("16k"):
            continue
        ns = _f32_noise(7, t2s.frame_tables(feats[3], fs_, kw["const_rate_ms"])[4])
        got = mp.synthesis_from_compressed_type2_batch([feats, feats], fs_, noise=[ns, ns], **kw)
        ref, _ = t2s.synthesis(*feats, fs_, v_noise=ns, **kw)
        within(_rel(got[0], ref), T2S_PCM_TOL, "T2S_PCM_TOL")
        assert np.array_equal(got[0], got[1]), name


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
    for u, x in enumerate(utts):
        assert np.all(np.isfinite(a[u])) and np.array_equal(a[u], b[u])
        v = ns[int(off[u]):int(off[u + 1])]
        assert v.size == plan.ns_len[u] and np.all(np.abs(v) <= 1.0)
        ref, _ = t2s.synthesis(*x, fs, v_noise=v)
        within(_rel(a[u], ref), T2S_PCM_TOL, "T2S_PCM_TOL")


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
    assert np.all(np.isfinite(y))
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
