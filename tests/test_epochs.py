"""
Built-in epoch / voicing front end (magphase_amd/epochs.py + csrc/magphase_epochs.hip).  PARITY
UNPINNED (REAPER is an external binary that is not available): quality is measured on synthetic utterances whose epochs
are known exactly, and on the reference's ten bundled natural recordings (voicing against the phone labels; copy synthesis on two).
Device kernels: -m gpu.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _score(pm, voi, e_pm, e_voi):
    tv, ev = pm[voi > 0], e_pm[e_voi > 0]
    err = ev[np.abs(ev[None, :] - tv[:, None]).argmin(1)] - tv
    hit = float((np.abs(err) < 0.0005).mean())                                   # within 0.5 ms
    fa = float((np.abs(tv[None, :] - ev[:, None]).min(1) > 0.001).mean())        # estimated epoch with no true one within 1 ms
    return hit, fa, float(np.median(err))


def test_epochs_of_synthetic_utterances_batched():
    from magphase_amd import epochs, synthetic as syn
    for fs, us in ((48000, (0, 2, 3)), (16000, (5, 6))):
        data = [syn.make_utterance(u, dur_s=2.5, fs=fs) for u in us]
        res = epochs.track_epochs_batch([d[0] for d in data], fs)
        for (pcm, pm, voi), (e_pm, e_voi) in zip(data, res):
            assert np.all(np.diff(e_pm) > 0) and set(np.unique(e_voi)) <= {0.0, 1.0}
            assert e_pm[0] > 0 and e_pm[-1] * fs < pcm.size - 1
            hit, fa, med = _score(pm, voi, e_pm, e_voi)
            assert hit > 0.85 and fa < 0.08 and abs(med) < 0.0002, (hit, fa, med)
            # unvoiced marks every 5 ms, about as many as the generator placed (a coarse count: the voiced stretches come out
            # one or two correlation frames longer at each end; the voicing error itself is bounded by the accuracy test
            # below, 0.03 on a 5 ms grid)
            n_unv, n_unv_true = int((e_voi == 0).sum()), int((voi == 0).sum())
            assert abs(n_unv - n_unv_true) < 0.4 * n_unv_true + 10
        one = epochs.track_epochs(data[1][0], fs)                     # batching does not change the result
        assert np.array_equal(one[0], res[1][0]) and np.array_equal(one[1], res[1][1])


def test_accuracy_figures_on_synthetic_truth(capsys):
    """The figures a reader can see (DESIGN.md section 1 / profiles/r03_epoch_accuracy.json quote them): identification
    rate, miss / false-alarm rate, timing jitter, gross F0 error and voicing error of the built-in tracker on synthetic
    utterances whose epochs are known exactly, pooled per sample rate -- printed, and bounded."""
    from magphase_amd import epochs, synthetic as syn
    for fs, us in ((48000, range(20, 28)), (16000, range(30, 36))):
        data = [syn.make_utterance(u, dur_s=3.0, fs=fs) for u in us]
        res = epochs.track_epochs_batch([d[0] for d in data], fs)
        rows = [epochs.accuracy_against_truth(pm, voi, e_pm, e_voi) for (_p, pm, voi), (e_pm, e_voi) in zip(data, res)]
        w = np.array([r["true_voiced_epochs"] for r in rows], dtype=np.float64)
        pooled = {k: float(np.sum(w * np.array([r[k] for r in rows])) / w.sum())
                  for k in ("identification_rate", "miss_rate", "false_alarm_rate", "jitter_us", "bias_us",
                            "gross_f0_error_rate", "voicing_error_rate")}
        with capsys.disabled():
            print("\nepoch tracker @ %d Hz, %d utterances, %d true voiced epochs: %s"
                  % (fs, len(rows), int(w.sum()), ", ".join("%s %.4g" % kv for kv in pooled.items())))
        # measured on MI355X (profiles/r04_epoch_accuracy.json, 64 utterances of 5 s per rate): identification 0.991-0.993,
        # misses 2-8e-4, false alarms 0.007-0.008, jitter 49-50 us, |bias| 38-120 us, gross F0 errors 1e-4, voicing errors
        # 0.029-0.031, worst utterance 0.980.  (Round 3: identification 0.905-0.909, misses 8.4-8.8 % -- not at voicing
        # boundaries, as believed, but in the middle of voiced stretches whose correlation stage had locked onto the double
        # period: the spacing filter then dropped every second epoch; it now measures against the crossings' own rhythm.)
        assert pooled["identification_rate"] > 0.975 and pooled["miss_rate"] < 0.01 and pooled["false_alarm_rate"] < 0.02
        assert pooled["jitter_us"] < 120.0 and abs(pooled["bias_us"]) < 200.0
        assert pooled["gross_f0_error_rate"] < 0.005 and pooled["voicing_error_rate"] < 0.06


def test_corpus_pipeline_with_builtin_tracker_matches_sequential(tmp_path, monkeypatch):
    """the tracker runs in iobatch's READER thread (wavs without .est, MAGPHASE_EPOCHS=builtin) while the
    compute thread uses the engine's staging buffer.  The threaded corpus run with batches > 1 must write exactly the
    files a sequential, one-file-at-a-time run writes."""
    from magphase_amd import iobatch, libaudio as la, magphase as mp, synthetic as syn
    monkeypatch.setenv("MAGPHASE_EPOCHS", "builtin")
    wav_dir = tmp_path / "w"
    os.makedirs(str(wav_dir))
    wavs = []
    for u in range(7):
        pcm, _pm, _voi = syn.make_utterance(800 + u, dur_s=0.7 + 0.15 * (u % 3), fs=48000)
        f = str(wav_dir / ("t%02d.wav" % u))
        la.write_audio_file(f, pcm / 32768.0, 48000, norm=None)
        wavs.append(f)
    seq, thr = str(tmp_path / "seq"), str(tmp_path / "thr")
    monkeypatch.setenv("MAGPHASE_IO_PIPELINE", "0")
    iobatch.extract_features_corpus(wavs, seq, batch_utts=1, phase_dim=45, verbose=False)
    monkeypatch.setenv("MAGPHASE_IO_PIPELINE", "1")
    for _rep in range(3):            # a race does not show every time
        rep = iobatch.CorpusReport()
        iobatch.extract_features_corpus(wavs, thr, batch_utts=3, phase_dim=45, verbose=False, report=rep)
        assert rep["done"] == 7 and not rep.get("failed")
        for f in wavs:
            tok = os.path.basename(f)[:-4]
            for ext in (".mag", ".real", ".imag", ".lf0", ".shift"):
                a, b = open(os.path.join(seq, tok + ext), "rb").read(), open(os.path.join(thr, tok + ext), "rb").read()
                assert len(a) > 0 and a == b, tok + ext


def test_polarity_does_not_matter():
    from magphase_amd import epochs, synthetic as syn
    pcm, _pm, _voi = syn.make_utterance(1, dur_s=2.0)
    a = epochs.track_epochs(pcm.astype(np.float64) / 32768.0, 48000)
    b = epochs.track_epochs(-pcm.astype(np.float64) / 32768.0, 48000)
    assert a[0].size == b[0].size and np.allclose(a[0], b[0], atol=1.0 / 48000) and np.array_equal(a[1], b[1])


def test_noise_and_silence_are_unvoiced():
    from magphase_amd import epochs
    rng = np.random.RandomState(0)
    for sig in (0.1 * rng.randn(32000), np.zeros(32000)):
        pm, voi = epochs.track_epochs(sig, 16000)
        assert voi.sum() <= 0.02 * voi.size
        assert np.allclose(np.diff(pm)[voi[1:] + voi[:-1] == 0], 0.005, atol=1e-6)


@pytest.mark.parametrize("tok", ["hvd_593", "hvd_577"])
def test_natural_recordings_copy_synthesis(tok, tmp_path):
    """BASELINE configs[0] on the reference's own demo recordings (bundled as data): built-in epochs (opt-in), lossless
    copy synthesis reproduces the waveform, the low-dimensional copy synthesis runs, the voicing track is sane."""
    import warnings
    from magphase_amd import epochs, libaudio as la, magphase as mp
    wav = os.path.join(ROOT, "demos", "data_48k", "wavs_nat", tok + ".wav")
    x, fs = la.read_audio_file(wav)
    assert fs == 48000 and x.size > 100000
    pm, voi = epochs.track_epochs(x, fs)
    dur = x.size / fs
    v_frac = float(np.sum(np.diff(pm)[voi[1:] > 0]) / dur)
    f0 = 1.0 / np.diff(pm)[(voi[1:] > 0) & (voi[:-1] > 0)]
    assert 0.25 < v_frac < 0.85, v_frac                             # read speech: roughly half of the time is voiced
    assert 70.0 < np.median(f0) < 350.0 and np.mean((f0 > 60) & (f0 < 420)) > 0.97
    assert np.std(np.diff(np.log(f0))) < 0.15                       # consecutive periods agree (no octave hopping)
    mp.use_builtin_epoch_tracker()
    try:
        m_mag, m_real, m_imag, v_f0, fs2, v_shift = mp.analysis_lossless(wav)
        v_syn = mp.synthesis_from_lossless(m_mag, m_real, m_imag, v_f0, fs)
        n = min(x.size, v_syn.size)
        a, b = int(0.05 * n), int(0.95 * n)
        # Q2: cumsum(fs / f0) re-times ~0.01 % of the epochs by one sample; everywhere else the half windows sum to one
        err = v_syn[a:b] - x[a:b]
        assert np.median(np.abs(err)) < 1e-6 * np.max(np.abs(x))
        snr = 10 * np.log10(np.sum(x[a:b] ** 2) / np.sum(err ** 2))
        assert snr > 30.0, snr
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            c = mp.analysis_compressed(wav, mag_dim=60, phase_dim=45)
            np.random.seed(0)
            y = mp.synthesis_from_compressed(c[0], c[1], c[2], c[3], fs)
        assert np.all(np.isfinite(y)) and abs(y.size - x.size) < 0.02 * x.size
        r = np.sqrt(np.mean(y ** 2)) / np.sqrt(np.mean(x ** 2))
        assert 0.5 < r < 2.0, r
    finally:
        mp.set_epoch_provider(None)


def test_natural_recordings_against_label_voicing(capsys):
    """All ten of the reference's natural recordings (demos/data_48k/wavs_nat, bundled as data with their HTS state labels):
    the tracker's voiced / unvoiced decision against the voicing the phone identities imply (sonorants voiced, voiceless
    obstruents and silence unvoiced; voiced obstruents not scored; 15 ms margins: epochs.score_against_labels), and the
    continuity of its periods inside voiced phones.  The one natural-speech truth available offline;
    tools/epoch_natural.py writes the per-file table (profiles/r06_epoch_natural.json)."""
    from magphase_amd import epochs, libaudio as la
    d = os.path.join(ROOT, "demos", "data_48k")
    toks = sorted(f[:-4] for f in os.listdir(os.path.join(d, "wavs_nat")) if f.endswith(".wav"))
    assert len(toks) == 10
    sigs = [la.read_audio_file(os.path.join(d, "wavs_nat", t + ".wav"))[0] for t in toks]
    res = epochs.track_epochs_batch(sigs, 48000)
    rows = [epochs.score_against_labels(pm, voi, os.path.join(d, "labs", t + ".lab")) for t, (pm, voi) in zip(toks, res)]
    w = np.array([r["voiced_points"] + r["unvoiced_points"] for r in rows], dtype=np.float64)
    pooled = {k: float(np.sum(w * np.array([r[k] for r in rows])) / w.sum())
              for k in ("voiced_recall", "unvoiced_recall", "agreement", "f0_jump_rate")}
    with capsys.disabled():
        print("\nepoch tracker on the 10 natural recordings vs label voicing: %s; worst file %.3f; F0 medians %s Hz"
              % (", ".join("%s %.4f" % kv for kv in pooled.items()), min(r["agreement"] for r in rows),
                 " ".join("%.0f" % r["f0_median_hz"] for r in rows)))
    assert all(r["voiced_points"] > 80 and r["unvoiced_points"] > 80 for r in rows)
    # measured on MI355X: agreement 0.9745, voiced recall 0.9707, unvoiced recall 0.9769, worst file 0.9537, F0 jump rate
    # 0.0109 -- the figures of profiles/r06_epoch_natural.json to every printed digit.  The bounds sit 0.03 from them.
    assert pooled["agreement"] > 0.945 and pooled["voiced_recall"] > 0.941 and pooled["unvoiced_recall"] > 0.947
    assert min(r["agreement"] for r in rows) > 0.924
    assert pooled["f0_jump_rate"] < 0.04
    assert all(60.0 < r["f0_median_hz"] < 400.0 for r in rows)
