"""
-m gpu: the round-trip launch with compact-support frames taking their class instances (LosslessRoundTripPlan's default at
fft_len 4096) against the same launch with every frame in the full class (MAGPHASE_RT_SUPPORT=full) and against the oracle.

A frame's feature rows come out of the forward transform, whose pruned first stages return what the full stages return for
zero operands: the three matrices must be EQUAL under both settings.  The waveform loses the rounding residue the full
inverse transform adds outside a frame's support: it agrees with the full form's to PCM_TOL and stays within the existing
round-trip bound of the oracle.  48 kHz (N = 4096); hand-built epoch lists put L and R on both sides of the class limits
(L <= 512, R <= 511) and of the next multiple of the row length, narrow and wide frames next to each other in one run.
"""
import warnings

import numpy as np
import pytest

from _tol import note, within

pytestmark = pytest.mark.gpu

PCM_TOL = 1e-6       # of the signal peak: tests/test_gpu_lossless.py
FS = 48000


def _utt_from_gaps(gaps, seed, first=300):
    """Noise with an impulse at every epoch; the epochs `first`, first + gaps[0], ... (samples).  Frame i has
    L = the gap before epoch i and R = the gap after it."""
    pos = first + np.concatenate(([0], np.cumsum(gaps)))
    n = int(pos[-1]) + 700
    rng = np.random.RandomState(seed)
    x = 0.05 * rng.randn(n)
    x[pos] += 0.4
    pcm = np.round(np.clip(x, -0.99, 0.99) * 32767.0).astype(np.int16)
    return pcm, FS, (pos + 0.25) / FS, np.ones(pos.size)


def _edge_batch():
    # every (L, R) with both values out of the list, narrow and wide neighbours in both orders
    vals = [511, 512, 513, 1023, 1024, 1025]
    gaps = []
    for a in vals:
        for b in vals:
            gaps += [a, b]
    gaps += [300, 513, 300, 300, 1025, 200, 200, 511, 512, 511, 240, 1420, 171]
    rng = np.random.RandomState(9)
    x = (rng.uniform(-0.5, 0.5, 30000) * 32767).astype(np.int16)
    pm_long = np.array([0.0, 0.01, 0.02, 0.15, 0.16, 0.4]) + 1e-4    # gaps of 6 240 and 11 520 samples: frames longer than N
    pm0 = np.array([0.0, 0.004, 0.009, 0.015, 0.02])                   # first epoch at sample 0: L = 0
    return [_utt_from_gaps(np.asarray(gaps), 1), (x, FS, pm_long, np.ones(pm_long.size)),
            (x[:2000], FS, pm0, np.array([1.0, 1, 0, 0, 1])),
            (np.zeros(4000, dtype=np.int16), FS, np.arange(1, 16) * 0.005, np.zeros(15)),      # silence
            (x[:1500], FS, np.array([0.005, 0.012]), np.ones(2))]


def _utterance_batch():
    from magphase_amd import synthetic as syn
    out = []
    for u in range(3):
        pcm, pm, voi = syn.make_utterance(500 + u, dur_s=0.5 + 0.1 * u, fs=FS)
        out.append((pcm, FS, pm, voi))
    return out


_BATCHES = {"edges": _edge_batch, "utterances": _utterance_batch}
_ORACLE = {}


def _oracle(name):
    """The oracle's copy synthesis per utterance of a batch, computed once."""
    if name not in _ORACLE:
        from oracle import magphase_oracle as orc
        out = []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for pcm, fs, pm, voi in _BATCHES[name]():
                o = orc.analysis_lossless_from_epochs(pcm.astype(np.float64) / 32768.0, fs, pm, voi)
                out.append(orc.synthesis_from_lossless(o[0], o[1], o[2], o[3], fs))
        _ORACLE[name] = out
    return _ORACLE[name]


def _plan(monkeypatch, support, utts, **kw):
    from magphase_amd.engine import LosslessRoundTripPlan, get_engine
    if support == "full":
        monkeypatch.setenv("MAGPHASE_RT_SUPPORT", "full")
    else:
        monkeypatch.delenv("MAGPHASE_RT_SUPPORT", raising=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        p = LosslessRoundTripPlan(get_engine(), utts, **kw)
    assert p.full_support == (support == "full")
    return p


def _run(plan):
    import torch
    feats, pcm = plan.run()
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in feats], pcm.cpu().numpy()


def _compare(monkeypatch, name, label, **kw):
    utts = _BATCHES[name]()
    pd, pf = _plan(monkeypatch, "default", utts, **kw), _plan(monkeypatch, "full", utts, **kw)
    assert pd.synthesis.runs_host.tobytes() == pf.synthesis.runs_host.tobytes()
    fd, yd = _run(pd)
    ff, yf = _run(pf)
    for a, b in zip(fd, ff):
        assert a.shape == b.shape and np.array_equal(a, b)
    peak = max(np.max(np.abs(yf)), 1e-30)
    within(np.max(np.abs(yd - yf)) / peak, PCM_TOL, "PCM_TOL:roundtrip-support-vs-full" + label)
    worst = {"class": 0.0, "full": 0.0}
    for u, ref in enumerate(_oracle(name)):
        sl = slice(pd.out_off_host[u], pd.out_off_host[u + 1])
        assert len(yd[sl]) == len(ref)
        scale = max(np.max(np.abs(ref)), 1e-30)
        worst["class"] = max(worst["class"], np.max(np.abs(yd[sl].astype(np.float64) - ref)) / scale)
        worst["full"] = max(worst["full"], np.max(np.abs(yf[sl].astype(np.float64) - ref)) / scale)
    print("%s%s: max |pcm - oracle| / peak: class instances %.3g, full class %.3g; class vs full %.3g"
          % (name, label, worst["class"], worst["full"], np.max(np.abs(yd - yf)) / peak))
    note("roundtrip-support oracle error, full class " + name + label, worst["full"])
    within(worst["class"], 2 * PCM_TOL, "PCM_TOL:roundtrip-support-vs-oracle" + label)
    # two runs identical
    fd2, yd2 = _run(pd)
    assert np.array_equal(yd, yd2) and all(np.array_equal(a, b) for a, b in zip(fd, fd2))
    return pd


@pytest.mark.parametrize("n_slots", [None, 12])
def test_class_limits_narrow_and_wide_neighbours_and_edge_frames(monkeypatch, n_slots):
    """L and R at 511 / 512 / 513 / 1023 / 1024 / 1025 in every combination, L = 0, frames longer than N, silence, an
    utterance of two frames; with the engine's slots (fewer frames than slots: one frame per run at the seams) and with 12
    slots (runs of a dozen frames that mix the classes)."""
    from magphase_amd import hostmath as hm
    pd = _compare(monkeypatch, "edges", "" if n_slots is None else "-12slots", n_slots=n_slots)
    left, right = pd.analysis._host_tabs[1], pd.analysis._host_tabs[2]
    pairs = set(zip(left.tolist(), right.tolist()))
    for a in (511, 512, 513, 1023, 1024, 1025):
        for b in (511, 512, 513, 1023, 1024, 1025):
            assert (a, b) in pairs, (a, b)
    assert int(left.min()) == 0 and int((left + right + 1).max()) > 4096
    cls = hm.roundtrip_support_classes(left, right, pd.fft_len)
    assert set(np.unique(cls).tolist()) == {4, 16}
    assert np.any(cls[:-1] != cls[1:])           # classes change inside a run
    if n_slots is None:
        assert pd.total_frames < pd.engine.synth_comp_slots()
    else:
        assert pd.synthesis.n_slots == 12


@pytest.mark.parametrize("fpr", [1, 7, None])
def test_utterance_batch_at_several_run_lengths(monkeypatch, fpr):
    pd = _compare(monkeypatch, "utterances", "-fpr%s" % fpr, frames_per_run=fpr)
    assert pd.fft_len == 4096


def test_16k_batch_has_only_the_full_class(monkeypatch):
    """fft_len 2048 (P = 16): no narrow class -- both switch settings launch the same kernel instance and give the very
    same rows and samples, within the existing bound of the oracle."""
    from magphase_amd import hostmath as hm, synthetic as syn
    from oracle import magphase_oracle as orc
    utts = []
    for u in range(2):
        pcm, pm, voi = syn.make_utterance(520 + u, dur_s=0.5, fs=16000)
        utts.append((pcm, 16000, pm, voi))
    pd, pf = _plan(monkeypatch, "default", utts), _plan(monkeypatch, "full", utts)
    assert pd.fft_len == 2048
    assert np.all(hm.roundtrip_support_classes(pd.analysis._host_tabs[1], pd.analysis._host_tabs[2], 2048) == 8)
    fd, yd = _run(pd)
    ff, yf = _run(pf)
    assert np.array_equal(yd, yf) and all(np.array_equal(a, b) for a, b in zip(fd, ff))
    for u, (pcm, fs, pm, voi) in enumerate(utts):
        o = orc.analysis_lossless_from_epochs(pcm.astype(np.float64) / 32768.0, fs, pm, voi)
        ref = orc.synthesis_from_lossless(o[0], o[1], o[2], o[3], fs)
        yu = yd[pd.out_off_host[u]:pd.out_off_host[u + 1]].astype(np.float64)
        within(np.max(np.abs(yu - ref)) / np.max(np.abs(ref)), 2 * PCM_TOL, "PCM_TOL:roundtrip")
