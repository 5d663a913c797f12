"""
-m gpu: the round trip with its frames dealt to the slots by cost (LosslessRoundTripPlan's default) against the same launch
with the shares by count (MAGPHASE_RT_DEAL=count) and against the oracle.

A frame's feature rows do not depend on the slot that analysed it, so the three matrices must be BIT-identical under both
dealings -- a frame skipped or done twice shows there; the waveform's run seams lie elsewhere, so it agrees to PCM_TOL.
Small slot counts (n_slots=12 / 6) put several runs, long and short frames and all three age classes into a batch of a
few hundred frames.
"""
import numpy as np
import pytest

from _tol import within

pytestmark = pytest.mark.gpu

PCM_TOL = 1e-6       # of the signal peak: tests/test_gpu_lossless.py


def _utt(kind, fs, dur=0.5, seed=0):
    """0.5 s of noise with an impulse at every epoch.  kind: f0 in Hz (voiced at that constant pitch) or None (unvoiced:
    an epoch every 5 ms, the epoch tracker's convention)."""
    rng = np.random.RandomState(100 + seed)
    n = int(round(dur * fs))
    step = 0.005 if kind is None else 1.0 / float(kind)
    pm = np.round(np.arange(1, int((n - 3) / fs / step)) * step + 1e-4, 6)
    x = 0.05 * rng.randn(n)
    x[np.round(pm * fs).astype(int)] += 0.4
    pcm = np.round(np.clip(x, -0.99, 0.99) * 32767.0).astype(np.int16)
    voi = np.zeros(pm.size) if kind is None else np.ones(pm.size)
    return pcm, fs, pm, voi


def _batch(fs):
    return [_utt(70.0, fs, seed=1), _utt(300.0, fs, seed=2), _utt(None, fs, seed=3)]


def _plan(monkeypatch, deal, utts, **kw):
    from magphase_amd.engine import LosslessRoundTripPlan, get_engine
    if deal == "count":
        monkeypatch.setenv("MAGPHASE_RT_DEAL", "count")
    else:
        monkeypatch.delenv("MAGPHASE_RT_DEAL", raising=False)
    return LosslessRoundTripPlan(get_engine(), utts, **kw)


def _run(plan):
    import torch
    feats, pcm = plan.run()
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in feats], pcm.cpu().numpy()


@pytest.fixture(scope="module")
def oracle_pcm():
    """The oracle's copy synthesis per (fs, utterance), computed once."""
    from oracle import magphase_oracle as orc
    cache = {}

    def get(fs):
        if fs not in cache:
            out = []
            for pcm, fs_, pm, voi in _batch(fs):
                o = orc.analysis_lossless_from_epochs(pcm.astype(np.float64) / 32768.0, fs_, pm, voi)
                out.append(orc.synthesis_from_lossless(o[0], o[1], o[2], o[3], fs_))
            cache[fs] = out
        return cache[fs]
    return get


@pytest.mark.parametrize("fs,n_slots", [(48000, 12), (16000, 6), (8000, 6)])
def test_cost_dealing_matches_count_dealing_and_the_oracle(monkeypatch, oracle_pcm, fs, n_slots):
    utts = _batch(fs)
    pc = _plan(monkeypatch, "count", utts, n_slots=n_slots)
    pk = _plan(monkeypatch, "cost", utts, n_slots=n_slots)
    assert pc.deal == "count" and pk.deal == "cost"
    assert pc.fft_len == pk.fft_len == {48000: 4096, 16000: 2048, 8000: 1024}[fs]
    assert pc.synthesis.n_slots == pk.synthesis.n_slots == n_slots
    if fs == 48000:    # the 70 Hz utterance's frames (1 373 samples) take the second sample tile
        left, right = pk.analysis._host_tabs[1], pk.analysis._host_tabs[2]
        assert np.max(left + right + 1) > 1024
    # every frame in exactly one run under the cost dealing
    seen = np.zeros(pk.total_frames, dtype=np.int64)
    for r in pk.synthesis.runs_host:
        seen[r["frame_begin"]:r["frame_end"]] += 1
    assert np.all(seen == 1)
    fc, yc = _run(pc)
    fk, yk = _run(pk)
    for a, b in zip(fc, fk):
        assert a.shape == b.shape and np.array_equal(a, b)
    assert yc.shape == yk.shape
    within(np.max(np.abs(yk - yc)) / np.max(np.abs(yc)), PCM_TOL, "PCM_TOL:roundtrip-deal-vs-count")
    for u, ref in enumerate(oracle_pcm(fs)):
        yu = yk[pk.out_off_host[u]:pk.out_off_host[u + 1]].astype(np.float64)
        assert len(yu) == len(ref)
        within(np.max(np.abs(yu - ref)) / np.max(np.abs(ref)), 2 * PCM_TOL, "PCM_TOL:roundtrip")


def test_fewer_frames_than_slots_fall_back_to_count_dealing(monkeypatch):
    """The engine's own slot count (six per compute unit) against a batch of a few hundred frames: the plan deals by count,
    and gives what it gives under MAGPHASE_RT_DEAL=count."""
    utts = _batch(48000)
    pk = _plan(monkeypatch, "cost", utts)
    pc = _plan(monkeypatch, "count", utts)
    assert pk.total_frames < pk.engine.synth_comp_slots()
    assert pk.deal == "count" and pc.deal == "count"
    assert pk.synthesis.runs_host.tobytes() == pc.synthesis.runs_host.tobytes()
    fk, yk = _run(pk)
    fc, yc = _run(pc)
    for a, b in zip(fc, fk):
        assert np.array_equal(a, b)
    assert np.array_equal(yk, yc)


def test_empty_batch(monkeypatch):
    pk = _plan(monkeypatch, "cost", [])
    feats, pcm = pk.run()
    assert pk.total_frames == 0 and pk.deal == "count"
    assert all(int(t.shape[0]) == 0 for t in feats) and int(pcm.numel()) == 0
