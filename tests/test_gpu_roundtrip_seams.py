"""
-m gpu: the round-trip launch with its run seams sized by what the frames add (LosslessRoundTripPlan's default at fft_len
4096) against the same launch with the seams of dense frames (MAGPHASE_RT_SEAMS=full) and against the oracle.

In the positions that change hands between a run, its successor's head strip and the fix-up, one of the two addends was an
exact zero -- a ring slot no frame touched.  The waveform must therefore be EQUAL under both settings, value for value
(only the sign of a zero may differ: compared after adding 0.0), and the feature rows, which the seams do not touch, bit
for bit.  pcm_out and the strips are filled with NaN before every launch: a kept sample nobody writes, or a strip element
the fix-up reads and nobody wrote, shows.  The batch (tests/_seams.py: seam_batch) puts narrow and dense frames on either
side of the run boundaries; tests/test_ola_seams_host.py runs the brute-force model on the same plans without a GPU.
"""
import warnings

import numpy as np
import pytest

import _seams
from _tol import within

pytestmark = pytest.mark.gpu

PCM_TOL = 1e-6       # of the signal peak: tests/test_gpu_lossless.py


@pytest.fixture(scope="module")
def oracle_pcm():
    """The oracle's copy synthesis per utterance of the seam batch, computed once."""
    from oracle import magphase_oracle as orc
    out = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for pcm, fs, pm, voi in _seams.seam_batch():
            o = orc.analysis_lossless_from_epochs(pcm.astype(np.float64) / 32768.0, fs, pm, voi)
            out.append(orc.synthesis_from_lossless(o[0], o[1], o[2], o[3], fs))
    return out


def _plan(monkeypatch, seams, utts, **kw):
    from magphase_amd.engine import LosslessRoundTripPlan, get_engine
    monkeypatch.delenv("MAGPHASE_RT_SUPPORT", raising=False)
    if seams == "full":
        monkeypatch.setenv("MAGPHASE_RT_SEAMS", "full")
    else:
        monkeypatch.delenv("MAGPHASE_RT_SEAMS", raising=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        p = LosslessRoundTripPlan(get_engine(), utts, **kw)
    assert p.full_seams == (seams == "full") and not p.full_support
    assert p.seam_geometry == ("dense" if seams == "full" else "extents")
    return p


def _run_on_nan(plan):
    """plan.run() into a pcm_out and strips that hold NaN -> (rows, pcm) on the host."""
    import torch
    e = plan.engine
    strips = e.empty((max(plan.synthesis.strip_floats, 1),)).fill_(float("nan"))
    pcm = e.empty((plan.total_out,)).fill_(float("nan"))
    feats, out = plan.run(strips=strips, out=pcm)
    torch.cuda.synchronize()
    assert out is pcm
    return [t.cpu().numpy() for t in feats], pcm.cpu().numpy()


@pytest.mark.parametrize("n_slots", [6, 12])
def test_seams_by_extents_equal_dense_seams_exactly_and_hold_the_oracle_bound(monkeypatch, oracle_pcm, n_slots):
    utts = _seams.seam_batch()
    pd = _plan(monkeypatch, "default", utts, n_slots=n_slots)
    pf = _plan(monkeypatch, "full", utts, n_slots=n_slots)
    assert pd.fft_len == 4096 and pd.synthesis.n_slots == pf.synthesis.n_slots == n_slots
    rd, rf = pd.runs_host, pf.runs_host
    assert np.array_equal(rd["frame_begin"], rf["frame_begin"]) and np.array_equal(rd["frame_end"], rf["frame_end"])
    # every kind of seam is in the run table that is launched: dense frames on either side and inside a run, a gap of
    # zeros, non-empty fix ranges clipped by the kept part's start and by its end
    kinds = _seams.plan_seam_kinds(pd)
    assert _seams.SEAM_KINDS <= kinds, (n_slots, sorted(_seams.SEAM_KINDS - kinds))
    assert np.any((rd["fix_hi"] > rd["fix_lo"]) & (rd["fix_hi"] < rd["head_end"]))     # (clip-end, seen in the table itself)
    assert pd.seams.fix_width == _seams.fix_width(rd) and pf.seams is pf.synthesis
    assert pd.synthesis.runs_host.tobytes() == rf.tobytes()      # the synthesis plan inside keeps the dense table
    assert (rd["fix_hi"] - rd["fix_lo"]).sum() < (rf["fix_hi"] - rf["fix_lo"]).sum()
    fd, yd = _run_on_nan(pd)
    ff, yf = _run_on_nan(pf)
    assert not np.isnan(yd).any() and not np.isnan(yf).any()
    assert yd.shape == yf.shape and np.array_equal(yd + np.float32(0.0), yf + np.float32(0.0))
    for a, b in zip(fd, ff):
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for u, ref in enumerate(oracle_pcm):
        sl = slice(pd.out_off_host[u], pd.out_off_host[u + 1])
        assert len(yd[sl]) == len(ref)
        scale = max(np.max(np.abs(ref)), 1e-30)
        err_d = np.max(np.abs(yd[sl].astype(np.float64) - ref)) / scale
        err_f = np.max(np.abs(yf[sl].astype(np.float64) - ref)) / scale
        print("utterance %d, %d slots: max |pcm - oracle| / peak: seams by extents %.3g, dense seams %.3g"
              % (u, n_slots, err_d, err_f))
        within(err_d, 2 * PCM_TOL, "PCM_TOL:roundtrip-seams-vs-oracle")
        within(err_f, 2 * PCM_TOL, "PCM_TOL:roundtrip-seams-vs-oracle")
    # two runs identical
    fd2, yd2 = _run_on_nan(pd)
    assert np.array_equal(yd, yd2) and all(np.array_equal(a, b) for a, b in zip(fd, fd2))


def test_2048_plan_is_the_dense_plan(monkeypatch):
    """fft_len 2048 has no narrow class: the extents are (0, N) and the run table is the one MAGPHASE_RT_SEAMS=full gives;
    the launch, its fix-up sized by that table, gives the very same samples."""
    from magphase_amd import synthetic as syn
    utts = []
    for u in range(2):
        pcm, pm, voi = syn.make_utterance(520 + u, dur_s=0.5, fs=16000)
        utts.append((pcm, 16000, pm, voi))
    pd = _plan(monkeypatch, "default", utts, n_slots=6)
    pf = _plan(monkeypatch, "full", utts, n_slots=6)
    assert pd.fft_len == 2048 and pd.synthesis.n_runs > 2
    assert pd.runs_host.tobytes() == pf.runs_host.tobytes()
    fd, yd = _run_on_nan(pd)
    ff, yf = _run_on_nan(pf)
    assert not np.isnan(yd).any()
    assert np.array_equal(yd, yf) and all(np.array_equal(a, b) for a, b in zip(fd, ff))


def test_empty_batch_and_single_frame_utterances(monkeypatch):
    pe = _plan(monkeypatch, "default", [])
    feats, pcm = pe.run()
    assert pe.total_frames == 0 and all(int(t.shape[0]) == 0 for t in feats) and int(pcm.numel()) == 0
    rng = np.random.RandomState(1)
    x = (rng.uniform(-0.5, 0.5, 3000) * 32767).astype(np.int16)
    utts = [(x, 48000, np.array([0.02]), np.ones(1)), (x[:2000], 48000, np.array([0.01]), np.ones(1))]
    p1 = _plan(monkeypatch, "default", utts)
    pf = _plan(monkeypatch, "full", utts)
    assert p1.total_frames == 2 and p1.seams.fix_width == 0      # no seams: the fix-up is not launched
    f1, y1 = _run_on_nan(p1)
    ff, yf = _run_on_nan(pf)
    assert not np.isnan(y1).any() and np.array_equal(y1 + np.float32(0.0), yf + np.float32(0.0))
    assert all(np.array_equal(a, b) for a, b in zip(f1, ff))
