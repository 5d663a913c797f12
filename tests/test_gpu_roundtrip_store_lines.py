"""
-m gpu: the round-trip launch with its feature rows stored by line (MAGPHASE_RT_STORES=lines, lines_nt: blocks of two whole
128-byte lines of memory, csrc/mpx_common.hpp "Row stores by line") against the same launch with the blocks aligned to the
row (rows).  The store shape moves values between stores, it computes nothing: the three row matrices must be equal bit for
bit, the waveform within the round trip's bound (2 PCM_TOL of the peak, tests/test_gpu_roundtrip_seams.py).

Every plane lies in a buffer filled with a sentinel, 64 guard floats in front and behind, and starts 1, 7 and 31 floats into
its aligned allocation, so that the three planes of a frame have three different phases and, with a dense pitch, every phase
occurs; afterwards the guards and the pad columns still hold the sentinel and no element of a row does.  tests/
test_row_store_lines_host.py holds the shape itself, phase by phase, without a GPU.
"""
import warnings

import numpy as np
import pytest

import _seams
from _tol import within

pytestmark = pytest.mark.gpu

PCM_TOL = 1e-6       # of the signal peak: tests/test_gpu_lossless.py
SENT = -3.0e33       # no feature has this value: magnitudes are >= 0, the other two lie in [-1, 1]
GUARD = 64
OFFSETS = (1, 7, 31)
H = 2049


def store_batch():
    """Three utterances of about 0.3 s at 48 kHz, 100 frames or more together (with a dense pitch every phase 0 ... 31
    occurs on either wave of a pair, at run starts and run ends): periods around 150 and around 240 samples (class 4),
    stretches around 800 (L > 512: the full class), and one utterance whose first epoch is its first sample (L = 0)."""
    rng = np.random.RandomState(77)
    utts = []
    for k in range(3):
        g = []
        while sum(g) < 13000:
            g += list(rng.randint(140, 171, rng.randint(3, 9))) + list(rng.randint(225, 256, rng.randint(3, 9)))
            g += list(rng.randint(760, 840, rng.randint(1, 3)))
        utts.append(_seams.utt_from_gaps(np.asarray(g), 90 + k, first=0 if k == 1 else 37 + k))
    return utts


def _plan(monkeypatch, stores, utts, **kw):
    from magphase_amd.engine import LosslessRoundTripPlan, get_engine
    for name in ("MAGPHASE_RT_SUPPORT", "MAGPHASE_RT_SEAMS"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("MAGPHASE_RT_STORES", stores)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        p = LosslessRoundTripPlan(get_engine(), utts, **kw)
    assert p.stores == stores and not p.full_support
    return p


def _guarded_planes(engine, F, ld, h=H):
    """Three sentinel-filled buffers and the [F x h] views into them with row pitch ld, the views' first floats 1, 7 and 31
    floats past a 128-byte boundary and GUARD floats or more into their buffers."""
    import torch
    bufs, views = [], []
    for off in OFFSETS:
        buf = torch.full((GUARD + off + F * ld + GUARD,), SENT, dtype=torch.float32, device=engine.device)
        assert buf.data_ptr() % 128 == 0
        v = buf[GUARD + off:GUARD + off + F * ld].view(F, ld)[:, :h]
        assert F == 0 or (v.data_ptr() // 4) % 32 == off
        bufs.append(buf)
        views.append(v)
    return bufs, tuple(views)


def _run_guarded(plan, ld=H, h=H):
    """plan.run() into guarded planes and NaN-filled pcm_out / strips -> (rows on the host, pcm on the host); the guards, the
    pad columns and the rows' own elements are checked against the sentinel here."""
    import torch
    e, F = plan.engine, plan.total_frames
    bufs, feats = _guarded_planes(e, F, ld, h)
    strips = e.empty((max(plan.synthesis.strip_floats if plan.synthesis is not None else 0, 1),)).fill_(float("nan"))
    pcm = e.empty((plan.total_out,)).fill_(float("nan"))
    got, out = plan.run(feats=feats, strips=strips, out=pcm)
    torch.cuda.synchronize()
    assert out is pcm and all(a is b for a, b in zip(got, feats))
    rows = []
    for off, buf, v in zip(OFFSETS, bufs, feats):
        b = buf.cpu().numpy()
        lo = GUARD + off
        assert np.all(b[:lo] == np.float32(SENT)), "front guard of the plane at offset %d" % off
        body = b[lo:lo + F * ld].reshape(F, ld)
        assert np.all(body[:, h:] == np.float32(SENT)), "pad columns of the plane at offset %d" % off
        assert np.all(b[lo + F * ld:] == np.float32(SENT)), "back guard of the plane at offset %d" % off
        assert not np.any(body[:, :h] == np.float32(SENT)), "an element of a row was not written (offset %d)" % off
        rows.append(body[:, :h].copy())
    return rows, pcm.cpu().numpy()


_REF = {}


def _rows_reference(monkeypatch, n_slots, ld):
    """The launch under `rows` on the store batch, once per (slots, pitch)."""
    if (n_slots, ld) not in _REF:
        _REF[(n_slots, ld)] = _run_guarded(_plan(monkeypatch, "rows", store_batch(), n_slots=n_slots), ld=ld)
    return _REF[(n_slots, ld)]


def _assert_same(stores, got, ref, label):
    (rows, pcm), (rows0, pcm0) = got, ref
    for name, a, b in zip(("mag", "real", "imag"), rows, rows0):
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), (stores, label, name)
    assert pcm.shape == pcm0.shape and not np.isnan(pcm).any() and not np.isnan(pcm0).any()
    peak = max(float(np.max(np.abs(pcm0), initial=0.0)), 1e-30)
    err = float(np.max(np.abs(pcm.astype(np.float64) - pcm0), initial=0.0)) / peak
    print("%s against rows, %s: max |pcm - pcm_rows| / peak %.3g, bit-identical: %s"
          % (stores, label, err, bool(np.array_equal(pcm.view(np.uint32), pcm0.view(np.uint32)))))
    within(err, 2 * PCM_TOL, "PCM_TOL:roundtrip-stores-vs-rows")


def test_the_batch_has_every_phase_and_both_support_classes(monkeypatch):
    p = _plan(monkeypatch, "lines", store_batch(), n_slots=6)
    left = np.asarray(p.analysis._host_tabs[1])
    assert p.fft_len == 4096 and p.total_frames >= 96
    assert (left > 512).any() and (left == 0).any() and (left <= 512).sum() > 32
    durs = [len(u[0]) / 48000.0 for u in store_batch()]
    assert all(0.25 <= d <= 0.4 for d in durs), durs


@pytest.mark.parametrize("n_slots", [6, 12])
@pytest.mark.parametrize("stores", ["lines", "lines_nt"])
def test_rows_by_line_equal_rows_by_row(monkeypatch, stores, n_slots):
    ref = _rows_reference(monkeypatch, n_slots, H)
    p = _plan(monkeypatch, stores, store_batch(), n_slots=n_slots)
    assert p.synthesis.n_slots == n_slots
    got = _run_guarded(p)
    _assert_same(stores, got, ref, "%d slots" % n_slots)
    again = _run_guarded(p)     # two runs identical
    assert np.array_equal(got[1], again[1]) and all(np.array_equal(a, b) for a, b in zip(got[0], again[0]))


@pytest.mark.parametrize("ld", [2050, 2080])
@pytest.mark.parametrize("stores", ["lines", "lines_nt"])
def test_other_row_pitches_keep_their_pad_columns(monkeypatch, stores, ld):
    """(ld 2049 is the test above; 2050: the phase advances by 2 per row, 2080: every row of a plane has the same phase)"""
    ref = _rows_reference(monkeypatch, 6, ld)
    _assert_same(stores, _run_guarded(_plan(monkeypatch, stores, store_batch(), n_slots=6), ld=ld), ref, "ld %d" % ld)


@pytest.mark.parametrize("stores", ["lines", "lines_nt"])
def test_edge_batches(monkeypatch, stores):
    pe = _plan(monkeypatch, stores, [])
    rows, pcm = _run_guarded(pe)
    assert pe.total_frames == 0 and all(r.shape == (0, H) for r in rows) and pcm.size == 0
    rng = np.random.RandomState(5)
    x = (rng.uniform(-0.5, 0.5, 3000) * 32767).astype(np.int16)
    one = [(x, 48000, np.array([0.02]), np.ones(1))]
    few = [_seams.utt_from_gaps(np.asarray([230, 240, 790]), 3, first=41)]      # 4 frames, 6 slots
    for utts, frames, kw in ((one, 1, {}), (few, 4, {"n_slots": 6})):
        p, p0 = _plan(monkeypatch, stores, utts, **kw), _plan(monkeypatch, "rows", utts, **kw)
        assert p.total_frames == frames
        _assert_same(stores, _run_guarded(p), _run_guarded(p0), "%d frame(s)" % frames)


def test_2048_ignores_the_store_form(monkeypatch):
    from magphase_amd import synthetic as syn
    utts = []
    for u in range(2):
        pcm, pm, voi = syn.make_utterance(520 + u, dur_s=0.5, fs=16000)
        utts.append((pcm, 16000, pm, voi))
    pl, p0 = _plan(monkeypatch, "lines", utts, n_slots=6), _plan(monkeypatch, "rows", utts, n_slots=6)
    assert pl.fft_len == 2048
    (rl, yl), (r0, y0) = _run_guarded(pl, ld=1025, h=1025), _run_guarded(p0, ld=1025, h=1025)
    assert np.array_equal(yl.view(np.uint32), y0.view(np.uint32))
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(rl, r0))
