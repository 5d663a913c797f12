"""
-m gpu: the round-trip launch's direct arm (MAGPHASE_RT_INVERSE=direct, the default: at N = 4096 the kernel overlap-adds the
windowed frame it has just gathered) against its transform arm (MAGPHASE_RT_INVERSE=transform: Hermitian merge and inverse
transform of the frame's own spectrum, the earlier behaviour) and against the oracle's copy synthesis.

The arms differ in how the waveform is rebuilt and in nothing else: the three row matrices are equal bit for bit, between the
arms and across the three store forms; the waveforms differ by the float32 error of the two transforms the direct arm leaves
out, so the direct arm is no farther from the oracle than the transform arm on the same batch.  The batch
(_rt_direct.direct_batch) holds every kind of frame the arms tell apart, the slot counts give run seams of both kinds.
tests/test_roundtrip_direct_host.py holds the identity itself, in float64, without a GPU.
"""
import warnings

import numpy as np
import pytest

import _rt_direct as rtd
import _seams
from _tol import note, within

pytestmark = pytest.mark.gpu

PCM_TOL = 1e-6               # of the signal peak: tests/test_gpu_lossless.py
# the direct arm against the oracle: 3 x the worst case measured on the MI355X (profiles/rt_direct_tolerance_report.json:
# 1.16e-7 of the peak; the transform arm on the same batch: 1.25e-7), the convention of tests/_tol.py
DIRECT_VS_ORACLE_TOL = 3.5e-7
assert DIRECT_VS_ORACLE_TOL <= 2 * PCM_TOL
STORES = ("rows", "lines", "lines_nt")
H = 2049


@pytest.fixture(scope="module")
def orc():
    from oracle import magphase_oracle as o
    return o


def _plan(monkeypatch, inverse, stores, utts, **kw):
    from magphase_amd.engine import LosslessRoundTripPlan, get_engine
    for name in ("MAGPHASE_RT_SUPPORT", "MAGPHASE_RT_SEAMS", "MAGPHASE_RT_DEAL"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("MAGPHASE_RT_STORES", stores)
    monkeypatch.setenv("MAGPHASE_RT_INVERSE", inverse)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        p = LosslessRoundTripPlan(get_engine(), utts, **kw)
    assert p.inverse == inverse and p.stores == stores and not p.full_support
    return p


def _run(plan):
    """plan.run() into NaN-filled rows, strips and output -> (the three row matrices, pcm) on the host."""
    import torch
    e, F = plan.engine, plan.total_frames
    feats = tuple(e.empty_feats(F, plan.fft_len // 2 + 1).fill_(float("nan")) for _ in range(3))
    strips = e.empty((max(plan.synthesis.strip_floats, 1),)).fill_(float("nan"))
    pcm = e.empty((plan.total_out,)).fill_(float("nan"))
    got, out = plan.run(feats=feats, strips=strips, out=pcm)
    torch.cuda.synchronize()
    assert out is pcm
    rows = [t.cpu().numpy().copy() for t in got]
    y = pcm.cpu().numpy().copy()
    assert not np.isnan(y).any() and not any(np.isnan(r).any() for r in rows)
    return rows, y


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _assert_same_rows(rows, rows0, label):
    for name, a, b in zip(("mag", "real", "imag"), rows, rows0):
        if not _same_bits(a, b):
            bad = a.view(np.uint32) != b.view(np.uint32)
            raise AssertionError("%s, %s: %d of %d elements differ in their bits, largest difference %.3g"
                                 % (label, name, int(bad.sum()), bad.size, float(np.max(np.abs(a - b)))))


_CACHE = {}


def _batch():
    if "batch" not in _CACHE:
        _CACHE["batch"] = rtd.direct_batch()
    return _CACHE["batch"]


def _transform_reference(monkeypatch, key, utts, **kw):
    """The transform arm under `rows` (the parent's launch), once per key."""
    if key not in _CACHE:
        _CACHE[key] = _run(_plan(monkeypatch, "transform", "rows", utts, **kw))
    return _CACHE[key]


def _oracle_reference(orc):
    if "oracle" not in _CACHE:
        _CACHE["oracle"] = [rtd.quiet(rtd.oracle_copy_synthesis, orc, np.asarray(pcm, dtype=np.float64) / 32768.0, fs, pm, voi)
                            for pcm, fs, pm, voi in _batch()]
    return _CACHE["oracle"]


def _oracle_error(plan, y, refs):
    """Largest |y - oracle| over the batch, each utterance by its own peak."""
    worst = 0.0
    for u, ref in enumerate(refs):
        yu = y[plan.out_off_host[u]:plan.out_off_host[u + 1]].astype(np.float64)
        assert yu.shape == ref.shape
        peak = float(np.max(np.abs(ref), initial=0.0))
        if peak == 0.0:
            assert not np.any(yu)
            continue
        worst = max(worst, float(np.max(np.abs(yu - ref))) / peak)
    return worst


def test_the_batch_has_every_kind_of_frame(monkeypatch):
    utts = _batch()
    assert all(0.2 <= len(u[0]) / 48000.0 <= 0.4 for u in utts), [len(u[0]) / 48000.0 for u in utts]
    kinds = set()
    for n_slots in (6, 12):
        p = _plan(monkeypatch, "direct", "lines_nt", utts, n_slots=n_slots)
        a = p.analysis
        left, right = np.asarray(a._host_tabs[1]), np.asarray(a._host_tabs[2])
        assert p.fft_len == 4096 and p.synthesis.n_slots == n_slots and p.total_frames >= 96
        assert rtd.frame_kinds(left, right) == {"class-4", "full-class", "second-tile", "truncated", "L=0"}
        assert np.any(np.asarray(a.v_f0[1]) == 0.0)                   # the unvoiced stretch
        fa = int(a.frame_off[1])
        rel = np.asarray(p.synthesis._ola_host[0][1], dtype=np.int64)
        assert not np.array_equal(np.diff(rel), left[fa + 1:fa + rel.size])   # synthesis positions leave the analysis ones
        assert not np.any(_batch()[3][0])                              # silence
        kinds |= _seams.plan_seam_kinds(p)
    assert {"full-before", "full-after", "narrow-narrow", "inner-reach"} <= kinds, kinds   # seams of both kinds


@pytest.mark.parametrize("n_slots", [6, 12])
def test_direct_against_transform_and_oracle(monkeypatch, orc, n_slots):
    utts = _batch()
    rows0, y0 = _transform_reference(monkeypatch, ("ref", n_slots), utts, n_slots=n_slots)
    refs = _oracle_reference(orc)
    peak = float(np.max(np.abs(y0)))
    err_t = None
    for inverse in ("transform", "direct"):
        for stores in STORES:
            p = _plan(monkeypatch, inverse, stores, utts, n_slots=n_slots)
            rows, y = _run(p)
            _assert_same_rows(rows, rows0, "%s, %s" % (inverse, stores))
            d = float(np.max(np.abs(y.astype(np.float64) - y0))) / peak
            e = _oracle_error(p, y, refs)
            print("%d slots, %-9s %-8s: max |pcm - pcm(transform, rows)| / peak %.3g; against the oracle %.3g"
                  % (n_slots, inverse, stores, d, e))
            if inverse == "transform":
                assert d <= 2 * PCM_TOL, stores                        # the bound of tests/test_gpu_roundtrip_store_lines.py
                err_t = e if err_t is None else max(err_t, e)
            else:
                within(d, PCM_TOL, "PCM_TOL:roundtrip-direct-vs-transform")
                note("roundtrip-transform-vs-oracle:%d-slots" % n_slots, err_t)
                assert e <= err_t, "the direct arm is farther from the oracle (%.3g) than the transform arm (%.3g)" % (e, err_t)
                within(e, DIRECT_VS_ORACLE_TOL, "PCM_TOL:roundtrip-direct-vs-oracle")
                rows2, y2 = _run(p)                                    # two runs of the same plan: equal bits
                assert _same_bits(y, y2) and all(_same_bits(a, b) for a, b in zip(rows, rows2))


@pytest.mark.parametrize("fpr", [1, 7])
def test_runs_of_one_and_of_seven_frames(monkeypatch, fpr):
    utts = _batch()
    rows0, y0 = _transform_reference(monkeypatch, ("fpr", fpr), utts, frames_per_run=fpr)
    rows, y = _run(_plan(monkeypatch, "direct", "lines_nt", utts, frames_per_run=fpr))
    _assert_same_rows(rows, rows0, "direct, %d frame(s) per run" % fpr)
    within(float(np.max(np.abs(y.astype(np.float64) - y0))) / float(np.max(np.abs(y0))), PCM_TOL,
           "PCM_TOL:roundtrip-direct-vs-transform")


def test_full_support_instance(monkeypatch):
    """MAGPHASE_RT_SUPPORT=full: the instance without pruned passes has the direct arm too."""
    utts = _batch()
    got = {}
    for inverse in ("transform", "direct"):
        for name in ("MAGPHASE_RT_SEAMS", "MAGPHASE_RT_DEAL", "MAGPHASE_RT_STORES"):
            monkeypatch.delenv(name, raising=False)
        monkeypatch.setenv("MAGPHASE_RT_SUPPORT", "full")
        monkeypatch.setenv("MAGPHASE_RT_INVERSE", inverse)
        from magphase_amd.engine import LosslessRoundTripPlan, get_engine
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            p = LosslessRoundTripPlan(get_engine(), utts, n_slots=6)
        assert p.full_support and p.inverse == inverse
        got[inverse] = _run(p)
    (rd, yd), (rt, yt) = got["direct"], got["transform"]
    _assert_same_rows(rd, rt, "direct, full support")
    within(float(np.max(np.abs(yd.astype(np.float64) - yt))) / float(np.max(np.abs(yt))), PCM_TOL,
           "PCM_TOL:roundtrip-direct-vs-transform")


def test_16_khz_accepts_and_ignores_the_switch(monkeypatch):
    from magphase_amd import synthetic as syn
    utts = []
    for u in range(2):
        pcm, pm, voi = syn.make_utterance(620 + u, dur_s=0.4, fs=16000)
        utts.append((pcm, 16000, pm, voi))
    pd, pt = _plan(monkeypatch, "direct", "lines_nt", utts, n_slots=6), _plan(monkeypatch, "transform", "lines_nt", utts, n_slots=6)
    assert pd.fft_len == 2048
    (rd, yd), (rt, yt) = _run(pd), _run(pt)
    assert _same_bits(yd, yt) and all(_same_bits(a, b) for a, b in zip(rd, rt))


def test_bad_switch_values(monkeypatch):
    from magphase_amd import _lib
    from magphase_amd.engine import LosslessRoundTripPlan, get_engine
    eng = get_engine()
    monkeypatch.setenv("MAGPHASE_RT_INVERSE", "bogus")
    with pytest.raises(ValueError):
        LosslessRoundTripPlan(eng, _batch()[:1])
    monkeypatch.delenv("MAGPHASE_RT_INVERSE")
    p = LosslessRoundTripPlan(eng, _batch()[2:3], n_slots=6)
    with pytest.raises(ValueError):
        eng.roundtrip_lossless_ola(p.fft_len, p.analysis, p.seams, (None, None, None), None, None, inverse="bogus")
    # an unknown flag bit is still refused by the C entry (an empty launch: nothing is queued)
    for flags in (64, 32 | 64, 2):
        assert eng.lib.mpx_roundtrip_lossless_ola_flags(*([None, 4096] + [None] * 5 + [0, None, 0, None, None, 0]
                                                          + [None] * 6 + [H, flags])) != 0
    assert _lib.RT_INVERSE_FLAGS["transform"] == 32
