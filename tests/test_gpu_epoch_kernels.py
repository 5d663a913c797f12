"""GPU: the six kernels of magphase_epochs.hip through Engine.launch("mpx_epoch_f0_track" | "mpx_epoch_zff"), every
intermediate against the numpy model of tests/epochs_model.py (pinned on the CPU by tests/test_epochs_model_host.py), and
epochs.track_epochs_batch end to end against the model chain.  Every output buffer is filled with a sentinel and followed by
a sentinel tail; tails and unused slots must come back untouched.

Bounds (eps = 2^-53; "ld" = the longdouble model).  Derived:
  EPK_MEAN      |mean_dev - mean_ld| <= n eps mean|x|, for the signal mean and (over the device's own xd) the decimated mean.
  EPK_XD        |xd_dev - xd_ld| <= (2 dec + 2) eps (sum |x - m| over the window) / (2 dec), m the device's own mean.
  EPK_ENERGY    within 1 float32 ulp of float32(float64 model on the device's own xd and decimated mean).
  EPK_PEAK      1.2e-7 absolute: the (win + 2) eps cancellation bound of the ratio plus one float32 rounding.
  EPK_F0        2 float32 ulps, on frames whose lag decision is clear of rounding (margin > 1e-9 to the 0.06 threshold,
                |parabola denominator| >= 1e-6); all-zero frames give exactly float32(fs_d / (l_min + 1)), peak 0, energy 0.
                EPK_excluded records the share of frames the rule leaves out (at most 1 % per case).
  EPK_ZFF_B     |B_dev - B_ld| <= (n + 2) eps B_ld elementwise (sums of non-negative terms).
  EPK_CROSS     slope, frac and score within 1 float32 ulp of float32(model on the device's own buf_a and buf_b); counts and
                index sets exactly equal.  EPK_cross_bit_identical records whether every value was equal bit for bit.
  EPK_ZFF_FLOOR an output no larger than 16 (n + 2) eps times the largest intermediate of the chain (_chain_peak below) is
                the rounding residue of a result that is zero in exact arithmetic (two samples between three mean removals):
                it has no relative error; the device's must stay under the same floor.
Measured (the tree scan of k_epoch_scan rounds in another order than a sequential cumsum, so no bound follows from the
model's operation count):
  EPK_ZFF_A, EPK_ZFF_C   per utterance err = max|dev - ld| / max|ld| over yard = max|float64 model - ld| / max|ld|,
                as err / max(yard, n eps) <= K.  K is kept at <= 3 x the worst ratio measured on the MI355X
                (profiles/r14_epoch_kernels_tolerance_report.json).
"""
import numpy as np
import pytest

import epochs_model as em
from _tol import note, within
from magphase_amd.epochs import _geometry

pytestmark = pytest.mark.gpu
EPS = em.EPS
F64, LD = np.float64, np.longdouble
SENT, ISENT, TAIL = -7.0, -77, 9
K_ZFF_A = 4.0
K_ZFF_C = 4.0
_STATE = {"excluded": 0.0, "bit_identical": True}


def _engine():
    from magphase_amd.engine import get_engine
    return get_engine()


def _offsets(lens):
    return np.concatenate(([0], np.cumsum(lens))).astype(np.int64)


def _ulp32(v):
    return np.spacing(np.abs(np.asarray(v, dtype=np.float32))).astype(F64)


def _geom(fs):
    dec, fs_d, hop, win, l_min, l_max = _geometry(fs)
    return dec, fs_d, hop, win, l_min, l_max - l_min + 1


# ---------------------------------------------------------------------------------------------------------------------
# mpx_epoch_f0_track
# ---------------------------------------------------------------------------------------------------------------------
def _f0_launch(e, sigs, geom, refused_geom=None):
    """The buffers are laid out for `geom`.  refused_geom: what the entry is told instead, and must refuse."""
    import torch
    from magphase_amd._lib import MagphaseHipError
    dec, fs_d, hop, win, l_min, n_lags = geom
    U = len(sigs)
    off = _offsets([x.size for x in sigs])
    nd = [em.n_decimated(x.size, dec) for x in sigs]
    T = [em.n_frames(k, hop, win + l_min + n_lags - 1) for k in nd]
    doff, foff = _offsets(nd), _offsets(T)
    sig = e.to_device(np.concatenate(sigs), np.float32)
    d_off, d_doff, d_foff = (e.to_device(v, np.int64) for v in (off, doff, foff))
    xd = torch.full((int(doff[-1]) + TAIL,), SENT, dtype=torch.float64, device=e.device)
    means = torch.full((2 * U + TAIL,), SENT, dtype=torch.float64, device=e.device)
    f0, peak, energy = (torch.full((int(foff[-1]) + TAIL,), SENT, dtype=torch.float32, device=e.device) for _ in range(3))
    g = refused_geom or geom
    args = (sig, d_off, U, g[0], d_doff, max(nd), xd, means, d_foff, max(T), g[2], g[3], g[4], g[5], float(g[1]), f0, peak,
            energy)
    if refused_geom:
        with pytest.raises(MagphaseHipError):
            e.launch("mpx_epoch_f0_track", *args)
    else:
        e.launch("mpx_epoch_f0_track", *args)
    out = {k: v.cpu().numpy() for k, v in (("xd", xd), ("means", means), ("f0", f0), ("peak", peak), ("energy", energy))}
    out.update(off=off, doff=doff, foff=foff, U=U)
    return out


def _f0_untouched(out, everything=False):
    U, nd_all, T_all = out["U"], int(out["doff"][-1]), int(out["foff"][-1])
    assert np.all(out["xd"][0 if everything else nd_all:] == SENT), "xd written where it must not be"
    assert np.all(out["means"][0 if everything else 2 * U:] == SENT), "means written where they must not be"
    for k in ("f0", "peak", "energy"):
        assert np.all(out[k][0 if everything else T_all:] == SENT), k + " written where it must not be"


def _f0_check(out, sigs, geom, what):
    dec, fs_d, hop, win, l_min, n_lags = geom
    _f0_untouched(out)
    U = out["U"]
    n_frames = n_excl = n_cmp = 0
    for u, x in enumerate(sigs):
        n = x.size
        m_dev, dm_dev = out["means"][u], out["means"][U + u]
        xd_dev = out["xd"][out["doff"][u]:out["doff"][u + 1]]
        a, b = int(out["foff"][u]), int(out["foff"][u + 1])
        f0, peak, energy = out["f0"][a:b], out["peak"][a:b], out["energy"][a:b]
        # means
        xl = np.asarray(x, dtype=LD)
        tol = n * EPS * float(np.mean(np.abs(xl)))
        d = abs(float(LD(m_dev) - em.mean(x, LD)))
        assert d == 0.0 if tol == 0.0 else within(d / tol, 1.0, "EPK_MEAN"), (what, u, "mean", d, tol)
        if xd_dev.size:
            tol = xd_dev.size * EPS * float(np.mean(np.abs(xd_dev)))
            d = abs(float(LD(dm_dev) - em.mean(xd_dev, LD)))
            assert d == 0.0 if tol == 0.0 else within(d / tol, 1.0, "EPK_MEAN"), (what, u, "decimated mean", d, tol)
        else:
            assert dm_dev == 0.0
        # decimation
        assert xd_dev.size == em.n_decimated(n, dec)
        if xd_dev.size:
            ref = em.decimate(x, dec, LD, m=m_dev)
            tol = (2 * dec + 2) * EPS * em.decimate_bound_terms(x, dec, m_dev)
            err = np.abs(np.asarray(xd_dev, dtype=LD) - ref)
            zero = tol == 0
            assert np.all(err[zero] == 0), (what, u)
            if (~zero).any():
                within(float(np.max(err[~zero] / tol[~zero])), 1.0, "EPK_XD")
        # correlation: the float64 model on the device's own xd and decimated mean
        r = em.nccf(xd_dev, hop, win, l_min, n_lags, fs_d, F64, m=dm_dev)
        assert f0.size == r["f0"].size
        for t in range(f0.size):
            n_frames += 1
            if r["energy"][t] == 0.0:
                assert f0[t] == np.float32(fs_d / (l_min + 1)) and peak[t] == 0.0 and energy[t] == 0.0, (what, u, t)
                continue
            want_e = np.float32(r["energy"][t])
            within(abs(float(energy[t]) - float(want_e)) / float(_ulp32(want_e)), 1.0, "EPK_ENERGY")
            within(abs(float(peak[t]) - float(r["peak"][t])) / 1.2e-7, 1.0, "EPK_PEAK")
            if not (r["margin"][t] > em.MARGIN_MIN and abs(r["denom"][t]) >= em.DENOM_MIN):
                n_excl += 1
                continue
            n_cmp += 1
            want = np.float32(r["f0"][t])
            within(abs(float(f0[t]) - float(want)) / float(_ulp32(want)), 2.0, "EPK_F0")
            if abs(r["delta"][t]) < 0.45:       # the refined lag rounds back to the chosen one
                li = min(max(int(r["first"][t]), 1), n_lags - 2)
                assert int(round(fs_d / float(f0[t]))) - l_min == li, (what, u, t)
    share = n_excl / float(max(n_frames, 1))
    _STATE["excluded"] = max(_STATE["excluded"], share)
    note("EPK_excluded", _STATE["excluded"])
    print("%s: %d frames, %d compared, %d left out" % (what, n_frames, n_cmp, n_excl))
    assert share <= 0.01, (what, share)
    return n_cmp


@pytest.mark.parametrize("fs", em.F0_RATES)
def test_f0_track_ragged_batch_against_the_model(fs):
    e = _engine()
    sigs = [x for _kind, x in em.f0_batch(fs)]
    geom = _geom(fs)
    out = _f0_launch(e, sigs, geom)
    assert _f0_check(out, sigs, geom, "f0_track @ %d" % fs) >= 25
    # batching: every utterance alone gives the same bits
    for u, x in enumerate(sigs):
        one = _f0_launch(e, [x], geom)
        _f0_untouched(one, everything=em.n_decimated(x.size, geom[0]) == 0)     # no decimated sample: nothing is launched
        if em.n_decimated(x.size, geom[0]) == 0:
            continue
        for k, o in (("xd", "doff"), ("f0", "foff"), ("peak", "foff"), ("energy", "foff")):
            assert np.array_equal(one[k][:one[o][1]], out[k][out[o][u]:out[o][u + 1]]), (u, k)
        assert one["means"][0] == out["means"][u] and one["means"][1] == out["means"][out["U"] + u]


@pytest.mark.parametrize("l_min,n_lags", [(10, 64), (40, 3)])
def test_f0_track_lag_count_edges(l_min, n_lags):
    """64 lags: every lane of the wavefront holds a lag.  3 lags: the parabola's centre is pinned to lag index 1."""
    e = _engine()
    fs = 16000
    dec, fs_d, hop, win, _l, _n = _geom(fs)
    geom = (dec, fs_d, hop, win, l_min, n_lags)
    sigs = [em.make_signal("utt", 1468, fs, start=int(0.05 * fs))]
    out = _f0_launch(e, sigs, geom)
    assert _f0_check(out, sigs, geom, "f0_track %d lags" % n_lags) >= 6


@pytest.mark.parametrize("bad", ["n_lags=2", "n_lags=65", "dec=0"])
def test_f0_track_refuses_bad_geometry(bad):
    e = _engine()
    fs = 16000
    geom = _geom(fs)
    g = list(geom)
    g[0 if bad == "dec=0" else 5] = int(bad.split("=")[1])
    sigs = [em.make_signal("utt", 1468, fs, start=int(0.05 * fs))]
    out = _f0_launch(e, sigs, geom, refused_geom=tuple(g))
    _f0_untouched(out, everything=True)


# ---------------------------------------------------------------------------------------------------------------------
# mpx_epoch_zff
# ---------------------------------------------------------------------------------------------------------------------
def _zff_launch(e, sigs, half, w, cap, with_frac=True):
    import torch
    U = len(sigs)
    off = _offsets([x.size for x in sigs])
    total = int(off[-1])
    sig = e.to_device(np.concatenate(sigs), np.float32)
    d_off = e.to_device(off, np.int64)
    d_half = e.to_device(np.asarray(half), np.int32)
    bufs = [torch.full((total + TAIL,), SENT, dtype=torch.float64, device=e.device) for _ in range(3)]
    counts = torch.full((2 * U + TAIL,), ISENT, dtype=torch.int32, device=e.device)
    idx = torch.full((2 * U * cap + TAIL,), ISENT, dtype=torch.int32, device=e.device)
    slope, score, frac = (torch.full((2 * U * cap + TAIL,), SENT, dtype=torch.float32, device=e.device) for _ in range(3))
    e.launch("mpx_epoch_zff", sig, d_off, U, max(x.size for x in sigs), d_half, w, bufs[0], bufs[1], bufs[2], cap, counts,
             idx, slope, score, frac if with_frac else None)
    out = {k: v.cpu().numpy() for k, v in (("A", bufs[0]), ("B", bufs[1]), ("C", bufs[2]), ("counts", counts), ("idx", idx),
                                           ("slope", slope), ("score", score), ("frac", frac))}
    for k in ("A", "B", "C"):
        assert np.all(out[k][total:] == SENT), "buf_%s written past its end" % k.lower()
    assert np.all(out["counts"][2 * U:] == ISENT), "counts written past their end"
    assert np.all(out["idx"][2 * U * cap:] == ISENT)
    for k in ("slope", "score", "frac"):
        assert np.all(out[k][2 * U * cap:] == SENT), k
    if not with_frac:
        assert np.all(out["frac"] == SENT)
    out.update(off=off, U=U, cap=cap)
    return out


def _utt(out, k, u):
    return out[k][out["off"][u]:out["off"][u + 1]]


def _lists_of(out, u, p):
    """(idx, slope, frac, score) of list (u, p) sorted by idx, after checking that the unused slots are untouched."""
    cap = out["cap"]
    a = (2 * u + p) * cap
    k = min(int(out["counts"][2 * u + p]), cap)
    assert np.all(out["idx"][a + k:a + cap] == ISENT), (u, p)
    for name in ("slope", "score", "frac"):
        assert np.all(out[name][a + k:a + cap] == SENT), (u, p, name)
    order = np.argsort(out["idx"][a:a + k], kind="stable")
    return tuple(out[name][a:a + k][order] for name in ("idx", "slope", "frac", "score"))


def _check_crossings(out, sigs, w, with_frac=True):
    """Every list against epochs_model.crossings on the device's own buf_a and buf_b."""
    n_cross = 0
    for u in range(out["U"]):
        model = em.crossings(_utt(out, "A", u), _utt(out, "B", u), w)
        for p in (0, 1):
            assert int(out["counts"][2 * u + p]) == len(model[p]) <= out["cap"], (u, p)
            idx, slope, frac, score = _lists_of(out, u, p)
            assert np.array_equal(idx, [r[0] for r in model[p]]), (u, p)
            cols = ((slope, 1), (frac, 2), (score, 3)) if with_frac else ((slope, 1), (score, 3))
            for got, col in cols:
                want = np.asarray([r[col] for r in model[p]], dtype=F64).astype(np.float32)
                if want.size:
                    within(float(np.max(np.abs(got.astype(F64) - want.astype(F64)) / _ulp32(want))), 1.0, "EPK_CROSS")
                    _STATE["bit_identical"] &= bool(np.array_equal(got, want))
            n_cross += len(model[p])
    note("EPK_cross_bit_identical", _STATE["bit_identical"])
    return n_cross


def _chain_peak(x, h):
    """The largest magnitude of any intermediate of the float64 chain."""
    peak, A = 0.0, em.scan(em.scan(x, 1, F64), 0, F64)
    C = em.movmean(A, h, F64)
    S = em.scan(em.scan(C, 0, F64), 0, F64)
    for v in (A, C, S, em.movmean(S, h, F64)):
        peak = max(peak, float(np.max(np.abs(v))) if v.size else 0.0)
    return peak


@pytest.mark.parametrize("kind", em.SIGNALS)
@pytest.mark.parametrize("fs", em.ZFF_RATES)
def test_zff_ragged_batch_against_the_model(fs, kind):
    e = _engine()
    w = em.zff_w(fs)
    sigs, half, lens = em.zff_batch(fs, kind), em.zff_half_wins(fs), em.zff_lengths(fs)
    cap = max(lens) // 2 + 1                      # no list can overflow
    out = _zff_launch(e, sigs, half, w, cap)
    models = em.zff_models(fs, kind)
    worst = {"A": 0.0, "C": 0.0, "B": 0.0}
    for u, (x, h, (m64, mld)) in enumerate(zip(sigs, half, models)):
        n = x.size
        B_dev, B_ld = _utt(out, "B", u), mld[2]
        zero = B_ld == 0
        assert np.all(B_dev[zero] == 0.0), u
        if (~zero).any():
            r = float(np.max(np.abs(np.asarray(B_dev, dtype=LD) - B_ld)[~zero] / B_ld[~zero])) / ((n + 2) * EPS)
            worst["B"] = max(worst["B"], r)
            within(r, 1.0, "EPK_ZFF_B")
        floor = 16 * (n + 2) * EPS * _chain_peak(x, h)
        for name, k in (("C", 0), ("A", 1)):
            dev, ld, f64 = _utt(out, name, u), mld[k], m64[k]
            scale = float(np.max(np.abs(ld)))
            if kind in ("zeros", "const"):
                assert scale == 0.0 and np.all(dev == 0.0), (u, name)
                continue
            if scale <= floor:
                assert float(np.max(np.abs(dev))) <= floor, (u, name, "EPK_ZFF_FLOOR")
                continue
            err = float(np.max(np.abs(np.asarray(dev, dtype=LD) - ld))) / scale
            yard = float(np.max(np.abs(np.asarray(f64, dtype=LD) - ld))) / scale
            ratio = err / max(yard, n * EPS)
            if ratio > worst[name]:
                worst[name] = ratio
                print("buf_%s @ %d %s: utterance %d (n %d, half_win %d) err %.3g yard %.3g n eps %.3g -> %.3g"
                      % (name.lower(), fs, kind, u, n, h, err, yard, n * EPS, ratio))
            within(ratio, K_ZFF_A if name == "A" else K_ZFF_C, "EPK_ZFF_" + name)
    if kind in ("zeros", "const"):
        assert np.all(out["counts"][:2 * out["U"]] == 0)
        for k in ("A", "B", "C"):
            assert np.all(out[k][:int(out["off"][-1])] == 0.0)
    n_cross = _check_crossings(out, sigs, w)
    print("zff @ %d %s: %d crossings, worst ratios A %.3g C %.3g, B %.3g of its bound"
          % (fs, kind, n_cross, worst["A"], worst["C"], worst["B"]))
    if kind in ("utt", "noise"):
        assert n_cross > 100


@pytest.mark.parametrize("fs", em.ZFF_RATES)
def test_zff_batching_and_null_frac(fs):
    e = _engine()
    w = em.zff_w(fs)
    sigs, half, lens = em.zff_batch(fs, "utt"), em.zff_half_wins(fs), em.zff_lengths(fs)
    cap = max(lens) // 2 + 1
    out = _zff_launch(e, sigs, half, w, cap)
    for u, (x, h) in enumerate(zip(sigs, half)):
        one = _zff_launch(e, [x], [h], w, x.size // 2 + 1)
        for k in ("A", "B", "C"):
            assert np.array_equal(one[k][:x.size], _utt(out, k, u)), (u, k)
        for p in (0, 1):
            assert one["counts"][p] == out["counts"][2 * u + p]
            for a, b in zip(_lists_of(one, 0, p), _lists_of(out, u, p)):
                assert np.array_equal(a, b), (u, p)
    nof = _zff_launch(e, sigs, half, w, cap, with_frac=False)
    assert np.array_equal(nof["counts"], out["counts"])
    for k in ("A", "B", "C"):
        assert np.array_equal(nof[k], out[k])
    for u in range(out["U"]):
        for p in (0, 1):
            a, b = _lists_of(nof, u, p), _lists_of(out, u, p)
            assert all(np.array_equal(a[k], b[k]) for k in (0, 1, 3)), (u, p)


@pytest.mark.parametrize("fs", em.ZFF_RATES)
def test_zff_list_overflow_keeps_to_its_cap(fs):
    e = _engine()
    w, cap = em.zff_w(fs), 8
    sigs, half = em.zff_batch(fs, "noise"), em.zff_half_wins(fs)
    out = _zff_launch(e, sigs, half, w, cap)
    n_over = 0
    for u in range(out["U"]):
        model = em.crossings(_utt(out, "A", u), _utt(out, "B", u), w)
        for p in (0, 1):
            cnt = int(out["counts"][2 * u + p])
            assert cnt == len(model[p]), (u, p)
            n_over += cnt > cap
            idx, slope, frac, score = _lists_of(out, u, p)     # checks that the slots from min(cnt, cap) on are untouched
            assert idx.size == min(cnt, cap) and np.unique(idx).size == idx.size
            rows = {r[0]: r for r in model[p]}
            for i, sl, fr, sc in zip(idx, slope, frac, score):
                assert int(i) in rows, (u, p, i)
                want = np.asarray(rows[int(i)][1:], dtype=F64).astype(np.float32)
                got = np.asarray([sl, fr, sc], dtype=np.float32)
                assert np.all(np.abs(got.astype(F64) - want.astype(F64)) <= _ulp32(want)), (u, p, i)
    assert n_over >= 10      # the five utterances with a short mean window, both directions


# ---------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------
def _grid(n, fs):
    t = np.arange(0.005, n / float(fs) - 2.0 / fs, 0.005)
    return np.round(t, 6)


@pytest.mark.parametrize("fs", [16000, 48000])
def test_utterances_too_short_to_launch_anything(fs):
    import torch
    from magphase_amd import epochs, synthetic
    noise = em.make_signal("noise", 7, fs)
    shorts = [np.zeros(0), np.zeros(5), noise.astype(F64)]
    # whatever the allocator hands out next: not zeros
    junk = [torch.full((4096,), 1.0e4, dtype=torch.float32, device=_engine().device) for _ in range(8)]
    junk += [torch.full((4096,), 12345, dtype=torch.int32, device=_engine().device) for _ in range(8)]
    del junk
    for x in shorts:
        a, b = epochs.track_epochs_batch([x], fs), epochs.track_epochs_batch([x], fs)
        for pm, voi in (a[0], b[0]):
            assert np.array_equal(pm, _grid(x.size, fs)) and np.array_equal(voi, np.zeros(pm.size))
    long_x = synthetic.make_utterance(3, 1.0, fs)[0]
    alone = epochs.track_epochs_batch([long_x], fs)[0]
    assert alone[1].sum() > 20
    for order in ([0, 1, 3, 2], [3, 0, 1, 2], [0, 3, 1, 2]):
        batch = [(shorts + [long_x])[k] for k in order]
        res = epochs.track_epochs_batch(batch, fs)
        for k, (pm, voi) in zip(order, res):
            if k == 3:
                assert np.array_equal(pm, alone[0]) and np.array_equal(voi, alone[1]), order
            else:
                assert np.array_equal(pm, _grid(shorts[k].size, fs)) and voi.size == pm.size and not voi.any()


def test_track_epochs_against_the_model_chain():
    from magphase_amd import epochs, synthetic
    u, fs, dur = em.E2E_CASE
    pcm = synthetic.make_utterance(u, dur, fs)[0]
    x = (pcm / 32768.0).astype(np.float32)
    pm, voi = epochs.track_epochs(x, fs)
    m_pm, m_voi = em.track(x, fs, F64)
    assert pm.size == m_pm.size and np.array_equal(voi, m_voi)
    d = float(np.max(np.abs(pm - m_pm)))
    print("track_epochs vs model chain: %d epochs, %d voiced, max |d pm| %.3g s" % (pm.size, int(voi.sum()), d))
    within(d / 2e-6, 1.0, "EPK_E2E_PM")
