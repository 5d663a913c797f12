"""
CPU: tests/epochs_model.py -- the numpy model tests/test_gpu_epoch_kernels.py compares the kernels of
csrc/magphase_epochs.hip with -- against independent forms of the same operations, what the GPU tests rely on about their
inputs (decision margins, crossings next to the ends, float64 against longdouble), and the two host functions of
magphase_amd/epochs.py on arrays whose result can be worked out by hand.
"""
import numpy as np
import pytest

import epochs_model as em
from magphase_amd import epochs
from magphase_amd.epochs import _geometry

F64, LD = np.float64, np.longdouble


@pytest.mark.parametrize("dec", [2, 4, 11, 12])
def test_decimate_is_avg_pool1d(dec):
    import torch
    rng = np.random.RandomState(dec)
    for n in (1, dec - 1, dec, 2 * dec - 1, 2 * dec, 2 * dec + 1, 37 * dec + 5, 1000):
        x = rng.uniform(-1, 1, n)
        got = em.decimate(x, dec, F64, m=0.25)
        if n + 2 * (dec // 2) < 2 * dec:
            assert got.size == 0                      # avg_pool1d refuses an output of no element
            continue
        ref = torch.nn.functional.avg_pool1d(torch.from_numpy(x - 0.25)[None, None], 2 * dec, stride=dec, padding=dec // 2,
                                             count_include_pad=True)[0, 0].numpy()
        assert got.shape == ref.shape, (n, got.shape, ref.shape)
        assert np.max(np.abs(got - ref)) <= 1e-15 * np.max(np.abs(ref)), n
    assert em.mean(np.zeros(0), F64) == 0.0 and em.mean([1.0, 2.0, 6.0], LD) == 3.0


def test_movmean_is_a_window_loop_with_replicate_padding():
    rng = np.random.RandomState(1)
    for n in (1, 2, 5, 64):
        y = rng.uniform(-1, 1, n)
        for h in (1, 7, n - 1, n, 3 * n):
            yp = np.concatenate((np.full(h, y[0]), y, np.full(h, y[-1])))
            ref = np.array([y[i] - np.sum(yp[i:i + 2 * h + 1]) / (2 * h + 1) for i in range(n)])
            got = em.movmean(y, h, F64)
            assert np.max(np.abs(got - ref)) <= 4 * (n + 2 * h + 2) * em.EPS * np.max(np.abs(y)), (n, h)
    assert np.all(em.movmean(np.full(9, 0.25), 3, F64) == 0.0)


def test_scan_modes():
    x = (0.1 * np.random.RandomState(2).randn(300)).astype(np.float32)
    d = np.diff(x.astype(F64), prepend=x[:1].astype(F64))
    assert np.array_equal(em.scan(x, 1, F64), np.cumsum(d))
    assert np.array_equal(em.scan(x, 2, F64), np.cumsum(d ** 2))
    assert np.array_equal(em.scan(d, 0, F64), np.cumsum(d))
    assert em.scan(x, 1, F64)[0] == 0.0 and em.scan(x[:0], 2, LD).size == 0
    assert abs(em.scan(x, 1, LD)[-1] - (LD(x[-1]) - LD(x[0]))) <= 300 * 2.0 ** -64


def _crossings_loop(A, B, w):
    """epochs_model.crossings written out sample by sample, the windows as explicit sums of dx^2 (B's increments)."""
    n = len(A)
    e = np.diff(np.concatenate(([0.0], B)))        # dx^2
    lists = [[], []]
    for i in range(1, n):
        a, b = A[i - 1], A[i]
        p = 0 if (a > 0 and b <= 0) else (1 if (a < 0 and b >= 0) else -1)
        if p < 0:
            continue
        q = i if n < 2 * w + 1 else min(max(i, w), n - w - 1)
        after = np.sum(e[max(q, 0):min(q + w, n)])          # samples q .. q + w - 1, cut at the utterance's end
        before = np.sum(e[max(q - w, 0):min(q, n)])
        lists[p].append((i, abs(b - a), b / (b - a), after - before))
    return lists


def test_crossings_is_a_sample_loop():
    rng = np.random.RandomState(3)
    for n in (1, 2, 3, 8, 9, 10, 16, 17, 18, 100):
        for w in (2, 8, 16):
            A = rng.uniform(-1, 1, n)
            A[rng.randint(0, n, n // 5)] = 0.0                # exact zeros: b <= 0 and b >= 0 count, a == 0 does not
            B = np.cumsum(rng.uniform(0, 1, n) ** 2)
            got, ref = em.crossings(A, B, w), _crossings_loop(A, B, w)
            for p in (0, 1):
                assert [r[0] for r in got[p]] == [r[0] for r in ref[p]], (n, w, p)
                for g, r in zip(got[p], ref[p]):
                    assert g[1] == r[1] and g[2] == r[2]
                    assert abs(g[3] - r[3]) <= 4 * n * em.EPS * B[-1], (n, w, p, g, r)
    # no index leaves [-1, n - 1], at any length
    for n in range(1, 40):
        for i in range(1, n):
            assert all(-1 <= k <= n - 1 for k in em.crossing_score_indices(i, n, 8))


# ---------------------------------------------------------------------------------------------------------------------
# what the GPU tests rely on about their inputs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs", em.F0_RATES)
def test_f0_inputs_decide_clear_of_rounding(fs):
    dec, fs_d, hop, win, l_min, l_max = _geometry(fs)
    n_lags = l_max - l_min + 1
    assert 3 <= n_lags <= 64
    if fs == 44100:
        assert dec == 11
    if fs == 22050:
        assert (l_min, n_lags) == (9, 54)
    n_cmp = 0
    for kind, x in em.f0_batch(fs):
        a = em.nccf(em.decimate(x, dec, F64), hop, win, l_min, n_lags, fs_d, F64)
        b = em.nccf(em.decimate(x, dec, LD), hop, win, l_min, n_lags, fs_d, LD)
        assert np.array_equal(a["first"], b["first"]), (kind, x.size)
        live = a["energy"] > 0
        assert np.all(a["margin"][live] > em.MARGIN_MIN) and np.all(np.abs(a["denom"][live]) >= em.DENOM_MIN)
        assert np.all(np.abs(a["f0"] - b["f0"].astype(F64)) <= 1e-9 * a["f0"])
        n_cmp += int(live.sum())
        if kind in ("zeros", "const") or x.size < dec:
            assert not live.any() and np.all(a["f0"] == fs_d / (l_min + 1)) and np.all(a["peak"] == 0)
    assert n_cmp >= 25


def test_zff_float64_against_longdouble_on_voiced_slices():
    """The yardstick of buf_a and buf_c: the float64 chain against the longdouble chain, relative to max |A|, on slices of
    synthetic utterance 3 with the half window of a 140 Hz voice.  Ceilings: the figures the chain gave when the tests were
    designed (4e-12, 2.7e-11, 1.6e-10); no zero crossing moves."""
    from magphase_amd import synthetic
    for fs, n, h, ceil in ((16000, 4097, 85, 4e-12), (16000, 8193, 85, 2.7e-11), (48000, 40000, 257, 1.6e-10)):
        assert h == (int(round(1.5 / 140.0 * fs)) | 1) // 2
        x = (synthetic.make_utterance(3, 1.0, fs)[0] / 32768.0).astype(np.float32)[:n]
        a, b = em.zff(x, h, F64), em.zff(x, h, LD)
        for k in (0, 1):
            assert np.max(np.abs(a[k] - b[k])) / np.max(np.abs(b[k])) <= ceil, (fs, n, k)
        assert np.array_equal(np.sign(a[1]), np.sign(b[1].astype(F64)))
        assert np.max(np.abs(a[2] - b[2]) / np.maximum(b[2], 1e-300)) <= (n + 2) * em.EPS


@pytest.mark.parametrize("fs", em.ZFF_RATES)
def test_zff_inputs(fs):
    w = em.zff_w(fs)
    lens = em.zff_lengths(fs)
    assert sum(lens) < 150000 and w == (16 if fs == 16000 else 48)
    short = [u for u, n in enumerate(lens) if n < 2 * w + 1]
    assert 0 in short and len(lens) - 1 in short and any(0 < u < len(lens) - 1 for u in short)
    assert {h for h in em.zff_half_wins(fs)} >= {1, 7, 85 if fs == 16000 else 257}
    for kind in ("utt", "noise"):
        lo = hi = 0
        for n, (m64, mld) in zip(lens, em.zff_models(fs, kind)):
            for k in (0, 1, 2):
                assert np.all(np.isfinite(m64[k])) and m64[k].shape == (n,)
            if n >= 2 * w + 1:
                for rows in em.crossings(m64[1], m64[2], w):
                    lo += sum(r[0] < w for r in rows)
                    hi += sum(r[0] > n - w - 1 for r in rows)
        assert lo >= 1 and hi >= 1, (kind, lo, hi)       # the clamp of the window centre is exercised at both ends
    for kind in ("zeros", "const"):
        for m64, _mld in em.zff_models(fs, kind):
            assert all(np.all(v == 0.0) for v in m64) and em.crossings(m64[1], m64[2], w) == [[], []]


def test_end_to_end_case_sits_on_no_rounding_edge():
    u, fs, dur = em.E2E_CASE
    from magphase_amd import synthetic
    x = (synthetic.make_utterance(u, dur, fs)[0] / 32768.0).astype(np.float32)
    a, b = em.track(x, fs, F64), em.track(x, fs, LD)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert a[1].sum() > 50 and (a[1] == 0).sum() > 10           # voiced and unvoiced stretches


# ---------------------------------------------------------------------------------------------------------------------
# the host functions of magphase_amd/epochs.py
# ---------------------------------------------------------------------------------------------------------------------
FS = 16000
HOP_S, WIN_S = 0.005, 0.040


def _lists(cap, rows0, rows1):
    idx = np.zeros((2, cap), dtype=np.int32)
    slope, score, frac = np.zeros((2, cap)), np.zeros((2, cap)), np.zeros((2, cap))
    for p, rows in enumerate((rows0, rows1)):
        for k, (i, sl, sc) in enumerate(rows[:cap]):
            idx[p, k], slope[p, k], score[p, k] = i, sl, sc
    return idx, slope, score, frac


def test_no_voiced_frame_gives_the_5ms_grid():
    n = 3200
    f0, half = epochs._voicing_from_candidates(np.full(33, 100.0), np.full(33, 0.4), np.ones(33), FS)
    assert half == 1 and np.all(f0 == 0.0)
    idx, slope, score, frac = _lists(4, [(100, 1.0, 1.0)], [])
    # the crossing lists are not looked at: counts of any size change nothing
    for cnt in ([1, 0], [10 ** 6, -5]):
        pm, voi = epochs._epochs_from_crossings(n, FS, f0, np.array(cnt), idx, slope, score, frac, 4, HOP_S, WIN_S)
        assert np.array_equal(pm, np.round(np.arange(0.005, n / FS - 2.0 / FS, 0.005), 6)) and np.all(voi == 0)
        assert pm.size == 39
    for n in (0, 5, 7):
        pm, voi = epochs._epochs_from_crossings(n, FS, np.zeros(2), np.zeros(2, dtype=np.int32), idx, slope, score, frac, 4,
                                                HOP_S, WIN_S)
        assert pm.size == 0 and voi.size == 0


def test_voicing_decision_and_half_window():
    T = 20
    f0 = np.full(T, 100.0)
    peak = np.full(T, 0.9)
    e = np.ones(T)
    peak[:8] = 0.4            # unvoiced start
    peak[12] = 0.1            # one isolated flip: the median of 5 removes it
    e[16:] = 1e-5             # -50 dB: below the energy gate
    f0[3] = 400.0             # an outlier in an unvoiced frame; f0[13] in a voiced one
    f0[13] = 200.0
    got, half = epochs._voicing_from_candidates(f0, peak, e, FS)
    want = np.zeros(T)
    want[8:16] = 100.0
    assert np.array_equal(got, want)
    assert half == (int(round(1.5 * 0.01 * FS)) | 1) // 2 == 120
    # all-zero candidates (a launch that never ran): unvoiced, and no warning turns into an error
    got, half = epochs._voicing_from_candidates(np.zeros(2), np.zeros(2), np.zeros(2), FS)
    assert np.all(got == 0) and half == 1


def test_fewer_than_three_voiced_crossings_and_an_empty_list():
    n = 1600                                                  # 0.1 s
    f0 = np.full(13, 100.0)
    cap = 4
    # two crossings 10 ms apart in list 1 (the higher mean score); list 0 has one
    idx, slope, score, frac = _lists(cap, [(300, 1.0, -1.0)], [(480, 1.0, 2.0), (640, 1.0, 2.0)])
    pm, voi = epochs._epochs_from_crossings(n, FS, f0, np.array([1, 2]), idx, slope, score, frac, cap, HOP_S, WIN_S)
    t = (np.array([480, 640]) + 1.5) / FS
    want = [(0.005 * k, 0.0) for k in range(1, 6)] + [(t[0], 1.0), (t[1], 1.0)] + \
           [(t[1] + 0.005 * k, 0.0) for k in range(1, 12) if t[1] + 0.005 * k < 0.1 - 0.0025]
    want = [(a, v) for a, v in want if a * FS < n - 2]
    assert np.array_equal(pm, np.round([a for a, _ in want], 6)) and np.array_equal(voi, [v for _, v in want])
    # three crossings: the short pad branch (dt.size == 2 < 3); the middle one, 2 ms after the first, is spurious
    idx, slope, score, frac = _lists(cap, [], [(480, 1.0, 2.0), (512, 1.0, 2.0), (640, 1.0, 2.0)])
    pm3, voi3 = epochs._epochs_from_crossings(n, FS, f0, np.array([0, 3]), idx, slope, score, frac, cap, HOP_S, WIN_S)
    assert np.array_equal(pm3, pm) and np.array_equal(voi3, voi)
    # voiced frames but no crossing at all: unvoiced marks up to the end
    idx, slope, score, frac = _lists(cap, [], [])
    pm0, voi0 = epochs._epochs_from_crossings(n, FS, f0, np.array([0, 0]), idx, slope, score, frac, cap, HOP_S, WIN_S)
    assert np.all(voi0 == 0) and np.allclose(pm0, 0.005 * np.arange(1, pm0.size + 1), atol=1e-6) and pm0.size == 19


def test_count_above_cap_is_truncated_to_cap():
    n, cap = 1600, 2
    f0 = np.full(13, 100.0)
    idx, slope, score, frac = _lists(cap, [], [(480, 1.0, 2.0), (640, 1.0, 2.0)])
    a = epochs._epochs_from_crossings(n, FS, f0, np.array([0, 2]), idx, slope, score, frac, cap, HOP_S, WIN_S)
    b = epochs._epochs_from_crossings(n, FS, f0, np.array([0, 977]), idx, slope, score, frac, cap, HOP_S, WIN_S)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[1].sum() == 2
    # unordered lists (the device appends in any order) are sorted by index
    idx2, slope2, score2, frac2 = _lists(cap, [], [(640, 1.0, 2.0), (480, 1.0, 2.0)])
    c = epochs._epochs_from_crossings(n, FS, f0, np.array([0, 2]), idx2, slope2, score2, frac2, cap, HOP_S, WIN_S)
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])
