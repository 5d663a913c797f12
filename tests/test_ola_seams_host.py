"""
CPU: run seams sized by what the frames add (hostmath.ola_runs(extents=) and its native twin mpx_host_ola_runs_extents), the
per-frame extents of the round-trip kernel (hostmath.roundtrip_frame_extents / mpx_roundtrip_frame_extents), and the
round-trip plan's use of both.

The planner used to take every frame for dense: two adjacent runs then overlap in N - hop positions, all of which go
through the successor's head strip and the fix-up.  A class-4 frame of k_roundtrip_pair adds 1024 of its 4096 samples;
with the extents the seams hold only what the frames on either side really reach.  Checked here: the two twins agree field
for field; dense extents give the old planner's table; a brute-force model of the kernel's flush rules and the fix-up
(tests/_seams.py) finds every kept sample written once, nothing a frame added dropped, and the plain overlap-add as the
sum -- on hand-built tables with every kind of seam and on random ones; the same model refuses a table whose seam is a
few elements too narrow.
"""
import numpy as np
import pytest

from magphase_amd import _lib, hostmath as hm, hostplan

import _seams
from _seams import NARROW, check_runs

N = 4096
FULL = (0, N)


def _table(rng, N, n_utts, sizes=None, p_full=0.2, narrow=NARROW):
    """Ragged random utterances: hops of 60 .. 600 samples with the odd long one, frames narrow or dense at random."""
    rels, starts, lens, ext = [], [], [], []
    for u in range(n_utts):
        n = int(sizes[u]) if sizes is not None else int(rng.randint(1, 120))
        sh = rng.randint(60, 600, size=n)
        if n > 3 and rng.rand() < 0.5:
            sh[rng.randint(1, n)] = rng.choice([1500, 3000, 7000])      # further apart than a narrow / a dense frame
        sh[0] = rng.choice([150, N // 2 + 700, 90, 9000, N // 2])
        rel, start, out_len = hm.ola_plan(np.cumsum(sh), N)
        rels.append(rel), starts.append(start), lens.append(out_len)
        full = rng.rand(n) < p_full
        ext.append(np.where(full[:, None], np.asarray([(0, N)]), np.asarray([narrow])))
    out_off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    return rels, starts, lens, out_off, np.concatenate(ext).astype(np.int32)


def _native(rels, starts, lens, out_off, N, n_slots, gcuts=None, extents=None):
    rel_cat = np.concatenate(rels) if rels else np.zeros(0, np.int64)
    f_off = np.concatenate(([0], np.cumsum([len(r) for r in rels])))
    return hostplan.ola_runs(rel_cat, f_off, starts, lens, out_off[:len(rels)], N, n_slots, gcuts=gcuts, extents=extents)


@pytest.mark.parametrize("N,n_slots,sizes", [(4096, 24, None), (4096, 7, [1, 50, 2, 90, 1, 33]), (4096, 400, [3, 1, 5, 2]),
                                             (2048, 16, None), (1024, 9, None), (4096, 1, [40, 25])])
def test_native_planner_with_extents_equals_the_numpy_twin(N, n_slots, sizes):
    """Field for field, on tables that mix narrow and dense frames: utterances of one frame, of one run, and batches with
    fewer frames than slots; shares by count and the caller's own cuts; the model holds on each."""
    rng = np.random.RandomState(N + n_slots)
    narrow = (3 * N // 8, 5 * N // 8)
    for rep in range(4):
        n_utts = len(sizes) if sizes is not None else int(rng.randint(1, 7))
        rels, starts, lens, out_off, ext = _table(rng, N, n_utts, sizes, narrow=narrow)
        total = ext.shape[0]
        gcuts = None
        if rep % 2 and total > 2:     # the caller's cuts: ascending, distinct, some shares of one frame
            k = int(rng.randint(1, min(total, 40)))
            gcuts = np.concatenate(([0], np.sort(rng.choice(np.arange(1, total), size=k - 1, replace=False)), [total]))
        rp, so_p, sr_p = hm.ola_runs(rels, starts, lens, out_off, N, n_slots, gcuts=gcuts, extents=ext)
        if hostplan.enabled():     # (MAGPHASE_NATIVE_PLAN=0 switches the native planners off: the model below still runs)
            rn, so_n, sr_n = _native(rels, starts, lens, out_off, N, n_slots, gcuts=gcuts, extents=ext)
            assert rn.dtype == rp.dtype == hm.OLA_RUN_DTYPE
            for name in hm.OLA_RUN_DTYPE.names:
                assert np.array_equal(rn[name], rp[name]), name
            assert np.array_equal(so_n, so_p) and np.array_equal(sr_n, sr_p)
        check_runs(rp, rels, ext, N, starts, lens, out_off, seed=rep)
        assert 0 <= _seams.fix_width(rp) <= N + 127                        # what mpx_ola_fixup_width accepts


@pytest.mark.parametrize("N,n_slots,fpr", [(4096, 24, None), (2048, 5, None), (1024, 64, None), (4096, 8, 7), (4096, 4, 1)])
def test_dense_extents_give_the_old_table_in_both_twins(N, n_slots, fpr):
    rng = np.random.RandomState(7 * N + n_slots)
    for rep in range(3):
        rels, starts, lens, out_off, _ext = _table(rng, N, int(rng.randint(1, 7)))
        total = sum(len(r) for r in rels)
        dense = np.tile(np.asarray([(0, N)], dtype=np.int32), (total, 1))
        old = hm.ola_runs(rels, starts, lens, out_off, N, n_slots, frames_per_run=fpr)
        new = hm.ola_runs(rels, starts, lens, out_off, N, n_slots, frames_per_run=fpr, extents=dense)
        assert old[0].tobytes() == new[0].tobytes()
        assert np.array_equal(old[1], new[1]) and np.array_equal(old[2], new[2])
        if fpr is None and hostplan.enabled():
            n_old = _native(rels, starts, lens, out_off, N, n_slots)
            n_new = _native(rels, starts, lens, out_off, N, n_slots, extents=dense)
            assert n_old[0].tobytes() == n_new[0].tobytes() == old[0].tobytes()
            assert np.array_equal(n_old[1], n_new[1]) and np.array_equal(n_old[2], n_new[2])


def test_native_entry_without_extents_is_the_old_entry_and_refuses_bad_extents():
    lib = _lib.load()
    rng = np.random.RandomState(3)
    rels, starts, lens, out_off, ext = _table(rng, N, 3, [30, 1, 44])
    rel = np.concatenate(rels).astype(np.int64)
    f_off = np.concatenate(([0], np.cumsum([len(r) for r in rels]))).astype(np.int64)
    st, ln, oo = (np.ascontiguousarray(a, dtype=np.int64) for a in (starts, lens, out_off[:3]))
    gcuts = hm.slot_cuts(int(f_off[-1]), 6)
    cap = 3 + gcuts.size + 1

    def call(name, *extra):
        runs = np.zeros(cap, dtype=hm.OLA_RUN_DTYPE)
        n = getattr(lib, name)(3, rel.ctypes.data, f_off.ctypes.data, st.ctypes.data, ln.ctypes.data, oo.ctypes.data, N,
                               gcuts.ctypes.data, int(gcuts.size), *extra, runs.ctypes.data, cap)
        return int(n), runs

    n0, r0 = call("mpx_host_ola_runs")
    n1, r1 = call("mpx_host_ola_runs_extents", None)
    assert n0 == n1 > 3 and r0.tobytes() == r1.tobytes()
    for bad in ((-1, 100), (200, 100), (0, N + 1)):
        e = ext.copy()
        e[5] = bad
        assert call("mpx_host_ola_runs_extents", e.ctypes.data)[0] < 0
        with pytest.raises(ValueError):
            hm.ola_runs(rels, starts, lens, out_off, N, 6, extents=e)
    with pytest.raises(ValueError):
        hm.ola_runs(rels, starts, lens, out_off, N, 6, extents=ext[:-1])


# ---------------------------------------------------------------------------------------------------------------------
# hand-built tables: one utterance each, cuts given, every kind of seam
# ---------------------------------------------------------------------------------------------------------------------
def _hand(hops, full, cuts, start=None, out_len=None):
    """One utterance from its hops (rel = cumsum, first frame at 0), the indices of its dense frames and its cuts."""
    rel = np.concatenate(([0], np.cumsum(hops))).astype(np.int64)
    n = rel.size
    ext = np.tile(np.asarray([NARROW], dtype=np.int32), (n, 1))
    ext[list(full)] = FULL
    buf = int(rel[-1]) + N
    start = N // 2 if start is None else start
    out_len = buf - start - 100 if out_len is None else out_len
    gcuts = np.asarray([0] + list(cuts) + [n], dtype=np.int64)
    out_off = np.asarray([0, out_len], dtype=np.int64)
    return [rel], [start], [out_len], out_off, ext, gcuts


def _plan_hand(t):
    rels, starts, lens, out_off, ext, gcuts = t
    runs = hm.ola_runs(rels, starts, lens, out_off, N, gcuts.size - 1, gcuts=gcuts, extents=ext)[0]
    if hostplan.enabled():
        assert _native(rels, starts, lens, out_off, N, gcuts.size - 1, gcuts=gcuts, extents=ext)[0].tobytes() == runs.tobytes()
    check_runs(runs, rels, ext, N, starts, lens, out_off)
    return runs


_HOPS = [240] * 59        # 60 frames, runs of 20: a run spans 4800 samples, more than N


def test_seams_between_narrow_frames_hold_what_the_frames_reach():
    t = _hand(_HOPS, [], [20, 40])
    runs = _plan_hand(t)
    rel = t[0][0]
    assert runs.size == 3
    for k in (1, 2):
        r, fb = runs[k], int(runs[k]["frame_begin"])
        prev_hi = int(rel[fb - 1]) + NARROW[1]
        assert int(r["x0"]) + int(r["head_end"]) == prev_hi
        assert int(r["x0"]) + int(r["fix_lo"]) == int(rel[fb]) + NARROW[0]
        assert int(r["x0"]) + int(r["fix_hi"]) == prev_hi
        assert int(r["fix_hi"]) - int(r["fix_lo"]) == 1024 - 240         # against N - hop = 3856 for dense frames
        assert int(runs[k - 1]["x0"]) + int(runs[k - 1]["flush_end"]) == prev_hi
    dense = hm.ola_runs(t[0], t[1], t[2], t[3], N, 3, gcuts=t[5])[0]
    assert np.all((dense["fix_hi"] - dense["fix_lo"])[1:] == N - 240)
    assert np.array_equal(dense["frame_begin"], runs["frame_begin"])       # the cuts keep their N-wide rule


@pytest.mark.parametrize("full,kind", [([15], "inner-reach"), ([19], "full-before"), ([20], "full-after"),
                                       ([19, 20], "full-before"), ([18, 21, 39, 40], "full-after"),
                                       (range(60), "full-before")])
def test_seams_with_dense_frames_on_either_side_and_inside_a_run(full, kind):
    """A dense frame mid-run whose rel + N lies past the last narrow frame's rel + 2560 sets the run's end; a dense frame
    as the last of a run or the first of the next widens the seam on its side only."""
    t = _hand(_HOPS, full, [20, 40])
    runs = _plan_hand(t)
    rel = t[0][0]
    assert kind in _seams.seam_kinds(runs, rel, t[4], N)
    if list(full) == [15]:
        assert int(rel[15]) + N > int(rel[19]) + NARROW[1]
        assert int(runs[1]["x0"]) + int(runs[1]["head_end"]) == int(rel[15]) + N
    if list(full) == [20]:     # the successor's dense first frame begins below the predecessor's reach: fixed from there
        assert int(runs[1]["x0"]) + int(runs[1]["fix_lo"]) == int(rel[20])
        assert int(runs[1]["x0"]) + int(runs[1]["fix_hi"]) == int(rel[19]) + NARROW[1]


def test_a_short_last_run_ends_no_earlier_than_its_predecessor():
    """The last run has no span rule: two narrow frames after a run that ends in a dense one reach less far than it does.
    The run's end is then its predecessor's, and its whole share of the seam is head strip."""
    t = _hand([240] * 29, [27], [28])
    runs = _plan_hand(t)
    rel = t[0][0]
    assert int(rel[29]) + NARROW[1] < int(rel[27]) + N
    assert int(runs[1]["x0"]) + int(runs[1]["head_end"]) == int(rel[27]) + N
    assert int(runs[1]["flush_end"]) >= int(runs[1]["head_end"])


@pytest.mark.parametrize("hop,full", [(1500, []), (3000, []), (7000, []), (7000, [20]), (5000, [19, 20])])
def test_frames_further_apart_than_their_support_leave_a_gap_the_next_run_writes(hop, full):
    hops = list(_HOPS)
    hops[19] = hop            # between the last frame of run 0 and the first of run 1
    hops[30] = 1300           # and one inside a run
    t = _hand(hops, full, [20, 40])
    runs = _plan_hand(t)
    assert "gap" in _seams.seam_kinds(runs, t[0][0], t[4], N)
    assert int(runs[1]["fix_hi"]) == int(runs[1]["fix_lo"])     # nothing to fix across a gap


@pytest.mark.parametrize("start,out_len", [(0, None), (N // 2, None), (20 * 240 + 1800, 6000), (20 * 240 + 2100, 300),
                                           (100, 20 * 240 + 2000), (100, 20 * 240 + 1700), (19 * 240 + 2559, 2),
                                           (40 * 240 + 2200, 50)])
def test_kept_part_clipping_at_both_ends_of_a_seam(start, out_len):
    """[start, start + out_len) beginning inside, before and after the first seam's fix range, and ending inside it."""
    t = _hand(_HOPS, [], [20, 40], start=start, out_len=out_len)
    runs = _plan_hand(t)
    for r in runs:
        assert int(r["x0"]) + int(r["fix_lo"]) >= start or int(r["fix_hi"]) == int(r["fix_lo"])
        assert int(r["x0"]) + int(r["fix_hi"]) <= start + t[2][0] or int(r["fix_hi"]) == int(r["fix_lo"])


@pytest.mark.parametrize("field,delta", [("fix_lo", 8), ("fix_hi", -8), ("head_end", -8), ("flush_end", -72)])
def test_the_model_refuses_a_seam_that_drops_what_a_frame_added(field, delta):
    t = _hand(_HOPS, [], [20, 40])
    rels, starts, lens, out_off, ext, gcuts = t
    runs = hm.ola_runs(rels, starts, lens, out_off, N, 3, gcuts=gcuts, extents=ext)[0].copy()
    check_runs(runs, rels, ext, N, starts, lens, out_off)
    runs[field][0 if field == "flush_end" else 1] += delta
    with pytest.raises(AssertionError):
        check_runs(runs, rels, ext, N, starts, lens, out_off)


def test_the_model_refuses_narrow_seams_under_dense_frames():
    """What the planner must never do: believe in zeros the kernel adds (a table planned for narrow frames, run on dense)."""
    t = _hand(_HOPS, [], [20, 40])
    rels, starts, lens, out_off, ext, gcuts = t
    runs = hm.ola_runs(rels, starts, lens, out_off, N, 3, gcuts=gcuts, extents=ext)[0]
    dense = np.tile(np.asarray([FULL], dtype=np.int32), (60, 1))
    with pytest.raises(AssertionError):
        check_runs(runs, rels, dense, N, starts, lens, out_off)


# ---------------------------------------------------------------------------------------------------------------------
# the frames' extents
# ---------------------------------------------------------------------------------------------------------------------
def _native_extents(left, right, n_fft, flags=0):
    lib = _lib.load()
    left, right = np.ascontiguousarray(left, dtype=np.int32), np.ascontiguousarray(right, dtype=np.int32)
    out = np.full((left.size, 2), -7, dtype=np.int32)
    assert lib.mpx_roundtrip_frame_extents(n_fft, left.ctypes.data, right.ctypes.data, left.size, flags, out.ctypes.data) == 0
    return out


@pytest.mark.parametrize("n_fft", [4096, 2048, 1024])
def test_extents_twin_equals_the_native_function(n_fft):
    vals = np.asarray([-1, 0, 1, 127, 128, 255, 256, 510, 511, 512, 513, 1023, 1024, 2047, 2048, 4095, 4096, 5000])
    left, right = (a.reshape(-1) for a in np.meshgrid(vals, vals))
    got = _native_extents(left, right, n_fft)
    assert np.array_equal(got, hm.roundtrip_frame_extents(left, right, n_fft))
    cls = hm.roundtrip_support_classes(left, right, n_fft)
    if n_fft == 4096:
        assert np.all(got[cls == 4] == np.asarray(NARROW)) and np.all(got[cls != 4] == np.asarray((0, n_fft)))
        assert np.any(cls == 4) and np.any(cls != 4)
    else:
        assert np.all(got == np.asarray((0, n_fft)))
    full = _native_extents(left, right, n_fft, flags=1)          # MPX_RT_FULL_SUPPORT: the instance that prunes nothing
    assert np.all(full == np.asarray((0, n_fft)))
    assert np.array_equal(full, hm.roundtrip_frame_extents(left, right, n_fft, full_support=True))
    lib = _lib.load()
    assert lib.mpx_roundtrip_frame_extents(n_fft, None, None, 0, 0, None) == 0
    assert lib.mpx_roundtrip_frame_extents(n_fft, None, None, 3, 0, None) != 0
    assert lib.mpx_roundtrip_frame_extents(1000, None, None, 0, 0, None) != 0
    assert lib.mpx_roundtrip_frame_extents(n_fft, None, None, 0, 2, None) != 0       # unknown flag


def test_narrow_extent_is_the_rows_the_class_keeps():
    """(1536, 2560) = the 128-sample rows P/2 - 4 <= q < P/2 + 4 (csrc/mpx_common.hpp: support_row_live) of 32."""
    rows = [q for q in range(32) if 16 - 4 <= q < 16 + 4]
    assert (128 * rows[0], 128 * rows[-1] + 128) == NARROW
    assert tuple(hm.roundtrip_frame_extents([300], [200], 4096)[0]) == NARROW


# ---------------------------------------------------------------------------------------------------------------------
# the round-trip plan (built without a GPU: tests/_seams.py: HostEngine)
# ---------------------------------------------------------------------------------------------------------------------
def _rt_plan(monkeypatch, utts, seams=None, support=None, **kw):
    import warnings
    from magphase_amd.engine import LosslessRoundTripPlan
    for name, val in (("MAGPHASE_RT_SEAMS", seams), ("MAGPHASE_RT_SUPPORT", support)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, val)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return LosslessRoundTripPlan(_seams.HostEngine(kw.pop("engine_slots", 1536)), utts, **kw)


def _plan_tables(p):
    s = p.synthesis
    pm_rel, starts, lens, _nfr = s._ola_host
    return [np.asarray(r, dtype=np.int64) for r in pm_rel], starts, lens, s.out_off_host


@pytest.mark.parametrize("n_slots", [6, 12])
def test_roundtrip_plan_sizes_its_seams_by_the_frames_extents(monkeypatch, n_slots):
    utts = _seams.seam_batch()
    pd = _rt_plan(monkeypatch, utts, n_slots=n_slots)
    pf = _rt_plan(monkeypatch, utts, seams="full", n_slots=n_slots)
    ps = _rt_plan(monkeypatch, utts, support="full", n_slots=n_slots)
    assert (pd.full_seams, pf.full_seams, ps.full_seams) == (False, True, True) and ps.full_support and not pf.full_support
    assert pd.fft_len == 4096 and pd.deal == pf.deal == "cost" and pd.synthesis.n_slots == n_slots
    assert (pd.seam_geometry, pf.seam_geometry, ps.seam_geometry) == ("extents", "dense", "dense")
    rd, rf = pd.runs_host, pf.runs_host
    assert rf.tobytes() == ps.runs_host.tobytes()
    assert np.array_equal(rd["frame_begin"], rf["frame_begin"]) and np.array_equal(rd["frame_end"], rf["frame_end"])
    # the synthesis plan inside keeps the table for dense frames under every setting (any overlap-add kernel may run it);
    # the table sized by this kernel's extents is the round trip's own
    for p in (pd, pf, ps):
        assert p.synthesis.runs_host.tobytes() == rf.tobytes() and not hasattr(p.synthesis, "fix_width")
    assert pf.seams is pf.synthesis and ps.seams is ps.synthesis and pd.seams is not pd.synthesis
    assert pd.seams.runs_host is rd and np.array_equal(pd.seams.runs.view(hm.OLA_RUN_DTYPE), rd)
    assert pd.seams.slot_off is pd.synthesis.slot_off and pd.seams.strip_floats == pd.synthesis.strip_floats
    assert pd.seams.fix_width == _seams.fix_width(rd)
    assert 0 < pd.seams.fix_width <= 4096 + 127
    left, right = pd.analysis._host_tabs[1], pd.analysis._host_tabs[2]
    ext = hm.roundtrip_frame_extents(left, right, 4096)
    assert np.array_equal(pd._frame_extents(pd.total_frames), ext)
    assert np.all(ps._frame_extents(ps.total_frames) == np.asarray((0, 4096)))
    rels, starts, lens, out_off = _plan_tables(pd)
    check_runs(rd, rels, ext, 4096, starts, lens, out_off)
    dense = np.tile(np.asarray([(0, 4096)], dtype=np.int32), (pd.total_frames, 1))
    check_runs(rf, rels, dense, 4096, starts, lens, out_off)
    assert (rd["fix_hi"] - rd["fix_lo"]).sum() < (rf["fix_hi"] - rf["fix_lo"]).sum()
    assert np.array_equal(rd["strip_off"], rf["strip_off"])       # the strips stay N + 64 floats per run


def test_seam_batch_has_every_kind_of_seam(monkeypatch):
    """What the GPU test of the same batch relies on, decided on the plans' run tables, with 6 and with 12 slots: seams with
    a dense frame before, after and inside a run, between narrow frames, across a gap of zeros, and non-empty fix ranges
    that the kept part clips at `start` and at `start + out_len`."""
    utts = _seams.seam_batch()
    durs = [len(u[0]) / 48000.0 for u in utts]
    assert all(0.3 <= d <= 0.6 for d in durs), durs
    for n_slots in (6, 12):
        pd = _rt_plan(monkeypatch, utts, n_slots=n_slots)
        kinds = _seams.plan_seam_kinds(pd)
        assert _seams.SEAM_KINDS <= kinds, (n_slots, sorted(_seams.SEAM_KINDS - kinds))
        rels, starts, lens, out_off = _plan_tables(pd)
        f_off = np.concatenate(([0], np.cumsum([len(r) for r in rels])))
        clip_lo = clip_hi = gap = 0
        for r in pd.runs_host:       # the same, spelled out on the table's fields
            u = int(np.searchsorted(f_off, int(r["frame_begin"]), side="right") - 1)
            x0, live = int(r["x0"]), int(r["fix_hi"]) > int(r["fix_lo"])
            clip_lo += live and x0 + int(r["fix_lo"]) == starts[u]
            clip_hi += live and x0 + int(r["fix_hi"]) == starts[u] + lens[u] < x0 + int(r["head_end"])
            gap += int(r["head_end"]) > 0 and not live and int(r["frame_begin"]) > f_off[u]
        assert clip_lo >= 1 and clip_hi >= 1 and gap >= 1, (n_slots, clip_lo, clip_hi, gap)
        cls = hm.roundtrip_support_classes(pd.analysis._host_tabs[1], pd.analysis._host_tabs[2], 4096)
        assert set(np.unique(cls).tolist()) == {4, 16}
        check_runs(pd.runs_host, rels, pd._frame_extents(pd.total_frames), 4096, starts, lens, out_off)


def test_roundtrip_plan_at_2048_keeps_the_dense_seams(monkeypatch):
    from magphase_amd import synthetic as syn
    utts = []
    for u in range(2):
        pcm, pm, voi = syn.make_utterance(520 + u, dur_s=0.5, fs=16000)
        utts.append((pcm, 16000, pm, voi))
    pd = _rt_plan(monkeypatch, utts, n_slots=6)
    pf = _rt_plan(monkeypatch, utts, seams="full", n_slots=6)
    assert pd.fft_len == 2048 and pd.runs_host.size > 2
    assert pd.runs_host.tobytes() == pf.runs_host.tobytes() == pd.synthesis.runs_host.tobytes()
    assert np.all(pd._frame_extents(pd.total_frames) == np.asarray((0, 2048)))


def test_roundtrip_plan_of_single_frames_and_of_nothing(monkeypatch):
    pe = _rt_plan(monkeypatch, [])
    assert pe.total_frames == 0 and pe.synthesis is None and pe.runs_host.size == 0 and not pe.full_seams
    rng = np.random.RandomState(1)
    x = (rng.uniform(-0.5, 0.5, 3000) * 32767).astype(np.int16)
    p1 = _rt_plan(monkeypatch, [(x, 48000, np.array([0.02]), np.ones(1)), (x[:2000], 48000, np.array([0.01]), np.ones(1))])
    assert p1.total_frames == 2 and p1.synthesis.n_runs == 2
    assert p1.seams.fix_width == 0            # no run has a predecessor: the fix-up is not launched at all


def test_a_plan_without_host_frame_tables_says_that_its_seams_are_dense(monkeypatch):
    """The extents come from the analysis plan's host tables; a plan that has none keeps the dense seams (always valid)
    and says so in seam_geometry, although full_seams was not asked for."""
    from magphase_amd import plans
    monkeypatch.setattr(plans.LosslessRoundTripPlan, "_frame_extents", lambda self, total: None)
    p = _rt_plan(monkeypatch, _seams.seam_batch(), n_slots=6)
    assert not p.full_seams and p.seam_geometry == "dense" and p.seams is p.synthesis
    assert p.runs_host.tobytes() == p.synthesis.runs_host.tobytes()
