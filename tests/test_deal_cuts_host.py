"""
CPU: the planner that deals the round trip's frames to the slots by cost.

  * mpx_host_deal_cuts against hostmath.deal_cuts, bit for bit; optimality against exhaustive search; the bound
    T <= T_ideal + the largest single-frame cost;
  * mpx_roundtrip_frame_terms against a numpy restatement of noise_fft's tile count and row test;
  * on the bench batch's kind of input (64 synthetic 5 s utterances, 1 536 slots): every frame in exactly one run, the
    modelled largest slot cost within 5 % of the mean, and MAGPHASE_RT_DEAL=count gives today's cuts.
"""
import itertools

import numpy as np
import pytest

from magphase_amd import _lib, hostmath as hm, hostplan


def _native(terms, coef):
    terms = np.ascontiguousarray(terms, dtype=np.int32)
    coef = np.ascontiguousarray(coef, dtype=np.int32)
    cuts = np.full(coef.shape[0] + 1, -7, dtype=np.int64)
    t = np.full(1, -7, dtype=np.int64)
    rc = _lib.load().mpx_host_deal_cuts(terms.ctypes.data, terms.shape[0], terms.shape[1], coef.ctypes.data,
                                        coef.shape[0], cuts.ctypes.data, t.ctypes.data)
    assert rc == 0
    return cuts, int(t[0])


def _slot_costs(terms, coef, cuts):
    c = np.asarray(terms, dtype=np.int64) @ np.asarray(coef, dtype=np.int64).T    # [frames, slots]
    return np.asarray([c[cuts[s]:cuts[s + 1], s].sum() for s in range(coef.shape[0])], dtype=np.int64)


def _check_pair(terms, coef):
    terms, coef = np.asarray(terms), np.asarray(coef)
    cn, tn = _native(terms, coef)
    cp, tp = hm.deal_cuts(terms, coef)
    assert cp.dtype == np.int64 and np.array_equal(cn, cp) and tn == tp
    n = terms.shape[0]
    assert cn[0] == 0 and cn[-1] == n and np.all(np.diff(cn) >= 0)
    costs = _slot_costs(terms, coef, cn)
    assert (costs.max() if n else 0) == tn          # T is attained: no smaller T holds the largest share
    return cn, tn


def _random_case(rng, n, ns, zero_bc=False, slow=None):
    terms = np.stack([np.ones(n, dtype=np.int64), rng.randint(0, 40, n), rng.randint(0, 2, n)], axis=1)
    base = np.asarray([[100, 7, 300], [141, 9, 420], [200, 13, 610]])
    coef = base[(np.arange(ns) % 6 * 2) // 4].copy()
    if zero_bc:
        coef[:, 1:] = 0
    if slow is not None:
        coef[slow::3] *= 8
    return terms, coef


@pytest.mark.parametrize("ns", [1, 6, 12])
def test_native_and_numpy_dealing_agree_bit_for_bit(ns):
    rng = np.random.RandomState(ns)
    for n in sorted({1, 5, max(ns - 1, 0), ns, 40 * ns}):
        for kw in ({}, {"zero_bc": True}, {"slow": 1}):
            _check_pair(*_random_case(rng, n, ns, **kw))
    # arbitrary coefficients (every slot its own class) and term counts other than three
    for n_terms in (1, 2, 4):
        terms = rng.randint(0, 50, (37, n_terms))
        coef = rng.randint(0, 1000, (ns, n_terms))
        _check_pair(terms, coef)
    # nothing costs anything: the first slot takes every frame at T = 0
    c, t = _check_pair(np.ones((9, 3), dtype=np.int64), np.zeros((ns, 3), dtype=np.int64))
    assert t == 0 and c[1] == 9


def test_zero_coefficients_reproduce_shares_by_count():
    """b = c = 0 and a = 100 / 141 / 200: the shares are 1 : 1/1.41 : 1/2 of the frames, as the age weights deal them."""
    ns, n = 12, 4800
    terms, coef = _random_case(np.random.RandomState(0), n, ns, zero_bc=True)
    cuts, t = _check_pair(terms, coef)
    sizes = np.diff(cuts)
    a = coef[:, 0]
    assert np.all(sizes * a <= t) and np.all((sizes[:-1] + 1) * a[:-1] > t)       # every share but the last is full


def test_dealing_is_optimal_by_exhaustive_search():
    rng = np.random.RandomState(3)
    for n in range(1, 13):
        terms, coef = _random_case(rng, n, 3, slow=(n % 3 if n % 2 else None))
        _cuts, t = _check_pair(terms, coef)
        c = terms.astype(np.int64) @ coef.astype(np.int64).T
        best = min(max(c[0:i, 0].sum(), c[i:j, 1].sum(), c[j:n, 2].sum())
                   for i, j in itertools.combinations_with_replacement(range(n + 1), 2))
        assert t == best, (n, t, best)


@pytest.mark.parametrize("ns,n", [(6, 240), (12, 500), (12, 13), (1, 30)])
def test_largest_share_is_within_one_frame_of_the_ideal(ns, n):
    """T <= T_ideal + max over slots of that slot's largest single-frame cost, T_ideal = 1 / sum_s (1 / slot s's cost
    for all frames): were the frames divisible, every slot would end at T_ideal."""
    rng = np.random.RandomState(ns + n)
    for kw in ({}, {"slow": 2}):
        terms, coef = _random_case(rng, n, ns, **kw)
        _cuts, t = _check_pair(terms, coef)
        c = terms.astype(np.int64) @ coef.astype(np.int64).T
        t_ideal = 1.0 / np.sum(1.0 / c.sum(axis=0).astype(np.float64))
        assert t <= t_ideal + c.max()


def test_bad_arguments_are_refused():
    lib = _lib.load()
    terms = np.asarray([[1, -1, 0]], dtype=np.int32)
    coef = np.ones((2, 3), dtype=np.int32)
    cuts = np.zeros(3, dtype=np.int64)
    assert lib.mpx_host_deal_cuts(terms.ctypes.data, 1, 3, coef.ctypes.data, 2, cuts.ctypes.data, None) == -1
    assert lib.mpx_host_deal_cuts(None, 1, 3, coef.ctypes.data, 2, cuts.ctypes.data, None) == -1
    assert lib.mpx_host_deal_cuts(terms.ctypes.data, 1, 3, coef.ctypes.data, 0, cuts.ctypes.data, None) == -1
    with pytest.raises(ValueError):
        hm.deal_cuts(terms, coef)
    assert lib.mpx_roundtrip_frame_terms(1000, None, None, 0, None) == -1
    assert lib.mpx_roundtrip_frame_terms(4096, None, None, 3, None) == -1
    assert lib.mpx_roundtrip_frame_terms(4096, None, None, 0, None) == 0


# ---------------------------------------------------------------------------------------------------------------------
# the cost terms
# ---------------------------------------------------------------------------------------------------------------------
def _terms_restated(L, R, N):
    """noise_fft (csrc/magphase_comp.hip) restated: tiles of 32 P samples in the compact form (P = 32), 64 P otherwise;
    register row j of a tile is gathered when (128 j < len - rot) or (128 j + 127 >= N - rot)."""
    P = N // 128
    ln = min(L + R + 1, N)
    rot = L if L < N else 0
    tile = 32 * P if P == 32 else 64 * P
    ntiles = -(-ln // tile)
    pairs = sum(1 for _t in range(ntiles) for j in range(P) if (128 * j < ln - rot) or (128 * j + 127 >= N - rot))
    return [1, pairs, ntiles - 1]


@pytest.mark.parametrize("N", [4096, 2048, 1024])
def test_frame_terms_match_the_kernels_row_and_tile_conditions(N):
    cases = [(0, 5), (0, 0), (3, 0), (N, 40), (N + 7, 3), (N - 1, 2), (N // 2, N // 2), (N // 2, N // 2 - 1),
             (700, 720), (N - 100, 300), (5, N + 20)]
    for total in (1, 127, 128, 129, 1024, 1025):        # frame lengths L + R + 1, split in three ways
        for L in sorted({0, (total - 1) // 2, total - 1}):
            cases.append((L, total - 1 - L))
    rng = np.random.RandomState(N)
    cases += [(int(a), int(b)) for a, b in zip(rng.randint(0, N + 300, 200), rng.randint(0, N + 300, 200))]
    left = np.asarray([c[0] for c in cases], dtype=np.int32)
    right = np.asarray([c[1] for c in cases], dtype=np.int32)
    want = np.asarray([_terms_restated(int(a), int(b), N) for a, b in cases], dtype=np.int32)
    got = hostplan.roundtrip_frame_terms(left, right, N)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert np.array_equal(hm.roundtrip_frame_terms(left, right, N), want)
    assert any(L + R + 1 > N for L, R in cases) and any(L >= N for L, R in cases)
    if N == 4096:   # the second tile starts at 1 025 samples
        k = {L + R + 1: t for (L, R), t in zip(cases, want.tolist())}
        assert k[1024][2] == 0 and k[1025][2] == 1


def test_slot_costs_follow_the_age_rule_of_the_slot_weights():
    lib = _lib.load()
    ns = 30
    coef = np.zeros((ns, 3), dtype=np.int32)
    w = np.zeros(ns, dtype=np.float32)
    assert lib.mpx_roundtrip_slot_costs(coef.ctypes.data, ns) == 0 and lib.mpx_roundtrip_slot_weights(w.ctypes.data, ns) == 0
    assert np.all(coef[:, 0] > 0) and np.all(coef >= 0)
    for s in range(ns):     # slots of one weight share one coefficient row, and the dearer class has the smaller weight
        for s2 in range(ns):
            if w[s] == w[s2]:
                assert np.array_equal(coef[s], coef[s2])
            elif w[s] > w[s2]:
                assert coef[s, 0] < coef[s2, 0]


# ---------------------------------------------------------------------------------------------------------------------
# the bench batch's kind of input
# ---------------------------------------------------------------------------------------------------------------------
N_SLOTS = 1536


@pytest.fixture(scope="module")
def batch():
    """64 synthetic 5 s utterances at 48 kHz: the analysis tables and the synthesis positions, on the host."""
    from magphase_amd import synthetic as syn
    fs, N = 48000, 4096
    left, right, f0s, n_frames = [], [], [], []
    for u in range(64):
        pcm, pm_sec, voi = syn.make_utterance(u, dur_s=5.0, fs=fs)
        pm_sec, voi = hm.clean_epochs(pm_sec, voi, check_len_smpls=pcm.size, fs=fs)
        _pm, lft, rgt = hm.frame_bounds(pm_sec * fs, pcm.size)
        left.append(lft), right.append(rgt), n_frames.append(lft.size)
        f0s.append(hm.shift_to_f0(lft, voi, fs))
    rel, starts, lens = [], [], []
    for f0 in f0s:
        v_pm = np.cumsum(hm.f0_to_shift(np.asarray(f0, dtype=np.float64), fs)).astype(int)
        r, s, n = hm.ola_plan(v_pm, N)
        rel.append(r), starts.append(s), lens.append(n)
    out_off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    coef = np.zeros((N_SLOTS, 3), dtype=np.int32)
    assert _lib.load().mpx_roundtrip_slot_costs(coef.ctypes.data, N_SLOTS) == 0
    terms = hostplan.roundtrip_frame_terms(np.concatenate(left), np.concatenate(right), N)
    return dict(N=N, rel=rel, starts=starts, lens=lens, out_off=out_off, coef=coef, terms=terms, total=int(sum(n_frames)))


def test_bench_batch_is_dealt_within_five_percent_of_the_mean(batch):
    b = batch
    cuts, t = hostplan.deal_cuts(b["terms"], b["coef"])
    c2, t2 = hm.deal_cuts(b["terms"], b["coef"])
    assert np.array_equal(cuts, c2) and t == t2
    assert cuts.size == N_SLOTS + 1 and cuts[0] == 0 and cuts[-1] == b["total"] and np.all(np.diff(cuts) >= 0)
    runs, slot_off, slot_runs = hm.ola_runs(b["rel"], b["starts"], b["lens"], b["out_off"], b["N"], N_SLOTS, gcuts=cuts)
    # every frame in exactly one run, every run in exactly one slot
    seen = np.zeros(b["total"], dtype=np.int64)
    for r in runs:
        seen[r["frame_begin"]:r["frame_end"]] += 1
    assert np.all(seen == 1)
    assert slot_off.size == N_SLOTS + 1 and slot_off[0] == 0 and slot_off[-1] == runs.size
    assert np.array_equal(np.sort(slot_runs), np.arange(runs.size))
    # the native run planner on the same cuts
    rel_cat = np.concatenate(b["rel"])
    f_off = np.concatenate(([0], np.cumsum([r.size for r in b["rel"]])))
    runs_n, so_n, sr_n = hostplan.ola_runs(rel_cat, f_off, b["starts"], b["lens"], b["out_off"][:-1], b["N"], N_SLOTS,
                                           gcuts=cuts)
    assert runs_n.tobytes() == runs.tobytes() and np.array_equal(so_n, slot_off) and np.array_equal(sr_n, slot_runs)
    # the modelled cost of what every slot really got (after the planner moved the cuts it had to move)
    cost =np.zeros(N_SLOTS, dtype=np.int64)
    per_class = {}
    for s in range(N_SLOTS):
        key = tuple(b["coef"][s].tolist())
        if key not in per_class:
            per_class[key] = b["terms"].astype(np.int64) @ b["coef"][s].astype(np.int64)
        for ci in slot_runs[slot_off[s]:slot_off[s + 1]]:
            cost[s] += per_class[key][runs[ci]["frame_begin"]:runs[ci]["frame_end"]].sum()
    print("modelled slot cost: max %d, mean %.1f, max/mean %.4f; T %d; frames per slot %d .. %d"
          % (cost.max(), cost.mean(), cost.max() / cost.mean(), t, np.diff(cuts).min(), np.diff(cuts).max()))
    assert cost.max() <= 1.05 * cost.mean()


def test_count_dealing_is_unchanged_and_selectable(batch, monkeypatch):
    """gcuts=None is today's dealing, and LosslessRoundTripPlan hands the synthesis plan no cuts of its own under
    MAGPHASE_RT_DEAL=count (read when the plan is built)."""
    import os
    from magphase_amd import plans
    b = batch
    w = np.zeros(N_SLOTS, dtype=np.float32)
    assert _lib.load().mpx_roundtrip_slot_weights(w.ctypes.data, N_SLOTS) == 0
    today = hm.slot_cuts(b["total"], N_SLOTS, w)
    r0 = hm.ola_runs(b["rel"], b["starts"], b["lens"], b["out_off"], b["N"], N_SLOTS, weights=w)
    r1 = hm.ola_runs(b["rel"], b["starts"], b["lens"], b["out_off"], b["N"], N_SLOTS, weights=w, gcuts=None)
    r2 = hm.ola_runs(b["rel"], b["starts"], b["lens"], b["out_off"], b["N"], N_SLOTS, gcuts=today)
    for x, y, z in zip(r0, r1, r2):
        assert x.tobytes() == y.tobytes() == z.tobytes()

    seen = {}

    class FakeAnalysis:
        def __init__(self, engine, utts, fft_len=None, **kw):
            self.fft_len, self.v_f0, self.fs, self.total_frames = b["N"], [], [], 0

    class FakeSynthesis:
        def __init__(self, engine, f0, fs, fft_len, gcuts=None, **kw):
            seen["gcuts"] = gcuts
            self.total_frames = self.total_out = 0
            self.out_off_host = np.zeros(1, dtype=np.int64)

    monkeypatch.setattr(plans, "LosslessAnalysisPlan", FakeAnalysis)
    monkeypatch.setattr(plans, "LosslessSynthesisPlan", FakeSynthesis)
    monkeypatch.setenv("MAGPHASE_RT_DEAL", "count")
    p = plans.LosslessRoundTripPlan(None, [object()])
    assert seen["gcuts"] is None and p.deal == "count"
    monkeypatch.delenv("MAGPHASE_RT_DEAL")
    plans.LosslessRoundTripPlan(None, [object()])
    assert callable(seen["gcuts"])
    plans.LosslessRoundTripPlan(None, [object()], frames_per_run=5)
    assert seen["gcuts"] is None
    assert "MAGPHASE_RT_DEAL" not in os.environ
