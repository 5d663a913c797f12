"""
Batch planners in the library (csrc/magphase_plan.cpp) behind numpy-friendly wrappers.  They are the same float64 /
integer arithmetic as the numpy forms in hostmath.py and plan_synthesis_numpy below (which remain: they are what a failed
native call falls back to -- raising the exceptions the reference's arithmetic would -- and what tests/test_host_plans.py
compares these against, bit for bit), for a whole batch per call instead of ~60 numpy calls per utterance.
MAGPHASE_NATIVE_PLAN=0 disables them.  The numpy planners that need the library's host scans (plan_synthesis_numpy,
plan_const_rate_synthesis) live here too: nothing in this module needs torch or a GPU.
"""
import os

import numpy as np

from . import _lib, hostmath as hm
from .hostmath import OLA_RUN_DTYPE


class PlanFallback(Exception):
    """The native planner declined (an utterance the numpy form raises on, or planners disabled): use the numpy form."""


def enabled():
    return os.environ.get("MAGPHASE_NATIVE_PLAN", "1") != "0"


def _cat(arrs, dtype):
    if len(arrs) == 1:
        return np.ascontiguousarray(arrs[0], dtype=dtype).reshape(-1)
    return np.concatenate([np.asarray(a, dtype=dtype).reshape(-1) for a in arrs])


def plan_analysis(pm_sec_list, voi_list, n_smpls, fs_list, sig_off):
    """-> dict(pos, pm, left, right (int64[F]), f0 (float64[F]), frame_off (int64[U+1])) for the batch."""
    if not enabled():
        raise PlanFallback()
    lib = _lib.load()
    U = len(pm_sec_list)
    pm_sec = _cat(pm_sec_list, np.float64)
    voi = _cat(voi_list, np.float64)
    sizes = [int(np.size(p)) for p in pm_sec_list]
    if [int(np.size(v)) for v in voi_list] != sizes:
        raise PlanFallback()
    ep_off = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    E = int(ep_off[-1])
    n_smpls = np.ascontiguousarray(n_smpls, dtype=np.int64)
    fs = np.ascontiguousarray(fs_list, dtype=np.float64)
    sig_off = np.ascontiguousarray(sig_off, dtype=np.int64)
    pos, pm, left, right = (np.empty(max(E, 1), dtype=np.int64) for _ in range(4))
    f0 = np.empty(max(E, 1), dtype=np.float64)
    frame_off = np.empty(U + 1, dtype=np.int64)
    F = int(lib.mpx_host_plan_analysis(U, pm_sec.ctypes.data, voi.ctypes.data, ep_off.ctypes.data, n_smpls.ctypes.data,
                                       fs.ctypes.data, sig_off.ctypes.data, pos.ctypes.data, pm.ctypes.data,
                                       left.ctypes.data, right.ctypes.data, f0.ctypes.data, frame_off.ctypes.data))
    if F < 0:
        raise PlanFallback()
    return dict(pos=pos[:F], pm=pm[:F], left=left[:F], right=right[:F], f0=f0[:F], frame_off=frame_off)


def plan_synthesis(f0_list, fs, fft_len, b_const_rate, b_voi_ap_win):
    """f0_list: exp(lf0) per utterance.  -> dict of the per-frame tables of CompressedSynthesisPlan for the batch."""
    if not enabled():
        raise PlanFallback()
    lib = _lib.load()
    U = len(f0_list)
    f0 = _cat(f0_list, np.float64)
    row_off = np.concatenate(([0], np.cumsum([int(np.size(f)) for f in f0_list]))).astype(np.int64)
    cap = 2 * int(row_off[-1]) + 2
    i64 = lambda: np.empty(cap, dtype=np.int64)      # noqa: E731
    i32 = lambda: np.empty(cap, dtype=np.int32)      # noqa: E731
    o = dict(v_shift=i64(), v_pm=i64(), npos=i64(), nleft=i32(), nright=i32(), wtype=i32(), voiced=i32(), row0=i32(),
             row1=i32(), rowt=np.empty(cap, dtype=np.float64), win_l=i32(), win_r=i32(), pm_rel=i64())
    frame_off = np.empty(U + 1, dtype=np.int64)
    ns_len, out_start, out_len = (np.empty(max(U, 1), dtype=np.int64) for _ in range(3))
    F = int(lib.mpx_host_plan_synthesis(
        U, f0.ctypes.data, row_off.ctypes.data, float(fs), int(fft_len), int(bool(b_const_rate)), int(bool(b_voi_ap_win)),
        cap, o["v_shift"].ctypes.data, o["v_pm"].ctypes.data, o["npos"].ctypes.data, o["nleft"].ctypes.data,
        o["nright"].ctypes.data, o["wtype"].ctypes.data, o["voiced"].ctypes.data, o["row0"].ctypes.data,
        o["row1"].ctypes.data, o["rowt"].ctypes.data, o["win_l"].ctypes.data, o["win_r"].ctypes.data,
        o["pm_rel"].ctypes.data, frame_off.ctypes.data, ns_len.ctypes.data, out_start.ctypes.data, out_len.ctypes.data))
    if F < 0:
        raise PlanFallback()
    o = {k: v[:F] for k, v in o.items()}
    o.update(frame_off=frame_off, ns_len=ns_len[:U], out_start=out_start[:U], out_len=out_len[:U], row_off=row_off)
    return o


def plan_lossless_synthesis(f0_list, fs_list, fft_len):
    """-> dict(v_pm, pm_rel (int64[F]), frame_off (int64[U+1]), out_start, out_len (int64[U]))."""
    if not enabled():
        raise PlanFallback()
    lib = _lib.load()
    U = len(f0_list)
    if U == 0:
        raise PlanFallback()
    f0 = _cat(f0_list, np.float64)
    frame_off = np.concatenate(([0], np.cumsum([int(np.size(f)) for f in f0_list]))).astype(np.int64)
    fs = np.ascontiguousarray(fs_list, dtype=np.float64)
    F = int(frame_off[-1])
    v_pm, pm_rel = np.empty(max(F, 1), dtype=np.int64), np.empty(max(F, 1), dtype=np.int64)
    out_start, out_len = np.empty(U, dtype=np.int64), np.empty(U, dtype=np.int64)
    rc = int(lib.mpx_host_plan_lossless_synthesis(U, f0.ctypes.data, frame_off.ctypes.data, fs.ctypes.data, int(fft_len),
                                                  v_pm.ctypes.data, pm_rel.ctypes.data, out_start.ctypes.data,
                                                  out_len.ctypes.data))
    if rc < 0:
        raise PlanFallback()
    return dict(v_pm=v_pm[:F], pm_rel=pm_rel[:F], frame_off=frame_off, out_start=out_start, out_len=out_len)


def deal_cuts(terms, coef):
    """hostmath.deal_cuts in the library (mpx_host_deal_cuts) -> (cuts int64[n_slots + 1], T)."""
    if not enabled():
        raise PlanFallback()
    lib = _lib.load()
    coef = np.ascontiguousarray(coef, dtype=np.int32)
    if coef.ndim != 2 or coef.shape[0] < 1 or coef.shape[1] < 1:
        raise PlanFallback()
    terms = np.ascontiguousarray(terms, dtype=np.int32).reshape(-1, coef.shape[1])
    cuts = np.empty(coef.shape[0] + 1, dtype=np.int64)
    t = np.zeros(1, dtype=np.int64)
    if int(lib.mpx_host_deal_cuts(terms.ctypes.data, int(terms.shape[0]), int(coef.shape[1]), coef.ctypes.data,
                                  int(coef.shape[0]), cuts.ctypes.data, t.ctypes.data)) != 0:
        raise PlanFallback()
    return cuts, int(t[0])


def roundtrip_frame_terms(left, right, fft_len):
    """mpx_roundtrip_frame_terms -> int32 [n_frames, 3] (hostmath.roundtrip_frame_terms is the numpy form)."""
    if not enabled():
        raise PlanFallback()
    left, right = np.ascontiguousarray(left, dtype=np.int32), np.ascontiguousarray(right, dtype=np.int32)
    if left.shape != right.shape or left.ndim != 1:
        raise PlanFallback()
    terms = np.empty((left.size, 3), dtype=np.int32)
    if int(_lib.load().mpx_roundtrip_frame_terms(int(fft_len), left.ctypes.data, right.ctypes.data, int(left.size),
                                                 terms.ctypes.data)) != 0:
        raise PlanFallback()
    return terms


def ola_runs(pm_rel_cat, frame_off, starts, out_lens, out_offs, fft_len, n_slots, weights=None, gcuts=None, extents=None):
    """hostmath.ola_runs (default equal-share mode, or the caller's gcuts) on the concatenated frame positions ->
    (runs, slot_off, slot_runs).  extents: per-frame (ext_lo, ext_hi) or None (mpx_host_ola_runs_extents)."""
    if not enabled():
        raise PlanFallback()
    lib = _lib.load()
    frame_off = np.ascontiguousarray(frame_off, dtype=np.int64)
    U = int(frame_off.size - 1)
    total = int(frame_off[-1])
    n_slots = max(1, int(n_slots))
    gcuts = np.ascontiguousarray(hm.slot_cuts(total, n_slots, weights) if gcuts is None else gcuts, dtype=np.int64)
    pm_rel = np.ascontiguousarray(pm_rel_cat, dtype=np.int64)
    starts, out_lens, out_offs = (np.ascontiguousarray(a, dtype=np.int64) for a in (starts, out_lens, out_offs))
    cap = U + int(gcuts.size) + 1
    runs = np.zeros(cap, dtype=OLA_RUN_DTYPE)
    if extents is None:
        n = int(lib.mpx_host_ola_runs(U, pm_rel.ctypes.data, frame_off.ctypes.data, starts.ctypes.data,
                                      out_lens.ctypes.data, out_offs.ctypes.data, int(fft_len), gcuts.ctypes.data,
                                      int(gcuts.size), runs.ctypes.data, cap))
    else:
        extents = np.ascontiguousarray(extents, dtype=np.int32).reshape(-1, 2)
        if extents.shape[0] != total:
            raise PlanFallback()
        n = int(lib.mpx_host_ola_runs_extents(U, pm_rel.ctypes.data, frame_off.ctypes.data, starts.ctypes.data,
                                              out_lens.ctypes.data, out_offs.ctypes.data, int(fft_len), gcuts.ctypes.data,
                                              int(gcuts.size), extents.ctypes.data, runs.ctypes.data, cap))
    if n < 0:
        raise PlanFallback()
    runs = runs[:n]
    ns = gcuts.size - 1
    slot_of = np.clip(np.searchsorted(gcuts, runs["frame_begin"], side="right") - 1, 0, ns - 1)
    slot_off = np.searchsorted(slot_of, np.arange(ns + 1), side="left").astype(np.int64)
    return runs, slot_off, np.arange(runs.size, dtype=np.int64)


def _const_to_variable_scan(v_shift_c_rate, frm_rate_ms, fs):
    """
    magphase.py:1426-1449 (Q16): serial backward scan pos_{k-1} = pos_k - lerp(shift)(pos_k) from the last
    constant-rate centre until the position leaves the grid.  Runs in the library's host function
    mpx_host_const_to_var_scan (scipy interp1d's float64 operation sequence without the per-step Python / scipy call:
    bit-identical results, golden G7; hostmath._const_to_variable_scan_scipy is the literal form the tests compare it with).
    """
    v = np.ascontiguousarray(v_shift_c_rate, dtype=np.float64)
    n = int(v.shape[0])
    step = fs * frm_rate_ms / 1000
    centres = np.ascontiguousarray(step * np.arange(1, n + 1), dtype=np.float64)
    shifts, locs = np.empty(2 * n), np.empty(2 * n)
    start = int(_lib.load().mpx_host_const_to_var_scan(centres.ctypes.data, v.ctypes.data, n, shifts.ctypes.data,
                                                       locs.ctypes.data))
    if start < 0:
        return hm._const_to_variable_scan_scipy(v_shift_c_rate, frm_rate_ms, fs)
    return shifts[start:], locs[start:]


def const_to_variable_scan_uncapped(v_shift_c_rate, frm_rate_ms, fs):
    """
    get_shifts_and_frm_locs_from_const_shifts (magphase.py:1426-1449) run to the start of the grid: the reference keeps 2n
    slots, and an utterance that needs more than 2n - 1 pitch-synchronous frames loses its head there (a zero-shift
    frame is left at slot 0).  mpx_host_const_to_var_scan_cap with a capacity from the grid length and the smallest shift:
    where 2n slots suffice, the result is _const_to_variable_scan's, element for element.  n == 1: one frame at the single
    centre; n == 0: no frame.  Shifts must be finite and > 0 (ValueError).
    """
    v = np.ascontiguousarray(v_shift_c_rate, dtype=np.float64)
    n = int(v.shape[0])
    if n == 0:
        return np.zeros(0), np.zeros(0)
    if not np.all(np.isfinite(v)) or np.any(v <= 0.0):
        raise ValueError("constant-rate shifts must be finite and > 0 (f0 >= 0 and finite)")
    step = fs * frm_rate_ms / 1000
    centres = np.ascontiguousarray(step * np.arange(1, n + 1), dtype=np.float64)
    cap = int((centres[-1] - centres[0]) // float(v.min())) + 4   # every step moves by at least min(v)
    shifts, locs = np.empty(cap), np.empty(cap)
    start = int(_lib.load().mpx_host_const_to_var_scan_cap(centres.ctypes.data, v.ctypes.data, n, shifts.ctypes.data,
                                                           locs.ctypes.data, cap))
    if start < 0:
        raise _lib.MagphaseHipError("mpx_host_const_to_var_scan_cap failed (%d)" % start)
    return shifts[start:].copy(), locs[start:].copy()


def plan_const_rate_synthesis(f0_list, fs_list, const_rate_ms):
    """
    Host side of LosslessConstRateSynthesisPlan, float64 (no device): per utterance with rows, f0 -> shifts
    (magphase.py:848), const_to_variable_scan_uncapped, hostmath.const_to_variable_rows on the voicing f0 > 1.0 (one
    row: every frame takes it), shift_to_f0 (b_smooth=False).  Returns a
    dict of per-utterance lists over the utterances with rows ("live", their indices): v_shift, v_locs, v_voi, v_f0, and
    the batch's row tables row0 / row1 (offset by the rows of the utterances before) and rowt; n_rows per utterance.
    Raises ValueError on const_rate_ms <= 0 and on f0 that gives no positive finite shift.
    """
    cr = hm.check_const_rate_ms(const_rate_ms)
    n_rows = [int(np.size(f)) for f in f0_list]
    row_base = np.concatenate(([0], np.cumsum(n_rows))).astype(np.int64)
    r = {k: [] for k in ("live", "v_shift", "v_locs", "v_voi", "v_f0", "row0", "row1", "rowt")}
    for u, n in enumerate(n_rows):
        if n == 0:
            continue
        f0c, fs = np.asarray(f0_list[u], dtype=np.float64), fs_list[u]
        if not np.all(np.isfinite(f0c)) or np.any(f0c < 0.0):
            raise ValueError("v_f0 of utterance %d: values must be finite and >= 0" % u)
        v_shift, v_locs = const_to_variable_scan_uncapped(hm.f0_to_shift(f0c, fs), cr, fs)
        if n == 1:
            lo = hi = np.zeros(v_locs.size, dtype=np.int64)
            t, v_voi = np.zeros(v_locs.size), np.full(v_locs.size, bool(f0c[0] > 1.0))
        else:
            lo, hi, t, v_voi = hm.const_to_variable_rows(f0c > 1.0, v_locs, cr, fs)
        for k, v in (("live", u), ("v_shift", v_shift), ("v_locs", v_locs), ("v_voi", v_voi),
                     ("v_f0", hm.shift_to_f0(v_shift, v_voi, fs)), ("row0", lo + row_base[u]),
                     ("row1", hi + row_base[u]), ("rowt", t)):
            r[k].append(v)
    for k in ("row0", "row1"):
        r[k] = np.concatenate(r[k]) if r[k] else np.zeros(0, np.int64)
    r["rowt"] = np.concatenate(r["rowt"]) if r["rowt"] else np.zeros(0)
    r["n_rows"] = n_rows
    return r


def plan_synthesis_numpy(lf0s, fs, N, b_const_rate, b_voi_ap_win, const_rate_ms=5.0, type2=False):
    """
    The per-utterance index arithmetic of synthesis_from_compressed in numpy, reference line by reference line; returns
    the batch's tables in hostplan.plan_synthesis' layout.  The native planner (csrc/magphase_plan.cpp) is this, for the
    whole batch in one call; this form raises what the reference's arithmetic raises and is what the tests compare the
    native one with.
    const_rate_ms: the grid's period (the native planner knows 5 ms only).  type2: the voicing rules of
    synthesis_from_compressed_type2 (magphase.py:1511-1512, :1524) -- on the grid f0 > 0.0 counts as voiced, and after
    the interpolation a frame is voiced when fs / shift of a voiced frame exceeds 1.
    """
    keys = ("v_shift", "v_pm", "npos", "nleft", "nright", "wtype", "voiced", "row0", "row1", "rowt", "win_l", "win_r",
            "pm_rel")
    acc = {k: [] for k in keys}
    ns_lens, starts, lens, nfr = [], [], [], []
    row_base, noise_base = 0, 0
    for lf0 in lf0s:
        lf0 = np.atleast_1d(np.asarray(lf0, dtype=np.float64))
        n_rows = lf0.shape[0]
        v_f0 = np.exp(lf0)                                         # magphase.py:846
        v_voi = v_f0 > 1.0                                         # :847
        v_shift = hm.f0_to_shift(v_f0, fs)                         # :848
        if b_const_rate:                                           # :861-870
            if type2:
                v_voi = v_f0 > 0.0                                 # :1511
            v_shift, v_locs = _const_to_variable_scan(v_shift, const_rate_ms, fs)
            lo, hi, t, v_voi = hm.const_to_variable_rows(v_voi, v_locs, const_rate_ms, fs)
            if type2:
                v_voi = (v_voi * fs / v_shift.astype("float64")) > 1   # :1512 (shift_to_f0), :1524
        else:
            lo = hi = np.arange(n_rows)
            t = np.zeros(n_rows)
        v_shift = v_shift.astype(int)                              # :879
        v_pm = np.cumsum(v_shift)                                  # :880
        n = v_pm.size
        if type2 and n < 2:   # (the reference indexes v_pm[-2], :1519)
            raise ValueError("utterance %d: fewer than two synthesis frames" % len(nfr))
        ns_len = int(v_pm[-1] + (v_pm[-1] - v_pm[-2]))             # :882
        _, lft, rgt = hm.frame_bounds(v_pm, ns_len)                # windowing(v_ns, v_pm): magphase.py:77-98
        if np.any(lft > N // 2) or np.any(rgt + 1 > N // 2):
            raise ValueError("negative dimensions are not allowed")   # np.zeros(<0) in la.frm_list_to_matrix
        se = np.r_[v_shift[0], v_shift, v_shift[-1], v_shift[-1]]   # :969
        wl, wr = se[:n] + se[1:n + 1], se[2:n + 2] + se[3:n + 3]
        if np.any(wl > N // 2) or np.any(wr + 1 > N // 2):
            raise ValueError("could not broadcast input array (anti-ringing window longer than the frame)")
        rel, start, out_len = hm.ola_plan(v_pm, N)
        for k, v in (("v_shift", v_shift), ("v_pm", v_pm), ("npos", v_pm + noise_base), ("nleft", lft), ("nright", rgt),
                     ("wtype", (v_voi & bool(b_voi_ap_win)).astype(np.int32)), ("voiced", v_voi.astype(np.int32)),
                     ("row0", lo + row_base), ("row1", hi + row_base), ("rowt", t), ("win_l", wl), ("win_r", wr),
                     ("pm_rel", rel)):
            acc[k].append(v)
        ns_lens.append(ns_len), starts.append(start), lens.append(out_len), nfr.append(n)
        row_base += n_rows
        noise_base += ns_len
    i32 = ("nleft", "nright", "wtype", "voiced", "row0", "row1", "win_l", "win_r")
    out = {k: (np.concatenate(v).astype(np.int32 if k in i32 else (np.float64 if k == "rowt" else np.int64))
               if v else np.zeros(0)) for k, v in acc.items()}
    out.update(frame_off=np.concatenate(([0], np.cumsum(nfr))).astype(np.int64), ns_len=np.asarray(ns_lens, dtype=np.int64),
               out_start=np.asarray(starts, dtype=np.int64), out_len=np.asarray(lens, dtype=np.int64))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# Whole-launch planners (mpx_host_plan_analysis_batch / mpx_host_plan_synthesis_batch) through the marshalling layer
# _mpx_pyhost (csrc/magphase_pyhost.cpp): the utterance list is walked once in native code, the interpreter lock is
# released for the call.  Used by Engine.prepare_analysis / prepare_synthesis; the list-based functions above stay as the
# generic path (any array-like input) and as what the tests compare against.
# ----------------------------------------------------------------------------------------------------------------------
_PYHOST = False


def pyhost():
    """The _mpx_pyhost extension module, or None (not built: no Python.h at build time; MAGPHASE_PYHOST=0)."""
    global _PYHOST
    if _PYHOST is False:
        _PYHOST = None
        if enabled() and os.environ.get("MAGPHASE_PYHOST", "1") != "0":
            try:
                _lib.load()                      # the extension links against the C-ABI library
                from . import _mpx_pyhost
                _PYHOST = _mpx_pyhost
            except Exception:
                _PYHOST = None
    return _PYHOST


# order of the device tables mpx_host_plan_synthesis_batch lays out in its `desc` buffer: (name, numpy dtype)
SYNTH_TABLES = (("utt_frame_off", np.int32), ("npos", np.int64), ("nleft", np.int32), ("nright", np.int32),
                ("wtype", np.int32), ("voiced", np.int32), ("tile_first", np.int32), ("row0", np.int32),
                ("row1", np.int32), ("rowt", np.float32), ("win_l", np.int32), ("win_r", np.int32), ("pm_rel", np.int32),
                ("out_start", np.int32), ("out_off", np.int64), ("runs", np.uint8), ("slot_off", np.int32),
                ("slot_runs", np.int32))


def synth_desc_bytes(n_rows, n_utts, n_slots, b_const_rate):
    """Upper bound of the bytes mpx_host_plan_synthesis_batch writes into `desc`."""
    cap = (2 * int(n_rows) + 2 * int(n_utts)) if b_const_rate else int(n_rows)
    runs = int(n_utts) + int(n_slots) + 1
    return 52 * cap + 4 * (int(n_rows) // 31 + 3) + 16 * (int(n_utts) + 1) + 60 * runs + 4 * (int(n_slots) + 1) + 256 * 20
