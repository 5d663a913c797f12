"""
Host-side float64 index arithmetic of the MagPhase hot path.

The reference computes every epoch / shift / frame index in float64 numpy with np.round (half-to-even),
truncating int casts and sequential cumsum.  "Bit-exact indices" means reproducing
that IEEE-754 op sequence, so it stays on the host in numpy and is never recomputed on the device.
Reference lines are cited per function.
"""
import warnings

import numpy as np

MAGIC = -1.0e10  # libaudio.py:17


def round_to_int(x):
    """libutils.py:131-133."""
    return np.round(x).astype(int)


def define_alpha(fs):
    """magphase.py:3279-3290."""
    table = {16000: 0.58, 22050: 0.65, 44100: 0.76, 48000: 0.77}
    if fs not in table:
        raise ValueError("Sample rate %d not supported yet." % fs)
    return table[fs]


def define_fft_len(fs):
    """magphase.py:3292-3299."""
    if fs in (22050, 16000):
        return 2048
    if fs == 8000:
        return 1024
    return 4096


def define_crossfade_params(fs):
    """magphase.py:3301-3317."""
    crsf_bw = 2000
    if fs == 48000:
        return 5000, crsf_bw
    if fs == 16000:
        return 2500, crsf_bw
    warnings.warn("Constant crsf_cf not tested nor tunned to synthesise at fs=%d Hz." % fs)
    return (4500 if fs == 44100 else 3500), crsf_bw


def clean_epochs(v_pm_sec, v_voi, check_len_smpls=-1, fs=-1):
    """libaudio.py:435-447: the two protections applied to REAPER's epoch list."""
    if (check_len_smpls > 0) and (fs == -1):
        raise ValueError("If check_len_smpls given, fs must be provided as well.")
    v_pm_sec = np.asarray(v_pm_sec, dtype=np.float64)
    v_voi = np.asarray(v_voi, dtype=np.float64)
    keep = np.hstack((True, np.diff(v_pm_sec) > 0))
    v_pm_sec, v_voi = v_pm_sec[keep], v_voi[keep]
    if check_len_smpls > 0:
        pm = round_to_int(v_pm_sec * fs)
        if pm[-1] >= (check_len_smpls - 1):
            keep2 = pm < (check_len_smpls - 1)
            v_pm_sec, v_voi = v_pm_sec[keep2], v_voi[keep2]
    return v_pm_sec, v_voi


def frame_bounds(v_pm_smpls, n_smpls):
    """
    magphase.py:77-83,90-98: epochs rounded (Q1), extended with 0 and n-1 (Q4).
    Returns (pm int64[F], left int64[F], right int64[F]); left is the reference's v_shift.
    """
    pm = round_to_int(np.asarray(v_pm_smpls))
    ext = np.hstack((0, pm, n_smpls - 1))
    return pm.astype(np.int64), (ext[1:-1] - ext[:-2]).astype(np.int64), (ext[2:] - ext[1:-1]).astype(np.int64)


def two_period_frame_bounds(pm, n_smpls):
    """
    magphase.py:2806-2816: analysis_lossless_type2 analyses the even and the odd epochs separately (windowing of each
    subset, magphase.py:77-98) and interleaves the rows again, so frame i spans the rounded epochs i-2 .. i+2, with 0
    and n - 1 as the outer limits.  pm: the rounded epochs (frame_bounds).  Returns (left int64[F], right int64[F]).
    """
    pm = np.asarray(pm, dtype=np.int64)
    ext = np.hstack((0, 0, pm, n_smpls - 1, n_smpls - 1)).astype(np.int64)
    return pm - ext[:-4], ext[4:] - pm


def type2_shift(v_pm_smpls):
    """magphase.py:2821: la.pm_to_shift(v_pm_smpls[1:]) of the UNROUNDED epochs, float64 (the first entry is pm[1])."""
    v_pm_smpls = np.asarray(v_pm_smpls, dtype=np.float64)
    return np.diff(np.hstack((0, v_pm_smpls[1:])))


def shift_to_f0(v_shift, v_voi, fs):
    """magphase.py:2198-2207 with b_smooth=False (Q2)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return v_voi * fs / v_shift.astype("float64")


def f0_to_shift(v_f0_in, fs, unv_frm_rate_ms=5):
    """magphase.py:2210-2215 (Q3)."""
    v_f0 = np.array(v_f0_in, dtype=np.float64)
    v_f0[v_f0 == 0] = 1000.0 / unv_frm_rate_ms
    return fs / v_f0


def medfilt3_batch(vectors):
    """scipy.signal.medfilt(v) (kernel 3, zero-padded ends) for a list of 1-D float64 vectors in ONE numpy pass: the
    vectors are laid end to end with a zero between them (the padding scipy adds), the median of every three neighbours is
    their sum minus their minimum and maximum -- exact (all three operands are the inputs themselves: the median is
    selected, not computed).  Returns a list of arrays equal to [signal.medfilt(v) for v in vectors] bit for bit."""
    sizes = [int(np.size(v)) for v in vectors]
    if not sizes:
        return []
    total = int(sum(sizes)) + len(sizes) + 1
    cat = np.zeros(total, dtype=np.float64)
    starts = np.cumsum([1] + [n + 1 for n in sizes[:-1]])
    for v, a, n in zip(vectors, starts, sizes):
        cat[a:a + n] = v
    lo, mid, hi = cat[:-2], cat[1:-1], cat[2:]
    med = np.maximum(np.minimum(lo, mid), np.minimum(np.maximum(lo, mid), hi))   # median of three by selection
    return [med[a - 1:a - 1 + n] for a, n in zip(starts, sizes)]


HANN_TABLE_CAP = 2048   # half lengths covered by hann_half_table (F0 >= 23.4 Hz at 48 kHz); longer halves: analytic window


def hann_half_table(cap=HANN_TABLE_CAP):
    """
    The rising halves np.hanning(2 h + 1)[0 .. h] for every half length h <= cap, laid end to end (half h at offset
    h (h + 1) / 2; (cap + 1)(cap + 2) / 2 float64 values, 16.8 MB at cap = 2048).  Built with numpy's own np.hanning -- the
    function the reference windows with (libaudio.py:70-84: both halves of a frame are rising halves, the right one
    flipped) -- so that mpx_analysis_frames_f64w multiplies by the reference's very weights.  np.hanning(1) = [1.0].
    """
    out = np.empty((cap + 1) * (cap + 2) // 2, dtype=np.float64)
    for h in range(cap + 1):
        off = h * (h + 1) // 2
        out[off:off + h + 1] = np.hanning(2 * h + 1)[:h + 1]
    return out


def ola_plan(v_pm, frmlen):
    """
    Index bookkeeping of magphase.py:34-62 (ola): returns (pm_rel int64[F], out_start, out_len) such that
    out[t] = sum_i frame_i[t + out_start - pm_rel[i]].  Python slice semantics are kept, including the
    negative-start case ``v_sig[(frmlen/2 - pm_0):]`` when the first epoch lies beyond frmlen/2.
    """
    v_pm = np.asarray(v_pm).astype(int)
    buf_len = int(v_pm[-1]) + frmlen
    start = frmlen // 2 - int(v_pm[0])
    if start < 0:
        start = max(buf_len + start, 0)
    start = min(start, buf_len)
    len1 = buf_len - start
    last_shift = int(v_pm[-1] - v_pm[-2]) if v_pm.size > 1 else int(v_pm[-1])
    stop = int(v_pm[-1]) + last_shift + 1
    if stop < 0:
        stop = max(len1 + stop, 0)
    out_len = min(len1, stop)
    return (v_pm - v_pm[0]).astype(np.int64), int(start), int(out_len)


# numpy record layout of the C struct mpx_ola_run (include/magphase_hip.h), 56 bytes
OLA_RUN_DTYPE = np.dtype([("frame_begin", "<i4"), ("frame_end", "<i4"), ("x0", "<i4"), ("head_end", "<i4"),
                          ("out_lo", "<i4"), ("out_hi", "<i4"), ("flush_end", "<i4"), ("fix_lo", "<i4"),
                          ("fix_hi", "<i4"), ("pad", "<i4"), ("out_base", "<i8"), ("strip_off", "<i8")])


# numpy record layout of the C struct mpx_pack_desc (include/magphase_hip.h), 32 bytes, and its element type codes
ROWS_PACK_DTYPE = np.dtype([("base", "<u8"), ("row_stride", "<i8"), ("dtype", "<i4"), ("n_rows", "<i4"),
                            ("out_row0", "<i8")])
ROWS_PACK_CODES = {"torch.float32": 0, "torch.float16": 1, "torch.bfloat16": 2, "torch.float64": 3}


def check_feature_tensor(t, name, lf0=False):
    """Argument check of a torch tensor given where the batch API takes a feature matrix (lf0: the lf0 vector): float32,
    float16, bfloat16 or float64 -- integer, bool and complex tensors are refused, and so is a float16 lf0 (the unvoiced
    marker -1e10 is not representable in float16).  Needs no device."""
    if str(t.dtype) not in ROWS_PACK_CODES:
        raise ValueError("%s: dtype %s is not supported (float32, float16, bfloat16 or float64)" % (name, t.dtype))
    if lf0 and str(t.dtype) == "torch.float16":
        raise ValueError("%s: a float16 lf0 cannot hold the unvoiced marker -1e10 (float32, bfloat16 or float64)" % name)
    if lf0 and t.dim() != 1:
        raise ValueError("%s: must be 1-D, got %d-D" % (name, t.dim()))
    if not lf0 and t.dim() != 2:
        raise ValueError("%s: must be 2-D [rows x width], got %d-D" % (name, t.dim()))


def wants_grad(return_device, candidates, cpu_too=False):
    """THE rule for running a call inside its torch.autograd.Function (magphase_amd/autograd.py): the result stays on the
    device, torch is loaded, grad mode is on, and one of candidates (the call's flattened differentiable inputs, tensors
    or host arrays) is a tensor that is not on the CPU and requires grad -- a CPU tensor is a host array to every path.
    cpu_too: a CPU tensor that requires grad counts as well (la.true_envelope_batch alone).  Imports neither torch nor the
    engine."""
    import sys

    torch = sys.modules.get("torch")
    return bool(return_device and torch is not None and torch.is_grad_enabled()
                and any(torch.is_tensor(x) and x.requires_grad and (cpu_too or x.device.type != "cpu")
                        for x in candidates))


def rows_pack_table(streams):
    """
    The descriptor table of mpx_rows_pack: streams is a list (at most three) of lists of 2-D tensors, streams[s][u] =
    the rows of utterance u in stream s, unit column stride, float32 / float16 / bfloat16 / float64.  A pure function of
    the tensors' shapes, strides, dtypes and data_ptr()s (CPU tensors serve as well as device ones).
    Returns (table, widths, rows): a ROWS_PACK_DTYPE array of len(streams) * U entries, entry [s * U + u], the utterances
    of a stream one after the other in its output; per stream the row width and the total number of rows.
    """
    if not 0 < len(streams) <= 3:
        raise ValueError("rows_pack_table: one to three streams")
    U = len(streams[0])
    if any(len(st) != U for st in streams):
        raise ValueError("rows_pack_table: every stream needs one tensor per utterance")
    table = np.zeros(len(streams) * U, dtype=ROWS_PACK_DTYPE)
    widths, rows = [], []
    for s, st in enumerate(streams):
        width, row0 = None, 0
        for u, t in enumerate(st):
            code = ROWS_PACK_CODES.get(str(t.dtype))
            if code is None:
                raise ValueError("rows_pack_table: stream %d, utterance %d: dtype %s (float32, float16, bfloat16 or float64)"
                                 % (s, u, t.dtype))
            if t.dim() != 2:
                raise ValueError("rows_pack_table: stream %d, utterance %d: %d-D, expected [rows x width]" % (s, u, t.dim()))
            n, w = int(t.shape[0]), int(t.shape[1])
            if width is not None and w != width:
                raise ValueError("rows_pack_table: stream %d, utterance %d: %d columns, the stream has %d" % (s, u, w, width))
            width = w
            if w > 1 and n > 0 and int(t.stride(1)) != 1:
                raise ValueError("rows_pack_table: stream %d, utterance %d: column stride %d (must be 1)"
                                 % (s, u, int(t.stride(1))))
            if n >= 1 << 31:
                raise ValueError("rows_pack_table: stream %d, utterance %d: too many rows" % (s, u))
            e = table[s * U + u]
            e["base"] = int(t.data_ptr()) if n and w else 0
            e["row_stride"] = int(t.stride(0)) if n > 1 else w   # (the stride of a single row is never used)
            e["dtype"], e["n_rows"], e["out_row0"] = code, n, row0
            row0 += n
        widths.append(int(width or 0))
        rows.append(int(row0))
    return table, widths, rows


def _run_cuts(rel, N, target):
    """
    Frame indices at which one utterance's frames are cut into runs of about ``target`` frames, such that only ADJACENT
    runs overlap in the OLA buffer: rel[cut_{k+1}] - rel[cut_k - 1] >= N for every run k with both neighbours
    (a frame covers [rel, rel + N)).  Returns int64 cuts, cuts[0] == 0, cuts[-1] == n.
    """
    n = int(rel.size)
    k = max(1, min(n, int(round(n / float(max(1, target))))))
    cuts = np.round(np.linspace(0, n, k + 1)).astype(np.int64)
    if k > 2:
        inner = cuts[1:-1]   # runs 1 .. k-2 have both neighbours: span from the frame before their first to the next run's first
        ok = np.all(rel[inner[1:]] - rel[inner[:-1] - 1] >= N)
    else:
        ok = True
    if ok and (k < 2 or np.all(np.diff(cuts) > 0)):
        return cuts
    # rare (tiny utterances, tiny targets): greedy left-to-right
    out = [0]
    fb = 0
    while True:
        fe = min(n, fb + max(1, int(target)))
        if fb > 0:
            while fe < n and rel[fe] - rel[fb - 1] < N:
                fe += 1
        if fe >= n:
            break
        out.append(fe)
        fb = fe
    out.append(n)
    return np.asarray(out, dtype=np.int64)


def _enforce_span(rel, N, cuts):
    """Moves (or, where there is no room, drops) cuts until every run with both neighbours satisfies
    rel[next run's first] - rel[own first - 1] >= N: a cut that comes too early is moved forward to the first frame
    that is far enough, as long as that leaves its successor a frame; otherwise the run grows into its successor.
    (Round 4: until then a violating cut was always dropped -- one slot idle and its neighbour with twice the frames;
    with shares below ~25 frames per run that made the pair kernels 45 % slower.)"""
    cuts = [int(c) for c in cuts]
    rel = np.asarray(rel)
    k = 1
    while k < len(cuts) - 2:
        need = int(rel[cuts[k] - 1]) + N
        if rel[cuts[k + 1]] < need:
            c2 = int(np.searchsorted(rel, need, side="left"))   # rel ascends within an utterance
            if c2 < cuts[k + 2]:
                cuts[k + 1] = c2     # the run takes the first frames of its successor's share
                k += 1
            else:
                del cuts[k + 1]      # no frame of the successor is far enough: the run grows into it
        else:
            k += 1
    return np.asarray(cuts, dtype=np.int64)


def slot_cuts(total, n_slots, weights=None):
    """Frame indices that deal `total` frames to the slots: equal shares, or shares in proportion to `weights` (the
    slots' relative speeds, mpx_synth_ola_slot_weights).  int64[min(n_slots, max(total, 1)) + 1], cuts[0] == 0."""
    ns = min(max(1, int(n_slots)), max(int(total), 1))
    if weights is None:
        return np.round(np.linspace(0, total, ns + 1)).astype(np.int64)
    w = np.asarray(weights, dtype=np.float64)[:ns]
    if w.size != ns or np.any(w <= 0):
        raise ValueError("slot weights must be positive, one per slot")
    return np.round(total * np.concatenate(([0.0], np.cumsum(w))) / w.sum()).astype(np.int64)


def deal_cuts(terms, coef):
    """Consecutive shares of the frame sequence whose LARGEST slot cost is minimal (the literal form of
    mpx_host_deal_cuts, bit for bit).  terms: int [n_frames, n_terms], coef: int [n_slots, n_terms], none negative; frame
    f costs slot s  sum_k coef[s, k] * terms[f, k]  (int64).  The smallest integer T for which the greedy fill -- slots
    0, 1, ... each take the longest run of consecutive frames whose summed cost is <= T -- consumes every frame, by
    bisection (a larger T never consumes fewer frames).  Returns (cuts int64[n_slots + 1], T): cuts[0] == 0, ascending,
    cuts[-1] == n_frames; trailing slots may be empty."""
    coef = np.asarray(coef, dtype=np.int64)
    if coef.ndim != 2 or coef.shape[0] < 1 or coef.shape[1] < 1:
        raise ValueError("deal_cuts: coef must be [n_slots, n_terms]")
    terms = np.asarray(terms, dtype=np.int64).reshape(-1, coef.shape[1])
    if np.any(terms < 0) or np.any(coef < 0):
        raise ValueError("deal_cuts: terms and coefficients must not be negative")
    n, ns = int(terms.shape[0]), int(coef.shape[0])
    # slots with equal coefficients share one prefix-sum array: prefix[c][i] = cost of the frames [0, i) in class c
    rows, cls = [], np.empty(ns, dtype=np.int64)
    for s in range(ns):
        key = tuple(coef[s].tolist())
        if key not in rows:
            rows.append(key)
        cls[s] = rows.index(key)
    prefix = [np.concatenate(([0], np.cumsum(terms @ np.asarray(k, dtype=np.int64)))).astype(np.int64) for k in rows]
    cls = cls.tolist()

    def fill(T):
        cuts, i = [0], 0
        for s in range(ns):
            p = prefix[cls[s]]
            i = int(np.searchsorted(p, p[i] + T, side="right")) - 1   # the last j >= i with p[j] - p[i] <= T
            cuts.append(i)
        return cuts

    lo, hi = 0, max(int(p[n]) for p in prefix)   # with T = the dearest class's cost of the batch slot 0 takes everything
    while lo < hi:
        mid = lo + (hi - lo) // 2
        if fill(mid)[-1] == n:
            hi = mid
        else:
            lo = mid + 1
    return np.asarray(fill(lo), dtype=np.int64), lo


def roundtrip_frame_terms(left, right, fft_len):
    """mpx_roundtrip_frame_terms in numpy (what the round-trip plan falls back to without the native planners): per frame
    (1, active_rows, extra_tiles) of k_roundtrip_pair's analysis -- noise_fft's tile count and row test (csrc/mpx_common.hpp:
    frame_cost_terms) on len = min(L + R + 1, N), rot = L if L < N else 0, tiles of 32 P samples for P = N / 128 = 32 and
    64 P otherwise.  int32 [n_frames, 3]."""
    N = int(fft_len)
    P = N // 128
    L, Rr = np.asarray(left, dtype=np.int64).reshape(-1), np.asarray(right, dtype=np.int64).reshape(-1)
    ln = np.minimum(L + Rr + 1, N)
    rot = np.where(L < N, L, 0)
    tile = (32 if P == 32 else 64) * P
    ntiles = (ln + tile - 1) // tile
    m0 = 128 * np.arange(P, dtype=np.int64)[None, :]
    rows = ((m0 < (ln - rot)[:, None]) | (m0 + 127 >= (N - rot)[:, None])).sum(axis=1)
    return np.stack([np.ones_like(ln), rows * ntiles, ntiles - 1], axis=1).astype(np.int32)


def roundtrip_support_classes(left, right, fft_len):
    """mpx_roundtrip_support_classes in numpy (csrc/mpx_common.hpp: frame_support_class): class W of a frame of
    k_roundtrip_pair -- its samples lie in the register rows j < W or j >= P - W of the rotated analysis input and in the
    rows P/2 - W <= q < P/2 + W of the rebuilt frame.  4 where N = 4096, 0 <= L <= 512 and 0 <= R <= 511; otherwise the
    full class P / 2 = N / 256.  int32 [n_frames]."""
    N = int(fft_len)
    P = N // 128
    L, Rr = np.asarray(left, dtype=np.int64).reshape(-1), np.asarray(right, dtype=np.int64).reshape(-1)
    narrow = (P == 32) & (L >= 0) & (Rr >= 0) & (L <= 128 * 4) & (Rr <= 128 * 4 - 1)
    return np.where(narrow, 4, P // 2).astype(np.int32)


def roundtrip_frame_extents(left, right, fft_len, full_support=False):
    """mpx_roundtrip_frame_extents in numpy, for the library's default build: per frame the half-open range (ext_lo,
    ext_hi) of its samples that k_roundtrip_pair can add to the overlap-add ring.  A frame of support class W below the
    full one adds the register rows P/2 - W <= q < P/2 + W only (csrc/mpx_common.hpp: support_row_live), samples
    [128 (P/2 - W), 128 (P/2 + W)) -- class 4 at N = 4096: (1536, 2560); every other frame, every other N and every frame
    under full_support (MPX_RT_FULL_SUPPORT: the instance without pruned passes is launched): (0, N).  A library built
    without the pruned instances answers (0, N) throughout; the plans ask the library, never this twin.
    int32 [n_frames, 2]."""
    N = int(fft_len)
    P = N // 128
    W = roundtrip_support_classes(left, right, N).astype(np.int64)
    if full_support:
        W = np.full_like(W, P // 2)
    return np.stack([128 * (P // 2 - W), 128 * (P // 2 + W)], axis=1).astype(np.int32)


def roundtrip_store_map(fft_len, phase):
    """mpx_roundtrip_store_map in numpy (csrc/mpx_common.hpp, "Row stores by line"): how k_roundtrip_pair's line-aligned
    forms store one feature row of M + 1 = fft_len / 2 + 1 floats whose float 0 lies `phase` (0 ... 31) floats into a
    128-byte line.  Per store of a plane in issue order -- (ascending q, mirror q) for q = 0 ... P/2 - 1, the ascending tail,
    the mirror tail: 2 (P/2) + 2 = 34 -- the row float each of the 64 lanes writes, -1 where the lane is masked.  Lane l
    holds the own bin l + 64 q and its mirror M - l - 64 q at step q; block B_c = floats [64 c - phase, 64 c - phase + 63] is
    two whole lines of memory.  Ascending: the lanes < 64 - phase store step q's value, the others step q - 1's 64 floats
    lower (none at q = 0; their last values are the tail).  Mirrors: the lanes <= phase store step q's mirror, the others
    step q - 1's 64 floats higher (none at q = 0); the tail is bin M/2 from lane 0 and the last step's mirrors from the
    lanes > phase.  Only fft_len 4096 has these forms.  int32 [34, 64]."""
    if int(fft_len) != 4096:
        raise ValueError("roundtrip_store_map: only fft_len 4096 has the line-aligned stores")
    s = int(phase)
    if not 0 <= s <= 31:
        raise ValueError("roundtrip_store_map: phase must be 0 ... 31")
    P = int(fft_len) // 128
    HP, M = P // 2, 64 * P
    lane = np.arange(64, dtype=np.int64)
    prev, cur = lane >= 64 - s, lane <= s
    asc = lane - np.where(prev, 64, 0)
    mir = np.where(cur, M - 64 - lane, M - lane)
    out = np.full((2 * HP + 2, 64), -1, dtype=np.int64)
    for q in range(HP):
        out[2 * q] = np.where(prev & (q == 0), -1, asc + 64 * q)
        out[2 * q + 1] = np.where(~cur & (q == 0), -1, mir - 64 * (q - 1))
    out[2 * HP] = np.where(prev, asc + 64 * HP, -1)
    out[2 * HP + 1] = np.where((lane == 0) | ~cur, mir - 64 * (HP - 1), -1)
    return out.astype(np.int32)


def ola_runs(pm_rel_list, starts, out_lens, out_offs, fft_len, n_slots, frames_per_run=None, weights=None, gcuts=None,
             extents=None):
    """
    Plans the fused overlap-add (include/magphase_hip.h: mpx_synthesis_lossless_ola).  The batch's frames, in utterance
    order, are dealt to the device's pair slots in consecutive shares: equal ones (slot s gets the frames
    [round(s F / n_slots), round((s+1) F / n_slots)) of the concatenated sequence), or, with ``weights`` (one relative
    speed per slot, mpx_synth_ola_slot_weights), shares in proportion to them -- the kernel ends when the slowest slot does.  A share that crosses an utterance boundary is two (or more) RUNS -- the end
    of one utterance and the beginning of the next; runs never cross utterances.  ``frames_per_run`` instead cuts every
    utterance on its own into runs of about that many frames and balances the slots longest-run-first (tests, tuning).
    ``gcuts`` (int64[slots + 1], ascending, gcuts[0] == 0, gcuts[-1] == the frame count; equal neighbours = an empty
    slot) replaces the shares by count: the caller dealt the frames itself (deal_cuts: by cost).
    Per run the positions are classified as head strip / final output / dropped (see mpx_ola_run) in the coordinates
    of the reference's OLA buffer (magphase.py:38-61): frame i covers [pm_rel[i], pm_rel[i] + N), the kept part is
    [start, start + out_len).  Only ADJACENT runs of an utterance may overlap: rel[next run's first frame] -
    rel[own first frame - 1] >= N for every run with both neighbours (a cut violating it is MOVED FORWARD to the first
    frame that satisfies it, _enforce_span; only a cut with no such frame left in the utterance is dropped).

    ``extents`` (int [total frames, 2], or None): per frame the half-open range (ext_lo, ext_hi) of its samples that can be
    non-zero (roundtrip_frame_extents; None: (0, N), a dense frame).  The seams between runs are then sized by what the
    frames really reach: a run ends at hi_t = the largest rel + ext_hi of its frames (and never before its predecessor's
    end), its successor's head strip, the positions both write, ends there, and the fix range begins no earlier than
    lo_t = the smallest rel + ext_lo of the successor's frames.  Everything outside the extents must be an exact zero
    that the kernel never adds to its ring.  The cuts keep their N-wide rule.

    pm_rel_list: per utterance int64[F_u]; starts / out_lens: ola_plan's (out_start, out_len) per utterance;
    out_offs: int64[U+1] offsets of the utterances in pcm_out.
    Returns (runs, slot_off, slot_runs): a structured array (OLA_RUN_DTYPE) of the runs in utterance / frame order and
    the slots' work lists (slot s processes runs slot_runs[slot_off[s] : slot_off[s+1]] in that order).
    """
    N = int(fft_len)
    strip_floats = N + 64
    n_frames = np.asarray([int(np.size(r)) for r in pm_rel_list], dtype=np.int64)
    total = int(n_frames.sum())
    n_slots = max(1, int(n_slots))
    if frames_per_run:
        target, gcuts = int(frames_per_run), None
    else:
        target = max(1, -(-total // n_slots))
        gcuts = slot_cuts(total, n_slots, weights) if gcuts is None else np.asarray(gcuts, dtype=np.int64)
    if extents is not None:
        extents = np.asarray(extents, dtype=np.int64).reshape(-1, 2)
        if extents.shape[0] != total or np.any(extents[:, 0] < 0) or np.any(extents[:, 1] < extents[:, 0]) \
                or np.any(extents[:, 1] > N):
            raise ValueError("ola_runs: extents must be [total frames, 2] with 0 <= ext_lo <= ext_hi <= N")
    recs = []
    f_base = 0
    for u, rel in enumerate(pm_rel_list):
        rel = np.asarray(rel, dtype=np.int64)
        n = int(rel.size)
        if n == 0:
            continue
        start, out_len, o0 = int(starts[u]), int(out_lens[u]), int(out_offs[u])
        if gcuts is None:
            cuts = _run_cuts(rel, N, target)
        else:   # the global cuts that fall inside this utterance
            inner = gcuts[(gcuts > f_base) & (gcuts < f_base + n)] - f_base
            cuts = _enforce_span(rel, N, np.concatenate(([0], inner, [n])))
        fb, fe = cuts[:-1], cuts[1:]
        k = fb.size
        hi = rel[fe - 1] + N                          # end of the run's last frame
        lo_t = rel[fb]                                # beginning of its first
        if extents is not None:   # ... of what its frames reach, and never before the end of the previous run
            p_lo, p_hi = rel + extents[f_base:f_base + n, 0], rel + extents[f_base:f_base + n, 1]
            hi, lo_t, reach = hi.copy(), lo_t.copy(), 0
            for i in range(k):
                if fe[i] > fb[i]:
                    reach = max(reach, int(p_hi[fb[i]:fe[i]].max()))
                    lo_t[i] = p_lo[fb[i]:fe[i]].min()
                hi[i] = reach
        prev_hi = np.concatenate(([0], hi[:-1]))      # positions < prev_hi also get the previous run's frames
        lo_t = np.minimum(lo_t, prev_hi)              # (a head that begins past the predecessor's end: nothing to fix)
        # first position the run is responsible for: its first frame, or the end of the previous run's last frame if
        # that comes first (consecutive frames further apart than N leave a gap of zeros, which this run writes)
        lo = np.minimum(rel[fb], prev_hi)
        # element 0 at a position whose pcm_out index is a multiple of 64 (aligned 256-byte output blocks)
        x0 = lo - ((lo - start + o0) % 64)
        head_end = np.where(np.arange(k) > 0, prev_hi - x0, 0)
        if np.any(head_end > strip_floats):
            raise ValueError("ola_runs: a run's head overlap exceeds the strip (frames not in ascending position order?)")
        # final positions of run k: [prev_hi (0 for the first run), hi_k), the last run up to the end of the kept part
        own_lo = np.where(np.arange(k) > 0, prev_hi, 0)
        own_hi = hi.copy()
        own_hi[-1] = max(int(hi[-1]), start + out_len)
        out_lo = np.maximum(own_lo, start) - x0
        out_hi = np.minimum(own_hi, start + out_len) - x0
        out_hi = np.maximum(out_hi, out_lo)
        flush_end = np.maximum(hi, own_hi) - x0
        fix_lo = np.maximum(np.maximum(lo, lo_t), start) - x0
        fix_hi = np.minimum(prev_hi, start + out_len) - x0
        fix_hi = np.where(np.arange(k) > 0, np.maximum(fix_hi, fix_lo), fix_lo)
        r = np.zeros(k, dtype=OLA_RUN_DTYPE)
        r["frame_begin"], r["frame_end"] = fb + f_base, fe + f_base
        r["x0"], r["head_end"] = x0, head_end
        r["out_lo"], r["out_hi"], r["flush_end"] = out_lo, out_hi, flush_end
        r["fix_lo"], r["fix_hi"] = fix_lo, fix_hi
        r["out_base"] = o0 + x0 - start
        recs.append(r)
        f_base += n
    runs = np.concatenate(recs) if recs else np.zeros(0, dtype=OLA_RUN_DTYPE)
    runs["strip_off"] = np.arange(runs.size, dtype=np.int64) * strip_floats
    if gcuts is None:
        slot_off, slot_runs = balance_chunks(runs["frame_end"] - runs["frame_begin"], n_slots)
    else:   # a run belongs to the share its first frame lies in; shares are consecutive, so are their runs
        ns = gcuts.size - 1
        slot_of = np.clip(np.searchsorted(gcuts, runs["frame_begin"], side="right") - 1, 0, ns - 1)
        slot_off = np.searchsorted(slot_of, np.arange(ns + 1), side="left").astype(np.int64)
        slot_runs = np.arange(runs.size, dtype=np.int64)
    return runs, slot_off, slot_runs


def balance_chunks(n_frames_per_chunk, n_slots, overhead=2):
    """
    Longest-processing-time-first assignment of chunks (already sorted longest first) to wave slots.
    cost(chunk) = frames + overhead (ring tail flush ~ 2 frames' worth of LDS/global work).
    Returns (slot_off int64[n_slots+1], slot_chunks int64[n_chunks]).
    """
    import heapq

    n_frames_per_chunk = np.asarray(n_frames_per_chunk, dtype=np.int64)
    n_slots = int(max(1, min(n_slots, max(1, n_frames_per_chunk.size))))
    heap = [(0, s) for s in range(n_slots)]
    lists = [[] for _ in range(n_slots)]
    for ci in np.argsort(-n_frames_per_chunk, kind="stable"):
        load, s_ = heapq.heappop(heap)
        lists[s_].append(int(ci))
        heapq.heappush(heap, (load + int(n_frames_per_chunk[ci]) + overhead, s_))
    slot_off = np.concatenate(([0], np.cumsum([len(l) for l in lists]))).astype(np.int64)
    slot_chunks = np.asarray([c for l in lists for c in l], dtype=np.int64)
    return slot_off, slot_chunks


# ======================================================================================================
# compressed-feature constants (float64 on the host, uploaded once per (fs, dims) as float32)
# ======================================================================================================
def warp_axis(alpha, nbins):
    """libaudio.py:612-614 / :711-715: all-pass warped frequency axis on nbins points in [0, pi]."""
    w = np.linspace(0, np.pi, num=nbins)
    ww = np.arctan((1 - alpha ** 2) * np.sin(w) / ((1 + alpha ** 2) * np.cos(w) - 2 * alpha))
    ww[ww < 0] += np.pi
    return ww


def build_mel_curve(alpha, nbins, amp=np.pi):
    """libaudio.py:711-718."""
    return warp_axis(alpha, nbins) * (amp / np.pi)


_COS_CACHE = {}


def cos_matrix(n_cep, n_spbins, alpha):
    """libaudio.py:611-619: trans[i, k] = cos(i * warp_alpha(pi k / (n_spbins - 1))), cached per configuration."""
    key = (int(n_cep), int(n_spbins), float(alpha))
    if key not in _COS_CACHE:
        _COS_CACHE[key] = np.cos(np.arange(key[0])[:, None] * warp_axis(key[2], key[1])[None, :])
    return _COS_CACHE[key]


def unwarp_matrix(ncoeffs, nbins_out, alpha):
    """
    la.sp_mel_unwarp(in_type='log') (libaudio.py:667-684) as the matrix it is: out = x @ U,
    U[ncoeffs x nbins_out].  Even extension -> real IFFT -> coefficients 1..ncoeffs-3 doubled (Q6) ->
    cosine matrix on the alpha-warped axis (libaudio.py:605-619).
    """
    eye = np.eye(ncoeffs)
    ext = np.hstack((eye, eye[:, -2:0:-1]))
    ceps = np.fft.ifft(ext).real[:, :ncoeffs]
    ceps[:, 1:(ncoeffs - 2)] *= 2
    cosm = np.cos(np.arange(ncoeffs)[:, None] * warp_axis(alpha, nbins_out)[None, :])
    return ceps @ cosm


def fbank_centres(n_melbands, nbins, alpha):
    """Band centres (linear-frequency bins) of the mel filter bank, libaudio.py:839-846 / :730-736."""
    from scipy import interpolate

    v_bins_warp = build_mel_curve(alpha, nbins, amp=np.pi)
    v_cntrs_mel = np.linspace(0, v_bins_warp[-1], n_melbands)
    f_interp = interpolate.interp1d(v_bins_warp, np.arange(nbins), kind="quadratic")
    return round_to_int(f_interp(v_cntrs_mel))


def warp_fbank_matrix(n_melbands, nbins, alpha):
    """
    la.sp_mel_warp_fbank / apply_fbank(mode='average') (libaudio.py:721-769) as W[n_melbands x nbins] acting on
    ln(mag): band b = the asymmetric Hann window (rising half of np.hanning(1 + 2 l), falling half of
    np.hanning(1 + 2 r), l / r = distances to the neighbouring band centres, first and last centre repeated)
    normalised to unit sum, placed from centre b-1 on.  Same float64 construction as the reference.
    """
    v_cntrs = fbank_centres(n_melbands, nbins, alpha)
    ext = np.r_[v_cntrs[0], v_cntrs, v_cntrs[-1]]
    w = np.zeros((n_melbands, nbins))
    for b in range(1, n_melbands + 1):
        ll, rr = int(ext[b] - ext[b - 1]), int(ext[b + 1] - ext[b])
        win = np.hstack((np.hanning(1 + 2 * ll)[:ll + 1], np.flipud(np.hanning(1 + 2 * rr)[:rr + 1])[1:]))
        win = win / np.sum(win)
        w[b - 1, ext[b - 1]:ext[b - 1] + win.size] = win
    return w


def unwarp_fbank_matrix(n_melbands, nbins, alpha):
    """
    la.sp_mel_unwarp_fbank (libaudio.py:815-864): per frame, a quadratic spline (scipy interp1d) through the band
    centres, evaluated on every bin.  For fixed knots that is linear in the frame, so it is the matrix
    U[n_melbands x nbins] = the spline of each unit vector (same scipy call as the reference).
    """
    from scipy import interpolate

    v_cntrs = fbank_centres(n_melbands, nbins, alpha)
    f_interp = interpolate.interp1d(v_cntrs, np.eye(n_melbands), kind="quadratic", axis=0)
    return f_interp(np.arange(nbins)).T.copy()


def get_num_full_mel_coeffs_from_num_phase_coeffs(freq_hz, phase_dim, alpha, fs):
    """magphase.py:2479-2487."""
    cw = 2 * np.pi * freq_hz / float(fs)
    cf_mel = np.arctan((1 - alpha ** 2) * np.sin(cw) / ((1 + alpha ** 2) * np.cos(cw) - 2 * alpha))
    if cf_mel < 0:
        cf_mel += np.pi
    return int(round_to_int(1 + (np.pi * (phase_dim - 1) / float(cf_mel))))


def phase_unwarp_matrix(phase_dim, fft_len, fs, alpha):
    """
    magphase.py:1219-1235 as a matrix [phase_dim x H]: nearest-neighbour extension phase_dim -> K (the last
    coefficient repeated) followed by the K-coefficient unwarp: rows >= phase_dim-1 of U_K fold into the last row.
    """
    cf = define_crossfade_params(fs)[0]
    k_full = get_num_full_mel_coeffs_from_num_phase_coeffs(cf, phase_dim, alpha, fs)
    u_full = unwarp_matrix(k_full, fft_len // 2 + 1, alpha)
    if k_full <= phase_dim:
        return u_full[:phase_dim].copy() if k_full == phase_dim else np.vstack(
            (u_full, np.zeros((phase_dim - k_full, u_full.shape[1]))))  # (index >= K never read: columns cut)
    u = u_full[:phase_dim].copy()
    u[phase_dim - 1] += u_full[phase_dim:].sum(axis=0)
    return u


def _crossfade_bins(nbins_half, cut_off, bw, fs):
    """libaudio.py:165-169: the crossfade's lower and upper edge as bins."""
    nfft = (nbins_half - 1) * 2
    bin_l = int(round_to_int((cut_off - bw / 2.0) * nfft / float(fs)))
    bin_r = int(round_to_int((cut_off + bw / 2.0) * nfft / float(fs)))
    return bin_l, bin_r


def crossfade_lowpass_curve(nbins_half, cut_off, bw, fs):
    """libaudio.py:160-186 for (ones, zeros): 1 below bin_l, falling Hann half on [bin_l, bin_r], 0 above."""
    bin_l, bin_r = _crossfade_bins(nbins_half, cut_off, bw, fs)
    bw_bin = bin_r - bin_l
    return np.hstack((np.ones(bin_l), np.hanning(2 * bw_bin + 1)[bw_bin:], np.zeros(nbins_half - bin_r - 1)))


def crossfade_highpass_curve(nbins_half, cut_off, bw, fs):
    """libaudio.py:160-186 for (zeros, ones): 0 below bin_l, rising Hann half on [bin_l, bin_r], 1 above -- the
    low-pass curve's window mirrored (np.hanning is symmetric), not 1 - low-pass, which differs in the last bit."""
    bin_l, bin_r = _crossfade_bins(nbins_half, cut_off, bw, fs)
    fall = crossfade_lowpass_curve(nbins_half, cut_off, bw, fs)[bin_l:bin_r + 1]
    return np.hstack((np.zeros(bin_l), fall[::-1], np.ones(nbins_half - bin_r - 1)))


def synthesis_bin_curves(fs, fft_len):
    """
    Per-bin constant vectors of synthesis_from_compressed (magphase.py:873-875, 917-918, 940-941, 946-952):
      per_v = tilt_voiced * sqrt(mask)      periodic component of voiced frames  (0 where mask == 0)
      ap_v  = sqrt(1 - mask)                aperiodic component of voiced frames (0 where mask == 1)
      ap_u  = tilt_unvoiced                 aperiodic component of unvoiced frames (mask == 0 there)
    tilt_voiced = 10**(melcurve(0.6, H, 2.0)/20); tilt_unvoiced = 10**((melcurve(alpha, H, 3.5) - 3.5)/20) (Q13).
    """
    half = fft_len // 2 + 1
    cf, bw = define_crossfade_params(fs)
    alpha = define_alpha(fs)
    mask = crossfade_lowpass_curve(half, cf, bw, fs)
    tilt_v = 10 ** (build_mel_curve(0.6, half, amp=2.0) / 20)
    tilt_u = 10 ** ((build_mel_curve(alpha, half, amp=3.5) - 3.5) / 20)
    return tilt_v * mask ** 0.5, (1 - mask) ** 0.5, tilt_u


def type2_synthesis_bin_curves(fs, fft_len, hf_slope_coeff=1.0):
    """
    Per-bin constant vectors of synthesis_from_compressed_type2 (magphase.py:1544-1553), float64:
      per_v = crossfade low-pass            periodic component of voiced frames (la.spectral_crossfade(mag, 0): plain Hann)
      ap_v  = crossfade high-pass           aperiodic component of voiced frames (la.spectral_crossfade(0, mag / rms))
      ap_u  = linspace(1, hf_slope_coeff)   aperiodic component of unvoiced frames (:1547-1548)
    No square root of the mask and no spectral tilt, unlike synthesis_bin_curves.  per_v is zero from the crossfade's
    upper edge on, ap_v below its lower edge.
    """
    half = fft_len // 2 + 1
    cf, bw = define_crossfade_params(fs)
    return (crossfade_lowpass_curve(half, cf, bw, fs), crossfade_highpass_curve(half, cf, bw, fs),
            np.linspace(1, hf_slope_coeff, num=half))


def type2_phase_unwarp_matrix(phase_dim, mag_dim, nbins_out, alpha):
    """
    magphase.py:1494-1501 as a matrix [phase_dim x nbins_out]: nearest-neighbour extension of the phase coefficients to
    mag_dim columns (the last coefficient repeated) followed by the mag_dim-coefficient unwarp at alpha, so rows
    >= phase_dim - 1 of the unwarp matrix fold into the last row, as in phase_unwarp_matrix.  phase_dim > mag_dim: the
    extension only reads the first mag_dim coefficients (interp1d(...)(np.arange(mag_dim))): the other rows are zero.
    """
    u_full = unwarp_matrix(mag_dim, nbins_out, alpha)
    if phase_dim >= mag_dim:
        return np.vstack((u_full, np.zeros((phase_dim - mag_dim, u_full.shape[1]))))
    u = u_full[:phase_dim].copy()
    u[phase_dim - 1] += u_full[phase_dim:].sum(axis=0)
    return u


# ======================================================================================================
# mel warp (compressed analysis) as a matrix -- SPTK-3.9 ``mcep -j 0`` restated (PARITY UNPINNED: external binary)
# ======================================================================================================
def freqt_matrix(n_in, order_out, alpha):
    """
    Frequency transformation of cepstra by a first-order all-pass (Tokuda et al. 1994; SPTK ``freqt``) as a matrix
    A[(order_out+1) x n_in]: mc = A @ c.  The recursion consumes the input from c[n_in-1] down to c[0]; running it on
    the identity gives the matrix.  alpha == 0 is the identity truncation.
    """
    m2 = int(order_out)
    if alpha == 0.0:
        a_mat = np.zeros((m2 + 1, n_in))
        a_mat[np.arange(min(m2 + 1, n_in)), np.arange(min(m2 + 1, n_in))] = 1.0
        return a_mat
    b = 1.0 - alpha * alpha
    g = np.zeros((n_in, m2 + 1))          # one "frame" per unit input vector
    for i in range(n_in - 1, -1, -1):
        d = g.copy()
        g[:, 0] = alpha * d[:, 0]
        g[i, 0] += 1.0                     # c1[-i] of the unit vector e_i
        if m2 >= 1:
            g[:, 1] = b * d[:, 0] + alpha * d[:, 1]
        for j in range(2, m2 + 1):
            g[:, j] = d[:, j - 1] + alpha * (d[:, j] - g[:, j - 1])
    return g.T.copy()


_WARP_CACHE = {}


def warp_matrix(nbins_out, nbins_half, alpha, nrows=None):
    """
    la.sp_mel_warp (libaudio.py:643-661) as W[nrows x nbins_half] acting on the log-periodogram:
      c[n]  = (1/N) sum_k w_k logP[k] cos(2 pi k n / N), n = 0..N/2   (real IFFT of the even extension; w_0 = w_{N/2} = 1, else 2)
      c[0] /= 2, c[N/2] /= 2 ;  mc = freqt(c, nbins_out - 1, alpha) ;  out[i] = sum_n mc[n] cos(n pi i / (nbins_out - 1))
    alpha is rounded to two decimals as on the mcep command line (libaudio.py:589).  nrows: keep only the first rows
    (the phase features are cut to phase_dim, magphase.py:2523-2524).
    """
    key = (int(nbins_out), int(nbins_half), float("%1.2f" % alpha))
    if key not in _WARP_CACHE:
        nb, half = key[0], key[1]
        n_fft = 2 * (half - 1)
        w = np.full(half, 2.0)
        w[0] = w[-1] = 1.0
        idct = np.cos(2 * np.pi * np.outer(np.arange(half), np.arange(half)) / n_fft) * w[None, :] / n_fft
        idct[0] *= 0.5
        idct[-1] *= 0.5
        a_mat = freqt_matrix(half, nb - 1, key[2])
        cosm = np.cos(np.arange(nb)[:, None] * np.linspace(0, np.pi, nb)[None, :]).T
        _WARP_CACHE[key] = cosm @ (a_mat @ idct)
    wm = _WARP_CACHE[key]
    return wm if nrows is None else wm[:nrows]


def _kappa(P, lane):
    """wave_fft.hpp kappa(lane): the output-index residue a lane holds (identity for P = 32)."""
    lane = np.asarray(lane)
    if P == 32:
        return lane
    if P == 16:
        return (lane & 15) | (((lane >> 5) & 1) << 4) | (((lane >> 4) & 1) << 5)
    return (lane & 7) | (((lane >> 5) & 1) << 3) | (lane & 16) | (((lane >> 3) & 1) << 5)


def fused_chunk_bins(fft_len):
    """Bin of column c of chunk q in mpx_analysis_compressed_fused's published tile: int64[P/2, 128] --
    c < 64: the low bin 64 q + c, c >= 64: its mirror M - 64 q - (c - 64)  (M = fft_len / 2; bin M/2 is not in any chunk)."""
    P = fft_len // 128
    M = fft_len // 2
    q = np.arange(P // 2)[:, None]
    c = np.arange(64)[None, :]
    return np.concatenate((64 * q + c, M - 64 * q - c), axis=1).astype(np.int64)


def pack_warp_fused(w_mag, w_ph, fft_len, n_waves=8, layout=0):
    """
    The two warp matrices ([mag_dim x H] and [phase_dim x H], float64) in the order mpx_analysis_compressed_fused's MFMA
    (v_mfma_f32_16x16x4_f32) consumes them.  A workgroup of n_waves waves (mpx_analysis_compressed_fused_waves) cuts a
    chunk's 128 columns into n_waves slices of 128 / n_waves columns = kh groups of 16:
      wpack[q][wave][h][tile][lane][e] = W_tile[16 jt + (lane & 15)][bin(q, (128 / n_waves) wave + 16 h + 4 (lane >> 4) + e)]
    -- one 16-byte load per lane, tile and 16-column group; tiles = 4 magnitude column tiles, then ceil(phase_dim / 16)
    phase tiles (shared by the real and the imaginary stream); rows past the matrix are zero.
    whalf[tile][16] = the same rows' weight of bin M/2 (added outside the chunks).  Returns (wpack, whalf) float32.

    layout = 1 (mpx_analysis_compressed_fused_layout, n_waves = 8): the magnitude product runs on v_mfma_f32_4x4x1_16b_f32 --
    per (chunk q, wave) eight magnitude fragments, then the phase tiles' fragments as above:
      wpack[q][wave][2 kg + half][lane][e] = W_mag[32 half + (lane & 31)][bin(q, 16 wave + 4 kg + e)]      (kg < 4, half < 2)
      wpack[q][wave][8 + jt][lane][e]      = W_ph[16 jt + (lane & 15)][bin(q, 16 wave + 4 (lane >> 4) + e)]
    whalf is the same in both layouts.
    """
    w_mag, w_ph = np.asarray(w_mag, dtype=np.float64), np.asarray(w_ph, dtype=np.float64)
    H = fft_len // 2 + 1
    assert w_mag.shape[1] == H and w_ph.shape[1] == H and w_mag.shape[0] <= 64 and w_ph.shape[0] <= 48
    assert n_waves in (4, 8)
    ntm, ntp = 4, (w_ph.shape[0] + 15) // 16
    tiles = []
    for src, nt in ((w_mag, ntm), (w_ph, ntp)):
        for jt in range(nt):
            t = np.zeros((16, H))
            rows = src[16 * jt:16 * jt + 16]
            t[:rows.shape[0]] = rows
            tiles.append(t)
    tiles = np.stack(tiles)                                # [T, 16, H]
    bins = fused_chunk_bins(fft_len)                       # [P/2, 128]
    lane = np.arange(64)
    li, g = lane & 15, lane >> 4
    cols, kh = 128 // n_waves, 128 // n_waves // 16
    col = (cols * np.arange(n_waves)[:, None, None, None] + 16 * np.arange(kh)[None, :, None, None]
           + 4 * g[None, None, :, None] + np.arange(4)[None, None, None, :])                    # [wave, h, lane, e]
    b = bins[:, col]                                       # [q, wave, h, lane, e]
    wpack = tiles[:, li[None, None, None, :, None], b]     # [T, q, wave, h, lane, e]
    wpack = np.ascontiguousarray(np.transpose(wpack, (1, 2, 3, 0, 4, 5)), dtype=np.float32)   # [q, wave, h, T, lane, e]
    whalf = np.ascontiguousarray(tiles[:, :, fft_len // 4], dtype=np.float32)   # [T, 16]
    if layout == 1:
        assert n_waves == 8
        wm64 = np.zeros((64, H))
        wm64[:w_mag.shape[0]] = w_mag
        colm = (16 * np.arange(8)[:, None, None] + 4 * np.arange(4)[None, :, None] + np.arange(4)[None, None, :])   # [wave, kg, e]
        bm = bins[:, colm]                                                                     # [q, wave, kg, e]
        rows = 32 * np.arange(2)[:, None] + (lane & 31)[None, :]                               # [half, lane]
        magf = wm64[rows[None, None, None, :, :, None], bm[:, :, :, None, None, :]]            # [q, wave, kg, half, lane, e]
        magf = magf.reshape(bm.shape[0], 8, 8, 64, 4)
        phf = wpack[:, :, 0, ntm:]                                                             # [q, wave, ntp, lane, e]
        out = np.concatenate((magf, phf), axis=2)
        return np.ascontiguousarray(out, dtype=np.float32).reshape(-1), whalf.reshape(-1)
    return wpack.reshape(-1), whalf.reshape(-1)


def var_to_const_rate_table(v_pm_smpls, const_rate_ms, fs):
    """
    Row/weight table of magphase.py:2219-2239 (Q15): grid arange(step, pm[-1], step); the first row is duplicated at
    t = 0 when pm[0] > 0.  Returns (row_lo, row_hi int64[Fc], t float64[Fc]) with out = (1-t)*rows[lo] + t*rows[hi].
    """
    v_pm_smpls = np.asarray(v_pm_smpls)
    step = fs * const_rate_ms / 1000
    centres = np.arange(step, v_pm_smpls[-1], step)
    if v_pm_smpls[0] > 0:
        x = np.r_[0, v_pm_smpls]
        node_row = np.r_[0, np.arange(v_pm_smpls.size)]
    else:
        x = v_pm_smpls
        node_row = np.arange(v_pm_smpls.size)
    idx = np.clip(np.searchsorted(x, centres), 1, x.size - 1)   # scipy interp1d's bracketing
    lo, hi = idx - 1, idx
    t = (centres - x[lo]) / (x[hi] - x[lo]).astype(np.float64)
    return node_row[lo].astype(np.int64), node_row[hi].astype(np.int64), t


def check_const_rate_ms(const_rate_ms):
    """A constant frame period in ms: finite and > 0 (ValueError otherwise)."""
    if isinstance(const_rate_ms, (bool, np.bool_)) or not isinstance(const_rate_ms, (int, float, np.integer, np.floating)):
        raise ValueError("const_rate_ms must be a number > 0, got %r" % (const_rate_ms,))
    v = float(const_rate_ms)
    if not np.isfinite(v) or v <= 0.0:
        raise ValueError("const_rate_ms must be finite and > 0, got %r" % (const_rate_ms,))
    return v


def _const_rate_f0_voi(v_f0, v_pm_smpls, fs, const_rate_ms=5.0):
    """magphase.py:2975-2980: f0 interpolated through the voiced points only, voicing by interpolation > 0.5."""
    from scipy import interpolate

    step = fs * const_rate_ms / 1000

    def interp1(y, x):
        centres = np.arange(step, x[-1], step)
        if x[0] > 0:
            f = interpolate.interp1d(np.r_[0, x], np.r_[y[0], y], axis=0, kind='linear')
        else:
            f = interpolate.interp1d(x, y, axis=0, kind='linear')
        return f(centres)

    v_voi = v_f0 > 1.0
    v_f0_c = interp1(np.r_[v_f0[v_voi][0], v_f0[v_voi], v_f0[v_voi][-1]], np.r_[0, v_pm_smpls[v_voi], v_pm_smpls[-1]])
    v_voi_c = interp1(v_voi.astype(np.float64), v_pm_smpls) > 0.5
    return v_f0_c * v_voi_c


def var_to_const_rate_batch(shift_list, f0_list, row_bases, fs, const_rate_ms):
    """
    Variable -> constant rate for a batch: per utterance the epochs cumsum(shifts), var_to_const_rate_table on them (rows
    offset by the utterance's base row) and _const_rate_f0_voi.  fs: one rate, or one per utterance.  Returns
    (row0, row1 int64, rowt float64: the batch's tables, concatenated; f0 per utterance at the constant rate; out_off
    int64[U + 1]: utterance u's constant-rate rows are out_off[u] .. out_off[u + 1]).
    """
    fs_list = fs if isinstance(fs, (list, tuple, np.ndarray)) else [fs] * len(shift_list)
    row0, row1, rowt, f0_out = [], [], [], []
    for v_shift, v_f0, base, fs_u in zip(shift_list, f0_list, row_bases, fs_list):
        v_pm = np.cumsum(v_shift)
        lo, hi, t = var_to_const_rate_table(v_pm, const_rate_ms, fs_u)
        f0_out.append(_const_rate_f0_voi(np.asarray(v_f0), v_pm, fs_u, const_rate_ms))
        row0.append(lo + int(base)), row1.append(hi + int(base)), rowt.append(t)
    cat = (lambda v, dt: np.concatenate(v).astype(dt) if v else np.zeros(0, dt))   # noqa: E731
    out_off = np.concatenate(([0], np.cumsum([f.size for f in f0_out]))).astype(np.int64)
    return cat(row0, np.int64), cat(row1, np.int64), cat(rowt, np.float64), f0_out, out_off


def const_to_variable_rows(v_voi_c, v_locs, const_rate_ms, fs):
    """Row tables of interp_from_const_to_variable_rate (magphase.py:2242-2252) from the grid's n rows to the frame
    locations v_locs, with scipy interp1d's bracketing.  v_voi_c: the voicing on the grid (bool[n]: f0 > 1.0 for type 1,
    magphase.py:847; f0 > 0.0 for type 2, :1511).  Returns (row_lo, row_hi int64, t float64, v_voi bool): the voicing at
    v_locs is interp(v_voi_c) > 0.5 (:866-868).  A grid of one row is what scipy makes of one point: the callers that take
    that row for every frame do so themselves (hostplan.plan_const_rate_synthesis)."""
    from scipy import interpolate

    if np.asarray(v_voi_c).dtype != np.bool_:
        raise TypeError("const_to_variable_rows: v_voi_c is the voicing mask on the grid (bool), not f0")
    n = int(np.size(v_voi_c))
    centres = (fs * const_rate_ms / 1000) * np.arange(1, n + 1)
    v_voi = interpolate.interp1d(centres, v_voi_c, axis=0, kind="linear")(v_locs) > 0.5
    idx = np.clip(np.searchsorted(centres, v_locs), 1, n - 1)   # scipy's _call_linear bracketing
    lo, hi = idx - 1, idx
    t = (v_locs - centres[lo]) / (centres[hi] - centres[lo])
    return lo.astype(np.int64), hi.astype(np.int64), t, v_voi


def lerp_adjoint_table(row0, row1, rowt, n_rows):
    """
    Frame ranges of the adjoint of out[f] = (1 - rowt[f]) rows[row0[f]] + rowt[f] rows[row1[f]] (mpx_rows_lerp_adjoint):
    int32 [n_rows x 4] = (a0, a1, b0, b1) per row r -- the frames with row0 == r are [a0, a1), those with row1 == r are
    [b0, b1).  Both tables must be non-decreasing (they are, within an utterance and across the utterances of a batch,
    whose rows follow one another), so each set is contiguous; a row no frame reads gets two empty ranges.  Pure index
    arithmetic: no torch, no GPU.
    """
    row0 = np.asarray(row0, dtype=np.int64).reshape(-1)
    row1 = np.asarray(row1, dtype=np.int64).reshape(-1)
    n_rows = int(n_rows)
    if row0.size != row1.size or np.size(rowt) != row0.size:
        raise ValueError("lerp_adjoint_table: row0, row1 and rowt must have one length")
    if n_rows < 0 or row0.size >= 2 ** 31:
        raise ValueError("lerp_adjoint_table: n_rows < 0 or too many frames")
    for name, r in (("row0", row0), ("row1", row1)):
        if r.size and (r.min() < 0 or r.max() >= n_rows):
            raise ValueError("lerp_adjoint_table: %s outside [0, %d)" % (name, n_rows))
        if np.any(np.diff(r) < 0):
            raise ValueError("lerp_adjoint_table: %s must be non-decreasing" % name)
    rows = np.arange(n_rows, dtype=np.int64)
    out = np.empty((n_rows, 4), dtype=np.int32)
    out[:, 0] = np.searchsorted(row0, rows, side="left")
    out[:, 1] = np.searchsorted(row0, rows, side="right")
    out[:, 2] = np.searchsorted(row1, rows, side="left")
    out[:, 3] = np.searchsorted(row1, rows, side="right")
    return out


def lossless_backward_table(pm_rel, frame_off, out_start, out_len, out_off, fft_len):
    """
    Where every frame of a lossless synthesis batch finds its gradient samples (mpx_synthesis_lossless_backward).  The
    forward is out_u[t] = sum_i frame_i[t + out_start[u] - pm_rel[i]] for 0 <= t < out_len[u] (ola_plan), so sample n of
    frame i receives the gradient of t = pm_rel[i] - out_start[u] + n when that lies in [0, out_len[u]) and nothing
    otherwise.  pm_rel: the frames' positions, concatenated (utterance u: frame_off[u] .. frame_off[u + 1]); out_off[u]:
    the utterance's offset in the gradient buffer.  Returns (pos int64[F] = index of sample 0 in the buffer -- may lie
    outside it --, lo, hi int32[F]: the samples lo <= n < hi are read).
    """
    pm_rel = np.asarray(pm_rel, dtype=np.int64).reshape(-1)
    frame_off = np.asarray(frame_off, dtype=np.int64)
    n_fr = np.diff(frame_off)
    if frame_off.size < 1 or int(frame_off[-1]) != pm_rel.size:
        raise ValueError("lossless_backward_table: frame_off does not cover pm_rel")
    rep = lambda v: np.repeat(np.asarray(v, dtype=np.int64)[:n_fr.size], n_fr)   # noqa: E731
    t0 = pm_rel - rep(out_start)
    lo = np.clip(-t0, 0, int(fft_len))
    hi = np.maximum(np.clip(rep(out_len) - t0, 0, int(fft_len)), lo)
    return rep(out_off) + t0, lo.astype(np.int32), hi.astype(np.int32)


def check_signal_tensor(t, name):
    """Argument check of a torch tensor given where the batch API takes a waveform: float32, float16, bfloat16 or
    float64, 1-D (any element stride).  Needs no device."""
    if str(t.dtype) not in ROWS_PACK_CODES:
        raise ValueError("%s: dtype %s is not supported (float32, float16, bfloat16 or float64)" % (name, t.dtype))
    if t.dim() != 1:
        raise ValueError("%s: must be 1-D, got %d-D" % (name, t.dim()))


def analysis_backward_table(pos, left, right, fft_len, total_smpls):
    """
    Where every frame of a lossless analysis batch puts its windowed gradient samples, and where the gather finds them
    (mpx_analysis_lossless_backward).  Frame f covers the samples start[f] = pos[f] - left[f] .. start[f] + n[f] - 1 of the
    batch's signal buffer, n[f] = min(left[f] + right[f] + 1, fft_len) (a longer frame is truncated by the forward); its
    n[f] gradient samples lie at scratch_off[f] in a compact scratch buffer of scratch_off[-1] floats.  The gather adds,
    per signal sample, the frames that cover it in ascending frame order: those are a contiguous index range when start
    and start + n are non-decreasing over the batch -- they are (within an utterance both ends of a frame are epochs or
    the utterance's ends, and the utterances follow one another in the buffer), and a table for which they are not is
    refused, as is a frame that leaves [0, total_smpls).  Returns (start int64[F], scratch_off int64[F + 1]).  Pure index
    arithmetic: no torch, no GPU.
    """
    pos = np.asarray(pos, dtype=np.int64).reshape(-1)
    left = np.asarray(left, dtype=np.int64).reshape(-1)
    right = np.asarray(right, dtype=np.int64).reshape(-1)
    N, total = int(fft_len), int(total_smpls)
    if not (pos.size == left.size == right.size):
        raise ValueError("analysis_backward_table: pos, left and right must have one length")
    if N < 1 or total < 0 or pos.size >= 2 ** 31:
        raise ValueError("analysis_backward_table: fft_len < 1, total_smpls < 0 or too many frames")
    if pos.size and (left.min() < 0 or right.min() < 0):
        raise ValueError("analysis_backward_table: negative left or right")
    n = np.minimum(left + right + 1, N)
    start = pos - left
    if pos.size and (start.min() < 0 or (start + n).max() > total):
        raise ValueError("analysis_backward_table: a frame leaves the signal buffer [0, %d)" % total)
    if np.any(np.diff(start) < 0) or np.any(np.diff(start + n) < 0):
        raise ValueError("analysis_backward_table: frame starts and ends must be non-decreasing")
    return start, np.concatenate(([0], np.cumsum(n))).astype(np.int64)


def _const_to_variable_scan_scipy(v_shift_c_rate, frm_rate_ms, fs):
    """The constant -> variable rate scan (magphase.py:1426-1449) written like the reference: one scipy interp1d call per
    step (8 us each).  hostplan._const_to_variable_scan is the native form the tests compare with this one."""
    from scipy import interpolate

    n = np.size(v_shift_c_rate, 0)
    step = fs * frm_rate_ms / 1000
    centres = step * np.arange(1, n + 1)
    f = interpolate.interp1d(centres, v_shift_c_rate, axis=0, kind="linear")
    shifts, locs = np.zeros(n * 2), np.zeros(n * 2)
    pos = centres[-1]
    for i in range(2 * n - 1, 0, -1):
        locs[i] = pos
        try:
            shifts[i] = f(pos)
        except ValueError:
            locs, shifts = locs[i + 1:], shifts[i + 1:]
            break
        pos = pos - shifts[i]
    return shifts, locs


def _first_all_zero_from(v):
    """Smallest n with v[k] == 0 for every k >= n."""
    nz = np.flatnonzero(np.asarray(v) != 0)
    return int(nz[-1]) + 1 if nz.size else 0


def synth_comp_phase_columns(fft_len, n_per_bins):
    """Leading columns of the real / imag rows that mpx_synthesis_compressed_ola (one row per frame) reads of a voiced
    frame when it is given n_per_bins (include/magphase_hip.h): the kernel loads phase in whole 64-bin groups -- below
    fft_len/4 the groups [64 q, 64 q + 63], above it the groups [fft_len/4 + 1 + 64 j, fft_len/4 + 64 + 64 j] (the mirror
    bins of a lane's pair) -- so for n_per_bins <= fft_len/4 + 1 this is n_per_bins rounded up to 64, beyond it
    fft_len/4 + 1 + (n_per_bins - fft_len/4 - 1 rounded up to 64), never more than fft_len/2 + 1.  What fills the rows for that
    entry must write this many columns."""
    H, Q = int(fft_len) // 2 + 1, int(fft_len) // 4
    n = H if (n_per_bins <= 0 or n_per_bins > H) else int(n_per_bins)
    if n <= Q + 1:
        return min((n + 63) // 64 * 64, H)
    return min(Q + 1 + (n - Q - 1 + 63) // 64 * 64, H)


def post_filter_tables(mag_dim, fs, av_len_at_zero=None, av_len_at_nyq=None, boost_at_zero=None, boost_at_nyq=None):
    """
    Host tables of the MagPhase post-filter (magphase.py:2300-2347, Q20): defaults per sample rate (same warnings /
    ValueError as the reference), bins with a moving average v_nx, their half lengths, and the tilt factors.
    Returns (nx_first, nx_last, half_len int64[], tilt float64[mag_dim]).
    """
    if mag_dim != 60:
        warnings.warn('Post-filter: It has been only tested with 60 dimensional mag data. '
                      'If you use another dimension, the result may be suboptimal.')
    opts = [av_len_at_zero, av_len_at_nyq, boost_at_zero, boost_at_nyq]
    if fs == 48000:
        defaults = [round_to_int(11.0 * (mag_dim / 60.0)), round_to_int(3.0 * (mag_dim / 60.0)), 1.8, 2.0]
    elif fs == 16000:
        if any(o is None for o in opts):
            warnings.warn('Post-filter: The default parameters for 16kHz sample rate have not being tunned.')
        defaults = [round_to_int(9.0 * (mag_dim / 60.0)), round_to_int(12.0 * (mag_dim / 60.0)), 2.0, 1.6]
    else:
        if any(o is None for o in opts):
            raise ValueError('Post-filter: It has only been tested with 16kHz and 48kHz sample rates.'
                             '\nProvide your own values for the options: av_len_at_zero, av_len_at_nyq, '
                             'boost_at_zero,\nboost_at_nyq if you use another sample rate')
        defaults = opts
    av0, avn, b0, bn = [d if o is None else o for o, d in zip(opts, defaults)]
    v_nx = np.arange(np.floor(av0 / 2), mag_dim - np.floor(avn / 2)).astype(int)
    v_lens = (2 * np.ceil(np.linspace(av0, avn, v_nx.size) / 2) - 1).astype(int)
    return int(v_nx[0]), int(v_nx[-1]), (v_lens // 2).astype(np.int64), np.linspace(b0, bn, mag_dim)


def post_filter_matrix(mag_dim, nx_first, nx_last, half_len, tilt):
    """
    The MagPhase post-filter as the [mag_dim x mag_dim] float64 matrix M it is per frame (y = x M^T), from
    post_filter_tables' output: M = diag(tilt) (I - A) + A with A the moving average of half length
    half_len[clamp(b, nx_first, nx_last) - nx_first] around the clamped bin, and the two end rows identity rows.
    """
    mag_dim, nx_first, nx_last = int(mag_dim), int(nx_first), int(nx_last)
    half_len = np.asarray(half_len, dtype=np.int64)
    tilt = np.asarray(tilt, dtype=np.float64)
    if not (0 <= nx_first <= nx_last < mag_dim) or half_len.size != nx_last - nx_first + 1 or tilt.size != mag_dim:
        raise ValueError("post_filter_matrix: tables do not fit mag_dim = %d" % mag_dim)
    centre = np.clip(np.arange(mag_dim), nx_first, nx_last)
    half = half_len[centre - nx_first]
    if np.any(half < 0) or np.any(centre - half < 0) or np.any(centre + half >= mag_dim):
        raise ValueError("post_filter_matrix: an averaging window leaves the row (half lengths %d .. %d)"
                         % (half.min(), half.max()))
    m_ave = np.zeros((mag_dim, mag_dim))
    for b in range(mag_dim):
        m_ave[b, centre[b] - half[b]:centre[b] + half[b] + 1] = 1.0 / (2 * half[b] + 1)
    m = tilt[:, None] * (np.eye(mag_dim) - m_ave) + m_ave
    m[0] = 0.0
    m[0, 0] = 1.0
    m[-1] = 0.0
    m[-1, -1] = 1.0
    return m


def post_filter_backward_tables(mag_dim, nx_first, nx_last, half_len, tilt):
    """
    Inverse tables of the MagPhase post-filter for mpx_post_filter_backward's gather (g_x = g_y M, column by column): per
    input bin i the output bins j with M[j][i] != 0 in ascending order and their weights M[j][i].
    Returns (cnt int32 [mag_dim], idx int32 [fan x mag_dim], w float64 [fan x mag_dim], fan); entry t of bin i is at
    [t][i], unused entries are (idx i, w 0).
    """
    m = post_filter_matrix(mag_dim, nx_first, nx_last, half_len, tilt)
    cover = [np.flatnonzero(m[:, i]) for i in range(int(mag_dim))]
    cnt = np.array([c.size for c in cover], dtype=np.int32)
    fan = max(1, int(cnt.max()))
    idx = np.tile(np.arange(int(mag_dim), dtype=np.int32), (fan, 1))
    w = np.zeros((fan, int(mag_dim)))
    for i, c in enumerate(cover):
        idx[:c.size, i] = c
        w[:c.size, i] = m[c, i]
    return cnt, idx, w, fan


HPF_DESIGNS = ("butter40", "ellip60")


def hpf_tables(fs, block, design="butter40"):
    """
    Output high-pass as two second-order sections (scipy output='sos') and, per section, the tables of the blocked scan
    of mpx_output_hpf: the direct-form-II-transposed state update z' = A z + Bx x with A = [[-a1, 1], [-a2, 0]],
    y = z0 + b0 x.  Returns (sos [2 x 6], A^block [2 x 4], G [2 x block x 2] with G[n] = [1, 0] A^n), float64.
    design: 'butter40' = Butterworth order 4 at 40 Hz (synthesis_from_compressed, magphase.py:981-995); 'ellip60' =
    elliptic order 4, 0.5 dB ripple, 80 dB stop band, 60 Hz (synthesis_from_compressed_type2, :1599-1604).  A^block and
    G depend on the sections' poles only; the zeros (on the unit circle for the elliptic design, at z = 1 for
    Butterworth) enter through b0, b1, b2 in the kernels' recurrence.
    """
    from scipy import signal

    if design == "butter40":
        sos = signal.butter(4, 40 / (fs / 2.0), btype='highpass', output='sos')
    elif design == "ellip60":
        sos = signal.ellip(4, 0.5, 80, 60 / (fs / 2.0), btype='highpass', output='sos')
    else:
        raise ValueError("hpf design must be one of %r, not %r" % (HPF_DESIGNS, design))
    sos = np.ascontiguousarray(sos, dtype=np.float64)
    pm = np.zeros((2, 4))
    g = np.zeros((2, block, 2))
    ld = np.longdouble
    for sec in range(2):
        # The powers of A are built in longdouble from the float64 a1, a2 the kernels use, and rounded once.  The poles of a
        # section are a close pair (angle 0.004 at 48 kHz), A is nearly defective and a rounding of a low power is amplified
        # ~1e5 times in A^256: np.linalg.matrix_power in float64 was 1.2e-9 off (1e-11 of the largest entry), which
        # was half of the blocked scan's whole error (tests/test_output_stage_host.py).
        a1, a2 = ld(sos[sec, 4] / sos[sec, 3]), ld(sos[sec, 5] / sos[sec, 3])
        amat = np.array([[-a1, ld(1)], [-a2, ld(0)]], dtype=ld)
        power = np.eye(2, dtype=ld)
        for n in range(block):
            g[sec, n] = power[0].astype(np.float64)
            power = power @ amat
        pm[sec] = power.reshape(-1).astype(np.float64)
    return sos, pm, g


# ======================================================================================================
# Merlin-style mel-cepstral post-filter (magphase.py:3375-3465)
# ======================================================================================================
def _f32(x):
    """One SPTK pipe boundary: every tool reads and writes float32, computes in double."""
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def rceps_compact(m_log):
    """
    la.rceps(in_type='log', out_type='compact') (libaudio.py:252-270): real cepstrum of the even extension of
    [F x n] log spectra (length 2(n-1)), first n coefficients, coefficients 1..n-3 doubled (the reference's slice
    1:(ncoeffs-2) leaves n-2 undoubled, Q6).
    """
    m_log = np.asarray(m_log, dtype=np.float64)
    n = m_log.shape[1]
    m_ext = np.hstack((m_log, m_log[:, -2:0:-1]))
    m_c = np.fft.ifft(m_ext).real
    m_c[:, 1:(n - 2)] *= 2
    return m_c[:, :n]


def sptk_mc2b(m_mc, alpha):
    """SPTK ``mc2b``: MLSA filter coefficients b[m] = mc[m] - alpha b[m+1], from the top coefficient down."""
    m_b = np.array(m_mc, dtype=np.float64)
    for m in range(m_b.shape[1] - 2, -1, -1):
        m_b[:, m] -= alpha * m_b[:, m + 1]
    return m_b


def sptk_b2mc(m_b, alpha):
    """SPTK ``b2mc`` (inverse of mc2b): mc[m] = b[m] + alpha b[m+1]."""
    m_mc = np.array(m_b, dtype=np.float64)
    m_mc[:, :-1] += alpha * np.asarray(m_b, dtype=np.float64)[:, 1:]
    return m_mc


_FREQT_CACHE = {}


def sptk_freqt(m_c, order_out, alpha_in, alpha_out=0.0):
    """SPTK ``freqt -m m1 -a alpha_in -M order_out -A alpha_out`` on [F x (m1+1)] cepstra, as one matrix product."""
    a = (alpha_out - alpha_in) / (1.0 - alpha_in * alpha_out)
    key = (m_c.shape[1], int(order_out), float(a))
    if key not in _FREQT_CACHE:
        _FREQT_CACHE[key] = freqt_matrix(m_c.shape[1], order_out, a).T.copy()   # [n_in x (order_out+1)]
    return np.asarray(m_c, dtype=np.float64) @ _FREQT_CACHE[key]


def sptk_c2acr_r0(m_c, fft_len):
    """SPTK ``c2acr -M 0 -l fft_len``: r[0] = mean over the fft_len bins of exp(2 Re FFT(c)) -- the frame energy."""
    m_x = np.zeros((m_c.shape[0], fft_len))
    m_x[:, :m_c.shape[1]] = m_c
    m_re = np.fft.fft(m_x, axis=1).real
    return np.exp(2.0 * m_re).sum(axis=1) / fft_len


def cos_matrix_log_spectrum(m_mcep, n_spbins):
    """la.mcep_to_sp_cosmat(alpha=0.0, out_type='log') (libaudio.py:605-631): out[k] = sum_n mc[n] cos(n pi k/(n_spbins-1))."""
    v_w = np.linspace(0, np.pi, num=n_spbins)
    m_trans = np.cos(np.outer(np.arange(m_mcep.shape[1]), v_w))
    return np.asarray(m_mcep, dtype=np.float64) @ m_trans


_MERLIN_CACHE = {}


def merlin_tables(dim, fs, pf_coef=1.4, fft_len=4096):
    """
    Constant tables of the device form of the Merlin post-filter (mpx_post_filter_merlin), float64:
      c1 [dim x dim]   rceps_compact as a matrix (mcep = x @ c1)
      lifter [dim]     (1, 1, pf, pf, ...) with pf printed with two decimals like the reference's command line
      g [dim x H]      freqt(alpha -> 0, order fft_len/2 - 1) followed by the real part of the fft_len-point DFT, on the
                       H = fft_len/2 + 1 distinct bins;  wk [H] = (1, 2, ..., 2, 1) / fft_len  (c2acr -M 0 -l fft_len)
      cf [dim x dim]   cosine matrix of cos_matrix_log_spectrum (alpha = 0);  alpha = define_alpha(fs)
    """
    key = (int(dim), int(fs), float("%1.2f" % pf_coef), int(fft_len))
    if key not in _MERLIN_CACHE:
        dim, alpha, half = key[0], define_alpha(fs), fft_len // 2
        c1 = rceps_compact(np.eye(dim))
        lifter = np.concatenate(([1.0, 1.0], np.full(dim - 2, key[2])))
        a = (0.0 - alpha) / (1.0 - alpha * 0.0)
        fq = freqt_matrix(dim, half - 1, a).T                     # [dim x half] cepstrum on the linear axis
        dcos = np.cos(2.0 * np.pi * np.outer(np.arange(half), np.arange(half + 1)) / fft_len)   # [half x H]
        wk = np.full(half + 1, 2.0 / fft_len)
        wk[0] = wk[-1] = 1.0 / fft_len
        cf = np.cos(np.outer(np.arange(dim), np.linspace(0, np.pi, num=dim)))
        _MERLIN_CACHE[key] = dict(c1=c1, lifter=lifter, g=fq @ dcos, wk=wk, cf=cf, alpha=alpha)
    return _MERLIN_CACHE[key]


# ======================================================================================================
# Griffin-Lim (magphase.py:3320-3372)
# ======================================================================================================
GL_FFT_LENS = (1024, 2048, 4096)


def griffin_lim_shifts(m_mag, v_shift):
    """
    Host checks of griffin_lim's inputs (magphase.py:3327-3330): returns (v_shift int64 rounded as lu.round_to_int, N).
    ValueError where the reference fails, or would fail at its first analysis (libaudio.py:122-140: np.zeros(N/2 - left)
    and np.zeros(N/2 - right - 1)), and where the port does not go (fft lengths without a kernel, no frames, negative
    shifts).  The right bound of the last frame is its own shift (ola's last shift repeated), of a lone frame its epoch.
    """
    m_mag = np.asarray(m_mag)
    if m_mag.ndim != 2:
        raise ValueError("griffin_lim: m_mag must be a 2-D [frames x bins] matrix")
    nfrms, H = m_mag.shape
    if nfrms == 0:
        raise ValueError("griffin_lim: no frames")
    N = 2 * (H - 1)
    if N not in GL_FFT_LENS:
        raise ValueError("griffin_lim: fft_len 2 (H - 1) = %d; supported: %s" % (N, GL_FFT_LENS))
    v = np.atleast_1d(np.asarray(v_shift, dtype=np.float64))
    if v.ndim != 1 or v.size != nfrms:
        raise ValueError("griffin_lim: len(v_shift) = %d != m_mag.shape[0] = %d" % (v.size, nfrms))
    if not np.all(np.isfinite(v)):
        raise ValueError("griffin_lim: v_shift must be finite")
    v = round_to_int(v).astype(np.int64)
    if np.any(v < 0):
        raise ValueError("griffin_lim: negative shifts")
    right = np.append(v[1:], v[-1])
    if v[0] > N // 2 or np.any(right > N // 2 - 1):
        raise ValueError("griffin_lim: shifts outside the reference's domain (v_shift[0] <= %d, v_shift[1:] <= %d and a "
                         "lone frame's shift <= %d: np.zeros of a negative length in frm_list_to_matrix)"
                         % (N // 2, N // 2 - 1, N // 2 - 1))
    return v, N


def griffin_lim_plan(shift_list, N):
    """
    Bookkeeping of a batch of Griffin-Lim utterances (integer shift vectors, one fft_len N): per utterance v_pm =
    cumsum(v_shift) (la.shift_to_pm), ola's (pm_rel, out_start, out_len) (ola_plan), the concatenated output offsets
    out_off, and the analysis tables of windowing(v_sig, v_pm) on the concatenated signal: frame_pos = out_off[u] + pm_f,
    frame_left / frame_right with the bounds [0, pm..., out_len - 1] (magphase.py:74-119).  In the reference's domain
    out_start = N/2 - pm_0 >= 0, so ola puts epoch pm_f at output index pm_f: the frame tables index straight into the
    previous iteration's output.
    """
    v_pm, pm_rel, starts, lens, pos, left, right, nfr = [], [], [], [], [], [], [], []
    for v in shift_list:
        pm = np.cumsum(np.asarray(v, dtype=np.int64))
        rel, start, out_len = ola_plan(pm, N)
        v_pm.append(pm), pm_rel.append(rel), starts.append(start), lens.append(out_len), nfr.append(pm.size)
    out_off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    for u, pm in enumerate(v_pm):
        p, lft, rgt = frame_bounds(pm, lens[u])
        pos.append(p + out_off[u]), left.append(lft), right.append(rgt)
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)   # noqa: E731
    return {"v_pm": v_pm, "pm_rel": pm_rel, "out_start": np.asarray(starts, dtype=np.int64),
            "out_len": np.asarray(lens, dtype=np.int64), "out_off": out_off,
            "frame_off": np.concatenate(([0], np.cumsum(nfr))).astype(np.int64),
            "frame_pos": cat(pos, np.int64), "frame_left": cat(left, np.int64), "frame_right": cat(right, np.int64)}


def griffin_lim_initial_phase(phase_init, m_mag, rng=np.random):
    """
    magphase.py:3334-3352: the initial phase of one utterance as the reference builds it, before its Hermitian extension.
    Returns (phase, full): full=True -> [F x N] (`'random'`: drawn from numpy's global generator, 'linear'), full=False ->
    [F x H] rows that the reference extends with la.add_hermitian_half(.., 'phase') -- columns 0 and H - 1 ZEROED IN PLACE
    (an ndarray init is the caller's array: the reference mutates it, and so does this).  'min_phase' returns None
    (computed on the device: mpx_min_phase).
    """
    F, H = np.shape(m_mag)
    N = 2 * (H - 1)
    if isinstance(phase_init, str):
        if phase_init == "random":
            return 2 * np.pi * (rng.rand(F, N) - 0.5), True
        if phase_init == "linear":
            row = np.zeros((1, N))
            row[:, N // 2] = 1.0
            return np.broadcast_to(np.angle(np.fft.fft(row)), (F, N)), True
        if phase_init == "min_phase":
            return None, False
    phase_init[:, 0] = 0
    phase_init[:, -1] = 0
    return phase_init, False


def griffin_lim_fold(m_mag, phase, full):
    """
    The first synthesis of griffin_lim, frames = ifft(M e^{j phi}).real with phi not necessarily Hermitian, restated as
    the existing lossless synthesis fftshift(ifft(hermitian(mag' . phasor))) (mpx_synthesis_lossless_ola): .real of the
    iFFT is the iFFT of H_k = M_k (e^{j phi_k} + e^{-j phi_{N-k}}) / 2 (H_0 = M_0 cos phi_0, H_{N/2} = M_{N/2} cos phi_{N/2}),
    H = M c; with mag' = M |c| and phasor c (-1)^k / |c| (|c| = 0: mag' = 0, phasor 0) the fftshift's (-1)^k cancels.
    full=False: phase is [F x H] of a Hermitian extension with phi_0 = phi_{N/2} = 0 (c = e^{j phi}).
    Returns float64 (mag', phasor real, phasor imag), each [F x H].
    """
    m_mag = np.asarray(m_mag, dtype=np.float64)
    F, H = m_mag.shape
    N = 2 * (H - 1)
    sgn = np.where(np.arange(H) % 2 == 0, 1.0, -1.0)
    if full:
        ph = np.asarray(phase, dtype=np.float64)
        mir = ph[:, (N - np.arange(H)) % N]   # phi_{N-k} for k = 0..N/2
        cr = 0.5 * (np.cos(ph[:, :H]) + np.cos(mir))
        ci = 0.5 * (np.sin(ph[:, :H]) - np.sin(mir))
        cr[:, 0], ci[:, 0] = np.cos(ph[:, 0]), 0.0
        cr[:, -1], ci[:, -1] = np.cos(ph[:, N // 2]), 0.0
        a = np.hypot(cr, ci)
        nz = a > 0
        inv = np.where(nz, 1.0 / np.where(nz, a, 1.0), 0.0)
        return m_mag * a, cr * inv * sgn, ci * inv * sgn
    ph = np.array(phase, dtype=np.float64)
    ph[:, 0] = 0.0
    ph[:, -1] = 0.0
    return m_mag.copy(), np.cos(ph) * sgn, np.sin(ph) * sgn


TRUE_ENV_IN_TYPES = ("abs", "db", "log")   # in_type of la.true_envelope, in the order of mpx_true_envelope's codes
TRUE_ENV_MAX_ITERS = 100                   # la.true_envelope's n_maxiter (libaudio.py:310)


def true_envelope_lifter(N, ncoeffs, fade=0.7):
    """
    The weight w[n], n < N, by which la.spectral_smoothing_rceps (libaudio.py:203-238) multiplies the real cepstrum of
    its N-point even extension: rceps_to_min_phase_rceps doubles c[1 : N/2], then c[ncoeffs:] = 0 and
    c[ncoeffs - nf : ncoeffs] *= hanning(2 nf + 3)[nf + 2 : -1], nf = round(fade * ncoeffs) (numpy's half-to-even).
    float64; ncoeffs = 0 gives all zeros.  ncoeffs above N/2 keeps part of the anticausal half, undoubled.
    """
    N, ncoeffs = int(N), int(ncoeffs)
    if ncoeffs < 0 or ncoeffs > N:
        raise ValueError("ncoeffs must be in 0..%d (the FFT length), got %d" % (N, ncoeffs))
    fade = float(fade)
    if not 0.0 <= fade <= 1.0:
        raise ValueError("fade_to_total must be in [0, 1], got %r" % (fade,))
    nf = int(np.round(fade * ncoeffs))
    w = np.ones(N)
    w[1:N // 2] = 2.0
    w[ncoeffs:] = 0.0
    w[ncoeffs - nf:ncoeffs] *= np.hanning(2 * nf + 3)[nf + 2:-1]
    return w


def true_envelope_check(H, in_type, ncoeffs):
    """Argument checks of la.true_envelope / spectral_smoothing_rceps on [F x H] rows -> fft_len N = 2 (H - 1)."""
    if in_type not in TRUE_ENV_IN_TYPES:
        raise ValueError("in_type must be 'abs', 'db' or 'log', got %r" % (in_type,))
    if int(H) - 1 not in (512, 1024, 2048):
        raise ValueError("spectra must have 513, 1025 or 2049 bins (fft_len 1024 / 2048 / 4096), got %d" % int(H))
    N = 2 * (int(H) - 1)
    if int(ncoeffs) != ncoeffs or not 0 <= int(ncoeffs) <= N:
        raise ValueError("ncoeffs must be an integer in 0..%d (the FFT length), got %r" % (N, ncoeffs))
    return N


# ---------------------------------------------------------------------------------------------
# MLPG: argument checks of the public functions, all before any device call
# ---------------------------------------------------------------------------------------------
def mlpg_windows(windows):
    """The dynamic windows of MLPG as a float64 [n_win x 3] array of taps (w[-1], w[0], w[+1]); n_win is 1 or 2."""
    try:
        w = np.array([[float(v) for v in row] for row in windows], dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("windows: one or two windows of three taps (w[-1], w[0], w[+1]) expected, got %r" % (windows,))
    if w.ndim != 2 or w.shape[0] not in (1, 2) or w.shape[1] != 3:
        raise ValueError("windows: one or two windows of three taps (w[-1], w[0], w[+1]) expected, got %r" % (windows,))
    if not np.all(np.isfinite(w)):
        raise ValueError("windows: every tap must be finite")
    return w


def _mlpg_matrix(m, name, width=None):
    """One [F x width] operand of MLPG: a numpy array (any real dtype: float64 unless float32), or a torch tensor (float32 /
    float64; a CPU tensor becomes a host array, a non-unit column stride is made contiguous)."""
    import sys

    torch = sys.modules.get("torch")
    if torch is not None and torch.is_tensor(m):
        if m.dtype not in (torch.float32, torch.float64):
            raise ValueError("%s: dtype %s is not supported (float32 or float64)" % (name, m.dtype))
        if m.dim() != 2:
            raise ValueError("%s: must be 2-D [frames x width], got %d-D" % (name, m.dim()))
        if m.device.type == "cpu":
            m = m.detach().numpy()
        elif m.shape[1] > 1 and m.stride(1) != 1:
            m = m.contiguous()
    else:
        m = np.asarray(m)
        if m.dtype.kind not in "fiu":
            raise ValueError("%s: a real matrix expected, got dtype %s" % (name, m.dtype))
        if m.dtype != np.float32:
            m = m.astype(np.float64, copy=False)
        if m.ndim != 2:
            raise ValueError("%s: must be 2-D [frames x width], got %d-D" % (name, m.ndim))
    if width is not None and int(m.shape[1]) != width:
        raise ValueError("%s: %d columns expected, got %d" % (name, width, int(m.shape[1])))
    return m


def _mlpg_host_var_ok(v, name, cols=None):
    if isinstance(v, np.ndarray):
        x = v if cols is None else v[..., cols]
        if not (np.all(np.isfinite(x)) and np.all(x > 0)):
            raise ValueError("%s: every variance must be finite and > 0" % name)


def mlpg_check(means, var, windows, what="mlpg_batch", width_of=None, var_cols=None):
    """Checks of mlpg_batch / mlpg_streams_batch.  means: list of [F_i x width] matrices; var: one [width] vector or a
    list of [F_i x width] matrices; width_of(width, K): checks the width and is what is returned as D (default: width / K).
    Variances held in host arrays must be finite and > 0 (var_cols: in these columns only); those of device tensors are
    NOT inspected.  -> (means, var, windows [n_win x 3], D, per_frame)."""
    import sys

    w = mlpg_windows(windows)
    K = w.shape[0] + 1
    if isinstance(means, np.ndarray) or not isinstance(means, (list, tuple)):
        raise ValueError("%s: means must be a list of [frames x width] matrices" % what)
    means = [_mlpg_matrix(m, "%s: means[%d]" % (what, i)) for i, m in enumerate(means)]
    torch = sys.modules.get("torch")
    is_t = torch is not None and torch.is_tensor(var)
    per_frame = isinstance(var, (list, tuple)) and not (len(var) > 0 and np.isscalar(var[0]))
    if not means:
        return means, var, w, 0, per_frame
    width = int(means[0].shape[1])
    if any(int(m.shape[1]) != width for m in means):
        raise ValueError("%s: every mean matrix must have the same number of columns" % what)
    if width_of is None:
        if width < K or width % K:
            raise ValueError("%s: %d columns are not [static | delta | acc] blocks of %d streams" % (what, width, K))
        D = width // K
    else:
        D = width_of(width, K)
    if per_frame:
        if len(var) != len(means):
            raise ValueError("%s: var must be one vector or one matrix per utterance (%d given for %d utterances)"
                             % (what, len(var), len(means)))
        var = [_mlpg_matrix(v, "%s: var[%d]" % (what, i), width) for i, v in enumerate(var)]
        for i, (v, m) in enumerate(zip(var, means)):
            if int(v.shape[0]) != int(m.shape[0]):
                raise ValueError("%s: var[%d] has %d rows, means[%d] has %d" % (what, i, v.shape[0], i, m.shape[0]))
            _mlpg_host_var_ok(v, "%s: var[%d]" % (what, i), var_cols)
    else:
        if is_t:
            if var.dtype not in (torch.float32, torch.float64) or var.dim() != 1 or int(var.numel()) != width:
                raise ValueError("%s: var must be a float32 / float64 vector of %d values" % (what, width))
            var = var.detach().numpy() if var.device.type == "cpu" else var.detach().contiguous()
        else:
            var = np.asarray(var)
            if var.dtype.kind not in "fiu" or var.ndim != 1 or var.shape[0] != width:
                raise ValueError("%s: var must be a vector of %d values (or a list of matrices)" % (what, width))
            if var.dtype != np.float32:
                var = var.astype(np.float64, copy=False)
        _mlpg_host_var_ok(var, "%s: var" % what, var_cols)
    return means, var, w, D, per_frame


def mlpg_var_inputs(var_given, var, per_frame):
    """The variance tensors a gradient can reach, for var_grad=True and for the trajectory likelihood: var_given = what
    the caller passed, var = what mlpg_check made of it.  Per-frame: the checked matrices (still attached to the caller's
    tensors); global: the caller's own vector.  -> the list, or None when one of them is a host array or a CPU tensor."""
    import sys

    torch = sys.modules.get("torch")
    if torch is None:
        return None
    cand = list(var) if per_frame else [var_given]
    if not cand or not all(torch.is_tensor(v) and v.device.type != "cpu" for v in cand):
        return None
    return cand


def mlpg_var_grad_check(var_grad, return_device, var_given, var, per_frame, what):
    """var_grad of mlpg_batch / mlpg_streams_batch -> the variance tensors to differentiate ([] without var_grad).
    var_grad=True needs return_device and variances in device tensors (ValueError)."""
    if not var_grad:
        return []
    if not return_device:
        raise ValueError("%s: var_grad=True needs return_device=True (a host result carries no gradient)" % what)
    cand = mlpg_var_inputs(var_given, var, per_frame)
    if cand is None:
        raise ValueError("%s: var_grad=True needs the variances in device tensors, not host arrays" % what)
    return cand


def mlpg_targets_check(targets, means, D, what="mlpg_trajectory_nll_batch"):
    """The static targets of the trajectory likelihood: one [F_i x D] matrix per utterance (as the means: numpy or torch,
    float32 / float64).  Host targets must be finite."""
    if isinstance(targets, np.ndarray) or not isinstance(targets, (list, tuple)):
        raise ValueError("%s: targets must be a list of [frames x D] matrices" % what)
    if len(targets) != len(means):
        raise ValueError("%s: one target matrix per utterance expected (%d given for %d utterances)"
                         % (what, len(targets), len(means)))
    out = [_mlpg_matrix(x, "%s: targets[%d]" % (what, i), D) for i, x in enumerate(targets)]
    for i, (x, m) in enumerate(zip(out, means)):
        if int(x.shape[0]) != int(m.shape[0]):
            raise ValueError("%s: targets[%d] has %d rows, means[%d] has %d" % (what, i, x.shape[0], i, m.shape[0]))
        if isinstance(x, np.ndarray) and not np.all(np.isfinite(x)):
            raise ValueError("%s: targets[%d]: every value must be finite" % (what, i))
    return out


def mlpg_layout(layout, vuv, K, what="mlpg_streams_batch"):
    """The streams of mlpg_streams_batch: layout = ((name, dim), ...), stream s in K dim_s columns [static | delta | acc]
    one after the other, then one voicing column when vuv.  -> (layout as ((str, int), ...), [(first column, dim), ...],
    the number of columns it asks for)."""
    try:
        layout = tuple((str(n), int(d)) for n, d in layout)
    except (TypeError, ValueError):
        raise ValueError("%s: layout must be ((name, dim), ...), got %r" % (what, layout))
    if not layout or any(d < 1 for _, d in layout):
        raise ValueError("%s: layout needs at least one stream and every dim >= 1" % what)
    if len(set(n for n, _ in layout)) != len(layout):
        raise ValueError("%s: stream names must differ" % what)
    if any(n == "lf0" and d != 1 for n, d in layout) or (vuv and not any(n == "lf0" for n, _ in layout)):
        raise ValueError("%s: the stream 'lf0' has dim 1, and vuv needs it in the layout" % what)
    streams, c = [], 0
    for _, d in layout:
        streams.append((c, d))
        c += K * d
    return layout, streams, c + (1 if vuv else 0)


# ---------------------------------------------------------------------------------------------
# Acoustic composition: argument checks of the public functions, all before any device call
# ---------------------------------------------------------------------------------------------
CMP_MAX_STREAMS = 16     # the layout travels to the kernels by value (magphase_cmp.hip: CmpLayout)
_VOI_OPS = {">": np.greater, ">=": np.greater_equal, "<": np.less, "<=": np.less_equal, "==": np.equal,
            "!=": np.not_equal}


def cmp_voi_cond(voi_cond):
    """la.interp_unv_regions' voi_cond, '<op><number>' (the reference evaluates 'v_voi ' + voi_cond) -> (numpy
    comparison, number).  No eval."""
    import re

    m = re.fullmatch(r"\s*(>=|<=|==|!=|>|<)\s*([-+]?(?:\d+\.?\d*|\.\d+)(?:[eE][-+]?\d+)?)\s*", str(voi_cond))
    if m is None:
        raise ValueError("voi_cond: '<op><number>' expected (op one of > >= < <= == !=), got %r" % (voi_cond,))
    return _VOI_OPS[m.group(1)], float(m.group(2))


def cmp_operand(m, name, dim, lf0=False):
    """One stream of one utterance as acoustic_compose_batch takes it -> a 2-D [F x dim] host array (float32 / float64) or
    device tensor (float16 / bfloat16 / float32 / float64, unit column stride).  A vector is a [F x 1] matrix.  TypeError:
    not a float dtype; ValueError: shape, width, a float16 lf0 (check_feature_tensor's rule)."""
    import sys

    torch = sys.modules.get("torch")
    if torch is not None and torch.is_tensor(m):
        if not m.dtype.is_floating_point:
            raise TypeError("%s: dtype %s is not a float dtype" % (name, m.dtype))
        if m.dim() == 1 and dim == 1:
            m = m.unsqueeze(1)
        check_feature_tensor(m, name)
        if lf0 and m.dtype == torch.float16:
            raise ValueError("%s: a float16 lf0 cannot hold the unvoiced marker -1e10 (float32, bfloat16 or float64)" % name)
        if m.device.type == "cpu":
            m = m.detach()
            m = (m.float() if m.dtype in (torch.float16, torch.bfloat16) else m).numpy()
        elif m.shape[1] > 1 and m.stride(1) != 1:
            m = m.contiguous()
    else:
        m = np.asarray(m)
        if m.dtype.kind != "f":
            raise TypeError("%s: dtype %s is not a float dtype" % (name, m.dtype))
        if lf0 and m.dtype == np.float16:
            raise ValueError("%s: a float16 lf0 cannot hold the unvoiced marker -1e10 (float32 or float64)" % name)
        if m.dtype != np.float32:
            m = m.astype(np.float64, copy=False)
        if m.ndim == 1 and dim == 1:
            m = m.reshape(-1, 1)
        if m.ndim != 2:
            raise ValueError("%s: must be 2-D [frames x %d], got %d-D" % (name, dim, m.ndim))
    if int(m.shape[1]) != dim:
        raise ValueError("%s: %d columns expected, got %d" % (name, dim, int(m.shape[1])))
    return m


def cmp_check(feats, layout, vuv, windows, unv_fill, what="acoustic_compose_batch"):
    """Checks of acoustic_compose_batch.  feats: list of per-utterance tuples in layout order.  -> (layout, streams
    [(first output column, dim)], W, windows [n_win x 3], feats as lists of 2-D operands, index of the 'lf0' stream or
    -1).  The column map is mlpg_layout's."""
    w = mlpg_windows(windows)
    layout, streams, W = mlpg_layout(layout, vuv, w.shape[0] + 1, what)
    if len(layout) > CMP_MAX_STREAMS:
        raise ValueError("%s: at most %d streams" % (what, CMP_MAX_STREAMS))
    if isinstance(unv_fill, bool) or not isinstance(unv_fill, (int, float)) or not np.isfinite(unv_fill):
        raise ValueError("%s: unv_fill must be a finite number" % what)
    if isinstance(feats, np.ndarray) or not isinstance(feats, (list, tuple)):
        raise ValueError("%s: feats must be a list of per-utterance tuples %s" % (what, tuple(n for n, _ in layout)))
    out = []
    for u, f in enumerate(feats):
        if isinstance(f, np.ndarray) or not isinstance(f, (list, tuple)) or len(f) != len(layout):
            raise ValueError("%s: feats[%d] must be a tuple of %d streams %s"
                             % (what, u, len(layout), tuple(n for n, _ in layout)))
        ops = [cmp_operand(m, "%s: feats[%d] (%s)" % (what, u, n), d, lf0=(n == "lf0"))
               for m, (n, d) in zip(f, layout)]
        if any(int(m.shape[0]) != int(ops[0].shape[0]) for m in ops):
            raise ValueError("%s: feats[%d]: the streams have %s frames" % (what, u, [int(m.shape[0]) for m in ops]))
        out.append(ops)
    interp = next((i for i, (n, d) in enumerate(layout) if n == "lf0" and d == 1), -1)
    return layout, streams, W, w, out, interp


def cmp_norm(norm, W, what="acoustic_compose_batch"):
    """norm=(mean, std): two [W] vectors (host arrays -> float64 arrays; device tensors stay, as float64).  std must be
    finite and > 0, mean finite (ValueError)."""
    import sys

    if norm is None:
        return None
    if isinstance(norm, np.ndarray) or not isinstance(norm, (list, tuple)) or len(norm) != 2:
        raise ValueError("%s: norm must be (mean, std)" % what)
    torch = sys.modules.get("torch")
    out = []
    for name, v in zip(("mean", "std"), norm):
        if torch is not None and torch.is_tensor(v):
            if not v.dtype.is_floating_point:
                raise TypeError("%s: norm %s: dtype %s is not a float dtype" % (what, name, v.dtype))
            v = v.detach().double()
            if v.device.type == "cpu":
                v = v.numpy()
        else:
            v = np.asarray(v)
            if v.dtype.kind not in "fiu":
                raise TypeError("%s: norm %s: dtype %s is not a real dtype" % (what, name, v.dtype))
            v = v.astype(np.float64)
        if len(v.shape) != 1 or int(v.shape[0]) != W:
            raise ValueError("%s: norm %s must be a vector of %d values" % (what, name, W))
        if isinstance(v, np.ndarray):
            ok = np.all(np.isfinite(v)) and (name == "mean" or np.all(v > 0))
        else:
            ok = bool(torch.isfinite(v).all()) and (name == "mean" or bool((v > 0).all()))
        if not ok:
            raise ValueError("%s: norm %s must be finite%s" % (what, name, "" if name == "mean" else " and > 0"))
        out.append(v)
    return tuple(out)
