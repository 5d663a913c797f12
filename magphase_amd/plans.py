"""
Batch plans: host float64 index arithmetic (hostmath / hostplan) -> descriptor tensors resident in HBM -> run(), the
launch sequence of one batch.  A plan talks to the Engine object it is handed (uploads, allocations, Engine.launch) and
imports nothing from engine.py; LosslessAnalysisPlan and LosslessSynthesisPlan build on any object that offers
to_device / to_device_packed (the hasattr guards are for that).
"""
import ctypes
import os

import numpy as np

from . import _lib, hostmath as hm, hostplan


def _torch():
    import torch

    return torch


def _is_tensor(x):
    """torch.is_tensor without importing torch for what cannot be one (a tensor's class lives in the torch package)."""
    return type(x).__module__.startswith("torch") and _torch().is_tensor(x)


def _rows_or_array(engine, x, name):
    """One coefficient matrix of a synthesis batch that is not a plain 2-D ndarray: a tensor on the engine's device stays
    what it is (checked: a float type, 2-D; a non-unit column stride made contiguous), a CPU tensor becomes a host array
    (float16 / bfloat16 widened to float32: exact), a tensor elsewhere is an error; anything else goes through numpy."""
    if not _is_tensor(x):
        return np.atleast_2d(np.asarray(x))
    hm.check_feature_tensor(x, name)
    if x.device.type == "cpu":
        x = x.detach()
        return (x.float() if x.element_size() == 2 else x).numpy()
    if not (hasattr(engine, "is_device_rows") and engine.is_device_rows(x)):
        raise ValueError("%s is on %s, the engine runs on %s" % (name, x.device, getattr(engine, "device", None)))
    x = x.detach()
    return x if x.shape[1] <= 1 or x.stride(1) == 1 else x.contiguous()


def _signal_inputs(engine, utts):
    """torch tensors among the v_sig of an analysis batch utts = [(v_sig, fs, v_pm_sec, v_voi), ...]: checked (float32 /
    float16 / bfloat16 / float64, 1-D: ValueError naming the utterance otherwise); a CPU tensor becomes a host array
    (float16 / bfloat16 widened to float32: exact), a tensor on the engine's device stays, a tensor elsewhere is an error.
    Returns (utts, True when a device tensor remains); a batch without tensors comes back as it is."""
    if not any(_is_tensor(u[0]) for u in utts):
        return utts, False
    out, on_dev = [], False
    for i, u in enumerate(utts):
        x = u[0]
        if _is_tensor(x):
            name = "utts[%d]: v_sig" % i
            hm.check_signal_tensor(x, name)
            if x.device.type == "cpu":
                x = x.detach()
                x = (x.float() if x.element_size() == 2 else x).numpy()
            elif x.device != getattr(engine, "device", None):
                raise ValueError("%s is on %s, the engine runs on %s" % (name, x.device, getattr(engine, "device", None)))
            else:
                on_dev = True
        out.append((x,) + tuple(u[1:]))
    return out, on_dev


TYPE2_ENV_NCOEFFS = 600   # la.true_envelope(..., ncoeffs=600, thres_db=0.1) of analysis_lossless_type2 (magphase.py:2829)
TYPE2_ENV_THRES_DB = 0.1


class _FlatRows:
    """A list of per-utterance rows kept as ONE array + offsets; iterating / indexing cuts the views."""

    def __init__(self, flat, off):
        self.flat, self.off = flat, np.asarray(off, dtype=np.int64)
        self._o = self.off.tolist()

    def __len__(self):
        return len(self._o) - 1

    def __getitem__(self, u):
        if u < 0:
            u += len(self._o) - 1
        return self.flat[self._o[u]:self._o[u + 1]]

    def __iter__(self):
        return (self[u] for u in range(len(self)))


def _plan_ola_runs(plan, pm_rel_list, starts, out_lens, out_off_host, fft_len, n_slots, frames_per_run, up, weights=None,
                   gcuts=None, extents=None):
    """Shared by the two synthesis plans: runs + slot work lists (hostmath.ola_runs / balance_chunks) -> upload list.
    weights: the slots' relative speeds (Engine.synth_ola_slot_weights) or None for equal shares; gcuts: the caller's own
    cuts of the frame sequence instead of shares by count (hostmath.ola_runs; ignored with frames_per_run).
    extents: what each frame of ONE kernel can add to the ring (hostmath.ola_runs), or None.  The plan's own run table
    (plan.runs / plan.runs_host) is always the one for dense frames, which every overlap-add kernel may use; with extents a
    second table of the same runs, its seams sized by them, is planned beside it (plan.seam_runs / plan.seam_runs_host,
    plan.seam_fix_width = its widest fix range) for that kernel alone -- _SeamRuns."""
    fpr = frames_per_run or int(os.environ.get("MAGPHASE_OLA_FRAMES_PER_RUN", 0)) or None

    def plan_runs(ext):
        try:
            if fpr:
                raise hostplan.PlanFallback()      # per-utterance run lengths (tests, tuning): the numpy planner only
            if isinstance(pm_rel_list, _FlatRows):   # already one array + offsets (CompressedSynthesisPlan)
                rel_cat, f_off = np.asarray(pm_rel_list.flat, dtype=np.int64), pm_rel_list.off
                sizes = np.diff(f_off)
            else:
                sizes = [int(np.size(r)) for r in pm_rel_list]
                rel_cat = np.concatenate([np.asarray(r, dtype=np.int64) for r in pm_rel_list]) if pm_rel_list else np.zeros(0, np.int64)
                f_off = np.concatenate(([0], np.cumsum(sizes)))
            return hostplan.ola_runs(rel_cat, f_off, starts, out_lens, np.asarray(out_off_host)[:len(sizes)], fft_len,
                                     n_slots, weights=weights, gcuts=gcuts, extents=ext)
        except hostplan.PlanFallback:
            return hm.ola_runs(pm_rel_list, starts, out_lens, out_off_host, fft_len, n_slots, frames_per_run=fpr,
                               weights=None if fpr else weights, gcuts=None if fpr else gcuts, extents=ext)

    runs, slot_off, slot_runs = plan_runs(None)
    plan.n_runs = int(runs.size)
    plan.runs_host = runs
    plan.strip_floats = plan.n_runs * (int(fft_len) + 64)
    plan.n_slots = int(slot_off.size - 1)
    up.append(("runs", runs.view(np.uint8), np.uint8))
    up.append(("slot_off", slot_off, np.int32))
    up.append(("slot_runs", slot_runs, np.int32))
    if extents is not None:
        seam, s_off, s_runs = plan_runs(extents)
        # the same frames in the same runs on the same slots: the seam fields alone differ
        if not (np.array_equal(seam["frame_begin"], runs["frame_begin"]) and np.array_equal(seam["frame_end"], runs["frame_end"])
                and np.array_equal(seam["strip_off"], runs["strip_off"]) and np.array_equal(s_off, slot_off)
                and np.array_equal(s_runs, slot_runs)):
            raise ValueError("run planning with extents must keep the runs of the dense plan")
        # as k_ola_fixup walks a range: from the 64-element block fix_lo lies in to fix_hi (runs with nothing to fix: 0)
        width = np.where(seam["fix_hi"] > seam["fix_lo"], seam["fix_hi"] - (seam["fix_lo"] & ~63), 0)
        plan.seam_runs_host = seam
        plan.seam_fix_width = int(width.max()) if width.size else 0
        up.append(("seam_runs", seam.view(np.uint8), np.uint8))


class _SeamRuns:
    """A synthesis plan seen through its second run table (_plan_ola_runs with extents): what the launch of the one kernel
    whose frames have those extents and the fix-up after it read -- the same runs, slots, positions and strips as the plan's
    own, dense table, the seam fields sized by the extents, and the widest fix range for Engine.ola_fixup."""

    def __init__(self, plan):
        self.runs, self.runs_host, self.fix_width = plan.seam_runs, plan.seam_runs_host, plan.seam_fix_width
        self.n_runs, self.n_slots, self.strip_floats = plan.n_runs, plan.n_slots, plan.strip_floats
        self.slot_off, self.slot_runs, self.pm_rel = plan.slot_off, plan.slot_runs, plan.pm_rel
        # mpx_ola_fixup_width leaves a range wider than the width it is given uncompleted and cannot see the table: the
        # width must cover every range as k_ola_fixup walks it
        r = self.runs_host
        assert not r.size or self.fix_width >= int(np.max(np.where(r["fix_hi"] > r["fix_lo"],
                                                                   r["fix_hi"] - (r["fix_lo"] & ~63), 0)))


def _run_ola(engine, entry, fft_len, runs, strips, out, total_out):
    """What every fused overlap-add run does: strips / out allocated when the caller brought none, entry(strips, out)
    launches the pair kernel over `runs` (a plan with run tables: every output sample written once, and the runs' head
    strips), ola_fixup completes the run boundaries.  Returns out."""
    if strips is None:
        strips = engine.empty((max(runs.strip_floats, 1),))
    if out is None:
        out = engine.empty((total_out,))
    entry(strips, out)
    return engine.ola_fixup(fft_len, runs, strips, out)


def _upload_rows(engine, rows, head=(), tail=()):
    """ONE packed upload of the row tables rows = (row0, row1, rowt) host arrays (-> int32, int32, float32) with the items
    `head` in front of and `tail` behind them in the same copy.  Returns ((row0, row1, rowt) device, {name: tensor} of
    the other items)."""
    d = engine.to_device_packed(list(head) + [("row0", rows[0], np.int32), ("row1", rows[1], np.int32),
                                              ("rowt", rows[2], np.float32)] + list(tail))
    return (d.pop("row0"), d.pop("row1"), d.pop("rowt")), d


def _check_prepared(prepared, engine, utts):
    """A Prepared* handed to a plan constructor must be the host side of these utterances on this engine."""
    if prepared.n_utts != len(utts) or prepared.engine is not engine:
        prepared.release()
        raise ValueError("prepared: not the host side of this batch on this engine")


def _wait_ready(plan):
    """A plan may be run on another stream than the one it was built on (bench.py alternates streams): that stream
    waits for the plan's uploads too (the build stream already does)."""
    ev = getattr(plan, "_ready", None)
    if ev is not None:
        _torch().cuda.current_stream(plan.engine.device).wait_event(ev)


def _widen_pcm16(engine, raw, total):
    """16-bit samples on the device (two per float32 of `raw`, or bytes) -> float32 [total] (mpx_pcm16_to_f32)."""
    sig = engine.empty((max(total, 1),))
    engine.launch("mpx_pcm16_to_f32", raw, total, sig)
    return sig[:total]


# ======================================================================================================
# lossless features
# ======================================================================================================
class LosslessAnalysisPlan:
    """
    Frame descriptors of a batch of utterances for mpx_analysis_frames.
    utts: list of (v_sig float array in [-1,1) or int16 PCM, fs, v_pm_sec, v_voi).  All must share fft_len.
    Host math follows magphase.py:2877-2879 (pm_sec*fs), libaudio.py:435-447, magphase.py:77-98, :2198-2199.
    """

    def __init__(self, engine, utts, fft_len=None, prepared=None, keep_frame_tabs=False):
        # prepared: a PreparedAnalysis of these utterances (Engine.prepare_analysis, e.g. from the planner thread); None:
        # prepared here when the batch is in the plain shape the native path takes, else the generic path below
        # keep_frame_tabs: keep a host copy of the frame tables (pos, left, right) in self._host_tabs (LosslessRoundTripPlan
        # deals its frames by them)
        self.engine = engine
        self._keep_tabs = bool(keep_frame_tabs)
        utts, on_dev = _signal_inputs(engine, utts)
        if on_dev:      # some v_sig is a tensor on the engine's device: the samples never visit the host
            if prepared is not None:
                prepared.release()
                raise ValueError("prepared= was built from host arrays: it cannot be combined with tensor inputs")
            self._from_device(engine, utts, fft_len)
            return
        if prepared is None and hasattr(engine, "prepare_analysis") and os.environ.get("MAGPHASE_NATIVE_PREPARE", "1") != "0":
            prepared = engine.prepare_analysis(utts, fft_len, wait=False)
        if prepared is not None:
            self._from_prepared(prepared, utts)
            return
        pos, left, right = [], [], []
        self.v_shift, self.v_f0, self.fs, self.n_frames, self.n_smpls, self.v_pm = [], [], [], [], [], []
        # the samples of all utterances go straight into ONE float32 buffer (page-locked when the engine has one):
        # int16 PCM * 2^-15 and float64 -> float32 are each a single pass, no per-utterance temporaries, no concatenate
        total = int(sum(np.shape(u[0])[0] for u in utts))
        staged = hasattr(engine, "host_staging")
        # a batch of 16-bit wavs (what the batch scripts read) is staged and uploaded as int16 and widened on the
        # device (mpx_pcm16_to_f32): half the PCIe bytes and no host pass over the samples
        all_i16 = staged and len(utts) > 0 and all(np.asarray(u[0]).dtype == np.int16 for u in utts)
        if all_i16:
            buf = engine.host_staging((total + 1) // 2 + 2).view(np.int16)
        else:
            buf = engine.host_staging(total) if staged else np.empty(total, dtype=np.float32)
        off = 0
        if all_i16 and len(utts) > 1:   # 16-bit PCM of the whole batch into the staging buffer on a few native threads
            arrs = [np.ascontiguousarray(u[0]) for u in utts]
            k = len(arrs)
            src = (ctypes.c_void_p * k)(*[a.ctypes.data for a in arrs])
            nb = np.asarray([a.nbytes for a in arrs], dtype=np.int64)
            doff = np.concatenate(([0], np.cumsum(nb)[:-1])).astype(np.int64)
            n_thr = engine.host_threads(int(nb.sum())) if hasattr(engine, "host_threads") else 8

            def _copy(arrs=arrs, src=src, nb=nb, doff=doff):   # (keeps the arrays alive until the copy is done)
                if engine.lib.mpx_host_copy_many(len(arrs), src, nb.ctypes.data, doff.ctypes.data, buf.ctypes.data, n_thr) != 0:
                    raise _lib.MagphaseHipError("mpx_host_copy_many failed")

            copy_done = engine.background(_copy) if hasattr(engine, "background") else None
            if copy_done is None:
                _copy()
            copied = True
        else:
            copied, copy_done = False, None
        try:
            self._build_generic(engine, utts, fft_len, buf, off, copied, all_i16, staged, total, pos, left, right)
        except BaseException:
            # Whatever goes wrong between the submit and the upload (a malformed utterance, an fft_len mismatch): the native
            # copy must have stopped writing into the page-locked staging buffer before this constructor is left --
            # iobatch retries a failed batch one utterance at a time straight away, and host_staging would hand the same
            # buffer out again while the copy still runs (silent corruption of the retry's samples)
            if copy_done is not None:
                try:
                    copy_done.result()
                except BaseException:
                    pass
            raise
        if copy_done is not None:
            copy_done.result()   # the staged samples are in place (the copy ran beside the index arithmetic)
        self._upload_generic(engine, buf, all_i16, staged, total, pos, left, right)

    def _build_generic(self, engine, utts, fft_len, buf, off, copied, all_i16, staged, total, pos, left, right):
        for (v_sig, fs, v_pm_sec, v_voi) in utts:
            if not _is_tensor(v_sig):   # (a device tensor: _from_device, which copies no samples here)
                v_sig = np.asarray(v_sig)
            n = int(v_sig.shape[0])
            if copied:
                pass
            elif all_i16:
                buf[off:off + n] = v_sig
            elif v_sig.dtype == np.int16:
                np.multiply(v_sig, np.float32(1.0 / 32768.0), out=buf[off:off + n])   # exact: == astype(f32) / 32768
            else:
                buf[off:off + n] = v_sig
            N = fft_len if fft_len is not None else hm.define_fft_len(fs)
            if not hasattr(self, "fft_len"):
                self.fft_len = N
            elif N != self.fft_len:
                raise ValueError("all utterances of a plan must share fft_len (bucket by sample rate)")
            self.fs.append(fs)
            self.n_smpls.append(n)
            off += n
        sig_off = np.concatenate(([0], np.cumsum(self.n_smpls)))[:-1] if utts else np.zeros(0)
        try:     # the index arithmetic of the whole batch in one native call (hostplan / csrc/magphase_plan.cpp) ...
            r = hostplan.plan_analysis([u[2] for u in utts], [u[3] for u in utts], self.n_smpls, self.fs, sig_off)
            fo = r["frame_off"]
            for u in range(len(utts)):
                a, b = int(fo[u]), int(fo[u + 1])
                self.v_shift.append(r["left"][a:b]), self.v_pm.append(r["pm"][a:b]), self.v_f0.append(r["f0"][a:b])
                self.n_frames.append(b - a)
            pos[:], left[:], right[:] = [r["pos"]], [r["left"]], [r["right"]]
        except hostplan.PlanFallback:   # ... or utterance by utterance in numpy (same arithmetic; raises what it raises)
            for (v_sig, fs, v_pm_sec, v_voi), n, o in zip(utts, self.n_smpls, sig_off):
                pm_sec, voi = hm.clean_epochs(v_pm_sec, v_voi, check_len_smpls=n, fs=fs)
                pm, lft, rgt = hm.frame_bounds(pm_sec * fs, n)
                pos.append(pm + int(o))
                left.append(lft)
                right.append(rgt)
                self.v_shift.append(lft)
                self.v_pm.append(pm)
                self.v_f0.append(hm.shift_to_f0(lft, voi, fs))
                self.n_frames.append(pm.size)
        self.total_frames = int(sum(self.n_frames))
        self.frame_off = np.concatenate(([0], np.cumsum(self.n_frames))).astype(np.int64)
        right_cat = np.concatenate(right) if right else np.zeros(0, dtype=np.int64)
        # frames longer than fft_len (the reference warns once per such frame): rare -- one pass over the batch, the
        # per-utterance lists only where there is something to list
        self.long_frame_lens = [[] for _ in self.v_shift]
        if right_cat.size:
            left_cat = np.concatenate(left) if len(left) > 1 else np.asarray(left[0])
            tot = left_cat + right_cat + 1
            hit = np.flatnonzero(tot > self.fft_len)
            if hit.size:
                utt_of = np.searchsorted(self.frame_off, hit, side="right") - 1
                for i, u in zip(hit.tolist(), utt_of.tolist()):
                    self.long_frame_lens[u].append(int(tot[i]))
        self.total_smpls = int(off)

    def _upload_generic(self, engine, buf, all_i16, staged, total, pos, left, right):
        e = engine
        if all_i16:
            self.sig = _widen_pcm16(e, e.upload_staged((total + 1) // 2 + 2), total)
        else:
            self.sig = e.upload_staged(total) if staged else e.to_device(buf, np.float32)
        cat = [np.concatenate(x) if x else np.zeros(0) for x in (pos, left, right)]
        if self._keep_tabs:
            self._host_tabs = tuple(cat)
        desc = e.to_device_packed([("pos", cat[0], np.int64), ("left", cat[1], np.int32), ("right", cat[2], np.int32)])     # one H2D copy
        self.pos, self.left, self.right = desc["pos"], desc["left"], desc["right"]

    def _from_device(self, engine, utts, fft_len):
        """A batch with device-tensor signals (_signal_inputs has checked them): the tables as for host signals
        (hostplan.plan_analysis or its numpy fallback: they need the lengths only), self.sig = ONE contiguous float32
        device buffer -- a single float32 contiguous utterance where it lies, else torch converts and concatenates on the
        device (copy_: float64 -> float32 rounds to nearest even, as numpy's cast on the host path; float16 / bfloat16
        widen exactly; any element stride).  Host arrays in the same batch are uploaded one by one (the slow mixed case).
        No host staging, no D2H copy of samples; everything is queued on torch's current stream."""
        torch = _torch()
        pos, left, right = [], [], []
        self.v_shift, self.v_f0, self.fs, self.n_frames, self.n_smpls, self.v_pm = [], [], [], [], [], []
        self._build_generic(engine, utts, fft_len, None, 0, True, False, False, 0, pos, left, right)
        sigs = [u[0] for u in utts]
        with torch.cuda.device(engine.device):
            if len(sigs) == 1 and sigs[0].dtype == torch.float32 and sigs[0].is_contiguous():
                self.sig = sigs[0].detach()
            else:
                self.sig = engine.empty((max(self.total_smpls, 1),))[:self.total_smpls]
                a = 0
                for v, n in zip(sigs, self.n_smpls):
                    if _is_tensor(v):
                        self.sig[a:a + n].copy_(v.detach())
                    else:
                        v = np.asarray(v)
                        v = v.astype(np.float32) * np.float32(1.0 / 32768.0) if v.dtype == np.int16 else v.astype(np.float32)
                        self.sig[a:a + n].copy_(torch.from_numpy(np.ascontiguousarray(v)))
                    a += n
        cat = [np.concatenate(x) if x else np.zeros(0, dtype=np.int64) for x in (pos, left, right)]
        self._host_tabs = tuple(cat)
        desc = engine.to_device_packed([("pos", cat[0], np.int64), ("left", cat[1], np.int32), ("right", cat[2], np.int32)])
        self.pos, self.left, self.right = desc["pos"], desc["left"], desc["right"]

    def backward_tables(self):
        """(scratch_off device int64 [F + 1], scratch floats) of mpx_analysis_lossless_backward
        (hostmath.analysis_backward_table).  Built and uploaded by the first backward pass; a plan that kept no host
        copy of its frame tables reads them back from the device for that."""
        if getattr(self, "_bwd", None) is None:
            tabs = getattr(self, "_host_tabs", None)
            if tabs is None:
                _wait_ready(self)
                tabs = tuple(t.cpu().numpy() for t in (self.pos, self.left, self.right))
            _start, soff = hm.analysis_backward_table(tabs[0], tabs[1], tabs[2], self.fft_len, self.total_smpls)
            self._bwd = (self.engine.to_device(soff, np.int64), int(soff[-1]))
        return self._bwd

    def check_differentiable(self):
        """What run_backward cannot take, said before any launch: nothing."""

    def run_backward(self, mag, real, imag, grads):
        """The gradient of a loss with respect to the batch's samples, float32 [total_smpls] (utterance u at the offset
        of its samples in self.sig), given mag / real / imag = run()'s rows and grads = (dL/d mag, dL/d real, dL/d imag)
        as contiguous float32 [total_frames x H] matrices or None: k_analysis_lossless_bwd + k_analysis_bwd_gather."""
        _wait_ready(self)
        return self.engine.analysis_lossless_backward(self.fft_len, self, mag, real, imag, grads)

    def _from_prepared(self, p, utts):
        """Takes over a PreparedAnalysis: two DMAs (samples, tables) and, for 16-bit input, the widening kernel."""
        e, torch = self.engine, _torch()
        _check_prepared(p, e, utts)
        self.fft_len, self.fs = p.fft_len, p.fs
        self.n_smpls = [int(u[0].shape[0]) for u in utts]
        fo = self.frame_off = p.frame_off
        self.total_frames, self.total_smpls = p.total_frames, p.total_smpls
        self.n_frames = np.diff(fo).tolist()
        self.v_shift, self.v_pm, self.v_f0 = _FlatRows(p.left64, fo), _FlatRows(p.pm, fo), _FlatRows(p.f0, fo)
        self.f0_med_flat = p.f0_med
        self.long_frame_lens = [[] for _ in range(p.n_utts)]
        if p.long:
            utt_of = np.searchsorted(fo, [i for i, _n in p.long], side="right") - 1
            for (i, n), u in zip(p.long, utt_of.tolist()):
                self.long_frame_lens[u].append(n)
        F, total = p.total_frames, p.total_smpls
        o_pos, o_left, o_right, o_voi = p.offs
        if self._keep_tabs:   # (before the slot is handed to the upload: its descriptor block is reused afterwards)
            d = p.slot["desc_np"]
            self._host_tabs = tuple(d[o:o + w * F].view(t).copy()
                                    for o, w, t in ((o_pos, 8, np.int64), (o_left, 4, np.int32), (o_right, 4, np.int32)))
        slot, p.slot = p.slot, None          # from here on the upload's event guards the slot
        sd, dd, ev = e._slot_upload(slot, p.stage_bytes, p.desc_bytes)
        self._ready = ev
        if p.all_i16:
            self.sig = _widen_pcm16(e, sd, total)
        else:
            self.sig = sd[:4 * total].view(torch.float32)
        self.pos = dd[o_pos:o_pos + 8 * F].view(torch.int64)
        self.left = dd[o_left:o_left + 4 * F].view(torch.int32)
        self.right = dd[o_right:o_right + 4 * F].view(torch.int32)
        self.voi_dev = dd[o_voi:o_voi + 4 * F].view(torch.float32)    # (f0 > 0): CompressedAnalysisPlan's voicing row

    def run(self, out=None, precise=False, rows_in_use=None):
        _wait_ready(self)
        return self.engine.analysis_frames(self.fft_len, self.sig, self.pos, self.left, self.right, out=out,
                                           precise=precise, rows_in_use=rows_in_use if precise else None)


class LosslessSynthesisPlan:
    """
    PSOLA bookkeeping for a batch: per utterance v_f0 (float64) -> shift -> pm (magphase.py:1771-1772, Q2/Q3)
    -> ola() offsets and trimming (magphase.py:34-62) -> runs of frames for the fused overlap-add (hostmath.ola_runs).
    All float64/int host math; device gets int tables.
    """

    def __init__(self, engine, f0_list, fs_list, fft_len, frames_per_run=None, comp_slots=False, gcuts=None, n_slots=None,
                 extents=None):
        # extents: int [total frames, 2], what each frame of one kernel can add to the ring, or a callable(total frames) that
        #          returns them or None: a second run table for that kernel beside the plan's own (_plan_ola_runs, _SeamRuns)
        # comp_slots: the slot count and weights of the compressed / round-trip pair kernels (mpx_synth_comp_slots)
        # n_slots: overrides the engine's slot count (small tests; the launch grid follows it)
        # gcuts: the caller's cuts of the frame sequence, one share per slot, or a callable(n_slots, total_frames) that
        #        returns them or None (LosslessRoundTripPlan deals by cost); None: shares by count
        n_slots_arg = n_slots
        self.engine = engine
        self.fft_len = fft_len
        pm_rel, starts, lens, nfr = [], [], [], []
        self.v_pm = []
        try:
            r = hostplan.plan_lossless_synthesis(f0_list, fs_list, fft_len)
            fo = r["frame_off"]
            for u in range(len(f0_list)):
                a, b = int(fo[u]), int(fo[u + 1])
                self.v_pm.append(r["v_pm"][a:b]), pm_rel.append(r["pm_rel"][a:b])
                starts.append(int(r["out_start"][u])), lens.append(int(r["out_len"][u])), nfr.append(b - a)
        except hostplan.PlanFallback:
            for v_f0, fs in zip(f0_list, fs_list):
                v_pm = np.cumsum(hm.f0_to_shift(np.asarray(v_f0, dtype=np.float64), fs)).astype(int)
                rel, start, out_len = hm.ola_plan(v_pm, fft_len)
                self.v_pm.append(v_pm)
                pm_rel.append(rel)
                starts.append(start)
                lens.append(out_len)
                nfr.append(v_pm.size)
        self.out_len = [int(x) for x in lens]
        self.out_off_host = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
        self.total_out = int(self.out_off_host[-1])
        self.max_out_len = int(max(lens)) if lens else 0
        self.total_frames = int(sum(nfr))
        self._ola_host = (pm_rel, starts, lens, nfr)   # what backward_tables() is built from, should it ever be asked for
        self._bwd = None
        e = engine
        _up = []   # (attribute, host array, dtype): uploaded together (Engine.to_device_packed)
        _up.append(("utt_frame_off", np.concatenate(([0], np.cumsum(nfr))), np.int32))
        _up.append(("pm_rel", np.concatenate(pm_rel) if pm_rel else np.zeros(0), np.int32))
        _up.append(("out_start", np.asarray(starts), np.int32))
        _up.append(("out_off", self.out_off_host, np.int64))
        if comp_slots:   # True: the compressed synthesis kernel's slots and shares; "roundtrip": k_roundtrip_pair's
            n_slots = e.synth_comp_slots()
            weights = e.synth_ola_slot_weights(comp=comp_slots)
            if os.environ.get("MAGPHASE_RT_WEIGHTS") and weights is not None:   # experiment: "w0,w1,w2" by age rank of the pair
                w3 = [float(x) for x in os.environ["MAGPHASE_RT_WEIGHTS"].split(",")]
                # (6 wave pairs per 12-wave workgroup; pairs 0-1 / 2-3 / 4-5 hold the oldest / middle / youngest waves)
                weights = np.asarray([w3[((i % 6) * 2) // 4] for i in range(n_slots)], dtype=np.float32)
        else:
            n_slots = e.synth_ola_slots() if hasattr(e, "synth_ola_slots") else 1024
            weights = e.synth_ola_slot_weights() if hasattr(e, "synth_ola_slot_weights") else None
        if n_slots_arg is not None:
            n_slots = max(1, int(n_slots_arg))
            if weights is not None:   # the weights follow the slot's place in its workgroup: the first n_slots of them
                weights = np.asarray(weights)[:n_slots] if len(weights) >= n_slots else None
        if callable(gcuts):
            gcuts = gcuts(n_slots, self.total_frames)
        if callable(extents):
            extents = extents(self.total_frames)
        _plan_ola_runs(self, pm_rel, starts, lens, self.out_off_host, fft_len, n_slots, frames_per_run, _up, weights=weights,
                       gcuts=gcuts, extents=extents)
        for _k, _t in e.to_device_packed(_up).items():
            setattr(self, _k, _t)

    def run(self, mag, real, imag, strips=None, out=None):
        """Fused path: k_synth_ola_pair (per-run LDS overlap-add, output written in place) + k_ola_fixup (run boundaries)."""
        e = self.engine
        return _run_ola(e, lambda strips, out: e.synthesis_lossless_ola(self.fft_len, mag, real, imag, self, strips, out),
                        self.fft_len, self, strips, out, self.total_out)

    def backward_tables(self):
        """(pos, lo, hi) device tables of mpx_synthesis_lossless_backward: where every frame finds its gradient samples in
        the [total_out] buffer (hostmath.lossless_backward_table).  Built and uploaded by the first backward pass."""
        if self._bwd is None:
            pm_rel, starts, lens, nfr = self._ola_host
            rel = np.concatenate([np.asarray(r, dtype=np.int64) for r in pm_rel]) if pm_rel else np.zeros(0, np.int64)
            pos, lo, hi = hm.lossless_backward_table(rel, np.concatenate(([0], np.cumsum(nfr))), starts, lens,
                                                     self.out_off_host, self.fft_len)
            d = self.engine.to_device_packed([("pos", pos, np.int64), ("lo", lo, np.int32), ("hi", hi, np.int32)])
            self._bwd = (d["pos"], d["lo"], d["hi"])
        return self._bwd

    def check_differentiable(self):
        """What run_backward cannot take, said before any launch: nothing."""

    def run_backward(self, grad_out, mag, real, imag, need=(True, True, True)):
        """The gradients of run()'s waveform with respect to the rows of mag / real / imag, given grad_out = dL/d(waveform)
        (contiguous float32 [total_out]): k_synth_lossless_bwd.  None where need[k] is false."""
        return self.engine.synthesis_lossless_backward(self.fft_len, grad_out, self, mag, real, imag, need=need)

    def run_unfused(self, mag, real, imag, frames=None, out=None):
        """Two-kernel form: frames to HBM, then the ascending-order gather (bit-for-bit the reference's sum order)."""
        e = self.engine
        frames = e.synthesis_lossless_frames(self.fft_len, mag, real, imag, out=frames)
        return e.ola_gather(self.fft_len, frames, self.utt_frame_off, self.pm_rel, self.out_start, self.out_off,
                            self.max_out_len, self.total_out, out=out)


class LosslessRoundTripPlan:
    """
    Copy synthesis of a batch (analysis_lossless followed by synthesis_from_lossless on the same frames,
    demos/demo_copy_synthesis_lossless.py:44-50) as ONE launch: the analysis plan's frame tables plus a synthesis plan
    built from the f0 values the analysis derives on the host (magphase.py:2198-2207 -> :1771-1772), cut into runs for
    the round-trip kernel's slots.  run() returns ((mag, real, imag), pcm): the feature rows analysis_lossless returns
    and the waveform synthesis_from_lossless builds from them.
    """

    DEFAULT_STORES = "lines_nt"   # DESIGN.md 3.3a, "Row stores by line": the fastest form of the A/B
    DEFAULT_INVERSE = "direct"    # DESIGN.md 3.3a, "The windowed frame, added directly"

    def __init__(self, engine, utts, fft_len=None, frames_per_run=None, n_slots=None):
        # n_slots: overrides the engine's slot count (small tests)
        self.engine = engine
        self.deal = "count"   # how the frames were dealt to the slots: "cost" (_deal_by_cost) or "count"
        # MAGPHASE_RT_SUPPORT=full (read here, at plan build): every frame takes the full support class -- the A/B switch of
        # the kernel's compact-support instances (csrc/mpx_common.hpp: frame_support_class)
        self.full_support = os.environ.get("MAGPHASE_RT_SUPPORT", "") == "full"
        # MAGPHASE_RT_SEAMS=full (read here, at plan build; implied by MAGPHASE_RT_SUPPORT=full): the seams between runs are
        # sized as if every frame filled its N samples -- the A/B switch of the seams sized by what the frames really add
        # (_frame_extents, hostmath.ola_runs)
        self.full_seams = self.full_support or os.environ.get("MAGPHASE_RT_SEAMS", "") == "full"
        # MAGPHASE_RT_STORES=rows|lines|lines_nt (read here, at plan build): how the N = 4096 compact-support instance stores
        # the feature rows -- in 256-byte blocks aligned to the row, in blocks of two whole 128-byte lines of memory, or those
        # with the interior stores non-temporal (csrc/mpx_common.hpp, "Row stores by line"); the rows are the same, every
        # other instance ignores it
        self.stores = os.environ.get("MAGPHASE_RT_STORES", "") or self.DEFAULT_STORES
        if self.stores not in _lib.RT_STORE_FLAGS:
            raise ValueError("MAGPHASE_RT_STORES must be rows, lines or lines_nt, not %r" % self.stores)
        # MAGPHASE_RT_INVERSE=direct|transform (read here, at plan build): whether the N = 4096 instances overlap-add the
        # windowed frame they have just gathered, or rebuild it by Hermitian merge and inverse transform from its own
        # spectrum -- the A/B switch; the rows are the same, every other N transforms and ignores it
        self.inverse = os.environ.get("MAGPHASE_RT_INVERSE", "") or self.DEFAULT_INVERSE
        if self.inverse not in _lib.RT_INVERSE_FLAGS:
            raise ValueError("MAGPHASE_RT_INVERSE must be direct or transform, not %r" % self.inverse)
        if not utts:   # an empty batch: nothing to plan, run() returns empty tensors
            self.analysis = self.synthesis = self.seams = None
            self.seam_geometry = "dense" if self.full_seams else "extents"
            self.fft_len = fft_len or 4096
            self.total_frames = self.total_out = 0
            self.out_off_host = np.zeros(1, dtype=np.int64)
            return
        self.analysis = LosslessAnalysisPlan(engine, utts, fft_len=fft_len, keep_frame_tabs=True)
        self.fft_len = self.analysis.fft_len
        by_cost = (os.environ.get("MAGPHASE_RT_DEAL", "cost") != "count" and not frames_per_run
                   and not os.environ.get("MAGPHASE_OLA_FRAMES_PER_RUN"))
        self.synthesis = LosslessSynthesisPlan(engine, self.analysis.v_f0, self.analysis.fs, self.fft_len,
                                               frames_per_run=frames_per_run, comp_slots="roundtrip", n_slots=n_slots,
                                               gcuts=self._deal_by_cost if by_cost else None,
                                               extents=None if self.full_seams else self._frame_extents)
        if self.synthesis.total_frames != self.analysis.total_frames:
            raise ValueError("round trip: the synthesis plan must cover exactly the analysed frames")
        self.total_frames = self.analysis.total_frames
        self.total_out = self.synthesis.total_out
        self.out_off_host = self.synthesis.out_off_host
        # What run() launches by.  self.synthesis stays a complete plan for dense frames (its run table serves any
        # overlap-add kernel, k_synth_ola_pair on rows from elsewhere included); the table whose seams are sized by what THIS
        # kernel's frames add is the round trip's own: self.seams / self.runs_host (the dense one under MAGPHASE_RT_SEAMS=full)
        self.seams = _SeamRuns(self.synthesis) if hasattr(self.synthesis, "seam_runs") else self.synthesis
        # the geometry run() really has: "extents", or "dense" -- asked for (full_seams), or because the analysis plan kept
        # no host tables to take the extents from (dense is always valid; this attribute is where that shows)
        self.seam_geometry = "extents" if isinstance(self.seams, _SeamRuns) else "dense"

    @property
    def runs_host(self):
        """The run table run() launches by, as a host array (OLA_RUN_DTYPE); empty for an empty batch."""
        return self.seams.runs_host if self.seams is not None else np.zeros(0, dtype=hm.OLA_RUN_DTYPE)

    def _frame_extents(self, total_frames):
        """Per frame the samples that the instance of k_roundtrip_pair this plan launches can add to the ring
        (mpx_roundtrip_frame_extents: the library's own answer, from the kernel's compile-time condition and the launch
        flags), for the run planner's seams.  None -- dense frames -- without the analysis plan's host tables."""
        tabs = getattr(self.analysis, "_host_tabs", None)
        if tabs is None or int(np.size(tabs[1])) != total_frames or int(np.size(tabs[2])) != total_frames:
            return None
        left, right = (np.ascontiguousarray(t, dtype=np.int32) for t in (tabs[1], tabs[2]))
        ext = np.empty((total_frames, 2), dtype=np.int32)
        _lib.check(self.engine.lib.mpx_roundtrip_frame_extents(int(self.fft_len), left.ctypes.data, right.ctypes.data,
                                                               int(total_frames), 1 if self.full_support else 0,
                                                               ext.ctypes.data), "mpx_roundtrip_frame_extents")
        return ext

    def _deal_by_cost(self, n_slots, total_frames):
        """The cuts that deal the batch's frames to k_roundtrip_pair's slots by what they cost there, not by their number:
        a frame's cost grows with its length (the register rows its gather visits, a second sample tile beyond 1024
        samples), and a batch's long frames sit together in its low-pitched utterances -- shares of equal COUNT leave the
        slots that got those frames working while the others' compute units idle at the end of the launch.  Terms per frame
        from the analysis plan's left / right tables (mpx_roundtrip_frame_terms), coefficients per slot from the library
        (mpx_roundtrip_slot_costs: fitted per age class of the wave pair), min-max dealing (mpx_host_deal_cuts; the numpy
        twins when the native planners are off).  None -- shares by count, as every other plan -- with fewer frames than
        slots, or when neither form of the planner is to be had.  MAGPHASE_RT_DEAL=count (read at plan build) switches
        the dealing off: the A/B switch."""
        tabs = getattr(self.analysis, "_host_tabs", None)
        if tabs is None or total_frames < n_slots or int(np.size(tabs[1])) != total_frames:
            return None
        coef = np.zeros((n_slots, 3), dtype=np.int32)
        _lib.check(self.engine.lib.mpx_roundtrip_slot_costs(coef.ctypes.data, int(n_slots)), "mpx_roundtrip_slot_costs")
        if os.environ.get("MAGPHASE_RT_COSTS"):   # experiment: "a0,b0,c0,a1,b1,c1,a2,b2,c2" by age rank of the pair
            k9 = np.asarray([int(x) for x in os.environ["MAGPHASE_RT_COSTS"].split(",")], dtype=np.int32).reshape(3, 3)
            coef = np.ascontiguousarray(k9[((np.arange(n_slots) % 6) * 2) // 4])
        try:
            terms = hostplan.roundtrip_frame_terms(tabs[1], tabs[2], self.fft_len)
            cuts, _t = hostplan.deal_cuts(terms, coef)
        except hostplan.PlanFallback:
            try:
                terms = hm.roundtrip_frame_terms(tabs[1], tabs[2], self.fft_len)
                cuts, _t = hm.deal_cuts(terms, coef)
            except ValueError:   # the numpy twin refuses its input: the shares by count are always there
                return None
        self.deal = "cost"
        return cuts

    def run(self, feats=None, strips=None, out=None):
        e, a, s = self.engine, self.analysis, self.seams
        if feats is None:
            feats = tuple(e.empty_feats(self.total_frames, self.fft_len // 2 + 1) for _ in range(3))
        if out is None:
            out = e.empty((self.total_out,))
        if self.total_frames == 0:
            return feats, out
        _run_ola(e, lambda strips, out: e.roundtrip_lossless_ola(self.fft_len, a, s, feats, strips, out,
                                                                 full_support=self.full_support, stores=self.stores,
                                                                 inverse=self.inverse),
                 self.fft_len, s, strips, out, self.total_out)
        return feats, out


class LosslessConstRateAnalysisPlan:
    """
    analysis_lossless on a constant frame rate (magphase.py:2967-2980 with const_rate_ms as a parameter, without the mel
    warp that follows there): a LosslessAnalysisPlan (k_analysis writes the variable-rate rows into scratch), the row
    tables and f0 of hostmath.var_to_const_rate_batch (rows offset per utterance).  run() = k_analysis ->
    k_rows_lerp; the scratch is released once the interpolation is queued.
    """

    def __init__(self, engine, utts, fft_len=None, const_rate_ms=5.0, prepared=None):
        self.engine = e = engine
        self.const_rate_ms = hm.check_const_rate_ms(const_rate_ms)
        self.lossless = pl = LosslessAnalysisPlan(engine, utts, fft_len=fft_len, prepared=prepared)
        self.fft_len, self.fs, self.long_frame_lens = pl.fft_len, pl.fs, pl.long_frame_lens
        U = len(utts)
        self.row0_host, self.row1_host, self.rowt_host, self.v_f0, self.out_off = hm.var_to_const_rate_batch(
            [pl.v_shift[u] for u in range(U)], [pl.v_f0[u] for u in range(U)], pl.frame_off[:U], pl.fs,
            self.const_rate_ms)
        self.total_out_frames = int(self.out_off[-1])
        self.rows, _ = _upload_rows(e, (self.row0_host, self.row1_host, self.rowt_host))

    def run(self, out=None):
        """Returns (mag, real, imag) [total_out_frames x H] device rows (utterance u: rows out_off[u] .. out_off[u+1])."""
        e = self.engine
        H = self.fft_len // 2 + 1
        if out is None:
            out = tuple(e.empty_feats(self.total_out_frames, H) for _ in range(3))
        if self.total_out_frames == 0:
            return out
        var = self.lossless.run()
        e.rows_lerp(var, self.rows, self.total_out_frames, out=out)
        del var   # (stream-ordered: the allocator reuses the scratch after the interpolation)
        return out

    def check_differentiable(self):
        """What run_backward cannot take, said before any launch: nothing."""

    def _backward_inputs(self, grads):
        """The checks both backward forms share -> True when there is something to propagate."""
        torch = _torch()
        shp = (self.total_out_frames, self.fft_len // 2 + 1)
        if len(grads) != 3:
            raise ValueError("run_backward: grads = (g_mag, g_real, g_imag)")
        for g in grads:
            if g is not None and (g.dtype != torch.float32 or tuple(g.shape) != shp or not g.is_contiguous()):
                raise ValueError("run_backward: gradients must be contiguous float32 [%d x %d]" % shp)
        pl = self.lossless
        return not (self.total_out_frames == 0 or int(pl.total_frames) == 0 or int(pl.total_smpls) == 0
                    or all(g is None for g in grads))

    def _adjoint_table(self):
        """Per VARIABLE frame the constant-rate rows that read it (hostmath.lerp_adjoint_table of the plan's own host
        tables), device int32 [4 total_frames]; built and uploaded by the first backward pass."""
        if getattr(self, "_adj", None) is None:
            self._adj = self.engine.to_device(hm.lerp_adjoint_table(self.row0_host, self.row1_host, self.rowt_host,
                                                                    int(self.lossless.total_frames)).reshape(-1), np.int32)
        return self._adj

    def _zero_grad(self):
        return _torch().zeros((int(self.lossless.total_smpls),), dtype=_torch().float32, device=self.engine.device)

    def run_backward(self, grads):
        """The gradient of a loss with respect to the batch's samples, float32 [total_smpls] (utterance u at the offset of
        its samples in self.lossless.sig), given grads = (dL/d mag, dL/d real, dL/d imag) of run()'s constant-rate rows:
        contiguous float32 [total_out_frames x H], or None for an output nobody differentiated (not read).  Zeros when
        there are no rows, no frames or no gradients.  The variable-rate rows are RECOMPUTED (run() released them:
        nothing is kept between the passes); then the fused form, k_analysis_lossless_bwd<P, CR = true> (the frame's
        gradient row gathered from the constant-rate ones in registers) + k_analysis_bwd_gather.
        Equals run_backward_staged bit for bit."""
        if not self._backward_inputs(grads):
            return self._zero_grad()
        pl = self.lossless
        rows = pl.run()
        _wait_ready(pl)
        out = self.engine.analysis_lossless_const_rate_backward(self.fft_len, pl, rows[0], rows[1], rows[2], grads,
                                                                self._adjoint_table(), self.rows[2])
        del rows   # (stream-ordered: the allocator reuses the scratch after the backward launches)
        return out

    def run_backward_staged(self, grads):
        """run_backward from existing kernels only, the cross-check of the fused form: self.lossless.run() writes every
        row, k_rows_lerp_adjoint folds the constant-rate gradients onto [total_frames x H] scratch rows, then
        LosslessAnalysisPlan.run_backward (k_analysis_lossless_bwd<P> + k_analysis_bwd_gather)."""
        if not self._backward_inputs(grads):
            return self._zero_grad()
        e, pl = self.engine, self.lossless
        rows = pl.run()
        g_rows = e.rows_lerp_adjoint(grads, self._adjoint_table(), self.rows[2], int(pl.total_frames))
        out = pl.run_backward(rows[0], rows[1], rows[2], g_rows)
        del rows, g_rows
        return out


class LosslessConstRateSynthesisPlan:
    """
    synthesis_from_lossless from constant-rate rows (the reference's constant -> variable rate steps of
    synthesis_from_compressed, magphase.py:848, :861-870, followed by :1759-1776): per utterance f0 -> shifts, the
    uncapped scan (hostplan.const_to_variable_scan_uncapped), the row tables and voicing at the frame locations
    (hostmath.const_to_variable_rows), f0 at the variable rate (shift_to_f0, b_smooth=False); then a LosslessSynthesisPlan for the
    PSOLA bookkeeping.  run(): the LERP arm of k_synth_ola_pair (rows interpolated as they are loaded); run_staged():
    k_rows_lerp into variable-rate scratch rows, then k_synth_ola_pair.  Utterances without rows give empty signals.
    """

    def __init__(self, engine, f0_list, fs_list, fft_len, const_rate_ms=5.0, frames_per_run=None, host=None):
        # host: hostplan.plan_const_rate_synthesis(f0_list, fs_list, const_rate_ms) when the caller has it already
        self.engine = e = engine
        self.fft_len = int(fft_len)
        self.const_rate_ms = hm.check_const_rate_ms(const_rate_ms)
        r = host if host is not None else hostplan.plan_const_rate_synthesis(f0_list, fs_list, self.const_rate_ms)
        self.live, self.n_rows = r["live"], r["n_rows"]
        self.v_shift, self.v_locs, self.v_voi, self.v_f0 = r["v_shift"], r["v_locs"], r["v_voi"], r["v_f0"]
        self.row0_host, self.row1_host, self.rowt_host = r["row0"], r["row1"], r["rowt"]
        self.total_rows = int(sum(self.n_rows))
        self.inner = None
        out_len = [0] * len(self.n_rows)
        if self.live:
            self.inner = LosslessSynthesisPlan(e, self.v_f0, [fs_list[u] for u in self.live], self.fft_len,
                                               frames_per_run=frames_per_run)
            for k, u in enumerate(self.live):
                out_len[u] = self.inner.out_len[k]
            self.rows, _ = _upload_rows(e, (self.row0_host, self.row1_host, self.rowt_host))
        self.total_frames = self.inner.total_frames if self.inner is not None else 0
        self.out_len = out_len
        self.out_off_host = np.concatenate(([0], np.cumsum(out_len))).astype(np.int64)
        self.total_out = int(self.out_off_host[-1])

    def _check_rows(self, mag):
        if int(mag.shape[0]) != self.total_rows:
            raise ValueError("constant-rate rows: %d given, the plan has %d" % (int(mag.shape[0]), self.total_rows))

    def run(self, mag, real, imag, strips=None, out=None):
        """Fused: k_synth_ola_pair<P, LERP = true> + k_ola_fixup.  Returns the signals [total_out] (u at out_off_host[u])."""
        e = self.engine
        self._check_rows(mag)
        if out is None:
            out = e.empty((self.total_out,))
        if self.inner is None:
            return out
        s = self.inner
        return _run_ola(e, lambda strips, out: e.synthesis_lossless_ola_lerp(self.fft_len, mag, real, imag, self.rows, s,
                                                                              strips, out),
                        self.fft_len, s, strips, out, self.total_out)

    def check_differentiable(self):
        """What run_backward cannot take, said before any launch: nothing."""

    def run_backward(self, grad_out, mag, real, imag, need=(True, True, True)):
        """The gradients of run()'s waveform with respect to the constant-rate rows of mag / real / imag, given grad_out
        (contiguous float32 [total_out]): k_synth_lossless_bwd<P, LERP = true> into per-frame scratch rows, then
        k_rows_lerp_adjoint (frame ranges: hostmath.lerp_adjoint_table, uploaded by the first backward pass).  None where
        need[k] is false; rows that no frame reads get zeros."""
        e = self.engine
        self._check_rows(mag)
        H = self.fft_len // 2 + 1
        if self.inner is None:
            return tuple(e.empty_feats(self.total_rows, H).zero_() if n else None for n in need)
        if getattr(self, "_adj", None) is None:
            self._adj = e.to_device(hm.lerp_adjoint_table(self.row0_host, self.row1_host, self.rowt_host,
                                                          self.total_rows).reshape(-1), np.int32)
        var = e.synthesis_lossless_backward(self.fft_len, grad_out, self.inner, mag, real, imag, need=need, rows=self.rows)
        out = e.rows_lerp_adjoint(var, self._adj, self.rows[2], self.total_rows)
        del var   # (stream-ordered: the allocator reuses the scratch after the adjoint)
        return out

    def run_staged(self, mag, real, imag, rows_out=None, out=None):
        """Staged: k_rows_lerp into variable-rate rows [total_frames x H], then the unchanged k_synth_ola_pair."""
        self._check_rows(mag)
        if out is None:
            out = self.engine.empty((self.total_out,))
        if self.inner is None:
            return out
        var = self.engine.rows_lerp((mag, real, imag), self.rows, self.total_frames, out=rows_out)
        return self.inner.run(var[0], var[1], var[2], out=out)


class _OlaRuns:
    """Run / slot tables of one overlap-add kernel over a GriffinLimPlan's frames (pm_rel shared with the plan)."""


class GriffinLimPlan:
    """
    Device tables of griffin_lim (magphase.py:3320-3372) for a batch of utterances sharing fft_len: shifts -> epochs ->
    ola bookkeeping and the analysis frame tables of every iteration (hostmath.griffin_lim_plan), the runs of the first
    synthesis (k_synth_ola_pair's slots, mpx_synthesis_lossless_ola) and of the iterations (k_griffin_lim_pair's: the
    round-trip kernel's slots and weights), two signal buffers (ping-pong: an iteration never reads the buffer it writes)
    and the head strips.  run() returns (signal, phase rows or None).
    """

    def __init__(self, engine, shift_list, fft_len, frames_per_run=None):
        self.engine = e = engine
        self.fft_len = N = int(fft_len)
        r = hm.griffin_lim_plan(shift_list, N)
        self.v_pm = r["v_pm"]
        self.out_len = [int(x) for x in r["out_len"]]
        self.out_off_host = r["out_off"]
        self.frame_off = r["frame_off"]
        self.total_out = int(self.out_off_host[-1])
        self.total_frames = int(self.frame_off[-1])
        up = [("pm_rel", np.concatenate(r["pm_rel"]), np.int32), ("frame_pos", r["frame_pos"], np.int64),
              ("frame_left", r["frame_left"], np.int32), ("frame_right", r["frame_right"], np.int32)]
        for k, t in e.to_device_packed(up).items():
            setattr(self, k, t)
        self.synth, self.iter = _OlaRuns(), _OlaRuns()
        starts = [int(x) for x in r["out_start"]]
        for runs, n_slots, w in ((self.synth, e.synth_ola_slots(), e.synth_ola_slot_weights()),
                                 (self.iter, e.synth_comp_slots(), e.synth_ola_slot_weights(comp="roundtrip"))):
            up = []
            _plan_ola_runs(runs, r["pm_rel"], starts, self.out_len, self.out_off_host, N, n_slots, frames_per_run, up,
                           weights=w)
            for k, t in e.to_device_packed(up).items():
                setattr(runs, k, t)
            runs.pm_rel = self.pm_rel
        self.strips = e.empty((max(self.synth.strip_floats, self.iter.strip_floats, 1),))
        self.bufs = (e.empty((max(self.total_out, 1),)), e.empty((max(self.total_out, 1),)))

    def run(self, target, init, niters, phase_rows=False):
        """target: device magnitude rows [F x H] (row pitch target.stride(0)); init: a LIST [mag', phasor real, phasor imag]
        of rows of the same pitch for the first synthesis (hostmath.griffin_lim_fold), emptied once that synthesis is
        queued -- nothing else reads them, so their memory goes back to the allocator (stream-ordered) before the
        iterations; niters >= 1 syntheses.  phase_rows (niters >= 2): rows of the same pitch receive the phase
        synthesised last (written by the last iteration), allocated after the init rows are released.
        Returns (signal buffer: total_out samples, utterance u at out_off_host[u]; phase rows or None)."""
        e, N = self.engine, self.fft_len
        a, b = self.bufs
        e.synthesis_lossless_ola(N, init[0], init[1], init[2], self.synth, self.strips, a)
        e.ola_fixup(N, self.synth, self.strips, a)
        init.clear()
        phase = None
        if phase_rows and niters > 1:
            phase = e.empty((max(self.total_frames, 1), int(target.stride(0))))[:self.total_frames, :target.shape[1]]
        for i in range(1, int(niters)):
            e.griffin_lim_ola(N, self, target, a, b, self.strips, phase_out=phase if i == niters - 1 else None)
            e.ola_fixup(N, self.iter, self.strips, b)
            a, b = b, a
        return a[:self.total_out], phase


# ======================================================================================================
# compressed-feature synthesis (magphase.py:825-997)
# ======================================================================================================
class CompressedSynthesisPlan:
    """
    Host fp64 bookkeeping + device tables for a batch of utterances synthesised from compressed features.
    utts: list of (m_mag_mel_log [F x mag_dim], m_real_mel [F x phase_dim], m_imag_mel, v_lf0 [F]) float arrays.
    Follows magphase.py:836-897 (constants, f0/voicing/shift, constant->variable rate scan, epochs, noise length,
    noise windows) and :969-976 (anti-ringing lengths, ola) -- all index math in float64/int on the host.
    """

    # what Type2SynthesisPlan changes: the planner for a grid the native one does not know, the phase unwarp matrix and
    # the per-bin curves, the noise statistic and the entry of the pair kernel
    _native_planner = True      # Engine.prepare_synthesis / hostplan.plan_synthesis serve this plan's frame tables
    _n_per_key = "n_per"
    _ola_entry = "mpx_synthesis_compressed_ola"
    _bwd_entry = "mpx_synthesis_compressed_backward"

    def __init__(self, engine, utts, fs, fft_len=None, b_voi_ap_win=True, b_const_rate=False, alpha_phase=None,
                 noise=None, frames_per_run=None, per_phase_type="magphase", post_filter=False, b_fbank_mel=False,
                 noise_mode="reference", noise_seeds=None, defer_rng=False, noise_spectra=None, prepared=None):
        # prepared: a PreparedSynthesis of these utterances (Engine.prepare_synthesis, e.g. from the planner thread)
        # noise_spectra: None = MAGPHASE_NOISE_SPECTRA ("recompute", the default / "store"); True: every noise frame is
        #            transformed once, its spectrum kept in HBM between the statistics and the synthesis launch (N = 4096)
        # defer_rng: the reference noise stream's advanced state stays on the device (Engine.numpy_global_uniform(defer=True));
        #            the caller owes Engine.mt_sync() before numpy's global generator is used again
        # post_filter: False / True ('magphase': mp.post_filter on the device) / 'merlin' (mp.post_filter_merlin on the device)
        # (the reference's pf_type vocabulary: 'no' means no filtering, magphase.py:3229-3262 -- anything else is an error,
        #  not silently "on")
        if isinstance(post_filter, str):
            if post_filter not in ("no", "magphase", "merlin"):
                raise ValueError("post_filter must be False / None / 'no', True / 'magphase' or 'merlin', not %r" % (post_filter,))
            self.apply_post_filter = {"no": False, "magphase": "magphase", "merlin": "merlin"}[post_filter]
        elif post_filter is None or isinstance(post_filter, (bool, np.bool_, int, np.integer)):
            # truthy non-bool callers (b_post_filter=1, a numpy comparison's np.bool_) mean what bool() says
            if post_filter is not None and not isinstance(post_filter, (bool, np.bool_)) and int(post_filter) not in (0, 1):
                raise ValueError("post_filter must be False / None / 'no', True / 'magphase' or 'merlin', not %r" % (post_filter,))
            self.apply_post_filter = bool(post_filter)
        else:
            raise ValueError("post_filter must be False / None / 'no', True / 'magphase' or 'merlin', not %r" % (post_filter,))
        self.b_const_rate = bool(b_const_rate)
        if noise_mode not in ("reference", "device"):
            raise ValueError("noise_mode must be 'reference' (numpy global RNG, magphase.py:883) or 'device' (Philox on the GPU)")
        self.noise_mode = noise_mode
        if noise_mode == "device" and noise is not None:
            raise ValueError("noise_mode='device' generates the source itself: do not pass noise")

        if per_phase_type not in ("magphase", "min_phase", "linear"):
            raise ValueError("per_phase_type must be 'magphase', 'min_phase' or 'linear'")
        self.per_phase_type = per_phase_type

        self.engine = e = engine
        self.fs = fs
        N = self.fft_len = int(fft_len) if fft_len else hm.define_fft_len(fs)
        alpha = hm.define_alpha(fs)
        self.alpha_phase = alpha if alpha_phase is None else alpha_phase
        # Variable-rate features (rows == frames: identity tables, weight 0) take the same unwarp launch as constant-rate ones
        # (mpx_mel_unwarp_rows): the interpolation is then exact (fmaf(0, 0, m) = m: the same values as mpx_mel_unwarp), and the
        # phase rows are produced only where the synthesis reads them -- voiced frames, bins below the crossfade's end: a
        # quarter of the work of the plain form, which unwarped all 2 049 bins of both phase streams for every frame (round 5:
        # 0.81 -> ... ms per 128-utterance generation launch).  MAGPHASE_UNWARP_ROWS_VAR=0: the plain form.
        self.unwarp_rows = self.b_const_rate or os.environ.get("MAGPHASE_UNWARP_ROWS_VAR", "1") != "0"
        # the native whole-launch planner (Engine.prepare_synthesis; `prepared`: built ahead, e.g. on the planner thread) takes
        # the plain case: ndarray coefficient matrices, the default run planner
        if prepared is not None and any(_is_tensor(x) for utt in utts for x in utt):
            prepared.release()
            raise ValueError("prepared= was built from host arrays: it cannot be combined with tensor inputs")
        if (prepared is None and frames_per_run is None and self._native_planner and hasattr(e, "prepare_synthesis")
                and not os.environ.get("MAGPHASE_OLA_FRAMES_PER_RUN") and os.environ.get("MAGPHASE_NATIVE_PREPARE", "1") != "0"):
            prepared = e.prepare_synthesis(utts, fs, fft_len=fft_len, b_voi_ap_win=b_voi_ap_win, b_const_rate=b_const_rate,
                                           wait=False)
        if prepared is not None:
            _check_prepared(prepared, e, utts)
        if prepared is not None and (frames_per_run is not None or prepared.key != (
                int(fs), N, bool(b_const_rate), bool(b_voi_ap_win), bool(self.unwarp_rows))):
            prepared.release()
            prepared = None
        # either builder sets the batch's shape (mag_dim, phase_dim, n_rows, n_utts, frame_off, ns_len, out_len), the host
        # tables behind v_shift / v_pm / v_voi (_tabs), the runs (n_runs, n_slots, runs_host) and the device tables, and
        # returns the staged coefficients on the device; what follows from those is the same for both
        if prepared is not None:
            coef, mt_device = self._tables_prepared(prepared, noise, noise_mode, noise_seeds)
        else:
            coef, mt_device = self._tables_generic(utts, b_voi_ap_win, noise, noise_mode, noise_seeds, frames_per_run)
        self.strip_floats = self.n_runs * (N + 64)
        n_m, n_p = self.n_rows * self.mag_dim, self.n_rows * self.phase_dim
        self.a_mag = coef[:n_m].view(self.n_rows, self.mag_dim)
        self.a_real = coef[n_m:n_m + n_p].view(self.n_rows, self.phase_dim)
        self.a_imag = coef[n_m + n_p:n_m + 2 * n_p].view(self.n_rows, self.phase_dim)
        H = N // 2 + 1
        # constants: unwarp matrices and per-bin curves (float64 -> float32)
        # (resident on the device per configuration: rebuilding them costs 7 ms on the host, as much as the rest of a
        # single-utterance call -- tools/archive/latency_probe.py)
        if b_fbank_mel:   # magphase.py:851-852: filter-bank unwarp = a different [mag_dim x H] matrix, same kernel
            self.u_mag = e.constant(("u_mag_fbank", self.mag_dim, H, float(alpha)),
                                    lambda: hm.unwarp_fbank_matrix(self.mag_dim, H, alpha))
        else:
            self.u_mag = e.constant(("u_mag", self.mag_dim, H, float(alpha)),
                                    lambda: hm.unwarp_matrix(self.mag_dim, H, alpha))
        self._phase_and_curve_constants()
        self._gains_dev = None
        # "noise spectra once" (opt-in): see run()
        self.noise_spectra = ((os.environ.get("MAGPHASE_NOISE_SPECTRA", "recompute") == "store")
                              if noise_spectra is None else bool(noise_spectra))
        if noise_mode == "device":
            self.noise = e.empty((max(int(self.noise_off_host[-1]), 1),))
            e.launch("mpx_noise_uniform", self.n_utts, self.noise_seeds_dev, self.noise_off_dev, int(max(self.ns_len)),
                     self.noise)
        elif mt_device:
            self.noise = e.numpy_global_uniform(int(sum(self.ns_len)), defer=bool(defer_rng))

    def _phase_and_curve_constants(self):
        e, fs, N = self.engine, self.fs, self.fft_len
        self.u_phase = e.constant(("u_phase", self.phase_dim, N, int(fs), float(self.alpha_phase)),
                                  lambda: hm.phase_unwarp_matrix(self.phase_dim, N, fs, self.alpha_phase))
        self.per_v, self.ap_v, self.ap_u = (
            e.constant(("bin_curve", k, int(fs), N), lambda k=k: hm.synthesis_bin_curves(fs, N)[k]) for k in range(3))

    def _bin_curves_host(self):
        return hm.synthesis_bin_curves(self.fs, self.fft_len)

    def _n_per(self):
        """Bins from n_per on have no periodic component (the curve is exactly zero there)."""
        return self.engine.host_constant((self._n_per_key, int(self.fs), self.fft_len), lambda: hm._first_all_zero_from(
            np.asarray(self._bin_curves_host()[0], dtype=np.float32)))

    def _plan_tables(self, lf0s, b_voi_ap_win):
        """The batch's frame tables (hostplan.plan_synthesis' layout)."""
        fs, N, b_const_rate = self.fs, self.fft_len, self.b_const_rate
        try:    # index arithmetic of the whole batch in one native call (hostplan / csrc/magphase_plan.cpp) ...
            return hostplan.plan_synthesis([np.exp(l) for l in lf0s], fs, N, b_const_rate, b_voi_ap_win)   # :846
        except hostplan.PlanFallback:   # ... or utterance by utterance in numpy: the same arithmetic, spelled out
            return hostplan.plan_synthesis_numpy(lf0s, fs, N, b_const_rate, b_voi_ap_win)

    def _mt_device(self, noise, noise_mode, mt_total):
        """Reference noise (np.random.uniform from numpy's GLOBAL generator, magphase.py:883) for more than a few utterances
        is continued on the device from numpy's own MT19937 state (mpx_noise_numpy_mt19937: the same samples, the state put
        back advanced) -- the host draw is 4 ns per sample, 0.13 s per 128 utterances."""
        return (noise_mode == "reference" and noise is None and mt_total >= (1 << 18)
                and os.environ.get("MAGPHASE_MT_DEVICE", "1") != "0" and np.random.get_state()[0] == "MT19937")

    def _host_noise(self, noise, ui, ns_len):
        e = self.engine
        if noise is not None:
            v_ns = np.asarray(noise[ui], dtype=np.float64)
            if v_ns.size != ns_len:
                raise ValueError("noise length %d != ns_len %d" % (v_ns.size, ns_len))
            return v_ns
        if hasattr(e, "mt_sync"):
            e.mt_sync()                                            # a deferred device state goes back first
        return np.random.uniform(-1, 1, ns_len)                    # :883 (global numpy RNG, as the reference)

    def _set_layout(self, frame_off, ns_len, out_len, tabs, noise, noise_mode):
        """What both table builders derive from the planner's per-utterance results: frame_off int64[U + 1], ns_len /
        out_len per utterance, tabs with v_shift / v_pm / voiced per frame.  Returns _mt_device's decision."""
        # per-utterance views (v_shift / v_pm / v_voi: properties below) are cut from the batch tables on demand
        self._tabs = tabs
        self.frame_off = self._fo = np.asarray(frame_off, dtype=np.int64)
        self.n_utts, self.total_frames = int(self.frame_off.size - 1), int(self.frame_off[-1])
        self.ns_len = [int(x) for x in np.asarray(ns_len).tolist()]
        self.out_len = [int(x) for x in np.asarray(out_len).tolist()]
        self.out_off_host = np.concatenate(([0], np.cumsum(self.out_len))).astype(np.int64)
        self.total_out = int(self.out_off_host[-1])
        self.max_out_len = int(max(self.out_len))
        self.voiced_host = np.asarray(tabs["voiced"]).astype(bool)
        # bins from n_per on have no periodic component (the crossfade mask is exactly zero there): their phase rows are
        # neither unwarped nor read
        self.n_per = self._n_per()
        return self._mt_device(noise, noise_mode, int(sum(self.ns_len)))

    def _noise_seed_tables(self, noise_seeds):
        """noise_mode='device': the seeds and the utterances' offsets into the noise, as items of a packed upload."""
        seeds = np.arange(self.n_utts, dtype=np.uint64) if noise_seeds is None else np.asarray(noise_seeds).astype(np.uint64)
        if seeds.size != self.n_utts:
            raise ValueError("noise_seeds: one per utterance")
        self.noise_seeds = seeds
        self.noise_off_host = np.concatenate(([0], np.cumsum(self.ns_len))).astype(np.int64)
        return [("noise_seeds_dev", seeds.view(np.int64), np.int64), ("noise_off_dev", self.noise_off_host, np.int64)]

    def _host_noise_cat(self, noise):
        return np.concatenate([self._host_noise(noise, ui, n) for ui, n in enumerate(self.ns_len)])

    def _tables_prepared(self, p, noise, noise_mode, noise_seeds):
        """Takes over a PreparedSynthesis (Engine.prepare_synthesis): two DMAs (coefficient rows, every table)."""
        e, torch = self.engine, _torch()
        self.mag_dim, self.phase_dim, self.n_rows = p.mag_dim, p.phase_dim, p.n_rows
        F, U = p.total_frames, p.n_utts
        mt_device = self._set_layout(p.frame_off, p.ns_len, p.out_len,
                                     {"v_shift": p.v_shift, "v_pm": p.v_pm, "voiced": p.voiced_host}, noise, noise_mode)
        self.n_runs, self.n_slots, self.runs_host = p.n_runs, p.n_slots, p.runs_host
        slot, p.slot = p.slot, None
        sd, dd, self._ready = e._slot_upload(slot, p.stage_bytes, p.desc_bytes)
        sizes = {"utt_frame_off": U + 1, "tile_first": p.n_tiles1, "out_start": U, "out_off": U + 1,
                 "runs": 56 * p.n_runs, "slot_off": p.n_slots + 1, "slot_runs": p.n_runs}
        tmap = {np.int32: torch.int32, np.int64: torch.int64, np.float32: torch.float32, np.uint8: torch.uint8}
        for (name, dt), off in zip(hostplan.SYNTH_TABLES, p.desc_off.tolist()):
            n = sizes.get(name, F)
            if name == "tile_first" and not self.unwarp_rows:
                continue
            setattr(self, name, dd[off:off + n * np.dtype(dt).itemsize].view(tmap[dt]))
        if noise_mode == "device":
            for k, t in e.to_device_packed(self._noise_seed_tables(noise_seeds)).items():
                setattr(self, k, t)
        elif not mt_device:
            self.noise = e.to_device(self._host_noise_cat(noise), np.float32)
        return sd.view(torch.float32), mt_device

    def _tables_generic(self, utts, b_voi_ap_win, noise, noise_mode, noise_seeds, frames_per_run):
        """The generic path: any array-like input, utterance by utterance in Python where the native planner declines.
        One staged upload (coefficient rows) and one packed upload (every table)."""
        e = self.engine
        self.mag_dim = int(np.shape(utts[0][0])[1])
        self.phase_dim = int(np.shape(utts[0][1])[1])
        a_mag, a_real, a_imag, lf0s = [], [], [], []
        nd = np.ndarray
        # Coefficient matrices that are tensors on the engine's device (an acoustic model's output) stay there: the three
        # streams are gathered into a fresh device `coef` by one mpx_rows_pack launch (Engine.pack_rows) -- no host staging,
        # no upload.  Host arrays in such a batch are uploaded one by one and packed with the rest (the slow mixed case).
        # lf0 always comes to the host (the frame tables are float64 host arithmetic): device vectors in ONE copy.
        on_dev = lf0_tensors = False
        for ui, (mml, rm, im, lf0) in enumerate(utts):
            # the coefficient matrices go to the device as float32 whatever they arrive as: no float64 round trip here
            # (a plan is built per launch of a corpus job: the usual case -- 2-D ndarrays -- skips the generic conversions)
            if not (type(mml) is nd and type(rm) is nd and type(im) is nd and mml.ndim == 2 and rm.ndim == 2 and im.ndim == 2):
                mml, rm, im = (_rows_or_array(e, x, "utterance %d: %s" % (ui, n_))
                               for x, n_ in ((mml, "m_mag_mel_log"), (rm, "m_real_mel"), (im, "m_imag_mel")))
                on_dev = on_dev or any(type(x) is not nd for x in (mml, rm, im))
            if type(lf0) is not nd and _is_tensor(lf0):
                hm.check_feature_tensor(lf0, "utterance %d: v_lf0" % ui, lf0=True)
                lf0_tensors = True     # (brought down after the loop, all of them in one copy)
            else:
                lf0 = np.atleast_1d(np.asarray(lf0, dtype=np.float64))
            n_rows = mml.shape[0]
            if rm.shape[0] != n_rows or im.shape[0] != n_rows or lf0.shape[0] != n_rows:
                raise ValueError("utterance %d: mag / real / imag / lf0 have %d / %d / %d / %d frames"
                                 % (ui, n_rows, rm.shape[0], im.shape[0], lf0.shape[0]))
            if rm.shape[1] != im.shape[1]:
                raise ValueError("utterance %d: real and imag have different dimensions" % ui)
            if mml.shape[1] != self.mag_dim or rm.shape[1] != self.phase_dim:
                # (stage_rows checks totals only: rows of another width whose totals happen to match would be copied flat,
                # silently scrambled -- np.concatenate(axis=0, out=[rows x dim]) used to raise here)
                raise ValueError("utterance %d: mag / phase dimensions %d / %d differ from the batch's %d / %d"
                                 % (ui, mml.shape[1], rm.shape[1], self.mag_dim, self.phase_dim))
            a_mag.append(mml), a_real.append(rm), a_imag.append(im), lf0s.append(lf0)
        self.n_rows = int(sum(a.shape[0] for a in a_mag))
        if lf0_tensors:
            lf0s = e.lf0_to_host(lf0s)

        r = self._plan_tables(lf0s, b_voi_ap_win)
        mt_device = self._set_layout(r["frame_off"], r["ns_len"], r["out_len"], r, noise, noise_mode)
        starts = [int(x) for x in np.asarray(r["out_start"]).tolist()]
        pm_rel = _FlatRows(np.asarray(r["pm_rel"]), r["frame_off"])
        up = [("utt_frame_off", self.frame_off, np.int32)]   # (attribute, host array, dtype): ONE upload (to_device_packed)
        # coefficient matrices: concatenated straight into the page-locked staging buffer, one DMA
        n_m, n_p = self.n_rows * self.mag_dim, self.n_rows * self.phase_dim
        if not on_dev:
            stage = e.host_staging(n_m + 2 * n_p)
            # (inline: on the helper thread -- Engine.background -- the launch loop of a generation job got 5 % SLOWER, the
            # three calls' Python glue fights the constructor for the GIL; the analysis plan's single native copy gains 7 %)
            e.stage_rows(a_mag, stage[:n_m].reshape(self.n_rows, self.mag_dim))
            e.stage_rows(a_real, stage[n_m:n_m + n_p].reshape(self.n_rows, self.phase_dim))
            e.stage_rows(a_imag, stage[n_m + n_p:].reshape(self.n_rows, self.phase_dim))
        if noise_mode == "device":
            up += self._noise_seed_tables(noise_seeds)
        elif not mt_device:
            up.append(("noise", self._host_noise_cat(noise), np.float32))
        up += [("npos", r["npos"], np.int64), ("nleft", r["nleft"], np.int32), ("nright", r["nright"], np.int32),
               ("wtype", r["wtype"], np.int32), ("voiced", r["voiced"], np.int32)]
        if self.unwarp_rows:   # frames of every 31-row tile of the coefficient matrix (mpx_mel_unwarp_rows)
            self._check_rows_for_tiles(r["row0"], r["row1"])
            up.append(("tile_first", np.searchsorted(r["row0"], 31 * np.arange((self.n_rows + 30) // 31 + 1), side="left"),
                       np.int32))
        up += [("row0", r["row0"], np.int32), ("row1", r["row1"], np.int32), ("rowt", r["rowt"], np.float32),
               ("win_l", r["win_l"], np.int32), ("win_r", r["win_r"], np.int32), ("pm_rel", pm_rel.flat, np.int32),
               ("out_start", np.asarray(starts), np.int32), ("out_off", self.out_off_host, np.int64)]
        # OLA runs
        n_slots = e.synth_comp_slots() if hasattr(e, "synth_comp_slots") else 1024
        _plan_ola_runs(self, pm_rel, starts, self.out_len, self.out_off_host, self.fft_len, n_slots, frames_per_run, up,
                       weights=e.synth_ola_slot_weights(comp=True) if hasattr(e, "synth_ola_slot_weights") else None)
        if on_dev:
            coef = e.empty((max(n_m + 2 * n_p, 1),))
            e.pack_rows([a_mag, a_real, a_imag], [coef[:n_m].view(self.n_rows, self.mag_dim),
                                                  coef[n_m:n_m + n_p].view(self.n_rows, self.phase_dim),
                                                  coef[n_m + n_p:n_m + 2 * n_p].view(self.n_rows, self.phase_dim)])
        else:
            coef = e.upload_staged(n_m + 2 * n_p)
        for k, t in e.to_device_packed(up).items():
            setattr(self, k, t)
        return coef, mt_device

    def _per_utt(self, key, cast=None):
        r, fo = self._tabs, self._fo
        out = [r[key][int(fo[u]):int(fo[u + 1])] for u in range(len(self.ns_len))]
        return [cast(x) for x in out] if cast else out

    @property
    def v_shift(self):
        """Per utterance: the frames' shifts in samples (magphase.py:862-868 / :2210-2215)."""
        return self._per_utt("v_shift")

    @property
    def v_pm(self):
        """Per utterance: the frames' epochs in samples (la.shift_to_pm, magphase.py:880)."""
        return self._per_utt("v_pm")

    @property
    def v_voi(self):
        """Per utterance: the frames' voicing decisions (magphase.py:847, :866)."""
        return self._per_utt("voiced", lambda x: x.astype(bool))

    @staticmethod
    def _check_rows_for_tiles(r0, r1):
        """What the tiled unwarp relies on: row0 ascending over the batch, row1 - row0 in {0, 1}."""
        if r0.size and (np.any(np.diff(r0) < 0) or np.any((r1 - r0) < 0) or np.any((r1 - r0) > 1)):
            raise ValueError("constant -> variable rate tables out of order")

    @property
    def gains(self):
        """[(g_voiced, g_unvoiced)] per utterance (float64), fetched from the device on demand."""
        if self._gains_dev is None:
            return None
        g = self._gains_dev.cpu().numpy()
        return [(float(a), float(b)) for a, b in g]

    def noise_gains(self, sums_host):
        """magphase.py:902-906 (Q10) from the per-frame sums of (ln|Ns|)^2: two gains per utterance, float64."""
        H = self.fft_len // 2 + 1
        inv = np.ones(self.total_frames)
        gains = []
        for u in range(len(self.out_len)):
            a, b = int(self.frame_off[u]), int(self.frame_off[u + 1])
            s = np.asarray(sums_host[a:b], dtype=np.float64)
            v = self.voiced_host[a:b]
            g = []
            for cls in (v, ~v):
                ncls = int(np.sum(cls))
                g.append(np.sqrt(np.exp(np.sum(s[cls]) / (ncls * (H - 2)))) if ncls else np.nan)
                if ncls:
                    inv[a:b][cls] = 1.0 / g[-1]
            gains.append(tuple(g))
        return inv

    def _buffers(self):
        """Work buffers of run(), allocated once per plan (the caching allocator makes a re-allocation per call cheap
        but not free: ~1.6 GB of spectra + strips + per-frame scalars)."""
        b = getattr(self, "_buf", None)
        if b is None:
            e, torch = self.engine, _torch()
            H = self.fft_len // 2 + 1
            ld = int(e.lib.mpx_spec_ld(H))
            b = self._buf = dict(
                ld=ld,
                # unwarped spectra at the VARIABLE rate: one row per synthesis frame (mpx_mel_unwarp_rows interpolates)
                spec=tuple(e.empty((self.total_frames, ld))[:, :H] for _ in range(3)),
                sums=e.empty((self.total_frames,)),
                inv_gain=e.empty((self.total_frames,)),
                gains=torch.empty((self.n_utts, 2), dtype=torch.float64, device=e.device),
                strips=e.empty((max(self.strip_floats, 1),)),
            )
            if self.per_phase_type != "magphase":
                F = self.total_frames
                b["ident"] = torch.arange(F, dtype=torch.int32, device=e.device)
                b["zeros_t"] = torch.zeros(F, dtype=torch.float32, device=e.device)
                b["spec_v"] = tuple(e.empty((F, ld))[:, :H] for _ in range(3))
        return b

    def _launch_noise_statistic(self, tab, buf, mark):
        """The noise statistic of the utterances and buf["inv_gain"] from it; returns the stored noise spectra, or None."""
        e, N = self.engine, self.fft_len
        H = N // 2 + 1
        sums, inv_gain = buf["sums"], buf["inv_gain"]
        nspec = None
        if N == 4096 and self.total_frames > 0 and self.noise_spectra:
            nspec = buf.get("nspec")
            if nspec is None:
                nspec = buf["nspec"] = e.empty((int(e.lib.mpx_noise_spectra_floats(N, self.total_frames)),))
        stats = (N, tab, self.noise, self.npos, self.nleft, self.nright, self.wtype, self.total_frames, sums)
        if nspec is not None:
            e.launch("mpx_noise_stats_spectra", *stats, nspec)
        else:
            e.launch("mpx_noise_stats", *stats)
        mark("k_noise_stats")
        # two gains per utterance (Q10): float64 reduction on the device, no host round trip
        self._gains_dev = buf["gains"]
        e.launch("mpx_noise_gains", sums, self.voiced, self.utt_frame_off, self.n_utts, H - 2, inv_gain, self._gains_dev)
        mark("k_noise_gains")
        return nspec

    def run(self, out=None, keep=False, mark=None):
        """mark: optional callable(name), called after every kernel launch has been enqueued (bench.py: HIP events)."""
        e, N = self.engine, self.fft_len
        H = N // 2 + 1
        tab = e.tables(N)
        mark = mark or (lambda name: None)
        _wait_ready(self)
        buf = self._buffers()
        # unwarped spectra: internal matrices, rows 128-byte aligned (mpx_spec_ld: full-line stores of the MFMA unwarp)
        ld = buf["ld"]
        mag, real, imag = buf["spec"]
        sums, strips, inv_gain = buf["sums"], buf["strips"], buf["inv_gain"]
        pcm = out if out is not None else e.empty((self.total_out,))
        magphase = self.per_phase_type == "magphase"
        mark("start")
        a_mag = self.a_mag
        if self.apply_post_filter == "merlin":   # magphase.py:3262-3264
            a_mag = e.post_filter_merlin(self.a_mag, self.fs)
            mark("k_post_filter_merlin")
        elif self.apply_post_filter:   # magphase.py:3259-3261
            a_mag = e.post_filter(self.a_mag, self.fs)
            mark("k_post_filter")
        if self.unwarp_rows:   # constant -> variable rate inside the unwarp: one spectrum row per synthesis frame
            e.launch("mpx_mel_unwarp_rows", self.total_frames, H, a_mag, self.mag_dim, self.u_mag, mag, self.a_real,
                     self.a_imag, self.phase_dim, self.u_phase, real, imag, ld, self.row0, self.row1, self.rowt,
                     self.n_rows, self.tile_first, self.voiced if magphase else None,
                     hm.synth_comp_phase_columns(N, self.n_per) if magphase else 0)   # every column the synthesis reads
        else:                   # variable-rate features: rows == frames
            e.launch("mpx_mel_unwarp", self.n_rows, H, a_mag, self.mag_dim, self.u_mag, mag, self.a_real, self.a_imag,
                     self.phase_dim, self.u_phase, real, imag, ld)
        mark("k_mel_unwarp_mfma")
        # (the noise chain is independent of the unwarp, but a second HIP stream does not help: measured 3.13 vs
        # 3.18 ms per step with 12-wave and 3.15 vs 3.16 with 8-wave noise workgroups -- the two grids do not co-run)
        # "noise spectra once" (opt-in, MAGPHASE_NOISE_SPECTRA=store; N = 4096): the statistics launch
        # stores every frame's noise spectrum and the synthesis launch loads it instead of a second transform --
        # 17.4 KB per frame each way for the arithmetic of one forward FFT (measured: docs/LAB_NOTES.md, round 5)
        nspec = self._launch_noise_statistic(tab, buf, mark)
        if not magphase:
            # periodic component's phase is not the transmitted one (magphase.py:933-938):
            #   'min_phase': complex-cepstrum minimum phase of the magnitude, per frame
            #   'linear'   : zero phase
            if self.per_phase_type == "min_phase":
                ident, spec_v = buf["ident"], buf["spec_v"]
                e.launch("mpx_min_phase", N, tab, mag, ident, ident, buf["zeros_t"], self.total_frames, *spec_v, ld)
                mark("k_min_phase")
                mag, real, imag = spec_v
            else:
                real.fill_(1.0)
                imag.fill_(0.0)
        ola_args = (N, tab, mag, real, imag, self.noise, self.npos, self.nleft, self.nright, self.wtype, self.voiced,
                    inv_gain, None, None, None, self.win_l, self.win_r, self.pm_rel, self.per_v, self.ap_v, self.ap_u,
                    self.runs, self.n_runs, self.slot_off, self.slot_runs, self.n_slots, strips, pcm, ld,
                    self.n_per if magphase else 0)
        if nspec is not None:
            e.launch("mpx_synthesis_compressed_ola_spectra", *ola_args, nspec)
        else:
            e.launch(self._ola_entry, *ola_args)
        mark("k_synth_comp_pair")
        e.ola_fixup(N, self, strips, pcm)
        mark("k_ola_fixup")
        if keep:
            self.debug = dict(mag=mag, real=real, imag=imag, sums=sums)
        return pcm

    # ------------------------------------------------------------------ backward pass
    def backward_tables(self):
        """The device tables of run_backward, built and uploaded by the first backward pass: where every frame finds its
        gradient samples in the [total_out] buffer (hostmath.lossless_backward_table, from the plan's own pm_rel /
        out_start tables), the index that reverses every utterance in place (the adjoint high-pass; formed on the device
        from the utterances' offsets) and, at the constant rate, the frame ranges of the row interpolation's adjoint
        (hostmath.lerp_adjoint_table)."""
        b = getattr(self, "_bwd", None)
        if b is None:
            e, torch = self.engine, _torch()
            _wait_ready(self)
            rel = self.pm_rel.cpu().numpy().astype(np.int64)
            starts = self.out_start.cpu().numpy().astype(np.int64)
            pos, lo, hi = hm.lossless_backward_table(rel, self.frame_off, starts, self.out_len, self.out_off_host,
                                                     self.fft_len)
            b = dict(e.to_device_packed([("pos", pos, np.int64), ("lo", lo, np.int32), ("hi", hi, np.int32),
                                         ("off", self.out_off_host, np.int64)]))
            # sample t of utterance u <-> sample off[u] + off[u + 1] - 1 - t: built on the device from the offsets
            off = b["off"]
            utt = torch.repeat_interleave(torch.arange(self.n_utts, device=e.device), off[1:] - off[:-1],
                                          output_size=self.total_out)
            b["rev"] = (off[:-1] + off[1:] - 1)[utt] - torch.arange(self.total_out, device=e.device)
            if self.b_const_rate:
                r0, r1 = self.row0.cpu().numpy(), self.row1.cpu().numpy()
                b["adj"] = e.to_device(hm.lerp_adjoint_table(r0, r1, np.zeros(r0.size), self.n_rows).reshape(-1), np.int32)
            self._bwd = b
        return b

    def check_differentiable(self):
        """What run_backward cannot take, said before any launch."""
        if not self._bwd_entry:
            raise NotImplementedError("%s has no backward pass" % type(self).__name__)
        if self.per_phase_type != "magphase":
            raise NotImplementedError("per_phase_type=%r has no backward pass (only 'magphase')" % (self.per_phase_type,))
        if self.apply_post_filter:
            raise NotImplementedError("b_post_filter has no backward pass")

    def adjoint_hpf(self, grad, fs=None, design="butter40"):
        """The adjoint of the output high-pass (Engine.output_hpf: a causal LTI filter per utterance, from a zero state) is
        the same filter run backwards in time: grad [total_out] -> float32, every utterance reversed, filtered, reversed
        again, float32.  design: Engine.output_hpf's ('ellip60': the type-2 synthesis' output filter)."""
        torch = _torch()
        rev = self.backward_tables()["rev"]
        g = grad.to(torch.float32).reshape(-1)
        g = self.engine.output_hpf(g.index_select(0, rev).contiguous(), self.out_off_host, self.fs if fs is None else fs,
                                   design=design)
        return g.index_select(0, rev).to(torch.float32)

    def run_backward(self, grad_pcm, need=(True, True, True), mark=None):
        """The gradients of run()'s waveform with respect to the coefficient rows (a_mag [n_rows x mag_dim], a_real and
        a_imag [n_rows x phase_dim]), given grad_pcm = dL/d(run()'s result): contiguous float32 [total_out].  None where
        need[k] is false.  After run(): the unwarped rows (spec) and the noise gains of the plan's work buffers are read,
        not recomputed.  k_synth_comp_bwd (per-frame gradient rows; the noise spectra are recomputed -- a plan that
        stores them, MAGPHASE_NOISE_SPECTRA=store, is differentiated the same way and the stored spectra are not read),
        at the constant rate k_rows_lerp_adjoint at width H and the forward's unwarp again at the rows' rate (E),
        k_mel_unwarp_bwd (up to three jobs in one launch), at the constant rate k_rows_lerp_adjoint at width phase_dim."""
        return self._run_backward(grad_pcm, "spec", tuple(bool(n) for n in need), mark=mark)

    def _run_backward(self, grad_pcm, spec, need, min_phase=False, phase_jobs=True, mark=None):
        """The body of run_backward, here and in MagnitudeSynthesisPlan.  spec: the key of the three work-buffer rows the
        pair kernel read ('spec', or 'spec_v': k_min_phase's outputs); need: which of the per-frame gradient rows (g_m, g_a,
        g_b) k_synth_comp_bwd writes; min_phase: k_min_phase_bwd folds g_a / g_b into g_m (in place) after it; phase_jobs:
        k_mel_unwarp_bwd runs the phase jobs that need[1:] ask for (false: the magnitude job alone, no phase operand).
        -> (o_m, o_a, o_b), None where not computed."""
        self.check_differentiable()
        torch = _torch()
        e, N = self.engine, self.fft_len
        H = N // 2 + 1
        F, R = self.total_frames, self.n_rows
        mark = mark or (lambda name: None)
        if (grad_pcm.dtype != torch.float32 or int(grad_pcm.numel()) != self.total_out or not grad_pcm.is_contiguous()):
            raise ValueError("run_backward: grad_pcm must be a contiguous float32 [%d]" % self.total_out)
        want = need if phase_jobs else (need[0], False, False)
        if F == 0 or R == 0 or not any(need):
            return tuple(torch.zeros((R, d), dtype=torch.float32, device=e.device) if n else None
                         for n, d in zip(want, (self.mag_dim, self.phase_dim, self.phase_dim)))
        buf = getattr(self, "_buf", None)
        if buf is None:
            raise RuntimeError("run_backward: call run() first (the backward pass reads the forward's unwarped rows)")
        t = self.backward_tables()
        ld = buf["ld"]
        mag, real, imag = buf[spec]
        n_per = int(self.n_per)
        n_ph = min((n_per + 63) // 64 * 64, H)
        tab = e.tables(N)
        mark("start")
        # per-frame gradient rows, allocated apart from spec (whose rows the kernel reads)
        g_m, g_a, g_b = (e.empty((F, ld))[:, :H] if n else None for n in need)
        e.launch(self._bwd_entry, N, tab, grad_pcm, self.total_out, t["pos"], t["lo"], t["hi"],
                 F, mag, real, imag, ld, self.noise, self.npos, self.nleft, self.nright, self.wtype, self.voiced,
                 buf["inv_gain"], self.win_l, self.win_r, self.per_v, self.ap_v, self.ap_u, n_per, g_m, g_a, g_b, ld)
        mark("k_synth_comp_bwd")
        if min_phase:   # in place: element k of a row is read and written by one lane
            e.launch("mpx_min_phase_backward", N, tab, mag, real, imag, ld, g_m, g_a, g_b, ld, n_ph, F, g_m, ld)
            mark("k_min_phase_bwd")
        # E, the unwarped magnitude the mel unwarp's backward multiplies by: spec's, whichever rows the pair kernel read
        e_mag, g_e, ld_g = buf["spec"][0], g_m, ld
        if self.b_const_rate and need[0]:
            g_e = e.rows_lerp_adjoint((g_m, None, None), t["adj"], self.rowt, R)[0]
            ld_g = int(g_e.stride(0))
            mark("k_rows_lerp_adjoint")
            # E = exp(U_mag^T a_mag) at the rows' rate: the forward's unwarp again (its phase outputs are scratch)
            e_mag, s_r, s_i = (e.empty((R, ld)) for _ in range(3))
            e.launch("mpx_mel_unwarp", R, H, self.a_mag, self.mag_dim, self.u_mag, e_mag, self.a_real, self.a_imag,
                     self.phase_dim, self.u_phase, s_r, s_i, ld)
            del s_r, s_i
            mark("k_mel_unwarp_mfma")
        o_m = e.empty((R, self.mag_dim)) if need[0] else None
        if phase_jobs:
            n_prow = F if self.b_const_rate else R      # (variable rate: rows == frames)
            o_a, o_b = (e.empty((n_prow, self.phase_dim)) if n else None for n in need[1:])
            u_phase = self.u_phase
        else:   # the magnitude job alone
            g_a = g_b = o_a = o_b = u_phase = None
            n_ph = n_prow = 0
        e.launch("mpx_mel_unwarp_backward", H, e_mag, ld, g_e, ld_g, self.u_mag, self.mag_dim, R, o_m, g_a, g_b, ld, n_ph,
                 u_phase, self.phase_dim, n_prow, o_a, o_b)
        mark("k_mel_unwarp_bwd")
        if self.b_const_rate and (o_a is not None or o_b is not None):
            _none, o_a, o_b = e.rows_lerp_adjoint((None, o_a, o_b), t["adj"], self.rowt, R)
            mark("k_rows_lerp_adjoint")
        return o_m, o_a, o_b


def check_type2_grad_dims(mag_dim, phase_dim):
    """The backward pass of the type-2 synthesis goes through k_mel_unwarp_bwd, which produces at most 64 coefficient
    columns per job."""
    for name, d in (("m_mag_mel_log (mag_dim)", mag_dim), ("m_real_mel / m_imag_mel (phase_dim)", phase_dim)):
        if int(d) > 64:
            raise NotImplementedError("%s has %d columns: the backward pass of the type-2 synthesis takes at most 64"
                                      % (name, int(d)))


class Type2SynthesisPlan(CompressedSynthesisPlan):
    """
    synthesis_from_compressed_type2 (magphase.py:1452-1597, the output filter excluded) for a batch of utterances: the
    type-1 plan's tables, buffers and launch sequence with
      * the grid's period as a parameter (const_rate_ms > 0; <= 0: the variable rate) and type 2's voicing rules on it
        (hostplan.plan_synthesis_numpy(type2=True); the variable rate keeps the native planner, its arithmetic is type 1's),
      * the phase coefficients extended to mag_dim columns and unwarped at alpha (hm.type2_phase_unwarp_matrix),
      * the plain crossfade curves and the hf_slope line (hm.type2_synthesis_bin_curves),
      * one noise gain per utterance, rms of the noise spectra over all frames and bins, from mpx_noise_power +
        mpx_noise_rms (no transform) instead of mpx_noise_stats + mpx_noise_gains,
      * the type-2 arm of the pair kernel (mpx_synthesis_compressed_type2_ola: signed real DC / Nyquist bins).
    Constants are cached under keys of their own and the gain buffers belong to the plan: running a type-2 plan leaves
    nothing behind that a type-1 plan on the same engine reads.
    """
    _n_per_key = "n_per_t2"
    _ola_entry = "mpx_synthesis_compressed_type2_ola"
    _bwd_entry = "mpx_synthesis_compressed_type2_backward"

    def __init__(self, engine, utts, fs, fft_len=None, hf_slope_coeff=1.0, b_voi_ap_win=True, const_rate_ms=-1.0,
                 noise=None, frames_per_run=None, noise_mode="reference", noise_seeds=None, defer_rng=False):
        self.const_rate_ms = float(const_rate_ms)
        self.hf_slope_coeff = float(hf_slope_coeff)
        const = self.const_rate_ms > 0.0
        self._native_planner = not const
        super().__init__(engine, utts, fs, fft_len=fft_len, b_voi_ap_win=b_voi_ap_win, b_const_rate=const, noise=noise,
                         frames_per_run=frames_per_run, noise_mode=noise_mode, noise_seeds=noise_seeds,
                         defer_rng=defer_rng, noise_spectra=False)
        self._rms_dev = None

    def _plan_tables(self, lf0s, b_voi_ap_win):
        if not self.b_const_rate:
            return super()._plan_tables(lf0s, b_voi_ap_win)
        return hostplan.plan_synthesis_numpy(lf0s, self.fs, self.fft_len, True, b_voi_ap_win,
                                             const_rate_ms=self.const_rate_ms, type2=True)

    def _bin_curves_host(self):
        return hm.type2_synthesis_bin_curves(self.fs, self.fft_len, self.hf_slope_coeff)

    def _phase_and_curve_constants(self):
        e, fs, N = self.engine, self.fs, self.fft_len
        H, alpha = N // 2 + 1, hm.define_alpha(fs)
        self.u_phase = e.constant(("u_phase_t2", self.phase_dim, self.mag_dim, H, float(alpha)),
                                  lambda: hm.type2_phase_unwarp_matrix(self.phase_dim, self.mag_dim, H, alpha))
        self.per_v, self.ap_v, self.ap_u = (
            e.constant(("bin_curve_t2", k, int(fs), N, self.hf_slope_coeff), lambda k=k: self._bin_curves_host()[k])
            for k in range(3))

    def check_differentiable(self):
        """run_backward serves this plan as it stands: u_phase and n_per are the type-2 ones, the
        gain is constant.  What k_mel_unwarp_bwd cannot take is said here, before any launch."""
        super().check_differentiable()
        check_type2_grad_dims(self.mag_dim, self.phase_dim)

    @property
    def gains(self):
        """Type 2 has one gain per utterance: see rms."""
        return None

    @property
    def rms(self):
        """[rms_noise] per utterance (float64, magphase.py:1539), fetched from the device on demand."""
        return None if self._rms_dev is None else [float(x) for x in self._rms_dev.cpu().numpy()]

    def _buffers(self):
        b = getattr(self, "_buf", None)
        if b is None:
            b = super()._buffers()
            torch = _torch()
            b["power"] = torch.empty((max(self.total_frames, 1),), dtype=torch.float64, device=self.engine.device)
            b["rms"] = torch.empty((self.n_utts,), dtype=torch.float64, device=self.engine.device)
        return b

    def _launch_noise_statistic(self, tab, buf, mark):
        e, N, power = self.engine, self.fft_len, buf["power"]
        e.launch("mpx_noise_power", N, self.noise, self.npos, self.nleft, self.nright, self.wtype, self.total_frames, power)
        mark("k_noise_power")
        self._rms_dev = buf["rms"]
        e.launch("mpx_noise_rms", N, power, self.utt_frame_off, self.n_utts, buf["inv_gain"], self._rms_dev)
        mark("k_noise_rms")
        return None


class MagnitudeSynthesisPlan(CompressedSynthesisPlan):
    """
    Synthesis from the mel-log magnitudes and lf0 alone (magphase.py:922-938: per_phase_type 'min_phase' / 'linear'), with
    a backward pass.  utts: list of (m_mag_mel_log [F x mag_dim], v_lf0 [F]); phase: 'min_phase'
    (the complex-cepstrum minimum phase of the unwarped magnitude, k_min_phase) or 'zero' (the reference's 'linear').
    The caller supplies no phase matrices: the plan feeds the unwarp one zero column per stream (its phase outputs are
    overwritten before anything reads them).  run() is CompressedSynthesisPlan.run() with that per_phase_type -- the same
    launches, the same samples.  run_backward(grad_pcm) -> float32 [n_rows x mag_dim]:
      k_synth_comp_bwd against the rows the pair kernel read (g_m, and for 'min_phase' g_a / g_b),
      k_min_phase_bwd ('min_phase': g_m += T^t g_phi / m, in place),
      at the constant rate k_rows_lerp_adjoint at width H and the forward's unwarp again at the rows' rate (E),
      k_mel_unwarp_bwd with the magnitude job only.
    """
    _PHASES = {"min_phase": "min_phase", "zero": "linear"}

    def __init__(self, engine, utts, fs, fft_len=None, phase="min_phase", b_voi_ap_win=True, b_const_rate=False,
                 noise=None, frames_per_run=None, post_filter=False, b_fbank_mel=False, noise_mode="reference",
                 noise_seeds=None, defer_rng=False):
        if phase not in self._PHASES:
            raise ValueError("phase must be 'min_phase' or 'zero', not %r" % (phase,))
        self.phase = phase
        full = []
        for ui, u in enumerate(utts):
            if len(u) != 2:
                raise ValueError("utterance %d: expected (m_mag_mel_log, v_lf0)" % ui)
            mml, lf0 = u
            if not _is_tensor(mml):
                mml = np.asarray(mml)
            if mml.ndim != 2:
                raise ValueError("utterance %d: m_mag_mel_log must be 2-D" % ui)
            if _is_tensor(mml):
                z = _torch().zeros((int(mml.shape[0]), 1), dtype=_torch().float32, device=mml.device)
            else:
                z = np.zeros((int(mml.shape[0]), 1), dtype=np.float32)
            full.append((mml, z, z, lf0))
        super().__init__(engine, full, fs, fft_len=fft_len, b_voi_ap_win=b_voi_ap_win, b_const_rate=b_const_rate,
                         noise=noise, frames_per_run=frames_per_run, per_phase_type=self._PHASES[phase],
                         post_filter=post_filter, b_fbank_mel=b_fbank_mel, noise_mode=noise_mode, noise_seeds=noise_seeds,
                         defer_rng=defer_rng)

    def check_differentiable(self):
        """What run_backward cannot take, said before any launch.  The plan's own rules, not CompressedSynthesisPlan's: its
        per_phase_type is the one this backward pass is for."""
        if self.apply_post_filter:
            raise NotImplementedError("b_post_filter has no backward pass")
        if int(self.mag_dim) > 64:
            raise NotImplementedError("m_mag_mel_log (mag_dim) has %d columns: the backward pass takes at most 64"
                                      % int(self.mag_dim))

    def run_backward(self, grad_pcm, mark=None):
        """The gradient of run()'s waveform with respect to the magnitude rows a_mag, float32 [n_rows x mag_dim], given
        grad_pcm = dL/d(run()'s result): contiguous float32 [total_out].  After run(): the rows the pair kernel read and
        the noise gains are taken from the plan's work buffers."""
        min_phase = self.phase == "min_phase"
        # the rows k_synth_comp_pair read: k_min_phase's outputs, or the unwarped magnitude beside the constant phasor 1 + 0j
        return self._run_backward(grad_pcm, "spec_v" if min_phase else "spec", (True, min_phase, min_phase),
                                  min_phase=min_phase, phase_jobs=False, mark=mark)[0]


# ======================================================================================================
# compressed-feature analysis (magphase.py:2947-2988, 2490-2544)
# ======================================================================================================
def _check_warp_grads(plan, grads):
    """The (dL/d m_mag_mel_log, dL/d m_real_mel, dL/d m_imag_mel) a compressed analysis' run_backward takes."""
    torch, Fo = _torch(), plan.total_out_frames
    for g, shp in zip(grads, ((Fo, plan.mag_dim), (Fo, plan.phase_dim), (Fo, plan.phase_dim))):
        if g is not None and (g.dtype != torch.float32 or tuple(g.shape) != shp or not g.is_contiguous()):
            raise ValueError("run_backward: gradients must be contiguous float32 of the outputs' shapes")


def _lerp_adjoint_table(plan, n_var):
    """The frame ranges of the row interpolation's adjoint over the plan's n_var variable-rate rows
    (hostmath.lerp_adjoint_table of its host row tables), uploaded by the first backward pass."""
    if getattr(plan, "_adj", None) is None:
        r0, r1, rt = plan._rows_host
        plan._adj = plan.engine.to_device(hm.lerp_adjoint_table(r0, r1, rt, n_var).reshape(-1), np.int32)
    return plan._adj


def _warp_backward(plan, outs, grads, rows, tabs, live, n_var, mask_nonfinite=False, mark=None):
    """The gradients of a compressed analysis' three matrices taken back through the two mel warps, onto the n_var
    variable-rate rows = (mag, real, imag) the warps read (recomputed by the caller): k_phase_grad_mask (the forward's
    voicing mask and clip, read from outs), k_mel_warp_bwd (the three jobs in one launch; live: the phase job's row flags
    or None) and, where the forward read its rows through the row tables tabs = (row0, row1, rowt) (None: output rows ==
    rows), k_rows_lerp_adjoint at width phase_dim before it and on the magnitude gradients after it.  mask_nonfinite: an
    output frame whose log-mel row the forward wrote non-finite gets a zero magnitude gradient.  -> per-row gradients."""
    e, H = plan.engine, int(plan.fft_len) // 2 + 1
    mark = mark or (lambda name: None)
    g_m, g_r, g_i = grads
    h_r, h_i = e.phase_grad_mask(outs[1], outs[2], plan.voi, g_r, g_i)
    if tabs is not None:
        # the masked phase gradients onto the variable-rate rows the forward interpolated from (width phase_dim)
        _none, h_r, h_i = e.rows_lerp_adjoint((None, h_r, h_i), _lerp_adjoint_table(plan, n_var), plan.rowt, n_var)
    mark("k_phase_grad_mask")
    have_ph = h_r is not None or h_i is not None
    g_rows = e.mel_warp_backward(H, mag=(g_m, plan.w_mag, rows[0], tabs) if g_m is not None else None,
                                 phase=(h_r, h_i, plan.w_ph, rows[1], rows[2], live) if have_ph else None)
    mark("k_mel_warp_bwd")
    if g_rows[0] is not None and mask_nonfinite:
        # An output frame whose log-mel row the forward wrote as NaN (an envelope row it reads has a zero bin: digital
        # silence) has no gradient: zero -- not the kernel's NaN x 0, which the interpolation's adjoint would carry
        # into the finite neighbouring row.  (k_true_envelope_bwd gives such an envelope row a zero gradient too.)
        g_rows[0].masked_fill_((~_torch().isfinite(outs[0]).all(dim=1))[:, None], 0.0)
    if g_rows[0] is not None and tabs is not None:
        g_rows = (e.rows_lerp_adjoint((g_rows[0], None, None), _lerp_adjoint_table(plan, n_var), plan.rowt, n_var)[0],) \
            + tuple(g_rows[1:])
        mark("k_rows_lerp_adjoint")
    return g_rows


class CompressedAnalysisPlan:
    """
    Lossless analysis plan + host tables for the mel warp of a batch (one sample rate).  run() = k_analysis ->
    k_mel_warp, everything resident on the device; host fp64 does f0 / lf0 / constant-rate tables only.
    """

    def __init__(self, engine, utts, fft_len=None, mag_dim=60, phase_dim=10, b_const_rate=False, alpha_phase=None,
                 b_mag_fbank_mel=False, prepared=None):
        # prepared: see LosslessAnalysisPlan (Engine.prepare_analysis, e.g. from the planner thread)
        self.engine = e = engine
        self.lossless = plan = LosslessAnalysisPlan(engine, utts, fft_len=fft_len, prepared=prepared)
        fs = self.fs = plan.fs[0]
        if plan.fs.count(fs) != len(plan.fs):
            raise ValueError("one sample rate per batch")
        N = self.fft_len = plan.fft_len
        H = N // 2 + 1
        self.mag_dim, self.phase_dim, self.b_const_rate = int(mag_dim), int(phase_dim), bool(b_const_rate)
        alpha = hm.define_alpha(fs)
        a_ph = alpha if alpha_phase is None else alpha_phase
        cf, _ = hm.define_crossfade_params(fs)
        k_full = hm.get_num_full_mel_coeffs_from_num_phase_coeffs(cf, phase_dim, a_ph, fs)
        self.w_mag, self._warp_name = e.warp_mag_matrix(mag_dim, H, alpha, b_mag_fbank_mel)
        self.w_ph = e.constant(("w_ph", int(k_full), H, float(a_ph), int(phase_dim)),
                               lambda: hm.warp_matrix(k_full, H, a_ph, nrows=phase_dim))
        rows = None
        if b_const_rate:
            U = len(utts)
            row0, row1, rowt, self.f0_out, self.out_off = hm.var_to_const_rate_batch(
                [plan.v_shift[u] for u in range(U)], [plan.v_f0[u] for u in range(U)], plan.frame_off[:U], fs, 5.0)
            rows = (row0, row1, rowt)
            self._rows_host = rows   # (run_backward builds the adjoint's frame ranges from them)
        else:   # variable rate: output rows == frames (no row tables go to the device)
            self.f0_out = plan.v_f0 if isinstance(plan.v_f0, _FlatRows) else list(plan.v_f0)
            self.out_off = np.asarray(plan.frame_off, dtype=np.int64)
        self.total_out_frames = int(self.out_off[-1])
        if isinstance(self.f0_out, _FlatRows):
            f0_cat = self.f0_out.flat
        else:
            f0_cat = np.concatenate(self.f0_out) if self.f0_out else np.zeros(0)
        voi_dev = None if b_const_rate else getattr(plan, "voi_dev", None)   # already in the prepared tables' upload
        items, tail = ([] if voi_dev is not None else [("voi", (f0_cat > 0).astype(np.float32), np.float32)]), []
        # phase streams warped on the variable-rate rows, their 45 outputs interpolated afterwards (mpx_mel_warp_rows):
        # the rows a voiced constant-rate frame interpolates from
        self.phase_on_rows = bool(b_const_rate) and os.environ.get("MAGPHASE_WARP_PHASE_ROWS", "1") != "0"
        if self.phase_on_rows:
            voiced = f0_cat > 0
            need = np.zeros(plan.total_frames, dtype=np.float32)
            need[row0[voiced]] = 1.0
            need[row1[voiced]] = 1.0
            tail.append(("rows_in_use", need, np.float32))
        # one H2D copy
        if rows is not None:
            (self.row0, self.row1, self.rowt), desc = _upload_rows(e, rows, head=items, tail=tail)
        else:
            self.row0 = self.row1 = self.rowt = None
            desc = e.to_device_packed(items) if items else {}
        self.voi = desc["voi"] if voi_dev is None else voi_dev
        self.rows_in_use = desc.get("rows_in_use")
        self._phase_tmp = None
        # Variable frame rate: ONE fused kernel, the lossless features never reach HBM (mpx_analysis_compressed_fused;
        # MAGPHASE_COMP_FUSED=0 keeps the staged pair k_analysis_f64 -> k_mel_warp_mfma).  The constant-rate path
        # interpolates staged lossless rows, as the reference does (SURVEY.md 8d allows that staging).
        fusable = (N in (2048, 4096) and self.mag_dim <= 64 and self.phase_dim <= 48
                   and os.environ.get("MAGPHASE_COMP_FUSED", "1") != "0"
                   and os.environ.get("MAGPHASE_COMP_ANALYSIS", "f64") != "f32")
        self.fused = fusable and not b_const_rate
        # Constant rate: the staged pair k_analysis_f64 -> k_mel_warp_mfma, which interpolates staged lossless rows as the
        # reference does (SURVEY.md 8d allows that staging), or -- MAGPHASE_COMP_FUSED_CR=1 -- the same ONE kernel with the
        # row interpolation inside (mpx_analysis_compressed_fused_cr: the magnitudes' operand rows are built per
        # constant-rate frame, the phase streams are warped at the variable rate and finished by mpx_warp_phase_rows).
        # Measured on configs[2] (round 6, bench.py configs2.analysis_one_kernel): HBM traffic of the analysis side 2.87 ->
        # 0.37 GB, no 1.4 GB of staged rows -- and 1.38 ms instead of 0.98: opt-in.  (The filter-bank magnitudes take the
        # logarithm AFTER the product: staged only.)
        self.fused_cr = (fusable and b_const_rate and self.phase_on_rows and self._warp_name != "mpx_mel_warp_fbank"
                         and self.total_out_frames > 0 and int(e.lib.mpx_analysis_compressed_fused_waves()) == 8
                         and int(e.lib.mpx_analysis_compressed_fused_layout()) == 1
                         and os.environ.get("MAGPHASE_COMP_FUSED_CR", "0") == "1")
        self._cr_work = None
        if self.fused or self.fused_cr:
            nw = int(e.lib.mpx_analysis_compressed_fused_waves())
            layout = int(e.lib.mpx_analysis_compressed_fused_layout())   # fragment order this build of the kernel reads
            key = ("wpack", self._warp_name, int(mag_dim), int(k_full), int(phase_dim), H, float(alpha), float(a_ph), nw,
                   layout)
            if key not in e._tables:
                wm = (hm.warp_fbank_matrix(mag_dim, H, alpha) if self._warp_name == "mpx_mel_warp_fbank"
                      else hm.warp_matrix(mag_dim, H, alpha))
                wph = hm.warp_matrix(k_full, H, a_ph, nrows=phase_dim)
                wpack, whalf = hm.pack_warp_fused(wm, wph, N, n_waves=nw, layout=layout)
                e._tables[key] = (e.to_device(wpack, np.float32), e.to_device(whalf, np.float32))
            self.wpack, self.whalf = e._tables[key]

    def _phase_rows_tmp(self):
        """The two phase streams warped at the variable rate, allocated at the first run and kept."""
        if self._phase_tmp is None:
            e, shape = self.engine, (int(self.lossless.total_frames), self.phase_dim)
            self._phase_tmp = (e.empty(shape), e.empty(shape))
        return self._phase_tmp

    def run(self, feats=None, out=None, mark=None):
        e, pl, N = self.engine, self.lossless, int(self.fft_len)
        H = N // 2 + 1
        Fo, fbank = self.total_out_frames, 1 if self._warp_name == "mpx_mel_warp_fbank" else 0
        mark = mark or (lambda name: None)
        mark("start")
        # float64 transform: the warp's log / division amplify an fp32 FFT's noise on weak bins (magphase_f64.hip)
        precise = os.environ.get("MAGPHASE_COMP_ANALYSIS", "f64") != "f32"
        _wait_ready(pl)

        def outputs():   # called once per run, by the path taken: the staged path allocates its lossless rows first
            return out if out is not None else (e.empty((Fo, self.mag_dim)), e.empty((Fo, self.phase_dim)),
                                                e.empty((Fo, self.phase_dim)))

        if self.fused:   # (feats, the staged path's lossless feature buffers, are not used)
            out = outputs()
            e.launch("mpx_analysis_compressed_fused", N, e.tables_f64(N), pl.sig, pl.pos, pl.left, pl.right,
                     int(pl.total_frames), *e.hann_window_args(), self.wpack, self.whalf, self.mag_dim, self.phase_dim,
                     self.voi, fbank, out[0], out[1], out[2])
            mark("k_analysis_warp_fused")
            return out
        n_var = int(pl.total_frames)
        if self.fused_cr:
            out = outputs()
            self._phase_rows_tmp()
            if self._cr_work is None:
                nbytes = int(e.lib.mpx_analysis_compressed_fused_cr_work_bytes(N, n_var))
                self._cr_work = e.empty(((nbytes + 3) // 4,))
            e.launch("mpx_analysis_compressed_fused_cr", N, e.tables_f64(N), pl.sig, pl.pos, pl.left, pl.right, n_var,
                     *e.hann_window_args(), self.wpack, self.whalf, self.mag_dim, self.phase_dim, self.rows_in_use,
                     self.row0, self.row1, self.rowt, int(Fo), out[0], *self._phase_tmp, self._cr_work)
            mark("k_analysis_warp_fused_cr")
            e.launch("mpx_warp_phase_rows", int(Fo), self.phase_dim, *self._phase_tmp, self.row0, self.row1, self.rowt,
                     self.voi, out[1], out[2])
            mark("k_warp_phase_rows")
            return out
        # (the phase rows nobody reads -- rows_in_use == 0 -- are not written either)
        mag, real, imag = pl.run(out=feats, precise=precise, rows_in_use=self.rows_in_use if self.phase_on_rows else None)
        mark("k_analysis_f64" if precise else "k_analysis")
        out = outputs()
        warp = (Fo, H, mag, real, imag, self.row0, self.row1, self.rowt, self.w_mag, self.mag_dim, self.w_ph, self.phase_dim,
                self.voi, out[0], out[1], out[2], e.feat_ld(mag, real, imag))
        if self.phase_on_rows:
            e.launch("mpx_mel_warp_rows", *warp, fbank, n_var, self.rows_in_use, *self._phase_rows_tmp())
        else:
            e.launch(self._warp_name, *warp)
        mark("k_mel_warp_mfma")
        return out

    def check_differentiable(self):
        """What run_backward cannot take, said before any launch."""
        if self._warp_name == "mpx_mel_warp_fbank":
            raise NotImplementedError("the filter-bank magnitudes (b_mag_fbank_mel) have no backward pass")

    def run_backward(self, outs, grads, mark=None):
        """The gradient of a loss with respect to the batch's samples, float32 [total_smpls] (utterance u at the offset of
        its samples in self.lossless.sig), given outs = run()'s three matrices and grads = (dL/d m_mag_mel_log,
        dL/d m_real_mel, dL/d m_imag_mel): contiguous float32 matrices of their shapes, or None for an output nobody
        differentiated (not read, contributes zero).  DESIGN.md section 3.3j.
        The lossless rows are RECOMPUTED (the fused forward never wrote them, and nothing of size F x H is kept between the
        passes): self.lossless.run with the forward's precision and rows_in_use=None -- every row is written, also the phase
        rows the constant-rate forward leaves out: the lossless backward multiplies real / imag into its result even where
        the gradient is zero.  Then _warp_backward (at the constant rate through the row tables) and
        LosslessAnalysisPlan.run_backward."""
        self.check_differentiable()
        torch = _torch()
        e, pl = self.engine, self.lossless
        Fo, n_var, total = self.total_out_frames, int(pl.total_frames), int(pl.total_smpls)
        mark = mark or (lambda name: None)
        mark("start")
        _check_warp_grads(self, grads)
        if Fo == 0 or n_var == 0 or total == 0 or all(g is None for g in grads):
            return torch.zeros((total,), dtype=torch.float32, device=e.device)
        precise = os.environ.get("MAGPHASE_COMP_ANALYSIS", "f64") != "f32"
        rows = pl.run(precise=precise, rows_in_use=None)
        mark("rows")
        if self.b_const_rate:   # (rows_in_use is None under MAGPHASE_WARP_PHASE_ROWS=0: no tile is skipped)
            tabs, live = (self.row0, self.row1, self.rowt), self.rows_in_use
        else:
            tabs, live = None, self.voi
        g_rows = _warp_backward(self, outs, grads, rows, tabs, live, n_var, mark=mark)
        gsig = pl.run_backward(rows[0], rows[1], rows[2], g_rows)
        mark("k_analysis_lossless_bwd")
        return gsig


class FrameTable:
    """A frame table over a batch's signal buffer, as Engine.analysis_lossless_backward reads one -- the part of a
    LosslessAnalysisPlan that call uses, for a second table over the same samples: pos (int64) / left / right (int32) on the
    device, total_frames, total_smpls and backward_tables() -> (scratch_off device int64 [F + 1], scratch floats) of
    hostmath.analysis_backward_table, built from the host copies on the first call."""

    def __init__(self, engine, fft_len, pos, left, right, total_frames, total_smpls, host_tabs):
        self.engine, self.fft_len = engine, int(fft_len)
        self.pos, self.left, self.right = pos, left, right
        self.total_frames, self.total_smpls = int(total_frames), int(total_smpls)
        self._host_tabs, self._bwd = host_tabs, None

    def backward_tables(self):
        if self._bwd is None:
            _start, soff = hm.analysis_backward_table(*self._host_tabs, self.fft_len, self.total_smpls)
            self._bwd = (self.engine.to_device(soff, np.int64), int(soff[-1]))
        return self._bwd


class Type2AnalysisPlan:
    """
    analysis_lossless_type2 (magphase.py:2793-2866) for a batch of utterances with epochs, (v_sig, fs, v_pm_sec, v_voi),
    one fft_len.  A LosslessAnalysisPlan holds the signal and the one-period frame table (phase, f0, gain); this plan adds
    the two-period half lengths of the same epochs (hostmath.two_period_frame_bounds: the magnitude frames), the voicing
    of the gain and the float shifts of the unrounded epochs (hostmath.type2_shift).  Rows are those of the lossless plan:
    utterance u's output is rows frame_off[u] + 1 .. frame_off[u + 1] (the reference drops row 0).
    run(): k_analysis_f64 over the one-period frames (float64 transform: the mel warp of the compressed form reads the
    phase, as in analysis_compressed), k_analysis_f64 over the two-period frames into the same magnitude rows (magnitudes
    only: the phase rows keep the one-period values), k_frame_gain, k_true_envelope at 600 coefficients on those rows.
    """

    def __init__(self, engine, utts, fft_len=None):
        self.engine = e = engine
        utts = list(utts)
        self.lossless = pl = LosslessAnalysisPlan(engine, utts, fft_len=fft_len)
        N = self.fft_len = pl.fft_len
        self.fs = list(pl.fs)
        l2, r2, voi = [], [], []
        self.v_f0, self.v_shift, self.long_frame_lens = [], [], []
        for u, (_sig, fs, v_pm_sec, v_voi) in enumerate(utts):
            n = int(pl.n_smpls[u])
            pm_sec, vv = hm.clean_epochs(v_pm_sec, v_voi, check_len_smpls=n, fs=fs)
            pm = np.asarray(pl.v_pm[u], dtype=np.int64)
            if pm.size != vv.size:
                raise RuntimeError("Type2AnalysisPlan: %d epochs planned, %d cleaned" % (pm.size, vv.size))
            lft2, rgt2 = hm.two_period_frame_bounds(pm, n)
            # the reference's warnings: the even-epoch frames, the odd ones (both incl. row 0), then the one-period ones
            tot2 = lft2 + rgt2 + 1
            self.long_frame_lens.append([int(x) for x in np.concatenate((tot2[0::2], tot2[1::2])) if x > N]
                                        + list(pl.long_frame_lens[u]))
            l2.append(lft2), r2.append(rgt2), voi.append((vv == 1).astype(np.float32))
            self.v_f0.append(np.asarray(pl.v_f0[u], dtype=np.float64)[1:])
            self.v_shift.append(hm.type2_shift(pm_sec * fs))
        self.frame_off = np.asarray(pl.frame_off, dtype=np.int64)
        F = self.total_frames = int(pl.total_frames)
        cat = (lambda v, dt: np.concatenate(v).astype(dt) if v else np.zeros(0, dt))   # noqa: E731
        t = e.to_device_packed([("left2", cat(l2, np.int64), np.int32), ("right2", cat(r2, np.int64), np.int32),
                                ("voi", cat(voi, np.float32), np.float32),
                                ("mag_only", np.zeros(F, dtype=np.float32), np.float32)])
        self.left2, self.right2, self.voi, self.mag_only = t["left2"], t["right2"], t["voi"], t["mag_only"]
        self._host_lr2 = (cat(l2, np.int64), cat(r2, np.int64))   # (the backward pass' scratch table is built from them)
        self.ld = int(e.lib.mpx_spec_ld(N // 2 + 1))   # one row pitch for the analysis rows and the envelope

    def out_rows(self, u):
        """Rows of utterance u in run()'s outputs: (first, end)."""
        a, b = int(self.frame_off[u]), int(self.frame_off[u + 1])
        return min(a + 1, b), b

    def run(self, want_iters=False, forced_iters=None, gain_blocks_per_cu=0):
        """-> (env, real, imag, gain, iters): float32 device rows [F x H] (one row pitch, self.ld; see out_rows), float64
        device gain [F], int32 device passes per envelope row (want_iters / forced_iters) or None."""
        e, torch = self.engine, _torch()
        pl, N, F = self.lossless, self.fft_len, self.total_frames
        H = N // 2 + 1
        mag, real, imag, env = (e.empty((max(F, 1), self.ld)) for _ in range(4))
        gain = torch.empty(max(F, 1), dtype=torch.float64, device=e.device)
        iters = None
        if want_iters or forced_iters is not None:
            iters = torch.empty(max(F, 1), dtype=torch.int32, device=e.device)
        feats = (mag[:F, :H], real[:F, :H], imag[:F, :H])
        if F == 0:
            return env[:0, :H], feats[1], feats[2], gain[:0], (iters[:0] if iters is not None else None)
        pl.run(out=feats, precise=True)
        # the two-period magnitudes overwrite the one-period ones (stream order); rows_in_use = 0: no phase row written
        e.analysis_frames(N, pl.sig, pl.pos, self.left2, self.right2, out=feats, precise=True, rows_in_use=self.mag_only)
        w = e.constant(("true_env_w", N, TYPE2_ENV_NCOEFFS, 0.7),
                       lambda: hm.true_envelope_lifter(N, TYPE2_ENV_NCOEFFS, 0.7))
        forced = None
        if forced_iters is not None:   # (a device int32 tensor -- run(want_iters=True)'s own -- is taken as it is)
            forced = forced_iters.reshape(F) if _is_tensor(forced_iters) else \
                e.to_device(np.asarray(forced_iters, dtype=np.int32).reshape(F), np.int32)
        tk = torch.empty(1, dtype=torch.int32, device=e.device)
        e.launch("mpx_frame_gain", N, pl.sig, pl.pos, pl.left, pl.right, self.voi, F, gain, int(gain_blocks_per_cu))
        e.launch("mpx_true_envelope", N, e.tables(N), w, mag, self.ld, F, hm.TRUE_ENV_IN_TYPES.index("abs"),
                 TYPE2_ENV_THRES_DB, hm.TRUE_ENV_MAX_ITERS, env, self.ld, iters, forced, tk)
        del mag   # (stream-ordered: the allocator reuses the magnitude rows after the envelope)
        return env[:F, :H], feats[1], feats[2], gain[:F], iters

    def two_period_table(self):
        """The two-period frame table as a FrameTable for Engine.analysis_lossless_backward.  Truncated frames keep
        starts and ends non-decreasing, so hostmath.analysis_backward_table accepts the table."""
        if getattr(self, "_tab2", None) is None:
            pl = self.lossless
            _wait_ready(pl)
            tabs = getattr(pl, "_host_tabs", None)
            pos = tabs[0] if tabs is not None else pl.pos.cpu().numpy()
            self._tab2 = FrameTable(self.engine, self.fft_len, pl.pos, self.left2, self.right2, self.total_frames,
                                    pl.total_smpls, (pos,) + self._host_lr2)
        return self._tab2

    def check_differentiable(self):
        """What run_backward cannot take, said before any launch: nothing."""

    def run_backward(self, grads, iters, want_decisions=False):
        """The gradient of a loss with respect to the batch's samples, float32 [total_smpls], given grads = (dL/d env,
        dL/d real, dL/d imag) of run()'s three matrices -- float32 [total_frames x H] with unit column stride, or None for
        an output nobody differentiated -- and iters, run(want_iters=True)'s passes per envelope row.  DESIGN.md section
        3.3m.  Nothing of size F x H is kept between the passes: the two-period rows are recomputed into buffers of their
        own (all three: the magnitude gradient needs the phase rows of the two-period frames, which the forward never
        writes), k_true_envelope_bwd takes dL/d env to the two-period magnitudes, the lossless analysis' backward kernels
        take those over the table (pos, left2, right2) to the samples; the one-period rows are recomputed with every row
        written and the same kernels take (None, dL/d real, dL/d imag) over (pos, left, right); the two sample gradients
        are added.  Row 0 of every utterance, which the outputs drop, arrives with zero gradients.  want_decisions
        (tests): -> (gradient, the envelope kernel's decision words or None)."""
        e, torch = self.engine, _torch()
        pl, N, F = self.lossless, self.fft_len, self.total_frames
        H, total = N // 2 + 1, int(pl.total_smpls)
        for g in grads:
            if g is not None and (g.dtype != torch.float32 or tuple(g.shape) != (F, H) or g.stride(1) != 1):
                raise ValueError("run_backward: gradients must be float32 [%d x %d] with unit column stride" % (F, H))
        g_env, g_real, g_imag = grads
        gsig, dec = None, None
        if F == 0 or total == 0 or all(g is None for g in grads):
            return (torch.zeros((total,), dtype=torch.float32, device=e.device), None) if want_decisions else \
                torch.zeros((total,), dtype=torch.float32, device=e.device)
        if g_env is not None:
            _wait_ready(pl)
            rows2 = tuple(e.empty((F, self.ld))[:, :H] for _ in range(3))
            e.analysis_frames(N, pl.sig, pl.pos, self.left2, self.right2, out=rows2, precise=True, rows_in_use=None)
            r = e.true_envelope_backward(rows2[0], iters, g_env, H, "abs", TYPE2_ENV_NCOEFFS,
                                         want_decisions=want_decisions)
            g_mag2, dec = (r[0], r[1]) if want_decisions else (r, None)
            gsig = e.analysis_lossless_backward(N, self.two_period_table(), rows2[0], rows2[1], rows2[2],
                                                (g_mag2[:, :H], None, None))
        if g_real is not None or g_imag is not None:
            rows1 = tuple(e.empty((F, self.ld))[:, :H] for _ in range(3))
            pl.run(out=rows1, precise=True, rows_in_use=None)
            g1 = pl.run_backward(rows1[0], rows1[1], rows1[2], (None, g_real, g_imag))
            gsig = g1 if gsig is None else gsig + g1
        return (gsig, dec) if want_decisions else gsig


class Type2CompressedAnalysisPlan:
    """
    analysis_compressed_type2 (magphase.py:3123-3196): a Type2AnalysisPlan, then format_for_modelling's two warps on its
    device rows (mpx_mel_warp, alpha_phase = alpha), which read their input rows through row tables: at the variable
    rate every row but row 0 of each utterance, at const_rate_ms > 0 the rows and weights of the grid
    arange(step, pm[-1], step) over the float epochs cumsum(v_shift), f0 / voicing by hostmath._const_rate_f0_voi
    (hostmath.var_to_const_rate_batch).  The gain is interpolated on the host (float64, as the reference).
    """

    def __init__(self, engine, utts, fft_len=None, mag_dim=60, phase_dim=45, const_rate_ms=-1.0):
        self.engine = e = engine
        self.t2 = t2 = Type2AnalysisPlan(engine, utts, fft_len=fft_len)
        fs = self.fs = t2.fs[0] if t2.fs else None
        if t2.fs.count(fs) != len(t2.fs):
            raise ValueError("one sample rate per batch")
        N = self.fft_len = t2.fft_len
        H = N // 2 + 1
        self.mag_dim, self.phase_dim = int(mag_dim), int(phase_dim)
        self.const_rate_ms = float(const_rate_ms)
        alpha = hm.define_alpha(fs)
        cf, _ = hm.define_crossfade_params(fs)
        k_full = hm.get_num_full_mel_coeffs_from_num_phase_coeffs(cf, phase_dim, alpha, fs)
        self.w_mag = e.constant(("w_mag", self.mag_dim, H, float(alpha)), lambda: hm.warp_matrix(mag_dim, H, alpha))
        self.w_ph = e.constant(("w_ph", int(k_full), H, float(alpha), self.phase_dim),
                               lambda: hm.warp_matrix(k_full, H, alpha, nrows=phase_dim))
        self.const = self.const_rate_ms > 0.0
        spans = [t2.out_rows(u) for u in range(len(t2.v_f0))]
        self.grid = []
        if self.const:
            self.grid = [np.cumsum(s) for s in t2.v_shift]   # la.shift_to_pm (magphase.py:3130)
            row0, row1, rowt, self.f0_out, self.out_off = hm.var_to_const_rate_batch(
                t2.v_shift, t2.v_f0, [a for a, _b in spans], fs, self.const_rate_ms)
        else:   # every row but row 0 of each utterance, weight 0
            row0 = np.concatenate([np.arange(a, b, dtype=np.int64) for a, b in spans] or [np.zeros(0, np.int64)])
            row1, rowt, self.f0_out = row0, np.zeros(row0.size), list(t2.v_f0)
            self.out_off = np.concatenate(([0], np.cumsum([f.size for f in self.f0_out]))).astype(np.int64)
        self.total_out_frames = int(self.out_off[-1])
        self._rows_host = (np.asarray(row0), np.asarray(row1), np.asarray(rowt, dtype=np.float64))   # (backward pass)
        f0_cat = np.concatenate(self.f0_out) if self.f0_out else np.zeros(0)
        (self.row0, self.row1, self.rowt), d = _upload_rows(
            e, (row0, row1, rowt), head=[("voi", (f0_cat > 0).astype(np.float32), np.float32)])
        self.voi = d["voi"]

    def run(self, want_iters=False):
        """-> ((mag [Fo x mag_dim], real, imag [Fo x phase_dim]) float32 device, gain float64 device [F]: the type-2
        plan's rows, see Type2AnalysisPlan.out_rows); want_iters: the envelope's int32 device passes per row as a third
        result (what run_backward takes)."""
        outs, gain, iters = self._run(want_iters)
        return (outs, gain, iters) if want_iters else (outs, gain)

    def check_differentiable(self):
        """What run_backward cannot take, said before any launch: k_mel_warp_bwd produces the gradient of at most 64
        coefficient columns per job."""
        for name, d in (("mag_dim", self.mag_dim), ("phase_dim", self.phase_dim)):
            if int(d) > 64:
                raise NotImplementedError("%s = %d: the backward pass of the type-2 analysis takes at most 64 coefficient "
                                          "columns" % (name, int(d)))

    def run_backward(self, outs, grads, iters):
        """The gradient of a loss with respect to the batch's samples, float32 [total_smpls], given outs = run()'s three
        matrices, grads = (dL/d m_mag_mel_log, dL/d m_real_mel, dL/d m_imag_mel) as contiguous float32 matrices of their
        shapes or None, and iters = run(want_iters=True)'s pass counts.  The type-2 rows are recomputed
        with the forward's pass counts forced; _warp_backward, as in CompressedAnalysisPlan.run_backward, on the type-2 row
        tables (which the forward reads at either rate), the magnitude job against the envelope rows; then
        Type2AnalysisPlan.run_backward.  DESIGN.md section 3.3m."""
        self.check_differentiable()
        torch = _torch()
        e, t2 = self.engine, self.t2
        Fo, F, total = self.total_out_frames, int(t2.total_frames), int(t2.lossless.total_smpls)
        _check_warp_grads(self, grads)
        if Fo == 0 or F == 0 or total == 0 or all(g is None for g in grads):
            return torch.zeros((total,), dtype=torch.float32, device=e.device)
        rows = t2.run(forced_iters=iters)[:3]   # (env, real, imag)
        g_rows = _warp_backward(self, outs, grads, rows, (self.row0, self.row1, self.rowt), None, F, mask_nonfinite=True)
        return t2.run_backward(g_rows, iters)

    def _run(self, want_iters):
        e = self.engine
        H = self.fft_len // 2 + 1
        env, real, imag, gain, iters = self.t2.run(want_iters=want_iters)
        Fo = self.total_out_frames
        out = (e.empty((max(Fo, 1), self.mag_dim)), e.empty((max(Fo, 1), self.phase_dim)),
               e.empty((max(Fo, 1), self.phase_dim)))
        if Fo:
            e.launch("mpx_mel_warp", Fo, H, env, real, imag, self.row0, self.row1, self.rowt, self.w_mag, self.mag_dim,
                     self.w_ph, self.phase_dim, self.voi, out[0], out[1], out[2], e.feat_ld(env, real, imag))
        return tuple(o[:Fo] for o in out), gain, iters
