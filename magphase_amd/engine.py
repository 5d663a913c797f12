"""
Device plumbing for the HIP hot path: PyTorch-ROCm tensors are the allocator/stream provider, every
computation is a libmagphase_hip.so call (ctypes, include/magphase_hip.h; Engine.launch is the one place that makes
one).  One Engine per GPU/process.  The batch plans that drive it are in plans.py, the host arithmetic they rest on in
hostmath.py / hostplan.py; their names are re-exported at the end of this module.

Data layout in HBM (all float32, row-major):
  sig      [sum_u n_u]          PCM of the batch's utterances, concatenated
  pos/left/right [F_tot]        per-frame epoch index into sig (int64) and Hann half lengths (int32)
  mag/real/imag  [F_tot x H]    lossless features, H = N/2+1 (same layout as the reference's arrays)
  frames   [F_tot x N]          epoch-centred time-domain frames (scratch between IFFT and PSOLA)
  pcm_out  [sum_u len_u]        resynthesised PCM, concatenated
"""
import ctypes
import os

import numpy as np

from . import _lib, hostmath as hm, hostplan


def _torch():
    import torch

    return torch


class HostTicket:
    """A batch result that is still on its way to the host: views of a page-locked ring slot filled by a non-blocking
    D2H copy.  wait() blocks until the copy has landed (releases the GIL: meant for the writer thread of iobatch),
    release() hands the slot back to the ring once the views have been consumed."""

    def __init__(self, ring, slot, event, keep):
        self._ring, self._slot, self._event, self._keep = ring, slot, event, keep

    def wait(self):
        if self._event is not None:
            self._event.synchronize()
            self._event = self._keep = None

    def release(self):
        if self._ring is not None:
            self.wait()
            self._ring.release(self._slot)
            self._ring = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class _PinnedRing:
    """A few page-locked host buffers (grown on demand, never shrunk).  A slot is reusable after its ticket's release();
    acquire() takes ANY free slot (a queue of free slots: two concurrent acquirers can never get the same one) and waits
    for one when the writer is behind -- the natural back-pressure of the pipeline.  If none comes free within
    MAGPHASE_RING_WAIT_S (default 20 s: e.g. a batch that needs more tickets at once than there are slots) it returns
    (None, None) and the caller falls back to a synchronous copy instead of stalling."""

    def __init__(self, slots=4):
        import queue
        import threading

        self._bufs = [None] * slots
        # SimpleQueue: release() runs from HostTicket.__del__, i.e. possibly from the cyclic GC while this very thread
        # is inside get() / put() -- queue.Queue's mutex is not reentrant (deadlock), SimpleQueue.put() is documented
        # safe from destructors and weakref callbacks
        self._freeq = queue.SimpleQueue()
        for k in range(slots):
            self._freeq.put(k)
        self._lock = threading.Lock()

    def acquire(self, nbytes, timeout=None):
        import queue

        torch = _torch()
        if timeout is None:
            timeout = float(os.environ.get("MAGPHASE_RING_WAIT_S", "20"))
        try:
            slot = self._freeq.get(timeout=timeout)
        except queue.Empty:
            return None, None
        try:
            with self._lock:
                buf = self._bufs[slot]
                if buf is None or buf.numel() < nbytes:
                    # Page-locking is slow (about 60 ms per 24 MB here): every slot is sized by the largest request so far
                    # with headroom, and a request that outgrows the slots re-sizes ALL the free ones at once -- the first
                    # (warm-up) launch of a job with larger launches pays, once, instead of each of the next launches paying
                    # for its own slot inside the job (round 5: bench.py's corpus shard ran at 2/3 of its warm rate because
                    # the slots sized by the earlier blocks re-grew one per launch).
                    size = max([int(nbytes * 1.25), 1 << 20] + [b.numel() for b in self._bufs if b is not None])
                    self._bufs[slot] = buf = torch.empty(size, dtype=torch.uint8).pin_memory()
                    idle = []
                    while True:   # the slots nobody holds right now
                        try:
                            idle.append(self._freeq.get_nowait())
                        except queue.Empty:
                            break
                    try:
                        for k in idle:
                            if self._bufs[k] is None or self._bufs[k].numel() < size:
                                self._bufs[k] = torch.empty(size, dtype=torch.uint8).pin_memory()
                    finally:
                        for k in idle:
                            self._freeq.put(k)
        except BaseException:
            self._freeq.put(slot)
            raise
        return slot, buf

    def release(self, slot):
        self._freeq.put(slot)


class Engine:
    def __init__(self, device=None):
        torch = _torch()
        self.lib = _lib.load()  # raises if the HIP library is missing: no fallback
        if not torch.cuda.is_available():
            raise _lib.MagphaseHipError("magphase_amd needs a ROCm GPU (torch.cuda.is_available() is False); "
                                        "there is no CPU fallback")
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        self._tables = {}

    # ------------------------------------------------------------------ helpers
    def stream_ptr(self):
        return _torch().cuda.current_stream(self.device).cuda_stream

    def launch(self, name, *args):
        """The C entry point `name` on this engine's device and current stream: self.lib.<name>(stream, *args), tensors
        passed as their pointers (data_ptr), None and scalars as they are; a non-zero return raises MagphaseHipError
        labelled `name`.  Every stream-taking mpx_* call goes through here.  (A run() that queues several launches pays a
        device guard and a stream lookup per launch: measured against one guard per run() and against the parent in
        profiles/r09_engine_split_ab.txt -- the three are not told apart.)"""
        tensor = _torch().Tensor
        with _torch().cuda.device(self.device):
            rc = getattr(self.lib, name)(self.stream_ptr(), *[a.data_ptr() if isinstance(a, tensor) else a for a in args])
        if rc != 0:
            _lib.check(rc, name)

    def background(self, fn, *args):
        """fn(*args) on the engine's helper thread -> Future (result() re-raises).  For the native, GIL-free host passes of a
        plan build (staging copies into page-locked memory): they run while the constructor goes on with its index
        arithmetic, and are joined before the upload.  MAGPHASE_HOST_THREAD=0: inline."""
        import concurrent.futures as cf

        if os.environ.get("MAGPHASE_HOST_THREAD", "1") == "0":
            f = cf.Future()
            try:
                f.set_result(fn(*args))
            except BaseException as exc:   # noqa: B902 -- delivered by result(), as the threaded form does
                f.set_exception(exc)
            return f
        ex = getattr(self, "_helper", None)
        if ex is None:
            ex = self._helper = cf.ThreadPoolExecutor(max_workers=1, thread_name_prefix="mpx-host")
        return ex.submit(fn, *args)

    def copy_stream(self, kind):
        """The engine's H2D ('up') / D2H ('down') stream, or None (MAGPHASE_COPY_STREAMS=0: copies in the compute stream).
        A corpus job's launches are device-bound, and a third of a launch's device time was its own PCIe traffic queued
        in front of / behind its kernels (30 MB of PCM or 17 MB of coefficients up, 15 MB of PCM down): on their own
        streams the next launch's upload and the previous launch's download run beside this launch's kernels -- the
        host builds plans ahead of the device, so the uploads are there to be overlapped."""
        if os.environ.get("MAGPHASE_COPY_STREAMS", "1") == "0":
            return None
        cs = getattr(self, "_copy_streams", None)
        if cs is None:
            torch = _torch()
            cs = self._copy_streams = {"up": torch.cuda.Stream(self.device), "down": torch.cuda.Stream(self.device)}
        if kind == "rng" and os.environ.get("MAGPHASE_RNG_STREAM", "1") == "0":
            return None          # the noise generator's kernels in the compute stream (measured: generation -10 %)
        if kind not in cs:   # "rng": the noise stream's generator kernels (a few workgroups each: numpy_global_uniform)
            cs[kind] = _torch().cuda.Stream(self.device)
        return cs[kind]

    def _download(self, pairs):
        """pairs: [(pinned host tensor view, device tensor)]: non-blocking D2H copies on the download stream, behind
        what the compute stream has queued so far.  Returns the event that marks their completion."""
        torch = _torch()
        cur = torch.cuda.current_stream(self.device)
        down = self.copy_stream("down")
        if down is None:
            for dst, src in pairs:
                dst.copy_(src, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(cur)
            return ev
        ready = torch.cuda.Event()
        ready.record(cur)
        with torch.cuda.stream(down):
            down.wait_event(ready)
            for dst, src in pairs:
                dst.copy_(src, non_blocking=True)
                src.record_stream(down)
            ev = torch.cuda.Event()
            ev.record(down)
        return ev

    def empty(self, shape, dtype=None):
        torch = _torch()
        return torch.empty(shape, dtype=dtype or torch.float32, device=self.device)

    def empty_feats(self, n_frames, n_bins, ld=None):
        """
        One lossless feature matrix [n_frames x n_bins] float32 on the device, as a VIEW of a buffer whose rows are
        `ld` floats apart (default mpx_feat_ld(): the dense layout, measured fastest; MAGPHASE_FEAT_LD overrides it
        for experiments).  .stride(0) is the `ld` the C entry points take.
        """
        ld = int(ld or os.environ.get("MAGPHASE_FEAT_LD", 0) or self.lib.mpx_feat_ld(2 * (int(n_bins) - 1)) or n_bins)
        return self.empty((int(n_frames), ld))[:, :int(n_bins)]

    def feats_cat_to_device(self, parts, n_bins):
        """List of host [F_u x n_bins] arrays (float64 or float32) -> ONE dense device float32 matrix [sum F_u x n_bins]:
        narrowed / copied into the page-locked staging buffer by a few native threads (numpy's float64 -> float32 cast
        is one thread), then one DMA.  Returns None when the engine's feature pitch is not the dense one."""
        H = int(n_bins)
        if int(os.environ.get("MAGPHASE_FEAT_LD", 0) or self.lib.mpx_feat_ld(2 * (H - 1)) or H) != H:
            return None
        rows = [int(np.shape(p)[0]) for p in parts]
        total = int(sum(rows)) * H
        if total == 0 or total > (128 << 20):   # more than 512 MB per stream: not worth page-locking, the plain path does it
            return None
        stage = self.host_staging(total)
        n_thr = self.host_threads(4 * total, big=16)
        off = 0
        for p_, r in zip(parts, rows):
            a = np.asarray(p_)
            if a.ndim != 2 or a.shape[1] != H:
                raise ValueError("feature matrices must be [frames x %d]" % H)
            if a.dtype == np.float64 and a.flags.c_contiguous:
                if self.lib.mpx_host_narrow_f64(a.ctypes.data, stage[off:off + r * H].ctypes.data, r * H, n_thr) != 0:
                    raise _lib.MagphaseHipError("mpx_host_narrow_f64 failed")
            else:
                stage[off:off + r * H] = a.reshape(-1)
            off += r * H
        return self.upload_staged(total).view(int(sum(rows)), H)

    def feats_to_device(self, arr):
        """Host [F x H] array -> device float32 matrix (see empty_feats)."""
        torch = _torch()
        arr = np.ascontiguousarray(arr, dtype=np.float32)
        out = self.empty_feats(arr.shape[0], arr.shape[1])
        out.copy_(torch.from_numpy(arr))
        return out

    # ------------------------------------------------------------------ pinned staging
    def _pinned_ring(self, n_floats, depth):
        """`depth` page-locked float32 staging buffers of at least n_floats elements (grown on demand, kept)."""
        torch = _torch()
        cur = getattr(self, "_pinned", None)
        if cur is None or len(cur) < depth or cur[0].numel() < n_floats:   # grown with headroom: page-locking is slow
            n_alloc = max(int(n_floats * 1.5), 1 << 20)
            self._pinned = tuple(torch.empty(n_alloc, dtype=torch.float32).pin_memory() for _ in range(depth))
        return self._pinned

    def to_host_f64_many(self, tensors, chunk_bytes=None, depth=3):
        """
        Device float32 tensors (1-D or 2-D, rows may be pitched) -> fresh float64 numpy arrays through a ring of pinned
        staging buffers: the chunks of ALL tensors form one pipeline -- chunks i+1, i+2 cross PCIe (async copies on the
        current stream) while the host widens chunk i to float64 (native threads, streaming stores).  One matrix at a
        time with two 64 MB chunks each, the three feature matrices of a batch paid the pipeline's fill and drain
        three times (12 of a call's 16 ms); as one stream of 16 MB chunks the copies hide behind the widening.
        Bounded pinned memory (depth x chunk_bytes) whatever the sizes.
        """
        torch = _torch()
        # the widening writes 2 bytes for every byte that crosses PCIe: eight threads sustain ~75 GB/s of streaming stores on
        # this host, half of what the link delivers (round 6: 16 utterances' features 14 ms for 0.35 GB); 32 threads from
        # 16 MB up (Engine.host_threads: capped by the cores this rank may use)
        # (tools/array_api_probe.py, 16 utterances: 8 / 16 / 32 / 64 threads = 0.54 / 0.73 / 0.64 / 0.63 M frames/s)
        n_thr = self.host_threads(sum(int(t.numel()) * 4 for t in tensors), big=16)
        if chunk_bytes is None:
            chunk_bytes = int(os.environ.get("MAGPHASE_D2H_CHUNK_MB", "32")) << 20
        outs, views, work = [], [], []
        for k, t in enumerate(tensors):
            v = t.view(1, -1) if t.dim() == 1 else t
            rows, cols = int(v.shape[0]), int(v.shape[1])
            out = np.empty((rows, cols), dtype=np.float64)
            outs.append(out.reshape(-1) if t.dim() == 1 else out)
            views.append((v, out, cols))
            if rows and cols:
                rows_per = max(1, int(chunk_bytes) // (4 * cols))
                work.extend((k, r0, min(rows, r0 + rows_per)) for r0 in range(0, rows, rows_per))
        if not work:
            return outs
        biggest = max((r1 - r0) * views[k][2] for k, r0, r1 in work)
        bufs = self._pinned_ring(biggest, depth)
        events = [torch.cuda.Event() for _ in range(depth)]

        def drain(i):
            k, r0, r1 = work[i]
            _v, out, cols = views[k]
            events[i % depth].synchronize()
            if self.lib.mpx_host_widen_f32(bufs[i % depth].data_ptr(), out[r0:r1].ctypes.data, (r1 - r0) * cols, n_thr) != 0:
                raise _lib.MagphaseHipError("mpx_host_widen_f32 failed")

        with torch.cuda.device(self.device):
            for i, (k, r0, r1) in enumerate(work):
                if i >= depth:
                    drain(i - depth)                  # the buffer about to be overwritten
                v, _out, cols = views[k]
                bufs[i % depth][:(r1 - r0) * cols].view(r1 - r0, cols).copy_(v[r0:r1], non_blocking=True)
                events[i % depth].record()
            for i in range(max(0, len(work) - depth), len(work)):
                drain(i)
        return outs

    def to_host_f64(self, t, chunk_bytes=None):
        """One tensor through to_host_f64_many."""
        return self.to_host_f64_many([t], chunk_bytes=chunk_bytes)[0]

    def to_host_f32(self, t):
        """Device float32 tensor (rows may be pitched) -> fresh float32 numpy array (one D2H copy into a new pageable
        array: for the megabyte-sized compressed features that beats staging + a second host copy)."""
        torch = _torch()
        dst = torch.empty(tuple(int(x) for x in t.shape), dtype=torch.float32)
        if dst.numel():
            with torch.cuda.device(self.device):
                dst.copy_(t)
        return dst.numpy()

    def out_ring(self):
        r = getattr(self, "_out_ring", None)
        if r is None:
            r = self._out_ring = _PinnedRing(slots=max(2, int(os.environ.get("MAGPHASE_OUT_RING_SLOTS", "4"))))
        return r

    def to_host_f32_async(self, tensors):
        """Device float32 tensors -> float32 numpy VIEWS of one page-locked ring slot, copied without blocking; returns
        (views, HostTicket).  The views are valid after ticket.wait() and until ticket.release()."""
        torch = _torch()
        sizes = [int(t.numel()) for t in tensors]
        offs = np.concatenate(([0], np.cumsum([(n + 63) // 64 * 64 for n in sizes]))).astype(np.int64)
        slot, buf = self.out_ring().acquire(4 * int(offs[-1]) + 256)
        if slot is None:   # ring exhausted: plain synchronous copies, a ticket with nothing to wait for
            return [t.detach().to("cpu").numpy() for t in tensors], HostTicket(None, None, None, None)
        try:
            host = buf[:4 * int(offs[-1])].view(torch.float32)
            views, pairs = [], []
            with torch.cuda.device(self.device):
                for t, n, o in zip(tensors, sizes, offs[:-1]):
                    dst = host[int(o):int(o) + n].view(tuple(int(x) for x in t.shape))
                    if n:
                        pairs.append((dst, t))
                    views.append(dst.numpy())
                ev = self._download(pairs)
        except BaseException:
            self.out_ring().release(slot)   # a failed copy must not leak the slot
            raise
        return views, HostTicket(self.out_ring(), slot, ev, list(tensors))

    def output_pcm16(self, y, out_off_host, norm=0.98, async_out=False, return_device=False):
        """
        libaudio.py:352-365 on the device (mpx_pcm16): y float64 or float32 [total] (utterances at out_off_host) ->
        int16 numpy [total], each utterance peak-normalised to `norm` (None: no normalisation) and rounded like
        libsndfile's PCM_16 conversion -- bit-identical to la.write_audio_file's samples.
        async_out: returns (view of a page-locked ring slot, HostTicket) without waiting for the copy.
        return_device: stops before the download -- the int16 device tensor [total].
        """
        torch = _torch()
        out_off_host = np.asarray(out_off_host, dtype=np.int64)
        lens = np.diff(out_off_host)
        total = int(out_off_host[-1])
        d_off = self.to_device(out_off_host, np.int64)
        peaks = torch.empty(max(lens.size, 1), dtype=torch.float64, device=self.device)
        out = torch.empty(max(total, 1), dtype=torch.int16, device=self.device)
        self.launch("mpx_pcm16", y, 1 if y.dtype == torch.float64 else 0, d_off, int(lens.size),
                    int(lens.max()) if lens.size else 0, float(norm) if norm is not None else 0.0, peaks, out)
        if return_device:
            return out[:total]
        with torch.cuda.device(self.device):
            if async_out:   # non-blocking copy into a page-locked ring slot; the consumer waits on the ticket
                slot, buf = self.out_ring().acquire(2 * max(total, 1))
                if slot is not None:
                    try:
                        host = buf[:2 * max(total, 1)].view(torch.int16)
                        ev = self._download([(host, out)])
                    except BaseException:
                        self.out_ring().release(slot)
                        raise
                    return host[:total].numpy(), HostTicket(self.out_ring(), slot, ev, [out, peaks, d_off])
                host = torch.empty(max(total, 1), dtype=torch.int16)   # ring exhausted: synchronous copy
                host.copy_(out)
                return host[:total].numpy(), HostTicket(None, None, None, None)
            # one D2H copy into a fresh pageable array (pinning a new 15-30 MB buffer per batch cost 7 ms, more than the copy)
            host = torch.empty(max(total, 1), dtype=torch.int16)
            host.copy_(out)
        return host[:total].numpy()

    @staticmethod
    def _mt_next_pos(pos, n_words):
        """Position of numpy's MT19937 word cursor (0..624) after n_words more 32-bit draws (randomkit: a draw at 624
        regenerates the state and restarts at 0)."""
        q = int(pos) + int(n_words)
        return q if (n_words == 0 or q <= 624) else ((q - 1) % 624) + 1

    def _mt_generate(self, key, pos, n, key_from_compute, with_raw=False):
        """n uniforms continuing numpy's MT19937 stream from (key [624 words on the device], word cursor pos), on the
        generator's own stream: (samples float32 [n], state int32 [625] = key + cursor after them, event).
        with_raw: the generator's raw words (int32 [2 n], two per sample) as a fourth element instead of dropping them.
        key_from_compute: the key was just uploaded in the compute stream (the generator's stream waits for it; a state
        that comes from the generator's own stream needs no wait -- and must not get one: waiting for the compute stream here
        is waiting for the previous launch)."""
        torch = _torch()
        # The generator's kernels are a ladder of launches of 1 .. 128 workgroups: they run on their own stream, beside
        # whatever the compute stream has queued (the previous launch's synthesis), one generation after the other; the
        # compute stream waits for the samples' event where it uses them.
        rng = self.copy_stream("rng")
        done = None
        with torch.cuda.device(self.device):
            cur = torch.cuda.current_stream(self.device)
            if rng is not None:
                ready = None
                if key_from_compute:
                    ready = torch.cuda.Event()
                    ready.record(cur)
                ctx = torch.cuda.stream(rng)
            else:
                import contextlib
                ctx = contextlib.nullcontext()
            with ctx:
                if rng is not None and ready is not None:
                    rng.wait_event(ready)
                out = self.empty((max(int(n), 1),))
                raw = torch.empty(max(2 * int(n), 1), dtype=torch.int32, device=self.device)
                state = torch.empty(625, dtype=torch.int32, device=self.device)
                work = getattr(self, "_mt_work", None)
                if work is None:   # segment windows + jump polynomials of the many-workgroup form
                    work = self._mt_work = torch.empty(int(self.lib.mpx_noise_numpy_mt19937_work_words()),
                                                       dtype=torch.int32, device=self.device)
                self.launch("mpx_noise_numpy_mt19937", key, int(pos), int(n), raw, out, state, state.data_ptr() + 4 * 624,
                            work)
                if rng is not None:
                    done = torch.cuda.Event()
                    done.record(rng)
                    for t_ in (key,):
                        t_.record_stream(rng)
        if with_raw:
            return out, state, done, raw
        return out, state, done

    def numpy_global_uniform(self, n, defer=False):
        """np.random.uniform(-1, 1, n).astype(float32) drawn from numpy's global generator, on the device
        (mpx_noise_numpy_mt19937): same values, and the global state is left where the host draw would leave it.
        defer=True (the batches of a corpus run, iobatch): the advanced state STAYS on the device and the next deferred
        call continues from it -- no download, no synchronisation per batch; numpy's own state is stale until mt_sync(),
        which the caller owes before anything else draws from it.  Deferred draws can be generated AHEAD
        (MAGPHASE_MT_AHEAD = k: k requests' worth per generation; a call that finds its samples in what an earlier call
        produced launches nothing; mt_sync() puts numpy's state where the samples actually HANDED OUT end).  Measured in
        round 6 on the generation workload: no gain (k = 4 / 8: 118-160 / 108-146 k x real time against 133-170 k at k = 1
        on the same box -- the larger draws' allocations and copies cost what the saved jump ladders gain), so k = 1."""
        torch = _torch()
        n = int(n)
        pend = getattr(self, "_mt_pending", None)
        fresh = pend is None
        if fresh:
            st = np.random.get_state()
            if st[0] != "MT19937":
                raise RuntimeError("numpy's global generator is not MT19937")
            key = self.to_device(np.ascontiguousarray(st[1], dtype=np.uint32).view(np.int32), np.int32)
            pend = {"key": key, "pos": int(st[2]), "meta": (st[0], st[3], st[4]), "buf": None, "gen": 0, "lead": 0, "used": 0,
                    "end_state": None, "end_pos": int(st[2]), "done": None}
        with torch.cuda.device(self.device):
            cur = torch.cuda.current_stream(self.device)
            if pend["buf"] is not None and pend["used"] + n <= pend["gen"]:      # already generated
                out = pend["buf"][pend["used"]:pend["used"] + n]
                pend = dict(pend, used=pend["used"] + n)
            else:
                left = pend["gen"] - pend["used"] if pend["buf"] is not None else 0
                ahead = max(1, int(os.environ.get("MAGPHASE_MT_AHEAD", "1"))) if defer else 1
                n_gen = max(n - left, ahead * n - left, 0)
                if pend["buf"] is not None:      # continue where the generated samples end
                    key, pos, from_compute = pend["end_state"], pend["end_pos"], False
                else:
                    key, pos, from_compute = pend["key"], pend["pos"], fresh
                gen, state, done = self._mt_generate(key, pos, n_gen, from_compute)
                if left:     # the unused tail of the previous generation in front of the new samples: one contiguous draw
                    rng = self.copy_stream("rng")
                    buf = self.empty((left + n_gen,))
                    ctx = torch.cuda.stream(rng) if rng is not None else None
                    if ctx is not None:
                        ctx.__enter__()
                    try:
                        buf[:left].copy_(pend["buf"][pend["used"]:pend["gen"]])
                        buf[left:].copy_(gen[:n_gen])
                        if rng is not None:
                            done = torch.cuda.Event()
                            done.record(rng)
                            buf.record_stream(rng)
                    finally:
                        if ctx is not None:
                            ctx.__exit__(None, None, None)
                else:
                    buf = gen
                pend = {"key": key, "pos": int(pos), "meta": pend["meta"], "buf": buf, "gen": left + n_gen, "lead": left,
                        "used": n, "end_state": state, "end_pos": self._mt_next_pos(pos, 2 * n_gen), "done": done}
                out = buf[:n]
            if pend["done"] is not None:
                cur.wait_event(pend["done"])       # everything the caller enqueues from here on sees the samples
                pend["buf"].record_stream(cur)
        self._mt_pending = pend
        if not defer:
            self.mt_sync()
        return out

    # words of at most this many samples are resident at a time when Griffin-Lim's 'random' initial phases are drawn on the
    # device (magphase.griffin_lim_batch(fold='device')): 2^27 samples = 1 GiB of raw words (+ 0.5 GiB of the float32
    # samples the generator's entry writes beside them)
    GL_WORDS_GROUP_SAMPLES = 1 << 27

    def numpy_global_words(self, n, defer=False):
        """The raw MT19937 words of np.random.rand's next n samples (int32 [2 n] on the device, two per sample: the `raw`
        buffer of mpx_noise_numpy_mt19937), numpy's global stream continued on the device as numpy_global_uniform does:
        the global state is left where n host draws would leave it, a pending deferred state is continued (samples that
        were generated ahead and not handed out are given up first: mt_sync), and with defer=True the advanced state
        stays on the device until mt_sync().  The words are ready on torch's current stream of the device."""
        torch = _torch()
        n = int(n)
        pend = getattr(self, "_mt_pending", None)
        if pend is not None and (pend["buf"] is None or pend["used"] != pend["gen"]):
            self.mt_sync()   # (numpy's state where the handed-out samples end; the words continue from there)
            pend = None
        if pend is None:
            st = np.random.get_state()
            if st[0] != "MT19937":
                raise RuntimeError("numpy's global generator is not MT19937")
            key = self.to_device(np.ascontiguousarray(st[1], dtype=np.uint32).view(np.int32), np.int32)
            pos, meta, fresh = int(st[2]), (st[0], st[3], st[4]), True
        else:
            key, pos, meta, fresh = pend["end_state"], pend["end_pos"], pend["meta"], False
        gen, state, done, raw = self._mt_generate(key, pos, n, fresh, with_raw=True)
        with torch.cuda.device(self.device):
            cur = torch.cuda.current_stream(self.device)
            if done is not None:
                cur.wait_event(done)
                raw.record_stream(cur)
        self._mt_pending = {"key": key, "pos": pos, "meta": meta, "buf": gen, "gen": n, "lead": 0, "used": n,
                            "end_state": state, "end_pos": self._mt_next_pos(pos, 2 * n), "done": done}
        if not defer:
            self.mt_sync()
        return raw[:2 * n]

    def mt_sync(self):
        """Puts a deferred MT19937 state (numpy_global_uniform(defer=True)) back into numpy's global generator: the state
        after the samples handed out so far (samples generated ahead and not handed out are dropped)."""
        pend = getattr(self, "_mt_pending", None)
        if pend is None:
            return
        self._mt_pending = None
        if pend["buf"] is None:
            return
        used_gen, total_gen = pend["used"] - pend["lead"], pend["gen"] - pend["lead"]
        if used_gen < 0:
            raise RuntimeError("MT19937: cursor inside the carried-over samples")
        if used_gen == total_gen:
            state, pos = pend["end_state"], pend["end_pos"]
        else:      # numpy's state where the handed-out samples end: the generation repeated up to there (once per job)
            _g, state, _d = self._mt_generate(pend["key"], pend["pos"], used_gen, False)
            pos = self._mt_next_pos(pend["pos"], 2 * used_gen)
        torch = _torch()
        with torch.cuda.device(self.device):
            rng = self.copy_stream("rng")
            if rng is not None:
                rng.synchronize()
            h = state.cpu().numpy()          # synchronises
        if int(h[624]) != int(pos):
            raise RuntimeError("MT19937 cursor: host %d, device %d" % (pos, int(h[624])))
        meta = pend["meta"]
        np.random.set_state((meta[0], h[:624].view(np.uint32).copy(), int(pos), meta[1], meta[2]))

    def mt_snapshot(self):
        """Opaque copy of the generator's current state (deferred device state or numpy's), for mt_restore.  (The device
        tensors of a deferred state are never written again once generated: the snapshot shares them.)"""
        pend = getattr(self, "_mt_pending", None)
        if pend is not None:
            return ("dev", dict(pend))
        return ("host", np.random.get_state())

    def mt_restore(self, snap):
        kind, val = snap
        if kind == "dev":
            self._mt_pending = dict(val)
        else:
            self._mt_pending = None
            np.random.set_state(val)

    def host_staging(self, n_floats):
        """float32 numpy view [n_floats] of a page-locked staging buffer (grown on demand, reused by every plan).  TWO
        buffers alternate: the DMA out of one (upload_staged, not waited for) runs while the host fills the other for the
        next plan; a buffer is waited for only when its turn comes again.  Always paired with upload_staged, one thread."""
        torch = _torch()
        st = getattr(self, "_stage", None)
        if st is None:
            st = self._stage = {"bufs": [None, None], "events": [None, None], "cur": 1}
        k = st["cur"] = 1 - st["cur"]
        if st["events"][k] is not None:
            st["events"][k].synchronize()
            st["events"][k] = None
        cur = st["bufs"][k]
        if cur is None or cur.numel() < n_floats:   # grown with headroom (batches of a corpus differ a little in length:
            # re-pinning 30 MB for every slightly longer batch cost 40 ms each); the OTHER buffer grows with it when it is
            # idle, so that the second launch of a job does not pay for it inside the job
            size = max(int(n_floats * 1.5), 1 << 22)
            st["bufs"][k] = cur = torch.empty(size, dtype=torch.float32).pin_memory()
            o = 1 - k
            if (st["bufs"][o] is None or st["bufs"][o].numel() < size) and (st["events"][o] is None or st["events"][o].query()):
                st["events"][o] = None
                st["bufs"][o] = torch.empty(size, dtype=torch.float32).pin_memory()
        self._stage_up = cur
        return cur.numpy()[:int(n_floats)]

    def stage_rows(self, arrays, out):
        """np.concatenate(arrays, axis=0, out=out, casting='same_kind') for a float32 ``out`` (a slice of the staging
        buffer): float32 C-contiguous blocks are copied, float64 ones narrowed (round to nearest even, as astype), both on
        a few native threads (mpx_host_copy_many / mpx_host_narrow_f64) -- numpy's concatenate is one thread at ~10 GB/s and
        was a quarter of a synthesis plan's build time.  Anything else goes through numpy."""
        # (launches of 100+ utterances stage tens of MB per matrix: 8 / 16 / 32 threads = 116 / 131 / 144 k x real time)
        n_thr = self.host_threads(out.nbytes)
        k = len(arrays)
        if k > 1 and all(a.dtype == np.float32 and a.flags.c_contiguous for a in arrays):
            src = (ctypes.c_void_p * k)(*[a.ctypes.data for a in arrays])
            nb = np.fromiter((a.nbytes for a in arrays), dtype=np.int64, count=k)
            doff = np.zeros(k, dtype=np.int64)
            np.cumsum(nb[:-1], out=doff[1:])
            if int(nb.sum()) != out.nbytes:
                raise ValueError("stage_rows: blocks do not fill the destination")
            if self.lib.mpx_host_copy_many(k, src, nb.ctypes.data, doff.ctypes.data, out.ctypes.data, n_thr) != 0:
                raise _lib.MagphaseHipError("mpx_host_copy_many failed")
            return
        if k > 0 and all(a.dtype == np.float64 and a.flags.c_contiguous for a in arrays):
            flat, o = out.reshape(-1), 0
            if int(sum(a.size for a in arrays)) != flat.size:
                raise ValueError("stage_rows: blocks do not fill the destination")
            for a in arrays:
                if a.size and self.lib.mpx_host_narrow_f64(a.ctypes.data, flat[o:].ctypes.data, a.size, n_thr) != 0:
                    raise _lib.MagphaseHipError("mpx_host_narrow_f64 failed")
                o += a.size
            return
        np.concatenate(arrays, axis=0, out=out, casting="same_kind")

    def upload_staged(self, n_floats):
        """The first n_floats of the current staging buffer -> a fresh device tensor (one DMA from pinned memory, in
        stream order; the buffer is protected by an event until host_staging hands it out again)."""
        torch = _torch()
        st = self._stage
        up = self.copy_stream("up")
        with torch.cuda.device(self.device):
            if up is None:
                t = self._stage_up[:int(n_floats)].to(self.device, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(self.device))
            else:   # on the upload stream; the compute stream waits for it, the tensor is the compute stream's from then on
                cur = torch.cuda.current_stream(self.device)
                with torch.cuda.stream(up):
                    t = self._stage_up[:int(n_floats)].to(self.device, non_blocking=True)
                    ev = torch.cuda.Event()
                    ev.record(up)
                cur.wait_event(ev)
                t.record_stream(cur)
            st["events"][st["cur"]] = ev
        return t

    # ------------------------------------------------------------------ feature rows that are already on the device
    def is_device_rows(self, x):
        """True for a torch tensor that lives on this engine's device."""
        torch = _torch()
        return torch.is_tensor(x) and x.device == self.device

    def pack_rows(self, streams, outs):
        """
        The rows of a batch gathered into dense device matrices by ONE mpx_rows_pack launch (k_rows_pack): streams is a
        list (at most three) of per-utterance lists of [rows x width] tensors on this device -- float32 / float16 /
        bfloat16 / float64, any row stride (column slices of one wide tensor are read where they lie; a non-unit column
        stride is made contiguous first); outs the streams' float32 device matrices [sum of rows x width] (unit column
        stride, any row pitch: the `coef` slices of a compressed synthesis plan, empty_feats matrices).  Returns outs.
        Host arrays (or CPU tensors) among the utterances are uploaded one by one and packed with the rest: the slow
        mixed case -- a batch of host arrays belongs in stage_rows / upload_staged, one copy and one DMA.
        The launch goes to torch's current stream of the device, like every other: rows produced on that stream need no
        synchronisation.
        """
        torch = _torch()
        if len(streams) != len(outs):
            raise ValueError("pack_rows: one output per stream")
        dev = []
        for st in streams:
            row = []
            for t in st:
                if not self.is_device_rows(t):
                    if torch.is_tensor(t):
                        if t.device.type != "cpu":
                            raise ValueError("pack_rows: tensor on %s, the engine runs on %s" % (t.device, self.device))
                        t = t.detach()
                        t = (t.float() if t.dtype in (torch.float16, torch.bfloat16) else t).numpy()
                    a = np.atleast_2d(np.asarray(t))
                    t = self.to_device(a, np.float32) if a.size else self.empty(a.shape)
                elif t.dim() == 2 and t.shape[1] > 1 and t.stride(1) != 1:
                    t = t.contiguous()
                row.append(t.detach())
            dev.append(row)
        table, widths, rows = hm.rows_pack_table(dev)
        args = []
        for s, o in enumerate(outs):
            if (not self.is_device_rows(o) or o.dtype != torch.float32 or o.dim() != 2
                    or (o.shape[1] > 1 and o.stride(1) != 1)):
                raise ValueError("pack_rows: output %d must be a 2-D float32 matrix on %s with unit column stride"
                                 % (s, self.device))
            if int(o.shape[0]) != rows[s] or (rows[s] and int(o.shape[1]) != widths[s]):
                raise ValueError("pack_rows: output %d is %d x %d, its stream has %d rows of %d"
                                 % (s, o.shape[0], o.shape[1], rows[s], widths[s]))
            ld = max(int(o.stride(0)), int(o.shape[1])) if o.shape[0] > 1 else int(o.shape[1])
            args += [o, int(o.shape[1]), ld, rows[s]]
        args += [None, 0, 0, 0] * (3 - len(outs))
        if table.size and sum(rows):
            d_table = self.to_device(table.view(np.uint8), np.uint8)
            self.launch("mpx_rows_pack", d_table, table.ctypes.data, len(dev[0]), len(dev), *args)
        return outs

    def lf0_to_host(self, lf0s, what="v_lf0"):
        """The lf0 vectors of a batch as float64 numpy arrays.  Host arrays are converted as always; device tensors
        (float32 / bfloat16 / float64 -- float16 cannot hold the unvoiced marker -1e10) are widened to float64 on the
        device (exact) and come down in ONE copy: the values of tensor.double().cpu().numpy()."""
        torch = _torch()
        out = [None] * len(lf0s)
        idx = [k for k, v in enumerate(lf0s) if torch.is_tensor(v)]
        for k, v in enumerate(lf0s):
            if not torch.is_tensor(v):
                out[k] = np.atleast_1d(np.asarray(v, dtype=np.float64))
        if idx:
            for k in idx:
                hm.check_feature_tensor(lf0s[k], "%s of utterance %d" % (what, k), lf0=True)
                if lf0s[k].device != self.device and lf0s[k].device.type != "cpu":
                    raise ValueError("%s of utterance %d is on %s, the engine runs on %s"
                                     % (what, k, lf0s[k].device, self.device))
            ts = [lf0s[k].detach().reshape(-1) for k in idx]
            on_dev = [t for t in ts if t.device == self.device]
            if on_dev:
                with torch.cuda.device(self.device):
                    same = len(set(t.dtype for t in on_dev)) == 1
                    cat = torch.cat(on_dev).double() if same else torch.cat([t.double() for t in on_dev])
                    flat = cat.cpu().numpy()
            o = 0
            for k, t in zip(idx, ts):
                if t.device == self.device:
                    out[k] = flat[o:o + t.numel()]
                    o += t.numel()
                else:
                    out[k] = t.double().numpy()
        return out

    # ------------------------------------------------------------------ prepared launches (native planners, planner thread)
    def host_threads(self, nbytes=0, big=32):
        """Native threads one staging pass of `nbytes` may use: MAGPHASE_IO_NATIVE_THREADS, or 8 (32 from 16 MB up: launches of
        100+ utterances), never more than the cores this process may run on (sharding.bind_rank_to_cores gives every rank of
        a node its own share -- the reference's model is one worker per core with nothing shared, libutils.py:61-62)."""
        env = os.environ.get("MAGPHASE_IO_NATIVE_THREADS")
        want = int(env) if env else (int(big) if nbytes >= (16 << 20) else 8)
        try:
            cores = len(os.sched_getaffinity(0))
        except (AttributeError, OSError):
            cores = os.cpu_count() or 1
        return max(1, min(want, cores))

    # Staging slots.  A slot is held from prepare_* until the upload out of it has completed; a generation batch is TWO launches
    # (one per sample rate) and the planner works one batch ahead of the thread that enqueues, so four are in use at once: with
    # three (rounds 5-6) the planner thread waited for a slot in every batch, the enqueuing thread for the planner, and the
    # device for the upload -- 13-19 ms of a 45 ms generation pass (tools/corpus_marks_probe.py)
    _N_SLOTS = max(2, int(os.environ.get("MAGPHASE_STAGE_SLOTS", "6")))

    def _slot_acquire(self, stage_bytes, desc_bytes, wait=True):
        """One of the engine's sets of page-locked buffers (sample / coefficient staging + table image) for a prepared launch;
        blocks while all are in use (wait=False: returns None instead -- a plan constructor that prepares its own launch must
        not wait for slots that launches prepared AHEAD of it hold: they are committed after it).  A slot is handed out again
        only after the H2D copies out of it have completed."""
        import queue

        torch = _torch()
        pool = getattr(self, "_slots", None)
        if pool is None:
            import threading

            with self.__dict__.setdefault("_slots_lock", threading.Lock()):
                pool = getattr(self, "_slots", None)
                if pool is None:
                    # tokens in a SimpleQueue (blocking; safe to put from a destructor running inside the cyclic collector,
                    # unlike queue.Queue's mutex), the slots themselves on a stack: the most recently returned slot -- page-
                    # locked, sized, its event long since passed -- goes out first, so one launch at a time keeps reusing ONE
                    # warm slot instead of walking through all of them (each first use pins tens of MB: 40 ms)
                    import collections
                    pool = queue.SimpleQueue()
                    self._slot_stack = collections.deque()
                    for _ in range(self._N_SLOTS):
                        self._slot_stack.append({"stage": None, "desc": None, "event": None})
                        pool.put(None)
                    self._slots = pool
        try:
            pool.get(block=bool(wait))
        except queue.Empty:
            return None
        # the most recently returned slot whose upload has completed (warm, and free NOW); none: the oldest one
        slot = None
        with self._slots_lock:   # (two acquirers -- the planner thread and a caller on the generic path -- must not pick the same entry)
            for k in range(len(self._slot_stack) - 1, -1, -1):
                ev_ = self._slot_stack[k]["event"]
                if ev_ is None or ev_.query():
                    slot = self._slot_stack[k]
                    del self._slot_stack[k]
                    break
            if slot is None:
                slot = self._slot_stack.popleft()
        try:
            if slot["event"] is not None:
                slot["event"].synchronize()
                slot["event"] = None
            def grow(sl, sizes):
                for key, need in sizes:
                    cur = sl[key]
                    if cur is None or cur.numel() < need:
                        sl[key] = None
                        sl[key] = torch.empty(need, dtype=torch.uint8).pin_memory()
                        sl[key + "_np"] = sl[key].numpy()

            with torch.cuda.device(self.device):
                sizes = []
                for key, need in (("stage", int(stage_bytes)), ("desc", int(desc_bytes))):
                    cur = slot[key]
                    if cur is None or cur.numel() < need:   # grown with headroom: page-locking is slow (40 ms per 30 MB)
                        sizes.append((key, max(int(need * 1.5), 1 << 20)))
                if sizes:
                    grow(slot, sizes)
                    # ... and the slots nobody holds grow with it, NOW: a job's first (warm-up) launch pays for all of them
                    # instead of the next launches paying one by one inside the job (as the output ring does)
                    idle = []
                    with self._slots_lock:
                        while True:
                            try:
                                pool.get_nowait()
                            except queue.Empty:
                                break
                            idle.append(self._slot_stack.pop())
                    try:
                        for sl in idle:
                            if sl["event"] is None or sl["event"].query():
                                sl["event"] = None
                                grow(sl, sizes)
                    finally:
                        for sl in idle:
                            self._slot_stack.append(sl)
                            pool.put(None)
        except BaseException:
            self._slot_stack.append(slot)
            pool.put(None)
            raise
        return slot

    def _slot_release(self, slot, event=None):
        slot["event"] = event
        self._slot_stack.append(slot)
        self._slots.put(None)

    def _slot_upload(self, slot, stage_bytes, desc_bytes):
        """The first stage_bytes / desc_bytes of the slot's two buffers -> device uint8 tensors (two DMAs on the upload stream);
        the slot goes back to the pool guarded by the copies' event.  Returns (stage_dev, desc_dev, ready event)."""
        torch = _torch()
        up = self.copy_stream("up")
        with torch.cuda.device(self.device):
            cur = torch.cuda.current_stream(self.device)
            ctx = torch.cuda.stream(up) if up is not None else None
            if ctx is not None:
                ctx.__enter__()
            try:
                sd = slot["stage"][:max(int(stage_bytes), 1)].to(self.device, non_blocking=True)
                dd = slot["desc"][:max(int(desc_bytes), 1)].to(self.device, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(up if up is not None else cur)
            finally:
                if ctx is not None:
                    ctx.__exit__(None, None, None)
            if up is not None:
                cur.wait_event(ev)
                sd.record_stream(cur), dd.record_stream(cur)
        self._slot_release(slot, ev)
        return sd, dd, ev

    def planner(self):
        """The engine's planner thread (one): prepare_* calls for launch i + 1 run here while the calling thread enqueues
        launch i -- the native planners release the interpreter lock.  MAGPHASE_PLANNER_THREAD=0: inline."""
        import concurrent.futures as cf

        ex = getattr(self, "_planner", None)
        if ex is None:
            # (one worker: two -- the two launches of a generation batch prepared side by side -- measured 207-214 k x real time
            # against 219-221 k on the same box: their staging copies compete for the same memory bandwidth)
            ex = self._planner = cf.ThreadPoolExecutor(max_workers=1, thread_name_prefix="mpx-plan")
        return ex

    def prepare_async(self, kind, *args, **kw):
        """Future of prepare_analysis / prepare_synthesis (kind 'analysis' / 'synthesis') on the planner thread."""
        import concurrent.futures as cf

        fn = self.prepare_analysis if kind == "analysis" else self.prepare_synthesis
        if os.environ.get("MAGPHASE_PLANNER_THREAD", "1") == "0":
            f = cf.Future()
            try:
                f.set_result(fn(*args, **kw))
            except BaseException as exc:   # noqa: B902 -- delivered by result()
                f.set_exception(exc)
            return f
        return self.planner().submit(fn, *args, **kw)

    def prepare_analysis(self, utts, fft_len=None, wait=True):
        """The host side of an analysis launch (LosslessAnalysisPlan / CompressedAnalysisPlan) without touching a stream:
        utterance list walked in native code, samples staged into a page-locked slot, frame tables written in their device
        types (mpx_host_plan_analysis_batch), f0 and its median-3 on the host.  Returns a PreparedAnalysis, or None when
        the batch is not in the plain shape the native path handles (the plan constructor then takes the generic path,
        which converts -- or raises what the reference's arithmetic raises)."""
        ph = hostplan.pyhost()
        if ph is None or not utts:
            return None
        m = ph.analysis_marshal(utts)
        if m is None:
            return None
        U, total, E, all_i16 = ph.analysis_info(m)
        fs_list = [u[1] for u in utts]
        N = None
        for fs in set(fs_list):
            n_ = fft_len if fft_len is not None else hm.define_fft_len(fs)
            if N is not None and n_ != N:
                return None    # the generic path raises "all utterances of a plan must share fft_len"
            N = n_
        if E <= 0 or total <= 0:
            return None
        stage_bytes = (2 * total + 8) if all_i16 else 4 * total
        a256 = lambda n: (int(n) + 255) // 256 * 256   # noqa: E731
        o_pos, o_left, o_right, o_voi = 0, a256(8 * E), a256(8 * E) + a256(4 * E), a256(8 * E) + 2 * a256(4 * E)
        desc_bytes = o_voi + a256(4 * E)
        slot = self._slot_acquire(stage_bytes, desc_bytes, wait=wait)
        if slot is None:
            return None
        try:
            d = slot["desc_np"]
            pm, left64, f0, f0_med = (np.empty(E, dtype=np.int64), np.empty(E, dtype=np.int64), np.empty(E), np.empty(E))
            frame_off = np.empty(U + 1, dtype=np.int64)
            long_f, long_l = np.empty(512, dtype=np.int64), np.empty(512, dtype=np.int64)
            F, n_long = ph.analysis_run(m, slot["stage"].data_ptr(), 0 if all_i16 else 1, d[o_pos:o_pos + 8 * E],
                                        d[o_left:o_left + 4 * E], d[o_right:o_right + 4 * E], d[o_voi:o_voi + 4 * E], pm,
                                        left64, f0, f0_med, frame_off, int(N), long_f, long_l,
                                        self.host_threads(stage_bytes))
            if F < 0 or n_long > 512:
                self._slot_release(slot)
                return None
        except BaseException:
            self._slot_release(slot)
            raise
        p = PreparedAnalysis()
        p.engine, p.slot, p.n_utts, p.fs, p.fft_len = self, slot, U, fs_list, int(N)
        p.total_smpls, p.total_frames, p.all_i16 = int(total), int(F), bool(all_i16)
        p.stage_bytes, p.desc_bytes, p.cap = stage_bytes, desc_bytes, int(E)
        p.offs = (o_pos, o_left, o_right, o_voi)
        p.frame_off, p.pm, p.left64, p.f0, p.f0_med = frame_off, pm[:F], left64[:F], f0[:F], f0_med[:F]
        p.long = [(int(long_f[k]), int(long_l[k])) for k in range(int(n_long))]
        return p

    def _comp_slot_shares(self):
        """(slots of the compressed synthesis kernel, np.concatenate(([0], cumsum(w))), w.sum()) of their float64 weights --
        what mpx_host_plan_synthesis_batch deals the frames by (hostmath.slot_cuts' operands, evaluated by numpy once)."""
        w = self.synth_ola_slot_weights(comp=True)
        n = self.host_constant("comp_slots_n", self.synth_comp_slots)
        if w is None:
            return n, None, 0.0
        key = ("comp_shares", id(w))
        if key not in self._tables:
            w64 = np.asarray(w, dtype=np.float64)[:n]
            self._tables[key] = (np.ascontiguousarray(np.concatenate(([0.0], np.cumsum(w64)))), float(w64.sum()))
        return (n,) + self._tables[key]

    def prepare_synthesis(self, utts, fs, fft_len=None, b_voi_ap_win=True, b_const_rate=False, wait=True):
        """The host side of a compressed-feature synthesis launch (CompressedSynthesisPlan) without touching a stream:
        coefficient rows staged into a page-locked slot, every device table written in its final type
        (mpx_host_plan_synthesis_batch).  Returns a PreparedSynthesis, or None when the batch is not in the plain shape the
        native path handles or the numpy form would raise (the plan constructor then takes the generic path)."""
        ph = hostplan.pyhost()
        if ph is None or not utts:
            return None
        m = ph.synthesis_marshal(utts)
        if m is None:
            return None
        U, R, mag_dim, phase_dim = ph.synthesis_info(m)
        if R <= 0 or R >= (1 << 30):
            return None
        N = int(fft_len) if fft_len else hm.define_fft_len(fs)
        f0 = np.empty(R)
        ph.synthesis_lf0(m, f0)
        np.exp(f0, out=f0)                                               # magphase.py:846 (numpy's exp, as the array API)
        n_slots, wcum, wsum = self._comp_slot_shares()
        unwarp_rows = bool(b_const_rate) or os.environ.get("MAGPHASE_UNWARP_ROWS_VAR", "1") != "0"
        stage_bytes = 4 * R * (mag_dim + 2 * phase_dim)
        desc_cap = hostplan.synth_desc_bytes(R, U, n_slots, True)
        cap = 2 * R + 2 * U
        slot = self._slot_acquire(stage_bytes, desc_cap, wait=wait)
        if slot is None:
            return None
        try:
            v_shift, v_pm = np.empty(cap, dtype=np.int64), np.empty(cap, dtype=np.int64)
            voiced_host = np.empty(cap, dtype=np.int32)
            frame_off = np.empty(U + 1, dtype=np.int64)
            ns_len, out_start, out_len = (np.empty(U, dtype=np.int64) for _ in range(3))
            runs_host = np.zeros(U + n_slots + 1, dtype=hm.OLA_RUN_DTYPE)
            counts, desc_off = np.zeros(8, dtype=np.int64), np.zeros(18, dtype=np.int64)
            def run(n_sl, wc, ws, stage_ptr):
                return ph.synthesis_run(m, stage_ptr, f0, float(fs), N, int(bool(b_const_rate)), int(bool(b_voi_ap_win)),
                                        int(n_sl), wc, float(ws), int(unwarp_rows), slot["desc_np"][:desc_cap], desc_off,
                                        v_shift, v_pm, voiced_host, frame_off, ns_len, out_start, out_len, runs_host, counts,
                                        self.host_threads(stage_bytes))

            F = run(n_slots, wcum, wsum, slot["stage"].data_ptr())
            if F == -4000000 and 0 < counts[0] < n_slots:   # fewer frames than slots: shares by the first F weights
                nf = int(counts[0])                        # (hostmath.slot_cuts: w[:ns], their sum numpy's)
                w64 = np.asarray(self.synth_ola_slot_weights(comp=True), dtype=np.float64)[:nf]
                F = run(nf, np.ascontiguousarray(np.concatenate(([0.0], np.cumsum(w64)))), float(w64.sum()), 0)
            if F < 0:
                self._slot_release(slot)
                return None
        except BaseException:
            self._slot_release(slot)
            raise
        p = PreparedSynthesis()
        p.engine, p.slot = self, slot
        p.key = (int(fs), N, bool(b_const_rate), bool(b_voi_ap_win), unwarp_rows)
        p.n_utts, p.n_rows, p.mag_dim, p.phase_dim = int(U), int(R), int(mag_dim), int(phase_dim)
        p.total_frames, p.n_runs, p.n_slots = int(F), int(counts[1]), int(counts[2])
        p.stage_bytes, p.desc_bytes, p.n_tiles1 = stage_bytes, int(counts[3]), int(counts[6])
        p.desc_off = desc_off
        p.v_shift, p.v_pm, p.voiced_host = v_shift[:F], v_pm[:F], voiced_host[:F]
        p.frame_off, p.ns_len, p.out_start, p.out_len = frame_off, ns_len, out_start, out_len
        p.runs_host = runs_host[:p.n_runs]
        return p

    def to_device_pinned(self, arr, dtype):
        """Host array -> device tensor through a page-locked copy (async H2D on the current stream)."""
        torch = _torch()
        h = torch.from_numpy(np.ascontiguousarray(arr, dtype=dtype)).pin_memory()
        return h.to(self.device, non_blocking=True)

    @staticmethod
    def feat_ld(mag, real, imag):
        """Common row pitch of three feature views (unit column stride, equal row stride) for the C ABI."""
        ld = int(mag.stride(0)) if mag.shape[0] > 1 else max(int(mag.stride(0)), int(mag.shape[1]))
        for t in (mag, real, imag):
            if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
                raise ValueError("feature matrices must be 2-D with unit column stride")
            if t.shape[0] > 1 and int(t.stride(0)) != ld:
                raise ValueError("mag/real/imag must share one row pitch")
        return ld

    def host_constant(self, key, build):
        """A host value computed once per key."""
        if key not in self._tables:
            self._tables[key] = build()
        return self._tables[key]

    def constant(self, key, build, dtype=np.float32):
        """Device-resident constant table, built (float64 on the host) and uploaded once per key."""
        if key not in self._tables:
            self._tables[key] = self.to_device(build(), dtype)
        return self._tables[key]

    def to_device_packed(self, items):
        """
        items: list of (name, array, numpy dtype).  ONE host-to-device copy for all of them (each ~25 us on its own: a
        plan has 15-25 small index tables); returns {name: tensor}, the tensors being 256-byte aligned views of one
        device buffer.  The arrays are cast straight into the page-locked arena (one pass: no intermediate host image) and
        the copy never blocks: round 5 found the tables of a launch of more than ~20 k frames (> 1 MB) going up as a PAGEABLE
        synchronous copy, which waits for everything queued on the stream -- the host and the device took turns.
        """
        torch = _torch()
        tmap = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64,
                np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64, np.dtype(np.uint8): torch.uint8}
        shapes, offs, sizes, total = [], [], [], 0
        for _name, arr, dt in items:
            shp = np.shape(arr)
            nb = int(np.prod(shp, dtype=np.int64)) * np.dtype(dt).itemsize
            total = (total + 255) // 256 * 256
            offs.append(total)
            shapes.append(shp)
            sizes.append(nb)
            total += nb
        total = max(total, 1)

        def fill(host):   # host: uint8 view of `total` bytes (page-locked arena, or a fresh array for oversized sets)
            for (_name, arr, dt), off, shp, nb in zip(items, offs, shapes, sizes):
                if nb:
                    np.copyto(host[off:off + nb].view(dt).reshape(shp), arr, casting="unsafe")

        if total <= self._ARENA_MAX_ITEM:
            dev = self._arena_upload(None, nbytes=total, fill=fill)
        else:
            host = np.zeros(total, dtype=np.uint8)
            fill(host)
            dev = torch.from_numpy(host).to(self.device, non_blocking=False)
        out = {}
        for (name, _arr, dt), off, shp, nb in zip(items, offs, shapes, sizes):
            if nb == 0:
                out[name] = torch.empty(shp, dtype=tmap[np.dtype(dt)], device=self.device)
            else:
                out[name] = dev[off:off + nb].view(tmap[np.dtype(dt)]).view(shp)
        return out

    _ARENA_BYTES = 64 << 20
    _ARENA_PARTS = 4
    _ARENA_MAX_ITEM = (64 << 20) // 4

    def _arena_upload(self, a, nbytes=None, fill=None):
        """A host array (or `nbytes` written by fill(view)) -> device tensor through a page-locked bump arena, WITHOUT
        blocking: a pageable `tensor.to(device)` waits for everything queued on the stream before it -- after a batch's
        kernels have been launched that is the whole batch, which serialised the host with the device once per table.
        The arena is four parts used in turn; a part is waited for (the event of its last copy) only when the bump pointer
        comes round to it again, three parts of uploads later -- in practice never a wait."""
        import threading

        torch = _torch()
        ar = getattr(self, "_arena", None)
        if ar is None:
            buf = torch.empty(self._ARENA_BYTES, dtype=torch.uint8).pin_memory()
            ar = self._arena = {"t": buf, "np": buf.numpy(), "off": 0, "lock": threading.Lock(),
                                "ev": [None] * self._ARENA_PARTS}
        n = int(a.nbytes) if a is not None else int(nbytes)
        part = self._ARENA_BYTES // self._ARENA_PARTS
        with ar["lock"]:
            off = (ar["off"] + 255) // 256 * 256
            q = off // part
            if q >= self._ARENA_PARTS or off + n > (q + 1) * part:   # does not fit the part the pointer is in: on to the next
                q = (q + 1) % self._ARENA_PARTS if q < self._ARENA_PARTS else 0
                off = q * part
            if q != ar.get("cur"):   # entering a part (by overflow or because the pointer walked into it): its old copies first
                if ar["ev"][q] is not None:
                    ar["ev"][q].synchronize()
                    ar["ev"][q] = None
                ar["cur"] = q
            ar["off"] = off + n
            view = ar["np"][off:off + n]
            if a is not None:
                view[:] = a.reshape(-1).view(np.uint8)
            else:
                fill(view)
            with torch.cuda.device(self.device):
                dev = ar["t"][off:off + n].to(self.device, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(self.device))
                ar["ev"][q] = ev
        if a is None:
            return dev
        tmap = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64, np.dtype(np.int32): torch.int32,
                np.dtype(np.int64): torch.int64, np.dtype(np.uint8): torch.uint8, np.dtype(np.int16): torch.int16}
        return dev.view(tmap[a.dtype]).view(a.shape)

    def to_device(self, arr, dtype):
        torch = _torch()
        a = np.ascontiguousarray(arr, dtype=dtype)
        if 0 < a.nbytes <= self._ARENA_MAX_ITEM and a.dtype in (np.float32, np.float64, np.int32, np.int64, np.uint8,
                                                                 np.int16) and a.ndim >= 1:
            return self._arena_upload(a)
        return torch.from_numpy(a).to(self.device, non_blocking=False)

    def tables(self, fft_len):
        if fft_len not in self._tables:
            torch = _torch()
            nbytes = self.lib.mpx_tables_bytes(int(fft_len))
            if nbytes == 0:
                raise ValueError("fft_len %r not supported by the HIP path (1024, 2048 or 4096)" % (fft_len,))
            t = torch.empty(nbytes // 4, dtype=torch.float32, device=self.device)
            self.launch("mpx_tables_init", int(fft_len), t)
            self._tables[fft_len] = t
        return self._tables[fft_len]

    def tables_f64(self, fft_len):
        key = ("f64", fft_len)
        if key not in self._tables:
            torch = _torch()
            nbytes = self.lib.mpx_tables_f64_bytes(int(fft_len))
            if nbytes == 0:
                raise ValueError("fft_len %r not supported by the HIP path (1024, 2048 or 4096)" % (fft_len,))
            t = torch.empty(nbytes // 8, dtype=torch.float64, device=self.device)
            self.launch("mpx_tables_f64_init", int(fft_len), t)
            self._tables[key] = t
        return self._tables[key]

    # ------------------------------------------------------------------ kernels
    def hann_table(self):
        """hostmath.hann_half_table on the device (float64, built once per engine: ~30 ms of numpy, 16.8 MB)."""
        t = getattr(self, "_hann_table", None)
        if t is None:
            t = self._hann_table = self.to_device(hm.hann_half_table(), np.float64)
        return t

    def hann_window_args(self):
        """(table, its cap) of the float64 analysis kernels' window weights: numpy's own np.hanning from hann_table, or
        (None, 0) with MAGPHASE_F64_WINDOW=analytic (evaluated on the device)."""
        if os.environ.get("MAGPHASE_F64_WINDOW", "table") == "analytic":
            return None, 0
        return self.hann_table(), hm.HANN_TABLE_CAP

    def analysis_frames(self, fft_len, sig, pos, left, right, out=None, precise=False, rows_in_use=None):
        """sig f32[n], pos i64[F], left/right i32[F] (device) -> (mag, real, imag) f32[F x H] (device).
        precise: window / transform / epilogue in float64 (mpx_analysis_frames_f64): the compressed analysis' choice;
        rows_in_use (precise only): f32[F], 0 = this frame's phase rows are never read, write the magnitudes only."""
        nfr = int(pos.numel())
        H = fft_len // 2 + 1
        if out is None:
            out = tuple(self.empty_feats(nfr, H) for _ in range(3))
        ld = self.feat_ld(*out)
        if precise:
            self.launch("mpx_analysis_frames_f64w", int(fft_len), self.tables_f64(fft_len), sig, pos, left, right, nfr,
                        out[0], out[1], out[2], ld, rows_in_use, *self.hann_window_args())
        else:
            self.launch("mpx_analysis_frames", int(fft_len), self.tables(fft_len), sig, pos, left, right, nfr,
                        out[0], out[1], out[2], ld)
        return out

    def synthesis_lossless_frames(self, fft_len, mag, real, imag, out=None):
        nfr = int(mag.shape[0])
        if out is None:
            out = self.empty((nfr, fft_len))
        self.launch("mpx_synthesis_lossless_frames", int(fft_len), self.tables(fft_len), mag, real, imag, nfr, out,
                    self.feat_ld(mag, real, imag))
        return out

    def ola_gather(self, fft_len, frames, utt_frame_off, pm_rel, out_start, out_off, max_out_len, total_out, out=None):
        if out is None:
            out = self.empty((int(total_out),))
        self.launch("mpx_ola_gather", int(fft_len), frames, int(out_start.numel()), utt_frame_off, pm_rel, out_start,
                    out_off, int(max_out_len), out)
        return out

    def synth_ola_slots(self):
        torch = _torch()
        with torch.cuda.device(self.device):
            n = int(self.lib.mpx_synth_ola_slots())
        cus = os.environ.get("MAGPHASE_SYN_CUS")   # experiment: the synthesis launch on fewer CUs (slots = 6 per workgroup)
        return n if not cus else max(6, min(n, 6 * int(cus)))

    def synth_ola_slot_weights(self, comp=False):
        """Relative speeds of the slots of the lossless (comp=True: the compressed, comp="roundtrip": the one-launch copy
        synthesis) kernel (mpx_synth_ola_slot_weights / mpx_synth_comp_slot_weights / mpx_roundtrip_slot_weights), cached;
        MAGPHASE_OLA_WEIGHTS=0 -> None (equal shares)."""
        if os.environ.get("MAGPHASE_OLA_WEIGHTS", "1") == "0":
            return None
        key = ("rt_w" if comp == "roundtrip" else "comp_w") if comp else "ola_w"
        if key not in self._tables:
            n = self.synth_comp_slots() if comp else self.synth_ola_slots()
            w = np.zeros(n, dtype=np.float32)
            name = ("mpx_roundtrip_slot_weights" if comp == "roundtrip" else
                    "mpx_synth_comp_slot_weights") if comp else "mpx_synth_ola_slot_weights"
            _lib.check(getattr(self.lib, name)(w.ctypes.data, n), name)
            self._tables[key] = w
        return self._tables[key]

    def post_filter(self, mag_mel_log, fs, **kw):
        """Device MagPhase post-filter (mpx_post_filter) of a float32 [F x D] tensor; kw as magphase.post_filter."""
        F, D = int(mag_mel_log.shape[0]), int(mag_mel_log.shape[1])
        key = ("post_filter", D, int(fs)) + tuple(sorted(kw.items()))
        if key not in self._tables:   # device-resident per configuration (two small uploads per call otherwise)
            nx0, nx1, half, tilt = hm.post_filter_tables(D, fs, **kw)
            self._tables[key] = (nx0, nx1, self.to_device(half, np.int32), self.to_device(tilt, np.float32))
        nx0, nx1, d_half, d_tilt = self._tables[key]
        out = self.empty((F, D))
        self.launch("mpx_post_filter", mag_mel_log, F, D, d_half, nx0, nx1, d_tilt, out)
        return out

    def post_filter_merlin(self, mag_mel_log, fs, pf_coef=1.4):
        """Device Merlin-style post-filter (mpx_post_filter_merlin, magphase.py:3375-3465) of a float32 [F x D] tensor
        (3 <= D <= 64) -> float32 [F x D].  Tables: hostmath.merlin_tables, resident on the device per configuration."""
        from . import libaudio as la

        F, D = int(mag_mel_log.shape[0]), int(mag_mel_log.shape[1])
        key = ("merlin", D, int(fs), float("%1.2f" % pf_coef))
        if key not in self._tables:
            t = hm.merlin_tables(D, fs, pf_coef)
            self._tables[key] = (t["alpha"], int(t["g"].shape[1])) + tuple(
                self.to_device(t[k], np.float32) for k in ("c1", "lifter", "g", "wk", "cf"))
        alpha, nb, c1, lifter, g, wk, cf = self._tables[key]
        mcep, mcep_w, out = (self.empty((max(F, 1), D)) for _ in range(3))
        r0, p_r0 = self.empty((max(F, 1),)), self.empty((max(F, 1),))
        x = mag_mel_log.contiguous()
        self.launch("mpx_post_filter_merlin", x, F, D, c1, lifter, g, wk, nb, float(alpha), cf, float(la.MAGIC), mcep,
                    mcep_w, r0, p_r0, out)
        return out[:F]

    def post_filter_pack(self, mats):
        """The [F_i x D] matrices of mp.post_filter_batch (host arrays or tensors on this device, any of pack_rows' dtypes
        and row strides) as ONE dense float32 device matrix [sum F_i x D] (one mpx_rows_pack launch) and the row offsets."""
        D = int(mats[0].shape[1])
        offs = np.concatenate(([0], np.cumsum([int(m.shape[0]) for m in mats]))).astype(np.int64)
        x = self.empty((int(offs[-1]), D))
        self.pack_rows([list(mats)], [x])
        return x, offs

    @staticmethod
    def _grad_rows(grad_out, what):
        """grad_out as the dense float32 [F x D] matrix the backward entries read."""
        torch = _torch()
        if grad_out.dim() != 2:
            raise ValueError("%s: grad_out must be [frames x dim]" % what)
        return grad_out.to(torch.float32).contiguous()

    def post_filter_backward(self, grad_out, fs, **kw):
        """mpx_post_filter_backward (k_post_filter_bwd): grad_out = the gradient with respect to Engine.post_filter's output,
        [F x D] -> the gradient with respect to its input, float32 [F x D].  fs / kw as Engine.post_filter; the gather
        tables (hostmath.post_filter_backward_tables of the forward's own tables) are resident per configuration."""
        g = self._grad_rows(grad_out, "post_filter_backward")
        F, D = int(g.shape[0]), int(g.shape[1])
        key = ("post_filter_bwd", D, int(fs)) + tuple(sorted(kw.items()))
        if key not in self._tables:
            import warnings

            with warnings.catch_warnings():   # (the forward gave the tables' warnings)
                warnings.simplefilter("ignore")
                fwd = hm.post_filter_tables(D, fs, **kw)
            cnt, idx, w, fan = hm.post_filter_backward_tables(D, *fwd)
            self._tables[key] = (fan, self.to_device(cnt, np.int32), self.to_device(idx, np.int32),
                                 self.to_device(w, np.float32))
        fan, d_cnt, d_idx, d_w = self._tables[key]
        out = self.empty((F, D))
        self.launch("mpx_post_filter_backward", g, F, D, d_cnt, d_idx, d_w, fan, out)
        return out

    def post_filter_merlin_backward(self, mag_mel_log, grad_out, fs, pf_coef=1.4):
        """mpx_post_filter_merlin_backward (k_rows_gemm, k_merlin_r0_bwd): mag_mel_log = the float32 [F x D] rows
        Engine.post_filter_merlin was given, grad_out = the gradient with respect to its output -> the gradient with respect
        to mag_mel_log, float32 [F x D].  A row for which the forward wrote la.MAGIC (or an infinity) gets zeros.  Workspace:
        four [F x D] matrices."""
        g = self._grad_rows(grad_out, "post_filter_merlin_backward")
        F, D = int(mag_mel_log.shape[0]), int(mag_mel_log.shape[1])
        if tuple(g.shape) != (F, D):
            raise ValueError("post_filter_merlin_backward: grad_out is %s, the input [%d x %d]" % (tuple(g.shape), F, D))
        key = ("merlin_bwd", D, int(fs), float("%1.2f" % pf_coef))
        if key not in self._tables:
            t = hm.merlin_tables(D, fs, pf_coef)
            self._tables[key] = (int(t["g"].shape[1]),) + tuple(self.to_device(a, np.float32) for a in (
                t["c1"], t["lifter"], t["g"], t["wk"], np.ascontiguousarray(t["cf"].T), np.ascontiguousarray(t["c1"].T)))
        nb, c1, lifter, gmat, wk, cf_t, c1_t = self._tables[key]
        mcep, mcep_w, g_pf, g_c, out = (self.empty((max(F, 1), D)) for _ in range(5))
        x = mag_mel_log.to(_torch().float32).contiguous()
        self.launch("mpx_post_filter_merlin_backward", x, g, F, D, c1, lifter, gmat, wk, nb, cf_t, c1_t, mcep, mcep_w,
                    g_pf, g_c, out)
        return out[:F]

    def output_hpf(self, pcm, out_off_host, fs, design="butter40"):
        """
        magphase.py:981-995 on the device: float32 pcm [total] (utterances concatenated at out_off_host) ->
        float64 tensor, every utterance filtered from a zero state (mpx_output_hpf: cascade of biquads, blocked scan).
        design: hostmath.hpf_tables' -- 'butter40' (type 1) or 'ellip60' (synthesis_from_compressed_type2, :1599-1604).
        """
        torch = _torch()
        block = int(self.lib.mpx_hpf_block())
        key = ("hpf", int(fs)) if design == "butter40" else ("hpf", int(fs), design)
        if key not in self._tables:
            sos, pm, g = hm.hpf_tables(fs, block, design)
            self._tables[key] = (sos, self.to_device(pm, np.float64), self.to_device(g, np.float64))
        sos, d_pm, d_g = self._tables[key]
        out_off_host = np.asarray(out_off_host, dtype=np.int64)
        lens = np.diff(out_off_host)
        nblk = (lens + block - 1) // block
        blk_off = np.concatenate(([0], np.cumsum(nblk))).astype(np.int32)
        d_off = self.to_device(out_off_host, np.int64)
        d_blk = self.to_device(blk_off, np.int32)
        total, tb = int(out_off_host[-1]), int(blk_off[-1])
        zend = torch.empty(2 * max(tb, 1), dtype=torch.float64, device=self.device)
        zstart = torch.empty(2 * max(tb, 1), dtype=torch.float64, device=self.device)
        y_tmp = torch.empty(max(total, 1), dtype=torch.float64, device=self.device)
        y = torch.empty(max(total, 1), dtype=torch.float64, device=self.device)
        sos_c = np.ascontiguousarray(sos, dtype=np.float64)
        self.launch("mpx_output_hpf", pcm, d_off, d_blk, int(lens.size), int(lens.max()) if lens.size else 0,
                    sos_c.ctypes.data_as(ctypes.c_void_p), d_pm, d_g, zend, zstart, y_tmp, y)
        return y[:total]

    def mel_unwarp_single(self, m_x, n_bins, alpha, exp_out=False):
        """la.sp_mel_unwarp for one [F x n] host matrix through mpx_mel_unwarp (the phase jobs run on a 1-frame dummy)."""
        m_x = np.atleast_2d(np.asarray(m_x, dtype=np.float64))
        F, n = m_x.shape
        u = self.constant(("u_mag", int(n), int(n_bins), float(alpha)), lambda: hm.unwarp_matrix(n, n_bins, alpha))
        ld = int(self.lib.mpx_spec_ld(int(n_bins)))
        a = self.to_device(m_x, np.float32)
        o_exp, o_lin, o_dummy = (self.empty((F, ld)) for _ in range(3))
        # magnitude job: exp(x U); "real" job: x U; "imag" job: scratch
        self.launch("mpx_mel_unwarp", F, int(n_bins), a, n, u, o_exp, a, a, n, u, o_lin, o_dummy, ld)
        return self.to_host_f64((o_exp if exp_out else o_lin)[:, :int(n_bins)])

    def mel_warp_single(self, m_abs, nbins_out, alpha):
        """la.sp_mel_warp's linear map for one host matrix of MAGNITUDES [F x H] through mpx_mel_warp (the magnitude job:
        W ln(x^2 + 1e-8) = the warped ln|f| (the one-sided cepstral sum carries the 1/2); the phase jobs run on a 1-row dummy):
        float64 [F x nbins_out]."""
        torch = _torch()
        m_abs = np.atleast_2d(np.asarray(m_abs, dtype=np.float64))
        F, H = m_abs.shape
        w = self.constant(("w_mag", int(nbins_out), H, float(alpha)), lambda: hm.warp_matrix(nbins_out, H, alpha))
        w1 = self.constant(("w_dummy", H), lambda: np.zeros((1, H)))
        mag = self.feats_to_device(m_abs)
        voi = torch.zeros(F, dtype=torch.float32, device=self.device)
        out, d0, d1 = self.empty((F, int(nbins_out))), self.empty((F, 1)), self.empty((F, 1))
        self.launch("mpx_mel_warp", F, H, mag, mag, mag, None, None, None, w, int(nbins_out), w1, 1, voi, out, d0, d1,
                    self.feat_ld(mag, mag, mag))
        return self.to_host_f64(out)

    def min_phase_single(self, m_mag):
        """la.build_min_phase_from_mag_spec for one [F x H] host matrix through mpx_min_phase."""
        torch = _torch()
        m_mag = np.atleast_2d(m_mag)
        F, H = m_mag.shape
        N = 2 * (H - 1)
        tab = self.tables(N)
        ld = int(self.lib.mpx_spec_ld(H))
        mag = self.empty((F, ld))
        mag[:, :H].copy_(torch.from_numpy(np.ascontiguousarray(m_mag, dtype=np.float32)))
        ident = torch.arange(F, dtype=torch.int32, device=self.device)
        zeros_t = torch.zeros(F, dtype=torch.float32, device=self.device)
        o_m, o_r, o_i = (self.empty((F, ld)) for _ in range(3))
        self.launch("mpx_min_phase", N, tab, mag, ident, ident, zeros_t, F, o_m, o_r, o_i, ld)
        m = self.to_host_f64(o_m[:, :H])
        return m * (self.to_host_f64(o_r[:, :H]) + 1j * self.to_host_f64(o_i[:, :H]))

    def min_phase_rows(self, mats):
        """la.build_min_phase_from_mag_spec for a list of [F_i x H] magnitude matrices (host arrays or tensors on this
        device, any of pack_rows' dtypes) through ONE mpx_min_phase launch -> (m, cos phi, sin phi), float32 [sum F_i x H]
        views of rows at mpx_spec_ld(H)."""
        torch = _torch()
        H = int(mats[0].shape[1])
        if any(m.ndim != 2 or int(m.shape[1]) != H for m in mats):
            raise ValueError("min_phase_rows: every matrix must be [F x %d]" % H)
        N = 2 * (H - 1)
        F = int(sum(int(m.shape[0]) for m in mats))
        ld = int(self.lib.mpx_spec_ld(H))
        mag = self.empty((F, ld))[:, :H]
        if any(torch.is_tensor(m) for m in mats):
            self.pack_rows([list(mats)], [mag])
        elif F:
            mag.copy_(torch.from_numpy(np.concatenate([np.asarray(m, dtype=np.float32) for m in mats], axis=0)))
        o_m, o_r, o_i = (self.empty((F, ld))[:, :H] for _ in range(3))
        if F:
            ident = torch.arange(F, dtype=torch.int32, device=self.device)
            zeros_t = torch.zeros(F, dtype=torch.float32, device=self.device)
            self.launch("mpx_min_phase", N, self.tables(N), mag, ident, ident, zeros_t, F, o_m, o_r, o_i, ld)
        return o_m, o_r, o_i

    def min_phase_backward(self, o_m, o_r, o_i, g_m, g_r, g_i, n_phase=None):
        """mpx_min_phase_backward (k_min_phase_bwd): (o_m, o_r, o_i) = mpx_min_phase's own output rows ([F x H] views of one
        pitch), (g_m, g_r, g_i) the gradients with respect to them ([F x H], None: zero) -> the gradient with respect to the
        magnitude rows, float32 [F x H] (a view of rows at the outputs' pitch)."""
        torch = _torch()
        F, H = int(o_m.shape[0]), int(o_m.shape[1])
        N = 2 * (H - 1)
        ld = self.feat_ld(o_m, o_r, o_i)
        gs = [None if g is None else g.to(torch.float32) for g in (g_m, g_r, g_i)]
        have = [g for g in gs if g is not None]
        if any(tuple(g.shape) != (F, H) for g in have):
            raise ValueError("min_phase_backward: gradients must be [%d x %d]" % (F, H))
        if have and (any(g.stride(1) != 1 for g in have) or len({int(g.stride(0)) for g in have}) > 1
                     or int(have[0].stride(0)) < H):
            gs = [None if g is None else g.contiguous() for g in gs]
            have = [g for g in gs if g is not None]
        out = self.empty((F, ld))[:, :H]
        if F:
            self.launch("mpx_min_phase_backward", N, self.tables(N), o_m, o_r, o_i, ld, gs[0], gs[1], gs[2],
                        int(have[0].stride(0)) if have else H, H if n_phase is None else int(n_phase), F, out, ld)
        return out

    def true_envelope(self, mats, in_type="abs", ncoeffs=60, thres_db=0.1, fade=0.7, max_iters=hm.TRUE_ENV_MAX_ITERS,
                      forced_iters=None, want_iters=False, ticket=True, return_input=False):
        """
        la.true_envelope on a list of [F_i x H] matrices (numpy, or float32 device tensors) through ONE mpx_true_envelope
        launch: the rows are concatenated at mpx_spec_ld(H).  -> (device out [sum F_i x ld], row offsets, device int32
        passes per row or None).  max_iters = 1 with fade = fade_to_total is la.spectral_smoothing_rceps.
        forced_iters (tests): int per row, exactly that many passes.  ticket: frames handed out by a device counter (the
        faster form); False: by grid stride.  return_input: the packed float32 input rows [sum F_i x ld] as a
        fourth result (what true_envelope_backward takes).
        """
        torch = _torch()
        H = int(mats[0].shape[1])
        N = hm.true_envelope_check(H, in_type, ncoeffs)
        if any(int(m.shape[1]) != H for m in mats):
            raise ValueError("true_envelope_batch: every matrix must have the same number of bins")
        offs = np.concatenate(([0], np.cumsum([int(m.shape[0]) for m in mats]))).astype(np.int64)
        F = int(offs[-1])
        ld = int(self.lib.mpx_spec_ld(H))
        x = self.empty((F, ld))
        out = self.empty((F, ld))
        for m, a, b in zip(mats, offs[:-1], offs[1:]):
            if b > a:
                src = m if torch.is_tensor(m) else torch.from_numpy(np.ascontiguousarray(m, dtype=np.float32))
                x[int(a):int(b), :H].copy_(src, non_blocking=torch.is_tensor(m))
        w = self.constant(("true_env_w", N, int(ncoeffs), float(fade)), lambda: hm.true_envelope_lifter(N, ncoeffs, fade))
        iters = torch.empty(F, dtype=torch.int32, device=self.device) if (want_iters or forced_iters is not None) else None
        forced = None
        if forced_iters is not None:
            forced = self.to_device(np.asarray(forced_iters, dtype=np.int32).reshape(F), np.int32)
        tk = torch.empty(1, dtype=torch.int32, device=self.device) if ticket else None
        self.launch("mpx_true_envelope", N, self.tables(N), w, x, ld, F, hm.TRUE_ENV_IN_TYPES.index(in_type),
                    float(thres_db), int(max_iters), out, ld, iters, forced, tk)
        return (out, offs, iters, x) if return_input else (out, offs, iters)

    def true_envelope_backward(self, x, iters, grad_out, n_bins, in_type="abs", ncoeffs=60, fade=0.7,
                               max_iters=hm.TRUE_ENV_MAX_ITERS, want_decisions=False, want_env=False, ticket=True):
        """
        Gradient of true_envelope's output rows with respect to its input rows through ONE mpx_true_envelope_backward launch
        (k_true_envelope_bwd).  x: the forward's float32 device input rows [F x >= H], H = n_bins (row pitch =
        stride(0)); iters: device int32 [F], the forward's passes per row; grad_out: float32 device [F x >= H].  -> the gradient
        [F x ld] (columns >= H are not written), or with want_decisions / want_env (tests) the tuple (gradient, decision
        words int32 [F x max_iters x ceil(H / 32)] or None, recomputed envelope rows [F x ld] or None).
        """
        torch = _torch()
        F, H = int(x.shape[0]), int(n_bins)
        ld = int(x.stride(0)) if F > 1 else int(x.shape[1])
        N = hm.true_envelope_check(H, in_type, ncoeffs)
        if int(x.shape[1]) < H or int(grad_out.shape[1]) < H:
            raise ValueError("true_envelope_backward: rows shorter than n_bins")
        if x.dtype != torch.float32 or grad_out.dtype != torch.float32 or iters.dtype != torch.int32:
            raise TypeError("true_envelope_backward: float32 rows and int32 pass counts expected")
        if x.stride(1) != 1 or grad_out.stride(1) != 1 or int(grad_out.shape[0]) != F or int(iters.numel()) != F:
            raise ValueError("true_envelope_backward: [F x H] rows with unit column stride and F pass counts expected")
        ld_g = int(grad_out.stride(0)) if F > 1 else int(grad_out.shape[1])
        old = int(self.lib.mpx_spec_ld(H))
        gx = self.empty((F, old))
        w = self.constant(("true_env_w", N, int(ncoeffs), float(fade)), lambda: hm.true_envelope_lifter(N, ncoeffs, fade))
        dec = torch.empty((F, int(max_iters), (H + 31) // 32), dtype=torch.int32, device=self.device) \
            if want_decisions else None
        env = self.empty((F, old)) if want_env else None
        tk = torch.empty(1, dtype=torch.int32, device=self.device) if ticket else None
        self.launch("mpx_true_envelope_backward", N, self.tables(N), w, x, ld, F, hm.TRUE_ENV_IN_TYPES.index(in_type),
                    int(max_iters), iters.contiguous(), grad_out, ld_g, gx, old, dec, env, old, tk)
        return (gx, dec, env) if (want_decisions or want_env) else gx

    # ------------------------------------------------------------------ MLPG
    def mlpg_pack(self, mats, width):
        """List of [F_i x width] matrices (numpy, or device tensors; float32 / float64, any row stride) -> (ONE device
        matrix [sum F_i x width], float64 if any of them is, else float32; row offsets int64 [n + 1]).  A batch of one
        device tensor with unit column stride is not copied: the kernels read it where it lies.  Host matrices go up in
        one copy; a mixed batch is gathered utterance by utterance."""
        torch = _torch()
        offs = np.concatenate(([0], np.cumsum([int(m.shape[0]) for m in mats]))).astype(np.int64)
        total = int(offs[-1])
        is_t = [torch.is_tensor(m) for m in mats]
        f64 = any((m.dtype == torch.float64) if t else (np.asarray(m).dtype == np.float64) for m, t in zip(mats, is_t))
        dt, ndt = (torch.float64, np.float64) if f64 else (torch.float32, np.float32)
        if len(mats) == 1 and is_t[0] and mats[0].dtype == dt and (mats[0].shape[1] <= 1 or mats[0].stride(1) == 1) \
                and (total <= 1 or mats[0].stride(0) >= width):
            return mats[0].detach(), offs
        if total == 0:
            return torch.empty((0, width), dtype=dt, device=self.device), offs
        if not any(is_t):
            host = np.concatenate([np.asarray(m, dtype=ndt).reshape(-1, width) for m in mats], axis=0)
            return self.to_device(host, ndt).view(total, width), offs
        buf = torch.empty((total, width), dtype=dt, device=self.device)
        for m, t, a, b in zip(mats, is_t, offs[:-1], offs[1:]):
            if b > a:
                src = m.detach() if t else torch.from_numpy(np.ascontiguousarray(m, dtype=ndt))
                buf[int(a):int(b)].copy_(src, non_blocking=t)
        return buf, offs

    @staticmethod
    def _mlpg_operand(t, width, what, total):
        """(is_float64, row pitch) of a device operand of the MLPG entries: [total x >= width], unit column stride."""
        torch = _torch()
        if t.dtype not in (torch.float32, torch.float64):
            raise TypeError("%s: float32 or float64 expected, got %s" % (what, t.dtype))
        if t.dim() != 2 or int(t.shape[0]) != total or int(t.shape[1]) != width or (width > 1 and t.stride(1) != 1):
            raise ValueError("%s: a [%d x %d] matrix with unit column stride expected, got %s"
                             % (what, total, width, tuple(t.shape)))
        return int(t.dtype == torch.float64), (int(t.stride(0)) if total > 1 else max(int(t.stride(0)), width))

    def _mlpg_var(self, var, width, total):
        torch = _torch()
        if var.dim() == 1:   # the global variance: one row, pitch 0
            if var.dtype not in (torch.float32, torch.float64) or int(var.numel()) != width or \
                    (width > 1 and var.stride(0) != 1):
                raise ValueError("mlpg: a global variance is one dense float32 / float64 row of %d values" % width)
            return int(var.dtype == torch.float64), 0
        return self._mlpg_operand(var, width, "mlpg: var", total)

    def mlpg_solve(self, mean, var, offs_dev, D, windows, rhs=False, out=None, work=None):
        """ONE mpx_mlpg_solve launch (k_mlpg_solve).  mean: device [total x K D] (a column slice of a wider
        matrix is passed as the view it is; rhs: the right-hand side itself, [total x D]); var: device [K D] (global) or
        [total x K D]; offs_dev: device int32 [n_utts + 1]; windows: hostmath.mlpg_windows(...).  -> out, float64 [total x D]
        (given: a view with unit column stride, written in place).  work: float64 [>= mpx_mlpg_work_doubles]."""
        torch = _torch()
        total, K = int(mean.shape[0]), int(windows.shape[0]) + 1
        m64, ld_m = self._mlpg_operand(mean, D if rhs else K * D, "mlpg: mean", total)
        v64, ld_v = self._mlpg_var(var, K * D, total)
        if out is None:
            out = torch.empty((total, D), dtype=torch.float64, device=self.device)
        o64, ld_o = self._mlpg_operand(out, D, "mlpg: out", total)
        if not o64:
            raise TypeError("mlpg: out must be float64")
        need = int(self.lib.mpx_mlpg_work_doubles(total, D))
        if work is None:
            work = torch.empty(need, dtype=torch.float64, device=self.device)
        if work.dtype != torch.float64 or int(work.numel()) < need or not work.is_contiguous():
            raise ValueError("mlpg: work must be %d contiguous float64" % need)
        wins = (ctypes.c_double * windows.size)(*[float(v) for v in windows.reshape(-1)])
        self.launch("mpx_mlpg_solve", mean, m64, ld_m, var, v64, ld_v, offs_dev, int(offs_dev.numel()) - 1, total, int(D),
                    K - 1, wins, int(bool(rhs)), out, ld_o, work)
        return out

    def mlpg_apply(self, x, var, offs_dev, D, windows, out=None):
        """ONE mpx_mlpg_apply launch (k_mlpg_apply): y_k = [P_k] W_k x for every stream.  x: device [total x D]; var: None
        (no precision factor: the dynamic features of x), or as mlpg_solve takes it.  -> out, float64 [total x K D]."""
        torch = _torch()
        total, K = int(x.shape[0]), int(windows.shape[0]) + 1
        x64, ld_x = self._mlpg_operand(x, D, "mlpg: x", total)
        v64, ld_v = (0, 0) if var is None else self._mlpg_var(var, K * D, total)
        if out is None:
            out = torch.empty((total, K * D), dtype=torch.float64, device=self.device)
        o64, ld_o = self._mlpg_operand(out, K * D, "mlpg: y", total)
        if not o64:
            raise TypeError("mlpg: y must be float64")
        wins = (ctypes.c_double * windows.size)(*[float(v) for v in windows.reshape(-1)])
        self.launch("mpx_mlpg_apply", x, x64, ld_x, var, v64, ld_v, offs_dev, int(offs_dev.numel()) - 1, total, int(D),
                    K - 1, wins, out, ld_o)
        return out

    def mlpg_streams(self, buf, var, offs_dev, streams, windows):
        """MLPG of several streams of one packed matrix, one mpx_mlpg_solve launch per stream on column slices.  buf:
        device [total x W]; var: device [W] or [total x W]; streams: [(first column, D), ...], stream s holding its K D
        columns [static | delta | acc] from its first column.  -> float64 [total x sum D], the streams side by side."""
        torch = _torch()
        total, K = int(buf.shape[0]), int(windows.shape[0]) + 1
        out = torch.empty((total, sum(d for _, d in streams)), dtype=torch.float64, device=self.device)
        work = torch.empty(int(self.lib.mpx_mlpg_work_doubles(total, max(d for _, d in streams))), dtype=torch.float64,
                           device=self.device)
        o = 0
        for c, d in streams:
            v = var[c:c + K * d] if var.dim() == 1 else var[:, c:c + K * d]
            self.mlpg_solve(buf[:, c:c + K * d], v, offs_dev, d, windows, out=out[:, o:o + d], work=work)
            o += d
        return out

    def mlpg_streams_backward(self, grad_out, var, offs_dev, streams, windows, width):
        """Gradient of mlpg_streams' output with respect to the packed means: per stream z = A^-1 g (the solve with the
        right-hand side given, refactoring A from the variances) and P_k W_k z (mpx_mlpg_apply).  grad_out: float64
        [total x sum D].  -> float64 [total x width]; columns of no stream are zero."""
        torch = _torch()
        total, K = int(grad_out.shape[0]), int(windows.shape[0]) + 1
        covered = sum(K * d for _, d in streams) == width
        g = (torch.empty if covered else torch.zeros)((total, width), dtype=torch.float64, device=self.device)
        dmax = max(d for _, d in streams)
        z = torch.empty((total, dmax), dtype=torch.float64, device=self.device)
        work = torch.empty(int(self.lib.mpx_mlpg_work_doubles(total, dmax)), dtype=torch.float64, device=self.device)
        o = 0
        for c, d in streams:
            v = var[c:c + K * d] if var.dim() == 1 else var[:, c:c + K * d]
            self.mlpg_solve(grad_out[:, o:o + d], v, offs_dev, d, windows, rhs=True, out=z[:, :d], work=work)
            self.mlpg_apply(z[:, :d], v, offs_dev, d, windows, out=g[:, c:c + K * d])
            o += d
        return g

    def _mlpg_f64(self, t, width, what, total):
        o64, ld = self._mlpg_operand(t, width, what, total)
        if not o64:
            raise TypeError("%s must be float64" % what)
        return ld

    def mlpg_column_sums(self, x, sums=None):
        """ONE mpx_mlpg_column_sums call (k_mlpg_colsum_tiles, k_mlpg_colsum_final): the column sums of a float64
        [total x width] device matrix in a fixed order (tiles of 128 rows, then the tiles) -> float64 [width]."""
        torch = _torch()
        total, width = int(x.shape[0]), int(x.shape[1])
        ld = self._mlpg_f64(x, width, "mlpg: x", total)
        if sums is None:
            sums = torch.zeros(width, dtype=torch.float64, device=self.device)
        if sums.dtype != torch.float64 or int(sums.numel()) != width or not sums.is_contiguous():
            raise ValueError("mlpg: sums must be %d contiguous float64" % width)
        work = torch.empty(int(self.lib.mpx_mlpg_colsum_work_doubles(total, width)), dtype=torch.float64,
                           device=self.device)
        self.launch("mpx_mlpg_column_sums", x, ld, total, width, sums, work)
        return sums

    def mlpg_var_backward(self, z, c, mean, var, offs_dev, D, windows, out=None, gsum=None):
        """ONE mpx_mlpg_var_backward call (k_mlpg_var_bwd; with a global variance also the column pass): the gradient of a
        loss on the trajectory with respect to the variances, -p^2 (W_k z)(mu_k - W_k c), for z = A^-1 dL/dc and the
        trajectory c (float64 [total x D]), mean and var as mlpg_solve takes them.  -> (float64 [total x K D], float64
        [K D] column sums with a global variance, else None)."""
        torch = _torch()
        total, K = int(mean.shape[0]), int(windows.shape[0]) + 1
        ld_z = self._mlpg_f64(z, D, "mlpg: z", total)
        ld_c = self._mlpg_f64(c, D, "mlpg: c", total)
        m64, ld_m = self._mlpg_operand(mean, K * D, "mlpg: mean", total)
        v64, ld_v = self._mlpg_var(var, K * D, total)
        if out is None:
            out = torch.empty((total, K * D), dtype=torch.float64, device=self.device)
        ld_o = self._mlpg_f64(out, K * D, "mlpg: g", total)
        work = None
        if ld_v == 0:
            if gsum is None:
                gsum = torch.zeros(K * D, dtype=torch.float64, device=self.device)
            if gsum.dtype != torch.float64 or int(gsum.numel()) != K * D or not gsum.is_contiguous():
                raise ValueError("mlpg: gsum must be %d contiguous float64" % (K * D))
            work = torch.empty(int(self.lib.mpx_mlpg_colsum_work_doubles(total, K * D)), dtype=torch.float64,
                               device=self.device)
        else:
            gsum = None
        wins = (ctypes.c_double * windows.size)(*[float(v) for v in windows.reshape(-1)])
        self.launch("mpx_mlpg_var_backward", z, ld_z, c, ld_c, mean, m64, ld_m, var, v64, ld_v, offs_dev,
                    int(offs_dev.numel()) - 1, total, int(D), K - 1, wins, out, ld_o, gsum, work)
        return out, gsum

    def mlpg_trajectory_nll(self, c, x, var, offs_dev, D, windows):
        """ONE mpx_mlpg_trajectory_nll launch (k_mlpg_nll): -log N(x; c, A^-1) per system for the trajectory c (float64
        [total x D], of mlpg_solve on the same variances) and the static target x (float32 / float64 [total x D]).
        -> float64 [n_utts x D]; 0 for an utterance without frames."""
        torch = _torch()
        total, K, n_utts = int(c.shape[0]), int(windows.shape[0]) + 1, int(offs_dev.numel()) - 1
        ld_c = self._mlpg_f64(c, D, "mlpg: c", total)
        x64, ld_x = self._mlpg_operand(x, D, "mlpg: x", total)
        v64, ld_v = self._mlpg_var(var, K * D, total)
        nll = torch.zeros((n_utts, D), dtype=torch.float64, device=self.device)
        wins = (ctypes.c_double * windows.size)(*[float(v) for v in windows.reshape(-1)])
        self.launch("mpx_mlpg_trajectory_nll", c, ld_c, x, x64, ld_x, var, v64, ld_v, offs_dev, n_utts, total, int(D),
                    K - 1, wins, nll)
        return nll

    def mlpg_trajectory_nll_backward(self, mean, var, c, x, go, offs_dev, D, windows, need_mean=True, need_var=True):
        """ONE mpx_mlpg_trajectory_nll_backward launch (k_mlpg_nll_bwd; with a global variance also
        mpx_mlpg_column_sums): the gradients of sum go * nll (go: float64 [n_utts x D]) with respect to the means and the
        variances.  -> (g_mean float64 [total x K D] or None, g_var: float64 [total x K D] for per-frame variances, [K D]
        for a global row, or None)."""
        torch = _torch()
        total, K, n_utts = int(mean.shape[0]), int(windows.shape[0]) + 1, int(offs_dev.numel()) - 1
        m64, ld_m = self._mlpg_operand(mean, K * D, "mlpg: mean", total)
        v64, ld_v = self._mlpg_var(var, K * D, total)
        ld_c = self._mlpg_f64(c, D, "mlpg: c", total)
        x64, ld_x = self._mlpg_operand(x, D, "mlpg: x", total)
        if go.dtype != torch.float64 or tuple(go.shape) != (n_utts, D) or not go.is_contiguous():
            raise ValueError("mlpg: go must be a contiguous float64 [%d x %d] matrix" % (n_utts, D))
        if not (need_mean or need_var):
            return None, None
        g_mean = torch.empty((total, K * D), dtype=torch.float64, device=self.device) if need_mean else None
        g_var = torch.empty((total, K * D), dtype=torch.float64, device=self.device) if need_var else None
        work = torch.empty(int(self.lib.mpx_mlpg_nll_work_doubles(total, D)), dtype=torch.float64,
                           device=self.device) if need_var else None
        wins = (ctypes.c_double * windows.size)(*[float(v) for v in windows.reshape(-1)])
        self.launch("mpx_mlpg_trajectory_nll_backward", mean, m64, ld_m, var, v64, ld_v, c, ld_c, x, x64, ld_x, go, offs_dev,
                    n_utts, total, int(D), K - 1, wins, g_mean, K * D, g_var, K * D, work)
        if need_var and ld_v == 0:
            g_var = self.mlpg_column_sums(g_var)
        return g_mean, g_var

    def mlpg_streams_var_backward(self, grad_out, buf, out, var, offs_dev, streams, windows, width, need_mean=True):
        """mlpg_streams_backward with the variances' gradient as well: per stream z = A^-1 g, then P_k W_k z (need_mean)
        and mpx_mlpg_var_backward on z, the trajectory `out` (mlpg_streams' result) and the packed means `buf`.
        -> (float64 [total x width] or None, the variances' gradient: float64 [total x width] for per-frame variances,
        [width] for a global row); columns of no stream are zero."""
        torch = _torch()
        total, K = int(grad_out.shape[0]), int(windows.shape[0]) + 1
        covered = sum(K * d for _, d in streams) == width
        alloc = torch.empty if covered else torch.zeros
        g = alloc((total, width), dtype=torch.float64, device=self.device) if need_mean else None
        glob = var.dim() == 1
        gv = alloc((total, width), dtype=torch.float64, device=self.device)
        gsum = torch.zeros(width, dtype=torch.float64, device=self.device) if glob else None
        dmax = max(d for _, d in streams)
        z = torch.empty((total, dmax), dtype=torch.float64, device=self.device)
        work = torch.empty(int(self.lib.mpx_mlpg_work_doubles(total, dmax)), dtype=torch.float64, device=self.device)
        o = 0
        for c, d in streams:
            v = var[c:c + K * d] if glob else var[:, c:c + K * d]
            self.mlpg_solve(grad_out[:, o:o + d], v, offs_dev, d, windows, rhs=True, out=z[:, :d], work=work)
            if need_mean:
                self.mlpg_apply(z[:, :d], v, offs_dev, d, windows, out=g[:, c:c + K * d])
            self.mlpg_var_backward(z[:, :d], out[:, o:o + d], buf[:, c:c + K * d], v, offs_dev, d, windows,
                                   out=gv[:, c:c + K * d], gsum=gsum[c:c + K * d] if glob else None)
            o += d
        return g, (gsum if glob else gv)

    # ------------------------------------------------------------------ acoustic composition
    def cmp_pack(self, utts, dims):
        """The statics of a batch as ONE device matrix [sum F_i x sum dims] (streams side by side) and the row offsets
        int64 [n + 1].  utts: per utterance the list of [F_i x dims[s]] operands (hostmath.cmp_operand).  Host arrays go up
        in one copy (float64 unless all are float32); device tensors without a float64 one among them are gathered by
        mpx_rows_pack into float32 rows (three streams per launch; float16 / bfloat16 widen exactly); anything else is
        copied block by block into a float64 matrix, as mlpg_pack does."""
        torch = _torch()
        offs = np.concatenate(([0], np.cumsum([int(u[0].shape[0]) for u in utts]))).astype(np.int64)
        total, SD = int(offs[-1]), int(sum(dims))
        cols = np.concatenate(([0], np.cumsum(dims))).astype(int)
        flat = [m for u in utts for m in u]
        is_t = [torch.is_tensor(m) for m in flat]
        f64 = any((m.dtype == torch.float64) if t else (m.dtype == np.float64) for m, t in zip(flat, is_t))
        dt, ndt = (torch.float64, np.float64) if f64 else (torch.float32, np.float32)
        if total == 0:
            return torch.empty((0, SD), dtype=dt, device=self.device), offs
        if not any(is_t):
            host = np.concatenate([np.concatenate([np.asarray(m, dtype=ndt) for m in u], axis=1) for u in utts], axis=0)
            return self.to_device(host, ndt).view(total, SD), offs
        buf = torch.empty((total, SD), dtype=dt, device=self.device)
        if all(is_t) and not f64:
            for s0 in range(0, len(dims), 3):
                ss = range(s0, min(s0 + 3, len(dims)))
                self.pack_rows([[u[s] for u in utts] for s in ss], [buf[:, cols[s]:cols[s + 1]] for s in ss])
            return buf, offs
        for u, a, b in zip(utts, offs[:-1], offs[1:]):
            if b > a:
                for s, m in enumerate(u):
                    t = torch.is_tensor(m)
                    src = m.detach() if t else torch.from_numpy(np.ascontiguousarray(m, dtype=ndt))
                    buf[int(a):int(b), cols[s]:cols[s + 1]].copy_(src, non_blocking=t)
        return buf, offs

    @staticmethod
    def _cmp_layout_args(dims, windows):
        n_win = 0 if windows is None else int(windows.shape[0])
        wins = (ctypes.c_double * (3 * n_win))(*[float(v) for v in windows.reshape(-1)]) if n_win else None
        return (ctypes.c_int32 * len(dims))(*[int(d) for d in dims]), len(dims), n_win, wins

    def cmp_neighbours(self, v, offs_dev, out=None):
        """ONE mpx_cmp_voiced_neighbours launch (k_cmp_neighbours).  v: device float32 / float64 [total] (any element
        stride: a column of a matrix) or [total x 1]; voiced where v > 0.  -> int32 [2 x total]: row 0 the last voiced
        frame at or before each frame, row 1 the first at or after it (utterance-relative, -1: none)."""
        torch = _torch()
        if v.dim() == 2:
            v = v[:, 0]
        if v.dtype not in (torch.float32, torch.float64) or v.dim() != 1:
            raise TypeError("cmp_neighbours: a float32 / float64 vector expected")
        total = int(v.shape[0])
        if out is None:
            out = torch.empty((2, total), dtype=torch.int32, device=self.device)
        if out.dtype != torch.int32 or tuple(out.shape) != (2, total) or not out.is_contiguous():
            raise ValueError("cmp_neighbours: out must be a contiguous int32 [2 x %d]" % total)
        self.launch("mpx_cmp_voiced_neighbours", v, int(v.dtype == torch.float64), max(int(v.stride(0)), 1) if total > 1
                    else 1, offs_dev, int(offs_dev.numel()) - 1, total, out)
        return out

    def _cmp_norm(self, norm, W):
        if norm is None:
            return None, None
        torch = _torch()
        out = []
        for v in norm:
            v = self.to_device(v, np.float64) if isinstance(v, np.ndarray) else v.detach().to(torch.float64).contiguous()
            if v.dim() != 1 or int(v.numel()) != W:
                raise ValueError("cmp: mean and std are vectors of %d values" % W)
            out.append(v)
        return tuple(out)

    def cmp_compose(self, x, nb, offs_dev, dims, interp, vuv, windows, norm=None, unv_fill=0.0, zeros=False,
                    out=None, out_f64=False):
        """ONE mpx_cmp_compose launch (k_cmp_compose).  x: device [total x sum dims] statics (float32 / float64, any row
        pitch); nb: cmp_neighbours' table (None without a carried stream); dims: the streams' dimensions; interp: the
        carried stream or -1; windows: hostmath.mlpg_windows(...) or None (statics only); norm: (mean, std) float64 [W]
        (host or device) or None.  -> out, float32 (out_f64: float64) [total x W] (given: a view with unit column stride,
        written in place)."""
        torch = _torch()
        total, SD = int(x.shape[0]), int(sum(dims))
        x64, ld_x = self._mlpg_operand(x, SD, "cmp: x", total)
        c_dims, n_streams, n_win, wins = self._cmp_layout_args(dims, windows)
        W = (n_win + 1) * SD + int(bool(vuv))
        odt = torch.float64 if out_f64 else torch.float32
        if out is None:
            out = torch.empty((total, W), dtype=odt, device=self.device)
        if out.dtype != odt or out.dim() != 2 or tuple(out.shape) != (total, W) or (W > 1 and out.stride(1) != 1):
            raise ValueError("cmp: out must be a %s [%d x %d] matrix with unit column stride" % (odt, total, W))
        ld_o = int(out.stride(0)) if total > 1 else max(int(out.stride(0)), W)
        if nb is not None and (nb.dtype != torch.int32 or tuple(nb.shape) != (2, total) or not nb.is_contiguous()):
            raise ValueError("cmp: nb must be a contiguous int32 [2 x %d]" % total)
        mean, std = self._cmp_norm(norm, W)
        self.launch("mpx_cmp_compose", x, x64, ld_x, c_dims, n_streams, int(interp), int(bool(zeros)), float(unv_fill),
                    int(bool(vuv)), nb, offs_dev, int(offs_dev.numel()) - 1, total, n_win, wins, mean, std, out,
                    int(bool(out_f64)), ld_o)
        return out

    def cmp_compose_backward(self, grad_out, nb, offs_dev, dims, interp, vuv, windows, std=None):
        """ONE mpx_cmp_compose_backward launch (k_cmp_compose_bwd): grad_out float32 [total x W] (unit column stride) ->
        the gradient of the statics, float64 [total x sum dims]; unvoiced entries of the carried stream get exactly 0."""
        torch = _torch()
        total, SD = int(grad_out.shape[0]), int(sum(dims))
        c_dims, n_streams, n_win, wins = self._cmp_layout_args(dims, windows)
        W = (n_win + 1) * SD + int(bool(vuv))
        g64, ld_g = self._mlpg_operand(grad_out, W, "cmp: grad_out", total)
        if g64:
            raise TypeError("cmp: grad_out must be float32")
        if std is not None:
            std = self._cmp_norm((std,), W)[0]
        gx = torch.empty((total, SD), dtype=torch.float64, device=self.device)
        self.launch("mpx_cmp_compose_backward", grad_out, ld_g, c_dims, n_streams, int(interp), int(bool(vuv)), nb, offs_dev,
                    int(offs_dev.numel()) - 1, total, n_win, wins, std, gx, SD)
        return gx

    def cmp_column_moments(self, x, out=None):
        """ONE mpx_cmp_column_moments call (k_cmp_moment_tiles, k_cmp_moment_final): x device [total x W] (float32 /
        float64, any row pitch) -> float64 [1 + 2 W] = (count, column sums, centred sums of squares) in a fixed order."""
        torch = _torch()
        total, W = int(x.shape[0]), int(x.shape[1])
        x64, ld = self._mlpg_operand(x, W, "cmp: x", total)
        if out is None:
            out = torch.zeros(1 + 2 * W, dtype=torch.float64, device=self.device)
        if out.dtype != torch.float64 or int(out.numel()) != 1 + 2 * W or not out.is_contiguous():
            raise ValueError("cmp: out must be %d contiguous float64" % (1 + 2 * W))
        work = torch.empty(int(self.lib.mpx_cmp_moments_work_doubles(total, W)), dtype=torch.float64, device=self.device)
        self.launch("mpx_cmp_column_moments", x, x64, ld, total, W, out, work)
        return out

    def warp_mag_matrix(self, mag_dim, H, alpha, b_mag_fbank_mel=False):
        """Device-resident [mag_dim x H] matrix of the magnitude compression and the name of the C entry point that goes
        with it: the cepstral mel warp (la.sp_mel_warp, mpx_mel_warp) or the mel filter bank (la.sp_mel_warp_fbank,
        mpx_mel_warp_fbank)."""
        if b_mag_fbank_mel:
            return (self.constant(("w_fbank", int(mag_dim), H, float(alpha)),
                                  lambda: hm.warp_fbank_matrix(mag_dim, H, alpha)), "mpx_mel_warp_fbank")
        return (self.constant(("w_mag", int(mag_dim), H, float(alpha)), lambda: hm.warp_matrix(mag_dim, H, alpha)),
                "mpx_mel_warp")

    def mel_warp_feats(self, mag, real, imag, voi_host, fs, mag_dim, phase_dim, alpha_phase=None, b_mag_fbank_mel=False):
        """format_for_modelling's two warps (magphase.py:2504-2529) on device feature matrices [F x H] -> three device
        matrices [F x mag_dim], [F x phase_dim], [F x phase_dim]."""
        F, H = int(mag.shape[0]), int(mag.shape[1])
        alpha = hm.define_alpha(fs)
        a_ph = alpha if alpha_phase is None else alpha_phase
        cf, _ = hm.define_crossfade_params(fs)
        k_full = hm.get_num_full_mel_coeffs_from_num_phase_coeffs(cf, phase_dim, a_ph, fs)
        w_mag, warp_name = self.warp_mag_matrix(mag_dim, H, alpha, b_mag_fbank_mel)
        w_ph = self.constant(("w_ph", int(k_full), H, float(a_ph), int(phase_dim)),
                             lambda: hm.warp_matrix(k_full, H, a_ph, nrows=phase_dim))
        voi = self.to_device(np.asarray(voi_host, dtype=np.float64), np.float32)
        out = (self.empty((F, int(mag_dim))), self.empty((F, int(phase_dim))), self.empty((F, int(phase_dim))))
        self.launch(warp_name, F, H, mag, real, imag, None, None, None, w_mag, int(mag_dim), w_ph, int(phase_dim), voi,
                    out[0], out[1], out[2], self.feat_ld(mag, real, imag))
        return out

    def synth_comp_slots(self):
        torch = _torch()
        with torch.cuda.device(self.device):
            return int(self.lib.mpx_synth_comp_slots())

    def synthesis_lossless_ola(self, fft_len, mag, real, imag, plan, strips, pcm_out):
        """plan: LosslessSynthesisPlan (run + slot tables resident on this device).  Writes every output sample of
        pcm_out once and the runs' head strips; ola_fixup(plan, strips, pcm_out) completes the run boundaries."""
        self.launch("mpx_synthesis_lossless_ola", int(fft_len), self.tables(fft_len), mag, real, imag, plan.runs,
                    int(plan.n_runs), plan.slot_off, plan.slot_runs, int(plan.n_slots), plan.pm_rel, strips, pcm_out,
                    self.feat_ld(mag, real, imag))
        return pcm_out

    def synthesis_lossless_ola_lerp(self, fft_len, mag, real, imag, rows, plan, strips, pcm_out):
        """synthesis_lossless_ola with row tables (mpx_synthesis_lossless_ola_lerp): rows = (row0, row1, rowt) device
        tensors, one entry per frame of plan; frame f's feature row is the interpolation of two rows of mag / real / imag."""
        r0, r1, rt = rows
        self.launch("mpx_synthesis_lossless_ola_lerp", int(fft_len), self.tables(fft_len), mag, real, imag, r0, r1, rt,
                    plan.runs, int(plan.n_runs), plan.slot_off, plan.slot_runs, int(plan.n_slots), plan.pm_rel, strips,
                    pcm_out, self.feat_ld(mag, real, imag))
        return pcm_out

    def rows_lerp(self, src, rows, n_out, out=None):
        """mpx_rows_lerp: src = (mag, real, imag) device rows, rows = (row0, row1, rowt) device tables of n_out entries ->
        (mag, real, imag) [n_out x H], out[c] = (1 - rowt[c]) src[row0[c]] + rowt[c] src[row1[c]]."""
        H = int(src[0].shape[1])
        if out is None:
            out = tuple(self.empty_feats(int(n_out), H) for _ in range(3))
        if n_out == 0:
            return out
        r0, r1, rt = rows
        self.launch("mpx_rows_lerp", H, src[0], src[1], src[2], self.feat_ld(*src), r0, r1, rt, int(n_out), out[0], out[1],
                    out[2], self.feat_ld(*out))
        return out

    def synthesis_lossless_backward(self, fft_len, grad_out, plan, mag, real, imag, need=(True, True, True), rows=None):
        """mpx_synthesis_lossless_backward: grad_out float32 [plan.total_out] (contiguous) = dL/d(the plan's waveform),
        plan: LosslessSynthesisPlan, mag / real / imag: the forward's rows -> (g_mag, g_real, g_imag), per-FRAME gradient
        rows [plan.total_frames x H] (None where need[k] is false: not computed).  rows = (row0, row1, rowt): the forward ran
        with row tables (synthesis_lossless_ola_lerp); rows_lerp_adjoint folds the result back onto the table's rows."""
        H = int(fft_len) // 2 + 1
        nfr = int(plan.total_frames)
        if int(grad_out.numel()) != int(plan.total_out) or grad_out.dtype != _torch().float32 or not grad_out.is_contiguous():
            raise ValueError("synthesis_lossless_backward: grad_out must be a contiguous float32 [%d]" % plan.total_out)
        out = tuple(self.empty_feats(nfr, H) if n else None for n in need)
        if nfr == 0 or not any(need):
            return out
        pos, lo, hi = plan.backward_tables()
        r0, r1, rt = rows if rows is not None else (None, None, None)
        first = next(o for o in out if o is not None)   # (empty_feats: one pitch for all)
        ld_g = self.feat_ld(first, first, first)
        self.launch("mpx_synthesis_lossless_backward", int(fft_len), self.tables(fft_len), grad_out, int(plan.total_out), pos,
                    lo, hi, nfr, mag, real, imag, self.feat_ld(mag, real, imag), r0, r1, rt, out[0], out[1], out[2], ld_g)
        return out

    def analysis_lossless_backward(self, fft_len, plan, mag, real, imag, grads):
        """mpx_analysis_lossless_backward: plan: LosslessAnalysisPlan (or a plans.FrameTable: pos / left / right,
        total_frames, total_smpls, backward_tables()), mag / real / imag: the rows its run() returned,
        grads = (g_mag, g_real, g_imag): float32 [plan.total_frames x H] rows with unit column stride and one row pitch, or
        None for an output nobody differentiated (not read, contributes zero) -> dL/d(samples), float32
        [plan.total_smpls] (zeros where no frame covers a sample, or when nothing is given)."""
        torch = _torch()
        H = int(fft_len) // 2 + 1
        nfr, total = int(plan.total_frames), int(plan.total_smpls)
        have = [g for g in grads if g is not None]
        for g in have:
            if g.dtype != torch.float32 or tuple(g.shape) != (nfr, H):
                raise ValueError("analysis_lossless_backward: gradients must be float32 [%d x %d]" % (nfr, H))
        if nfr == 0 or total == 0 or not have:
            return torch.zeros((total,), dtype=torch.float32, device=self.device)
        soff, scratch_floats = plan.backward_tables()
        scratch = self.empty((max(scratch_floats, 1),))
        out = self.empty((total,))
        self.launch("mpx_analysis_lossless_backward", int(fft_len), self.tables(fft_len), mag, real, imag,
                    self.feat_ld(mag, real, imag), grads[0], grads[1], grads[2], self.feat_ld(*(have * 3)[:3]),
                    plan.pos, plan.left, plan.right, soff, nfr, scratch, scratch_floats, out, total)
        return out

    def analysis_lossless_const_rate_backward(self, fft_len, plan, mag, real, imag, grads, ranges, rowt):
        """mpx_analysis_lossless_const_rate_backward (the one place that launches it): analysis_lossless_backward for
        gradients given on the CONSTANT-rate rows that mpx_rows_lerp made of plan's rows.  mag / real / imag: the
        variable-rate rows plan.run() returned; grads = (g_mag, g_real, g_imag): float32 [n_const_rows x H] with unit
        column stride and one row pitch, or None (not read, contributes zero); ranges: device int32 [plan.total_frames x 4]
        (hostmath.lerp_adjoint_table over the variable frames), rowt: device float32 [n_const_rows] -> dL/d(samples),
        float32 [plan.total_smpls].  The frame kernel forms every frame's gradient row as it loads it: no
        [total_frames x H] gradient rows, no mpx_rows_lerp_adjoint launch, the same bits as the two calls."""
        torch = _torch()
        H = int(fft_len) // 2 + 1
        nfr, total = int(plan.total_frames), int(plan.total_smpls)
        have = [g for g in grads if g is not None]
        n_const = int(have[0].shape[0]) if have else 0
        for g in have:
            if g.dtype != torch.float32 or tuple(g.shape) != (n_const, H) or g.stride(1) != 1:
                raise ValueError("analysis_lossless_const_rate_backward: gradients must be float32 [%d x %d]" % (n_const, H))
        if have and int(rowt.shape[0]) != n_const:
            raise ValueError("analysis_lossless_const_rate_backward: %d gradient rows, rowt has %d"
                             % (n_const, int(rowt.shape[0])))
        if nfr == 0 or total == 0 or n_const == 0:
            return torch.zeros((total,), dtype=torch.float32, device=self.device)
        if int(ranges.numel()) != 4 * nfr:
            raise ValueError("analysis_lossless_const_rate_backward: ranges must hold 4 entries per frame")
        soff, scratch_floats = plan.backward_tables()
        scratch = self.empty((max(scratch_floats, 1),))
        out = self.empty((total,))
        self.launch("mpx_analysis_lossless_const_rate_backward", int(fft_len), self.tables(fft_len), mag, real, imag,
                    self.feat_ld(mag, real, imag), grads[0], grads[1], grads[2], self.feat_ld(*(have * 3)[:3]), n_const,
                    ranges, rowt, plan.pos, plan.left, plan.right, soff, nfr, scratch, scratch_floats, out, total)
        return out

    def rows_lerp_adjoint(self, src, ranges, rowt, n_rows):
        """mpx_rows_lerp_adjoint: src = (g_mag, g_real, g_imag) per-frame rows (None: stream not wanted), ranges int32
        [n_rows x 4] (hostmath.lerp_adjoint_table) and rowt on the device -> the gradients of the n_rows table rows, a
        tuple with None where src has None.  Rows no frame reads are zero."""
        have = [s for s in src if s is not None]
        if not have:
            return (None, None, None)
        H = int(have[0].shape[1])
        out = tuple(self.empty_feats(int(n_rows), H) if s is not None else None for s in src)
        if int(n_rows) == 0:
            return out
        first = next(o for o in out if o is not None)
        self.launch("mpx_rows_lerp_adjoint", H, src[0], src[1], src[2], self.feat_ld(have[0], have[0], have[0]),
                    ranges, rowt, int(n_rows), out[0], out[1], out[2], self.feat_ld(first, first, first))
        return out

    def phase_grad_mask(self, out_real, out_imag, voi, g_real, g_imag):
        """mpx_phase_grad_mask: the upstream gradients g_real / g_imag (contiguous float32 [F x phase_dim], or None) of the
        compressed analysis' phase streams through its voicing mask and clip, read from the forward's own outputs
        out_real / out_imag and voi [F] -> (h_real, h_imag), None where g is None."""
        have = [g for g in (g_real, g_imag) if g is not None]
        if not have:
            return (None, None)
        F, pd = int(out_real.shape[0]), int(out_real.shape[1])
        for g in have:
            if g.dtype != _torch().float32 or tuple(g.shape) != (F, pd) or not g.is_contiguous():
                raise ValueError("phase_grad_mask: gradients must be contiguous float32 [%d x %d]" % (F, pd))
        h = tuple(self.empty((F, pd)) if g is not None else None for g in (g_real, g_imag))
        self.launch("mpx_phase_grad_mask", F, pd, voi, out_real, out_imag, g_real, g_imag, h[0], h[1])
        return h

    def mel_warp_backward(self, n_bins, mag=None, phase=None, out=None):
        """mpx_mel_warp_backward (k_mel_warp_bwd), its one caller: grad_x = d(x~) * (g . W) for up to three jobs in one launch.
        mag = (g [rows x mag_dim], w_mag [mag_dim x n_bins], x rows, rows_tables) or None, rows_tables = (row0, row1, rowt)
        device tables of `rows` entries (x~ interpolated as the forward does) or None (x~ = the rows of x);
        phase = (h_real, h_imag, w_phase [phase_dim x n_bins], x_real, x_imag, live) or None: h already masked
        (phase_grad_mask), either may be None, live = float32 [rows] flags or None.
        g / h: contiguous float32; x: feature rows of one pitch (unit column stride).  out: (grad_mag, grad_real, grad_imag)
        to write into (None where a job does not run; rows of one pitch), allocated when not given.
        Returns (grad_mag, grad_real, grad_imag), [rows x n_bins] each, None for a job that did not run."""
        torch = _torch()
        H = int(n_bins)

        def dense(g, n_out, what):
            if g.dtype != torch.float32 or g.dim() != 2 or int(g.shape[1]) != n_out or not g.is_contiguous():
                raise ValueError("mel_warp_backward: %s must be a contiguous float32 [rows x %d]" % (what, n_out))
            return int(g.shape[0])

        args_m = [None, None, 0, None, 0, None, None, None]
        args_p = [None, None, None, 0, None, None, 0, None]
        rows_m = rows_p = 0
        xs = []
        if mag is not None:
            g, w, x, tabs = mag
            rows_m = dense(g, int(w.shape[0]), "g_mag")
            r0, r1, rt = tabs if tabs is not None else (None, None, None)
            args_m = [g, w, int(w.shape[0]), x, rows_m, r0, r1, rt]
            xs.append(x)
        want_r = want_i = False
        if phase is not None:
            hr, hi, w, xr, xi, live = phase
            for h in (hr, hi):
                if h is not None:
                    rows_p = dense(h, int(w.shape[0]), "h_real / h_imag")
            want_r, want_i = hr is not None, hi is not None
            args_p = [hr, hi, w, int(w.shape[0]), xr if want_r else None, xi if want_i else None, rows_p, live]
            xs += [x for x, k in ((xr, want_r), (xi, want_i)) if k]
        want = (mag is not None, want_r, want_i)
        if out is None:
            out = tuple(self.empty_feats(rows_m if k == 0 else rows_p, H) if w_ else None for k, w_ in enumerate(want))
        if not xs:
            return out
        outs = [o for o in out if o is not None]
        for t in xs + outs:
            if int(t.shape[1]) != H:
                raise ValueError("mel_warp_backward: rows must have %d bins" % H)
        self.launch("mpx_mel_warp_backward", H, *args_m, out[0], *args_p, out[1], out[2],
                    self.feat_ld(*(xs * 3)[:3]), self.feat_ld(*(outs * 3)[:3]))
        return out

    def roundtrip_lossless_ola(self, fft_len, plan_a, plan_s, feats, strips, pcm_out, full_support=False, stores="lines_nt",
                               inverse="direct"):
        """Copy synthesis in one launch (mpx_roundtrip_lossless_ola_flags): plan_a's frames are analysed, their feature rows
        written to feats = (mag, real, imag) and overlap-added by plan_s' runs (a LosslessSynthesisPlan built for this
        kernel's slots from plan_a's v_f0); ola_fixup(plan_s, strips, pcm_out) completes the run boundaries.
        full_support: every frame takes the full support class (MPX_RT_FULL_SUPPORT).  stores: "rows", "lines" or
        "lines_nt" -- how the N = 4096 compact-support instance stores the feature rows (MPX_RT_STORE_*; the same values).
        inverse: "direct" -- at N = 4096 the windowed frame itself is overlap-added, which is what the merge and the inverse
        transform of its own spectrum rebuild -- or "transform" (MPX_RT_INVERSE_TRANSFORM); every other N transforms."""
        mag, real, imag = feats
        if stores not in _lib.RT_STORE_FLAGS:
            raise ValueError("roundtrip_lossless_ola: stores must be one of %s" % ", ".join(sorted(_lib.RT_STORE_FLAGS)))
        if inverse not in _lib.RT_INVERSE_FLAGS:
            raise ValueError("roundtrip_lossless_ola: inverse must be one of %s" % ", ".join(sorted(_lib.RT_INVERSE_FLAGS)))
        self.launch("mpx_roundtrip_lossless_ola_flags", int(fft_len), self.tables(fft_len), plan_a.sig, plan_a.pos, plan_a.left,
                    plan_a.right, int(plan_a.total_frames), plan_s.runs, int(plan_s.n_runs), plan_s.slot_off,
                    plan_s.slot_runs, int(plan_s.n_slots), plan_s.pm_rel, mag, real, imag, strips, pcm_out,
                    self.feat_ld(mag, real, imag), (1 if full_support else 0) | _lib.RT_STORE_FLAGS[stores] | _lib.RT_INVERSE_FLAGS[inverse])
        return pcm_out

    def griffin_lim_ola(self, fft_len, plan, target, sig_in, sig_out, strips, phase_out=None):
        """One Griffin-Lim iteration (mpx_griffin_lim_ola): plan (GriffinLimPlan) frames of sig_in analysed, magnitudes
        replaced by target's rows, overlap-added into sig_out by plan.iter's runs; ola_fixup(plan.iter, ...) afterwards."""
        it = plan.iter
        self.launch("mpx_griffin_lim_ola", int(fft_len), self.tables(fft_len), sig_in, plan.frame_pos, plan.frame_left,
                    plan.frame_right, int(plan.total_frames), target, it.runs, int(it.n_runs), it.slot_off, it.slot_runs,
                    int(it.n_slots), plan.pm_rel, phase_out, strips, sig_out, int(target.stride(0)))
        return sig_out

    GL_FOLD_FORMS = {"half": 0, "full": 1, "words": 2}   # MPX_GL_FOLD_HALF / _FULL / _WORDS

    def griffin_lim_fold(self, fft_len, form, target, phase, frame0, n_frames, outs, phase_out=None, phase_offset=0):
        """hostmath.griffin_lim_fold on the device (mpx_griffin_lim_fold, k_gl_fold) for rows frame0 .. frame0 + n_frames - 1
        of target (device magnitude rows [F x H]) into the same rows of outs = (mag', phasor real, phasor imag) and, if
        given, of phase_out -- all of target's row pitch.  form 'half' / 'full': phase is a float32 device matrix
        [n_frames x H] / [n_frames x fft_len] (unit column stride) whose row 0 belongs to frame0; 'words': the int32 words of
        numpy_global_words, the range's first sample at sample phase_offset."""
        torch = _torch()
        ld = int(target.stride(0)) if target.shape[0] > 1 else max(int(target.stride(0)), int(target.shape[1]))
        for t in tuple(outs) + ((phase_out,) if phase_out is not None else ()):
            if t.dtype != torch.float32 or t.shape != target.shape or (t.shape[0] > 1 and int(t.stride(0)) != ld):
                raise ValueError("griffin_lim_fold: the outputs must be float32 rows of the target's shape and pitch")
        if form == "words":
            if phase.dtype != torch.int32 or phase.dim() != 1 or not phase.is_contiguous():
                raise ValueError("griffin_lim_fold: words must be a contiguous int32 vector")
            if 2 * (int(phase_offset) + int(n_frames) * int(fft_len)) > phase.numel():
                raise ValueError("griffin_lim_fold: the words do not cover the frames")
            ptr, ld_phase = phase.data_ptr() + 8 * int(phase_offset), 0
        else:
            width = int(fft_len) if form == "full" else int(fft_len) // 2 + 1
            if (phase.dtype != torch.float32 or phase.dim() != 2 or phase.shape[0] < n_frames or phase.shape[1] != width
                    or phase.stride(1) != 1):
                raise ValueError("griffin_lim_fold: phase must be float32 [n_frames x %d] with unit column stride" % width)
            ptr, ld_phase = phase.data_ptr(), max(int(phase.stride(0)), width) if phase.shape[0] > 1 else width
        if target.dtype != torch.float32 or target.dim() != 2 or target.shape[1] != int(fft_len) // 2 + 1:
            raise ValueError("griffin_lim_fold: target must be float32 [F x fft_len / 2 + 1]")
        if frame0 < 0 or n_frames < 0 or frame0 + n_frames > target.shape[0]:
            raise ValueError("griffin_lim_fold: frames %d .. %d of %d" % (frame0, frame0 + n_frames, target.shape[0]))
        self.launch("mpx_griffin_lim_fold", int(fft_len), self.GL_FOLD_FORMS[form], target, ptr, ld_phase, int(frame0),
                    int(n_frames), outs[0], outs[1], outs[2], phase_out, ld)

    def ola_fixup(self, fft_len, plan, strips, pcm_out):
        """Completes the run boundaries; a run table that knows its widest fix range (fix_width: the round-trip plan's
        seams by frame extents, plans._SeamRuns) gets a launch sized by it (mpx_ola_fixup_width)."""
        width = getattr(plan, "fix_width", None)
        if width is None:
            self.launch("mpx_ola_fixup", int(fft_len), plan.runs, int(plan.n_runs), strips, pcm_out)
        else:
            self.launch("mpx_ola_fixup_width", int(fft_len), plan.runs, int(plan.n_runs), strips, pcm_out, int(width))
        return pcm_out


class _Prepared:
    """Host side of one launch, built by Engine.prepare_* (possibly on the planner thread): page-locked slot filled, tables
    ready; the plan constructor uploads it.  release(): hands the slot back when the launch is not going to happen."""
    slot = None
    engine = None

    def release(self):
        if self.slot is not None:
            slot, self.slot = self.slot, None
            self.engine._slot_release(slot)

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class PreparedAnalysis(_Prepared):
    pass


class PreparedSynthesis(_Prepared):
    pass


_ENGINES = {}


def get_engine(device=None):
    torch = _torch()
    if device is None:
        if not torch.cuda.is_available():
            return Engine()  # raises the loud error
        device = torch.device("cuda", torch.cuda.current_device())
    key = str(device)
    if key not in _ENGINES:
        _ENGINES[key] = Engine(device)
    return _ENGINES[key]


# ======================================================================================================
# Compatibility surface: what callers have always reached through this module and now lives elsewhere
# (inside the package, import these from the module that defines them)
# ======================================================================================================
from .hostmath import (_const_rate_f0_voi, _const_to_variable_scan_scipy, _first_all_zero_from,   # noqa: E402,F401
                       check_const_rate_ms, const_to_variable_rows)
from .hostplan import (_const_to_variable_scan, const_to_variable_scan_uncapped,   # noqa: E402,F401
                       plan_const_rate_synthesis, plan_synthesis_numpy)
from .plans import (TYPE2_ENV_NCOEFFS, TYPE2_ENV_THRES_DB, CompressedAnalysisPlan,   # noqa: E402,F401
                    CompressedSynthesisPlan, GriffinLimPlan, LosslessAnalysisPlan, LosslessConstRateAnalysisPlan,
                    LosslessConstRateSynthesisPlan, LosslessRoundTripPlan, LosslessSynthesisPlan, Type2AnalysisPlan,
                    Type2CompressedAnalysisPlan, Type2SynthesisPlan)
