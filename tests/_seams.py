"""
Shared by the tests of the run seams sized by frame extents (hostmath.ola_runs(extents=) / mpx_host_ola_runs_extents):
a brute-force numpy model of what the pair kernel and k_ola_fixup do with a run table when every frame adds only the
samples inside its extent, the seam kinds a run table contains, the round-trip test batch, and an engine that builds
plans on a box without a GPU.
"""
import numpy as np

FS = 48000
NARROW = (1536, 2560)     # what a class-4 frame adds at N = 4096 (rows 12 .. 19 of 128 samples)


def emulate_runs(runs, rels, ext, frames, N, starts, lens, out_off):
    """The planner's runs on frames that are non-zero only inside their extents (include/magphase_hip.h: mpx_ola_run).
    Per run the frames are summed at their strip positions; elements below flush_end are streamed out: e < head_end to
    the head strip, out_lo <= e < out_hi to pcm_out, the rest nowhere.  pcm_out and the strips start as NaN.  Asserted:
    nothing a frame touched stays in the ring, no touched element of the kept part is sent nowhere or left in a strip the
    fix-up does not read, every kept sample is written exactly once, the fix-up reads only strip elements that were
    written and adds them inside their utterance.  Returns pcm_out."""
    allrel = np.concatenate(rels)
    frame_off = np.concatenate(([0], np.cumsum([len(r) for r in rels])))
    total_out = int(out_off[-1])
    pcm = np.full(total_out, np.nan)
    writes = np.zeros(total_out, dtype=int)
    strips = np.full((len(runs), N + 64), np.nan)
    for ri, r in enumerate(runs):
        fb, fe, x0 = int(r["frame_begin"]), int(r["frame_end"]), int(r["x0"])
        u = int(np.searchsorted(frame_off, fb, side="right") - 1)
        assert fe > fb and fe <= frame_off[u + 1]
        fl = int(r["flush_end"])
        span = max(fl, int(allrel[fe - 1]) - x0 + N) + 64
        acc, touched = np.zeros(span), np.zeros(span, dtype=bool)
        for f in range(fb, fe):
            x = int(allrel[f]) - x0
            assert x >= 0                                   # the kernel's strip position of a frame is not negative
            lo_e, hi_e = int(ext[f, 0]), int(ext[f, 1])
            acc[x + lo_e:x + hi_e] += frames[f, lo_e:hi_e]
            touched[x + lo_e:x + hi_e] = True
        assert not touched[fl:].any()                       # the ring ends up cleared
        he, lo, hi = int(r["head_end"]), int(r["out_lo"]), int(r["out_hi"])
        assert 0 <= he <= N + 64 and int(r["out_base"]) % 64 == 0 and int(r["strip_off"]) == ri * (N + 64)
        strips[ri, :min(he, fl)] = acc[:min(he, fl)]
        if hi > lo:
            assert 0 <= lo and hi <= fl
            idx = int(r["out_base"]) + np.arange(lo, hi)
            assert idx[0] >= out_off[u] and idx[-1] < out_off[u + 1]
            pcm[idx] = acc[lo:hi]
            writes[idx] += 1
        e = np.arange(fl)
        kept = (e + x0 >= starts[u]) & (e + x0 < starts[u] + lens[u])
        nowhere = (e >= he) & ~((e >= lo) & (e < hi))
        assert not (nowhere & touched[:fl] & kept).any(), "run %d drops a sample a frame added" % ri
        unread = (e < he) & ~((e >= int(r["fix_lo"])) & (e < int(r["fix_hi"])))
        assert not (unread & touched[:fl] & kept).any(), "run %d: a strip element a frame added is never fixed up" % ri
    assert np.all(writes == 1)
    for ri, r in enumerate(runs):       # fix-up: predecessor's sum (in pcm) + head strip
        lo, hi = int(r["fix_lo"]), int(r["fix_hi"])
        if hi > lo:
            u = int(np.searchsorted(frame_off, int(r["frame_begin"]), side="right") - 1)
            assert 0 <= lo and hi <= int(r["head_end"])
            vals = strips[ri, lo:hi]
            assert not np.isnan(vals).any(), "run %d: the fix-up reads a strip element nobody wrote" % ri
            idx = int(r["out_base"]) + np.arange(lo, hi)
            assert idx[0] >= out_off[u] and idx[-1] < out_off[u + 1]
            pcm[idx] += vals
    assert not np.isnan(pcm).any()
    return pcm


def direct_ola(rels, ext, frames, N, starts, lens):
    """The plain overlap-add of the same frames, utterance by utterance, trimmed to the kept part."""
    out, f0 = [], 0
    for u, rel in enumerate(rels):
        # (the reference's buffer is pm[-1] + N long in absolute positions: the kept part may lie past the last frame)
        buf = np.zeros(max((int(rel[-1]) if len(rel) else 0) + N, starts[u] + lens[u]))
        for i, p in enumerate(rel):
            lo_e, hi_e = int(ext[f0 + i, 0]), int(ext[f0 + i, 1])
            buf[int(p) + lo_e:int(p) + hi_e] += frames[f0 + i, lo_e:hi_e]
        out.append(buf[starts[u]:starts[u] + lens[u]])
        f0 += len(rel)
    return np.concatenate(out) if out else np.zeros(0)


def check_runs(runs, rels, ext, N, starts, lens, out_off, seed=0):
    """emulate_runs on random frame values == direct_ola (to rounding: the two sum in another order)."""
    ext = np.asarray(ext).reshape(-1, 2)
    frames = np.random.RandomState(seed).uniform(0.5, 1.5, (ext.shape[0], N))    # no zeros inside an extent
    got = emulate_runs(runs, rels, ext, frames, N, starts, lens, out_off)
    ref = direct_ola(rels, ext, frames, N, starts, lens)
    assert got.shape == ref.shape
    assert np.max(np.abs(got - ref), initial=0.0) < 1e-9
    return got


def seam_kinds(runs, rel_cat, ext, N, starts=None, lens=None):
    """The kinds of run boundaries in a run table, as a set of names:
    full-before / full-after : the predecessor's last / the successor's first frame is dense
    narrow-narrow            : both frames at the boundary are narrower than N
    inner-reach              : the predecessor's end is set by a frame that is not its last
    gap                      : what the successor's frames add begins at or past the predecessor's end (nothing to fix)
    clip-start / clip-end    : (with the utterances' starts / lens) a non-empty fix range that the kept part [start, start +
                               out_len) cuts at its beginning (x0 + fix_lo == start) / at its end (x0 + fix_hi == start +
                               out_len, below the head strip's end)"""
    ext = np.asarray(ext).reshape(-1, 2)
    full = (ext[:, 0] == 0) & (ext[:, 1] == N)
    kinds = set()
    u = 0
    for a, b in zip(runs[:-1], runs[1:]):
        if rel_cat[int(b["frame_begin"])] == 0:
            u += 1
            continue                       # first run of the next utterance (its first frame is at position 0)
        if starts is not None and int(b["fix_hi"]) > int(b["fix_lo"]):
            x0 = int(b["x0"])
            if x0 + int(b["fix_lo"]) == int(starts[u]):
                kinds.add("clip-start")
            if x0 + int(b["fix_hi"]) == int(starts[u]) + int(lens[u]) < x0 + int(b["head_end"]):
                kinds.add("clip-end")
        last, first = int(a["frame_end"]) - 1, int(b["frame_begin"])
        kinds.add("full-before" if full[last] else "narrow-before")
        kinds.add("full-after" if full[first] else "narrow-after")
        if not full[last] and not full[first]:
            kinds.add("narrow-narrow")
        reach = rel_cat[int(a["frame_begin"]):last + 1] + ext[int(a["frame_begin"]):last + 1, 1]
        if reach.max() > reach[-1]:
            kinds.add("inner-reach")
        begin = rel_cat[first:int(b["frame_end"])] + ext[first:int(b["frame_end"]), 0]
        if begin.min() >= int(b["x0"]) + int(b["head_end"]):
            kinds.add("gap")
    return kinds


def utt_from_gaps(gaps, seed, first=300):
    """Noise with an impulse at every epoch; the epochs `first`, first + gaps[0], ... (samples).  Frame i has
    L = the gap before epoch i and R = the gap after it (the first frame: L = first)."""
    pos = first + np.concatenate(([0], np.cumsum(gaps)))
    n = int(pos[-1]) + 700
    rng = np.random.RandomState(seed)
    x = 0.05 * rng.randn(n)
    x[pos] += 0.4
    pcm = np.round(np.clip(x, -0.99, 0.99) * 32767.0).astype(np.int16)
    return pcm, FS, (pos + 0.25) / FS, np.ones(pos.size)


SEAM_KINDS = {"full-before", "full-after", "narrow-narrow", "inner-reach", "gap", "clip-start", "clip-end"}
SEAM_BATCH_SEED = 1215


def seam_batch(seed=SEAM_BATCH_SEED):
    """Three utterances of 0.3 - 0.6 s at 48 kHz (N = 4096).  Each begins with its first epoch 20 - 60 samples into the
    recording and three periods of about 155 samples (a cut after one of the first frames leaves a seam the kept part's
    `start` clips), goes on with stretches of epochs around 240 samples apart (200 Hz: class 4, a frame adds 1024 samples)
    and around 800 apart (60 Hz, period > 512: the full class), short enough that runs of a dozen frames begin and end in
    either, with two pauses longer than a frame (a cut there is a gap of zeros), and ends with one low-pitched period and
    seven high-pitched ones (a cut inside them leaves a short last run after a dense frame: a seam that `start + out_len`
    clips).  Where the cuts fall is the dealing's decision: the seed is one for which every kind of SEAM_KINDS occurs in the
    round-trip plan's run table with 6 and with 12 slots, which the tests assert on the table; after a change of the
    dealing, take the first seed for which they hold again."""
    rng = np.random.RandomState(seed)

    def hi(n):
        return list(rng.randint(225, 256, n))

    def lo(n):
        return list(rng.randint(760, 840, n))

    def sh(n):
        return list(rng.randint(140, 171, n))

    utts = []
    for k in range(3):
        g = sh(3)
        for seg in range(rng.randint(3, 6)):
            g += hi(rng.randint(2, 14)) + lo(rng.randint(1, 4))
            if seg in (0, 2):
                g += [int(rng.randint(4200, 4500))]
        g += hi(rng.randint(3, 9)) + lo(1) + hi(7)
        utts.append(utt_from_gaps(np.asarray(g), 40 + k, first=int(rng.randint(20, 61))))
    return utts


def plan_seam_kinds(plan):
    """seam_kinds of a LosslessRoundTripPlan's own run table (plan.runs_host), with its frames' extents and kept parts."""
    s = plan.synthesis
    rel_cat = np.concatenate([np.asarray(r, dtype=np.int64) for r in s._ola_host[0]])
    return seam_kinds(plan.runs_host, rel_cat, plan._frame_extents(plan.total_frames), plan.fft_len, s._ola_host[1],
                      s._ola_host[2])


class HostEngine:
    """Stands in for engine.Engine on a box without a GPU, for plans that ask the library's host functions: descriptor
    tensors stay numpy arrays, the slot count is the caller's."""

    def __init__(self, n_slots=1536):
        from magphase_amd import _lib
        self.lib = _lib.load()
        self._n_slots = int(n_slots)

    def to_device(self, arr, dtype):
        return np.ascontiguousarray(arr, dtype=dtype)

    def to_device_packed(self, items):
        return {name: np.ascontiguousarray(arr, dtype=dt) for name, arr, dt in items}

    def synth_comp_slots(self):
        return self._n_slots

    def synth_ola_slot_weights(self, comp=False):
        w = np.zeros(self._n_slots, dtype=np.float32)
        assert self.lib.mpx_roundtrip_slot_weights(w.ctypes.data, self._n_slots) == 0
        return w


def fix_width(runs):
    """The widest fix range of a run table as k_ola_fixup walks it: from the 64-element block fix_lo lies in to fix_hi."""
    w = np.where(runs["fix_hi"] > runs["fix_lo"], runs["fix_hi"] - (runs["fix_lo"] & ~63), 0)
    return int(w.max()) if w.size else 0
