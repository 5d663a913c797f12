"""GPU: the kernels of the output stage, each through its C entry point against its reference of
tests/output_stage_model.py (checked on the CPU by tests/test_output_stage_host.py):

  k_hpf_zero_state, k_hpf_carry, k_hpf_apply     mpx_output_hpf vs the longdouble cascade hpf_cascade
  k_rows_gemm, k_merlin_r0, k_merlin_b           mpx_post_filter_merlin vs oracle.magphase_oracle.post_filter_merlin
  k_peak_abs, k_pcm16, k_pcm16_to_f32            mpx_pcm16, mpx_pcm16_to_f32 vs la.write_audio_file's operations, exactly

Every output lies inside a larger buffer filled with a sentinel, between two guards: whatever the entry is not documented
to write must still hold the sentinel afterwards.  Floating-point operands are uploaded between runs of NaN.  No
utterance, frame or sample is left out of a comparison.

High-pass: max |y - hpf_cascade| over the utterance, of the INPUT's peak (1; not divided by the output's peak), per
(design, fs) over seven batches of ten utterances (osm.HPF_INPUTS x osm.HPF_LENS).  Measured on the MI355X: 1.6e-10 at
48 kHz down to 4e-14 at 8 kHz, every case within 2.5 x (every single input within 4.6 x) the float64 emulation of the
same algorithm on the CPU (hpf_blocked; the table stands at TOL_HPF) -- four orders of magnitude below the 1e-6 that scipy's direct-form lfilter
could be held to.  Merlin: max |out - oracle| per dimension, beside the older MERLIN_PF_ABS of 3e-5.
The tolerances are <= 3 x the measured worst case (profiles/r20_output_stage_tolerance_report.json).
"""
import ctypes

import numpy as np
import pytest

import output_stage_model as osm
from _tol import note, within
from magphase_amd import _lib
from magphase_amd import hostmath as hm
from magphase_amd import libaudio as la

pytestmark = pytest.mark.gpu

LD = osm.LD
GUARD = 64         # elements before and after every output (keeps 128-byte alignment for every element size used)
SPARE = 192        # elements after the last one an entry may write, inside the guards
NAN_GUARD = 2112   # NaNs before and after every floating-point operand

# ---- measured on the MI355X against hpf_cascade (longdouble); every tolerance <= 3 x its worst case ----
# worst of the seven inputs (the corner sine at 44.1 / 48 kHz, the noise below); beside it hpf_blocked, the float64
# emulation of the same algorithm on the CPU, for the same batches (tests/test_output_stage_host.py prints every row)
#                                  tolerance     measured    hpf_blocked
TOL_HPF = {("butter40", 48000): 4.5e-10,      # 1.64e-10    2.16e-10
           ("butter40", 44100): 2.0e-10,      # 6.87e-11    2.84e-11
           ("butter40", 22050): 2.2e-12,      # 7.70e-13    1.13e-12
           ("butter40", 16000): 3.4e-13,      # 1.16e-13    2.62e-13
           ("butter40", 8000): 1.3e-13,       # 4.35e-14    5.74e-14
           ("ellip60", 48000): 5.5e-10,       # 1.88e-10    1.22e-10
           ("ellip60", 8000): 9.5e-14}        # 3.19e-14    5.63e-14
# max |out - oracle| of the Merlin post-filter per dimension; MERLIN_PF_ABS (D = 60 and 24 through the Python API) is 3e-5.
# Measured 1.29e-6, 9.54e-6, 1.14e-5, 9.39e-6: the constant -23 rows set it (a float32 ulp at 23 is 1.9e-6), a formant row
# alone (F = 1) is within 3.2e-6 at every D
TOL_MERLIN = {3: 3.5e-6, 24: 2.8e-5, 60: 3.0e-5, 64: 2.8e-5}
# |(r0[wk_2048 = W] - r0[wk_2048 = 0]) - W exp(2 (mcep g)[2048])| / r0[wk_2048 = W]: measured 2.29e-5 -- twice the error of
# the float32 mcep[0] (a 60-term product of |x| <= 23) that the exponent carries
TOL_MERLIN_MASK = 6.0e-5


def _engine():
    from magphase_amd.engine import get_engine
    return get_engine()


def _sync():
    import torch
    torch.cuda.synchronize()


def _dev(e, a, dtype):
    """Upload; floating-point operands lie between two runs of NAN_GUARD NaNs, so a read before or past an operand puts a
    NaN into the output instead of whatever the allocator left there."""
    import torch
    a = np.ascontiguousarray(a, dtype=dtype)
    if not np.issubdtype(a.dtype, np.floating):
        return torch.from_numpy(a.reshape(-1) if a.size else np.zeros(1, dtype)).to(e.device)
    buf = np.full(a.size + 2 * NAN_GUARD, np.nan, dtype=dtype)
    buf[NAN_GUARD:NAN_GUARD + a.size] = a.ravel()
    return torch.from_numpy(buf).to(e.device)[NAN_GUARD:NAN_GUARD + a.size]


class Fenced:
    """n elements an entry may write, then SPARE it may not, between two guards; everything pre-filled with the sentinel."""

    def __init__(self, e, n, dtype, sentinel=osm.SENTINEL):
        import torch
        self.n, self.sentinel = int(n), sentinel
        self.buf = torch.full((2 * GUARD + SPARE + self.n,), sentinel, dtype=dtype, device=e.device)
        self.ptr = self.buf[GUARD:].data_ptr()

    def check(self, what, all_written=True):
        """-> the n elements; the rest must hold the sentinel (all_written: and none of the n does)."""
        h = self.buf.cpu().numpy()
        assert np.all(h[:GUARD] == self.sentinel), what + ": written before the buffer"
        assert np.all(h[GUARD + self.n:] == self.sentinel), what + ": written past the last element"
        out = h[GUARD:GUARD + self.n].copy()
        if all_written:
            assert not np.any(out == self.sentinel), what + ": elements of the output not written"
        return out

    def untouched(self, what):
        assert np.all(self.buf.cpu().numpy() == self.sentinel), what + ": written"


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 2: np.uint16}[a.dtype.itemsize])


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------------------------------
# high-pass
# ---------------------------------------------------------------------------------------------------------------------
_HPF_TABLES = {}


def _hpf_tables(e, design, fs):
    key = (design, fs)
    if key not in _HPF_TABLES:
        assert int(e.lib.mpx_hpf_block()) == osm.HPF_BLOCK
        sos, pm, g = hm.hpf_tables(fs, osm.HPF_BLOCK, design)
        _HPF_TABLES[key] = (np.ascontiguousarray(sos, dtype=np.float64), _dev(e, pm, np.float64), _dev(e, g, np.float64))
    return _HPF_TABLES[key]


def _hpf(e, tabs, sigs, what):
    """One call of mpx_output_hpf on the utterances `sigs` (float32) -> float64 [total], every buffer checked."""
    import torch
    sos, d_pm, d_g = tabs
    lens = np.array([x.size for x in sigs], dtype=np.int64)
    off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    blk = osm.block_offsets(lens)
    total, tb = int(off[-1]), int(blk[-1])
    pcm = _dev(e, np.concatenate(sigs) if total else np.zeros(0, np.float32), np.float32)
    d_off, d_blk = _dev(e, off, np.int64), _dev(e, blk, np.int32)
    zend, zstart = Fenced(e, 2 * tb, torch.float64), Fenced(e, 2 * tb, torch.float64)
    y_tmp, y = Fenced(e, total, torch.float64), Fenced(e, total, torch.float64)
    e.launch("mpx_output_hpf", pcm, d_off, d_blk, int(lens.size), int(lens.max()), sos.ctypes.data_as(ctypes.c_void_p),
             d_pm, d_g, zend.ptr, zstart.ptr, y_tmp.ptr, y.ptr)
    _sync()
    zend.check(what + " zend")          # beyond blk_off[-1]: untouched
    zstart.check(what + " zstart")
    y_tmp.check(what + " y_tmp")
    out = y.check(what + " y")           # nothing outside [out_off[0], out_off[-1]), every sample inside written
    return out, off


@pytest.mark.parametrize("design,fs", osm.HPF_CASES)
def test_hpf_against_the_longdouble_cascade(design, fs):
    """Block edges (255-257), wave and carry-tile edges (16 383-16 385), a three-tile carry (49 153), a zero-length
    utterance between the others; noise, DC, impulses at both ends of a block, the Nyquist alternation, the corner sine, and
    DC with noise (large per-block zero-state responses the carries must cancel).  Every utterance also equals the same
    utterance launched alone, bit for bit: the scan is per utterance."""
    e = _engine()
    tabs = _hpf_tables(e, design, fs)
    worst = 0.0
    for name in osm.HPF_INPUTS:
        sigs, refs = osm.hpf_reference(design, fs, name)
        what = "hpf %s %d %s" % (design, fs, name)
        y, off = _hpf(e, tabs, sigs, what)
        assert np.all(np.isfinite(y)), what
        fig = 0.0
        for u, (x, ref) in enumerate(zip(sigs, refs)):
            yu = y[off[u]:off[u + 1]]
            if x.size:
                fig = max(fig, float(np.max(np.abs(yu.astype(LD) - ref))))
            alone, _ = _hpf(e, tabs, [x], what + " utterance %d alone" % u)
            assert _same_bits(alone, yu), what + ": utterance %d differs from the same utterance launched alone" % u
        print("%s: max |y - hpf_cascade| %.3g" % (what, fig))
        note("OS_HPF_DEVICE/%s/%d/%s" % (design, fs, name), fig)
        worst = max(worst, fig)
        within(fig, TOL_HPF[(design, fs)], "OS_HPF_%s_%d" % (design, fs))
    print("hpf %s %d: worst %.3g, tolerance %.3g" % (design, fs, worst, TOL_HPF[(design, fs)]))


def test_hpf_empty_batches_touch_nothing():
    e = _engine()
    tabs = _hpf_tables(e, "butter40", 48000)
    for sigs in ([np.zeros(0, np.float32)], [np.zeros(0, np.float32)] * 3):
        y, _ = _hpf(e, tabs, sigs, "hpf of empty utterances")
        assert y.size == 0


# ---------------------------------------------------------------------------------------------------------------------
# Merlin post-filter
# ---------------------------------------------------------------------------------------------------------------------
_MERLIN_DEV = {}
_MERLIN_KEYS = ("c1", "lifter", "g", "wk", "cf")


def _merlin_tables(e, dim, fs, pf):
    key = (dim, fs, pf)
    if key not in _MERLIN_DEV:
        t = hm.merlin_tables(dim, fs, pf)
        _MERLIN_DEV[key] = (t, {k: _dev(e, t[k], np.float32) for k in _MERLIN_KEYS})
    return _MERLIN_DEV[key]


def _merlin(e, x, fs, pf=1.4, tables=None, what="merlin", n_bins=None, dim=None):
    """One call of mpx_post_filter_merlin on the rows x -> dict of the five buffers ('mcep' holds mcep_pf on return)."""
    import torch
    F, D = x.shape
    if tables is None:
        t, d = _merlin_tables(e, D, fs, pf)
    else:
        t, d = tables, {k: _dev(e, tables[k], np.float32) for k in _MERLIN_KEYS}
    dx = _dev(e, x, np.float32)
    bufs = {k: Fenced(e, F * D, torch.float32) for k in ("mcep", "mcep_w", "out")}
    bufs.update({k: Fenced(e, F, torch.float32) for k in ("r0", "p_r0")})
    e.launch("mpx_post_filter_merlin", dx, F, D if dim is None else dim, d["c1"], d["lifter"], d["g"], d["wk"],
             int(t["g"].shape[1]) if n_bins is None else n_bins, float(t["alpha"]), d["cf"], float(la.MAGIC),
             bufs["mcep"].ptr, bufs["mcep_w"].ptr, bufs["r0"].ptr, bufs["p_r0"].ptr, bufs["out"].ptr)
    _sync()
    res = {k: b.check(what + " " + k) for k, b in bufs.items()}
    for k in ("mcep", "mcep_w", "out"):
        res[k] = res[k].reshape(F, D)
    return res


def _blame(got, x, t):
    """Which launch: the scratch outputs against merlin_stages."""
    st = osm.merlin_stages(osm._f32(x), t)
    with np.errstate(all="ignore"):
        d = {"k_rows_gemm mcep_w": np.max(np.abs(got["mcep_w"] - st["mcep_w"])),
             "k_merlin_r0 r0 (relative)": np.max(np.abs(got["r0"] / st["r0"] - 1)),
             "k_merlin_r0 p_r0 (relative)": np.max(np.abs(got["p_r0"] / st["p_r0"] - 1)),
             "k_merlin_b mcep_pf": np.max(np.abs(got["mcep"] - st["mcep_pf"])),
             "k_rows_gemm out": np.max(np.abs(got["out"] - st["out"]))}
    return ", ".join("%s %.3g" % kv for kv in d.items())


def _merlin_vs_oracle(e, dim, fs, pf, frames):
    x, want = osm.merlin_reference(dim, fs, pf)
    worst = 0.0
    for F in frames:
        what = "merlin D %d F %d fs %d pf %.2f" % (dim, F, fs, pf)
        got = _merlin(e, x[:F], fs, pf, what=what)
        assert np.all(np.isfinite(got["out"])), what
        d = float(np.max(np.abs(got["out"].astype(np.float64) - want[:F])))
        print("%s: max |out - oracle| %.3g" % (what, d))
        if d > TOL_MERLIN[dim]:
            print(what + " by launch: " + _blame(got, x[:F], hm.merlin_tables(dim, fs, pf)))
        within(d, TOL_MERLIN[dim], "OS_MERLIN_ABS_D%d" % dim)
        worst = max(worst, d)
    return worst


@pytest.mark.parametrize("fs", osm.MERLIN_FS)
@pytest.mark.parametrize("dim", osm.MERLIN_DIMS)
def test_merlin_against_the_oracle(dim, fs):
    """D at the argument limits (3, 64 = the full LDS tiles) and between, F around the 64-frame group of k_merlin_r0 and
    the 4-frame group of k_rows_gemm: formant rows and constant -23 rows."""
    _merlin_vs_oracle(_engine(), dim, fs, 1.4, osm.MERLIN_FRAMES)


@pytest.mark.parametrize("pf", [1.0, 1.25])
def test_merlin_other_lifters(pf):
    e = _engine()
    for fs in osm.MERLIN_FS:
        _merlin_vs_oracle(e, 60, fs, pf, (65,))


def test_merlin_engine_path_equals_the_direct_call():
    """Engine.post_filter_merlin (tables without NaN guards, plain buffers) returns the direct call's rows bit for bit: the
    NaNs that follow wk's and g's last elements in the direct call reach nothing."""
    e = _engine()
    for dim, pf in ((60, 1.4), (60, 1.25), (3, 1.4), (64, 1.4)):
        x = osm.merlin_reference(dim, 48000, pf)[0][:65]
        got = _merlin(e, x, 48000, pf)
        assert np.all(np.isfinite(got["r0"])) and np.all(np.isfinite(got["p_r0"])) and np.all(got["r0"] > 0)
        eng = e.post_filter_merlin(e.to_device(x, np.float32), 48000, pf_coef=pf).cpu().numpy()
        assert _same_bits(eng, got["out"]), (dim, pf)


def test_merlin_stride_loop_past_4096_workgroups():
    """k_rows_gemm launches at most 4 096 workgroups of 4 frames and strides beyond: F = 16 384 + 7 rows, row f a copy of
    row f mod 257.  A row's arithmetic has a fixed order wherever the row lies, so every output row equals row f mod 257
    of the 257-row launch bit for bit -- and those are compared with the oracle above."""
    e = _engine()
    x = osm.merlin_reference(60, 48000)[0]
    base = _merlin(e, x, 48000, what="merlin 257 rows")
    F = 16384 + 7
    idx = np.arange(F) % osm.MERLIN_ROWS
    got = _merlin(e, x[idx], 48000, what="merlin 16391 rows")
    for k in ("out", "mcep", "mcep_w", "r0", "p_r0"):
        assert _same_bits(got[k], base[k][idx]), k


def test_merlin_bad_rows_become_magic_and_leave_their_neighbours_alone():
    """A row of NaNs and a row with one -inf at positions 0, 3 (the last of a 4-frame group), 63 and 64: they come back all
    la.MAGIC, as the oracle gives; every other row -- the bad rows share LDS tiles with them -- is bit-identical to the
    launch without the bad rows."""
    e = _engine()
    x = osm.merlin_reference(60, 48000)[0][:70]
    base = _merlin(e, x, 48000)["out"]
    pos = (0, 3, 63, 64)
    for nan_at, inf_col in (((0, 63), 7), ((3, 64), 0), ((0, 64), 59)):
        bad = x.copy()
        for p in pos:
            if p in nan_at:
                bad[p, :] = np.nan
            else:
                bad[p, inf_col] = -np.inf
        got = _merlin(e, bad, 48000, what="merlin with bad rows")["out"]
        assert np.all(got[list(pos)] == np.float32(la.MAGIC)), (nan_at, inf_col)
        good = np.setdiff1d(np.arange(70), pos)
        assert _same_bits(got[good], base[good]), (nan_at, inf_col)


def test_merlin_r0_weights_the_last_bin_alone_in_its_chunk():
    """2049 = 32 * 64 + 1: the last 64-bin chunk of k_merlin_r0 holds bin 2048 and 63 masked lanes.  With wk[2048] = 0 and
    then W = 4096, r0 moves by W exp(2 (mcep g)[2048]), the term of merlin_stages; of r0 with the large weight."""
    e = _engine()
    x = osm.merlin_reference(60, 48000)[0][:65]
    t = hm.merlin_tables(60, 48000)
    assert t["wk"].size == 2049 and t["g"].shape == (60, 2049)
    W = 4096.0
    r = []
    for w in (0.0, W):
        tt = dict(t, wk=t["wk"].copy())
        tt["wk"][2048] = w
        r.append(_merlin(e, x, 48000, tables=tt, what="merlin wk[2048] = %g" % w))
    st = osm.merlin_stages(x, t)
    worst = 0.0
    for key, c in (("r0", st["mcep"]), ("p_r0", st["mcep_w"])):
        term = W * np.exp(2.0 * (c @ t["g"][:, 2048]))
        lo, hi = r[0][key].astype(np.float64), r[1][key].astype(np.float64)
        assert np.all(hi > lo) and np.all(term > 0.05 * hi)      # the term is a visible share of r0
        worst = max(worst, float(np.max(np.abs((hi - lo) - term) / hi)))
    print("merlin last-bin term: %.3g of r0" % worst)
    within(worst, TOL_MERLIN_MASK, "OS_MERLIN_MASK_TERM")


def test_merlin_argument_checks_launch_nothing():
    import torch
    e = _engine()
    x = osm.merlin_reference(3, 48000)[0][:8]
    for kw in (dict(dim=2), dict(dim=65), dict(n_bins=0)):
        with pytest.raises(_lib.MagphaseHipError, match=r"\(-1\)"):
            _merlin(e, x, 48000, **kw)
    # no frames: OK, and nothing is touched
    t, d = _merlin_tables(e, 3, 48000, 1.4)
    bufs = [Fenced(e, 16, torch.float32) for _ in range(5)]
    e.launch("mpx_post_filter_merlin", _dev(e, x, np.float32), 0, 3, d["c1"], d["lifter"], d["g"], d["wk"], 2049,
             float(t["alpha"]), d["cf"], float(la.MAGIC), *[b.ptr for b in bufs])
    _sync()
    for b in bufs:
        b.untouched("mpx_post_filter_merlin with no frames")


# ---------------------------------------------------------------------------------------------------------------------
# 16-bit PCM
# ---------------------------------------------------------------------------------------------------------------------
def _pcm16(e, sigs, norm, dt, what):
    """One call of mpx_pcm16 -> (int16 [total], peaks [n_utts], offsets)."""
    import torch
    lens = np.array([x.size for x in sigs], dtype=np.int64)
    off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    total = int(off[-1])
    y = _dev(e, np.concatenate(sigs), dt)
    peaks = Fenced(e, lens.size, torch.float64)
    out = Fenced(e, total, torch.int16, sentinel=osm.SENTINEL_I16)
    e.launch("mpx_pcm16", y, 1 if dt == np.float64 else 0, _dev(e, off, np.int64), int(lens.size), int(lens.max()),
             0.0 if norm is None else float(norm), peaks.ptr, out.ptr)
    _sync()
    return out.check(what + " samples", all_written=False), peaks.check(what + " peaks"), off


def _pcm16_check(e, sigs, norm, dt, what):
    sigs = [np.asarray(x).astype(dt) for x in sigs]
    got, peaks, off = _pcm16(e, sigs, norm, dt, what)
    for u, x in enumerate(sigs):
        g, want = got[off[u]:off[u + 1]], osm.pcm16(x, norm)
        bad = np.flatnonzero(g != want)
        assert bad.size == 0, "%s: utterance %d, %d samples differ, the first at %d: device %d, model %d" % (
            what, u, bad.size, bad[0], g[bad[0]], want[bad[0]])
        assert peaks[u] == (float(np.max(np.abs(x.astype(np.float64)))) if x.size else 0.0), "%s: peak %d" % (what, u)
    return got, off


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_pcm16_without_normalisation_ties_and_clipping(dt):
    """norm=None: every one of the 65 535 exact ties (k + 0.5) / 32767 rounds to the even neighbour (float32 input: the
    float32 values of the same numbers, against the model), over-range values clip to the bounds, a zero-length utterance
    and a silent one sit between the others."""
    e = _engine()
    k, ties = osm.pcm16_ties()
    over = np.array([1.0, -1.0, 1.5, -1.5, 3.0, -3.0, 32767.5 / 32767.0, -32768.5 / 32767.0, 0.0, 1e300 if dt == np.float64 else 1e30])
    sigs = [ties, over, np.zeros(0), np.zeros(300), np.linspace(-0.9, 0.9, 4097)]
    got, off = _pcm16_check(e, sigs, None, dt, "pcm16 norm=None %s" % np.dtype(dt).name)
    g = got[off[0]:off[1]].astype(np.float64)
    if dt == np.float64:
        assert np.array_equal(ties * 32767.0, k + 0.5)
        assert np.array_equal(g, np.where(k % 2 == 0, k, k + 1))
        assert np.any(k % 2 == 0) and np.any(k % 2 == 1)
    assert np.array_equal(got[off[1]:off[2]][:8], [32767, -32767, 32767, -32768, 32767, -32768, 32767, -32768])
    assert np.all(got[off[3]:off[4]] == 0)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_pcm16_normalised_with_silent_and_empty_utterances(dt):
    """norm = 0.98: a peak that is negative and the very last sample of a 4 097-sample utterance (the second block of
    k_peak_abs holds that sample alone), a zero-length utterance, a SILENT utterance compared in full -- 0 / 0 is written
    as 0, what la.write_audio_file stores -- and peaks = max |y| exactly, 0 for the silent one."""
    e = _engine()
    rs = np.random.RandomState(12)
    a = rs.uniform(-1, 1, 4097) * 2.0
    a[-1] = -3.5
    sigs = [a, np.zeros(0), np.zeros(300), rs.uniform(-0.3, 0.3, 5000), np.zeros(4096), rs.uniform(-1, 1, 1)]
    got, off = _pcm16_check(e, sigs, 0.98, dt, "pcm16 norm=0.98 %s" % np.dtype(dt).name)
    assert got[off[1] - 1] == -32112                       # rint(0.98 * 32767) = 32112
    assert np.all(got[off[2]:off[3]] == 0) and np.all(got[off[4]:off[5]] == 0)


@pytest.mark.parametrize("n", [65536, 1, 2, 3, 5, 1023, 1025])
def test_pcm16_to_f32_is_exact_and_stays_inside(n):
    """All 65 536 values (n a multiple of 4: the vector arm alone), and the tails n mod 4 = 1, 2, 3 of one and two
    workgroups; nothing after out[n - 1] is written."""
    import torch
    e = _engine()
    p = (np.arange(n) * 40503 % 65536 - 32768 if n != 65536 else np.arange(n) - 32768).astype(np.int16)
    pcm = Fenced(e, n, torch.int16, sentinel=osm.SENTINEL_I16)
    pcm.buf[GUARD:GUARD + n] = torch.from_numpy(p).to(e.device)
    out = Fenced(e, n, torch.float32)
    e.launch("mpx_pcm16_to_f32", pcm.ptr, n, out.ptr)
    _sync()
    got = out.check("pcm16_to_f32 n = %d" % n)
    assert _same_bits(got, osm.pcm16_to_f32(p))
    if n == 65536:
        assert np.unique(p).size == 65536


def test_pcm16_to_f32_argument_checks_launch_nothing():
    import torch
    e = _engine()
    pcm = Fenced(e, 64, torch.int16, sentinel=osm.SENTINEL_I16)
    out = Fenced(e, 64, torch.float32)
    for p_off, o_off in ((2, 0), (0, 4), (4, 0), (0, 8)):
        with pytest.raises(_lib.MagphaseHipError, match="aligned"):
            e.launch("mpx_pcm16_to_f32", pcm.ptr + p_off, 8, out.ptr + o_off)
    e.launch("mpx_pcm16_to_f32", pcm.ptr, 0, out.ptr)      # n = 0: OK
    _sync()
    out.untouched("mpx_pcm16_to_f32 refused or empty")
