"""GPU: the forward kernels of the compressed path, each through its C entry point against its reference of
tests/compressed_kernels_model.py (float64 / longdouble; checked on the CPU, with the decision margins of every operand
set used here, by tests/test_compressed_kernels_host.py):

  k_mel_unwarp_mfma, k_mel_unwarp_tiled    mpx_mel_unwarp, mpx_mel_unwarp_rows without and with tile_first
  k_mel_warp_mfma, k_warp_phase_rows       mpx_mel_warp, mpx_mel_warp_fbank, mpx_mel_warp_rows, mpx_warp_phase_rows
  k_min_phase                              mpx_min_phase at the three transform sizes
  k_noise_stats, k_noise_gains             mpx_noise_stats at the three sizes, mpx_noise_gains
  k_post_filter                            mpx_post_filter

Every output lives inside a larger buffer filled with SENTINEL: whatever the entry is not documented to write (columns
[H, ld) of a row, rows past the last frame, the guard floats before and after) must still hold it afterwards.  No frame,
row, bin or element is left out of a comparison, except the one directed min-phase row with an exact-zero bin, which
makes no parity claim (the float32 transform of a -1e10 log cannot follow float64); _tol.note records that.

Derived bounds (asserted as a fraction of the bound, tolerance 1):
  CK_UNWARP_LIN   |d| <= (K + 8) 2^-24 |A| @ |U|: K products and sums in float32 (the bound mpx_mel_unwarp_backward is
                  held to); with row tables |A| is the interpolated (|A[r0]| (1 - t) + |A[r1]| t) and the operands keep two
                  rows' coefficients within a factor of two, so the float32 lerp rounds at that scale.
  CK_WARP_*       |d| <= ((64 + ceil(H / 64) + 8) 2^-24 + eps_pre) |pre(x)| @ |W|^T: 64 products per chunk accumulator, the
                  chunk sums added up, eps_pre the device prologue's own error (measured by the one-hot test).
  CK_PHASE_ROWS   |d| <= 2^-24 (|b - a| t + |y|): the float32 difference and the one rounding of the fma.
  CK_POST         |d| <= (2 h + 4) 2^-24 (sum |x| over the window + |x_b| |tilt_b|).
  CK_GAINS        relative 8 * 2^-53: the sums of float32 values are exact in float64 in any order; a division, exp, sqrt.
  CK_NOISE_ZERO   a frame of zeros: (N/2 - 1) 1e20 within (N/128 + 8) 2^-24 (the lane's N/128 terms and the six-step tree).
  phasors         |re^2 + im^2 - 1| <= 4 * 2^-23.
Measured on the MI355X against the float64 model (tolerance <= 3 x the worst case; the values stand beside the constants
below, in profiles/r19_compressed_kernels_tolerance_report.json and in DESIGN.md section 3.3f-k):
  CK_EXP_LOG, CK_UNWARP_EXP, CK_UNWARP_EXP_ROWS, CK_EPS_PRE_0 / _1 / _2, CK_MIN_PHASE_ANGLE, CK_NOISE_SUM.
CK_MIN_PHASE_CLOSED_* (the closed-form phase of all-pole envelopes) is held to the angle tolerance plus 2^-24 (ln N + 2),
what the float32 rounding of the magnitudes can move the phase by.  Float32 operands are uploaded between runs of NaN.
"""
import math

import numpy as np
import pytest

import compressed_kernels_model as ckm
from _tol import note, within

pytestmark = pytest.mark.gpu

LD = np.longdouble
U24 = ckm.U24
SENTINEL = ckm.SENTINEL
GUARD = 64   # floats before and after every output (a multiple of 4: the tiled form wants 16-byte aligned rows)
NAN_GUARD = 2112   # NaNs before and after every float32 operand (a multiple of 64: the operand keeps its alignment)

# ---- measured on the MI355X against the float64 / longdouble model; every tolerance <= 3 x its worst case ----
TOL_EXP_LOG = 3.0e-7          # |ln(exp job's output) - U| of the one-hot test (__expf alone): measured 1.24e-7
TOL_UNWARP_EXP = 2.0e-6       # relative error of the exp job, plain rows: measured 7.07e-7 (K = 60, |A| @ |U| <= 8)
TOL_UNWARP_EXP_ROWS = 2.0e-6  # ... interpolated between two rows (float32 lerp of two exponentials): measured 6.84e-7
# error of the device prologue relative to max(|pre|, 1) -- where a prologue crosses zero (x = 1) its error is absolute,
# 2^-24 from the rounding of the logarithm's argument: measured 1.60e-7 (mode 0), 3.34e-8 (modes 1 / 3), 1.79e-7 (mode 2)
EPS_PRE = {0: 4.0e-7, 1: 1.0e-7, 2: 4.5e-7}
# radians, every bin of every frame: measured 2.55e-6 / 2.84e-6 / 2.56e-6 (the float64 model is 2.7e-15 from longdouble)
TOL_MIN_PHASE_ANGLE = {1024: 7.0e-6, 2048: 8.0e-6, 4096: 7.0e-6}
TOL_NOISE_SUM = 3.0e-6        # relative error of a frame's sum (condition number <= 8, see noise_signal): measured 1.05e-6


def _engine():
    from magphase_amd.engine import get_engine
    return get_engine()


def _dev(e, a, dtype):
    """Upload; float32 operands lie between two runs of NaN_GUARD NaNs (more than a row of 2049 bins): a read before or
    past an operand -- the unwarp kernels' U rows past K are addressed through a scalar offset the buffer descriptor's
    bounds check does not see -- multiplies a NaN into the output instead of whatever the allocator left there."""
    import torch
    a = np.ascontiguousarray(a, dtype=dtype)
    if dtype != np.float32:
        return torch.from_numpy(a).to(e.device)
    buf = np.full(a.size + 2 * NAN_GUARD, np.nan, dtype=np.float32)
    buf[NAN_GUARD:NAN_GUARD + a.size] = a.ravel()
    return torch.from_numpy(buf).to(e.device)[NAN_GUARD:NAN_GUARD + a.size].view(a.shape)


class Guarded:
    """[rows_alloc x ld] float32 (or dtype) output rows between two guards, everything pre-filled with SENTINEL."""

    def __init__(self, e, rows, ld, extra_rows=3, dtype=None):
        import torch
        self.rows_alloc, self.ld = rows + extra_rows, int(ld)
        self.buf = torch.full((2 * GUARD + self.rows_alloc * self.ld,), SENTINEL, dtype=dtype or torch.float32, device=e.device)
        self.ptr = self.buf[GUARD:].data_ptr()

    def check(self, rows, cols, what, spill=0, written=None):
        """-> the [rows x cols] region.  Everything else must hold the sentinel; spill: floats after column cols - 1 of a
        written row that may hold anything (the tiled form's last quad); written: bool mask of the region's elements
        the entry writes (the others must still hold the sentinel)."""
        h = self.buf.cpu().numpy()
        assert np.all(h[:GUARD] == SENTINEL), what + ": guard before the buffer overwritten"
        assert np.all(h[-GUARD:] == SENTINEL), what + ": guard after the buffer overwritten"
        m = h[GUARD:-GUARD].reshape(self.rows_alloc, self.ld)
        assert np.all(m[rows:] == SENTINEL), what + ": rows past the last frame written"
        assert np.all(m[:rows, cols + spill:] == SENTINEL), what + ": columns past the last bin written"
        out = m[:rows, :cols]
        if written is not None:
            assert np.all(out[~written] == SENTINEL), what + ": written where the entry must leave the buffer alone"
            assert not np.any(out[written] == SENTINEL), what + ": not written where the entry must write"
        else:
            assert not np.any(out == SENTINEL), what + ": elements of the output not written"
        return out.copy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------------------------------
# unwarp
# ---------------------------------------------------------------------------------------------------------------------
def _unwarp(e, ops, F, H, ld, rows=None, n_rows=0, tile_first=None, voiced=None, n_phase_bins=0):
    """One call of mpx_mel_unwarp / mpx_mel_unwarp_rows -> the three Guarded outputs."""
    d = {k: _dev(e, v, np.float32) for k, v in ops.items()}
    k_mag, k_ph = ops["a_mag"].shape[1], ops["a_real"].shape[1]
    out = [Guarded(e, F, ld) for _ in range(3)]
    if rows is None:
        e.launch("mpx_mel_unwarp", F, H, d["a_mag"], k_mag, d["u_mag"], out[0].ptr, d["a_real"], d["a_imag"], k_ph,
                 d["u_phase"], out[1].ptr, out[2].ptr, ld)
    else:
        d_r0, d_r1, d_t = _dev(e, rows[0], np.int32), _dev(e, rows[1], np.int32), _dev(e, rows[2], np.float32)
        d_tf = None if tile_first is None else _dev(e, tile_first, np.int32)
        d_v = None if voiced is None else _dev(e, voiced, np.int32)
        e.launch("mpx_mel_unwarp_rows", F, H, d["a_mag"], k_mag, d["u_mag"], out[0].ptr, d["a_real"], d["a_imag"], k_ph,
                 d["u_phase"], out[1].ptr, out[2].ptr, ld, d_r0, d_r1, d_t, n_rows, d_tf, d_v, n_phase_bins)
    import torch
    torch.cuda.synchronize()
    return out


def _lin_ratio(got, ref, absdot, K):
    return float(np.max(np.abs(got.astype(LD) - ref) / ((K + 8) * U24 * absdot)))


def _rel(got, ref):
    return float(np.max(np.abs(got.astype(LD) - ref) / np.abs(ref)))


def _check_unwarp(out, ops, F, H, what, rows=None, spill=0, exp_label="CK_UNWARP_EXP", exp_tol=None):
    """The three outputs of one call against unwarp_ref, every element; -> the three arrays."""
    r = (None, None, None) if rows is None else rows
    got = [out[0].check(F, H, what + " mag", spill=spill), out[1].check(F, H, what + " real"), out[2].check(F, H, what + " imag")]
    ref, _ = ckm.unwarp_ref(ops["a_mag"], ops["u_mag"], 1, *r)
    rel = _rel(got[0], ref)
    lin = 0.0
    for k, name in ((1, "a_real"), (2, "a_imag")):
        ref, absdot = ckm.unwarp_ref(ops[name], ops["u_phase"], 0, *r)
        lin = max(lin, _lin_ratio(got[k], ref, absdot, ops[name].shape[1]))
    print("%s: exp job relative %.3g, linear jobs %.3g of the bound" % (what, rel, lin))
    within(lin, 1.0, "CK_UNWARP_LIN")
    within(rel, exp_tol if exp_tol is not None else TOL_UNWARP_EXP, exp_label)
    return got


@pytest.mark.parametrize("i", range(len(ckm.ONEHOT_K)))
def test_unwarp_one_hot_rows_return_the_matrix_bit_for_bit(i):
    """A[f] = e_{f mod K}: the linear jobs return U[f mod K] bit for bit, the exp job its exponential, at every KH, both
    special cases for U rows past K, the second column part of one column (H = 513) and a last row tile of 6 rows --
    through the plain kernel, the row-table kernels (identity tables) and the tiled kernel."""
    e = _engine()
    K, Km = ckm.ONEHOT_K[i], ckm.ONEHOT_K[(i + 5) % len(ckm.ONEHOT_K)]   # the exp job sweeps the same set, K != Km
    H, F = ckm.ONEHOT_H, ckm.ONEHOT_F
    ld = int(e.lib.mpx_spec_ld(H))
    a_m, u_m = ckm.onehot_unwarp_operands(Km, seed=50)
    a_p, u_p = ckm.onehot_unwarp_operands(K)
    a_i = np.zeros_like(a_p)
    a_i[np.arange(F), (np.arange(F) + 1) % K] = 1.0
    ops = {"a_mag": a_m, "u_mag": u_m, "a_real": a_p, "a_imag": a_i, "u_phase": u_p}
    rows = ckm.row_tables(F, F, 0, "identity")
    worst = 0.0
    for form in ("plain", "rows", "tiled"):
        out = _unwarp(e, ops, F, H, ld, rows=None if form == "plain" else rows, n_rows=F,
                      tile_first=ckm.tile_first_of(rows[0], F) if form == "tiled" else None)
        what = "one-hot K %d / %d %s" % (K, Km, form)
        mag = out[0].check(F, H, what + " mag", spill=3 if form == "tiled" else 0)
        assert _same_bits(out[1].check(F, H, what + " real"), u_p[np.arange(F) % K]), what
        assert _same_bits(out[2].check(F, H, what + " imag"), u_p[(np.arange(F) + 1) % K]), what
        assert np.all(mag > 0)
        worst = max(worst, float(np.max(np.abs(np.log(mag.astype(np.float64)) - u_m[np.arange(F) % Km].astype(np.float64)))))
    print("one-hot K %d / %d: |ln(out) - U| %.3g" % (K, Km, worst))
    within(worst, TOL_EXP_LOG, "CK_EXP_LOG")


@pytest.mark.parametrize("F,H,k_mag,k_phase", ckm.UNWARP_RANDOM)
def test_unwarp_random_operands_against_the_longdouble_product(F, H, k_mag, k_phase):
    e = _engine()
    ops = ckm.unwarp_operands(F, H, k_mag, k_phase, seed=F + H)
    for ld in (int(e.lib.mpx_spec_ld(H)), H):
        out = _unwarp(e, ops, F, H, ld)
        _check_unwarp(out, ops, F, H, "unwarp F %d H %d K %d/%d ld %d" % (F, H, k_mag, k_phase, ld))


@pytest.mark.parametrize("n_rows,F,H", [(50, 33, 513), (40, 129, 65), (70, 70, 100)])
def test_unwarp_row_tables(n_rows, F, H):
    """Random sorted row0, row1 in {row0, row0 + 1}, rowt in {0, 1, random}, fewer and more frames than rows; identity
    tables reproduce mpx_mel_unwarp bit for bit."""
    e = _engine()
    ops = ckm.unwarp_operands(n_rows, H, 45, 24, seed=n_rows + H)
    for ld in (int(e.lib.mpx_spec_ld(H)), H):
        rows = ckm.row_tables(n_rows, F, seed=F)
        assert np.any(rows[2] == 0) and np.any(rows[2] == 1) and np.any((rows[2] > 0) & (rows[2] < 1))
        out = _unwarp(e, ops, F, H, ld, rows=rows)
        _check_unwarp(out, ops, F, H, "unwarp rows %d -> %d H %d ld %d" % (n_rows, F, H, ld), rows=rows,
                      exp_label="CK_UNWARP_EXP_ROWS", exp_tol=TOL_UNWARP_EXP_ROWS)
    ident = ckm.row_tables(n_rows, n_rows, 0, "identity")
    a = _unwarp(e, ops, n_rows, H, ld, rows=ident)
    b = _unwarp(e, ops, n_rows, H, ld)
    for k in range(3):
        assert _same_bits(a[k].check(n_rows, H, "identity tables"), b[k].check(n_rows, H, "plain")), k


@pytest.mark.parametrize("n_rows,H", [(n, 513) for n in ckm.TILED_N_ROWS] + [(63, 2049)])
def test_unwarp_tiled_form_equals_the_two_product_form(n_rows, H):
    """tile_first as the plan builds it; a tile that owns no frame, one that owns more than 64 and one that owns 65.  Against
    unwarp_ref, and bit for bit against the form without tile_first ("the same values").  The quad store of the last bin
    may leave up to three floats in the row padding; nothing else is written."""
    e = _engine()
    ld = int(e.lib.mpx_spec_ld(H))
    rows = ckm.tiled_row_tables(n_rows, seed=n_rows)
    F = rows[0].size
    assert F <= 200
    tf = ckm.tile_first_of(rows[0], n_rows)
    counts = np.diff(tf)
    assert tf[0] == 0 and tf[-1] == F and np.max(counts) >= 65
    ops = ckm.unwarp_operands(n_rows, H, 60 if H > 600 else 24, 16, seed=n_rows + H)
    what = "tiled unwarp %d rows -> %d frames H %d (frames per tile %s)" % (n_rows, F, H, list(counts))
    tiled = _unwarp(e, ops, F, H, ld, rows=rows, n_rows=n_rows, tile_first=tf)
    got = _check_unwarp(tiled, ops, F, H, what, rows=rows, spill=3, exp_label="CK_UNWARP_EXP_ROWS", exp_tol=TOL_UNWARP_EXP_ROWS)
    plain = _unwarp(e, ops, F, H, ld, rows=rows)
    for k in range(3):
        assert _same_bits(got[k], plain[k].check(F, H, what + " (no tile_first)")), k


def test_unwarp_tiled_tables_hold_an_empty_tile():
    rows = ckm.tiled_row_tables(100, seed=100)
    counts = np.diff(ckm.tile_first_of(rows[0], 100))
    assert counts[1] == 0 and counts[0] > 64 and rows[0].size <= 200
    assert np.diff(ckm.tile_first_of(ckm.tiled_row_tables(31, seed=31)[0], 31))[0] == 65


def test_unwarp_rejects_unaligned_rows_in_the_tiled_form():
    """The tiled form stores 16-byte quads: ld must be a multiple of 4 (documented limitation, an argument check)."""
    from magphase_amd import _lib
    e = _engine()
    H, n_rows = 65, 10
    rows = ckm.row_tables(n_rows, n_rows, 0, "identity")
    ops = ckm.unwarp_operands(n_rows, H, 8, 8, seed=1)
    with pytest.raises(_lib.MagphaseHipError, match="16-byte aligned"):
        _unwarp(e, ops, n_rows, H, H, rows=rows, n_rows=n_rows, tile_first=ckm.tile_first_of(rows[0], n_rows))


def test_unwarp_skips_the_phase_rows_of_unvoiced_tiles():
    """voiced with whole 32-frame tiles unvoiced: their phase rows keep the sentinel, every other row (the unvoiced frames
    of the other tiles included) and every magnitude row is correct."""
    e = _engine()
    n_rows, F, H = 60, 100, 513
    ld = int(e.lib.mpx_spec_ld(H))
    rows = ckm.row_tables(n_rows, F, seed=5)
    voiced = (np.random.RandomState(3).uniform(0, 1, F) > 0.4).astype(np.int32)
    voiced[0], voiced[1] = 1, 0
    voiced[32:64] = 0    # a whole tile
    voiced[96:] = 0      # the last, partial tile
    voiced[64], voiced[65:96] = 1, 0   # one voiced frame keeps a tile
    ops = ckm.unwarp_operands(n_rows, H, 24, 45, seed=9)
    out = _unwarp(e, ops, F, H, ld, rows=rows, voiced=voiced)
    live = np.ones(F, dtype=bool)
    live[32:64] = live[96:] = False
    written = np.repeat(live[:, None], H, axis=1)
    mag = out[0].check(F, H, "voiced tiles mag")
    within(_rel(mag, ckm.unwarp_ref(ops["a_mag"], ops["u_mag"], 1, *rows)[0]), TOL_UNWARP_EXP_ROWS, "CK_UNWARP_EXP_ROWS")
    for k, name in ((1, "a_real"), (2, "a_imag")):
        got = out[k].check(F, H, "voiced tiles " + name, written=written)
        ref, absdot = ckm.unwarp_ref(ops[name], ops["u_phase"], 0, *rows)
        within(_lin_ratio(got[live], ref[live], absdot[live], 45), 1.0, "CK_UNWARP_LIN")


@pytest.mark.parametrize("n", ckm.PHASE_BINS + (600,))
def test_unwarp_produces_exactly_the_phase_columns_asked_for(n):
    e = _engine()
    n_rows, F, H = 20, 33, 600
    ld = int(e.lib.mpx_spec_ld(H))
    rows = ckm.row_tables(n_rows, F, seed=n)
    ops = ckm.unwarp_operands(n_rows, H, 10, 62, seed=n + 1)
    out = _unwarp(e, ops, F, H, ld, rows=rows, n_phase_bins=n)
    cols = H if n == 0 else min(H, (n + 63) // 64 * 64)
    written = np.zeros((F, H), dtype=bool)
    written[:, :cols] = True
    within(_rel(out[0].check(F, H, "phase bins mag"), ckm.unwarp_ref(ops["a_mag"], ops["u_mag"], 1, *rows)[0]),
           TOL_UNWARP_EXP_ROWS, "CK_UNWARP_EXP_ROWS")
    for k, name in ((1, "a_real"), (2, "a_imag")):
        got = out[k].check(F, H, "n_phase_bins %d %s" % (n, name), written=written)
        ref, absdot = ckm.unwarp_ref(ops[name], ops["u_phase"], 0, *rows)
        within(_lin_ratio(got[:, :cols], ref[:, :cols], absdot[:, :cols], 62), 1.0, "CK_UNWARP_LIN")


# ---------------------------------------------------------------------------------------------------------------------
# warp
# ---------------------------------------------------------------------------------------------------------------------
def _warp(e, entry, F, H, x, w_mag, w_ph, voi, ld=None, rows=None, fbank=0, n_var=0, in_use=None):
    """One call of mpx_mel_warp / _fbank / _rows -> (Guarded out_mag, out_real, out_imag, tmp_real, tmp_imag).  x: the
    three [rows x H] operand matrices, uploaded with the row pitch ld (padding: NaN, never to be read)."""
    import torch
    ld = ld or H
    d_x = []
    for m in x:
        p = np.full((m.shape[0], ld), np.nan, dtype=np.float32)
        p[:, :H] = m
        d_x.append(_dev(e, p, np.float32))
    md, pd = w_mag.shape[0], w_ph.shape[0]
    d_wm, d_wp, d_v = _dev(e, w_mag, np.float32), _dev(e, w_ph, np.float32), _dev(e, voi, np.float32)
    r = [None] * 3 if rows is None else [_dev(e, rows[0], np.int32), _dev(e, rows[1], np.int32), _dev(e, rows[2], np.float32)]
    out = [Guarded(e, F, md), Guarded(e, F, pd), Guarded(e, F, pd)]
    tmp = [None, None]
    if entry == "mpx_mel_warp_rows":
        d_use = None
        if n_var:
            tmp = [Guarded(e, n_var, pd), Guarded(e, n_var, pd)]
            d_use = _dev(e, in_use, np.float32)
        e.launch(entry, F, H, d_x[0], d_x[1], d_x[2], r[0], r[1], r[2], d_wm, md, d_wp, pd, d_v, out[0].ptr, out[1].ptr,
                 out[2].ptr, ld, fbank, n_var, d_use, tmp[0].ptr if n_var else None, tmp[1].ptr if n_var else None)
    else:
        e.launch(entry, F, H, d_x[0], d_x[1], d_x[2], r[0], r[1], r[2], d_wm, md, d_wp, pd, d_v, out[0].ptr, out[1].ptr,
                 out[2].ptr, ld)
    torch.cuda.synchronize()
    return out + tmp


def _warp_bound(H, absdot, mode):
    return ((64 + (H + 63) // 64 + 8) * U24 + EPS_PRE[1 if mode == 3 else mode]) * absdot


@pytest.mark.parametrize("F,H,mag_dim,phase_dim", ckm.WARP_SHAPES)
def test_warp_one_hot_matrix_returns_the_prologue_of_the_named_bin(F, H, mag_dim, phase_dim):
    """W[i] = c e_{k_i} (c = 1 for the magnitudes, 1/4 for the phase streams, which keeps 2 x inside the clip: a power of
    two, so the output is the device prologue of x[f][k_i] times c exactly -- sums of exact zeros are exact).  Pins the
    chunk swizzle, the chunk edges and the tail loop, and measures the prologues' own error eps_pre."""
    e = _engine()
    mag, real, imag = ckm.warp_operands(F, H, seed=F + H)
    w_mag, k_mag = ckm.warp_onehot_matrix(mag_dim, H, seed=1)
    w_ph, k_ph = ckm.warp_onehot_matrix(phase_dim, H, seed=2)
    voi = np.ones(F, dtype=np.float32)
    for entry, mode in (("mpx_mel_warp", 0), ("mpx_mel_warp_fbank", 2)):
        out = _warp(e, entry, F, H, (mag, real, imag), w_mag, (0.25 * w_ph).astype(np.float32), voi)
        what = "one-hot warp %s F %d H %d" % (entry, F, H)
        got = [out[0].check(F, mag_dim, what + " mag"), out[1].check(F, phase_dim, what + " real"),
               out[2].check(F, phase_dim, what + " imag")]
        for g, x, ks, m, c in ((got[0], mag, k_mag, mode, 1.0), (got[1], real, k_ph, 1, 0.25), (got[2], imag, k_ph, 1, 0.25)):
            pre = ckm.warp_prologue_ref(m, x[:, ks])
            eps = float(np.max(np.abs(g.astype(LD) / c - pre) / np.maximum(np.abs(pre), 1)))
            print("%s: prologue of mode %d, error %.3g of max(|pre|, 1)" % (what, m, eps))
            within(eps, EPS_PRE[m], "CK_EPS_PRE_%d" % m)


def _check_warp(out, F, dims, x, w, modes, voi, H, what, rows=None):
    for k in range(3):
        got = out[k].check(F, dims[k], "%s job %d" % (what, k))
        ref, absdot = ckm.warp_ref(x[k] if rows else x[k][:F], w[k], modes[k], voi if modes[k] == 1 else None,
                                   *(rows or (None, None, None)))
        ratio = float(np.max(np.abs(got.astype(LD) - ref) / _warp_bound(H, absdot, modes[k])))
        print("%s job %d mode %d: %.3g of the bound" % (what, k, modes[k], ratio))
        within(ratio, 1.0, "CK_WARP_MODE%d" % modes[k])
        if modes[k] == 1:   # unvoiced frames: +0.0, the sign bit included
            assert np.all(_bits(got[np.asarray(voi) == 0]) == 0), what


@pytest.mark.parametrize("F,H,mag_dim,phase_dim", ckm.WARP_SHAPES)
def test_warp_random_operands_against_the_longdouble_product(F, H, mag_dim, phase_dim):
    """Modes 0, 1 and 2 without and with row tables (the six kernel forms of a (mag_dim, phase_dim) pair that take no
    scratch; mpx_mel_warp_rows with scratch has its own test), operand rows at the pitch H and at a padded pitch."""
    e = _engine()
    n_in = F + 7
    x = ckm.warp_operands(n_in, H, seed=F + H + 1)
    w_mag, w_ph = ckm.warp_matrices(mag_dim, phase_dim, H, seed=F)
    w = (w_mag, w_ph, w_ph)
    voi = ckm.voicing(F, seed=H)
    rows = ckm.row_tables(n_in, F, seed=H)
    for entry, mode in (("mpx_mel_warp", 0), ("mpx_mel_warp_fbank", 2)):
        for tab, ld in ((None, H), (rows, H + 3)):
            out = _warp(e, entry, F, H, x, w_mag, w_ph, voi, ld=ld, rows=tab)
            _check_warp(out, F, (mag_dim, phase_dim, phase_dim), x, w, (mode, 1, 1), voi, H,
                        "%s F %d H %d dims %d/%d tables %s" % (entry, F, H, mag_dim, phase_dim, tab is not None), rows=tab)


def test_warp_mode1_epilogue_clips_masks_and_skips_unvoiced_tiles():
    e = _engine()
    F, H, pd, mag, real, imag, real_dev, imag_dev, voi, w_mag, w_ph, kind = ckm.epilogue_case()
    out = _warp(e, "mpx_mel_warp", F, H, (mag, real_dev, imag_dev), w_mag, w_ph, voi)
    for k, x, sign in ((1, real, 1.0), (2, imag, -1.0)):
        got = out[k].check(F, pd, "epilogue job %d" % k)
        ref, absdot = ckm.warp_ref(x, w_ph, 1, voi)
        within(float(np.max(np.abs(got.astype(LD) - ref) / _warp_bound(H, absdot, 1))), 1.0, "CK_WARP_MODE1")
        assert np.all(_bits(got[voi == 0]) == 0), "unvoiced frames must be +0.0"
        assert np.all(_bits(got[64:128]) == 0), "an unvoiced tile is zeros whatever its operand rows hold"
        kk = kind[k - 1]
        hi, lo = (kk == 0) & (voi != 0), (kk == 1) & (voi != 0)
        assert np.any(hi) and np.any(lo)
        assert np.all(got[hi] == sign) and np.all(got[lo] == -sign), "clipped rows must be exactly +-1"


def test_warp_mode2_floor_and_protected_log():
    """x == 0 bins take -1e10 in the prologue: through a one-hot W the output is exactly -1e10 for the row and bin, through a
    positive filter-bank W the whole row's sums lie far below -745.13 and come back as exactly -1e10."""
    e = _engine()
    F, H, md, mag, real, imag, zero_rows, zero_bin, w_fb, w_ph, voi = ckm.mode2_case()
    out = _warp(e, "mpx_mel_warp_fbank", F, H, (mag, real, imag), w_fb, w_ph, voi)
    got = out[0].check(F, md, "mode 2 floor")
    ref, absdot = ckm.warp_ref(mag, w_fb, 2)
    floored = np.zeros(F, dtype=bool)
    floored[zero_rows + [10]] = True
    assert np.all(ref[floored] == LD(ckm.MAGIC)) and np.all(got[floored] == np.float32(ckm.MAGIC))
    within(float(np.max(np.abs(got[~floored].astype(LD) - ref[~floored]) / _warp_bound(H, absdot[~floored], 2))), 1.0,
           "CK_WARP_MODE2")
    w_one, ks = ckm.warp_onehot_matrix(md, H, seed=5)
    w_one[0], ks[0] = 0.0, zero_bin
    w_one[0, zero_bin] = 1.0
    got = _warp(e, "mpx_mel_warp_fbank", F, H, (mag, real, imag), w_one, w_ph, voi)[0].check(F, md, "mode 2 one-hot")
    assert np.all(got[zero_rows, 0] == np.float32(ckm.MAGIC))
    keep = np.ones(F, dtype=bool)
    keep[zero_rows] = False
    pre = ckm.warp_prologue_ref(2, mag[:, ks])
    pre10 = np.isin(np.arange(F), [10])[:, None] & (ks == 3)[None, :]
    ok = keep[:, None] & ~pre10
    within(float(np.max((np.abs(got.astype(LD) - pre) / np.maximum(np.abs(pre), 1))[ok])), EPS_PRE[2], "CK_EPS_PRE_2")
    assert np.all(got[pre10] == np.float32(ckm.MAGIC))


@pytest.mark.parametrize("F,n_var,H,fbank", [(130, 70, 100, 0), (65, 150, 65, 0), (65, 150, 513, 1), (1, 3, 40, 0)])
def test_warp_rows_with_the_phase_streams_on_the_variable_rate_rows(F, n_var, H, fbank):
    """mpx_mel_warp_rows with scratch: the magnitudes interpolated before the prologue, the phase streams warped on the
    n_var rows (mode 3), interpolated, masked and clipped afterwards; n_var larger and smaller than n_frames; rows no
    voiced frame reads hold NaN."""
    e = _engine()
    md, pd = 24, 45
    mag, real, imag = ckm.warp_operands(n_var, H, seed=F + n_var)
    rows, voi, in_use = ckm.rows_case(F, n_var, H, seed=F)
    assert np.any(in_use == 0) or n_var < 10
    real_dev, imag_dev = real.copy(), imag.copy()
    real_dev[in_use == 0] = np.nan
    imag_dev[in_use == 0] = np.nan
    w_mag, w_ph = ckm.warp_matrices(md, pd, H, seed=n_var)
    out = _warp(e, "mpx_mel_warp_rows", F, H, (mag, real_dev, imag_dev), w_mag, w_ph, voi, ld=H + 1, rows=rows, fbank=fbank,
                n_var=n_var, in_use=in_use)
    what = "warp rows F %d n_var %d H %d" % (F, n_var, H)
    mode = 2 if fbank else 0
    got = out[0].check(F, md, what + " mag")
    ref, absdot = ckm.warp_ref(mag, w_mag, mode, None, *rows)
    within(float(np.max(np.abs(got.astype(LD) - ref) / _warp_bound(H, absdot, mode))), 1.0, "CK_WARP_MODE%d" % mode)
    t = rows[2].astype(LD)[:, None]
    for k, x in ((1, real), (2, imag)):
        got = out[k].check(F, pd, what + " phase %d" % k)
        y, absdot = ckm.warp_ref(x, w_ph, 3)
        bound = ckm.lerp(_warp_bound(H, absdot[rows[0]], 3), _warp_bound(H, absdot[rows[1]], 3), t) \
            + 2 * U24 * (np.abs(y[rows[0]]) + np.abs(y[rows[1]]))
        ref = ckm.warp_phase_rows_ref(y, y, rows[0], rows[1], rows[2], voi)[0]
        live = voi != 0
        ratio = float(np.max(np.abs(got[live].astype(LD) - ref[live]) / bound[live])) if np.any(live) else 0.0
        print("%s phase %d: %.3g of the bound" % (what, k, ratio))
        within(ratio, 1.0, "CK_WARP_MODE3")
        assert np.all(_bits(got[~live]) == 0)
        out[3 + k - 1].check(n_var, pd, what + " scratch", written=np.ones((n_var, pd), dtype=bool))


@pytest.mark.parametrize("F,pd", ckm.PHASE_ROWS_SIZES)
def test_warp_phase_rows_alone(F, pd):
    import torch
    e = _engine()
    tmp, row0, row1, rowt, voi = ckm.phase_rows_case(F, pd, seed=F + pd)
    out = [Guarded(e, F, pd), Guarded(e, F, pd)]
    e.launch("mpx_warp_phase_rows", F, pd, _dev(e, tmp[0], np.float32), _dev(e, tmp[1], np.float32), _dev(e, row0, np.int32),
             _dev(e, row1, np.int32), _dev(e, rowt, np.float32), _dev(e, voi, np.float32), out[0].ptr, out[1].ptr)
    torch.cuda.synchronize()
    ref = ckm.warp_phase_rows_ref(tmp[0], tmp[1], row0, row1, rowt, voi)
    t = rowt.astype(LD)[:, None]
    for k in range(2):
        got = out[k].check(F, pd, "phase rows %d x %d stream %d" % (F, pd, k))
        a, b = tmp[k][row0].astype(LD), tmp[k][row1].astype(LD)
        bound = U24 * (np.abs(b - a) * t + np.abs(ckm.lerp(a, b, t))) * (1 + 1e-6)
        ratio = float(np.max(np.abs(got.astype(LD) - ref[k]) / bound))
        print("phase rows %d x %d stream %d: %.3g of the bound" % (F, pd, k, ratio))
        within(ratio, 1.0, "CK_PHASE_ROWS")
        assert np.all(_bits(got[voi == 0]) == 0)
        clipped = np.abs(ref[k]) == 1
        assert np.all(got[clipped] == ref[k][clipped].astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------------
# min phase
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", ckm.FFT_LENS)
def test_min_phase_against_the_float64_cepstrum_and_the_closed_form(N):
    import torch
    e = _engine()
    H = N // 2 + 1
    ld = int(e.lib.mpx_spec_ld(H))
    mag, kinds, closed = ckm.min_phase_rows(N)
    r0, r1, t = ckm.min_phase_row_tables(mag.shape[0])
    # the one directed row with an exact-zero bin, through an identity frame of its own: no parity claim
    zrow = mag[-1].copy()
    zrow[H // 3] = 0.0
    mag = np.vstack((mag, zrow[None, :]))
    last = mag.shape[0] - 1
    r0, r1 = np.append(r0, last).astype(np.int32), np.append(r1, last).astype(np.int32)
    t = np.append(t, 0.0).astype(np.float32)
    F = r0.size
    note("CK_MIN_PHASE_rows_without_parity_claim", 1)
    padded = np.full((mag.shape[0], ld), np.nan, dtype=np.float32)
    padded[:, :H] = mag
    out = [Guarded(e, F, ld) for _ in range(3)]
    e.launch("mpx_min_phase", N, e.tables(N), _dev(e, padded, np.float32), _dev(e, r0, np.int32), _dev(e, r1, np.int32),
             _dev(e, t, np.float32), F, out[0].ptr, out[1].ptr, out[2].ptr, ld)
    torch.cuda.synchronize()
    omag, re, im = (out[k].check(F, H, "min phase N %d output %d" % (N, k)) for k in range(3))
    want = ckm.lerp_f32(mag[r0], mag[r1], t[:, None])
    assert _same_bits(omag, want), "the magnitude rows are fmaf(b - a, t, a) of the inputs"
    assert np.all(np.isfinite(re)) and np.all(np.isfinite(im))
    unit = float(np.max(np.abs(re.astype(np.float64) ** 2 + im.astype(np.float64) ** 2 - 1.0)))
    print("min phase N %d: |re^2 + im^2 - 1| %.3g" % (N, unit))
    within(unit / (4 * 2.0 ** -23), 1.0, "CK_MIN_PHASE_UNIT")
    assert np.all(re[:, H - 1] == 1.0) and np.all(im[:, H - 1] == 0.0), "bin N/2 is the phasor (1, 0)"
    par = np.arange(F) < F - 1   # every frame but the directed zero-bin row
    phi = ckm.min_phase_ref(want[par], N)
    if N == 1024:   # what judges: the float64 FFT form's own distance from the longdouble matrix form, six rows
        pick = np.arange(0, 70, 13)
        note("CK_MIN_PHASE_float64_model_vs_longdouble_dft_rad",
             float(np.max(np.abs(phi[pick] - ckm.min_phase_dft_ref(want[pick], N).astype(np.float64)))))
    err = np.abs(ckm.phasor_angle_error(re[par], im[par], phi))
    worst = float(np.max(err))
    print("min phase N %d: angle error %.3g rad (bin 0: %.3g)" % (N, worst, float(np.max(np.abs(im[par, 0])))))
    within(worst, TOL_MIN_PHASE_ANGLE[N], "CK_MIN_PHASE_ANGLE_%d" % N)
    within(float(np.max(np.abs(im[par, 0]))), TOL_MIN_PHASE_ANGLE[N], "CK_MIN_PHASE_ANGLE_%d" % N)
    n_closed = 0
    for f in range(mag.shape[0] - 1):   # the identity frames of the rows whose phase is known in closed form
        if f in closed:
            d = np.abs(ckm.phasor_angle_error(re[f], im[f], closed[f]))
            within(float(np.max(d)), TOL_MIN_PHASE_ANGLE[N] + ckm.hilbert_noise_bound(N), "CK_MIN_PHASE_CLOSED_%d" % N)
            n_closed += 1
    assert n_closed == 9


# ---------------------------------------------------------------------------------------------------------------------
# noise statistic and gains
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", ckm.FFT_LENS)
def test_noise_stats_of_every_frame_against_the_rfft_reference(N):
    import torch
    e = _engine()
    left, right, wtype, pos, x = ckm.noise_case(N)
    F = left.size
    assert np.min(pos - left) >= 0 and np.max(pos + right) < x.size
    if N == 4096:
        assert np.sum(left + right + 1 > 1024) >= 8
    out = Guarded(e, F, 1, extra_rows=5)
    e.launch("mpx_noise_stats", N, e.tables(N), _dev(e, x, np.float32), _dev(e, pos, np.int64), _dev(e, left, np.int32),
             _dev(e, right, np.int32), _dev(e, wtype, np.int32), F, out.ptr)
    torch.cuda.synchronize()
    got = out.check(F, 1, "noise stats N %d" % N)[:, 0].astype(np.float64)
    worst = 0.0
    for f in range(F - 2):
        ref = ckm.noise_stats_ref(x, int(pos[f]), int(left[f]), int(right[f]), int(wtype[f]), N)
        worst = max(worst, abs(got[f] - ref) / ref)
    flat = (N // 2 - 1) * math.log(ckm.DELTA_AMP) ** 2
    worst = max(worst, abs(got[F - 1] - flat) / flat)
    print("noise stats N %d: %d frames, relative error %.3g" % (N, F, worst))
    within(worst, TOL_NOISE_SUM, "CK_NOISE_SUM")
    zero = (N // 2 - 1) * 1.0e20
    within(abs(got[F - 2] - zero) / zero / ((N // 128 + 8) * U24), 1.0, "CK_NOISE_ZERO")


@pytest.mark.parametrize("pattern", ckm.GAIN_PATTERNS)
@pytest.mark.parametrize("N", ckm.FFT_LENS)
def test_noise_gains_over_ragged_utterances(N, pattern):
    import torch
    e = _engine()
    sums, voiced, off = ckm.gains_case(N, pattern)
    n_utts, total = off.size - 1, int(off[-1])
    inv = Guarded(e, total, 1, extra_rows=9)
    gains = torch.full((2 * n_utts + 4,), SENTINEL, dtype=torch.float64, device=e.device)
    e.launch("mpx_noise_gains", _dev(e, sums, np.float32), _dev(e, voiced, np.int32), _dev(e, off, np.int32), n_utts,
             N // 2 - 1, inv.ptr, gains)
    torch.cuda.synchronize()
    g = gains.cpu().numpy()
    assert np.all(g[2 * n_utts:] == SENTINEL)
    g = g[:2 * n_utts].reshape(n_utts, 2)
    got_inv = inv.check(total, 1, "noise gains")[:, 0]
    ref, ref_inv = ckm.noise_gains_ref(sums, voiced, off, N // 2 - 1)
    assert np.array_equal(np.isnan(g), np.isnan(ref)), "an empty class gives NaN, a class with frames a number"
    if pattern != "alternating":
        empty = 1 if pattern == "voiced" else 0
        assert np.all(np.isnan(ref[:, empty])) and not np.any(np.isnan(ref[:, 1 - empty]))
    ok = ~np.isnan(ref)
    ratio = float(np.max(np.abs(g[ok] / ref[ok] - 1.0))) / (8 * 2.0 ** -53)
    print("noise gains N %d %s: %.3g of the bound" % (N, pattern, ratio))
    within(ratio, 1.0, "CK_GAINS")
    assert np.all(np.isfinite(got_inv)), "every frame that exists has a finite inv_gain"
    want = ref_inv.astype(np.float32)
    d_inv = np.abs(got_inv.astype(np.float64) - want.astype(np.float64))
    assert np.all(d_inv <= np.spacing(want)), "float32(1 / g) or its neighbour"


# ---------------------------------------------------------------------------------------------------------------------
# post-filter
# ---------------------------------------------------------------------------------------------------------------------
def _post_tables(D, fs):
    import warnings
    from magphase_amd import hostmath as hm
    if fs:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            nx0, nx1, half, tilt = hm.post_filter_tables(D, fs)
        return nx0, nx1, half.astype(np.int32), tilt.astype(np.float32)
    return ckm.post_filter_synth_tables(D)


@pytest.mark.parametrize("D,fs", [(D, 0) for D in ckm.POST_DIMS] + [(60, 48000), (60, 16000)])
def test_post_filter_against_the_float64_reference(D, fs):
    import torch
    e = _engine()
    nx0, nx1, half, tilt = _post_tables(D, fs)
    d_half, d_tilt = _dev(e, half, np.int32), _dev(e, tilt, np.float32)
    hb = ckm.post_filter_bound_h(half, nx0, nx1, D)
    for F in ckm.post_filter_frames(D):
        x = ckm.post_filter_input(F, D)
        out = Guarded(e, F, D)
        e.launch("mpx_post_filter", _dev(e, x, np.float32), F, D, d_half, nx0, nx1, d_tilt, out.ptr)
        torch.cuda.synchronize()
        got = out.check(F, D, "post filter D %d F %d" % (D, F))
        ref, absterm = ckm.post_filter_ref(x, half, nx0, nx1, tilt)
        ratio = float(np.max(np.abs(got.astype(np.float64) - ref) / ((2 * hb[None, :] + 4) * U24 * absterm)))
        print("post filter D %d fs %d F %d: %.3g of the bound" % (D, fs, F, ratio))
        within(ratio, 1.0, "CK_POST")
        assert _same_bits(got[:, 0], x[:, 0]) and _same_bits(got[:, -1], x[:, -1]), "the end bins are copied"
