"""GPU: k_synth_comp_pair (csrc/magphase_comp.hip) launched through its three C entries -- mpx_synthesis_compressed_ola,
mpx_synthesis_compressed_ola_spectra, mpx_synthesis_compressed_type2_ola -- with tables built by hand (Engine.launch,
e.tables(N), hostmath.ola_runs, mpx_ola_fixup afterwards), against the float64 model tests/synth_comp_model.py (held to the
oracle by tests/test_synth_comp_model_host.py, which also checks every operand set used here).

Buffers: pcm_out is a view into a sentinel-filled buffer with guards and every kept sample must lose the sentinel; the head
strips are NaN before the launch between sentinel guards; the feature rows have pitch H + 5 with NaN pad columns between
NaN runs; the noise is NaN outside every frame's [pos - L, pos + R]; per_v, ap_v, ap_u are exactly H floats between NaN runs;
in the one-row form real / imag are NaN in every element the header's n_per_bins contract leaves unread (all of an unvoiced
frame, the complement of synth_comp_model.phase_read_set of a voiced one); rows no table entry names are NaN.  One NaN in
the output is a read outside the documented extent.  No frame, sample or bin is left out of a comparison; where the model's
norm is 0 (outside the window, a silent spectrum) the device must give an exact zero.

The sixteen instances synthesis_compressed_ola_impl can select, and the case that reaches each (test_single_frame,
test_one_hot_spectra and test_multi_frame run the first fourteen, test_n_per_sweep the one-row ones;
test_single_frame_stored_spectra and test_stored_spectra_against_recomputed the last two):

  <8, one row> <16, one row>                  type 1, type 2    fft_len 1024, 2048, no row tables
  <32, one row, any n_per>                    type 1, type 2    fft_len 4096, n_per_bins 0 (= 2049), 513, 700
  <32, one row, n_per <= 512 schedule>        type 1, type 2    fft_len 4096, n_per_bins 449, 512
  <8, rows> <16, rows> <32, rows>             type 1, type 2    row tables (single-frame, one-hot, multi-frame cases)
  <32, one row, n_per <= 512, spectra>        type 1            mpx_noise_stats_spectra -> _ola_spectra, n_per_bins 449
  <32, one row, any n_per, spectra>           type 1            the same with n_per_bins 0

Derived bound, u = 2^-24, one rounding <= 1 u of its result, L2N = log2(fft_len), per output sample n of a frame against
B[n] of the model (the largest the sample can be: w[n] sum_k c_k m_k (|apc inv_gain| ||noise frame||_1 + per_v) / N):

  |y_dev - y_model| <= (10 L2N + 46) u B[n]

  noise spectrum   (5 L2N + 20) u ||w x||_1 per bin: noise-window weight 10 (as the analysis bound of
                   tests/test_gpu_lossless_kernels.py; bartlett^2.5 = t t sqrt(t) with t accurate to 2 u: 5 + 3), weight x
                   sample 1, L2N - 1 butterfly levels of the N/2-point transform and the split as the last, 5 each (table
                   twiddle 1, complex product 3, sum 1), the split's own twiddle, E / T sums and T product 9
  assembly         aperiodic factor m apc inv_gain 2, its fused multiply-add into the sum 1; periodic term 8 (a^2 + b^2: 2,
                   rsq: 2, m per_v rsq: 2, a u: 1, the sum: 1) -- the larger of the two arms is the aperiodic one: 3 on top
                   of the noise spectrum's; |X| at bins 0 and N/2 3 (squares and sum 2, sqrt 1); the 0.5 / M scale 1
  Hermitian merge  8 (lane twiddle 6, sums 2), inverse transform 5 L2N, anti-ringing window weight 10 and its fused
                   multiply-add into the ring 1
  in all           5 L2N + 20 + 3 + 3 + 1 + 8 + 5 L2N + 11 = 10 L2N + 46      (146 / 156 / 166 u at 1024 / 2048 / 4096)

With row tables the float32 interpolation adds u B_lerp[n] (synth_comp_model's docstring); where several frames reach a
sample every addition into the ring and the fix-up's rounds the partial sum once: + count[n] u B[n], count the frames whose
window reaches the sample.  The fraction of (10 L2N + 46 + count) u B + u B_lerp the device reaches goes through
_tol.within under SCK_* labels.

Such a bound adds every rounding in the same direction and stands far above what the device reaches, so every instance
group is also pinned against the float64 model at <= 3 x the worst case measured on the MI355X, in units of u (B + B_lerp)
(PIN below; profiles/r31_synth_comp_kernel_tolerance_report.json).

Determinism the header documents (mpx_ola_run: predecessor's sum + head strip, a fixed order): the same tables twice, and the
same runs dealt to another number of slots, are bit-identical -- a run is overlap-added by one wave pair in frame order
whichever slot it is in.  Other run cuts move the seams, and with them the association of the float32 sums there: the two
results differ by at most 2 count u B per sample.

What these tests found: the header's sentence "real / imag and per_v of those bins are not read" held at the granularity
of 64-bin groups only, and above fft_len/4 the groups are the lanes' MIRROR bins, [N/4 + 1 + 64 j, N/4 + 64 + 64 j]: for
n_per_bins = N/4 + 2 the kernel reads bin N/4 + 64, one past n_per_bins rounded up to 64 -- the columns the plan's unwarp
fills -- and a NaN there reaches the output through a * u with u == 0.  No supported sample rate has n_per_bins above N/4,
so no output changed; the header now names the groups, hostmath.synth_comp_phase_columns counts the columns and the plan
passes that count to the unwarp (test_n_per_sweep poisons exactly the complement of the documented set)."""
import functools

import numpy as np
import pytest
import torch

import synth_comp_model as scm
from _tol import within
from magphase_amd import hostmath as hm
from test_gpu_lossless_kernels import GUARD, SENT, Out, _bits, _dev, _dev_rows, _engine

pytestmark = pytest.mark.gpu

U = scm.U
PAD = 5                       # ld = H + PAD
ENTRY = {False: "mpx_synthesis_compressed_ola", True: "mpx_synthesis_compressed_type2_ola"}

# <= 3 x the worst case measured on the MI355X against the float64 model, in units of u (B + B_lerp)
#                                                              measured, per fft_len (every case of the group)
PIN = {
    "one_row": {1024: 30.0, 2048: 29.0, 4096: 31.0},         # 10.11, 9.78, 10.53 (single-frame cases; multi-frame <= 0.9)
    "rows": {1024: 9.0, 2048: 8.8, 4096: 9.2},               # 3.02, 2.95, 3.07
    "spectra": {4096: 14.9},                                 # 4.97
}
# ... and as fractions of the derived bound: 0.069 / 0.062 / 0.063 (one row), 0.062 / 0.061 / 0.055 (rows), 0.030 (spectra);
# stored against recomputed spectra 0.0002 of twice the bound, identity row tables against the one-row form 0.006, other
# run cuts 0.014 / 0.009 / 0.008 of the re-association allowance.

# (N, row tables, type 2, n_per_bins): every instance but the stored-spectra pair
INSTANCES = [(N, lerp, t2, 0) for N in scm.FFT_LENS for lerp in (False, True) for t2 in (False, True)] + \
            [(4096, False, t2, 449) for t2 in (False, True)]
IDS = ["%d-%s-t%d-nper%d" % (N, "rows" if lerp else "one_row", 2 if t2 else 1, n) for N, lerp, t2, n in INSTANCES]


def _slot_tables(slot_off, n_slots):
    """hostmath.ola_runs deals to at most n_runs slots: the work lists for n_slots slots -- an empty list in second place
    (where there is room) and empty lists at the end."""
    so = [int(x) for x in slot_off]
    if len(so) - 1 < n_slots:
        so.insert(1, so[1] if len(so) > 1 else 0)
    while len(so) - 1 < n_slots:
        so.append(so[-1])
    assert len(so) - 1 == n_slots
    return np.asarray(so, dtype=np.int32)


def _tables(c, n_slots, frames_per_run=None):
    """The run and slot tables of one launch (host only), every store they name checked against pcm_out and the strips."""
    N = c.N
    runs, slot_off, slot_runs = hm.ola_runs(c.pm_rel, c.out_start, c.out_len, c.out_off, N, n_slots,
                                            frames_per_run=frames_per_run or c.frames_per_run)
    n_runs = int(runs.size)
    slot_off = _slot_tables(slot_off, n_slots)
    assert slot_off[-1] == n_runs and sorted(slot_runs.tolist()) == list(range(n_runs))
    assert np.all(runs["head_end"] <= N + 64) and np.all(runs["fix_hi"] <= N + 64) and np.all(runs["fix_lo"] >= 0)
    assert np.array_equal(runs["strip_off"], np.arange(n_runs) * (N + 64))
    total = int(c.out_off[-1])
    for r in runs:                                       # every store of the launch and of the fix-up lies inside pcm_out
        assert r["out_hi"] == r["out_lo"] or (0 <= r["out_base"] + r["out_lo"] and r["out_base"] + r["out_hi"] <= total)
        assert r["fix_hi"] == r["fix_lo"] or (0 <= r["out_base"] + r["fix_lo"] and r["out_base"] + r["fix_hi"] <= total)
        assert 0 <= r["frame_begin"] < r["frame_end"] <= c.F
    return runs, slot_off, slot_runs


def _launch(c, n_slots, spectra=False, frames_per_run=None):
    """One launch and its fix-up into fresh buffers -> (pcm float32 [total_out], runs)."""
    e, N, H, F = _engine(), c.N, c.H, c.F
    ld = H + PAD
    tab = e.tables(N)
    runs, slot_off, slot_runs = _tables(c, n_slots, frames_per_run)
    n_runs, total = int(runs.size), int(c.out_off[-1])
    out = Out(e, 1, total)
    n_strip = n_runs * (N + 64)
    assert int(e.lib.mpx_ola_strip_floats(N)) == N + 64
    strips = torch.full((n_strip + 2 * GUARD,), SENT, dtype=torch.float32, device=e.device)
    strips[GUARD:GUARD + n_strip] = float("nan")
    s_view = strips[GUARD:GUARD + n_strip]
    rdev = torch.from_numpy(np.frombuffer(runs.tobytes(), dtype=np.uint8).copy()).to(e.device)
    noise, npos, nleft, nright, wtype = (_dev(e, c.noise, np.float32), _dev(e, c.npos, np.int64), _dev(e, c.nleft, np.int32),
                                         _dev(e, c.nright, np.int32), _dev(e, c.wtype, np.int32))
    rows = [None, None, None]
    if c.lerp():
        rows = [_dev(e, c.row0, np.int32), _dev(e, c.row1, np.int32), _dev(e, c.row_t, np.float32)]
    args = [N, tab, _dev_rows(e, c.mag, ld), _dev_rows(e, c.real, ld), _dev_rows(e, c.imag, ld), noise, npos, nleft, nright,
            wtype, _dev(e, c.voiced, np.int32), _dev(e, c.inv_gain, np.float32)] + rows + \
           [_dev(e, c.win_l, np.int32), _dev(e, c.win_r, np.int32), _dev(e, c.pm_rel_cat, np.int32),
            _dev(e, c.per_v, np.float32), _dev(e, c.ap_v, np.float32), _dev(e, c.ap_u, np.float32), rdev, n_runs,
            _dev(e, slot_off, np.int32), _dev(e, slot_runs, np.int32), int(n_slots), s_view, out.t, ld, int(c.n_per_bins)]
    if spectra:
        assert N == 4096 and not c.type2 and not c.lerp()
        n_spec = int(e.lib.mpx_noise_spectra_floats(N, F))
        assert n_spec == F * 17 * 64 * 4
        spec = torch.full((n_spec + 2 * GUARD,), float("nan"), dtype=torch.float32, device=e.device)
        sums = Out(e, 1, F)
        e.launch("mpx_noise_stats_spectra", N, tab, noise, npos, nleft, nright, wtype, F, sums.t, spec[GUARD:GUARD + n_spec])
        assert np.all(np.isfinite(sums.check("noise sums")))
        e.launch("mpx_synthesis_compressed_ola_spectra", *args, spec[GUARD:GUARD + n_spec])
    else:
        e.launch(ENTRY[c.type2], *args)
    e.launch("mpx_ola_fixup", N, rdev, n_runs, s_view, out.t)
    got = out.check("pcm_out")[0]
    h = strips.cpu().numpy()
    assert np.all(h[:GUARD] == SENT) and np.all(h[GUARD + n_strip:] == SENT), "written outside the strips"
    assert not np.any(got == SENT), "kept samples that were not written"
    assert np.all(np.isfinite(got)), "NaN or infinity in pcm_out: a read outside the documented extent"
    return got, runs


@functools.lru_cache(maxsize=None)
def _case(kind, N, lerp, type2, n_per, fpr=None):
    make = dict(single=scm.single_frame_case, onehot=scm.one_hot_case, multi=scm.multi_frame_case)[kind]
    c = make(N, lerp, type2, n_per)
    scm.check_case(c)
    return c, scm.synthesis(c)


def _figures(c, m, got):
    """-> (fraction of the derived bound, worst error in units of u (B + B_lerp)); exact zeros where the norm is zero."""
    err = np.abs(np.asarray(got, dtype=np.float64) - m["pcm"])
    B, BL, cnt = m["B"], m["B_lerp"], m["count"]
    live = B > 0
    assert live.any()
    assert not np.asarray(got)[~live].any(), "a sample whose model norm is zero must be an exact zero"
    allow = U * ((scm.derived_units(c.N) + cnt) * B + BL)
    return float(np.max(err[live] / allow[live])), float(np.max(err[live] / (U * (B + BL)[live])))


def _group(c, spectra=False):
    return "spectra" if spectra else ("rows" if c.lerp() else "one_row")


def _hold(c, m, got, tag, spectra=False):
    frac, units = _figures(c, m, got)
    g = _group(c, spectra)
    print("%s N=%d %s t%d n_per=%d F=%d: %.4f of the derived bound (%.0f u), worst %.2f u (B + B_lerp)"
          % (tag, c.N, g, 2 if c.type2 else 1, c.n_per_bins, c.F, frac, scm.derived_units(c.N), units))
    within(frac, 1.0, "SCK_FRACTION_OF_BOUND:%s:%d" % (g, c.N))
    within(units, PIN[g][c.N], "SCK_PINNED_U:%s:%d" % (g, c.N))


# ====================================================================================== single-frame utterances
@pytest.mark.parametrize("N,lerp,type2,n_per", INSTANCES, ids=IDS)
def test_single_frame(N, lerp, type2, n_per):
    """Every frame shape (compressed_kernels_model.noise_shapes, lengths at tile - 1, tile, tile + 1 of both staging tiles,
    L == 0, R == 0) x both noise windows x voiced / unvoiced, one frame per run and per utterance: the output IS the
    windowed frame.  37 slots for more than a hundred runs (several runs per slot, no multiple of the 6 pairs of a
    workgroup)."""
    c, m = _case("single", N, lerp, type2, n_per)
    got, runs = _launch(c, 37)
    assert runs.size == c.F > 37 and not runs["head_end"].any()
    _hold(c, m, got, "single")
    # per frame: where the model's frame is silent outside the window the device is, sample for sample
    per = got.reshape(c.F, N)
    for f in (0, c.F // 2, c.F - 1):
        assert not per[f, :N // 2 - c.win_l[f]].any() and not per[f, N // 2 + c.win_r[f] + 1:].any()


@pytest.mark.parametrize("n_per", (449, 0))
def test_single_frame_stored_spectra(n_per):
    c, m = _case("single", 4096, False, False, n_per)
    got, _ = _launch(c, 37, spectra=True)
    _hold(c, m, got, "single/spectra", spectra=True)


@pytest.mark.parametrize("n_per", (512, 513, 700))
def test_single_frame_at_the_schedules_threshold(n_per):
    """fft_len 4096, one row per frame: 512 takes the n_per <= 512 schedule, 513 and 700 the general one."""
    c, m = _case("single", 4096, False, False, n_per)
    got, _ = _launch(c, 41)
    _hold(c, m, got, "single/threshold")


# ================================================================================================ one-hot spectra
ONE_HOT = [(N, lerp, t2, n) for (N, lerp, t2, _) in INSTANCES[:12] for n in (0, 200)] + \
          [(4096, False, t2, 449) for t2 in (False, True)]


@pytest.mark.parametrize("N,lerp,type2,n_per", ONE_HOT,
                         ids=["%d-%s-t%d-nper%d" % (N, "rows" if l else "one_row", 2 if t else 1, n) for N, l, t, n in ONE_HOT])
def test_one_hot_spectra(N, lerp, type2, n_per):
    """mag one-hot at bins 0, 1, 63, 64, n_per - 1, n_per, M/2 - 1, M/2, M/2 + 1, M - 1, M with the phase a unit phasor at
    six angles (pi and 0 among them: both signs at DC and Nyquist): voiced frames with ap_v == 0 -- the periodic term
    alone, a cosine of one bin whose amplitude, phase and sign the model fixes; from n_per on exact silence --, and unvoiced
    frames (per_v arbitrary, not used).  More slots than runs, one empty list in second place."""
    c, m = _case("onehot", N, lerp, type2, n_per)
    got, runs = _launch(c, c.F + 5)
    _hold(c, m, got, "one-hot")
    per, ref = got.reshape(c.F, N), m["pcm"].reshape(c.F, N)
    eff = scm.eff_n_per(n_per, N)
    silent = (c.voiced == 1) & (c.hot >= eff)
    assert silent.any() == (eff <= N // 2) and not per[silent].any()
    # type 1 gives |X| at bins 0 and N/2, type 2 keeps the sign: the frames with the phasor at pi tell them apart
    for k in (0, N // 2):
        f = np.flatnonzero((c.hot == k) & (c.voiced == 1) & (c.angle == np.pi))
        if k < eff:
            assert f.size == 1
            centre = per[f[0], N // 2]
            assert abs(ref[f[0], N // 2]) > 1e-5 and np.sign(centre) == np.sign(ref[f[0], N // 2])
            assert (centre < 0) == bool(type2)


# ================================================================================================== n_per_bins sweep
@pytest.mark.parametrize("N", scm.FFT_LENS)
@pytest.mark.parametrize("type2", (False, True), ids=("t1", "t2"))
def test_n_per_sweep(N, type2):
    """n_per_bins over 1, 63, 64, 65, 511, 512, 513, M/2, M/2 + 1, M/2 + 2, M/2 + 64, M/2 + 65, M - 63, M - 1, M, M + 1, 0 and
    H + 7 (where the value exists): per_v is nonzero exactly below n_per, real / imag are NaN on exactly the complement of
    the documented read set and large (1e3 x) on its bins from n_per on.  As many slots as runs."""
    for n_per in scm.n_per_values(N):
        c = scm.n_per_case(N, type2, n_per)
        scm.check_case(c)
        got, _ = _launch(c, c.F)
        _hold(c, scm.synthesis(c), got, "n_per")


# ================================================================================================= multi-frame runs
@pytest.mark.parametrize("N,lerp,type2,n_per", INSTANCES, ids=IDS)
def test_multi_frame(N, lerp, type2, n_per):
    """Six utterances of 2, 23, 41, 1, 57 and 30 frames whose noise-frame lengths go short -> long -> short, long -> short,
    all longer than a tile, and alternate (with the window type and the voicing): the prefetch of the next frame's tile in
    both orders; several runs per utterance: head strips and the fix-up."""
    c, m = _case("multi", N, lerp, type2, n_per)
    got, runs = _launch(c, 7)
    per_run = runs["frame_end"] - runs["frame_begin"]
    assert runs.size > 7 and runs["head_end"].any() and (runs["fix_hi"] > runs["fix_lo"]).any()
    assert per_run.min() >= 1 and per_run.max() <= 40 and (per_run >= 2).sum() >= 4
    _hold(c, m, got, "multi")
    again, _ = _launch(c, 7)
    assert np.array_equal(_bits(again), _bits(got)), "the same tables twice"
    other, runs11 = _launch(c, 11)
    assert np.array_equal(runs11.tobytes(), runs.tobytes())
    assert np.array_equal(_bits(other), _bits(got)), "the same runs dealt to 11 slots instead of 7"
    recut, runs2 = _launch(c, 7, frames_per_run=2 * c.frames_per_run + 3)
    assert runs2.size != runs.size
    _hold(c, m, recut, "multi/recut")
    d = np.abs(recut.astype(np.float64) - got)
    live = m["B"] > 0
    within(float(np.max(d[live] / (2 * np.maximum(m["count"], 1) * U * m["B"])[live])), 1.0, "SCK_RECUT_REASSOCIATION:%d" % N)


@pytest.mark.parametrize("n_per", (449, 0))
def test_stored_spectra_against_recomputed(n_per):
    """mpx_noise_stats_spectra -> mpx_synthesis_compressed_ola_spectra against mpx_synthesis_compressed_ola on the same
    tables: k_noise_stats and the pair kernel transform the frame by different instances (full-height / compact exchange),
    so the two differ by float32 rounding -- each is within the derived bound of the model, the pair within twice it."""
    c, m = _case("multi", 4096, False, False, n_per)
    stored, _ = _launch(c, 7, spectra=True)
    plain, _ = _launch(c, 7)
    _hold(c, m, stored, "multi/spectra", spectra=True)
    allow = 2 * U * (scm.derived_units(c.N) + m["count"]) * m["B"]
    live = m["B"] > 0
    d = np.abs(stored.astype(np.float64) - plain)
    print("stored vs recomputed n_per=%d: %.4f of twice the derived bound" % (n_per, np.max(d[live] / allow[live])))
    within(float(np.max(d[live] / allow[live])), 1.0, "SCK_STORED_VS_RECOMPUTED")
    assert not stored[~live].any() and not plain[~live].any()


@pytest.mark.parametrize("N", scm.FFT_LENS)
@pytest.mark.parametrize("type2", (False, True), ids=("t1", "t2"))
def test_identity_row_tables_against_the_one_row_form(N, type2):
    """row0 == row1 == f, row_t == 0: the interpolation is exact (fma(0, 0, x) = x), the same spectrum goes through the
    other instance's split and merge -- the two differ by float32 rounding, within twice the derived bound."""
    c, m = _case("single", N, False, type2, 0)
    ident = scm.identity_tables(c)
    scm.check_case(ident)
    a, _ = _launch(c, 37)
    b, _ = _launch(ident, 37)
    _hold(ident, scm.synthesis(ident), b, "identity rows")
    allow = 2 * U * scm.derived_units(N) * m["B"]
    live = m["B"] > 0
    within(float(np.max(np.abs(a.astype(np.float64) - b)[live] / allow[live])), 1.0, "SCK_IDENTITY_ROWS_VS_ONE_ROW:%d" % N)
