"""GPU: the float64 analysis front end (magphase_f64.hip), each kernel launched through its C entry with tables built by
hand, against tests/f64_analysis_model.py (held to the oracle and to a longdouble DFT by tests/test_f64_analysis_host.py):

  part A   k_analysis_f64<P>          mpx_analysis_frames_f64 (the analytic window everywhere) and mpx_analysis_frames_f64w
                                      with Engine.hann_table() (numpy's weights for halves <= HANN_TABLE_CAP), P = 8, 16, 32
  part B   k_analysis_warp_fused<P>   mpx_analysis_compressed_fused, P = 16, 32

Every output is a view into a buffer filled with a sentinel, with guard runs before and after (part A: and a row pitch of
H + 3): whatever the entry is not documented to write must still hold the sentinel.  Every floating-point operand lies
between runs of NaN and the signal is NaN in every sample outside a frame's [pos - L, pos - L + len): one NaN in an output
is a read outside the extent.  No frame and no bin is left out of a comparison of X or of the magnitude.

Part A, derived bounds.  u = 2^-24, v = 2^-53, l1 = ||w x||_1 of the windowed frame, sx = sum |x| of its samples,
L2N = log2(fft_len).  Per bin, X = mag (real + j imag) formed in float64 from the float32 outputs:

  |X_dev - X_model| <= REL |X_model| + c_N v l1 [+ c_w v sx + (where the device wrote (0, 0, 0)) 2^-45 l1] + 1e-27

  REL = 2 u + 2^-44   the float32 roundings of the outputs: mag <= 1 u of |X|; real and imag <= 1 u of their own size each,
                      so the phasor moves by <= 1 u as a vector (REL |X| is the form 2^-24 |X_model| with both
                      contributions counted: they add up to 2 u when they point the same way).  2^-44 = 5.7e-14: the
                      reciprocal square root (one Newton step on the fp32 estimate, 1.5 e0^2 < 3e-14) and its products.
  c_N = 5 L2N + 12 + MODEL_ERR_UNITS L2N / 10
                      per butterfly level 5 as for the float32 kernel (table twiddle 1, complex product 3, sum 1; L2N - 1
                      levels of the N/2-point transform and the real-FFT split counted as one more); weight x sample 1 (the
                      2^30 scaling of the table path is exact); the split: lane twiddle (sincospi 2, constant 1, complex
                      product 3) 6, E / T sums 2, T product 3.  MODEL_ERR_UNITS: np.fft's own distance from the longdouble
                      DFT, measured on the CPU at fft_len 1024 (tests/test_f64_analysis_host.py) and scaled with the levels.
  c_w = 17            frames whose window is evaluated on the device (no table, or a half above its cap) only.  np.hanning:
                      the argument pi n / (M - 1) carries 2.5 v relative, 8 v at pi, the cosine 1 v more, halved, one sum:
                      5 v absolute.  The device: t = k (1 / L) 2 v, pi t / 2 1 v, the polynomial 2 v, squared: 11 v of a
                      weight below 0.5 or of 1 - weight, one more rounding above: 12 v.  (Measured on the CPU in longdouble:
                      np.hanning 2.3 v, the device's formula without fma 2.9 v.)
  2^-45 l1            the analytic path stores (0, 0, 0) where |X| <= 2^-45 (float32 sum of |w x|): allowed for exactly
                      those bins; 2^-45 (1 + 2^-20) for the float32 sum.  1e-27: the table path's flush, 1e-18 / 2^30.

  |mag_dev - mag_model| is held to the same figure with REL_MAG = u + 2^-44 in the place of REL: the magnitude is rounded
  once.  real and imag ALONE: on every bin with |X_model| >= 2^-20 l1, within 2^-24 + that magnitude bound / |X_model|
  (the component's own rounding, and what moved the bin before it: 2 u and the absolute terms over |X|); on the noise and one-hot rows that is every bin (asserted: the excluded share is 0), the DC and
  alternation rows have cancelling bins and their share is noted (F64K_PHASOR_EXCLUDED_*).  A frame whose model row is
  exactly zero -- zero samples, or one sample under a window weight of exactly 0 -- gives exact zeros.
  |real^2 + imag^2 - 1| <= 4 * 2^-23 wherever mag > 0.

Part B, derived bound: |y_dev - y_model| <= (terms + 8) u |pre(x)| @ |W|^T + eps_pre max(|pre(x)|, 1) @ |W|^T, pre the
prologue of the model's float64 row.  terms = 16 + P/2 + 8 + 1: a product is added to a fresh accumulator with the 15 others
of its wave's 16 columns of the chunk, the chunk sums to the round's accumulator (P/2 of them), the eight waves' slices are
summed, and bin M/2 is one fused multiply-add.  eps_pre: the fused kernel's operands are formed in float32 from the float64
spectrum (|X| and the phasor within 2 ulp, the logarithm, a quadratic for the phase operand's 1e-8 e^{-2x}), not by the staged
warp's prologue, so it is measured here by one-hot matrices, relative to max(|pre|, 1) as in
tests/test_gpu_compressed_kernels.py.  That file multiplies its eps_pre by |pre| @ |W|^T; here it multiplies
max(|pre|, 1) @ |W|^T, the norm it is measured in (where a prologue crosses zero its error is absolute) -- a slightly looser
form than the one that file uses, and like the 2 u of part A a stated deviation; the pins below stand far inside both.  Unvoiced rows: +0.0 bit for bit; the -1e10 floor exactly where the model has it.

The derived fractions are also pinned at <= 3 x the worst case measured on the MI355X against the model (the values stand
beside the constants; profiles/r25_f64_analysis_kernels_tolerance_report.json, DESIGN.md "Kernel tests of the float64
analysis front end").

Launch geometry the shapes are chosen by: k_analysis_f64 runs 8 waves (frames in flight) per workgroup on at most one
workgroup per CU, the frames pulled from an LDS queue; k_analysis_warp_fused 8 frames per round, rounds dealt round-robin."""
import functools

import numpy as np
import pytest
import torch

import compressed_kernels_model as ckm
import f64_analysis_model as fm
from _tol import note, within
from magphase_amd import hostmath as hm

pytestmark = pytest.mark.gpu

U, V = 2.0 ** -24, 2.0 ** -53
LD = np.longdouble
SENT = -77.25
GUARD = 64
NAN_GUARD = 2112
WAVES = 8                                 # kAna64Waves, kFusedWaves
PATHS = ("analytic", "table")
REL = 2 * U + 2.0 ** -44
REL_MAG = U + 2.0 ** -44
C_W = 17.0
FLUSH = 2.0 ** -45 * (1 + 2.0 ** -20)
ABS_FLOOR = 1.0e-27
PHASOR_MIN = 2.0 ** -20


def c_n(N):
    return 5 * np.log2(N) + 12 + fm.MODEL_ERR_UNITS * np.log2(N) / 10


# ---- pinned at <= 3 x the worst case measured on the MI355X (fraction of the derived bound, every frame of the file) ----
# X reaches 0.82 .. 0.83 of its derived bound at every fft_len on both paths (the float32 roundings of the outputs: 1.65 u
# |X|) and mag 0.9992 .. 0.9999 of its own (one rounding of nearly u), so the derived bounds ARE within 3 x the measurement and carry no
# pin.  real / imag alone: 0.25 (half an ulp of a component in [0.5, 1), 2^-25, of an allowance of 2 u) at every fft_len on
# both paths.
PIN_PHASOR = 0.5
# part B.  The fused prologues' own error relative to max(|pre|, 1): measured 2.66e-7 (mode 0: ln(|X|^2 + 1e-8)), 1.71e-7
# (mode 1: the phase operand), 2.14e-7 (mode 2: ln|X|)
FUSED_EPS_PRE = {0: 7.5e-7, 1: 5.0e-7, 2: 6.0e-7}
# fraction of the warp bound, [fft_len][mag_fbank]: measured 0.0109 / 0.1195 at 2048 and 0.00705 / 0.0899 at 4096, each on
# the batch of 2 051 short frames (the derived bound adds every rounding of 2049 terms in one direction and stands 8 - 140 x
# above the device)
PIN_FUSED = {2048: {0: 0.025, 1: 0.23}, 4096: {0: 0.017, 1: 0.19}}


def _engine():
    from magphase_amd.engine import get_engine
    return get_engine()


def _cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _dev(e, a, dtype=None):
    """Upload.  A floating-point operand lies between two runs of NAN_GUARD NaNs."""
    a = np.ascontiguousarray(a, dtype=dtype)
    if not np.issubdtype(a.dtype, np.floating):
        return torch.from_numpy(a.reshape(-1) if a.size else np.zeros(1, a.dtype)).to(e.device)
    buf = np.full(a.size + 2 * NAN_GUARD, np.nan, dtype=a.dtype)
    buf[NAN_GUARD:NAN_GUARD + a.size] = a.ravel()
    return torch.from_numpy(buf).to(e.device)[NAN_GUARD:NAN_GUARD + a.size]


class Out:
    """rows x cols float32 written with pitch ld inside a sentinel-filled buffer with guards."""

    def __init__(self, e, rows, cols, ld=None):
        self.rows, self.cols, self.ld = int(rows), int(cols), int(ld or cols)
        h = np.full(2 * GUARD + self.rows * self.ld, SENT, dtype=np.float32)
        self.buf = torch.from_numpy(h).to(e.device)
        self.t = self.buf[GUARD:]

    def check(self, what):
        """-> the rows; guards and pad columns must hold the sentinel."""
        torch.cuda.synchronize()
        h = self.buf.cpu().numpy()
        n = self.rows * self.ld
        assert np.all(h[:GUARD] == SENT), what + ": written before the buffer"
        assert np.all(h[GUARD + n:] == SENT), what + ": written past the buffer"
        body = h[GUARD:GUARD + n].reshape(self.rows, self.ld)
        assert np.all(body[:, self.cols:] == SENT), what + ": written beyond a row's last column"
        return body[:, :self.cols].copy()


# ===================================================================== part A: mpx_analysis_frames_f64 / _f64w
def _launch_analysis(e, N, path, sig, pos, left, right, ld, flags=None):
    H, F = N // 2 + 1, len(pos)
    outs = [Out(e, F, H, ld) for _ in range(3)]
    args = (N, e.tables_f64(N), _dev(e, sig, np.float32), _dev(e, pos, np.int64), _dev(e, left, np.int32),
            _dev(e, right, np.int32), F, outs[0].t, outs[1].t, outs[2].t, ld, None if flags is None else _dev(e, flags, np.float32))
    if path == "analytic":
        e.launch("mpx_analysis_frames_f64", *args)
    else:
        e.launch("mpx_analysis_frames_f64w", *(args + (e.hann_table(), hm.HANN_TABLE_CAP)))
    return [o.check("analysis_f64 %s %s" % (path, s)) for o, s in zip(outs, ("mag", "real", "imag"))]


@functools.lru_cache(maxsize=None)
def _analysis_case(N, path):
    """Every geometry x every signal of fft_len N in ONE launch (f64_analysis_model.analysis_case)."""
    c = dict(fm.analysis_case(N))
    c["ld"] = N // 2 + 1 + 3
    c["dev"] = _launch_analysis(_engine(), N, path, c["sig"], c["pos"], c["left"], c["right"], c["ld"])
    c["analytic"] = fm.analytic_frames(c["left"], c["right"], path == "table")
    return c


def _analysis_figures(dev, model, analytic, N, rows=None):
    """Every bin of the frames `rows` (all by default) against the model -> dict of the figures as fractions of the bounds;
    nothing asserted but that no output is NaN."""
    rows = slice(None) if rows is None else rows
    mag, real, imag = [np.asarray(x, dtype=np.float64)[rows] for x in dev]
    r_mag, r_real, r_imag, l1, sx = [x[rows] for x in model]
    analytic = np.asarray(analytic)[rows]
    assert not np.isnan(mag).any() and not np.isnan(real).any() and not np.isnan(imag).any(), "a read outside a frame"
    X, Xr = mag * (real + 1j * imag), r_mag * (r_real + 1j * r_imag)
    live = l1 > 0
    fig = dict(x=0.0, mag=0.0, real=0.0, imag=0.0, dead=0.0, n=len(l1), excluded=0.0, flat_rel_u=0.0)
    if np.any(live):
        absolute = (c_n(N) * V * l1 + analytic * (C_W * V * sx))[:, None] + ABS_FLOOR
        absolute = absolute + ((mag == 0) & analytic[:, None]) * (FLUSH * l1)[:, None]
        bound, bound_mag = REL * r_mag + absolute, REL_MAG * r_mag + absolute
        fig["x"] = float(np.max((np.abs(X - Xr) / bound)[live]))
        fig["mag"] = float(np.max((np.abs(mag - r_mag) / bound_mag)[live]))
        flat = live & (np.max(r_mag, axis=1) - np.min(r_mag, axis=1) <= 1e-12 * l1)   # one-hot rows: |X| = l1 in every bin
        fig["flat_rel_u"] = float(np.max((np.abs(X - Xr) / np.maximum(r_mag, 1e-300))[flat])) / U if np.any(flat) else 0.0
        big = (r_mag >= PHASOR_MIN * l1[:, None]) & live[:, None]
        allow = U + bound_mag[big] / r_mag[big]
        fig["real"] = float(np.max(np.abs(real - r_real)[big] / allow))
        fig["imag"] = float(np.max(np.abs(imag - r_imag)[big] / allow))
        fig["excluded"] = float(1.0 - big[live].sum() / big[live].size)
    if np.any(~live):       # the model is exactly zero (zero samples, or one sample under a window weight of 0)
        fig["dead"] = float(max(np.abs(x[~live]).max() for x in (mag, real, imag)))
    fig["norm"] = float(np.max(np.abs(real ** 2 + imag ** 2 - 1.0)[mag > 0])) if np.any(mag > 0) else 0.0
    return fig


def _hold_analysis(dev, model, analytic, N, path, tag, rows=None, excluded_must_be_zero=False, hold=True, say=True):
    """Prints the figures (hold False: that is all), then holds them to the derived bounds and to the pins."""
    fig = _analysis_figures(dev, model, analytic, N, rows)
    if say:
        print("%s %s N=%d (%d frames): |dX| %.4g |dmag| %.4g real %.4g imag %.4g of the bound; flat rows |dX| / |X| %.4g u; "
              "|phasor|^2 - 1 %.2e; excluded from real / imag alone %.3g; frames with a zero model: max |out| %.3g"
              % (tag, path, N, fig["n"], fig["x"], fig["mag"], fig["real"], fig["imag"], fig["flat_rel_u"], fig["norm"],
                 fig["excluded"], fig["dead"]))
    if not hold:
        return fig
    assert fig["dead"] == 0.0, "a frame whose model is exactly zero must give exact zeros"
    if excluded_must_be_zero:
        assert fig["excluded"] == 0.0, "every bin of a noise or one-hot row is above 2^-20 l1"
    else:
        note("F64K_PHASOR_EXCLUDED_%s_%s_%d" % (tag, path, N), fig["excluded"])
    for key, name in (("x", "X"), ("mag", "MAG"), ("real", "PHASOR"), ("imag", "PHASOR")):
        within(fig[key], 1.0, "F64K_%s_FRACTION_OF_BOUND_%s_%d" % (name, path.upper(), N))
    for key in ("real", "imag"):
        within(fig[key], PIN_PHASOR, "F64K_PHASOR_PINNED_FRACTION_%s_%d" % (path.upper(), N))
    within(fig["norm"], 4 * 2.0 ** -23, "F64K_UNIT_PHASOR")
    return fig


@pytest.mark.parametrize("N", fm.FFT_LENS)
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("kind", ("noise", "dc", "alt", "zero"))
def test_analysis_every_geometry_within_the_derived_bound(N, path, kind):
    c = _analysis_case(N, path)
    rows = c["kinds"] == kind
    assert rows.sum() == len(fm.geometries(N)) == 150
    _hold_analysis(c["dev"], c["model"], c["analytic"], N, path, kind, rows, excluded_must_be_zero=(kind == "noise"))
    if kind == "zero":
        for x in c["dev"]:
            assert not x[rows].any()


@pytest.mark.parametrize("N", fm.FFT_LENS)
@pytest.mark.parametrize("path", PATHS)
def test_analysis_one_hot_rows_within_the_derived_bound(N, path):
    """One sample of 0.75 at frame offset 0, 1, L - 1, L, L + 1, len - 1 of every geometry: the model's row has |w x| in
    every bin, so every bin -- real and imag alone included -- is held to the bound at the scale of that one product.

    This test found that the analytic window was accurate to 2.2e-14 of FULL SCALE, not of the weight: hann_half_f64
    evaluated 0.5 + 0.5 sin(pi (t - 0.5)) at every t with a Taylor polynomial whose remainder at pi/2 is 4e-14.  On the
    MI355X a sample under a weight of exactly 0 (offset 0 with L > 0, len - 1 with R > 0) gave unit phasors where the
    model's row is (0, 0, 0), at every fft_len, and with the table too wherever a half is above its cap; a sample at
    offset 1 or len - 1 of a frame with a half of 4296 samples (fft_len 4096) came out 3.82 / 3.55 u off, 1.71 / 1.60 of this
    bound, where the other offsets stay below 1.65 u (at 1024 / 2048 the longest halves, 2049 / 2248, add 0.6 u in
    emulation and stayed inside the bound: 1.58 u).  hann_half_f64 now takes sin(pi t / 2)^2 below t = 0.5 and
    1 - sin(pi (1 - t) / 2)^2 above, exactly 0 and 1 at the ends: 1.49 u at the worst offset, exact zeros (DESIGN.md,
    "Kernel tests of the float64 analysis front end")."""
    c = _analysis_case(N, path)
    for hold in (False, True):          # every offset's figures are printed before the first is held
        for name in fm.ONE_HOT_AT:
            rows = c["kinds"] == "onehot:" + name
            assert rows.sum() > 50
            _hold_analysis(c["dev"], c["model"], c["analytic"], N, path, "onehot:" + name, rows, excluded_must_be_zero=True,
                           hold=hold, say=not hold)


@pytest.mark.parametrize("N", fm.FFT_LENS)
@pytest.mark.parametrize("path", PATHS)
def test_analysis_rows_in_use_repeated_and_dense_launches(N, path):
    """rows_in_use with period 3: a flagged-off row keeps the sentinel in real / imag bit for bit and has the unflagged
    launch's magnitudes; everything else, a repeated launch and a launch with the dense pitch are bit-identical."""
    c, e = _analysis_case(N, path), _engine()
    tabs = (c["sig"], c["pos"], c["left"], c["right"])
    again = _launch_analysis(e, N, path, *tabs, c["ld"])
    dense = _launch_analysis(e, N, path, *tabs, N // 2 + 1)
    for a, b, d in zip(c["dev"], again, dense):
        assert _same_bits(a, b) and _same_bits(a, d)
    flags = (np.arange(len(c["pos"])) % 3 != 1).astype(np.float32)
    flags[flags != 0] = np.where(np.arange(int(flags.sum())) % 2, 1.0, 0.5)      # any non-zero value is "in use"
    part = _launch_analysis(e, N, path, *tabs, c["ld"], flags)
    on = flags != 0
    assert (~on).sum() > 400 and _same_bits(part[0], c["dev"][0])
    for s in (1, 2):
        assert _same_bits(part[s][on], c["dev"][s][on])
        assert np.all(_bits(part[s][~on]) == _bits(np.float32(SENT)))
    ones = _launch_analysis(e, N, path, *tabs, c["ld"], np.ones(len(c["pos"]), np.float32))
    assert all(_same_bits(a, b) for a, b in zip(ones, c["dev"]))


@pytest.mark.parametrize("N", fm.FFT_LENS)
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("F", (1, WAVES - 1, WAVES, WAVES + 1, "queue"))
def test_analysis_frame_counts(F, path, N):
    """1, 7, 8, 9 frames, and 8 x CUs x 2 + 3 short frames overlapping in one signal (every workgroup pulls more than one
    round of eight frames from its LDS queue, which lies at a P-dependent offset in front of the window regions), at every
    fft_len on both paths.  The frames are noise: real / imag alone are compared on every bin."""
    n = WAVES * _cus() * 2 + 3 if F == "queue" else F
    (sig, pos, left, right), model = fm.count_model(N, n)
    dev = _launch_analysis(_engine(), N, path, sig, pos, left, right, N // 2 + 1 + 3)
    _hold_analysis(dev, model, fm.analytic_frames(left, right, path == "table"), N, path, "count_%s" % F, None,
                   excluded_must_be_zero=True)


# ===================================================================== part B: mpx_analysis_compressed_fused
def fused_terms(N):
    return 16 + N // 256 + 8 + 1


def _pack(e, w_mag, w_ph, N):
    nw, layout = int(e.lib.mpx_analysis_compressed_fused_waves()), int(e.lib.mpx_analysis_compressed_fused_layout())
    wpack, whalf = hm.pack_warp_fused(w_mag.astype(np.float64), w_ph.astype(np.float64), N, n_waves=nw, layout=layout)
    return _dev(e, wpack, np.float32), _dev(e, whalf, np.float32)


def _launch_fused(e, N, tabs, w_mag, w_ph, voi, fbank, table=True):
    sig, pos, left, right = tabs
    F, md, pd = len(pos), w_mag.shape[0], w_ph.shape[0]
    outs = [Out(e, F, md), Out(e, F, pd), Out(e, F, pd)]
    wpack, whalf = _pack(e, w_mag, w_ph, N)
    win = (e.hann_table(), hm.HANN_TABLE_CAP) if table else (None, 0)
    e.launch("mpx_analysis_compressed_fused", N, e.tables_f64(N), _dev(e, sig, np.float32), _dev(e, pos, np.int64),
             _dev(e, left, np.int32), _dev(e, right, np.int32), F, win[0], win[1], wpack, whalf, md, pd,
             _dev(e, voi, np.float32), int(fbank), outs[0].t, outs[1].t, outs[2].t)
    return [o.check("fused %s" % s) for o, s in zip(outs, ("mag", "real", "imag"))]


@functools.lru_cache(maxsize=None)
def _fused_frames(N):
    """The geometries of f64_analysis_model.fused_geometries with the noise signal, one frame of zeros, and the model's rows."""
    rng = np.random.default_rng(N + 5)
    frames = [(L, R, fm.frame_signals(L, R, N, rng)[0][1]) for L, R in fm.fused_geometries(N)]
    frames.insert(11, (30, 30, np.zeros(61, np.float32)))
    tabs = fm.layout_frames(frames)
    return tabs, fm.model_rows(*tabs, N)


def _hold_fused(got, rows, w_mag, w_ph, voi, fbank, N, what):
    """-> the largest fraction of the warp bound; the masks and the floor are asserted here."""
    ref, absdot, pre1 = fm.fused_model(rows, w_mag, w_ph, voi, fbank)
    mode = 2 if fbank else 0
    eps = (FUSED_EPS_PRE[mode], FUSED_EPS_PRE[1], FUSED_EPS_PRE[1])
    worst = 0.0
    for k in range(3):
        g = got[k]
        assert not np.isnan(g).any(), what + ": a read outside a frame or a matrix"
        bound = (fused_terms(N) + 8) * U * absdot[k] + eps[k] * pre1[k]
        if k == 0 and fbank:
            floor = np.asarray(ref[0] == LD(ckm.MAGIC))
            assert np.array_equal(g == np.float32(ckm.MAGIC), floor), what + ": the -1e10 floor"
        else:
            floor = np.zeros(g.shape, dtype=bool)
        if k > 0:
            off = np.asarray(voi) == 0
            assert np.all(_bits(g[off]) == 0), what + ": unvoiced rows are +0.0"
        frac = np.abs(g.astype(LD) - ref[k]) / bound
        worst = max(worst, float(np.max(frac[~floor])) if np.any(~floor) else 0.0)
    return worst


def _fused_check(N, md, pd, fbank, voi_kind="mixed", F=None, table=True, seed=0):
    e = _engine()
    tabs, rows = _fused_frames(N)
    F = len(tabs[1]) if F is None else F
    tabs, rows = (tabs[0],) + tuple(t[:F] for t in tabs[1:]), tuple(r[:F] for r in rows)
    H = N // 2 + 1
    w_mag, w_ph = ckm.warp_matrices(md, pd, H, seed=100 * md + pd + seed)
    if fbank:
        w_mag = np.abs(w_mag)
    voi = {"mixed": ckm.voicing(F, seed=F + md), "voiced": np.ones(F, np.float32), "unvoiced": np.zeros(F, np.float32)}[voi_kind]
    got = _launch_fused(e, N, tabs, w_mag, w_ph, voi, fbank, table)
    what = "fused N %d F %d %d/%d fbank %d %s" % (N, F, md, pd, fbank, voi_kind)
    worst = _hold_fused(got, rows, w_mag, w_ph, voi, fbank, N, what)
    print("%s: %.4f of the warp bound" % (what, worst))
    within(worst, 1.0, "F64K_FUSED_FRACTION_OF_BOUND_%d" % N)
    within(worst, PIN_FUSED[N][fbank], "F64K_FUSED_PINNED_FRACTION_%d_FBANK%d" % (N, fbank))
    return e, tabs, w_mag, w_ph, voi, got


@pytest.mark.parametrize("N", (2048, 4096))
def test_fused_one_hot_matrices_return_the_prologue_of_the_named_bin(N):
    """W[i] = c e_{k_i} (c = 1 for the magnitudes, 1/4 for the phase streams: a power of two, and sums of exact zeros are
    exact), so an output is the kernel's operand of bin k_i times c: pins hostmath.pack_warp_fused's fragment order bin by
    bin -- bins 0, M/2 and M, the chunk edges -- and measures the fused prologues' own error eps_pre against the model."""
    e = _engine()
    tabs, rows = _fused_frames(N)
    H, F = N // 2 + 1, len(tabs[1])
    edges = sorted({0, 1, 63, 64, 65, 127, 128, N // 4 - 1, N // 4, N // 4 + 1, N // 2 - 64, N // 2 - 63, N // 2 - 1, N // 2})
    rs = np.random.RandomState(N)
    voi = np.ones(F, np.float32)
    for fbank in (0, 1):
        k_mag = np.concatenate((edges, rs.choice(np.setdiff1d(np.arange(H), edges), 64 - len(edges), replace=False)))
        k_ph = np.concatenate((edges, rs.choice(np.setdiff1d(np.arange(H), edges), 48 - len(edges), replace=False)))
        w_mag, w_ph = np.zeros((64, H), np.float32), np.zeros((48, H), np.float32)
        w_mag[np.arange(64), k_mag] = 1.0
        w_ph[np.arange(48), k_ph] = 0.25
        got = _launch_fused(e, N, tabs, w_mag, w_ph, voi, fbank)
        mode = 2 if fbank else 0
        for g, x, ks, m, c in ((got[0], rows[0], k_mag, mode, 1.0), (got[1], rows[1], k_ph, 1, 0.25), (got[2], rows[2], k_ph, 1, 0.25)):
            pre = ckm.warp_prologue_ref(m, x[:, ks])
            if m == 2:      # (an exact zero: -1e10, floored again after the product)
                assert np.array_equal(g == np.float32(ckm.MAGIC), np.asarray(pre == LD(ckm.MAGIC)))
            eps = float(np.max(np.abs(g.astype(LD) / c - pre) / np.maximum(np.abs(pre), 1)))
            print("fused one-hot N %d fbank %d: prologue of mode %d, error %.3g of max(|pre|, 1)" % (N, fbank, m, eps))
            within(eps, FUSED_EPS_PRE[m], "F64K_FUSED_EPS_PRE_%d" % m)


@pytest.mark.parametrize("N", (2048, 4096))
@pytest.mark.parametrize("fbank", (0, 1))
@pytest.mark.parametrize("md,pd", fm.FUSED_DIMS)
def test_fused_every_dimension_within_the_warp_bound(N, md, pd, fbank):
    """Distinct matrix entries (a permuted fragment shows), voicing about two thirds; a repeated launch is bit-identical."""
    e, tabs, w_mag, w_ph, voi, got = _fused_check(N, md, pd, fbank)
    again = _launch_fused(e, N, tabs, w_mag, w_ph, voi, fbank)
    assert all(_same_bits(a, b) for a, b in zip(got, again))


@pytest.mark.parametrize("N", (2048, 4096))
@pytest.mark.parametrize("F", fm.FUSED_COUNTS)
def test_fused_frame_counts(N, F):
    _fused_check(N, 60, 45 if F % 2 else 10, 0, F=F)


@pytest.mark.parametrize("N", (2048, 4096))
@pytest.mark.parametrize("voi_kind", ("voiced", "unvoiced"))
def test_fused_all_voiced_and_all_unvoiced(N, voi_kind):
    _fused_check(N, 60, 45, 0, voi_kind=voi_kind)
    _fused_check(N, 33, 32, 1, voi_kind=voi_kind)


@pytest.mark.parametrize("N", (2048, 4096))
def test_fused_without_the_table_every_window_is_analytic(N):
    _fused_check(N, 60, 10, 0, table=False)


@pytest.mark.parametrize("N,md,pd,fbank", ((2048, 17, 17, 0), (2048, 60, 45, 1), (4096, 60, 45, 0), (4096, 33, 32, 1)))
def test_fused_short_frames_give_workgroups_a_second_round(N, md, pd, fbank):
    """8 x CUs + 3 short frames overlapping in one signal: CUs + 1 rounds over at most CUs resident workgroups, so a workgroup
    re-enters the round loop and reuses the reduction buffer, the bin-M/2 values and the tiles that lie over the window
    regions -- at both fft_len, with two and with three phase tiles (60 / 45 at 4096 is the four-buffer form)."""
    e = _engine()
    F = WAVES * _cus() + 3
    tabs, rows = fm.count_model(N, F)
    w_mag, w_ph = ckm.warp_matrices(md, pd, N // 2 + 1, seed=9 + md)
    if fbank:
        w_mag = np.abs(w_mag)
    voi = ckm.voicing(F, seed=3)
    got = _launch_fused(e, N, tabs, w_mag, w_ph, voi, fbank)
    worst = _hold_fused(got, rows, w_mag, w_ph, voi, fbank, N, "fused short frames")
    print("fused short frames N %d F %d %d/%d fbank %d: %.4f of the warp bound" % (N, F, md, pd, fbank, worst))
    within(worst, 1.0, "F64K_FUSED_FRACTION_OF_BOUND_%d" % N)
    within(worst, PIN_FUSED[N][fbank], "F64K_FUSED_PINNED_FRACTION_%d_FBANK%d" % (N, fbank))
