"""GPU: the six kernels of the lossless path that have a C entry of their own, each launched through Engine.launch with
tables built by hand, against tests/lossless_kernels_model.py (held to the oracle by tests/test_lossless_kernels_host.py):

  k_analysis<P>            mpx_analysis_frames             k_ola_fixup           mpx_ola_fixup, mpx_ola_fixup_width
  k_synth_lossless<P>      mpx_synthesis_lossless_frames   k_rows_lerp           mpx_rows_lerp
  k_ola_gather             mpx_ola_gather                  k_rows_lerp_adjoint   mpx_rows_lerp_adjoint

Every output is a view into a buffer filled with a sentinel, with guard runs before and after and (where the entry takes a
pitch) a row pitch wider than the row: whatever the entry is not documented to write must still hold the sentinel.  Every
floating-point operand lies between runs of NaN, the signal of mpx_analysis_frames is NaN in every sample outside a frame's
[pos - L, pos - L + len), source rows and strip elements that no table entry names are NaN: one NaN in an output is a read
outside the extent.  No frame, row, bin or sample is left out of a comparison, except that real / imag ALONE are compared
on bins above 1e-5 of the frame's peak (as tests/test_gpu_lossless.py does; the share is noted as LK_ANA_REAL_IMAG_EXCLUDED).

Derived bounds, u = 2^-24, one rounding <= 1 u of its result, L2N = log2(fft_len):

  analysis     |X_dev - X_model| <= (5 L2N + 28) u ||w x||_1 per bin, X = mag (real + j imag), ||w x||_1 of the windowed
               frame.  Per butterfly level (L2N - 1 levels of the N/2-point complex transform, the real-FFT split counted
               as the last): table twiddle 1, complex product 3, sum 1.  Constant part: window weight 10 (1 / L and
               k x (1 / L): 2, at most doubled by sin^2; the polynomial, sin(pi u) = u p and its square: 5 relative
               below t = 0.375, (1 + w) / w <= 4.3 above), weight x sample 1, split twiddle (sincospif 2, constant 1,
               complex product 3) + E / T sums 2 + T product 3, epilogue 8 (s2 = xr^2 + xi^2: 2, rsq: 2 each time it is
               used, three products): 30, of which the split's 5 as a level are counted twice -- the 28 stands.
               |mag_dev - mag_model| is held to the same figure.
  synthesis    |y_dev - y_model| <= (5 L2N + 14) u sum_k c_k mag_k / N per sample (c_k = 1 at bins 0 and N/2, else 2): unit
               phasor 6 (a^2 + b^2: 2, rsq: 2, two products), Hermitian merge 8 (lane twiddle as above 6, sums 2).
  rows_lerp    |y_dev - y_model| <= u (|b - a| t + |y|)          (the difference and the fused multiply-add)
  adjoint      |d_dev - d_model| <= (n + 2) u sum |w g|           (n terms: n fused multiply-adds, 1 - t, w g)

The fractions of these bounds that the MI355X reached are recorded through _tol.within under LK_* labels
(profiles/r22_lossless_kernels_tolerance_report.json).  The overlap-add gather and fix-up and the
exact-input cases of the two row kernels are asked for bit for bit.

Launch geometry the shapes are chosen by: k_analysis runs kAnaWaves = 12 frames per workgroup on at most one workgroup
per CU, k_synth_lossless 8; k_rows_lerp and the adjoint 4 rows per workgroup; k_ola_gather 256 samples, k_ola_fixup 1024
elements per block from fix_lo rounded down to 64."""
import functools

import numpy as np
import pytest
import torch

import lossless_kernels_model as lk
from _tol import note, within
from magphase_amd import hostmath as hm

pytestmark = pytest.mark.gpu

U = lk.U
SENT = -77.25
GUARD = 64
NAN_GUARD = 2112
ANA_WAVES, SYN_WAVES = 12, 8      # kAnaWaves, kWavesPerBlock (mpx_common.hpp)
FFT_LENS = (1024, 2048, 4096)
WIDTHS = (1, 2, 3, 4, 5, 7, 63, 64, 65, 255, 256, 257, 259, 513, 1025, 2049)
COUNTS = (0, 1, 3, 4, 5, 9)


def ana_bound(N):
    return (5 * np.log2(N) + 28) * U


def syn_bound(N):
    return (5 * np.log2(N) + 14) * U


# The derived bounds of the two transforms stand more than 10 x above what the device reaches (they add every rounding in
# the same direction), so both are also pinned against the float64 model: <= 3 x the worst case measured on the MI355X, in
# units of u x the same norm (profiles/r22_lossless_kernels_tolerance_report.json).
#                                                         measured on the MI355X, per fft_len
PIN_ANA = {1024: 20.0, 2048: 13.0, 4096: 13.0}          # 7.28 (9245 short frames), 4.49, 4.49 (13 short frames)
PIN_ANGLE = {1024: 15.0, 2048: 11.0, 4096: 13.0}        # 5.00, 3.82, 4.50 u (radians): every bin of every one-hot row
PIN_SYN = {1024: 16.0, 2048: 16.0, 4096: 18.0}          # 5.39, 5.39, 6.07 (each on a one-hot spectrum)


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


def _dev_rows(e, a, ld):
    """Rows [R x W] float32 uploaded with pitch ld > W, the pad columns NaN, between NaN runs -> (tensor at row 0, ld)."""
    a = np.asarray(a, dtype=np.float32)
    wide = np.full((a.shape[0], ld), np.nan, dtype=np.float32)
    wide[:, :a.shape[1]] = a
    return _dev(e, wide)


class Out:
    """rows x cols float32 written with pitch ld inside a sentinel-filled buffer with guards; fill: the initial content
    (None: the sentinel everywhere)."""

    def __init__(self, e, rows, cols, ld=None, fill=None):
        self.rows, self.cols, self.ld = int(rows), int(cols), int(ld or cols)
        h = np.full(2 * GUARD + self.rows * self.ld, SENT, dtype=np.float32)
        if fill is not None:
            h[GUARD:GUARD + self.rows * self.ld].reshape(self.rows, self.ld)[:, :self.cols] = fill
        self.buf = torch.from_numpy(h).to(e.device)
        self.t = self.buf[GUARD:]

    def check(self, what, written=None):
        """-> the first `written` rows (all by default); guards, pad columns and the other rows must hold the sentinel."""
        torch.cuda.synchronize()
        h = self.buf.cpu().numpy()
        n = self.rows * self.ld
        assert np.all(h[:GUARD] == SENT), what + ": written before the buffer"
        assert np.all(h[GUARD + n:] == SENT), what + ": written past the buffer"
        body = h[GUARD:GUARD + n].reshape(self.rows, self.ld)
        assert np.all(body[:, self.cols:] == SENT), what + ": written beyond a row's last column"
        w = self.rows if written is None else int(written)
        assert np.all(body[w:] == SENT), what + ": rows written that were not asked for"
        return body[:w, :self.cols].copy()


# ================================================================================================== mpx_analysis_frames
def _geometries(N):
    out = []
    for L in sorted({0, 1, 2, 63, 64, 65, N // 4, N // 2 - 1, N // 2, N // 2 + 1, N - 2, N - 1, N, N + 1, N + 200}):
        Rs = {0, 1, 64, N // 2} | {t - L - 1 for t in (N // 2, N // 2 + 1, N - 1, N, N + 1, N + 300)}
        out += [(L, R) for R in sorted(r for r in Rs if r >= 0)]
    return out


ONE_HOT_AT = ("0", "1", "L-1", "L", "L+1", "len-1")


def _frame_signals(L, R, N, rng):
    """[(kind, samples float32 [len])] of one geometry; a one-hot's kind names its sample, "onehot:L+1" (a sample that two
    of the names of ONE_HOT_AT mean is taken once, under the first)."""
    n = lk.frame_len(L, R, N)
    sigs = [("noise", rng.uniform(-0.6, 0.6, n))]
    seen = set()
    for name, k in zip(ONE_HOT_AT, (0, 1, L - 1, L, L + 1, n - 1)):
        if 0 <= k < n and k not in seen:
            seen.add(k)
            x = np.zeros(n)
            x[k] = 0.75
            sigs.append(("onehot:" + name, x))
    sigs += [("dc", np.full(n, 0.5)), ("alt", np.where(np.arange(n) % 2, -1.0, 1.0)), ("zero", np.zeros(n))]
    return [(kind, x.astype(np.float32)) for kind, x in sigs]


def _launch_analysis(e, N, sig, pos, left, right, ld):
    H, F = N // 2 + 1, len(pos)
    outs = [Out(e, F, H, ld) for _ in range(3)]
    e.launch("mpx_analysis_frames", N, e.tables(N), _dev(e, sig, np.float32), _dev(e, pos, np.int64), _dev(e, left, np.int32),
             _dev(e, right, np.int32), F, outs[0].t, outs[1].t, outs[2].t, ld)
    return [o.check("analysis " + s) for o, s in zip(outs, ("mag", "real", "imag"))]


def _model_rows(sig, pos, left, right, N):
    sig64 = np.asarray(sig, dtype=np.float64)
    rows = [lk.analysis_frame(sig64, p, L, R, N) for p, L, R in zip(pos, left, right)]
    return [np.array([r[i] for r in rows]) for i in range(4)]


@functools.lru_cache(maxsize=None)
def _analysis_case(N):
    """Every geometry x every signal of fft_len N in ONE launch: each frame has a segment of its own in the signal, the
    segments NaN apart.  -> dict of the tables, the device's rows (pitched) and the model's."""
    e, rng = _engine(), np.random.default_rng(N)
    segs, pos, left, right, kinds = [np.full(7, np.nan, np.float32)], [], [], [], []
    at = 7
    for L, R in _geometries(N):
        for kind, x in _frame_signals(L, R, N, rng):
            pos.append(at + L), left.append(L), right.append(R), kinds.append(kind)
            segs += [x, np.full(5, np.nan, np.float32)]
            at += x.size + 5
    sig = np.concatenate(segs)
    pos, left, right = np.array(pos, np.int64), np.array(left, np.int32), np.array(right, np.int32)
    ld = N // 2 + 1 + 3
    dev = _launch_analysis(e, N, sig, pos, left, right, ld)
    return dict(sig=sig, pos=pos, left=left, right=right, kinds=np.array(kinds), ld=ld, dev=dev,
                model=_model_rows(sig, pos, left, right, N))


def _analysis_figures(dev, model, N, rows=None):
    """Every bin of the frames `rows` (all by default) against the model -> dict of the figures, nothing asserted but that
    no output is NaN."""
    rows = slice(None) if rows is None else rows
    mag, real, imag = [np.asarray(x, dtype=np.float64)[rows] for x in dev]
    r_mag, r_real, r_imag, l1 = [x[rows] for x in model]
    assert not np.isnan(mag).any() and not np.isnan(real).any() and not np.isnan(imag).any(), "a read outside a frame"
    X, Xr = mag * (real + 1j * imag), r_mag * (r_real + 1j * r_imag)
    live = l1 > 0
    scale = np.where(live, l1, 1.0)[:, None]
    fig = dict(x=0.0, mag=0.0, real=0.0, imag=0.0, dead=0.0, n=len(l1), excluded=0.0)
    if np.any(live):
        fig["x"] = float(np.max((np.abs(X - Xr) / scale)[live]))
        fig["mag"] = float(np.max((np.abs(mag - r_mag) / scale)[live]))
        peak = np.max(r_mag, axis=1, keepdims=True)
        big = (r_mag > 1e-5 * peak) & live[:, None]
        allow = (ana_bound(N) * scale / np.maximum(r_mag, 1e-300))[big]
        fig["real"] = float(np.max((np.abs(real - r_real)[big] - 2e-7) / allow))
        fig["imag"] = float(np.max((np.abs(imag - r_imag)[big] - 2e-7) / allow))
        fig["excluded"] = float(1.0 - big[live].sum() / big[live].size)
    if np.any(~live):       # the model is exactly zero (zero samples, or one sample under a window weight of 0)
        fig["dead"] = float(max(np.abs(x[~live]).max() for x in (mag, real, imag)))
    fig["norm"] = float(np.max(np.abs(real ** 2 + imag ** 2 - 1.0)[mag > 0])) if np.any(mag > 0) else 0.0
    return fig


def _hold_analysis(dev, model, N, tag, rows=None, pin=None):
    """Prints the figures, then holds them to the derived bound (and |dX| to `pin`, in u, where one is given)."""
    fig = _analysis_figures(dev, model, N, rows)
    print("%s N=%d (%d frames): |dX| %.2f u |wx|_1, |dmag| %.2f u, bound %.0f u; real %.3f imag %.3f of the amplified "
          "bound; |phasor|^2 - 1 %.2e; frames with a zero model: max |out| %.3g"
          % (tag, N, fig["n"], fig["x"] / U, fig["mag"] / U, ana_bound(N) / U, fig["real"], fig["imag"], fig["norm"],
             fig["dead"]))
    note("LK_ANA_REAL_IMAG_EXCLUDED_%s_%d" % (tag, N), fig["excluded"])
    assert fig["dead"] == 0.0, "a frame whose model is exactly zero must give exact zeros"
    within(fig["x"] / ana_bound(N), 1.0, "LK_ANA_X_FRACTION_OF_BOUND_%d" % N)
    within(fig["mag"] / ana_bound(N), 1.0, "LK_ANA_MAG_FRACTION_OF_BOUND_%d" % N)
    within(fig["real"], 1.0, "LK_ANA_REAL_FRACTION_OF_AMPLIFIED_BOUND_%d" % N)
    within(fig["imag"], 1.0, "LK_ANA_IMAG_FRACTION_OF_AMPLIFIED_BOUND_%d" % N)
    within(fig["norm"], 1e-5, "LK_ANA_UNIT_PHASOR")
    if pin is not None:
        within(fig["x"] / U, pin, "LK_ANA_X_PINNED_U_%d" % N)


@pytest.mark.parametrize("N", FFT_LENS)
@pytest.mark.parametrize("kind", ("noise", "dc", "alt", "zero"))
def test_analysis_every_geometry_within_the_derived_bound(N, kind):
    c = _analysis_case(N)
    rows = c["kinds"] == kind
    assert rows.sum() == len(_geometries(N)) > 100
    _hold_analysis(c["dev"], c["model"], N, kind, rows, PIN_ANA[N])
    if kind == "zero":
        for x in c["dev"]:
            assert not x[rows].any()


@pytest.mark.parametrize("N", FFT_LENS)
def test_analysis_one_hot_rows_within_the_derived_bound(N):
    """One sample of 0.75 at frame offset 0, 1, L - 1, L, L + 1, len - 1 of every geometry: the model's row has |w x| in
    every bin, so every bin is held to (5 log2 N + 28) u |w x|.

    This test found that the Hann weight was accurate to 2 u of FULL SCALE, not of the weight: sin2_halfpi (mpx_common.hpp)
    evaluated sin^2(pi t / 2) as 0.5 + 0.5 sin(pi (t - 0.5)) at every t.  On the MI355X a sample at offset 1 of a frame with
    L = N + 200 (weight 1.65e-6 / 4.4e-7 / 1.1e-7) came out 2.7 % / 5.4 % / 48 % off -- 459 314 / 913 823 / 8 037 650 u |w x|
    at fft_len 1024 / 2048 / 4096 -- and a sample under a weight of exactly 0 (offset 0 with L > 0, len - 1 with R > 0,
    L + 1 with R == 1) gave |X| = 2.2e-8 in every bin with unit phasors where the model's row is zero; a float32 emulation
    of the polynomial on the CPU gave the same figures to the last digit.  sin2_halfpi now takes sin(pi t / 2)^2 from the
    same polynomial below t = 0.375, and every offset is within the bound."""
    c = _analysis_case(N)
    figs = {}
    for name in ONE_HOT_AT:
        rows = c["kinds"] == "onehot:" + name
        assert rows.sum() > 50
        figs[name] = f = _analysis_figures(c["dev"], c["model"], N, rows)
        print("one-hot at %-5s N=%d (%d frames): |dX| %.2f u |wx|_1, |dmag| %.2f u, bound %.0f u; frames with a zero model: "
              "max |out| %.3g" % (name, N, f["n"], f["x"] / U, f["mag"] / U, ana_bound(N) / U, f["dead"]))
    for name in ("L-1", "L") + tuple(n for n in ONE_HOT_AT if n not in ("L-1", "L")):
        f = figs[name]
        within(f["x"] / ana_bound(N), 1.0, "LK_ANA_ONE_HOT_X_FRACTION_OF_BOUND_%d" % N)
        within(f["mag"] / ana_bound(N), 1.0, "LK_ANA_ONE_HOT_X_FRACTION_OF_BOUND_%d" % N)
        assert f["dead"] == 0.0, "one sample under a window weight of exactly 0 must give exact zeros"


@pytest.mark.parametrize("N", FFT_LENS)
def test_analysis_one_hot_rows_have_the_models_angle_in_every_bin(N):
    """One sample: the model's row has the magnitude |w x| in every bin and a linear phase.  |X_model| sin(angle between
    the device's and the model's bin) <= |X_dev - X_model|, so the derived bound holds the angle of EVERY bin of every
    one-hot row whose model is not zero."""
    c = _analysis_case(N)
    mag, real, imag = [np.asarray(x, dtype=np.float64) for x in c["dev"]]
    r_mag, r_real, r_imag, l1 = c["model"]
    rows = np.array([k.startswith("onehot") for k in c["kinds"]]) & (l1 > 0)
    assert rows.sum() > 300
    within(np.max(np.abs(r_mag[rows] / l1[rows, None] - 1.0)), 1e-12, "LK_ANA_ONE_HOT_MODEL_IS_FLAT")
    d = (real[rows] + 1j * imag[rows]) * np.conj(r_real[rows] + 1j * r_imag[rows])
    ang = np.abs(np.angle(d))
    print("one-hot N=%d: largest angle error %.2f u of a bound of %.0f u" % (N, ang.max() / U, ana_bound(N) / U))
    within(np.max(np.sin(ang)) / ana_bound(N), 1.0, "LK_ANA_ONE_HOT_ANGLE_FRACTION_OF_BOUND_%d" % N)
    if PIN_ANGLE[N] is not None:
        within(ang.max() / U, PIN_ANGLE[N], "LK_ANA_ONE_HOT_ANGLE_PINNED_U_%d" % N)


@pytest.mark.parametrize("N", FFT_LENS)
def test_analysis_repeated_and_dense_launches_are_bit_identical(N):
    c, e = _analysis_case(N), _engine()
    again = _launch_analysis(e, N, c["sig"], c["pos"], c["left"], c["right"], c["ld"])
    dense = _launch_analysis(e, N, c["sig"], c["pos"], c["left"], c["right"], N // 2 + 1)
    for a, b, d in zip(c["dev"], again, dense):
        assert _same_bits(a, b) and _same_bits(a, d)


def _count_case(N, F, seed):
    """F short frames (L, R <= 40; every 7th L == 0, every 11th R == 0) at random places of one signal, overlapping freely;
    samples no frame covers are NaN."""
    rng = np.random.default_rng(seed)
    left = rng.integers(1, 41, F).astype(np.int32)
    right = rng.integers(1, 41, F).astype(np.int32)
    left[::7], right[::11] = 0, 0
    n = 4096
    pos = rng.integers(50, n - 50, F).astype(np.int64)
    sig = rng.uniform(-0.6, 0.6, n).astype(np.float32)
    cover = np.zeros(n, dtype=bool)
    for p, L, R in zip(pos, left, right):
        cover[p - L:p + R + 1] = True
    sig[~cover] = np.nan
    return sig, pos, left, right


@pytest.mark.parametrize("F", (1, ANA_WAVES - 1, ANA_WAVES, ANA_WAVES + 1, "three_per_wave"))
def test_analysis_frame_counts(F):
    """1, kAnaWaves - 1, kAnaWaves, kAnaWaves + 1 frames at every fft_len; more than 3 x CUs x kAnaWaves frames (every wave
    takes at least three frames through the prefetch pipeline) at 1024."""
    e = _engine()
    for N in (FFT_LENS if F != "three_per_wave" else (1024,)):
        n = 3 * _cus() * ANA_WAVES + 29 if F == "three_per_wave" else F
        sig, pos, left, right = _count_case(N, n, 1000 + n)
        dev = _launch_analysis(e, N, sig, pos, left, right, N // 2 + 1 + 3)
        _hold_analysis(dev, _model_rows(sig, pos, left, right, N), N, "count_%s" % F, None, PIN_ANA[N])


# ======================================================================================== mpx_synthesis_lossless_frames
def ONE_HOT_BINS(N):
    return (0, 1, 63, 64, N // 2 - 1, N // 2)


def _synthesis_rows(N, F, seed):
    """mag = exp(0.5 randn), unnormalised (real, imag) -- non-zero imag at bins 0 and N/2 included; from row 1 on: a row with
    bins whose real == imag == 0, a row with mag == 0, six one-hot spectra; the rest random."""
    rng, H = np.random.default_rng(seed), N // 2 + 1
    mag = np.exp(0.5 * rng.normal(size=(F, H)))
    real, imag = rng.normal(size=(F, H)), rng.normal(size=(F, H))
    kinds = ["random"] * F
    if F > 1:
        real[1, [0, 5, 64, H - 1]] = imag[1, [0, 5, 64, H - 1]] = 0.0
        real[1, 70], imag[1, 71] = 0.0, 0.0
    if F > 2:
        mag[2], kinds[2] = 0.0, "zero"
    for i, k in enumerate(ONE_HOT_BINS(N)):
        if F > 3 + i:
            keep = mag[3 + i, k]
            mag[3 + i] = 0.0
            mag[3 + i, k], kinds[3 + i] = keep, "onehot"
    return [x.astype(np.float32) for x in (mag, real, imag)], np.array(kinds)


def _launch_synthesis(e, N, feats, ld):
    F = feats[0].shape[0]
    out = Out(e, F, N)
    e.launch("mpx_synthesis_lossless_frames", N, e.tables(N), _dev_rows(e, feats[0], ld), _dev_rows(e, feats[1], ld),
             _dev_rows(e, feats[2], ld), F, out.t, ld)
    return out.check("synthesis frames")


def _hold_synthesis(y, feats, kinds, N, tag):
    assert not np.isnan(y).any(), "a read outside a row"
    ref = lk.synthesis_frame(feats[0], feats[1], feats[2], N)
    term = lk.synthesis_bound_term(feats[0], N)
    live = term > 0
    err = np.max(np.abs(y.astype(np.float64) - ref), axis=1)
    frac = (err[live] / term[live]).max() if live.any() else 0.0
    oh = kinds == "onehot"
    print("%s N=%d F=%d: %.2f u sum c|mag|/N (one-hot rows %.2f u), bound %.0f u"
          % (tag, N, len(y), frac / U, (err[oh] / term[oh]).max() / U if oh.any() else 0.0, syn_bound(N) / U))
    assert not y[~live].any(), "mag == 0 rows must give exact zeros"
    within(frac / syn_bound(N), 1.0, "LK_SYN_FRACTION_OF_BOUND_%d" % N)
    if PIN_SYN[N] is not None:
        within(frac / U, PIN_SYN[N], "LK_SYN_PINNED_U_%d" % N)


@pytest.mark.parametrize("N", FFT_LENS)
@pytest.mark.parametrize("F", (1, SYN_WAVES - 1, SYN_WAVES, SYN_WAVES + 1, 24))
def test_synthesis_frames_within_the_derived_bound_pitched_equals_dense(N, F):
    e = _engine()
    feats, kinds = _synthesis_rows(N, F, 10 * N + F)
    y = _launch_synthesis(e, N, feats, N // 2 + 1 + 3)
    _hold_synthesis(y, feats, kinds, N, "synthesis")
    assert _same_bits(y, _launch_synthesis(e, N, feats, N // 2 + 1))
    assert F < 24 or (kinds == "onehot").sum() == 6


def test_synthesis_more_than_two_frames_per_wave():
    e, N = _engine(), 1024
    F = 2 * _cus() * SYN_WAVES + 13
    feats, kinds = _synthesis_rows(N, F, 77)
    _hold_synthesis(_launch_synthesis(e, N, feats, N // 2 + 1 + 3), feats, kinds, N, "two_per_wave")


# ======================================================================================================= mpx_ola_gather
def _gather_batch(N, rng):
    """(pm_rel per utterance, out_start, out_len)."""
    steps = np.array([0, 1, 1, N - 1, N, N + 1, 3 * N, 40])
    utts = [
        (np.cumsum(np.r_[0, rng.integers(50, 300, 11)]), 100, 1500),
        (np.zeros(0, np.int64), 0, 0),                               # no frame, no sample
        (np.zeros(1, np.int64), -7, 257),                            # one frame, a negative out_start
        (np.zeros(0, np.int64), 3, 5),                               # no frame: five zeros
        (np.array([0, 0, 5, 5, 5, 9, 10, 11]), 2, 256),              # coincident epochs, steps of 1
        (np.cumsum(steps), N // 2 + 188, int(np.sum(steps)) + N - (N // 2 + 188) + 10),   # gaps; out_start > N/2
        (np.array([0, 30]), 17, 1),
        (np.array([0, 30, 60]), 0, 255),
        (np.cumsum(np.r_[0, rng.integers(1, 90, 60)]), 511, 9 * 256 + 3),
    ]
    return utts


@pytest.mark.parametrize("N", (1024, 4096))
def test_ola_gather_is_the_sequential_float32_sum_bit_for_bit(N):
    e, rng = _engine(), np.random.default_rng(N + 1)
    utts = _gather_batch(N, rng) if N == 1024 else [(np.array([0, 100, 100, N + 100]), -3, 2 * N + 400),
                                                    (np.zeros(0, np.int64), 0, 0), (np.array([0, 5 * N]), N // 2 + 1, 257)]
    frame_off = np.concatenate(([0], np.cumsum([len(u[0]) for u in utts]))).astype(np.int32)
    pm_rel = np.concatenate([u[0] for u in utts]).astype(np.int32)
    out_start = np.array([u[1] for u in utts], np.int32)
    out_off = np.concatenate(([0], np.cumsum([u[2] for u in utts]))).astype(np.int64)
    max_len = max(u[2] for u in utts)
    assert any(u[2] < max_len - 4 * 256 for u in utts if u[2] > 0)          # shorter than the grid by several blocks
    frames = rng.normal(size=(int(frame_off[-1]), N)).astype(np.float32)
    out = Out(e, 1, int(out_off[-1]))
    e.launch("mpx_ola_gather", N, _dev(e, frames), len(utts), _dev(e, frame_off), _dev(e, pm_rel), _dev(e, out_start),
             _dev(e, out_off), max_len, out.t)
    got = out.check("ola_gather")[0]
    ref = lk.ola_gather(frames, frame_off, pm_rel, out_start, out_off, N)
    assert not np.isnan(got).any() and _same_bits(got, ref)
    assert np.count_nonzero(ref == 0) >= 5 and np.count_nonzero(ref) > 1000


# ========================================================================================= mpx_ola_fixup, mpx_ola_fixup_width
def _fixup_tables(N, rng):
    """Hand-built runs: fix_lo x width, a run with fix_hi == fix_lo after every third; every run has a strip and a stretch
    of pcm of its own; out_base mostly no multiple of 64, the first one negative.  -> (runs, strips, pcm)."""
    strip_floats = N + 64
    rows = []
    for lo in (1000, 0, 1, 63, 64, 65):
        for w in (1, 0, 63, 64, 65, 1023, 1024, 1025, N + 64 - lo):
            if lo + w <= strip_floats:
                rows.append((lo, lo + w))
                if len(rows) % 3 == 0:
                    rows.append((lo + 7, lo + 7))
    runs = np.zeros(len(rows), dtype=lk.OLA_RUN_DTYPE)
    strips = np.full(len(rows) * strip_floats, np.nan, dtype=np.float32)
    at = 0
    for i, (lo, hi) in enumerate(rows):
        base = at - lo + (0 if i == 0 else i % 5)
        runs[i]["fix_lo"], runs[i]["fix_hi"] = lo, hi
        runs[i]["out_base"], runs[i]["strip_off"] = base, i * strip_floats
        runs[i]["frame_begin"], runs[i]["frame_end"], runs[i]["pad"] = -12345, -1, -1      # not the fix-up's business
        strips[i * strip_floats + lo:i * strip_floats + hi] = rng.normal(size=hi - lo)
        at = base + hi + 3
    assert runs[0]["out_base"] == -1000 and runs[0]["fix_hi"] > runs[0]["fix_lo"] and np.any(runs["out_base"] % 64 != 0)
    return runs, strips, rng.normal(size=at + 9).astype(np.float32)


def _launch_fixup(e, N, runs, strips, pcm, max_width=None):
    out = Out(e, 1, pcm.size, fill=pcm)
    sbuf = _dev(e, strips)
    rdev = torch.from_numpy(np.frombuffer(runs.tobytes(), dtype=np.uint8).copy()).to(e.device)
    if max_width is None:
        e.launch("mpx_ola_fixup", N, rdev, len(runs), sbuf, out.t)
    else:
        e.launch("mpx_ola_fixup_width", N, rdev, len(runs), sbuf, out.t, int(max_width))
    got = out.check("ola_fixup")[0]
    assert _same_bits(sbuf.cpu().numpy(), strips) and np.array_equal(rdev.cpu().numpy().tobytes(), runs.tobytes())
    return got


@pytest.mark.parametrize("N", (1024, 4096))
def test_ola_fixup_adds_exactly_the_named_elements(N):
    assert lk.OLA_RUN_DTYPE.itemsize == 56
    e, rng = _engine(), np.random.default_rng(N + 2)
    runs, strips, pcm = _fixup_tables(N, rng)
    ref = lk.ola_fixup(pcm, runs, strips)
    changed = np.flatnonzero(_bits(ref) != _bits(pcm))
    assert not np.isnan(ref).any() and changed.size > 0.98 * sum(int(r["fix_hi"] - r["fix_lo"]) for r in runs)
    got = _launch_fixup(e, N, runs, strips, pcm)
    assert _same_bits(got, ref)                     # every element outside the ranges keeps its bits, too
    # _width: the table's own width completes everything; 0 launches nothing; a smaller one completes whole 1024-blocks
    width = lk.fixup_width(runs)
    assert width == N + 64 and _same_bits(_launch_fixup(e, N, runs, strips, pcm, width), ref)
    assert _same_bits(_launch_fixup(e, N, runs, strips, pcm, 0), pcm)
    for w in (1, 1024) + ((1025, 3000) if N == 4096 else ()):
        part = lk.ola_fixup(pcm, runs, strips, w)
        assert np.count_nonzero(_bits(part) != _bits(ref)) > 0
        assert _same_bits(_launch_fixup(e, N, runs, strips, pcm, w), part), w


# ======================================================================================================== mpx_rows_lerp
#           row0 row1  t
LERP_TABLE = ((2, 2, 0.5), (3, 4, 0.0), (3, 4, 1.0), (0, 10, 0.5), (7, 5, 2.0 ** -24), (5, 7, 1.0 - 2.0 ** -24),
              (9, 9, 1.0), (0, 10, 0.37), (10, 0, 0.61))
LERP_ROWS = 12                      # rows 1, 6, 8 and 11 are named by no entry: NaN


def _lerp_tables(table):
    row0 = np.array([r[0] for r in table], np.int32)
    row1 = np.array([r[1] for r in table], np.int32)
    return row0, row1, np.array([r[2] for r in table], np.float32)


def _launch_lerp(e, H, src, row0, row1, t, n_out, ld_src, ld_dst):
    outs = [Out(e, len(row0), H, ld_dst) for _ in range(3)]
    e.launch("mpx_rows_lerp", H, _dev_rows(e, src[0], ld_src), _dev_rows(e, src[1], ld_src), _dev_rows(e, src[2], ld_src),
             ld_src, _dev(e, row0), _dev(e, row1), _dev(e, t), n_out, outs[0].t, outs[1].t, outs[2].t, ld_dst)
    return [o.check("rows_lerp", written=n_out) for o in outs]


def _lerp_source(H, rng, table, rows=LERP_ROWS):
    src = rng.normal(size=(3, rows, H)).astype(np.float32)
    named = {r for ent in table for r in ent[:2]}
    src[:, [r for r in range(rows) if r not in named]] = np.nan
    return src


@pytest.mark.parametrize("H", WIDTHS)
def test_rows_lerp_random_rows_within_the_rounding_bound(H):
    e, rng = _engine(), np.random.default_rng(H)
    src = _lerp_source(H, rng, LERP_TABLE)
    row0, row1, t = _lerp_tables(LERP_TABLE)
    ld_src, ld_dst = H + 3 + (H & 1), H + 5 + (H & 1)           # odd, and different: rows are 4-byte aligned only
    assert ld_src % 2 == 1 and ld_dst % 2 == 1
    worst = 0.0
    for n_out in COUNTS:
        got = _launch_lerp(e, H, src, row0, row1, t, n_out, ld_src, ld_dst)
        for s in range(3):
            ref, term = lk.rows_lerp(src[s], row0[:n_out], row1[:n_out], t[:n_out])
            assert got[s].shape == (n_out, H) and not np.isnan(got[s]).any(), "an unnamed source row was read"
            if n_out:
                worst = max(worst, float(np.max(np.abs(got[s] - ref) / (U * term))))
    within(worst, 1.0, "LK_LERP_FRACTION_OF_BOUND")
    # t == 0 and t == 1 name one row: fma(b - a, 0, a) is a; fma(b - a, 1, a) is b up to the rounding of b - a
    got = _launch_lerp(e, H, src, row0, row1, t, 9, ld_src, ld_dst)
    for s in range(3):
        assert _same_bits(got[s][1], src[s][3])


@pytest.mark.parametrize("H", WIDTHS)
def test_rows_lerp_exact_inputs_are_bit_identical(H):
    """Integers below 2^11 times a power of two, t = k / 8: neither the difference nor the fused multiply-add rounds."""
    e, rng = _engine(), np.random.default_rng(H + 1)
    table = tuple((a, b, k / 8.0) for (a, b, _), k in zip(LERP_TABLE, (4, 0, 8, 1, 2, 3, 5, 6, 7)))
    src = (rng.integers(-2047, 2048, size=(3, LERP_ROWS, H)) * 2.0 ** rng.integers(-20, 20, size=(3, 1, 1))).astype(np.float32)
    named = {r for ent in table for r in ent[:2]}
    src[:, [r for r in range(LERP_ROWS) if r not in named]] = np.nan
    row0, row1, t = _lerp_tables(table)
    got = _launch_lerp(e, H, src, row0, row1, t, 9, H + 1, H + 2)
    for s in range(3):
        ref, _ = lk.rows_lerp(src[s], row0, row1, t)
        assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref) and _same_bits(got[s], ref.astype(np.float32))


@pytest.mark.parametrize("H", WIDTHS)
def test_rows_lerp_of_one_row_is_that_row_in_every_column(H):
    """row0 == row1: the header says the result is the row itself -- -0.0, denormals, infinities and NaNs included, in the
    last n_bins mod 4 columns as in the 16-byte groups."""
    e, rng = _engine(), np.random.default_rng(H + 2)
    special = np.array([-0.0, 0.0, 1e-45, -1e-40, 1.1754942e-38, np.inf, -np.inf, np.nan, 3.4028235e38, -1.5], np.float32)
    src = rng.normal(size=(3, 4, H)).astype(np.float32)
    for s in range(3):
        for r in range(4):
            src[s, r] = np.where(rng.random(H) < 0.7, special[(np.arange(H) + s + 3 * r) % special.size], src[s, r])
    row0 = np.array([0, 3, 1, 2, 2], np.int32)
    t = np.array([0.0, 1.0, 0.5, 2.0 ** -24, 0.3], np.float32)
    got = _launch_lerp(e, H, src, row0, row0.copy(), t, 5, H + 1, H + 3)
    bad = [(s, c, int(np.flatnonzero(_bits(got[s][c]) != _bits(src[s][row0[c]]))[0])) for s in range(3) for c in range(5)
           if not _same_bits(got[s][c], src[s][row0[c]])]
    assert not bad, "(stream, entry, first differing column): %r" % (bad[:6],)


# ================================================================================================ mpx_rows_lerp_adjoint
def _hand_ranges():
    """a only; b only; a and b meeting in one frame; a and b apart; neither; 300 frames into one row (with four more);
    an empty range given as a1 < a0; both ranges the same frames; neither.  Frames 11 .. 13 are named by no range."""
    r = np.array([[0, 3, 0, 0], [0, 0, 3, 5], [5, 8, 7, 9], [9, 11, 14, 16], [16, 16, 16, 16], [20, 320, 16, 20],
                  [7, 3, 320, 322], [322, 325, 322, 325], [0, 0, 0, 0]], dtype=np.int32)
    return r, 325


def _launch_adjoint(e, H, g, ranges, t, n_rows, ld_src, ld_dst, streams=(True, True, True), null_src=False):
    outs = [Out(e, len(ranges), H, ld_dst) for _ in range(3)]
    srcs = [None if (null_src and not on) else _dev_rows(e, g[s], ld_src) for s, on in enumerate(streams)]
    dsts = [o.t if on else None for o, on in zip(outs, streams)]
    e.launch("mpx_rows_lerp_adjoint", H, srcs[0], srcs[1], srcs[2], ld_src, _dev(e, ranges.reshape(-1)), _dev(e, t), n_rows,
             dsts[0], dsts[1], dsts[2], ld_dst)
    return [o.check("rows_lerp_adjoint", written=n_rows if on else 0) for o, on in zip(outs, streams)]


def _adjoint_source(H, n_frames, ranges, rng, exact=False):
    if exact:
        g = (rng.integers(-2047, 2048, size=(3, n_frames, H)) * 2.0 ** rng.integers(-20, 20, size=(3, 1, 1))).astype(np.float32)
    else:
        g = rng.normal(size=(3, n_frames, H)).astype(np.float32)
    named = np.zeros(n_frames, dtype=bool)
    for a0, a1, b0, b1 in ranges:
        named[a0:max(a1, a0)] = True
        named[b0:max(b1, b0)] = True
    g[:, ~named] = np.nan
    return g


@pytest.mark.parametrize("H", WIDTHS)
def test_rows_lerp_adjoint_hand_built_ranges(H):
    e, rng = _engine(), np.random.default_rng(H + 3)
    ranges, nf = _hand_ranges()
    ld_src, ld_dst = H + 3 + (H & 1), H + 5 + (H & 1)
    # exact inputs: integers times a power of two, t = k / 8 -- no sum rounds
    g = _adjoint_source(H, nf, ranges, rng, exact=True)
    t = (rng.integers(0, 9, nf) / 8.0).astype(np.float32)
    got = _launch_adjoint(e, H, g, ranges, t, len(ranges), ld_src, ld_dst)
    for s in range(3):
        ref, _, _ = lk.rows_lerp_adjoint(np.nan_to_num(g[s]), ranges, t, len(ranges))
        assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref) and _same_bits(got[s], ref.astype(np.float32))
        assert not got[s][4].any() and not got[s][8].any()        # a row no frame feeds: zeros over n_bins columns
    # random inputs, every row count
    g = _adjoint_source(H, nf, ranges, rng)
    t = rng.random(nf).astype(np.float32)
    worst = 0.0
    for n_rows in COUNTS:
        got = _launch_adjoint(e, H, g, ranges, t, n_rows, ld_src, ld_dst)
        for s in range(3):
            ref, mag, count = lk.rows_lerp_adjoint(np.nan_to_num(g[s]), ranges, t, n_rows)
            assert got[s].shape == (n_rows, H) and not np.isnan(got[s]).any(), "a frame outside the ranges was read"
            err = np.abs(got[s] - ref)
            assert not err[mag == 0].any()
            if np.any(mag > 0):
                worst = max(worst, float(np.max((err / ((count[:, None] + 2) * U * np.where(mag > 0, mag, 1.0)))[mag > 0])))
    within(worst, 1.0, "LK_ADJOINT_FRACTION_OF_BOUND")


@pytest.mark.parametrize("H", (5, 257))
def test_rows_lerp_adjoint_every_combination_of_null_streams(H):
    e, rng = _engine(), np.random.default_rng(H + 4)
    ranges, nf = _hand_ranges()
    g = _adjoint_source(H, nf, ranges, rng)
    t = rng.random(nf).astype(np.float32)
    full = _launch_adjoint(e, H, g, ranges, t, len(ranges), H + 1, H + 2)
    for mask in range(8):
        streams = tuple(bool(mask >> s & 1) for s in range(3))
        for null_src in (False, True):
            got = _launch_adjoint(e, H, g, ranges, t, len(ranges), H + 1, H + 2, streams, null_src)
            for s in range(3):      # a stream that was asked for does not depend on the others; the others are not written
                assert (_same_bits(got[s], full[s]) if streams[s] else got[s].shape == (0, H)), (mask, s)


@pytest.mark.parametrize("H", WIDTHS)
def test_rows_lerp_and_its_adjoint_are_transposes_on_the_device(H):
    """<rows_lerp(x), g> against <x, rows_lerp_adjoint(g)>, both in float64 from the device's outputs, on the tables of a
    2 x time-stretch (hostmath.const_to_variable_rows -> hostmath.lerp_adjoint_table); bounded by the two kernels' bounds
    summed over the elements."""
    e, rng = _engine(), np.random.default_rng(H + 5)
    fs, rate, n_rows = 16000, 5.0, 9
    step = fs * rate / 1000
    locs = np.linspace(step, n_rows * step, 2 * n_rows + 1)
    lo, hi, t64, _ = hm.const_to_variable_rows(np.ones(n_rows, dtype=bool), locs, rate, fs)
    row0, row1, t = lo.astype(np.int32), hi.astype(np.int32), t64.astype(np.float32)
    ranges = hm.lerp_adjoint_table(row0, row1, t, n_rows)
    x = rng.normal(size=(3, n_rows, H)).astype(np.float32)
    g = rng.normal(size=(3, len(row0), H)).astype(np.float32)
    y = _launch_lerp(e, H, x, row0, row1, t, len(row0), H + 1, H + 2)
    back = _launch_adjoint(e, H, g, ranges, t, n_rows, H + 2, H + 1)
    worst = 0.0
    for s in range(3):
        ref, term = lk.rows_lerp(x[s], row0, row1, t)
        within(float(np.max(np.abs(y[s] - ref) / (U * term))), 1.0, "LK_LERP_FRACTION_OF_BOUND")
        bref, mag, count = lk.rows_lerp_adjoint(g[s], ranges, t, n_rows)
        within(float(np.max(np.abs(back[s] - bref) / ((count[:, None] + 2) * U * mag))), 1.0, "LK_ADJOINT_FRACTION_OF_BOUND")
        lhs = np.sum(y[s].astype(np.float64) * g[s])
        rhs = np.sum(x[s].astype(np.float64) * back[s])
        allow = np.sum(U * term * np.abs(g[s])) + np.sum((count[:, None] + 2) * U * mag * np.abs(x[s]))
        worst = max(worst, abs(lhs - rhs) / allow)
    within(worst, 1.0, "LK_DUALITY_FRACTION_OF_SUMMED_BOUNDS")
