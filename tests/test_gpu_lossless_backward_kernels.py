"""GPU: the three backward entries of magphase_grad.hip, each launched through Engine.launch on tables built by hand,
against tests/lossless_backward_kernels_model.py (held to torch float64 autograd by
tests/test_lossless_backward_kernels_host.py):

  A  mpx_synthesis_lossless_backward             k_synth_lossless_bwd<P, LERP>, six instances
  B  mpx_analysis_lossless_backward              k_analysis_lossless_bwd<P>, k_analysis_bwd_gather
  C  mpx_analysis_lossless_const_rate_backward   k_analysis_lossless_bwd<P, true>, k_analysis_bwd_gather

Every output is a view into a buffer filled with a sentinel, with guard rows before and after and a row pitch wider than the
row (ld_grad != ld): whatever the entry is not documented to write must still hold the sentinel.  Every floating-point
operand lies between runs of NaN; grad_out is NaN at every sample that no frame's [lo, hi) names, feature and gradient rows
that no table entry names are NaN: one NaN in an output is a read outside the extent.  No frame, bin or sample is left out
of a comparison.

The buffers whose clamps are tested with tables no planner builds (grad_out, scratch, grad_sig, the constant-rate gradient
rows) are views into larger allocations of the test's own with at least fft_len floats (rows: two full rows) of NaN or
sentinel on both sides, and the lying tables reach no further than that: a clamp that did not hold would show as a NaN or
a disturbed sentinel.

Launch geometry the frame counts are chosen by: one workgroup per CU at most, 12 waves (frames) per workgroup for
k_synth_lossless_bwd and for k_analysis_lossless_bwd at fft_len 1024 / 2048, 8 at 4096.  A wave takes a second frame only
from frame waves x CUs on: the second-trip cases have waves x CUs + waves + 1 frames, so that every wave of workgroup 0 and
one wave of workgroup 1 make the second trip (frame f and frame f + waves x CUs belong to one wave).  In part A the early
frame has a full window of samples of size 1e3 and the late one a narrow (or empty) window of samples of size 1: what the
late frame's mask lets through of the LDS words the copy skipped is about 1e3 times the bound.

Derived bounds, u = 2^-24, one rounding <= 1 u of its result, L2N = log2(fft_len), c_k = 2 (1 at bins 0 and N/2):

  A  |gX_dev - gX_model| <= E = (5 L2N + 11) u (c_k / N) ||window||_1 per bin.  Per butterfly level 5 (table twiddle 1,
     complex product 3, sum 1; tests/test_gpu_lossless_kernels.py counts the forward transform the same way); constant part
     11: split twiddle 6 (sincospif 2, constant 1, complex product 3), E / T sums 2, T product 3.  The halvings and the
     scale c_k / N are powers of two.  gX is not an output; with u = p / |p| carrying 4 u (a^2 + b^2: 2, halved by the
     root; rsq 2; the product 1):
       grad_mag  = Re(conj(u) gX):        |error| <= E + 6 u |gX|   (u: 4, the two products and their sum: 2 |gX| by Cauchy)
       grad_real, grad_imag = (mag / den)(gX - u d): gX -> gX - u Re(conj(u) gX) is a projection, so E passes through
                 once;                     |error| <= (mag / den)(E + 17 u |gX|)   (u twice: 8, d's products and sum 2,
                 u d 1, the difference 1, mag r and the last product 5)
     With row tables mag, den and u are those of the float32 row fma(x1 - x0, t, x0), which the model emulates exactly.
     Where the bound is 0 (an empty window; mag == 0 for grad_real / grad_imag) the output must be == 0; where p == 0
     grad_mag must be == 0.
  B  per scratch sample k of frame f: <= w(k) ((5 L2N + 19) u sum_k c_k |Y_k| + PW_f): Hermitian merge 8 (lane twiddle 6,
     sums 2), window weight 10 and weight x sample 1 (both as in tests/test_gpu_lossless_kernels.py); PW_f is the rounding
     of the pointwise step gX carried to a sample, term by term in lossless_backward_kernels_model.analysis_bound_terms
     (rcp: 2 u).  Where that is 0 (dead bins only, a weight of exactly 0) the sample must be == 0.
  C  as B, with the (n + 2) u sum |w g| of the row sums (tests/test_gpu_lossless_kernels.py, adjoint) passed through the
     pointwise step into PW_f.

The fractions of these bounds that the MI355X reached are recorded through _tol.within under LBK_* labels
(profiles/r32_lossless_backward_kernels_tolerance_report.json) and pinned below at <= 3 x the
worst value measured against the float64 model.  grad_sig is asked for bit for bit: it is the float32 sum, in ascending
frame order, of the device's own scratch; so are scratch and grad_sig of part C against mpx_rows_lerp_adjoint followed by
mpx_analysis_lossless_backward."""
import functools
import itertools

import numpy as np
import pytest
import torch

import lossless_backward_kernels_model as bk
from _tol import note, within
from lossless_analysis_autograd_model import window

pytestmark = pytest.mark.gpu

U = bk.U
SENT = -77.25
GUARD_ROWS = 2
NAN_GUARD = 2112
FFT_LENS = (1024, 2048, 4096)
SYN_WAVES = 12                                  # kAnaWaves (mpx_common.hpp)
C_A, C_MAG, C_RI, C_B = 11, 6, 17, 19

# Fractions of the derived bounds, pinned at <= 3 x the worst value measured on the MI355X against the float64 model
#                                                  measured, per fft_len
PIN_SYN = {1024: 0.27, 2048: 0.29, 4096: 0.28}             # 0.0915 (13 frames), 0.0970 (a one-hot window), 0.0965 (13 frames)
PIN_ANA = {1024: 0.31, 2048: 0.31, 4096: 0.30}             # 0.1036, 0.1046, 0.1015 (each on a one-hot gradient)
PIN_CR = {1024: 0.018, 2048: 0.0105, 4096: 0.0086}         # 0.00613, 0.00353, 0.00287 (each at the second-trip count)


def ana_waves(N):
    return 8 if N == 4096 else 12               # ana_bwd_waves<P>() (magphase_grad.hip)


def _engine():
    from magphase_amd.engine import get_engine
    return get_engine()


def _cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _dev(e, a, dtype=None, guard=NAN_GUARD):
    """Upload.  A floating-point operand lies between two runs of `guard` NaNs."""
    a = np.ascontiguousarray(a, dtype=dtype)
    if not np.issubdtype(a.dtype, np.floating):
        return torch.from_numpy(a.reshape(-1) if a.size else np.zeros(1, a.dtype)).to(e.device)
    buf = np.full(a.size + 2 * guard, np.nan, dtype=a.dtype)
    buf[guard:guard + a.size] = a.ravel()
    return torch.from_numpy(buf).to(e.device)[guard:guard + a.size]


def _dev_rows(e, a, ld, guard=NAN_GUARD):
    """Rows [R x W] float32 uploaded with pitch ld > W, the pad columns NaN, between NaN runs."""
    a = np.asarray(a, dtype=np.float32)
    wide = np.full((a.shape[0], ld), np.nan, dtype=np.float32)
    wide[:, :a.shape[1]] = a
    return _dev(e, wide, guard=guard)


class Rows:
    """rows x cols float32 written with pitch ld inside a sentinel-filled buffer, GUARD_ROWS rows before and after."""

    def __init__(self, e, rows, cols, ld):
        self.rows, self.cols, self.ld = int(rows), int(cols), int(ld)
        self.g = GUARD_ROWS * self.ld
        self.buf = torch.full((2 * self.g + self.rows * self.ld,), SENT, dtype=torch.float32, device=e.device)
        self.t = self.buf[self.g:]

    def check(self, what, written=None):
        """-> the first `written` rows (all by default); guards, pad columns and the other rows must hold the sentinel."""
        torch.cuda.synchronize()
        h = self.buf.cpu().numpy()
        n = self.rows * self.ld
        assert np.all(h[:self.g] == SENT), what + ": written before the buffer"
        assert np.all(h[self.g + n:] == SENT), what + ": written past the buffer"
        body = h[self.g:self.g + n].reshape(self.rows, self.ld)
        assert np.all(body[:, self.cols:] == SENT), what + ": written beyond a row's last column"
        w = self.rows if written is None else int(written)
        assert np.all(body[w:] == SENT), what + ": rows written that were not asked for"
        return body[:w, :self.cols].copy()


class Flat:
    """n float32 inside a sentinel-filled buffer, `margin` floats before and after (the allocation the clamps are tested in)."""

    def __init__(self, e, n, margin):
        self.n, self.m = int(n), int(margin)
        self.buf = torch.full((2 * self.m + self.n,), SENT, dtype=torch.float32, device=e.device)
        self.t = self.buf[self.m:]

    def check(self, what):
        torch.cuda.synchronize()
        h = self.buf.cpu().numpy()
        assert np.all(h[:self.m] == SENT), what + ": written before the buffer"
        assert np.all(h[self.m + self.n:] == SENT), what + ": written past the buffer"
        return h[self.m:self.m + self.n].copy()


def _second_trip(waves):
    return waves * _cus() + waves + 1


# ===================================================================================== A  mpx_synthesis_lossless_backward
def _narrow_windows(N):
    """(lo, hi): tile 1 only; tile 0 only; inside one 64-sample row; no multiples of 64, across the tiles; empty at 0, at N
    and at an interior odd value."""
    M = N // 2
    return [(M + 70, M + 270), (100, 300), (197, 232), (M - 37, M + 91), (0, 0), (N, N), (333, 333)]


def _geometry(N, total, rng):
    """25 frames (pos, lo, hi) in a buffer of `total` samples: see the comments."""
    M = N // 2
    g = [(N // 3, 0, N),                                   # a full window
         (-M - 3, 0, N), (total - M + 5, 0, N),            # pos < 0 / pos + N > total: clamped at the buffer's ends
         (700, -7, N + 9), (800, 300, 200), (900, -50, 40),   # lying tables: lo < 0, hi > N, hi < lo
         (-N + 1, 0, N), (total - 1, 0, N),                # one sample inside the buffer
         (-N, 0, N), (total, 0, N), (total + 3, -3, N + 4),   # wholly outside: empty
         (-5, 3, N - 3), (total - N + 5, 2, N)]
    g += [(1000 + 101 * i, lo, hi) for i, (lo, hi) in enumerate(_narrow_windows(N))]
    while len(g) < 25:
        lo = int(rng.integers(0, N - 1))
        g.append((int(rng.integers(0, total - N)), lo, int(rng.integers(lo + 1, N + 1))))
    return g


def _named_samples(gy_len, pos, lo, hi, N):
    named = np.zeros(gy_len, dtype=bool)
    for p, a, b in zip(pos, lo, hi):
        a, b = bk.clamp_window(p, a, b, N, gy_len)
        named[p + a:p + b] = True
    return named


def _syn_tables(N, F, rng):
    """-> (gy float32 [total] NaN where no frame names the sample, pos, lo, hi).  F == "second_trip": 12 x CUs frames with
    full windows over samples of size 1e3, 97 apart, then 13 frames with the narrow windows over samples of size 1, each in
    a stretch of its own."""
    if F == "second_trip":
        F1, late = SYN_WAVES * _cus(), SYN_WAVES + 1
        len_a = 97 * (F1 - 1) + N
        nw = _narrow_windows(N)
        pos = np.r_[97 * np.arange(F1), len_a + 5 + (N + 5) * np.arange(late)].astype(np.int64)
        lo = np.r_[np.zeros(F1), [nw[i % len(nw)][0] for i in range(late)]].astype(np.int32)
        hi = np.r_[np.full(F1, N), [nw[i % len(nw)][1] for i in range(late)]].astype(np.int32)
        gy = np.r_[1.0e3 * rng.normal(size=len_a), rng.normal(size=5 + (N + 5) * late)]
    else:
        total = 3 * N + 500
        tab = _geometry(N, total, rng)[:F]
        pos, lo, hi = (np.array([t[i] for t in tab], dtype=d) for i, d in enumerate((np.int64, np.int32, np.int32)))
        gy = rng.normal(size=total)
    gy[~_named_samples(gy.size, pos, lo, hi, N)] = np.nan
    return gy.astype(np.float32), pos, lo, hi


def _syn_rows(N, R, rng, opposite=False):
    """Log-normal mag, p = real + j imag of radius 0.25 .. 4; row 1: exact zeros of p (bins 0 and N/2 among them) and of
    one component; row 2: exact zeros of mag.  opposite: the last row is minus the one before it, to a thousandth."""
    H = N // 2 + 1
    mag = np.exp(0.5 * rng.normal(size=(R, H)))
    p = rng.uniform(0.25, 4.0, size=(R, H)) * np.exp(2j * np.pi * rng.random(size=(R, H)))
    if opposite:
        p[R - 1] = -p[R - 2] * (1 + 1.0e-3 * rng.normal(size=H))
    real, imag = p.real.copy(), p.imag.copy()
    if R > 1:
        real[1, [0, 5, 64, N // 4, H - 1]] = imag[1, [0, 5, 64, N // 4, H - 1]] = 0.0
        real[1, 70], imag[1, 71] = 0.0, 0.0
    if R > 2:
        mag[2, [0, 7, 63, N // 4, H - 1]] = 0.0
    return [x.astype(np.float32) for x in (mag, real, imag)]


LERP_ROWS = 12      # constant-rate rows of the row-table cases; rows 10 and 11 are nearly opposite


def _syn_lerp_tables(F, rng):
    """Row indices in no order; frame 0: row0 == row1 (weight exactly 1 whatever t), 1 / 2: t = 0 / 1, 3 / 4: the two nearly
    opposite rows about their middle, 5: the row with the zeros of p, twice."""
    row0 = rng.integers(0, 10, F).astype(np.int32)
    row1 = rng.integers(0, 10, F).astype(np.int32)
    t = rng.random(F).astype(np.float32)
    special = [(2, 2, 0.37), (3, 4, 0.0), (3, 4, 1.0), (10, 11, 0.5), (11, 10, 0.4999), (1, 1, 0.9)]
    for f, (a, b, w) in enumerate(special[:F]):
        row0[f], row1[f], t[f] = a, b, w
    return row0, row1, t


@functools.lru_cache(maxsize=None)
def _syn_case(N, F, lerp, onehot=False):
    """Tables, rows, device operands and the model of one part A case (computed once, shared, left unchanged)."""
    e = _engine()
    rng = np.random.default_rng([N, 0 if isinstance(F, str) else F, int(lerp), int(onehot)])
    H = N // 2 + 1
    if onehot:      # full windows over zeros with one sample of 0.75 at window sample 0, 1, N/2 - 1, N/2, N - 1
        at = (0, 1, N // 2 - 1, N // 2, N - 1)
        gy = np.zeros(len(at) * N, np.float32)
        pos = (N * np.arange(len(at))).astype(np.int64)
        gy[pos + np.array(at)] = 0.75
        lo, hi = np.zeros(len(at), np.int32), np.full(len(at), N, np.int32)
    else:
        gy, pos, lo, hi = _syn_tables(N, F, rng)
    n = len(pos)
    tabs = _syn_lerp_tables(n, rng) if lerp else None
    rows = _syn_rows(N, LERP_ROWS if lerp else n, rng, opposite=lerp)
    if lerp:
        named = np.zeros(LERP_ROWS, dtype=bool)
        named[tabs[0]] = named[tabs[1]] = True
        for x in rows:
            x[~named] = np.nan
    ld, ldg = H + 3, H + 5
    c = dict(N=N, F=n, gy=gy, pos=pos, lo=lo, hi=hi, rows=rows, tabs=tabs, ld=ld, ldg=ldg)
    c["d_gy"] = _dev(e, gy, guard=2 * N)
    c["d_tab"] = [_dev(e, pos), _dev(e, lo), _dev(e, hi)]
    c["d_rows"] = [_dev_rows(e, x, ld) for x in rows]
    c["d_lerp"] = [_dev(e, x) for x in tabs] if lerp else [None, None, None]
    p = bk.synth_backward_parts(np.nan_to_num(gy), pos, lo, hi, *[np.nan_to_num(x) for x in rows], N, *(tabs or ()))
    E = (5 * np.log2(N) + C_A) * U * (bk.ck(N) / N)[None, :] * p["l1"][:, None]
    aG = np.abs(p["gX"])
    gain = np.abs(p["m"]) / p["den"]
    c["ref"] = p["rows"]
    c["bound"] = (E + C_MAG * U * aG, gain * (E + C_RI * U * aG), gain * (E + C_RI * U * aG))
    c["p_zero"] = (p["a"] == 0) & (p["b"] == 0)
    c["empty"] = p["l1"] == 0
    c["model"] = p
    return c


def _launch_syn(c, streams=(True, True, True), rows=None, lerp=True):
    """One launch of the case -> three [F x H] arrays ([0 x H] for a null stream).  rows: other device rows (pitch ld) to be
    read without row tables."""
    e, N, F = _engine(), c["N"], c["F"]
    outs = [Rows(e, F, N // 2 + 1, c["ldg"]) for _ in range(3)]
    d_rows = c["d_rows"] if rows is None else rows
    d_lerp = c["d_lerp"] if (rows is None and lerp) else [None, None, None]
    e.launch("mpx_synthesis_lossless_backward", N, e.tables(N), c["d_gy"], c["gy"].size, *c["d_tab"], F, *d_rows, c["ld"],
             *d_lerp, *[o.t if on else None for o, on in zip(outs, streams)], c["ldg"])
    return [o.check("synthesis backward " + s, written=F if on else 0)
            for o, s, on in zip(outs, ("grad_mag", "grad_real", "grad_imag"), streams)]


def _syn_fraction(c, dev, streams=(True, True, True), tag=""):
    """Every element of every stream that was asked for against the model -> the largest fraction of the bound; the exact
    zeros are asserted here."""
    worst = 0.0
    for s, on in enumerate(streams):
        if not on:
            assert dev[s].shape == (0, c["N"] // 2 + 1)
            continue
        got, ref, B = dev[s].astype(np.float64), c["ref"][s], c["bound"][s]
        assert got.shape == ref.shape and not np.isnan(got).any(), "stream %d: a read outside the extent" % s
        assert np.all(got[c["empty"]] == 0), "stream %d: an empty window must give exact zeros" % s
        assert np.all(got[B == 0] == 0), "stream %d: a zero bound (empty window, mag == 0) must give exact zeros" % s
        if s == 0:
            assert np.all(got[c["p_zero"]] == 0), "grad_mag must be exactly 0 where real == imag == 0"
        live = B > 0
        if live.any():
            worst = max(worst, float(np.max(np.abs(got - ref)[live] / B[live])))
    print("synthesis backward %s N=%d F=%d streams %s: %.4f of the derived bound" % (tag, c["N"], c["F"], streams, worst))
    return worst


@pytest.mark.parametrize("lerp", (False, True), ids=("plain", "rows"))
@pytest.mark.parametrize("F", (1, 11, 12, 13, 25))
@pytest.mark.parametrize("N", FFT_LENS)
def test_synthesis_backward_frame_counts_and_window_geometry(N, F, lerp):
    """1, 11, 12, 13 and 25 frames; the 25 hold every window geometry of _geometry: clamped at both ends of the buffer,
    lying tables, windows in one tile or one 64-sample row, empty windows (exact zeros in all three rows)."""
    c = _syn_case(N, F, lerp)
    dev = _launch_syn(c)
    within(_syn_fraction(c, dev, tag="count"), PIN_SYN[N], "LBK_SYN_FRACTION_OF_BOUND_%d" % N)
    if F == 25:
        assert c["empty"].sum() == 7 and (~c["empty"]).sum() == 18
        assert c["p_zero"].sum() >= 5 and (c["model"]["m"] == 0).sum() >= 5
        for a, b in zip(dev, _launch_syn(c)):
            assert _same_bits(a, b)                    # deterministic


@pytest.mark.parametrize("streams", ((True, True, True), (True, False, False), (False, True, False), (False, False, True)),
                         ids=("all", "mag", "real", "imag"))
@pytest.mark.parametrize("lerp", (False, True), ids=("plain", "rows"))
@pytest.mark.parametrize("N", FFT_LENS)
def test_synthesis_backward_second_trip_of_the_persistent_loop(N, lerp, streams):
    """12 x CUs + 13 frames: the wave of frame f takes frame f + 12 x CUs next, through the prefetch of its first tile into
    the exchange buffer, g = gn and staged_wait<P + 1> -- with one stream alone a frame issues exactly P + 1 stores.  The
    early frame is 1e3 times the late one, whose window is narrow or empty: stale LDS words that passed the mask would
    stand about 1e3 times above the bound."""
    c = _syn_case(N, "second_trip", lerp)
    assert c["F"] == _second_trip(SYN_WAVES) and c["empty"][-(SYN_WAVES + 1):].sum() == 5
    dev = _launch_syn(c, streams)
    late = slice(SYN_WAVES * _cus(), None)
    c_late = dict(c, ref=[r[late] for r in c["ref"]], bound=[b[late] for b in c["bound"]], p_zero=c["p_zero"][late],
                  empty=c["empty"][late], F=SYN_WAVES + 1)
    f_late = _syn_fraction(c_late, [d[late] if d.size else d for d in dev], streams, tag="second trip, late frames")
    within(f_late, PIN_SYN[N], "LBK_SYN_FRACTION_OF_BOUND_%d" % N)
    within(_syn_fraction(c, dev, streams, tag="second trip"), PIN_SYN[N], "LBK_SYN_FRACTION_OF_BOUND_%d" % N)
    if all(streams):
        for a, b in zip(dev, _launch_syn(c, streams)):
            assert _same_bits(a, b)


@pytest.mark.parametrize("lerp", (False, True), ids=("plain", "rows"))
@pytest.mark.parametrize("N", FFT_LENS)
def test_synthesis_backward_every_subset_of_null_outputs(N, lerp):
    """13 frames; a null grad_X is not computed, all three null launches nothing (every sentinel intact: Rows.check)."""
    c = _syn_case(N, 13, lerp)
    for streams in itertools.product((False, True), repeat=3):
        dev = _launch_syn(c, streams)
        frac = _syn_fraction(c, dev, streams, tag="null subset")
        if any(streams):
            within(frac, PIN_SYN[N], "LBK_SYN_FRACTION_OF_BOUND_%d" % N)


@pytest.mark.parametrize("lerp", (False, True), ids=("plain", "rows"))
@pytest.mark.parametrize("N", FFT_LENS)
def test_synthesis_backward_one_hot_gradients(N, lerp):
    """One sample of 0.75 at window sample 0, 1, N/2 - 1, N/2, N - 1: |gX| is flat, so every bin is held to the bound of
    one sample."""
    c = _syn_case(N, 5, lerp, onehot=True)
    flat = np.abs(c["model"]["gX"]) / (bk.ck(N) / N * 0.75)
    assert np.max(np.abs(flat - 1.0)) < 1e-12
    within(_syn_fraction(c, _launch_syn(c), tag="one-hot"), PIN_SYN[N], "LBK_SYN_FRACTION_OF_BOUND_%d" % N)


@pytest.mark.parametrize("N", FFT_LENS)
def test_synthesis_backward_row_tables_against_the_plain_instance_on_interpolated_rows(N):
    """k_synth_lossless_bwd<P, true> on the row tables against k_synth_lossless_bwd<P, false> on the rows mpx_rows_lerp
    wrote from the same tables: both within the bound of the model, and their difference within it, too (whether they are
    bit-equal is noted, not asked for: two instantiations)."""
    e, c = _engine(), _syn_case(N, 25, True)
    H, F = N // 2 + 1, c["F"]
    outs = [Rows(e, F, H, c["ld"]) for _ in range(3)]
    e.launch("mpx_rows_lerp", H, *c["d_rows"], c["ld"], *c["d_lerp"], F, *[o.t for o in outs], c["ld"])
    got_rows = [o.check("rows_lerp") for o in outs]
    model_rows = [bk.lerp32(np.nan_to_num(x), *c["tabs"]) for x in c["rows"]]
    note("LBK_ROWS_LERP_EQUALS_THE_FMA_EMULATION_%d" % N, all(_same_bits(a, b) for a, b in zip(got_rows, model_rows)))
    plain = _launch_syn(c, rows=[_dev_rows(e, x, c["ld"]) for x in got_rows])
    tabled = _launch_syn(c)
    within(_syn_fraction(c, tabled, tag="row tables"), PIN_SYN[N], "LBK_SYN_FRACTION_OF_BOUND_%d" % N)
    if all(_same_bits(a, b) for a, b in zip(got_rows, model_rows)):     # then the model saw the plain instance's rows
        within(_syn_fraction(c, plain, tag="plain on interpolated rows"), PIN_SYN[N], "LBK_SYN_FRACTION_OF_BOUND_%d" % N)
    for s in range(3):
        diff, B = np.abs(tabled[s].astype(np.float64) - plain[s]), c["bound"][s]
        assert not np.isnan(diff).any() and np.all(diff <= B), "stream %d: the two instances differ by more than the bound" % s
    note("LBK_SYN_ROW_TABLES_BIT_EQUAL_TO_PLAIN_%d" % N, all(_same_bits(a, b) for a, b in zip(tabled, plain)))


# ====================================================================================== B  mpx_analysis_lossless_backward
def _ana_geometries(N):
    """name -> (L, R): L + R + 1 < N, == N, > N (truncated); L >= N (rot = 0); L = 0; R = 0; both 0 (len = 1)."""
    return dict(short=(100, 80), exact=(N // 2, N // 2 - 1), truncated=(N // 2 + 100, N // 2 + 300), rot0=(N + 50, 64),
                left0=(0, 37), right0=(41, 0), single=(0, 0), long_left=(N - 1, 5))


def _place(LR, N, rng, cap=None, gaps=True):
    """Frame positions with non-decreasing starts and ends, three samples no frame covers in front, some in between (after
    every fifth frame) and behind; total no multiple of 256.  cap: the slots' lengths where they are not the frames' len."""
    n = np.array([bk.frame_len(L, R, N) for L, R in LR]) if cap is None else np.asarray(cap)
    pos, start, end = [], 3, 3
    for i, (L, _R) in enumerate(LR):
        s = max(start + int(rng.integers(0, 40)), end - int(n[i]))
        if gaps and i % 5 == 4:
            s = max(s, end + 5)
        pos.append(s + L)
        start, end = s, s + int(n[i])
    total = end + 7
    total += 1 if total % 256 == 0 else 0
    return np.array(pos, np.int64), total


def _ana_rows(N, F, rng, special=True):
    """Forward-like rows: log-normal mag, unit phasors (bins 0 and N/2 included: their imaginary part must be dropped).
    special, by frame: 1: dead bins (mag 0, 1e-30, 1e-19) among live ones; 2: mag 1e-18 throughout (live, finite);
    3: nothing but dead bins under live phasors and gradients (exact zeros); 4: a silent frame, all three rows 0."""
    H = N // 2 + 1
    mag = np.exp(0.5 * rng.normal(size=(F, H)))
    ph = np.exp(2j * np.pi * rng.random(size=(F, H)))
    real, imag = ph.real.copy(), ph.imag.copy()
    if special and F > 1:
        mag[1, [0, 3, 64, N // 4, H - 1]], mag[1, [5, 6, H - 2]], mag[1, [9, 10, 65]] = 0.0, 1.0e-30, 1.0e-19
    if special and F > 2:
        mag[2] = 1.0e-18
    if special and F > 3:
        mag[3] = np.array([0.0, 1.0e-30, 1.0e-19])[np.arange(H) % 3]
    if special and F > 4:
        mag[4] = real[4] = imag[4] = 0.0
    return [x.astype(np.float32) for x in (mag, real, imag)]


def _count_frames(N, F, rng):
    """F short frames (L, R <= 40; every 7th L == 0, every 11th R == 0); at fft_len 4096 frames 5 .. 24 are long ones
    (L = R = 1500) fewer than 40 samples apart, closer than at 400 Hz: all twenty cover one sample."""
    left = rng.integers(1, 41, F)
    right = rng.integers(1, 41, F)
    left[::7], right[::11] = 0, 0
    if N == 4096 and F >= 25:
        left[5:25] = right[5:25] = 1500
    return list(zip(left.tolist(), right.tolist()))


def _ana_setup(e, N, LR, rng, grads=None, special=True, scale_early=None):
    """Host tables and rows of one launch of part B / C (no device work beyond the uploads of the rows)."""
    F, H = len(LR), N // 2 + 1
    left, right = np.array([x[0] for x in LR], np.int32), np.array([x[1] for x in LR], np.int32)
    pos, total = _place(LR, N, rng, gaps=not (N == 4096 and F >= 25))     # (the long frames follow one another closely)
    n = np.array([bk.frame_len(L, R, N) for L, R in LR])
    off = np.concatenate(([0], np.cumsum(n))).astype(np.int64)
    rows = _ana_rows(N, F, rng, special)
    if grads is None:
        grads = [rng.normal(size=(F, H)).astype(np.float32) for _ in range(3)]
        if scale_early:
            for g in grads:
                g[:scale_early] *= np.float32(1.0e3)
    ld, ldg = H + 3, H + 5
    return dict(N=N, F=F, left=left, right=right, pos=pos, total=total, off=off, n=n, rows=rows, grads=grads, ld=ld, ldg=ldg,
                d_rows=[_dev_rows(e, x, ld) for x in rows], d_geo=[_dev(e, pos), _dev(e, left), _dev(e, right)])


def _launch_ana(c, streams=(True, True, True), off=None, scratch_floats=None, d_grads=None):
    """mpx_analysis_lossless_backward -> (scratch [scratch_alloc], grad_sig [total]) read back, guards checked.  off /
    scratch_floats: tables other than the contract's; the scratch allocation always holds max(off) floats."""
    e, N, F = _engine(), c["N"], c["F"]
    off = c["off"] if off is None else np.asarray(off, np.int64)
    alloc = int(max(off.max(), c["off"][-1]))
    sf = alloc if scratch_floats is None else int(scratch_floats)
    scratch, gsig = Flat(e, alloc, 2 * N), Flat(e, c["total"], 2 * N)
    if d_grads is None:
        d_grads = [_dev_rows(e, g, c["ldg"]) for g in c["grads"]]
    e.launch("mpx_analysis_lossless_backward", N, e.tables(N), *c["d_rows"], c["ld"],
             *[g if on else None for g, on in zip(d_grads, streams)], c["ldg"], *c["d_geo"], _dev(e, off), F, scratch.t, sf,
             gsig.t, c["total"])
    return scratch.check("analysis backward scratch"), gsig.check("analysis backward grad_sig")


def _ana_model(c, grads, eg=None):
    """-> (per-frame float64 samples, per-frame additive bound: the sample's bound is w(k) times it)."""
    rows = [np.nan_to_num(x) for x in c["rows"]]
    frames = bk.analysis_backward_frames(*rows, *grads, c["left"], c["right"], c["N"])
    ysum, pw = bk.analysis_bound_terms(*rows, *grads, c["N"], eg)
    return frames, (5 * np.log2(c["N"]) + C_B) * U * ysum + pw


def _scratch_fraction(c, scratch, frames, bound, off=None, scratch_floats=None, tag=""):
    """Every sample of every frame's slot against the model; everything else of the scratch must hold the sentinel.
    -> the largest fraction of the bound."""
    off = c["off"] if off is None else np.asarray(off)
    sf = scratch.size if scratch_floats is None else int(scratch_floats)
    untouched = np.ones(scratch.size, dtype=bool)
    worst = 0.0
    for f in range(c["F"]):
        o, cap = int(off[f]), int(off[f + 1] - off[f])
        if o < 0 or cap < 0 or o + cap > sf:
            continue                                            # the slot does not lie within the scratch: nothing written
        nv = min(int(c["n"][f]), cap)
        untouched[o:o + nv] = False
        got = scratch[o:o + nv].astype(np.float64)
        assert not np.isnan(got).any(), "frame %d: a read outside the extent" % f
        B = window(int(c["left"][f]), int(c["right"][f]), int(c["n"][f]))[:nv] * bound[f]
        err = np.abs(got - frames[f][:nv])
        assert np.all(got[B == 0] == 0), "frame %d: a zero bound (dead bins, a weight of 0) must give exact zeros" % f
        if np.any(B > 0):
            worst = max(worst, float(np.max(err[B > 0] / B[B > 0])))
    assert np.all(scratch[untouched] == SENT), "written outside the frames' own part of the scratch"
    print("analysis backward %s N=%d F=%d: %.4f of the derived bound" % (tag, c["N"], c["F"], worst))
    return worst


def _hold_gather(c, scratch, gsig, off=None, scratch_floats=None):
    """grad_sig is the float32 sum, in ascending frame order, of the device's own scratch: bit for bit; 0 where no frame
    covers the sample."""
    off = c["off"] if off is None else np.asarray(off)
    sf = scratch.size if scratch_floats is None else int(scratch_floats)
    ref = bk.gather(scratch[:sf], c["pos"], c["left"], off, c["total"], np.float32)
    assert not np.isnan(gsig).any() and _same_bits(gsig, ref)
    covered = np.zeros(c["total"], dtype=bool)
    for f in range(c["F"]):
        s = int(c["pos"][f] - c["left"][f])
        covered[max(s, 0):s + int(off[f + 1] - off[f])] = True
    assert not gsig[~covered].any()
    return covered


def _ana_case_check(c, streams=(True, True, True), tag="", label="LBK_ANA_FRACTION_OF_BOUND_%d", pin=None):
    scratch, gsig = _launch_ana(c, streams)
    grads = [g if on else None for g, on in zip(c["grads"], streams)]
    frames, bound = _ana_model(c, grads)
    frac = _scratch_fraction(c, scratch, frames, bound, tag=tag)
    within(frac, (pin or PIN_ANA)[c["N"]], label % c["N"])
    covered = _hold_gather(c, scratch, gsig)
    return scratch, gsig, covered


@pytest.mark.parametrize("kind", ("short", "exact", "truncated", "rot0", "left0", "right0", "single", "long_left", "mixed"))
@pytest.mark.parametrize("N", FFT_LENS)
def test_analysis_backward_frame_geometries(N, kind):
    """Three frames of one geometry (one utterance), and all eight geometries three times over in one launch."""
    e, geo = _engine(), _ana_geometries(N)
    LR = [geo[kind]] * 3 if kind != "mixed" else [geo[k] for k in sorted(geo)] * 3
    if kind == "mixed":     # frame ends must not decrease: the long ones last
        LR = sorted(LR, key=lambda x: bk.frame_len(x[0], x[1], N))
    c = _ana_setup(e, N, LR, np.random.default_rng([N, len(LR)]), special=(kind == "mixed"))
    _s, gsig, covered = _ana_case_check(c, tag=kind)
    assert c["total"] % 256 != 0 and not covered[:3].any() and not covered[-7:].any()
    if kind == "mixed":
        assert (~covered[3:-7]).sum() >= 5 and np.any(c["left"] >= N) and np.any(c["n"] == 1)


@pytest.mark.parametrize("F", (1, 7, 8, 9, 12, 13, 25, "second_trip"))
@pytest.mark.parametrize("N", FFT_LENS)
def test_analysis_backward_frame_counts(N, F):
    """1 .. 25 frames, and waves x CUs + waves + 1 (12 waves per workgroup, 8 at fft_len 4096): every wave of workgroup 0 and
    one of workgroup 1 take a second frame; the first-trip frames' gradients are 1e3 times the others'."""
    e = _engine()
    n = _second_trip(ana_waves(N)) if F == "second_trip" else F
    rng = np.random.default_rng([N, n, 1])
    c = _ana_setup(e, N, _count_frames(N, n, rng), rng, scale_early=ana_waves(N) * _cus() if F == "second_trip" else None)
    scratch, gsig, covered = _ana_case_check(c, tag="count %s" % F)
    if N == 4096 and n >= 25:
        cover = np.zeros(c["total"], int)
        for f in range(n):
            cover[c["pos"][f] - c["left"][f]:c["pos"][f] - c["left"][f] + c["n"][f]] += 1
        assert cover.max() >= 15
    if n == 25:
        s2, g2 = _launch_ana(c)
        assert _same_bits(scratch, s2) and _same_bits(gsig, g2)


@pytest.mark.parametrize("N", FFT_LENS)
def test_analysis_backward_dead_region(N):
    """Bins with mag 0, 1e-30 and 1e-19 (mag^2 < 1e-37) contribute exactly zero, bins with mag 1e-18 are live and finite;
    a frame of dead bins only and a silent frame give exact zeros, never NaN."""
    e = _engine()
    c = _ana_setup(e, N, [(100, 80)] * 6, np.random.default_rng([N, 6, 2]))
    scratch, _g, _c = _ana_case_check(c, tag="dead region")
    for f in (3, 4):
        assert not scratch[c["off"][f]:c["off"][f + 1]].any()
    live = scratch[c["off"][2]:c["off"][3]]
    assert np.all(np.isfinite(live)) and np.max(np.abs(live)) > 1.0e15
    # the dead bins of frame 1 under huge gradients: still exactly nothing
    g2 = [g.copy() for g in c["grads"]]
    dead = c["rows"][0][1].astype(np.float64) ** 2 < 1.0e-37
    assert dead.sum() == 11
    for g in g2:
        g[1, dead] *= np.float32(1.0e6)
    s2, _ = _launch_ana(dict(c, grads=g2))
    assert _same_bits(s2[c["off"][1]:c["off"][2]], scratch[c["off"][1]:c["off"][2]])


def ONE_HOT_BINS(N):
    M = N // 2
    return (0, 1, 63, 64, M // 2 - 1, M // 2, M // 2 + 1, M - 1, M)


@pytest.mark.parametrize("N", FFT_LENS)
def test_analysis_backward_one_hot_gradients(N):
    """One gradient element per frame, at bins 0, 1, 63, 64, M/2 - 1, M/2, M/2 + 1, M - 1, M (M = N/2) of each stream:
    sum |Y| is that one bin, so the handover bin, the mirror blocks and the two real bins are each held on their own."""
    e, H = _engine(), N // 2 + 1
    bins = ONE_HOT_BINS(N)
    F = 3 * len(bins)
    grads = [np.zeros((F, H), np.float32) for _ in range(3)]
    for s in range(3):
        for i, k in enumerate(bins):
            grads[s][s * len(bins) + i, k] = 0.75
    c = _ana_setup(e, N, [(N // 3, N // 2)] * F, np.random.default_rng([N, F, 3]), grads=grads, special=False)
    scratch, _g, _c = _ana_case_check(c, tag="one-hot")
    assert np.count_nonzero(scratch != SENT) > 0.9 * c["off"][-1]


@pytest.mark.parametrize("N", FFT_LENS)
def test_analysis_backward_every_subset_of_null_streams(N):
    e = _engine()
    c = _ana_setup(e, N, _count_frames(N, 13, np.random.default_rng(N)), np.random.default_rng([N, 13, 4]))
    for streams in itertools.product((False, True), repeat=3):
        if any(streams):
            _ana_case_check(c, streams, tag="null subset %s" % (streams,))
        else:       # nothing to propagate: nothing launched, grad_sig and scratch keep their sentinels
            scratch, gsig = _launch_ana(c, streams)
            assert np.all(scratch == SENT) and np.all(gsig == SENT)


@pytest.mark.parametrize("N", FFT_LENS)
def test_analysis_backward_scratch_slots_off_contract(N):
    """scratch_off other than the prefix sums of len: a slot in front of the scratch (nothing written, nothing added); a
    slot longer than len (the rest keeps the sentinel); a slot shorter than len (only cap samples written); slots that
    reach past scratch_floats (nothing written, nothing added) -- inside an allocation that holds them all."""
    e = _engine()
    LR = [(100, 80), (60, 90), (120, 70), (100, 100), (90, 90), (40, 200)]
    n = np.array([bk.frame_len(L, R, N) for L, R in LR])
    cap = n + np.array([0, 3, -5, 0, 0, 0])
    off = np.concatenate(([-10], -10 + np.cumsum(cap))).astype(np.int64)
    sf = int(off[4] + cap[4] - 2)
    rng = np.random.default_rng([N, 5])
    c = _ana_setup(e, N, LR, rng, special=False)
    c["pos"], c["total"] = _place(LR, N, rng, cap=cap)
    c["d_geo"][0] = _dev(e, c["pos"])
    scratch, gsig = _launch_ana(c, off=off, scratch_floats=sf)
    frames, bound = _ana_model(c, c["grads"])
    frac = _scratch_fraction(c, scratch, frames, bound, off, sf, tag="off-contract slots")
    within(frac, PIN_ANA[N], "LBK_ANA_FRACTION_OF_BOUND_%d" % N)
    assert np.count_nonzero(scratch != SENT) == n[1] + cap[2] + n[3]
    _hold_gather(c, scratch, gsig, off, sf)
    s0 = int(c["pos"][0] - c["left"][0])
    assert np.any(gsig[int(c["pos"][1] - c["left"][1]):] != 0) and not gsig[:s0].any()


# =========================================================================== C  mpx_analysis_lossless_const_rate_backward
def _cr_ranges(F, n_c, rng, early):
    """Hand-built (a0, a1, b0, b1) per frame: ranges that overlap (weight 1), ranges of 25 rows, frames no row reads (also
    from frame `early` on: the second trip), ranges below 0 and above n_c, an empty range written as a1 < a0."""
    r = np.zeros((F, 4), np.int32)
    for f in range(F):
        a0 = (f * (n_c - 6)) // F
        a1 = a0 + int(rng.integers(0, 4))
        b0 = a1 - int(rng.integers(0, min(2, a1 - a0) + 1))
        r[f] = (a0, a1, b0, b0 + int(rng.integers(0, 4)))
        if f % 7 == 5 or (f >= early and f % 2 == 1):
            r[f] = (a0, a0, a1, a1)                        # no row reads this frame
    r[0] = (-2, 3, -1, 2)
    if F > 2:
        r[2] = (5, 30, 28, 31)
    if F > 3:
        r[3] = (7, 3, 8, 9)
    if F > 5:
        r[5] = (n_c + 1, n_c + 2, n_c, n_c + 2)            # wholly above: nothing
    r[F - 1] = (n_c - 2, n_c + 2, n_c - 1, n_c + 1)
    return r


def _cr_setup(N, F, seed):
    e, H = _engine(), N // 2 + 1
    rng = np.random.default_rng([N, F, seed])
    n_c = 40
    early = ana_waves(N) * _cus()
    c = _ana_setup(e, N, _count_frames(N, F, rng), rng, special=F >= 5)
    ranges = _cr_ranges(F, n_c, rng, early)
    rowt = rng.random(n_c).astype(np.float32)
    g = [rng.normal(size=(n_c, H)).astype(np.float32) for _ in range(3)]
    named = np.zeros(n_c, dtype=bool)
    for a0, a1, b0, b1 in bk.clamp_ranges(ranges, n_c).tolist():
        named[a0:max(a1, a0)] = True
        named[b0:max(b1, b0)] = True
    for x in g:
        x[~named] = np.nan
    c.update(n_c=n_c, ranges=ranges, rowt=rowt, g=g, d_g=[_dev_rows(e, x, c["ldg"], guard=2 * c["ldg"] + 64) for x in g],
             d_rowt=_dev(e, rowt))
    return c


def _launch_cr(c, ranges, n_c=None, tables=True):
    e, N = _engine(), c["N"]
    scratch, gsig = Flat(e, int(c["off"][-1]), 2 * N), Flat(e, c["total"], 2 * N)
    n_c = c["n_c"] if n_c is None else n_c
    e.launch("mpx_analysis_lossless_const_rate_backward", N, e.tables(N), *c["d_rows"], c["ld"], *c["d_g"], c["ldg"], n_c,
             _dev(e, ranges.reshape(-1)) if tables else None, c["d_rowt"] if tables else None, *c["d_geo"], _dev(e, c["off"]),
             c["F"], scratch.t, int(c["off"][-1]), gsig.t, c["total"])
    return scratch.check("const-rate backward scratch"), gsig.check("const-rate backward grad_sig")


@pytest.mark.parametrize("F", (1, 7, 8, 9, 12, 13, 25, "second_trip"))
@pytest.mark.parametrize("N", FFT_LENS)
def test_const_rate_backward_equals_the_staged_form_bit_for_bit_and_the_model(N, F):
    """Hand-built ranges, lying ones included: scratch and grad_sig equal mpx_rows_lerp_adjoint (on the clamped ranges: that
    entry does not clamp) followed by mpx_analysis_lossless_backward bit for bit; the scratch is within the bound of the
    float64 model with the clamped ranges; frames that no row reads write zeros to their scratch."""
    e, H = _engine(), N // 2 + 1
    n = _second_trip(ana_waves(N)) if F == "second_trip" else F
    c = _cr_setup(N, n, 6)
    scratch, gsig = _launch_cr(c, c["ranges"])
    clamped = bk.clamp_ranges(c["ranges"], c["n_c"])
    # ---- the staged form
    var = [Rows(e, n, H, c["ldg"]) for _ in range(3)]
    e.launch("mpx_rows_lerp_adjoint", H, *c["d_g"], c["ldg"], _dev(e, clamped.reshape(-1)), c["d_rowt"], n,
             *[v.t for v in var], c["ldg"])
    var_rows = [v.check("rows_lerp_adjoint") for v in var]
    assert not any(np.isnan(v).any() for v in var_rows), "a constant-rate row outside the clamped ranges was read"
    s2, g2 = _launch_ana(c, d_grads=[v.t for v in var])
    assert _same_bits(scratch, s2) and _same_bits(gsig, g2)
    if n <= 25:     # the staged rows are the float32 fma sequence of the model, bit for bit
        for v, x in zip(var_rows, c["g"]):
            assert _same_bits(v, bk.cr_gradient_rows(np.nan_to_num(x), c["ranges"], c["rowt"], c["n_c"], np.float32))
    # ---- the float64 model
    g64 = [np.nan_to_num(x) for x in c["g"]]
    grads = [bk.cr_gradient_rows(x, c["ranges"], c["rowt"], c["n_c"], np.float64) for x in g64]
    eg = [bk.cr_gradient_rows_error(x, c["ranges"], c["rowt"], c["n_c"]) for x in g64]
    frames, bound = _ana_model(c, grads, eg)
    frac = _scratch_fraction(c, scratch, frames, bound, tag="const rate %s" % F)
    within(frac, PIN_CR[N], "LBK_CR_FRACTION_OF_BOUND_%d" % N)
    _hold_gather(c, scratch, gsig)
    unread = [f for f, r in enumerate(clamped.tolist()) if r[1] <= r[0] and r[3] <= r[2]]
    assert len(unread) >= (1 if n > 5 else 0) and (n < 100 or max(unread) >= ana_waves(N) * _cus())
    for f in unread:
        assert not scratch[c["off"][f]:c["off"][f + 1]].any(), "frame %d: no row reads it, its scratch must be zeros" % f


@pytest.mark.parametrize("N", FFT_LENS)
def test_const_rate_backward_without_constant_rate_rows(N):
    """n_const_rows == 0: grad_sig is all zero (ranges and row_t may be null), the scratch is not touched."""
    c = _cr_setup(N, 9, 7)
    for tables in (True, False):
        scratch, gsig = _launch_cr(c, c["ranges"], n_c=0, tables=tables)
        assert np.all(scratch == SENT) and gsig.size == c["total"] and not gsig.any()
