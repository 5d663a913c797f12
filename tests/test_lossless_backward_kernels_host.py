"""CPU: tests/lossless_backward_kernels_model.py -- the table-driven float64 model that
tests/test_gpu_lossless_backward_kernels.py holds the kernels of magphase_grad.hip to -- against the autograd models
(torch float64 autograd: tests/lossless_autograd_model.py, lossless_analysis_autograd_model.py,
const_rate_analysis_autograd_model.py) on the tables hostmath builds from small plans, its adjoint identities against the
forward models of tests/lossless_kernels_model.py, its two float32 parts, and every argument-error branch of
mpx_synthesis_lossless_backward and mpx_analysis_lossless_backward (they return before any launch).  Needs no GPU."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import const_rate_analysis_autograd_model as cram
import lossless_analysis_autograd_model as lam
import lossless_autograd_model as lsm
import lossless_backward_kernels_model as bk
import lossless_kernels_model as lk
from magphase_amd import _lib
from magphase_amd import hostmath as hm

TOL = 1.0e-11       # relative to the largest value: the model itself is pinned


def _rel(got, ref):
    return lsm.rel_err(got, ref)


# ------------------------------------------------------------------------------------------------ the float32 parts
def test_fma32_is_the_correctly_rounded_fused_multiply_add():
    rng = np.random.default_rng(1)
    a = rng.normal(size=4000).astype(np.float32)
    b = rng.normal(size=4000).astype(np.float32)
    c = (-(a.astype(np.float64) * b) * (1 + rng.normal(size=4000) * 2.0 ** rng.integers(-30, 0, 4000))).astype(np.float32)
    # ties of the double rounding: a b + c exactly half an ulp of float32 above a float32, plus one bit far below
    a[:4], b[:4] = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12)     # 1 + 2^-11 + 2^-24: a tie of float32 ...
    c[:4] = np.array([2.0 ** -60, -2.0 ** -60, 0.0, 2.0 ** -100], np.float32)  # ... moved off it by less than float64 sees
    got = bk.fma32(a, b, c)
    for i in list(range(8)) + list(rng.integers(0, 4000, 300)):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = np.float32(float(exact))                  # Fraction -> float is correctly rounded; so is float64 -> float32 of
        cands = [np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))]   # a neighbour of it
        best = min(cands, key=lambda v: (abs(Fraction(float(v)) - exact), int(v.view(np.uint32)) & 1))
        assert got[i] == best, (i, got[i], best)
    assert got[0] == np.float32(1 + 2.0 ** -11 + 2.0 ** -23) and got[1] == np.float32(1 + 2.0 ** -11)
    assert got[2] == np.float32(1 + 2.0 ** -11)        # the tie itself: to even


def test_lerp32_of_one_row_and_at_the_ends():
    rng = np.random.default_rng(2)
    x = rng.normal(size=(5, 9)).astype(np.float32)
    y = bk.lerp32(x, [2, 0, 0, 3], [2, 4, 4, 1], [0.37, 0.0, 1.0, 0.5])
    assert np.array_equal(y[0], x[2]) and np.array_equal(y[1], x[0])
    assert np.max(np.abs(y[2] - x[4])) <= 2.0 ** -24 * np.max(np.abs(x))
    assert np.max(np.abs(y[3] - 0.5 * (x[3].astype(np.float64) + x[1]))) <= 2.0 ** -23 * np.max(np.abs(x))


def test_gather_in_float32_is_the_sequential_sum():
    rng = np.random.default_rng(3)
    left = np.array([3, 3, 0, 5], np.int32)
    pos = np.array([5, 6, 9, 20], np.int64)
    off = np.array([0, 7, 14, 15, 24], np.int64)
    scratch = rng.normal(size=24).astype(np.float32)
    out = bk.gather(scratch, pos, left, off, 27, np.float32)
    ref = np.zeros(27, np.float32)
    for f in range(4):
        for k in range(int(off[f + 1] - off[f])):
            ref[pos[f] - left[f] + k] = np.float32(ref[pos[f] - left[f] + k] + scratch[off[f] + k])
    assert out.dtype == np.float32 and np.array_equal(out, ref) and not out[:2].any() and not out[24:].any()
    # a slot that does not lie within the scratch adds nothing
    cut = bk.gather(scratch[:20], pos, left, off, 27, np.float32)
    assert np.array_equal(cut[:15], ref[:15]) and not cut[15:].any()


def test_cr_gradient_rows_float32_is_the_fma_sequence_and_clamps():
    rng = np.random.default_rng(4)
    g = rng.normal(size=(6, 11)).astype(np.float32)
    t = rng.random(6).astype(np.float32)
    ranges = np.array([[0, 2, 1, 4], [-3, 1, 5, 9], [4, 4, 2, 2], [7, 9, 6, 8]], np.int32)
    got = bk.cr_gradient_rows(g, ranges, t, 6, np.float32)
    ref = np.zeros((4, 11), np.float32)
    for f, rows in enumerate(([(0, 1 - t[0]), (1, 1.0), (2, t[2]), (3, t[3])], [(0, 1 - t[0]), (5, t[5])], [], [])):
        for c, w in rows:
            ref[f] = bk.fma32(np.float32(w), g[c], ref[f])
    assert got.dtype == np.float32 and np.array_equal(got, ref)
    wide = bk.cr_gradient_rows(g, ranges, t, 6, np.float64)
    assert np.max(np.abs(wide - got)) < 1e-6
    assert np.allclose(wide, cram.lerp_adjoint(g, bk.clamp_ranges(ranges, 6), t), rtol=0, atol=1e-15)
    assert np.all(bk.cr_gradient_rows_error(g, ranges, t, 6) >= np.abs(wide - got))
    assert bk.cr_gradient_rows(None, ranges, t, 6) is None


# ------------------------------------------------------------------------------- the model against the autograd models
def _synthesis_batch(N, seed, exact=False):
    """Three utterances (the last one's first epoch beyond N/2: ola_plan's negative-start case, in which no frame reaches
    the kept output and every gradient is zero) -> rows, tables, gradients."""
    rng = np.random.default_rng(seed)
    H = N // 2 + 1
    v_pm = [np.cumsum(rng.integers(40, 200, 9)), 300 + np.cumsum(rng.integers(30, 300, 6)),
            N // 2 + 70 + np.cumsum(rng.integers(30, 300, 4))]
    plans = [hm.ola_plan(p, N) for p in v_pm]
    frame_off = np.concatenate(([0], np.cumsum([p.size for p in v_pm])))
    out_len = [p[2] for p in plans]
    out_off = np.concatenate(([0], np.cumsum(out_len)))
    pos, lo, hi = hm.lossless_backward_table(np.concatenate([p[0] for p in plans]), frame_off, [p[1] for p in plans],
                                             out_len, out_off[:-1], N)
    F = int(frame_off[-1])
    R = F if not exact else F // 2 + 2
    if exact:       # integers times a power of two: the float32 interpolation with t = k / 8 does not round
        rows = [rng.integers(1, 2047, size=(R, H)) / 64.0] + [rng.integers(-2047, 2048, size=(R, H)) / 256.0 for _ in range(2)]
    else:
        rows = [np.exp(0.5 * rng.normal(size=(R, H))), rng.normal(size=(R, H)), rng.normal(size=(R, H))]
        rows[1][1, [0, 5, H - 1]] = rows[2][1, [0, 5, H - 1]] = 0.0       # p == 0: the divisor is 1
        rows[0][2, [0, 7, H - 1]] = 0.0
    rows = [x.astype(np.float32) for x in rows]
    gy = [rng.normal(size=n) for n in out_len]
    return dict(v_pm=v_pm, frame_off=frame_off, pos=pos, lo=lo, hi=hi, rows=rows, gy=gy, F=F, R=R)


@pytest.mark.parametrize("N", (1024, 2048))
def test_synthesis_model_equals_autograd_on_the_planners_tables(N):
    c = _synthesis_batch(N, N)
    assert np.any(c["lo"] > 0) and np.any(c["hi"] < N)
    got = bk.synth_backward_rows(np.concatenate(c["gy"]), c["pos"], c["lo"], c["hi"], *c["rows"], N)
    for u in range(3):
        a, b = c["frame_off"][u], c["frame_off"][u + 1]
        want = lsm.grads_autograd(*[x[a:b] for x in c["rows"]], c["gy"][u], c["v_pm"][u], N)
        for s in range(3):
            assert np.any(want[s] != 0) == (u < 2) and _rel(got[s][a:b], want[s]) <= TOL, (u, s, _rel(got[s][a:b], want[s]))
            assert u < 2 or not got[s][a:b].any()


def test_synthesis_model_with_row_tables_equals_autograd():
    N = 1024
    c = _synthesis_batch(N, 7, exact=True)
    F, R = c["F"], c["R"]
    row0 = (np.arange(F) // 2).astype(np.int32)
    row1 = np.minimum(row0 + np.arange(F) % 2, R - 1).astype(np.int32)
    rowt = (np.arange(F) % 9 / 8.0).astype(np.float32)
    assert np.any(row0 == row1) and np.any(rowt == 0) and np.any(rowt == 1)
    got = bk.synth_backward_rows(np.concatenate(c["gy"]), c["pos"], c["lo"], c["hi"], *c["rows"], N, row0, row1, rowt)
    table = hm.lerp_adjoint_table(row0, row1, rowt, R)
    want = lsm.const_rate_grads(c["rows"], c["gy"], (row0, row1, rowt), c["v_pm"], c["frame_off"], N)
    for s in range(3):
        folded = lsm.lerp_adjoint_by_table(table, rowt, got[s])
        assert np.any(want[s] != 0) and _rel(folded, want[s]) <= TOL, (s, _rel(folded, want[s]))


def test_synthesis_window_clamps():
    gy = np.arange(1.0, 21.0)
    w = bk.synth_windows(gy, [-3, 15, 4, 4, 4, -8, 20], [0, 0, -5, 6, 2, 0, 0], [8, 8, 99, 3, 2, 8, 8], 8)
    assert w[0].tolist() == [0, 0, 0, 1, 2, 3, 4, 5] and w[1].tolist() == [16, 17, 18, 19, 20, 0, 0, 0]
    assert w[2].tolist() == list(range(5, 13)) and not w[3:].any()
    assert bk.clamp_window(4, 6, 3, 8, 20) == (0, 0) and bk.clamp_window(-3, 0, 8, 8, 20) == (3, 8)


def _analysis_utt(N, seed, spacing=90):
    rng = np.random.RandomState(seed)
    pm_sec, voi, n = lam.epochs(14, spacing, True)
    sig = lam.tone_and_noise(rng, n)
    pm, left, right, _ = lam.frames_of(pm_sec, voi, n)
    return rng, sig, pm, left, right


@pytest.mark.parametrize("which", [(True, True, True), (True, False, False), (False, True, False), (False, False, True)])
@pytest.mark.parametrize("N,spacing", [(1024, 90), (1024, 700)])
def test_analysis_model_equals_autograd_on_the_planners_tables(N, spacing, which):
    rng, sig, pm, left, right = _analysis_utt(N, 3 + sum(which), spacing)
    assert spacing < 600 or np.any(left + right + 1 > N)
    rows = lam.forward_numpy(sig, pm, left, right, N)
    grads = tuple(rng.randn(pm.size, N // 2 + 1) if w else None for w in which)
    start, off = hm.analysis_backward_table(pm, left, right, N, sig.size)
    frames = bk.analysis_backward_frames(*rows, *grads, left, right, N)
    assert [f.size for f in frames] == np.diff(off).tolist() and np.array_equal(start, pm - left)
    got = bk.gather(np.concatenate(frames), pm, left, off, sig.size, np.float64)
    want = lam.grads_autograd(sig, grads, pm, left, right, N)
    assert np.any(want != 0) and _rel(got, want) <= TOL, _rel(got, want)
    assert _rel(got, lam.gather_by_table(np.concatenate(frames), start, off, sig.size)) <= 1e-15


@pytest.mark.parametrize("cr", [1.0, 5.0, 20.0])
def test_const_rate_model_equals_autograd_on_the_planners_tables(cr):
    N = 1024
    rng = np.random.RandomState(int(cr))
    pm_sec, voi, n = lam.epochs(30, 90, True)
    sig = lam.tone_and_noise(rng, n)
    frames, tabs, _f0 = cram.frames_and_tables(pm_sec, voi, n, lam.FS, cr)
    pm, left, right = frames
    rows = lam.forward_numpy(sig, pm, left, right, N)
    grads = tuple(rng.randn(tabs[0].size, N // 2 + 1) for _ in range(3))
    ranges = hm.lerp_adjoint_table(tabs[0], tabs[1], tabs[2], pm.size)
    g_var = [bk.cr_gradient_rows(g, ranges, tabs[2], tabs[0].size, np.float64) for g in grads]
    _start, off = hm.analysis_backward_table(pm, left, right, N, n)
    per_frame = bk.analysis_backward_frames(*rows, *g_var, left, right, N)
    got = bk.gather(np.concatenate(per_frame), pm, left, off, n, np.float64)
    want = cram.grads_autograd(sig, grads, frames, tabs, N)
    assert np.any(want != 0) and _rel(got, want) <= TOL, _rel(got, want)


def test_analysis_dead_region_is_decided_in_float32():
    H = 513
    mag = np.full((1, H), 1.0e-19)
    mag[0, ::2] = 1.0e-18
    gX, live = bk.analysis_gx(mag, np.ones((1, H)), np.zeros((1, H)), np.ones((1, H)), None, np.ones((1, H)))
    assert live[0, ::2].all() and not live[0, 1::2].any() and not gX[0, 1::2].any() and np.all(np.isfinite(gX))
    assert np.allclose(gX[0, ::2].imag, 1.0e18, rtol=1e-12)
    silent = bk.analysis_backward_frames(np.zeros((1, H)), np.zeros((1, H)), np.zeros((1, H)), np.ones((1, H)),
                                         np.ones((1, H)), None, [5], [7], 1024)
    assert silent[0].shape == (13,) and not silent[0].any()


# ------------------------------------------------------------------------------------------------- adjoint identities
@pytest.mark.parametrize("N", (1024, 4096))
def test_synthesis_backward_is_the_transpose_of_the_synthesis_frame(N):
    """<synthesis_frame(X), g> == <X, gX> over the real and imaginary parts of X = mag u (the imaginary parts of bins 0 and
    N/2 do not enter the forward), gX rebuilt from the model's three rows: gX = u grad_mag + (den / mag)(grad_real + j
    grad_imag)."""
    rng = np.random.default_rng(N)
    H, F = N // 2 + 1, 3
    real, imag = rng.normal(size=(F, H)), rng.normal(size=(F, H))
    mag = np.exp(0.5 * rng.normal(size=(F, H)))
    g = rng.normal(size=(F, N))
    pos = np.arange(F) * N
    p = bk.synth_backward_parts(g.ravel(), pos, np.zeros(F, int), np.full(F, N), mag, real, imag, N)
    m, a, b = p["m"], p["a"], p["b"]                       # the float32 rows the model used
    y = lk.synthesis_frame(m, a, b, N)
    u = (a + 1j * b) / p["den"]
    gX = u * p["rows"][0] + p["den"] / m * (p["rows"][1] + 1j * p["rows"][2])
    assert np.max(np.abs(gX - p["gX"])) <= 1e-12 * np.max(np.abs(gX))
    X = m * u
    X[:, [0, -1]] = X[:, [0, -1]].real
    lhs, rhs = np.sum(y * g), np.sum(X.real * gX.real + X.imag * gX.imag)
    assert abs(lhs - rhs) <= 1e-12 * np.sum(np.abs(y * g))
    # linear in mag alone: <S(mag), g> = <mag, grad_mag>
    assert abs(lhs - np.sum(m * p["rows"][0])) <= 1e-12 * np.sum(np.abs(y * g))


@pytest.mark.parametrize("L,R", [(100, 80), (0, 0), (0, 9), (9, 0), (700, 600), (1100, 50), (400, 623)])
def test_analysis_backward_is_the_transpose_of_the_analysis_frame(L, R):
    """<X(x), G> == <x, gfrm(G)> with X the spectrum of lossless_kernels_model.analysis_frame and (grad_mag, grad_real,
    grad_imag) chosen so that the model's gX is G: grad_mag = Re(conj(p) G), grad_real + j grad_imag = mag (G - p grad_mag)."""
    N = 1024
    rng = np.random.default_rng(L + R)
    n = lk.frame_len(L, R, N)
    x = rng.uniform(-0.6, 0.6, n)
    mag, real, imag, _l1 = lk.analysis_frame(x, L, L, R, N)
    X = mag * (real + 1j * imag)
    G = rng.normal(size=N // 2 + 1) + 1j * rng.normal(size=N // 2 + 1)
    pp = real + 1j * imag
    gm = (np.conj(pp) * G).real
    rest = mag * (G - pp * gm)
    rows = [v[None, :] for v in (mag, real, imag, gm, rest.real, rest.imag)]
    gX, live = bk.analysis_gx(*rows)
    Gd = G.copy()
    Gd[[0, -1]] = Gd[[0, -1]].real          # what the transform keeps of bins 0 and N/2
    assert live.all() and np.max(np.abs(half_real(gX[0]) - Gd)) <= 1e-9 * np.max(np.abs(G))
    frm = bk.analysis_backward_frames(*rows, [L], [R], N)[0]
    lhs = np.sum(X.real * G.real + X.imag * G.imag)
    assert frm.shape == (n,) and abs(lhs - np.sum(x * frm)) <= 1e-9 * np.sum(np.abs(x * frm))


def half_real(g):
    g = g.copy()
    g[[0, -1]] = g[[0, -1]].real
    return g


# ------------------------------------------------------------------------------------------- argument errors of the entries
def _failed(lib, name, rc, word):
    err = lib.mpx_last_error()
    assert rc == -1 and name in err and word in err, (rc, word, err)


def test_argument_errors_of_mpx_synthesis_lossless_backward():
    lib = _lib.load()
    one = ctypes.c_void_p(8)   # a non-null pointer that is never followed: every call below returns before a launch
    name = b"mpx_synthesis_lossless_backward"

    def call(N=1024, tables=one, gy=one, total=50, pos=one, lo=one, hi=one, n=3, rows=(one, one, one), ld=513,
             rt=(None, None, None), grads=(one, one, one), ldg=513):
        return lib.mpx_synthesis_lossless_backward(None, N, tables, gy, total, pos, lo, hi, n, rows[0], rows[1], rows[2], ld,
                                                   rt[0], rt[1], rt[2], grads[0], grads[1], grads[2], ldg)

    for bad in (1000, 512, 8192, 0):
        _failed(lib, name, call(N=bad), b"fft_len")
    for kw in (dict(n=-1), dict(total=-1)):
        _failed(lib, name, call(**kw), b"negative")
    _failed(lib, name, call(ld=512), b"ld <")
    _failed(lib, name, call(ldg=512), b"ld <")
    _failed(lib, name, call(N=4096, ld=2049, ldg=2048), b"ld <")
    for mask in range(1, 7):            # row0 / row1 / row_t given in part
        _failed(lib, name, call(rt=tuple(one if mask >> i & 1 else None for i in range(3))), b"come together")
    for kw in (dict(tables=None), dict(pos=None), dict(lo=None), dict(hi=None), dict(gy=None)):
        _failed(lib, name, call(**kw), b"null")
        _failed(lib, name, call(rt=(one, one, one), **kw), b"null")
    for s in range(3):
        rows = [one, one, one]
        rows[s] = None
        _failed(lib, name, call(rows=tuple(rows)), b"null")
    # nothing to do: no frames, or no gradient asked for -- no launch, whatever else is null; an empty buffer needs no pointer
    assert call(n=0, tables=None, pos=None, gy=None, rows=(None, None, None)) == 0
    assert call(grads=(None, None, None), tables=None, pos=None, lo=None, hi=None) == 0
    assert call(n=0, rt=(one, one, one)) == 0
    _failed(lib, name, call(n=0, rt=(one, None, one)), b"come together")       # the checks come before the early returns
    _failed(lib, name, call(grads=(None, None, None), ld=1), b"ld <")


def test_argument_errors_of_mpx_analysis_lossless_backward():
    lib = _lib.load()
    one = ctypes.c_void_p(8)
    name = b"mpx_analysis_lossless_backward"

    def call(N=1024, tables=one, rows=(one, one, one), ld=513, grads=(one, one, one), ldg=513, pos=one, left=one,
             right=one, soff=one, n=3, scratch=one, sf=100, gsig=one, total=50):
        return lib.mpx_analysis_lossless_backward(None, N, tables, rows[0], rows[1], rows[2], ld, grads[0], grads[1],
                                                  grads[2], ldg, pos, left, right, soff, n, scratch, sf, gsig, total)

    for bad in (1000, 512, 8192, 0):
        _failed(lib, name, call(N=bad), b"fft_len")
    for kw in (dict(n=-1), dict(total=-1), dict(sf=-1)):
        _failed(lib, name, call(**kw), b"negative")
    _failed(lib, name, call(ld=512), b"ld <")
    _failed(lib, name, call(ldg=512), b"ld <")
    _failed(lib, name, call(N=2048, ld=1024, ldg=1025), b"ld <")
    for kw in (dict(tables=None), dict(pos=None), dict(left=None), dict(right=None), dict(soff=None), dict(scratch=None),
               dict(gsig=None)):
        _failed(lib, name, call(**kw), b"null")
    for s in range(3):
        rows = [one, one, one]
        rows[s] = None
        _failed(lib, name, call(rows=tuple(rows)), b"null")
    _failed(lib, name, call(total=256 * 2147483647 + 1), b"too many")
    assert call(n=0, tables=None, pos=None, gsig=None, rows=(None, None, None)) == 0
    assert call(grads=(None, None, None), tables=None, soff=None, scratch=None) == 0
    for s in range(3):                  # one stream alone is a call like any other: the other checks still hold
        grads = [None, None, None]
        grads[s] = one
        _failed(lib, name, call(grads=tuple(grads), tables=None), b"null")
