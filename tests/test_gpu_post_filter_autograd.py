"""GPU: the backward kernels of the two post-filters through their C entry points, and mp.post_filter_batch with autograd,
against the float64 references of tests/post_filter_autograd_model.py (checked on the CPU by
tests/test_post_filter_autograd_host.py).

  k_post_filter_bwd              mpx_post_filter_backward vs g M, M the filter's matrix
  k_rows_gemm, k_merlin_r0_bwd   mpx_post_filter_merlin_backward vs the closed form of the gradient
  mp.post_filter_batch           forward bits, gradients of every input dtype, composition with the syntheses

Every output lies inside a larger buffer filled with a sentinel, between two guards; floating-point operands are uploaded
between runs of NaN.  No frame or bin is left out of a comparison.

MagPhase filter: the kernel sums n_i products w_ji g_j per element in float32 with fmaf, w_ji = M_ji rounded once to
float32: at most n_i + 1 roundings of relative size 2^-24, each of a partial sum bounded by sum_j |g_j M_ji|.  The
tolerance is the derived (n_i + 2) 2^-24 sum_j |g_j M_ji| per element, n_i the column's fan-in; every comparison records
error / bound (label PFA_PF_BWD_BOUND, tolerance 1).

Merlin filter: per row max |device - model| / max |model of the row|, the float64 closed form fed the device's own float32
rows.  The tolerances TOL_MERLIN_BWD are <= 3 x the worst case measured on the MI355X
(profiles/r24_post_filter_autograd_tolerance_report.json).
"""
import warnings

import numpy as np
import pytest
import torch

import compressed_synthesis_autograd_model as cs_model
import output_stage_model as osm
import post_filter_autograd_model as pfm
from _tol import within
from magphase_amd import _lib
from magphase_amd import hostmath as hm
from magphase_amd import libaudio as la
from magphase_amd import magphase as mp

pytestmark = pytest.mark.gpu

GUARD = 64         # elements before and after every output
SPARE = 192        # elements after the last one an entry may write, inside the guards
NAN_GUARD = 2112   # NaNs before and after every floating-point operand
U24 = 2.0 ** -24

# per row max |device - closed form| / max |closed form of the row|, worst over osm.MERLIN_FRAMES, both rates, pf_coef 1.4
# and 1.0 (and the hand-built tables at D = 60); measured on the MI355X, tolerance <= 3 x
#                    tolerance    measured
TOL_MERLIN_BWD = {3: 7.0e-6,      # 2.34e-6  (48 kHz, pf_coef 1.4, F = 257)
                  24: 3.0e-5,     # 1.01e-5  (48 kHz, pf_coef 1.4, F = 257)
                  60: 8.5e-6,     # 2.97e-6  (48 kHz, pf_coef 1.4, F = 257 and 16 391; hand-built tables 4.98e-7)
                  64: 9.0e-6}     # 3.09e-6  (48 kHz, pf_coef 1.4, F = 257)


def _engine():
    from magphase_amd.engine import get_engine
    return get_engine()


def _sync():
    torch.cuda.synchronize()


def _dev(e, a, dtype):
    """Upload; floating-point operands lie between two runs of NAN_GUARD NaNs."""
    a = np.ascontiguousarray(a, dtype=dtype)
    if not np.issubdtype(a.dtype, np.floating):
        return torch.from_numpy(a.reshape(-1) if a.size else np.zeros(1, dtype)).to(e.device)
    buf = np.full(a.size + 2 * NAN_GUARD, np.nan, dtype=dtype)
    buf[NAN_GUARD:NAN_GUARD + a.size] = a.ravel()
    return torch.from_numpy(buf).to(e.device)[NAN_GUARD:NAN_GUARD + a.size]


class Fenced:
    """n elements an entry may write, then SPARE it may not, between two guards; everything pre-filled with the sentinel."""

    def __init__(self, e, n, dtype=torch.float32, sentinel=osm.SENTINEL):
        self.n, self.sentinel = int(n), sentinel
        self.buf = torch.full((2 * GUARD + SPARE + self.n,), sentinel, dtype=dtype, device=e.device)
        self.ptr = self.buf[GUARD:].data_ptr()

    def check(self, what, all_written=True):
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


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# mpx_post_filter_backward
# ---------------------------------------------------------------------------------------------------------------------
PF_CASES = [(60, 48000, {}), (61, 48000, {}), (256, 48000, {}), (60, 16000, {}), (61, 16000, {}), (256, 16000, {}),
            (5, 48000, dict(av_len_at_zero=3, av_len_at_nyq=1))]
_PF = {}


def _pf_case(e, dim, fs, opts):
    """(M float64, fan-in per column, device tables) of one configuration; built once."""
    key = (dim, fs, tuple(sorted(opts.items())))
    if key not in _PF:
        tabs = pfm.pf_tables(dim, fs, **opts)
        m = pfm.pf_matrix(dim, *tabs)
        cnt, idx, w, fan = hm.post_filter_backward_tables(dim, *tabs)
        m.setflags(write=False)
        _PF[key] = (m, pfm.pf_fan_in(m), (fan, _dev(e, cnt, np.int32), _dev(e, idx, np.int32), _dev(e, w, np.float32)))
    return _PF[key]


def _pf_bwd(e, g, dim, dtab, what):
    """One call of mpx_post_filter_backward on g [F x dim] float32 -> float32 [F x dim], the buffer checked."""
    F = int(g.shape[0])
    fan, d_cnt, d_idx, d_w = dtab
    out = Fenced(e, F * dim)
    e.launch("mpx_post_filter_backward", _dev(e, g, np.float32), F, dim, d_cnt, d_idx, d_w, fan, out.ptr)
    _sync()
    if F == 0:
        out.untouched(what)
        return np.zeros((0, dim), np.float32)
    return out.check(what).reshape(F, dim)


def _pf_compare(got, g, m, fan_in, what):
    """Every element against g M within (n_i + 2) 2^-24 sum_j |g_j M_ji|; where that sum is 0 the element must be 0."""
    g64 = g.astype(np.float64)
    want = g64 @ m
    bound = (fan_in + 2)[None, :] * U24 * (np.abs(g64) @ np.abs(m))
    err = np.abs(got.astype(np.float64) - want)
    assert np.all(np.isfinite(got)), what
    zero = bound == 0
    assert np.all(got[zero] == 0), what + ": an element no output bin feeds is not zero"
    ratio = float(np.max(err[~zero] / bound[~zero])) if np.any(~zero) else 0.0
    print("%s: worst error / bound %.3g" % (what, ratio))
    within(ratio, 1.0, "PFA_PF_BWD_BOUND")


@pytest.mark.parametrize("dim,fs,opts", PF_CASES)
def test_pf_backward_one_hot_gradients_give_the_rows_of_the_matrix(dim, fs, opts):
    """Frame j carries a one-hot g_y at bin j: its g_x is row j of M -- every entry of M, the zeros exactly."""
    e = _engine()
    m, fan_in, dtab = _pf_case(e, dim, fs, opts)
    g = np.eye(dim, dtype=np.float32)
    got = _pf_bwd(e, g, dim, dtab, "pf bwd one-hot D %d fs %d" % (dim, fs))
    _pf_compare(got, g, m, fan_in, "pf bwd one-hot D %d fs %d" % (dim, fs))
    assert np.all((got != 0) == (m != 0))
    # bins 0 and D - 1 of g_y pass straight through and contribute to nothing else
    assert np.array_equal(got[0], np.eye(dim, dtype=np.float32)[0])
    assert np.array_equal(got[-1], np.eye(dim, dtype=np.float32)[-1])


@pytest.mark.parametrize("dim,fs,opts", PF_CASES)
def test_pf_backward_dense_gradients(dim, fs, opts):
    """F around the r = 256 // D rows of a workgroup, and 1031 rows (more than one workgroup at every D)."""
    e = _engine()
    m, fan_in, dtab = _pf_case(e, dim, fs, opts)
    r = 256 // dim
    rng = np.random.RandomState(dim + fs)
    g_all = _f32(rng.standard_normal((1031, dim)) * np.exp(rng.uniform(-3, 3, (1031, 1))))
    for F in sorted({1, r - 1, r, r + 1, 1031}):
        what = "pf bwd dense D %d fs %d F %d" % (dim, fs, F)
        got = _pf_bwd(e, g_all[:F], dim, dtab, what)
        if F:
            _pf_compare(got, g_all[:F], m, fan_in, what)


def test_pf_backward_engine_path_equals_the_direct_call():
    e = _engine()
    for dim, fs, opts in (PF_CASES[0], PF_CASES[5], PF_CASES[6]):
        _m, _n, dtab = _pf_case(e, dim, fs, opts)
        g = _f32(np.random.RandomState(3).standard_normal((37, dim)))
        want = _pf_bwd(e, g, dim, dtab, "pf bwd direct")
        got = e.post_filter_backward(e.to_device(g, np.float32), fs, **opts).cpu().numpy()
        assert _same_bits(got, want), (dim, fs)


def test_pf_backward_argument_checks_launch_nothing():
    e = _engine()
    _m, _n, (fan, d_cnt, d_idx, d_w) = _pf_case(e, 60, 48000, {})
    g = _dev(e, np.ones((4, 60)), np.float32)
    out = Fenced(e, 4 * 60)
    for args in ((g, 4, 2, d_cnt, d_idx, d_w, 1, out.ptr), (g, 4, 257, d_cnt, d_idx, d_w, fan, out.ptr),
                 (g, -1, 60, d_cnt, d_idx, d_w, fan, out.ptr), (g, 4, 60, d_cnt, d_idx, d_w, 0, out.ptr),
                 (g, 4, 60, d_cnt, d_idx, d_w, 61, out.ptr), (None, 4, 60, d_cnt, d_idx, d_w, fan, out.ptr),
                 (g, 4, 60, None, d_idx, d_w, fan, out.ptr), (g, 4, 60, d_cnt, None, d_w, fan, out.ptr),
                 (g, 4, 60, d_cnt, d_idx, None, fan, out.ptr), (g, 4, 60, d_cnt, d_idx, d_w, fan, None)):
        with pytest.raises(_lib.MagphaseHipError, match=r"\(-1\)"):
            e.launch("mpx_post_filter_backward", *args)
    e.launch("mpx_post_filter_backward", g, 0, 60, d_cnt, d_idx, d_w, fan, out.ptr)
    _sync()
    out.untouched("mpx_post_filter_backward that launches nothing")


# ---------------------------------------------------------------------------------------------------------------------
# mpx_post_filter_merlin_backward
# ---------------------------------------------------------------------------------------------------------------------
_MERLIN_TABLES = {}
_MERLIN_REF = {}


def _bwd_tables(t):
    return dict(c1=t["c1"], lifter=t["lifter"], g=t["g"], wk=t["wk"], cf_t=np.ascontiguousarray(np.asarray(t["cf"]).T),
                c1_t=np.ascontiguousarray(np.asarray(t["c1"]).T))


def _merlin_tables(e, dim, fs, pf):
    key = (dim, fs, pf)
    if key not in _MERLIN_TABLES:
        t = hm.merlin_tables(dim, fs, pf)
        _MERLIN_TABLES[key] = (t, {k: _dev(e, v, np.float32) for k, v in _bwd_tables(t).items()})
    return _MERLIN_TABLES[key]


def _merlin_bwd(e, x, g, fs, pf=1.4, tables=None, dim=None, n_bins=None, n_frames=None, null=(), what="merlin bwd",
                expect_written=True, refused=False):
    """One call of mpx_post_filter_merlin_backward on x, g [F x D] -> grad_in float32 [F x D]; every buffer checked."""
    F, D = x.shape
    if tables is None:
        t, d = _merlin_tables(e, D, fs, pf)
    else:
        t, d = tables, {k: _dev(e, v, np.float32) for k, v in _bwd_tables(tables).items()}
    d = dict(d, x=_dev(e, x, np.float32), g_out=_dev(e, g, np.float32))
    bufs = {k: Fenced(e, F * D) for k in ("mcep", "mcep_w", "g_pf", "g_c", "g_x")}
    ptr = {k: (None if k in null else (v.ptr if isinstance(v, Fenced) else v)) for k, v in dict(d, **bufs).items()}
    args = (ptr["x"], ptr["g_out"], F if n_frames is None else n_frames, D if dim is None else dim, ptr["c1"], ptr["lifter"],
            ptr["g"], ptr["wk"], int(np.asarray(t["g"]).shape[1]) if n_bins is None else n_bins, ptr["cf_t"], ptr["c1_t"],
            ptr["mcep"], ptr["mcep_w"], ptr["g_pf"], ptr["g_c"], ptr["g_x"])
    if refused:
        with pytest.raises(_lib.MagphaseHipError, match=r"\(-1\)"):
            e.launch("mpx_post_filter_merlin_backward", *args)
    else:
        e.launch("mpx_post_filter_merlin_backward", *args)
    _sync()
    if refused or not expect_written:
        for k, b in bufs.items():
            b.untouched(what + ": " + k)
        return None
    res = {k: b.check(what + ": " + k).reshape(F, D) for k, b in bufs.items()}
    return res["g_x"]


def _merlin_case(dim, fs, pf):
    """(x float32 [257 x D], g float32, closed form float64) -- computed once per session, never modified."""
    key = (dim, fs, pf)
    if key not in _MERLIN_REF:
        x = _f32(osm.merlin_input(dim))
        g = _f32(np.random.RandomState(1000 + dim).standard_normal(x.shape))
        want = pfm.merlin_closed_form(x, g, hm.merlin_tables(dim, fs, pf))
        assert np.all(np.isfinite(want))
        for a in (x, g, want):
            a.setflags(write=False)
        _MERLIN_REF[key] = (x, g, want)
    return _MERLIN_REF[key]


def _merlin_rel(got, want):
    """Per row max |got - want| / max |want of the row| -> the worst row."""
    assert got.shape == want.shape and np.all(np.isfinite(got))
    scale = np.max(np.abs(want), axis=1)
    assert np.all(scale > 0)
    return float(np.max(np.max(np.abs(got.astype(np.float64) - want), axis=1) / scale))


@pytest.mark.parametrize("fs", osm.MERLIN_FS)
@pytest.mark.parametrize("dim", osm.MERLIN_DIMS)
def test_merlin_backward_against_the_closed_form(dim, fs):
    """D at the argument limits and between, F around the 64-frame group of k_merlin_r0_bwd and the 4-frame group of
    k_rows_gemm; formant rows and the silent -23 rows (r0 down to 1e-20)."""
    e = _engine()
    for pf in (1.4, 1.0):
        x, g, want = _merlin_case(dim, fs, pf)
        for F in osm.MERLIN_FRAMES:
            what = "merlin bwd D %d F %d fs %d pf %.2f" % (dim, F, fs, pf)
            got = _merlin_bwd(e, x[:F], g[:F], fs, pf, what=what)
            rel = _merlin_rel(got, want[:F])
            print("%s: worst row %.3g" % (what, rel))
            within(rel, TOL_MERLIN_BWD[dim], "PFA_MERLIN_BWD_D%d" % dim)


def test_merlin_backward_engine_path_equals_the_direct_call():
    e = _engine()
    for dim, pf in ((60, 1.4), (3, 1.4), (64, 1.0)):
        x, g, _want = _merlin_case(dim, 48000, pf)
        want = _merlin_bwd(e, x[:65], g[:65], 48000, pf)
        got = e.post_filter_merlin_backward(e.to_device(x[:65], np.float32), e.to_device(g[:65], np.float32), 48000,
                                            pf_coef=pf).cpu().numpy()
        assert _same_bits(got, want), (dim, pf)


def test_merlin_backward_stride_loop_past_4096_workgroups():
    """k_rows_gemm launches at most 4 096 workgroups of 4 frames and strides beyond: F = 16 384 + 7 rows, row f a copy of row
    f mod 257.  Every row against the closed form; and a row's arithmetic has a fixed order wherever the row lies, so every
    row equals row f mod 257 of the 257-row launch bit for bit."""
    e = _engine()
    x, g, want = _merlin_case(60, 48000, 1.4)
    base = _merlin_bwd(e, x, g, 48000, what="merlin bwd 257 rows")
    F = 16384 + 7
    idx = np.arange(F) % osm.MERLIN_ROWS
    got = _merlin_bwd(e, x[idx], g[idx], 48000, what="merlin bwd 16391 rows")
    rel = _merlin_rel(got, want[idx])
    print("merlin bwd 16391 rows: worst row %.3g" % rel)
    within(rel, TOL_MERLIN_BWD[60], "PFA_MERLIN_BWD_D60")
    assert _same_bits(got, base[idx])


@pytest.mark.parametrize("last_only", [True, False])
@pytest.mark.parametrize("n_bins", [1, 64, 65])
def test_merlin_backward_chunk_cases_with_hand_built_tables(n_bins, last_only):
    """One bin, one full chunk, a full chunk and the lone tail bin.  With the weight on the last bin only S / R is that
    column of G exactly, so the gradient is lifter * (g_pf - g_d G[:, last]) + g_d G[:, last] through the two matrices."""
    e = _engine()
    dim, F = 60, 70
    rng = np.random.RandomState(n_bins)
    t = dict(hm.merlin_tables(dim, 48000, 1.4))
    t["g"] = _f32(rng.uniform(-0.05, 0.05, (dim, n_bins))).astype(np.float64)
    t["wk"] = np.zeros(n_bins)
    t["wk"][-1] = 0.75
    if not last_only:
        t["wk"][:] = _f32(rng.uniform(0.1, 1.0, n_bins))
    x, g, _ = _merlin_case(dim, 48000, 1.4)
    x, g = x[:F], g[:F]
    want = pfm.merlin_closed_form(x, g, t)
    if last_only:
        c1, cf, col = np.asarray(t["c1"]), np.asarray(t["cf"]), t["g"][:, -1]
        g_pf = g.astype(np.float64) @ cf.T
        direct = (t["lifter"] * (g_pf - g_pf[:, :1] * col) + g_pf[:, :1] * col) @ c1.T
        assert np.max(np.abs(direct - want)) <= 1e-12 * np.max(np.abs(want))
    what = "merlin bwd n_bins %d %s" % (n_bins, "last bin only" if last_only else "all bins")
    got = _merlin_bwd(e, x, g, 48000, tables=t, what=what)
    rel = _merlin_rel(got, want)
    print("%s: worst row %.3g" % (what, rel))
    within(rel, TOL_MERLIN_BWD[dim], "PFA_MERLIN_BWD_D%d" % dim)


def test_merlin_backward_magic_rows_get_zero_and_leave_their_neighbours_alone():
    """A row of +60 (both energies overflow: the forward writes la.MAGIC) and a row of NaNs at positions 0, 3 (the last of
    a 4-frame group), 63 and 64: their gradient rows are all zero; every other row -- the bad rows share LDS tiles and
    matrix tiles with them -- is bit-identical to the launch without the bad rows."""
    e = _engine()
    x, g, _ = _merlin_case(60, 48000, 1.4)
    x, g = x[:70].copy(), g[:70]
    base = _merlin_bwd(e, x, g, 48000)
    pos = (0, 3, 63, 64)
    for nan_at in ((0, 63), (3, 64)):
        bad = x.copy()
        for p in pos:
            bad[p, :] = np.nan if p in nan_at else 60.0
        fwd = e.post_filter_merlin(e.to_device(bad, np.float32), 48000).cpu().numpy()
        assert np.all(fwd[list(pos)] == np.float32(la.MAGIC))
        got = _merlin_bwd(e, bad, g, 48000, what="merlin bwd with bad rows")
        assert np.all(np.isfinite(got))
        assert np.all(got[list(pos)] == 0), nan_at
        good = np.setdiff1d(np.arange(70), pos)
        assert _same_bits(got[good], base[good]), nan_at


def test_merlin_backward_argument_checks_launch_nothing():
    e = _engine()
    x, g, _ = _merlin_case(3, 48000, 1.4)
    x, g = x[:8], g[:8]
    for kw in (dict(dim=2), dict(dim=65), dict(n_bins=0), dict(n_frames=-1), dict(null=("x",)), dict(null=("g_out",)),
               dict(null=("wk",)), dict(null=("cf_t",)), dict(null=("c1_t",)), dict(null=("g_c",)), dict(null=("g_x",))):
        _merlin_bwd(e, x, g, 48000, refused=True, what="refused mpx_post_filter_merlin_backward %r" % (kw,), **kw)
    _merlin_bwd(e, x, g, 48000, n_frames=0, expect_written=False, what="mpx_post_filter_merlin_backward with no frames")


# ---------------------------------------------------------------------------------------------------------------------
# mp.post_filter_batch
# ---------------------------------------------------------------------------------------------------------------------
PF_TYPES = ("magphase", "merlin")
DTYPES = (torch.float16, torch.bfloat16, torch.float32, torch.float64)
CAST_EPS = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8, torch.float32: 0.0, torch.float64: 0.0}


def _rows(n, dim=60, seed=0):
    """n formant rows of osm.merlin_input's generator, float32."""
    return _f32(osm.log_mel_mags(n, dim, seed=500 + seed + n))


def _engine_forward(e, x32, fs, pf_type):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return e.post_filter_merlin(x32, fs) if pf_type == "merlin" else e.post_filter(x32, fs)


@pytest.mark.parametrize("pf_type", PF_TYPES)
def test_batch_forward_is_the_engine_call_on_the_packed_rows(pf_type):
    e = _engine()
    fs = 48000
    wide = torch.from_numpy(_f32(np.random.RandomState(1).uniform(-8, 0, (9, 81)))).to(e.device)
    mats = [_rows(12).astype(np.float64),                                  # host array
            torch.from_numpy(_rows(7)).to(e.device).to(torch.float16),
            torch.from_numpy(_rows(5)).to(e.device).to(torch.bfloat16),
            torch.zeros((0, 60), device=e.device),                          # an utterance without frames
            torch.from_numpy(_rows(3)).to(e.device),
            torch.from_numpy(_rows(4).astype(np.float64)).to(e.device),
            wide[:, 10:70]]                                                # a column slice: row stride 81
    packed = torch.cat([(torch.from_numpy(m).to(e.device) if isinstance(m, np.ndarray) else m).to(torch.float32)
                        for m in mats])
    want = _engine_forward(e, packed.contiguous(), fs, pf_type).cpu().numpy()
    got = mp.post_filter_batch(mats, fs, pf_type=pf_type, return_device=True)
    host = mp.post_filter_batch(mats, fs, pf_type=pf_type)
    a = 0
    for m, gd, gh in zip(mats, got, host):
        n = int(m.shape[0])
        assert gd.dtype == torch.float32 and gd.device == e.device and tuple(gd.shape) == (n, 60) and gd.grad_fn is None
        assert isinstance(gh, np.ndarray) and gh.dtype == np.float64 and gh.shape == (n, 60)
        assert _same_bits(gd.cpu().numpy(), want[a:a + n])
        assert np.array_equal(gh, want[a:a + n].astype(np.float64))
        a += n
    assert a == want.shape[0] and np.all(np.isfinite(want)) and not np.array_equal(want, packed.cpu().numpy())
    # empty batches
    assert mp.post_filter_batch([], fs, pf_type=pf_type) == []
    none = mp.post_filter_batch([np.zeros((0, 60))], fs, pf_type=pf_type)
    assert len(none) == 1 and none[0].shape == (0, 60)
    none = mp.post_filter_batch([torch.zeros((0, 60), device=e.device)], fs, pf_type=pf_type, return_device=True)
    assert tuple(none[0].shape) == (0, 60) and none[0].dtype == torch.float32
    # the single-matrix form
    one = mp.post_filter_device(mats[0], fs, pf_type=pf_type)
    assert np.array_equal(one, host[0])


def test_batch_options_reach_the_filters():
    e = _engine()
    x = _rows(6)
    d = e.to_device(x, np.float32)
    opts = dict(av_len_at_zero=7, av_len_at_nyq=3, boost_at_zero=1.5, boost_at_nyq=1.2)
    got = mp.post_filter_batch([x], 44100, return_device=True, **opts)[0]
    assert torch.equal(got, e.post_filter(d, 44100, **opts))
    got = mp.post_filter_batch([x], 16000, pf_type="merlin", pf_coef=1.2, return_device=True)[0]
    assert torch.equal(got, e.post_filter_merlin(d, 16000, pf_coef=1.2))


def _synth_batch(cr):
    fs, N = 16000, 1024
    rng = np.random.RandomState(40 + cr)
    utts = []
    for kind, n in (("mixed", 12), ("unvoiced", 7)):
        lf0 = cs_model.lf0_track(rng, n, kind, fs)
        a_mag, a_real, a_imag = (_f32(a) for a in cs_model.features(rng, n, 60, 10))
        utts.append((a_mag, a_real, a_imag, lf0))
    return fs, N, utts


@pytest.mark.parametrize("cr", [False, True])
@pytest.mark.parametrize("pf_type", PF_TYPES)
def test_batch_in_front_of_the_synthesis_is_the_synthesis_with_its_own_filter(pf_type, cr):
    """synthesis_from_compressed_batch(b_post_filter=...) filters its packed float32 magnitudes with the same launches
    before the unwarp: the stage in front of the unfiltered synthesis gives the same samples, bit for bit."""
    e = _engine()
    fs, N, utts = _synth_batch(cr)
    kw = dict(fft_len=N, b_const_rate=cr, noise_mode="device", noise_seeds=[21, 22], return_device=True)
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        up = [tuple(e.to_device(a, np.float32) for a in u[:3]) + (u[3],) for u in utts]
        want = mp.synthesis_from_compressed_batch(up, fs, b_post_filter=(True if pf_type == "magphase" else "merlin"), **kw)
        plain = mp.synthesis_from_compressed_batch(up, fs, b_post_filter=False, **kw)
        filt = mp.post_filter_batch([u[0] for u in up], fs, pf_type=pf_type, return_device=True)
        got = mp.synthesis_from_compressed_batch([(f,) + u[1:] for f, u in zip(filt, up)], fs, b_post_filter=False, **kw)
    for u in range(len(utts)):
        assert got[u].grad_fn is None and bool(got[u].any())
        assert torch.equal(got[u], want[u]), (pf_type, cr, u)
        assert not torch.equal(plain[u], want[u])


def _model_gradient(pf_type, fs, x32, g32):
    """(float64 model of the gradient, per-element tolerance) for packed float32 rows x32 and gradients g32."""
    if pf_type == "merlin":
        want = pfm.merlin_closed_form(x32, g32, hm.merlin_tables(x32.shape[1], fs, 1.4))
        tol = TOL_MERLIN_BWD[x32.shape[1]] * np.max(np.abs(want), axis=1, keepdims=True) * np.ones_like(want)
    else:
        m = pfm.pf_matrix(x32.shape[1], *pfm.pf_tables(x32.shape[1], fs))
        want = g32.astype(np.float64) @ m
        tol = (pfm.pf_fan_in(m) + 2)[None, :] * U24 * (np.abs(g32.astype(np.float64)) @ np.abs(m))
    return want, tol


@pytest.mark.parametrize("pf_type", PF_TYPES)
def test_batch_gradients_of_every_input_dtype(pf_type):
    """Leaves of the four dtypes, a column slice of a wider leaf, a host array and an empty utterance in one batch: every
    leaf gets a gradient in its own dtype and shape, the model's within the kernel's tolerance plus half an ulp of the
    leaf's dtype."""
    e = _engine()
    fs = 48000
    rng = np.random.RandomState(9)
    leaves = [torch.from_numpy(_rows(5 + i, seed=i)).to(e.device).to(dt).requires_grad_(True) for i, dt in enumerate(DTYPES)]
    wide = torch.from_numpy(_f32(np.concatenate((np.zeros((6, 10)), _rows(6, seed=7), np.zeros((6, 11))), axis=1))) \
        .to(e.device).requires_grad_(True)
    empty = torch.zeros((0, 60), device=e.device, requires_grad=True)
    mats = leaves + [wide[:, 10:70], _rows(4, seed=8), empty]
    outs = mp.post_filter_batch(mats, fs, pf_type=pf_type, return_device=True)
    assert all(o.grad_fn is not None for o in outs[:5])
    gws = [torch.from_numpy(_f32(rng.standard_normal(tuple(o.shape)))).to(e.device) for o in outs]
    sum((o * gw).sum() for o, gw in zip(outs, gws)).backward()
    with torch.no_grad():
        ref = mp.post_filter_batch(mats, fs, pf_type=pf_type, return_device=True)
    for o, r in zip(outs, ref):
        assert r.grad_fn is None and torch.equal(o.detach(), r)       # the same bits with and without the graph
    for k, (leaf, gw) in enumerate(zip(leaves + [wide], gws)):
        assert leaf.grad is not None and leaf.grad.dtype == leaf.dtype and leaf.grad.shape == leaf.shape
        grad = leaf.grad.to(torch.float64).cpu().numpy()
        x32 = leaf.detach().to(torch.float32).cpu().numpy()
        if leaf is wide:
            assert np.all(grad[:, :10] == 0) and np.all(grad[:, 70:] == 0)
            grad, x32 = grad[:, 10:70], x32[:, 10:70]
        want, tol = _model_gradient(pf_type, fs, x32, gw.cpu().numpy())
        tol = tol + CAST_EPS[leaf.dtype] * (np.abs(want) + tol)       # the float32 gradient rounded to the leaf's dtype
        ratio = float(np.max(np.abs(grad - want) / tol))
        print("batch gradient %s leaf %d (%s): worst error / tolerance %.3g" % (pf_type, k, leaf.dtype, ratio))
        within(ratio, 1.0, "PFA_BATCH_GRAD_%s" % pf_type.upper())
    assert empty.grad is not None and tuple(empty.grad.shape) == (0, 60)


@pytest.mark.parametrize("pf_type", PF_TYPES)
def test_batch_without_grad_has_no_graph_and_backward_runs_once(pf_type):
    e = _engine()
    leaf = torch.from_numpy(_rows(9)).to(e.device).requires_grad_(True)
    with torch.no_grad():
        assert mp.post_filter_batch([leaf], 48000, pf_type=pf_type, return_device=True)[0].grad_fn is None
    assert not isinstance(mp.post_filter_batch([leaf], 48000, pf_type=pf_type)[0], torch.Tensor)     # host result: no graph
    out = mp.post_filter_batch([leaf], 48000, pf_type=pf_type, return_device=True)[0]
    out.sum().backward()
    with pytest.raises(RuntimeError, match="second time|already been freed"):
        out.sum().backward()
    # the syntheses still refuse their own filter under grad
    fs, N, utts = _synth_batch(False)
    with pytest.raises(NotImplementedError, match="b_post_filter"):
        mp.synthesis_from_mag_batch([(torch.from_numpy(utts[0][0]).to(e.device).requires_grad_(True), utts[0][3])], fs,
                                    fft_len=N, b_post_filter=(True if pf_type == "magphase" else "merlin"),
                                    return_device=True)


@pytest.mark.parametrize("synth", ["mag", "compressed"])
@pytest.mark.parametrize("pf_type", PF_TYPES)
def test_gradient_through_filter_and_synthesis_is_the_two_step_product(pf_type, synth):
    """A waveform loss through post_filter_batch -> synthesis reaches the leaf, and equals the synthesis' gradient with
    respect to the filtered rows pushed through the filter's backward alone: the same kernels, the same bits."""
    e = _engine()
    fs, N, utts = _synth_batch(True)
    kw = dict(fft_len=N, b_const_rate=True, noise_mode="device", noise_seeds=[31, 32], return_device=True)
    rng = np.random.RandomState(77)

    def synthesize(mags):
        if synth == "mag":
            return mp.synthesis_from_mag_batch([(m, u[3]) for m, u in zip(mags, utts)], fs, **kw)
        return mp.synthesis_from_compressed_batch(
            [(m, e.to_device(u[1], np.float32), e.to_device(u[2], np.float32), u[3]) for m, u in zip(mags, utts)], fs, **kw)

    def loss(wavs, gys):
        return sum((w * gy.to(w.dtype)).sum() for w, gy in zip(wavs, gys))

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        leaves = [torch.from_numpy(u[0]).to(e.device).requires_grad_(True) for u in utts]
        wavs = synthesize(mp.post_filter_batch(leaves, fs, pf_type=pf_type, return_device=True))
        gys = [torch.from_numpy(_f32(rng.standard_normal(int(w.numel())))).to(e.device) for w in wavs]
        loss(wavs, gys).backward()
        # two steps
        with torch.no_grad():
            filt = mp.post_filter_batch([lf.detach() for lf in leaves], fs, pf_type=pf_type, return_device=True)
        mid = [f.clone().requires_grad_(True) for f in filt]
        loss(synthesize(mid), gys).backward()
        g_mid = torch.cat([m.grad for m in mid])
        x = torch.cat([lf.detach() for lf in leaves])
        two = e.post_filter_merlin_backward(x, g_mid, fs) if pf_type == "merlin" else e.post_filter_backward(g_mid, fs)
    got = torch.cat([lf.grad for lf in leaves])
    assert bool(torch.isfinite(got).all()) and bool(got.any())
    assert torch.equal(got, two), (pf_type, synth)
