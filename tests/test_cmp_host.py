"""CPU: the model of the acoustic-composition kernels (tests/cmp_model.py) against the reference's la.interp_unv_regions
(tests/golden/g18_interp_unv.npz), scipy, mlpg_model and torch float64 autograd; the moments' fixed order; Chan's merge;
every argument check of the Python entries (all raise before an engine exists) and every argument-error branch of the C
entries of magphase_cmp.hip (they return before any launch, so no device is needed)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import cmp_model as cm
import mlpg_model as mm
from magphase_amd import _lib
from magphase_amd import hostmath as hm
from magphase_amd import libaudio as la
from magphase_amd import magphase as mp


def _golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "g18_interp_unv.npz"))
    for i in range(int(g["ncases"])):
        yield (str(g["names"][i]), g["c%d_data" % i], g["c%d_voi" % i], g["c%d_out" % i], str(g["conds"][i]),
               str(g["kinds"][i]))


# ------------------------------------------------------------------------------------------------ interpolation
def test_model_equals_the_reference_golden(golden_dir):
    n = 0
    for name, data, voi, want, cond, kind in _golden(golden_dir):
        op, thr = hm.cmp_voi_cond(cond)
        prev, nxt = cm.voiced_neighbours(op(voi, thr).astype(np.float64))
        got = cm.carried(data, prev, nxt, zeros=(kind == "zeros"))
        assert got.shape == want.shape, name
        assert np.max(np.abs(got - want)) <= 1e-12, (name, cond, kind)
        n += 1
    assert n >= 12


def test_model_never_reads_an_unvoiced_entry_and_equals_scipy():
    from scipy import interpolate

    rng = np.random.default_rng(3)
    for F in (2, 3, 17, 64, 65, 300):
        m = rng.random(F) < 0.4
        m[rng.integers(F)] = True
        m[rng.integers(F)] = True
        if m.sum() < 2:
            m[:2] = True
        x = np.where(m, 5.0 + rng.normal(size=F), np.nan)
        prev, nxt = cm.voiced_neighbours(x)
        got = cm.carried(x, prev, nxt)
        assert np.all(np.isfinite(got))
        nx = np.nonzero(m)[0]
        f = interpolate.interp1d(nx, x[m], bounds_error=False, fill_value=(x[nx[0]], x[nx[-1]]), kind="linear")
        assert np.max(np.abs(got - f(np.arange(F)))) <= 1e-12
        x2 = np.where(m, x, -1e10)
        assert np.array_equal(cm.carried(x2, *cm.voiced_neighbours(x2)), got)


def test_neighbours_and_special_utterances():
    p, n = cm.voiced_neighbours(np.array([-1e10, 2.0, np.nan, 0.0, 3.0, -1.0]))
    assert p.tolist() == [-1, 1, 1, 1, 4, 4] and n.tolist() == [1, 1, 4, 4, 4, -1]
    x = np.array([np.nan, np.nan, 4.5, np.nan])
    assert cm.carried(x, *cm.voiced_neighbours(x)).tolist() == [4.5] * 4           # one voiced frame: held everywhere
    x = np.full(3, -1e10)
    assert cm.carried(x, *cm.voiced_neighbours(x), fill=-2.5).tolist() == [-2.5] * 3   # none: unv_fill
    assert cm.voiced_neighbours(np.zeros(0))[0].size == 0
    assert cm.voiced_neighbours(np.array([0.0]))[0].tolist() == [-1]               # 0 is unvoiced: '>' not '>='


def test_dynamic_features_equal_mlpg_model():
    rng = np.random.default_rng(5)
    for F in (1, 2, 3, 64, 129):
        for windows in (mm.WINDOWS, mm.WINDOWS[:1], ((0.25, -0.5, 0.75),)):
            x = rng.normal(size=(F, 3))
            y = cm.compose(x, [3], windows=windows)
            K = len(windows) + 1
            for d in range(3):
                want = mm.apply(x[:, d], None, windows)
                assert np.max(np.abs(y[:, d::3][:, :K] - want)) <= 4 * 2.0 ** -53 * max(1.0, np.max(np.abs(want)))


def test_compose_layout_is_mlpg_layouts():
    layout = (("a", 2), ("lf0", 1), ("b", 3))
    _, streams, W = hm.mlpg_layout(layout, True, 3)
    rng = np.random.default_rng(6)
    x = rng.normal(size=(9, 6))
    x[:, 2] = 5.0 + rng.random(9)
    x[[0, 4, 5, 8], 2] = -1e10
    y = cm.compose(x, [2, 1, 3], interp=1, vuv=True)
    assert y.shape == (9, W)
    for (c, d), s0 in zip(streams, (0, 2, 3)):
        if d != 1:
            assert np.array_equal(y[:, c:c + d], x[:, s0:s0 + d])
    assert np.array_equal(y[:, W - 1], (x[:, 2] > 0).astype(float))
    lf0 = y[:, streams[1][0]]
    assert np.all(np.isfinite(y)) and lf0[0] == x[1, 2] and lf0[8] == x[7, 2]
    assert abs(lf0[4] - (x[3, 2] + (x[6, 2] - x[3, 2]) / 3.0)) < 1e-14


# ------------------------------------------------------------------------------------------------ autograd
@pytest.mark.parametrize("norm", (False, True))
def test_backward_model_equals_torch_float64(norm):
    rng = np.random.default_rng(7)
    dims, F = [2, 1, 3], 41
    x = rng.normal(size=(F, 6)) + 4.0
    x[[0, 1, 7, 8, 9, 20, 39, 40], 2] = np.nan
    W = 3 * 6 + 1
    mean, std = (rng.normal(size=W), np.exp(rng.normal(size=W))) if norm else (None, None)
    xt = torch.from_numpy(x).requires_grad_(True)
    y = cm.compose_torch(xt, dims, interp=1, vuv=True, mean=mean, std=std, fill=0.5)
    want = cm.compose(x, dims, interp=1, vuv=True, mean=mean, std=std, fill=0.5)
    assert np.max(np.abs(y.detach().numpy() - want)) <= 1e-13 * np.max(np.abs(want))
    g = rng.normal(size=(F, W)).astype(np.float32)
    y.backward(torch.from_numpy(g.astype(np.float64)))
    got = cm.compose_backward(g, x, dims, interp=1, vuv=True, std=std)
    ref = xt.grad.numpy()
    assert np.all(ref[np.isnan(x)] == 0) and np.all(got[np.isnan(x)] == 0)
    assert np.max(np.abs(got - ref)) <= 1e-13 * np.max(np.abs(ref))


# ------------------------------------------------------------------------------------------------ moments
def _moments_scalar(x):
    """The device's order with scalar loops: an emulation written independently of cmp_model.column_moments."""
    total, W = x.shape
    sums, m2 = np.zeros(W), np.zeros(W)
    for c in range(W):
        for second in (False, True):
            m = sums[c] / np.float64(total)
            acc = np.float64(0.0)
            for a in range(0, total, 128):
                s = np.float64(0.0)
                for r in range(a, min(a + 128, total)):
                    v = np.float64(x[r, c])
                    s = s + ((v - m) * (v - m) if second else v)
                acc = acc + s
            if second:
                m2[c] = acc
            else:
                sums[c] = acc
    return sums, m2


@pytest.mark.parametrize("dtype", (np.float32, np.float64))
def test_moments_model(dtype):
    rng = np.random.default_rng(8)
    for total, W in ((1, 3), (127, 2), (128, 1), (129, 4), (700, 3)):
        x = (3.0 + rng.normal(size=(total, W)) * np.array([1.0, 1e-3, 50.0, 7.0])[:W]).astype(dtype)
        n, sums, m2 = cm.column_moments(x)
        assert n == total
        s2, q2 = _moments_scalar(x)
        assert np.array_equal(sums, s2) and np.array_equal(m2, q2)
        x64 = x.astype(np.float64)
        mean, std = cm.finalize(n, sums, m2)
        assert np.max(np.abs(mean - x64.mean(0)) / np.abs(x64.mean(0))) <= 1e-12
        if total > 1:
            assert np.max(np.abs(std - x64.std(0)) / x64.std(0)) <= 1e-12
        else:
            assert np.all(std == 1.0)           # zero variance -> 1


def test_chan_merge_equals_one_pass():
    rng = np.random.default_rng(9)
    x = 10.0 + rng.normal(size=(1000, 5))
    acc = (0, np.zeros(5), np.zeros(5))
    for a, b in ((0, 1), (1, 130), (130, 130), (130, 777), (777, 1000)):
        if b > a:
            acc = cm.chan_merge(acc, cm.column_moments(x[a:b]))
    mean, std = cm.finalize(*acc)
    assert np.max(np.abs(mean - x.mean(0))) <= 1e-12 * 10 and np.max(np.abs(std - x.std(0))) <= 1e-12
    x[:, 2] = 3.25
    assert cm.finalize(*cm.column_moments(x))[1][2] == 1.0


# ------------------------------------------------------------------------------------------------ argument checks
def test_voi_cond_is_parsed_not_evaluated():
    op, thr = hm.cmp_voi_cond(">0")
    assert op is np.greater and thr == 0.0
    assert hm.cmp_voi_cond(" >= 0.5")[1] == 0.5 and hm.cmp_voi_cond("==1")[0] is np.equal
    assert hm.cmp_voi_cond("<-1e-3")[1] == -1e-3 and hm.cmp_voi_cond("!=2.")[0] is np.not_equal
    for bad in ("", "0", ">", "> x", ">0; import os", "__import__('os')", ">0 and True", "=>1"):
        with pytest.raises(ValueError):
            hm.cmp_voi_cond(bad)


def _feats(F=5, dt=np.float64):
    return (np.zeros((F, 60), dt), np.zeros((F, 10), dt), np.zeros((F, 10), dt), np.ones(F, dt))


def test_python_argument_checks_raise_before_any_engine():
    f = _feats()
    bad_calls = [
        (ValueError, dict(feats=[(f[0][:, :59],) + f[1:]])),                      # a wrong width
        (ValueError, dict(feats=[f[:3] + (np.ones(4),)])),                        # mixed frame counts
        (ValueError, dict(feats=[f[:3]])),                                        # a stream missing
        (ValueError, dict(feats=f[0])),                                           # not a list
        (ValueError, dict(feats=[f[0]])),                                         # not a tuple per utterance
        (TypeError, dict(feats=[f[:3] + (np.ones(5, dtype=np.int32),)])),         # not a float dtype
        (TypeError, dict(feats=[(torch.zeros((5, 60), dtype=torch.int64),) + f[1:]])),
        (ValueError, dict(feats=[f[:3] + (np.ones(5, dtype=np.float16),)])),      # a float16 lf0
        (ValueError, dict(feats=[f[:3] + (torch.ones(5, dtype=torch.float16),)])),
        (ValueError, dict(feats=[f[:3] + (np.ones((5, 1, 1)),)])),                # not 1-D / 2-D
        (ValueError, dict(feats=[f], windows=((1.0, 2.0),))),                     # bad windows
        (ValueError, dict(feats=[f], windows=())),
        (ValueError, dict(feats=[f], windows=((0.0, np.inf, 0.0),))),
        (ValueError, dict(feats=[f], layout=(("mag", 60), ("lf0", 2)))),          # lf0 of dim 2
        (ValueError, dict(feats=[f], layout=(("mag", 60), ("mag", 10)), vuv=False)),
        (ValueError, dict(feats=[f[:1]], layout=(("mag", 60),), vuv=True)),       # vuv without lf0
        (ValueError, dict(feats=[f], layout=tuple(("s%d" % i, 1) for i in range(16)) + (("lf0", 1),))),
        (ValueError, dict(feats=[f], unv_fill=np.nan)),
        (ValueError, dict(feats=[f], unv_fill="0")),
        (ValueError, dict(feats=[f], norm=(np.zeros(244),))),
        (ValueError, dict(feats=[f], norm=(np.zeros(243), np.ones(244)))),        # a wrong length
        (ValueError, dict(feats=[f], norm=(np.zeros(244), np.zeros(244)))),       # std == 0
        (ValueError, dict(feats=[f], norm=(np.zeros(244), -np.ones(244)))),
        (ValueError, dict(feats=[f], norm=(np.zeros(244), np.full(244, np.inf)))),
        (ValueError, dict(feats=[f], norm=(np.full(244, np.nan), np.ones(244)))),
        (ValueError, dict(feats=[f], norm=(torch.zeros(244), torch.zeros(244)))),
    ]
    for exc, kw in bad_calls:
        with pytest.raises(exc):
            mp.acoustic_compose_batch(**kw)
    assert mp.acoustic_compose_batch([]) == []
    with pytest.raises(ValueError):
        mp.acoustic_compose(f[0], f[1], f[2][:, :9], f[3])
    for w in (0, -1, 2.5, True):
        with pytest.raises(ValueError):
            mp.AcousticStats(w)
    st = mp.AcousticStats(4)
    with pytest.raises(ValueError):
        st.update(np.zeros((3, 4)))
    with pytest.raises(ValueError):
        st.update([np.zeros((3, 5))])
    with pytest.raises(ValueError):
        st.finalize()
    assert st.update([]) is st and st.update([np.zeros((0, 4))]) is st


def test_interp_unv_regions_argument_checks():
    x, v = np.ones((4, 2)), np.array([1.0, 0.0, 1.0, 0.0])
    for kind in ("cubic", "quadratic", "nearest", None):
        with pytest.raises(NotImplementedError):
            la.interp_unv_regions(x, v, interp_type=kind)
    with pytest.raises(ValueError):
        la.interp_unv_regions(x, v, voi_cond="> v_voi")
    with pytest.raises(ValueError):
        la.interp_unv_regions(x, np.zeros(4))                 # no voiced row (the reference: IndexError)
    with pytest.raises(ValueError):
        la.interp_unv_regions(x, v[:3])
    with pytest.raises(ValueError):
        la.interp_unv_regions_batch([x], [v, v])
    assert la.interp_unv_regions_batch([], []) == []


# ------------------------------------------------------------------------------------------------ the C entries
def _err(lib, rc, word):
    assert rc == -1 and word in lib.mpx_last_error(), (rc, lib.mpx_last_error())


def test_c_entries_argument_errors_without_gpu():
    lib = _lib.load()
    P = ctypes.c_void_p(64)        # a non-null pointer that is never dereferenced: every call returns before a launch
    dims = (ctypes.c_int32 * 2)(3, 1)
    wins = (ctypes.c_double * 6)(-0.5, 0.0, 0.5, 1.0, -2.0, 1.0)
    bad = (ctypes.c_double * 6)(-0.5, 0.0, float("nan"), 1.0, -2.0, 1.0)

    nbf = lib.mpx_cmp_voiced_neighbours
    _err(lib, nbf(None, P, 0, 1, P, 1, -1, P), b"negative total_frames")
    _err(lib, nbf(None, P, 0, 1, P, -1, 5, P), b"negative n_utts")
    _err(lib, nbf(None, P, 0, 1, P, 1, 1 << 31, P), b"2^31")
    _err(lib, nbf(None, P, 0, 0, P, 1, 5, P), b"ld_v")
    for k in range(3):
        a = [P, P, P]
        a[k] = None
        _err(lib, nbf(None, a[0], 0, 1, a[1], 1, 5, a[2]), b"null")
    assert nbf(None, None, 0, 1, None, 1, 0, None) == 0 and nbf(None, None, 0, 1, None, 0, 5, None) == 0

    def compose(x=P, ld_x=4, d=dims, ns=2, interp=1, fill=0.0, vuv=1, nb=P, off=P, n_utts=1, total=5, n_win=2, w=wins,
                mean=None, std=None, out=P, ld_out=13):
        return lib.mpx_cmp_compose(None, x, 0, ld_x, d, ns, interp, 0, fill, vuv, nb, off, n_utts, total, n_win, w, mean,
                                   std, out, 0, ld_out)

    _err(lib, compose(d=None), b"dims")
    _err(lib, compose(ns=0), b"streams")
    _err(lib, compose(ns=17), b"streams")
    _err(lib, compose(n_win=3), b"n_win")
    _err(lib, compose(n_win=-1), b"n_win")
    _err(lib, compose(w=None), b"windows")
    _err(lib, compose(w=bad), b"not finite")
    _err(lib, compose(interp=2), b"interp_stream")
    _err(lib, compose(interp=-2), b"interp_stream")
    _err(lib, compose(interp=-1, vuv=1), b"voicing column")
    _err(lib, compose(total=-1), b"negative total_frames")
    _err(lib, compose(n_utts=-1), b"negative n_utts")
    _err(lib, compose(total=1 << 31), b"2^31")
    _err(lib, compose(d=(ctypes.c_int32 * 2)(3, 0)), b"dimension")
    _err(lib, compose(d=(ctypes.c_int32 * 2)(1 << 20, 1)), b"static columns")
    _err(lib, compose(d=(ctypes.c_int32 * 2)(1 << 19, 1), total=(1 << 31) - 1, ld_x=1 << 20, ld_out=1 << 22), b"too many")
    _err(lib, compose(ld_x=3), b"ld_x")
    _err(lib, compose(ld_out=12), b"ld_out")
    _err(lib, compose(mean=P), b"mean and std")
    _err(lib, compose(std=P), b"mean and std")
    _err(lib, compose(fill=float("inf")), b"unv_fill")
    _err(lib, compose(x=None), b"null")
    _err(lib, compose(off=None), b"null")
    _err(lib, compose(out=None), b"null")
    _err(lib, compose(nb=None), b"nb")
    assert compose(total=0, x=None, out=None, nb=None, off=None) == 0
    assert compose(n_utts=0, x=None, out=None, nb=None, off=None) == 0
    assert compose(n_win=0, w=None, total=0, ld_out=5) == 0

    def bwd(g=P, ld_g=13, d=dims, ns=2, interp=1, vuv=1, nb=P, off=P, n_utts=1, total=5, n_win=2, w=wins, std=None, gx=P,
            ld_gx=4):
        return lib.mpx_cmp_compose_backward(None, g, ld_g, d, ns, interp, vuv, nb, off, n_utts, total, n_win, w, std, gx,
                                            ld_gx)

    _err(lib, bwd(d=None), b"dims")
    _err(lib, bwd(ns=0), b"streams")
    _err(lib, bwd(n_win=3), b"n_win")
    _err(lib, bwd(w=None), b"windows")
    _err(lib, bwd(w=bad), b"not finite")
    _err(lib, bwd(interp=2), b"interp_stream")
    _err(lib, bwd(interp=-1), b"voicing column")
    _err(lib, bwd(total=-1), b"negative total_frames")
    _err(lib, bwd(n_utts=-1), b"negative n_utts")
    _err(lib, bwd(ld_g=12), b"ld_g")
    _err(lib, bwd(ld_gx=3), b"ld_gx")
    _err(lib, bwd(g=None), b"null")
    _err(lib, bwd(off=None), b"null")
    _err(lib, bwd(gx=None), b"null")
    _err(lib, bwd(nb=None), b"nb")
    assert bwd(total=0, g=None, gx=None, nb=None, off=None) == 0
    assert bwd(n_utts=0, g=None, gx=None, nb=None, off=None) == 0

    mom = lib.mpx_cmp_column_moments
    _err(lib, mom(None, P, 0, 4, 5, 0, P, P), b"width")
    _err(lib, mom(None, P, 0, 4, -1, 4, P, P), b"negative total_frames")
    _err(lib, mom(None, P, 0, 4, 1 << 31, 4, P, P), b"2^31")
    _err(lib, mom(None, P, 0, 3, 5, 4, P, P), b"ld_x")
    _err(lib, mom(None, P, 0, 1 << 40, (1 << 31) - 1, 1 << 40, P, P), b"too many")
    for k in range(3):
        a = [P, P, P]
        a[k] = None
        _err(lib, mom(None, a[0], 0, 4, 5, 4, a[1], a[2]), b"null")
    assert mom(None, None, 0, 4, 0, 4, None, None) == 0
    assert lib.mpx_cmp_moments_work_doubles(129, 3) == 6 and lib.mpx_cmp_moments_work_doubles(128, 3) == 3
    assert lib.mpx_cmp_moments_work_doubles(-1, 3) == 0 and lib.mpx_cmp_moments_work_doubles(5, 0) == 0
