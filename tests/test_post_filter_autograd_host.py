"""CPU: the references of the post-filter backward tests (tests/post_filter_autograd_model.py) against the host forms and
torch autograd in float64, hostmath's inverse tables, and what mpx_post_filter_backward, mpx_post_filter_merlin_backward
and mp.post_filter_batch refuse before anything is launched."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import output_stage_model as osm
import post_filter_autograd_model as pfm
from magphase_amd import _lib
from magphase_amd import hostmath as hm
from magphase_amd import magphase as mp

PF_CASES = [(60, 48000, {}), (61, 48000, {}), (256, 48000, {}), (60, 16000, {}), (61, 16000, {}), (256, 16000, {}),
            (5, 48000, dict(av_len_at_zero=3, av_len_at_nyq=1)),
            (12, 22050, dict(av_len_at_zero=5, av_len_at_nyq=2, boost_at_zero=1.5, boost_at_nyq=1.0))]


@pytest.mark.parametrize("dim,fs,opts", PF_CASES)
def test_matrix_is_the_host_post_filter(dim, fs, opts):
    x = np.random.RandomState(dim + fs).uniform(-8, 2, (7, dim))
    m = pfm.pf_matrix(dim, *pfm.pf_tables(dim, fs, **opts))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = mp.post_filter(x, fs, **opts)
    d = np.max(np.abs(x @ m.T - want))
    print("D %d fs %d: max |x M^T - post_filter| %.3g" % (dim, fs, d))
    assert d <= 64 * 2.0 ** -52 * 8      # a few float64 roundings of values up to 8
    assert np.array_equal(m, hm.post_filter_matrix(dim, *pfm.pf_tables(dim, fs, **opts)))


@pytest.mark.parametrize("dim,fs,opts", PF_CASES)
def test_g_times_matrix_is_autograd_of_the_restated_forward(dim, fs, opts):
    tabs = pfm.pf_tables(dim, fs, **opts)
    rng = np.random.RandomState(7 * dim + fs)
    x = torch.tensor(rng.uniform(-8, 2, (5, dim)), requires_grad=True)
    g = rng.standard_normal((5, dim))
    y = pfm.pf_forward_torch(x, *tabs)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert np.max(np.abs(y.detach().numpy() - mp.post_filter(x.detach().numpy(), fs, **opts))) <= 1e-13
    y.backward(torch.as_tensor(g))
    m = pfm.pf_matrix(dim, *tabs)
    d = np.max(np.abs(x.grad.numpy() - g @ m))
    print("D %d fs %d: max |autograd - g M| %.3g" % (dim, fs, d))
    assert d <= 1e-13


@pytest.mark.parametrize("dim,fs,opts", PF_CASES)
def test_inverse_tables_are_the_columns_of_the_matrix(dim, fs, opts):
    tabs = pfm.pf_tables(dim, fs, **opts)
    m = pfm.pf_matrix(dim, *tabs)
    cnt, idx, w, fan = hm.post_filter_backward_tables(dim, *tabs)
    assert idx.shape == w.shape == (fan, dim) and cnt.shape == (dim,) and fan == int(pfm.pf_fan_in(m).max())
    assert idx.dtype == np.int32 and cnt.dtype == np.int32
    back = np.zeros((dim, dim))
    for i in range(dim):
        assert cnt[i] == pfm.pf_fan_in(m)[i] and np.all(np.diff(idx[:cnt[i], i]) > 0)    # ascending: a fixed order
        assert np.all(w[cnt[i]:, i] == 0) and np.all((idx[:, i] >= 0) & (idx[:, i] < dim))
        back[idx[:cnt[i], i], i] = w[:cnt[i], i]
    assert np.array_equal(back, m)
    # bins 0 and D - 1 of g_y pass straight through and feed nothing else
    assert np.array_equal(m[0], np.eye(dim)[0]) and np.array_equal(m[-1], np.eye(dim)[-1])
    print("D %d fs %d: fan-in at most %d" % (dim, fs, fan))
    if not opts and fs == 48000:      # (16 kHz averages over more bins at the Nyquist end: 73 at D = 256)
        assert fan <= (16 if dim <= 61 else 66)


def test_tables_with_a_negative_half_length_are_refused():
    tabs = pfm.pf_tables(3, 48000)
    assert tabs[2].min() == -1
    with pytest.raises(ValueError, match="window"):
        hm.post_filter_backward_tables(3, *tabs)
    with pytest.raises(ValueError, match="fit"):
        hm.post_filter_matrix(60, 5, 58, np.zeros(3, np.int64), np.ones(60))


@pytest.mark.parametrize("fs", osm.MERLIN_FS)
@pytest.mark.parametrize("dim", osm.MERLIN_DIMS)
def test_merlin_closed_form_is_autograd_of_the_launch_sequence(dim, fs):
    t = hm.merlin_tables(dim, fs, 1.4)
    x = osm.merlin_input(dim)[:osm.MERLIN_UNIQUE]
    g = np.random.RandomState(dim).standard_normal(x.shape)
    xt = torch.tensor(x, requires_grad=True)
    out = pfm.merlin_forward_torch(xt, t)
    assert torch.isfinite(out).all()
    st = osm.merlin_stages(x, t, pipe=False)
    assert np.max(np.abs(out.detach().numpy() - st["out"])) <= 1e-9
    out.backward(torch.as_tensor(g))
    want = xt.grad.numpy()
    got = pfm.merlin_closed_form(x, g, t)
    assert np.all(np.isfinite(got))
    rel = np.max(np.abs(got - want), axis=1) / np.max(np.abs(want), axis=1)
    print("D %d fs %d: worst row |closed form - autograd| / max |autograd| %.3g" % (dim, fs, rel.max()))
    assert rel.max() <= 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# argument errors of the C entries: no stream, no device -- nothing may be launched
# ---------------------------------------------------------------------------------------------------------------------
def _ptr():
    buf = (ctypes.c_float * 16)()
    return buf, ctypes.addressof(buf)


def test_post_filter_backward_argument_errors():
    lib = _lib.load()
    keep, p = _ptr()
    ok = dict(g=p, F=4, D=60, cnt=p, idx=p, w=p, fan=16, out=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.mpx_post_filter_backward(None, a["g"], a["F"], a["D"], a["cnt"], a["idx"], a["w"], a["fan"], a["out"])

    for kw, word in ((dict(F=-1), b"dim"), (dict(D=2), b"dim"), (dict(D=257), b"dim"), (dict(fan=0), b"fan"),
                     (dict(fan=61), b"fan"), (dict(g=None), b"null"), (dict(cnt=None), b"null"), (dict(idx=None), b"null"),
                     (dict(w=None), b"null"), (dict(out=None), b"null")):
        assert call(**kw) == -1, kw
        err = lib.mpx_last_error()
        assert b"mpx_post_filter_backward" in err and word in err, (kw, err)
    assert call(F=0, g=None, cnt=None, idx=None, w=None, out=None) == 0
    del keep


def test_post_filter_merlin_backward_argument_errors():
    lib = _lib.load()
    keep, p = _ptr()
    names = ("x", "g_out", "c1", "lifter", "g", "wk", "cf_t", "c1_t", "mcep", "mcep_w", "g_pf", "g_c", "g_x")
    ok = dict({n: p for n in names}, F=4, D=60, nb=2049)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.mpx_post_filter_merlin_backward(None, a["x"], a["g_out"], a["F"], a["D"], a["c1"], a["lifter"], a["g"],
                                                   a["wk"], a["nb"], a["cf_t"], a["c1_t"], a["mcep"], a["mcep_w"],
                                                   a["g_pf"], a["g_c"], a["g_x"])

    for kw in (dict(F=-1), dict(D=2), dict(D=65), dict(nb=0)):
        assert call(**kw) == -1, kw
        err = lib.mpx_last_error()
        assert b"mpx_post_filter_merlin_backward" in err and b"dim" in err, (kw, err)
    for n in names:
        assert call(**{n: None}) == -1, n
        err = lib.mpx_last_error()
        assert b"mpx_post_filter_merlin_backward" in err and b"null" in err, (n, err)
    assert call(F=0, **{n: None for n in names}) == 0
    del keep


# ---------------------------------------------------------------------------------------------------------------------
# mp.post_filter_batch: everything it refuses, it refuses before it asks for an engine (there is no GPU here)
# ---------------------------------------------------------------------------------------------------------------------
def test_post_filter_batch_value_errors():
    x60, x3, x2 = np.zeros((4, 60)), np.zeros((4, 3)), np.zeros((4, 2))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for args, kw, word in (
                (([x60], 48000), dict(pf_type="no"), "pf_type"),
                (([x60], 48000), dict(pf_type=True), "pf_type"),
                ((x60, 48000), {}, "list"),
                (([x60, np.zeros((4, 59))], 48000), {}, "columns"),
                (([np.zeros(60)], 48000), {}, "2-D"),
                (([x2], 48000), {}, "3 <= D <= 256"),
                (([np.zeros((1, 257))], 48000), {}, "3 <= D <= 256"),
                (([x2], 48000), dict(pf_type="merlin"), "3 <= D <= 64"),
                (([np.zeros((1, 65))], 48000), dict(pf_type="merlin"), "3 <= D <= 64"),
                (([x60], 48000), dict(pf_type="merlin", boost_at_zero=1.5), "boost_at_zero"),
                (([x60], 48000), dict(pf_type="merlin", av_len_at_nyq=3), "av_len_at_nyq"),
                (([x60], 48000), dict(pf_coef=1.2), "pf_coef"),
                (([x60], 44100), {}, "16kHz and 48kHz"),
                (([x3], 44100), dict(av_len_at_zero=1, av_len_at_nyq=1, boost_at_zero=1.5), "16kHz and 48kHz")):
            with pytest.raises(ValueError, match=word):
                mp.post_filter_batch(*args, **kw)
    assert mp.post_filter_batch([], 48000) == [] and mp.post_filter_batch([], 48000, pf_type="merlin") == []


def test_post_filter_batch_gives_the_tables_warnings():
    def call(*args):
        try:
            mp.post_filter_batch(*args)
        except _lib.MagphaseHipError:     # no GPU here: the warnings come before the engine is asked for
            assert not torch.cuda.is_available()

    with pytest.warns(UserWarning, match="not being tunned"):
        call([np.zeros((2, 60))], 16000)
    with pytest.warns(UserWarning, match="60 dimensional"):
        call([np.zeros((2, 40))], 48000)
