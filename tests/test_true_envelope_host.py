"""CPU tests of the true envelope's host side: the fp64 model (tests/true_envelope_model.py) and the cepstral helpers
against the reference's golden (tests/golden/g15_true_envelope.npz, tools/gen_golden_true_envelope.py), the weight
table against the reference's formulation, the argument checks (no device touched), the names in the src shim."""
import os
import sys

import numpy as np
import pytest

import true_envelope_model as tem
from magphase_amd import _lib, hostmath as hm
from magphase_amd import libaudio as la

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "g15_true_envelope.npz")


def _golden():
    return np.load(GOLD)


def _case(key):
    tag, in_type, nc, thres = key.split("_")
    return tag, in_type, int(nc), float(thres)


def _to_input(m, in_type):
    return m if in_type == "abs" else (np.log(m) if in_type == "log" else 20.0 * np.log10(m))


def _to_db(y, in_type):
    with np.errstate(divide="ignore", invalid="ignore"):
        return 20.0 * np.log10(y) if in_type == "abs" else ((20.0 / np.log(10.0)) * y if in_type == "log" else y)


def test_names_in_package_and_src_shim():
    sys.path.insert(0, os.path.join(ROOT, "src"))
    try:
        import libaudio as shim
    finally:
        sys.path.pop(0)
    for n in ("true_envelope", "true_envelope_batch", "spectral_smoothing_rceps", "rceps", "rceps_to_min_phase_rceps"):
        assert callable(getattr(la, n)), n
        assert getattr(shim, n) is getattr(la, n), n


def test_model_matches_golden():
    g = _golden()
    step = int(g["step"])
    for key in g["cases"]:
        tag, in_type, nc, thres = _case(str(key))
        x = _to_input(g[tag + "_mag"].astype(np.float64), in_type)
        y, iters = tem.true_envelope(x, in_type, nc, thres)
        np.testing.assert_array_equal(iters, g[key + "_iters"], err_msg=key)
        err = np.max(np.abs(_to_db(y, in_type)[:, ::step] - g[key + "_env_db"]))
        assert err < 1e-9, (key, err)


def test_model_zero_bin_row_is_nan():
    g = _golden()
    y, iters = tem.true_envelope(g["16k_zero_mag"].astype(np.float64), "abs", 60, 0.1)
    ref = g["16k_zero_env_db"]
    assert np.all(np.isnan(ref[2])) and np.all(np.isnan(y[2]))
    keep = [0, 1, 3, 4, 5]
    assert np.max(np.abs(_to_db(y, "abs")[keep, ::4] - ref[keep])) < 1e-9
    np.testing.assert_array_equal(iters, g["16k_zero_iters"])


def test_model_forced_passes_equal_free_run():
    g = _golden()
    x = g["48k_mag"].astype(np.float64)
    y, iters = tem.true_envelope(x, "abs", 60, 0.1)
    y2, iters2 = tem.true_envelope(x, "abs", 60, 0.1, forced=iters)
    np.testing.assert_array_equal(iters, iters2)
    np.testing.assert_array_equal(y, y2)


def test_model_smoothing_matches_golden():
    g = _golden()
    lg = np.log(g["16k_mag"].astype(np.float64))
    for nc, fade in ((60, 0.2), (600, 0.7)):
        y = tem.smooth(lg, hm.true_envelope_lifter(2048, nc, fade))
        assert np.max(np.abs(y[:, ::4] - g["smooth_%d_%g" % (nc, fade)])) < 1e-11


def _reference_weights(N, nc, fade):
    """libaudio.py:203-238's operations on the identity cepstrum (one row of ones), numpy's half-to-even rounding."""
    c = np.ones((1, N))
    c[:, 1:(N // 2)] *= 2
    nf = int(np.round(fade * nc))
    c[:, nc:] = 0
    c[:, nc - nf:nc] *= np.hanning(2 * nf + 3)[nf + 2:-1]
    return c[0]


@pytest.mark.parametrize("N,nc,fade", [(1024, 60, 0.7), (2048, 600, 0.7), (2048, 1500, 0.7), (4096, 60, 0.7),
                                       (4096, 4096, 0.7), (2048, 40, 0.2), (1024, 5, 0.7), (4096, 1, 0.5),
                                       (4096, 0, 0.7), (2048, 2048, 0.0)])
def test_lifter_equals_reference_weights(N, nc, fade):
    w = hm.true_envelope_lifter(N, nc, fade)
    assert w.dtype == np.float64 and w.shape == (N,)
    np.testing.assert_array_equal(w, _reference_weights(N, nc, fade))
    if nc == 0:
        assert not np.any(w)


def test_rceps_and_min_phase_rceps_equal_golden():
    g = _golden()
    m8 = g["rceps_in"]
    for in_type in ("abs", "log"):
        x = m8 if in_type == "abs" else np.log(m8 + 1e-3)
        for out_type in ("compact", "whole"):
            np.testing.assert_array_equal(la.rceps(x.copy(), in_type=in_type, out_type=out_type),
                                          g["rceps_%s_%s" % (in_type, out_type)])
    c = g["minph_in"].copy()
    out = la.rceps_to_min_phase_rceps(c)
    np.testing.assert_array_equal(out, g["minph_out"])
    np.testing.assert_array_equal(c, g["minph_in_after"])   # doubled in place, like the reference
    assert out.shape[0] == min(c.shape[0], c.shape[1] // 2 + 1)


@pytest.mark.parametrize("case", ["in_type", "nc_negative", "nc_above_N", "nc_float", "bins", "ndim", "fade"])
def test_value_errors_before_any_device_call(case, monkeypatch):
    from magphase_amd import engine

    def no_engine(*a, **k):
        raise AssertionError("device touched")

    monkeypatch.setattr(engine, "get_engine", no_engine)
    m = np.abs(np.random.RandomState(1).randn(3, 1025)) + 0.1
    kw = {}
    if case == "in_type":
        kw = {"in_type": "lin"}
    elif case == "nc_negative":
        kw = {"ncoeffs": -1}
    elif case == "nc_above_N":
        kw = {"ncoeffs": 2049}
    elif case == "nc_float":
        kw = {"ncoeffs": 60.5}
    elif case == "bins":
        m = m[:, :1000]
    elif case == "ndim":
        m = m[0]
    if case == "fade":
        with pytest.raises(ValueError):
            la.spectral_smoothing_rceps(np.log(m), nc_total=60, fade_to_total=1.5)
        return
    with pytest.raises(ValueError):
        la.true_envelope(m, **kw)
    with pytest.raises(ValueError):
        la.true_envelope_batch([m], **kw)


def test_c_abi_argument_errors():
    lib = _lib.load()
    args = [None, 4096, None, None, None, 2049, 4, 0, 0.1, 100, None, 2049, None, None, None]
    bad = list(args)
    bad[1] = 1000
    assert lib.mpx_true_envelope(*bad) == -1 and b"fft_len" in lib.mpx_last_error()
    bad = list(args)
    bad[7] = 3
    assert lib.mpx_true_envelope(*bad) == -1 and b"in_type" in lib.mpx_last_error()
    bad = list(args)
    bad[9] = 0
    assert lib.mpx_true_envelope(*bad) == -1 and b"max_iters" in lib.mpx_last_error()
    bad = list(args)
    bad[5] = 2048
    assert lib.mpx_true_envelope(*bad) == -1 and b"pitch" in lib.mpx_last_error()
    assert lib.mpx_true_envelope(*args) == -1 and b"null" in lib.mpx_last_error()
    zero = list(args)
    zero[6] = 0
    assert lib.mpx_true_envelope(*zero) == 0
