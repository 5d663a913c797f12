"""GPU: la.true_envelope / true_envelope_batch / spectral_smoothing_rceps (k_true_envelope) against the reference's golden
(tests/golden/g15_true_envelope.npz) and the fp64 model (tests/true_envelope_model.py) run with the device's own pass
counts.  Errors in dB; tolerances are <= 3 x the worst case measured on the MI355X (tests/_tol.py records it)."""
import numpy as np
import pytest

import true_envelope_model as tem
from _tol import note, within
from magphase_amd import libaudio as la
from magphase_amd import synthetic as syn
from oracle import magphase_oracle as orc

pytestmark = pytest.mark.gpu

TE_GOLD_TOL = 6.7e-4    # dB, any bin, frames whose pass count equals the reference's (measured 2.6e-4)
TE_MODEL_TOL = 3e-4     # dB, any bin, against the model forced to the device's pass counts (measured 1.4e-4)
TE_SMOOTH_TOL = 7e-6    # one pass on log magnitudes (natural log units), any bin (measured 2.3e-6)
TE_ITERS_FRAC = 0.01    # fraction of frames whose pass count differs from the fp64 stop decision (measured 0)
TE_ITERS_GAP = 3        # and by how many passes at most


def _golden(golden_dir):
    return np.load(golden_dir + "/g15_true_envelope.npz")


def _to_input(m, in_type):
    return m if in_type == "abs" else (np.log(m) if in_type == "log" else 20.0 * np.log10(m))


def _to_db(y, in_type):
    with np.errstate(divide="ignore", invalid="ignore"):
        return 20.0 * np.log10(y) if in_type == "abs" else ((20.0 / np.log(10.0)) * y if in_type == "log" else y)


def _engine():
    from magphase_amd.engine import get_engine
    return get_engine()


def _max_err_db(y, ym):
    """max |dB difference| over the finite rows; the all-NaN rows (a zero magnitude) must be the same rows."""
    bad, bad_m = np.isnan(y).all(axis=1), np.isnan(ym).all(axis=1)
    np.testing.assert_array_equal(bad, bad_m)
    assert np.all(np.isfinite(y[~bad]))
    return float(np.max(np.abs(_to_db(y[~bad], "abs") - _to_db(ym[~bad], "abs")))) if np.any(~bad) else 0.0


def _mags(fs, n_utts, dur, u0=0):
    out = []
    for u in range(u0, u0 + n_utts):
        pcm, pm, voi = syn.make_utterance(u, dur_s=dur, fs=fs)
        out.append(orc.analysis_lossless_from_epochs(syn.pcm_to_float(pcm), fs, pm, voi)[0])
    return np.concatenate(out).astype(np.float32).astype(np.float64)


def test_golden_cases(golden_dir):
    g = _golden(golden_dir)
    step = int(g["step"])
    n_diff = n_all = 0
    for key in g["cases"]:
        key = str(key)
        tag, in_type, nc, thres = key.split("_")
        x = _to_input(g[tag + "_mag"].astype(np.float64), in_type)
        (y,), (it,) = la.true_envelope_batch([x], in_type=in_type, ncoeffs=int(nc), thres_db=float(thres),
                                             return_iters=True)
        ref_it = g[key + "_iters"]
        same = it == ref_it
        n_diff += int(np.sum(~same))
        n_all += it.size
        assert np.all(np.abs(it.astype(int) - ref_it) <= TE_ITERS_GAP), key
        assert y.dtype == np.float64 and y.shape == x.shape
        err = np.max(np.abs(_to_db(y, in_type)[same][:, ::step] - g[key + "_env_db"][same]))
        within(err, TE_GOLD_TOL, "TE_GOLD_TOL")
        y1 = la.true_envelope(x, in_type=in_type, ncoeffs=int(nc), thres_db=float(thres))
        np.testing.assert_array_equal(y1, y)
    note("true_envelope:golden_pass_count_differs", n_diff / n_all)
    assert n_diff / n_all <= 0.05


@pytest.mark.parametrize("fs,n_utts,dur,nc", [(8000, 3, 2.0, 60), (16000, 3, 2.0, 60), (16000, 2, 2.0, 1500),
                                              (48000, 4, 3.0, 60), (48000, 2, 3.0, 600)])
def test_many_frames_against_model_with_device_pass_counts(fs, n_utts, dur, nc):
    x = _mags(fs, n_utts, dur, u0=fs // 1000)
    (y,), (it,) = la.true_envelope_batch([x], "abs", nc, 0.1, return_iters=True)
    assert x.shape[0] >= 700
    ym, itm = tem.true_envelope(x, "abs", nc, 0.1, forced=it)
    np.testing.assert_array_equal(itm, it)
    within(_max_err_db(y, ym), TE_MODEL_TOL, "TE_MODEL_TOL")
    # the free-running fp64 stop decisions: how often the device's fp32 sum lands on the other side of thres_db
    _, it_free = tem.true_envelope(x, "abs", nc, 0.1)
    frac = float(np.mean(it_free != it))
    note("true_envelope:pass_count_differs_%d_%d" % (fs, nc), frac)
    note("true_envelope:mean_passes_%d_%d" % (fs, nc), float(it.mean()))
    assert frac <= TE_ITERS_FRAC
    assert np.max(np.abs(it_free.astype(int) - it)) <= TE_ITERS_GAP


def test_forced_passes_and_thresholds():
    x = _mags(48000, 1, 1.0, u0=3)[:200]
    e = _engine()
    forced = (np.arange(x.shape[0]) % 7 + 1).astype(np.int32)
    out, _, it = e.true_envelope([x], "abs", 60, 0.1, forced_iters=forced)
    np.testing.assert_array_equal(it.cpu().numpy(), forced)
    ym, _ = tem.true_envelope(x, "abs", 60, 0.1, forced=forced)
    y = e.to_host_f64(out[:, :x.shape[1]])
    within(_max_err_db(y, ym), TE_MODEL_TOL, "TE_MODEL_TOL")
    (_,), (it1,) = la.true_envelope_batch([x], thres_db=1e3, return_iters=True)
    assert np.all(it1 == 1)
    (_,), (it0,) = la.true_envelope_batch([x], thres_db=0.0, return_iters=True)
    assert np.all(it0 == 100)


def test_ticket_and_grid_stride_give_the_same_frames():
    import torch

    e = _engine()
    x = _mags(48000, 2, 2.0, u0=21)
    a, _, ia = e.true_envelope([x], "abs", 60, 0.1, want_iters=True, ticket=True)
    b, _, ib = e.true_envelope([x], "abs", 60, 0.1, want_iters=True, ticket=False)
    H = x.shape[1]
    assert torch.equal(ia, ib)
    assert torch.equal(torch.nan_to_num(a[:, :H], nan=-7.0), torch.nan_to_num(b[:, :H], nan=-7.0))


def test_zero_bin_row_is_nan(golden_dir):
    g = _golden(golden_dir)
    mz = g["16k_zero_mag"].astype(np.float64)
    y = la.true_envelope(mz)
    assert np.all(np.isnan(y[2]))
    assert np.all(np.isnan(g["16k_zero_env_db"][2]))
    keep = [0, 1, 3, 4, 5]
    assert np.all(np.isfinite(y[keep]))
    clean = la.true_envelope(mz[keep])
    np.testing.assert_array_equal(y[keep], clean)
    for bad in (-1.0, np.inf, np.nan):
        m2 = mz[keep].copy()
        m2[1, 17] = bad
        y2 = la.true_envelope(m2)
        assert np.all(np.isnan(y2[1]))
        np.testing.assert_array_equal(np.delete(y2, 1, axis=0), np.delete(clean, 1, axis=0))


def test_batch_is_bit_identical_to_single_calls():
    mats = [_mags(16000, 1, 0.5, u0=u) for u in (1, 2, 3)] + [_mags(16000, 1, 0.3, u0=4)[:0]]
    for in_type in ("abs", "log"):
        xs = [_to_input(m, in_type) for m in mats]
        res, its = la.true_envelope_batch(xs, in_type=in_type, ncoeffs=60, return_iters=True)
        assert len(res) == len(xs)
        for x, r, it in zip(xs, res, its):
            assert r.shape == x.shape and it.shape == (x.shape[0],)
            if x.shape[0]:
                np.testing.assert_array_equal(r, la.true_envelope(x, in_type=in_type, ncoeffs=60))


def test_device_tensors_in_and_out():
    import torch

    e = _engine()
    x = _mags(48000, 1, 0.5, u0=9)
    xd = torch.from_numpy(x.astype(np.float32)).to(e.device)
    res = la.true_envelope_batch([xd, x], return_device=True)
    assert all(torch.is_tensor(r) and r.is_cuda and r.dtype == torch.float32 for r in res)
    assert tuple(res[0].shape) == x.shape
    torch.testing.assert_close(res[0], res[1], rtol=0, atol=0)
    np.testing.assert_array_equal(res[0].cpu().numpy().astype(np.float64), la.true_envelope(x))
    res2, its = la.true_envelope_batch([xd], return_device=True, return_iters=True)
    assert torch.is_tensor(its[0]) and its[0].dtype == torch.int32


def test_spectral_smoothing_against_golden(golden_dir):
    g = _golden(golden_dir)
    lg = np.log(g["16k_mag"].astype(np.float64))
    for nc, fade in ((60, 0.2), (600, 0.7)):
        y = la.spectral_smoothing_rceps(lg, nc_total=nc, fade_to_total=fade)
        assert y.dtype == np.float64 and y.shape == lg.shape
        within(np.max(np.abs(y[:, ::4] - g["smooth_%d_%g" % (nc, fade)])), TE_SMOOTH_TOL, "TE_SMOOTH_TOL")


def test_empty_input():
    assert la.true_envelope_batch([]) == []
    y = la.true_envelope(np.zeros((0, 2049)))
    assert y.shape == (0, 2049)
    assert la.spectral_smoothing_rceps(np.zeros((0, 513))).shape == (0, 513)
