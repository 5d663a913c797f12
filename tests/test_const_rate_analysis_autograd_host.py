"""CPU: the float64 model of the constant-rate lossless analysis' backward pass (tests/const_rate_analysis_autograd_model.py:
what k_analysis_lossless_bwd<P, CR = true> implements) -- its forward against the oracle, the
adjoint weights of hostmath.lerp_adjoint_table in the analysis direction against a dense matrix transpose, its closed form
against torch float64 autograd --, every argument-error branch of mpx_analysis_lossless_const_rate_backward and
hostmath.wants_grad's rule for the call.  Needs no GPU."""
import ctypes

import numpy as np
import pytest
import torch

import const_rate_analysis_autograd_model as model
from magphase_amd import _lib
from magphase_amd import hostmath as hm
from magphase_amd import synthetic as syn
from oracle import magphase_oracle as orc

TOL = 1.0e-12      # of the largest value: float64 round-off of two different orders of the same sums
FS, N = 16000, 2048


def _utt(u, dur, fs=FS):
    pcm, pm_sec, voi = syn.make_utterance(u, dur_s=dur, fs=fs)
    return syn.pcm_to_float(pcm), pm_sec, voi


@pytest.mark.parametrize("cr", [1.0, 5.0, 20.0])
def test_forward_equals_the_oracle(cr):
    sig, pm_sec, voi = _utt(1, 0.3)
    o = orc.analysis_lossless_from_epochs(sig, FS, pm_sec, voi, fft_len=N)
    ref = orc.to_const_rate(o[0], o[1], o[2], o[3], o[5], FS, cr)
    frames, tabs, f0_c = model.frames_and_tables(pm_sec, voi, sig.size, FS, cr)
    assert np.array_equal(frames[1], o[5]) and np.array_equal(f0_c, ref[3])
    got = model.forward_numpy(sig, frames, tabs, N)
    assert all(g.shape == r.shape and r.shape[0] > 0 for g, r in zip(got, ref[:3]))
    # the measure of const_rate_lossless_model.golden_rows: the magnitudes, and the spectrum mag (real + j imag), against
    # each row's peak magnitude -- a unit phasor alone is as ill-conditioned as its bin is weak (round-off of X over |X|)
    pk = np.max(ref[0], axis=1, keepdims=True)
    X, Xr = got[0] * (got[1] + 1j * got[2]), ref[0] * (ref[1] + 1j * ref[2])
    assert np.max(np.abs(got[0] - ref[0]) / pk) <= TOL and np.max(np.abs(X - Xr) / pk) <= TOL


@pytest.mark.parametrize("cr", [1.0, 5.0, 20.0])
def test_adjoint_weights_equal_the_dense_transpose(cr):
    rng = np.random.RandomState(int(cr))
    sig, pm_sec, voi = _utt(0, 0.25)
    frames, tabs, _f0 = model.frames_and_tables(pm_sec, voi, sig.size, FS, cr)
    n_var, n_c = frames[0].size, tabs[0].size
    ranges = hm.lerp_adjoint_table(tabs[0], tabs[1], tabs[2], n_var)
    assert ranges.shape == (n_var, 4) and ranges.dtype == np.int32
    A = model.lerp_matrix(tabs, n_var)
    assert np.allclose(A.sum(axis=1), 1.0, rtol=0, atol=1e-15)
    g = rng.randn(n_c, 7)
    got = model.lerp_adjoint(g, ranges, tabs[2])
    want = A.T @ g
    assert np.max(np.abs(got - want)) <= TOL * np.max(np.abs(want))
    reads = np.array([len(set(range(a0, a1)) | set(range(b0, b1))) for a0, a1, b0, b1 in ranges.tolist()])
    assert np.array_equal(reads > 0, A.any(axis=0))
    same = np.flatnonzero(tabs[0] == tabs[1])
    if cr == 1.0:
        assert reads.max() >= 10 and same.size > 0
        for c in same[:3].tolist():   # a row with row0 == row1 hands its gradient on with weight exactly 1
            hot = np.zeros((n_c, 1))
            hot[c, 0] = 0.1
            out = model.lerp_adjoint(hot, ranges, tabs[2])
            assert out[tabs[0][c], 0] == 0.1 and np.count_nonzero(out) == 1
    if cr == 20.0:
        assert np.sum(reads == 0) > 10          # frames no constant-rate row reads: a zero gradient row


@pytest.mark.parametrize("cr", [1.0, 5.0, 20.0])
@pytest.mark.parametrize("which", [(True, True, True), (True, False, False), (False, True, True)])
def test_closed_form_equals_autograd(cr, which):
    rng = np.random.RandomState(int(cr) + sum(which))
    sig, pm_sec, voi = _utt(2, 0.25)
    n_fft = 1024
    frames, tabs, _f0 = model.frames_and_tables(pm_sec, voi, sig.size, FS, cr)
    rows = model.base.forward_numpy(sig, frames[0], frames[1], frames[2], n_fft)
    grads = tuple(rng.randn(tabs[0].size, n_fft // 2 + 1) if w else None for w in which)
    want = model.grads_autograd(sig, grads, frames, tabs, n_fft)
    got = model.grads_closed(rows[0], rows[1], rows[2], grads, frames, tabs, sig.size, n_fft)
    assert np.all(np.isfinite(got)) and np.any(want != 0)
    assert model.rel_err(got, want) <= TOL, model.rel_err(got, want)


def test_an_utterance_shorter_than_one_step_has_no_rows_and_no_gradient():
    sig, pm_sec, voi = _utt(1, 0.3)
    keep = pm_sec < 0.018
    frames, tabs, f0_c = model.frames_and_tables(pm_sec[keep], voi[keep], int(0.019 * FS), FS, 20.0)
    assert tabs[0].size == 0 and f0_c.size == 0 and frames[0].size > 0
    out = model.forward_numpy(sig[:int(0.019 * FS)], frames, tabs, 1024)
    assert out[0].shape == (0, 513)
    zero = model.grads_autograd(sig[:int(0.019 * FS)], (np.zeros((0, 513)),) * 3, frames, tabs, 1024)
    assert zero.shape == (int(0.019 * FS),) and not zero.any()


def test_argument_errors_of_the_c_entry():
    lib = _lib.load()
    one = ctypes.c_void_p(8)   # a non-null pointer that is never followed: every call below returns before a launch
    name = b"mpx_analysis_lossless_const_rate_backward"

    def failed(rc, word):
        err = lib.mpx_last_error()
        assert rc == -1 and name in err and word in err, (rc, word, err)

    def call(N=1024, ld=513, ldg=513, n_c=5, n=3, sf=100, total=50, tables=one, rows=(one, one, one),
             grads=(one, one, one), rng=one, rowt=one, pos=one, left=one, right=one, soff=one, scratch=one, gsig=one):
        return lib.mpx_analysis_lossless_const_rate_backward(None, N, tables, rows[0], rows[1], rows[2], ld, grads[0],
                                                             grads[1], grads[2], ldg, n_c, rng, rowt, pos, left, right,
                                                             soff, n, scratch, sf, gsig, total)

    for bad in (1000, 512, 8192, 0):
        failed(call(N=bad), b"fft_len")
    for kw in (dict(n=-1), dict(total=-1), dict(sf=-1), dict(n_c=-1)):
        failed(call(**kw), b"negative")
    failed(call(ld=512), b"ld <")
    failed(call(ldg=512), b"ld <")
    failed(call(N=4096, ld=2049, ldg=2048), b"ld <")
    failed(call(n_c=2 ** 31), b"too many")
    for kw in (dict(tables=None), dict(rng=None), dict(rowt=None), dict(pos=None), dict(left=None), dict(right=None),
               dict(soff=None), dict(scratch=None), dict(gsig=None)):
        failed(call(**kw), b"null")
    for s in range(3):
        rows = [one, one, one]
        rows[s] = None
        failed(call(rows=tuple(rows)), b"null")
    failed(call(total=256 * 2147483647 + 1), b"too many")
    # nothing to do: no frames, or no gradient stream -- no launch, whatever else is null
    assert call(n=0, tables=None, rng=None, rowt=None, pos=None, gsig=None) == 0
    assert call(grads=(None, None, None), tables=None, rng=None, rowt=None) == 0
    assert call(scratch=None, sf=0, gsig=None, total=0, n=0) == 0


def test_wants_grad_rule_for_the_call():
    """analysis_lossless_const_rate_batch asks hostmath.wants_grad about its v_sig: only a tensor that is not on the CPU
    and requires grad, with return_device and grad mode on, takes the autograd path."""
    meta = torch.zeros(4, device="meta", requires_grad=True)     # stands for a device tensor: the rule reads no data
    cpu = torch.zeros(4, requires_grad=True)
    host = np.zeros(4, dtype=np.float32)
    assert hm.wants_grad(True, [host, meta])
    assert not hm.wants_grad(False, [host, meta])
    assert not hm.wants_grad(True, [host, cpu])
    assert not hm.wants_grad(True, [host, meta.detach()])
    with torch.no_grad():
        assert not hm.wants_grad(True, [meta])
    import inspect

    from magphase_amd import autograd, magphase
    src = inspect.getsource(magphase.analysis_lossless_const_rate_batch)
    assert "hm.wants_grad(return_device, [u[0] for u in utts])" in src and "analyze_const_rate" in src
    assert autograd._CONST_RATE.keep == ()                       # nothing is kept between the passes
