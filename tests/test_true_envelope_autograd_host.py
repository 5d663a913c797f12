"""CPU tests of the true envelope's backward pass: the float64 models of tests/true_envelope_autograd_model.py (the torch
model against tests/true_envelope_model.py and against central differences, the adjoint identity S^T = D^-1 S D, the
hand-written reverse recursion -- the specification of k_true_envelope_bwd -- against torch's autograd), the packing of
the decision words, and the argument errors of mpx_true_envelope_backward, which need no GPU."""
import ctypes

import numpy as np
import pytest
import torch

import true_envelope_autograd_model as tam
import true_envelope_model as tem
from magphase_amd import _lib
from magphase_amd import hostmath as hm

MODEL_TOL = 1e-12     # float64 models against each other, relative to the largest element of the frame
FD_MARGIN_DB = 1e-3   # central differences: only frames whose smallest decision margin exceeds this
FD_TOL = 1e-6         # relative to the frame's largest gradient element: step 1e-6, truncation ~ step^2, rounding ~ 1e-16 / step


_spectra = tam.spectra


def _rel(a, b):
    return float(np.max(np.max(np.abs(a - b), axis=1) / np.max(np.abs(b), axis=1)))


@pytest.mark.parametrize("in_type", ["abs", "db", "log"])
def test_torch_model_equals_numpy_model(in_type):
    x = _spectra(6, 513, 1)
    xin = x if in_type == "abs" else (np.log(x) if in_type == "log" else 20.0 * np.log10(x))
    y_ref, K = tem.true_envelope(xin, in_type, 60, 0.1)
    assert K.min() >= 2
    y, used, margin = tam.envelope_torch(torch.from_numpy(xin), in_type, 60, K)
    assert _rel(y.numpy(), y_ref) <= MODEL_TOL
    for f, k in enumerate(K):
        assert not used[f, k - 1:].any() and np.all(np.isinf(margin[f, k - 1:])) and np.all(np.isfinite(margin[f, :k - 1]))
    # replaying its own decisions changes nothing, in torch and in numpy
    y2, used2, _ = tam.envelope_torch(torch.from_numpy(xin), in_type, 60, K, decisions=used)
    assert _rel(y2.numpy(), y_ref) <= MODEL_TOL and np.array_equal(used, used2)
    assert _rel(tam.envelope_np(xin, in_type, 60, K, used), y_ref) <= MODEL_TOL


def test_model_gradient_against_central_differences():
    H, nc, step = 65, 12, 1e-6
    x = 20.0 * np.log10(_spectra(24, H, 7))
    K = (np.arange(x.shape[0]) % 5 + 2).astype(np.int32)
    r = np.random.default_rng(3).normal(size=x.shape)
    xt = torch.from_numpy(x).requires_grad_(True)
    y, used, margin = tam.envelope_torch(xt, "db", nc, K)
    (y * torch.from_numpy(r)).sum().backward()
    keep = np.flatnonzero(margin.reshape(x.shape[0], -1).min(axis=1) > FD_MARGIN_DB)
    assert keep.size >= 8, keep.size
    g = xt.grad.numpy()[keep]
    xk, Kk, rk = x[keep], K[keep], r[keep]
    fd = np.zeros_like(g)
    for b in range(H):
        e = np.zeros(H)
        e[b] = step
        yp = tem.true_envelope(xk + e, "db", nc, forced=Kk)[0]
        ym = tem.true_envelope(xk - e, "db", nc, forced=Kk)[0]
        fd[:, b] = ((yp - ym) * rk).sum(axis=1) / (2 * step)
    assert _rel(g, fd) <= FD_TOL


@pytest.mark.parametrize("H,nc", [(513, 60), (2049, 600), (513, 600)])
def test_smoothing_pass_is_its_own_adjoint_up_to_the_end_bins(H, nc):
    w = hm.true_envelope_lifter(2 * (H - 1), nc, 0.7)
    S = tem.smooth(np.eye(H), w).T            # column b = S e_b
    d = np.ones(H)
    d[0] = d[-1] = 2.0
    assert np.max(np.abs(S.T - (S * d[None, :]) / d[:, None])) <= MODEL_TOL * np.max(np.abs(S))
    g = np.random.default_rng(H + nc).normal(size=(3, H))
    assert _rel(tam.smooth_adjoint_np(g, w), g @ S) <= MODEL_TOL


@pytest.mark.parametrize("in_type", ["abs", "db", "log"])
@pytest.mark.parametrize("nc", [60, 600])
def test_reverse_recursion_equals_autograd(in_type, nc):
    x = _spectra(7, 513, 11 + nc, noise_only=(2,))
    xin = x if in_type == "abs" else (np.log(x) if in_type == "log" else 20.0 * np.log10(x))
    K = np.array([1, 2, 3, 5, 9, 14, 100], dtype=np.int32)
    gy = np.random.default_rng(5).normal(size=x.shape)
    xt = torch.from_numpy(xin).requires_grad_(True)
    y, used, _ = tam.envelope_torch(xt, in_type, nc, K)
    (y * torch.from_numpy(gy)).sum().backward()
    assert used[1:].any() and not used[0].any()
    assert _rel(tam.envelope_grad_np(xin, gy, in_type, nc, K, used), xt.grad.numpy()) <= MODEL_TOL
    # given decisions that are not the model's own (every one flipped): still the adjoint of that forward pass
    flipped = ~used & (np.arange(100)[None, :, None] < (K[:, None, None] - 1))
    xt2 = torch.from_numpy(xin).requires_grad_(True)
    y2, used2, _ = tam.envelope_torch(xt2, in_type, nc, K, decisions=flipped)
    (y2 * torch.from_numpy(gy)).sum().backward()
    assert np.array_equal(used2, flipped)
    assert _rel(tam.envelope_grad_np(xin, gy, in_type, nc, K, flipped), xt2.grad.numpy()) <= MODEL_TOL


@pytest.mark.parametrize("H", [513, 1025, 2049, 65])
def test_decision_words_pack_and_unpack(H):
    m = np.random.default_rng(H).random((3, 4, H)) < 0.5
    words = tam.pack_decisions(m)
    assert words.dtype == np.int32 and words.shape == (3, 4, (H + 31) // 32)
    assert np.array_equal(tam.unpack_decisions(words, H), m)
    one = np.zeros((1, 1, H), dtype=bool)
    one[0, 0, 31] = one[0, 0, 32] = one[0, 0, H - 1] = True
    w = tam.pack_decisions(one)[0, 0].view(np.uint32)
    assert w[0] == 1 << 31 and w[1] == 1 and w[-1] == 1 and int(np.count_nonzero(w)) == 3   # H - 1 is a multiple of 32


def test_c_abi_argument_errors_of_the_backward_entry():
    lib = _lib.load()
    p = ctypes.c_void_p(64)   # never dereferenced: every call below fails its checks or has no frames
    #       stream fft  tables w  in ld_in n  type max iters gy ld_gy gx ld_gx dec  env  ld_env ticket
    args = [None, 4096, p, p, p, 2049, 4, 0, 100, p, p, 2049, p, 2049, None, None, 0, None]
    fn = lib.mpx_true_envelope_backward

    def bad(i, v):
        a = list(args)
        a[i] = v
        return a

    assert fn(*bad(1, 1000)) == -1 and b"fft_len" in lib.mpx_last_error()
    for i in (5, 11, 13):
        assert fn(*bad(i, 2048)) == -1 and b"pitch" in lib.mpx_last_error()
    a = bad(15, p)   # env_out with a row pitch below H
    assert fn(*a) == -1 and b"pitch" in lib.mpx_last_error()
    assert fn(*bad(7, 3)) == -1 and b"in_type" in lib.mpx_last_error()
    assert fn(*bad(7, -1)) == -1 and b"in_type" in lib.mpx_last_error()
    assert fn(*bad(8, 0)) == -1 and b"max_iters" in lib.mpx_last_error()
    assert fn(*bad(8, 101)) == -1 and b"max_iters" in lib.mpx_last_error()
    assert fn(*bad(6, -1)) == -1 and b"n_frames" in lib.mpx_last_error()
    for i in (2, 3, 4, 9, 10, 12):   # tables, weights, in, iters, grad_out, grad_in
        assert fn(*bad(i, None)) == -1 and b"null" in lib.mpx_last_error(), i
    assert fn(*bad(6, 0)) == 0
    zero = [None if isinstance(v, ctypes.c_void_p) else v for v in bad(6, 0)]
    assert fn(*zero) == 0
    assert lib.mpx_version() == 2
