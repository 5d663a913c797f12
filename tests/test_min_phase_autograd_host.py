"""CPU: the float64 model of the minimum-phase stage and its adjoint (tests/min_phase_autograd_model.py) against the dense
matrix, the adjoint identity, closed-form rows, central differences and torch's autograd; the argument errors of
mpx_min_phase_backward, which need no GPU; and what stays refused."""
import ctypes

import numpy as np
import pytest
import torch

import min_phase_autograd_model as model
from magphase_amd import _lib


# ----------------------------------------------------------------------------------------------------------------------
# the model
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [64, 1024])
def test_T_and_its_transpose_equal_the_dense_matrix(N):
    H = N // 2 + 1
    T = model.T_dense(N)
    eye = np.eye(H)
    assert np.max(np.abs(model.T_apply(eye).T - T)) < 1e-13          # rows of T_apply(I) are the columns of T
    assert np.max(np.abs(model.Tt_apply(eye) - T)) < 1e-13           # row k of Tt_apply(I) = T^t e_k = row k of T
    assert not T[0].any() and not T[-1].any()


@pytest.mark.parametrize("N", [64, 1024, 4096])
def test_adjoint_identity(N):
    rng = np.random.RandomState(N)
    H = N // 2 + 1
    x, y = rng.randn(5, H), rng.randn(5, H)
    lhs = np.sum(model.T_apply(x) * y, axis=1)
    rhs = np.sum(x * model.Tt_apply(y), axis=1)
    assert np.max(np.abs(lhs - rhs) / np.maximum(np.abs(lhs), 1.0)) < 1e-12


@pytest.mark.parametrize("N", [64, 1024])
@pytest.mark.parametrize("q", [1, 3, 17])
def test_closed_form_cosine_rows(N, q):
    """L[k] = a cos(2 pi k q / N) gives phi[k] = -a sin(2 pi k q / N)."""
    k = np.arange(N // 2 + 1)
    a = 0.7
    phi = model.T_apply(a * np.cos(2 * np.pi * k * q / N)[None, :])[0]
    assert np.max(np.abs(phi + a * np.sin(2 * np.pi * k * q / N))) < 1e-12
    m, c, s = model.min_phase_rows(np.exp(a * np.cos(2 * np.pi * k * q / N))[None, :])
    assert np.max(np.abs(np.arctan2(s, c)[0] + a * np.sin(2 * np.pi * k * q / N))) < 1e-12


def test_chain_against_central_differences():
    N = 64
    H = N // 2 + 1
    rng = np.random.RandomState(3)
    m = np.exp(0.5 * rng.randn(2, H))
    w_m, w_a, w_b = rng.randn(2, H), rng.randn(2, H), rng.randn(2, H)
    mm, c, s = model.min_phase_rows(m)
    got = model.backward_rows(mm, c, s, w_m, w_a, w_b)
    ref = np.zeros_like(m)
    h = 1e-6
    for f in range(2):
        for k in range(H):
            d = np.zeros_like(m)
            d[f, k] = h
            ref[f, k] = (model.chain_loss(m + d, w_m, w_a, w_b) - model.chain_loss(m - d, w_m, w_a, w_b)) / (2 * h)
    assert model.rel_err_rows(got, ref) < 1e-8


@pytest.mark.parametrize("N", [64, 1024])
def test_model_against_torch_autograd(N):
    H = N // 2 + 1
    rng = np.random.RandomState(N + 1)
    m = np.exp(rng.randn(3, H))
    w = [rng.randn(3, H) for _ in range(3)]
    n_phase = 2 * H // 3
    w[1][:, n_phase:] = w[2][:, n_phase:] = 0.0
    t = torch.tensor(m, requires_grad=True)
    phi = model.T_torch(torch.log(t))
    (torch.from_numpy(w[0]) * t + torch.from_numpy(w[1]) * torch.cos(phi) + torch.from_numpy(w[2]) * torch.sin(phi)).sum().backward()
    mm, c, s = model.min_phase_rows(m)
    junk = [x.copy() for x in w]
    junk[1][:, n_phase:] = junk[2][:, n_phase:] = np.nan       # columns from n_phase on are not read
    got = model.backward_rows(mm, c, s, junk[0], junk[1], junk[2], n_phase=n_phase)
    assert model.rel_err_rows(got, t.grad.numpy()) < 1e-12
    # no phase gradient: g_m itself; a non-positive magnitude: no phase contribution at that bin
    assert np.array_equal(model.backward_rows(mm, c, s, w[0], None, None), w[0])
    m0 = m.copy()
    m0[1, 5] = 0.0
    mm, c, s = model.min_phase_rows(m0)
    got = model.backward_rows(mm, c, s, w[0], w[1], w[2])
    assert np.all(np.isfinite(got)) and got[1, 5] == w[0][1, 5]


# ----------------------------------------------------------------------------------------------------------------------
# the C entry's argument errors
# ----------------------------------------------------------------------------------------------------------------------
def _call(lib, fft_len=1024, tables=1, mag=1, real=1, imag=1, ld=None, g_m=1, g_a=1, g_b=1, ld_grad=None, n_phase=None,
          n_frames=4, out=2, ld_out=None):
    H = fft_len // 2 + 1
    p = lambda v: ctypes.c_void_p(v * 4096) if v else None        # never dereferenced: every error returns before a launch
    return lib.mpx_min_phase_backward(None, fft_len, p(tables), p(mag), p(real), p(imag), H if ld is None else ld, p(g_m),
                                      p(g_a), p(g_b), H if ld_grad is None else ld_grad, H if n_phase is None else n_phase,
                                      n_frames, p(out), H if ld_out is None else ld_out)


@pytest.mark.parametrize("kw,word", [
    (dict(fft_len=1000), b"fft_len"), (dict(fft_len=8192), b"fft_len"),
    (dict(n_frames=-1), b"negative n_frames"),
    (dict(n_phase=-1), b"n_phase"), (dict(n_phase=514), b"n_phase"),
    (dict(ld=512), b"ld <"), (dict(ld_grad=512), b"ld <"), (dict(ld_out=100), b"ld <"),
    (dict(tables=0), b"null"), (dict(mag=0), b"null"), (dict(real=0), b"null"), (dict(imag=0), b"null"),
    (dict(out=0), b"null"),
    (dict(out=1, g_m=1, ld_out=600), b"same pitch"),
])
def test_argument_errors_without_gpu(kw, word):
    lib = _lib.load()
    assert _call(lib, **kw) == -1
    msg = lib.mpx_last_error()
    assert b"mpx_min_phase_backward" in msg and word in msg, msg


def test_no_frames_is_no_launch():
    lib = _lib.load()
    assert _call(lib, n_frames=0) == 0
    assert _call(lib, n_frames=0, tables=0, mag=0, real=0, imag=0, g_m=0, g_a=0, g_b=0, out=0) == 0
    assert "mpx_min_phase_backward" in _lib.SYMBOLS


# ----------------------------------------------------------------------------------------------------------------------
# what stays refused, and what the new interface refuses, without a device
# ----------------------------------------------------------------------------------------------------------------------
def test_the_compressed_plan_still_refuses_these_phase_types():
    from magphase_amd.plans import CompressedSynthesisPlan, MagnitudeSynthesisPlan

    for ppt in ("min_phase", "linear"):
        plan = CompressedSynthesisPlan.__new__(CompressedSynthesisPlan)
        plan.per_phase_type, plan.apply_post_filter = ppt, False
        with pytest.raises(NotImplementedError, match="per_phase_type"):
            plan.check_differentiable()
        plan = MagnitudeSynthesisPlan.__new__(MagnitudeSynthesisPlan)      # its own backward pass: not refused
        plan.per_phase_type, plan.apply_post_filter, plan.mag_dim = ppt, False, 64
        plan.check_differentiable()
    plan = MagnitudeSynthesisPlan.__new__(MagnitudeSynthesisPlan)
    plan.apply_post_filter, plan.mag_dim = True, 60
    with pytest.raises(NotImplementedError, match="b_post_filter"):
        plan.check_differentiable()
    plan.apply_post_filter, plan.mag_dim = False, 65
    with pytest.raises(NotImplementedError, match="mag_dim"):
        plan.check_differentiable()


def test_bad_phase_is_a_value_error_before_any_device_work():
    from magphase_amd import magphase as mp

    x = np.zeros((4, 60))
    for bad in ("linear", "magphase", None, "Zero"):
        with pytest.raises(ValueError, match="phase"):
            mp.synthesis_from_mag_batch([(x, np.zeros(4))], 16000, phase=bad)
