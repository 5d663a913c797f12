"""GPU: k_true_envelope_bwd (mpx_true_envelope_backward, Engine.true_envelope_backward) and the autograd of
la.true_envelope_batch(return_device=True).  The kernel is tested as the exact adjoint of the forward pass AS THE DEVICE
DECIDED IT: it hands its decision words to the test, and the float64 reverse recursion of
tests/true_envelope_autograd_model.py replays them -- no frame and no bin is left out of a gradient comparison.  The
decisions themselves are compared with the model's own, where a disagreement must sit at a near tie.

Tolerances are <= 3 x the worst value measured on the MI355X against the float64 model
(profiles/r18_type2_analysis_autograd_tolerance_report.json).

Rows: harmonic spectra, one row of Gaussian noise, one row with a zero bin, one frame forced to a single pass, and -- at 60
coefficients, where it never meets the stop test -- a line spectrum 120 dB above its floor that runs all 100 passes (ordinary
noise stops after about 25).  At 600 coefficients that row is a harmonic one, and another harmonic row is given 100 passes
through `iters`, so that the whole decision history is exercised there too: there the FORWARD kernel's own rounding on
the line spectrum, 3.0e-4 .. 4.7e-4 dB after 56 .. 100 passes (measured; env_out was bit-identical to k_true_envelope's
output), exceeds the forward tolerance of 3e-4 dB, which tests/test_gpu_true_envelope.py measured on speech frames of
at most some 30 passes.  That is a property of k_true_envelope on such input, not of the backward kernel, whose gradient
on the same row was within 2.2e-5 and whose decisions differed from the model's in at most two bins (largest margin
6.3e-6 dB)."""
import numpy as np
import pytest

import true_envelope_autograd_model as tam
import true_envelope_model as tem
from _tol import note, within
from magphase_amd import hostmath as hm
from magphase_amd import libaudio as la

pytestmark = pytest.mark.gpu

TE_BWD_GRAD_TOL = 6e-5         # gradient, relative to the frame's largest gradient element (measured 3.2e-5)
TE_DECISION_MARGIN_DB = 8e-6   # a decision that differs from the float64 model's lies at a margin |s - a| below this
#                                (measured 3.5e-6 dB; at most 14 of a frame's ~10^4 .. 10^5 decisions differed: the
#                                harmonic row given 100 passes, which has converged long before and sits on near ties)
TE_MODEL_TOL = 3e-4            # dB: the forward tolerance of tests/test_gpu_true_envelope.py, for env_out

SENTINEL = -77.25
MAX_IT = hm.TRUE_ENV_MAX_ITERS
ROW_ONE_PASS, ROW_NOISE, ROW_COMB, ROW_ZERO = 1, 2, 3, 4   # forced to 1 pass; noise; line spectrum (nc 60); a zero bin
ROW_FULL = 5                                     # a harmonic row given 100 passes at 600 coefficients: the whole history
FRAMES = {1024: 40, 2048: 21, 4096: 13}          # odd counts, more than one workgroup each (8, 8 and 3 waves)


def _engine():
    from magphase_amd.engine import get_engine
    return get_engine()


def _to_input(m, in_type):
    with np.errstate(divide="ignore"):
        return m if in_type == "abs" else (np.log(m) if in_type == "log" else 20.0 * np.log10(m))


def _rows(N, in_type, nc=60):
    """float32-representable input rows [F x H] (float64) and the gradient rows gy."""
    H = N // 2 + 1
    m = tam.spectra(FRAMES[N], H, N, noise_only=(ROW_NOISE,), comb=(ROW_COMB,) if nc == 60 else ())
    m[ROW_ZERO, 17] = 0.0
    x = _to_input(m, in_type).astype(np.float32).astype(np.float64)
    gy = np.random.default_rng(N + 1).normal(size=x.shape).astype(np.float32).astype(np.float64)
    return x, gy


def _launch(e, N, x, gy, iters, in_type, nc, ticket=True):
    """mpx_true_envelope_backward on rows at an odd pitch inside a sentinel-filled buffer -> (grad_in, decision words,
    env_out) as host arrays; asserts that nothing outside the [F x H] gradient rows was written."""
    import torch

    F, H = x.shape
    ld, guard = H + 5, 64
    xd = torch.from_numpy(x.astype(np.float32)).to(e.device)
    gd = torch.from_numpy(gy.astype(np.float32)).to(e.device)
    it = torch.from_numpy(np.asarray(iters, dtype=np.int32)).to(e.device)
    buf = torch.full((guard + F * ld + guard,), SENTINEL, dtype=torch.float32, device=e.device)
    gx = buf[guard:guard + F * ld].view(F, ld)
    env = torch.full((F, ld), SENTINEL, dtype=torch.float32, device=e.device)
    dec = torch.full((F, MAX_IT, (H + 31) // 32), -1, dtype=torch.int32, device=e.device)
    w = e.constant(("true_env_w", N, int(nc), 0.7), lambda: hm.true_envelope_lifter(N, nc, 0.7))
    tk = torch.empty(1, dtype=torch.int32, device=e.device) if ticket else None
    e.launch("mpx_true_envelope_backward", N, e.tables(N), w, xd, H, F, hm.TRUE_ENV_IN_TYPES.index(in_type), MAX_IT, it,
             gd, H, gx, ld, dec, env, ld, tk)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert np.all(host[:guard] == SENTINEL) and np.all(host[-guard:] == SENTINEL)
    g = host[guard:guard + F * ld].reshape(F, ld)
    assert np.all(g[:, H:] == SENTINEL) and np.all(env[:, H:].cpu().numpy() == SENTINEL)
    return g[:, :H].copy(), dec.cpu().numpy(), env[:, :H].cpu().numpy()


def _forward_iters(e, x, in_type, nc):
    """The free-running forward's passes per frame, with ROW_ONE_PASS then set to 1 and, at 600 coefficients -- where no
    row of these runs 100 passes by itself -- ROW_FULL set to 100: the backward kernel takes the pass counts as given, and
    its gradient and decisions do not depend on the stop test."""
    _, _, it = e.true_envelope([x], in_type, nc, 0.1, want_iters=True)
    it = it.cpu().numpy().copy()
    free = it.copy()
    it[ROW_ONE_PASS] = 1
    if nc != 60:
        it[ROW_FULL] = MAX_IT
    return it, free


@pytest.mark.parametrize("in_type", ["abs", "db", "log"])
@pytest.mark.parametrize("N,nc", [(1024, 60), (1024, 600), (2048, 60), (2048, 600), (4096, 60), (4096, 600)])
def test_kernel_is_the_adjoint_of_the_forward_as_the_device_decided_it(N, nc, in_type):
    e = _engine()
    x, gy = _rows(N, in_type, nc)
    F, H = x.shape
    it, free = _forward_iters(e, x, in_type, nc)
    if nc == 60:
        assert free[ROW_COMB] == MAX_IT           # the line spectrum never meets the stop test: a full decision history
    assert it[ROW_ONE_PASS] == 1 and free.max() > 1 and it.max() == MAX_IT   # a full decision history in every case
    g, words, env = _launch(e, N, x, gy, it, in_type, nc)
    ok = np.ones(F, dtype=bool)
    ok[ROW_ZERO] = False
    assert np.all(g[ROW_ZERO] == 0.0) and np.all(np.isnan(env[ROW_ZERO])) and not words[ROW_ZERO].any()
    assert np.all(np.isfinite(g))
    dec = tam.unpack_decisions(words, H)
    for f in np.flatnonzero(ok):                   # the words of the passes that decide nothing are zero
        assert not words[f, it[f] - 1:].any(), f
    # ---- the gradient against the float64 reverse recursion replaying the device's decisions: every frame, every bin
    ref = tam.envelope_grad_np(x[ok], gy[ok], in_type, nc, it[ok], dec[ok])
    err = np.max(np.abs(g[ok] - ref), axis=1) / np.max(np.abs(ref), axis=1)
    print("te_bwd grad N=%d nc=%d %s: worst %.3g (frame %d, K %d)" % (N, nc, in_type, err.max(), int(np.argmax(err)),
                                                                      int(it[ok][np.argmax(err)])))
    # ---- the decisions against the model's own
    import torch
    _, own, margin = tam.envelope_torch(torch.from_numpy(x[ok]), in_type, nc, it[ok])
    diff = dec[ok] != own
    per_frame = diff.reshape(diff.shape[0], -1).sum(axis=1)
    worst = float(margin[diff].max()) if diff.any() else 0.0
    print("te_bwd decisions N=%d nc=%d %s: %d of %d differ, per frame max %d, largest margin %.3g dB"
          % (N, nc, in_type, int(diff.sum()), int(np.isfinite(margin).sum()), int(per_frame.max()), worst))
    note("te_bwd:decisions_differ_per_frame_max_%d_%d_%s" % (N, nc, in_type), int(per_frame.max()))
    note("te_bwd:decisions_differ_fraction_%d_%d_%s" % (N, nc, in_type), float(diff.sum()) / float(np.isfinite(margin).sum()))
    # ---- env_out: the forced-pass float64 model, and the forward kernel's own rows
    ym, _ = tem.true_envelope(x[ok], in_type, nc, forced=it[ok])
    to_db = tem._TO_DB[in_type]
    env_err = np.max(np.abs(to_db(env[ok].astype(np.float64)) - to_db(ym)), axis=1)
    print("te_bwd env_out N=%d nc=%d %s: worst %.3g dB (frame %d, K %d); noise row %.3g, row %d %.3g"
          % (N, nc, in_type, env_err.max(), int(np.argmax(env_err)), int(it[ok][np.argmax(env_err)]),
             env_err[ROW_NOISE], ROW_COMB, env_err[ROW_COMB]))
    out, _, _ = e.true_envelope([x], in_type, nc, 0.1, forced_iters=it)
    same = np.array_equal(out[:, :H].cpu().numpy()[ok], env[ok])
    note("te_bwd:env_out_bit_identical_to_forward_%d_%d_%s" % (N, nc, in_type), bool(same))
    # ---- every figure is printed above; now the bounds
    within(err.max(), TE_BWD_GRAD_TOL, "TE_BWD_GRAD_TOL")
    within(worst, TE_DECISION_MARGIN_DB, "TE_DECISION_MARGIN_DB")
    within(env_err.max(), TE_MODEL_TOL, "TE_MODEL_TOL")
    assert same


@pytest.mark.parametrize("N", [1024, 2048, 4096])
def test_reproducible_and_frame_order_does_not_matter(N):
    e = _engine()
    x, gy = _rows(N, "abs")
    it, _ = _forward_iters(e, x, "abs", 60)
    a = _launch(e, N, x, gy, it, "abs", 60, ticket=True)
    b = _launch(e, N, x, gy, it, "abs", 60, ticket=True)
    c = _launch(e, N, x, gy, it, "abs", 60, ticket=False)
    for u, v in ((a, b), (a, c)):
        assert np.array_equal(u[0], v[0]) and np.array_equal(u[1], v[1])
        assert np.array_equal(np.nan_to_num(u[2], nan=-7.0), np.nan_to_num(v[2], nan=-7.0))


def test_engine_backward_equals_the_direct_launch():
    import torch

    e = _engine()
    N, nc = 2048, 600
    x, gy = _rows(N, "log", nc)
    H = x.shape[1]
    out, _, it, xin = e.true_envelope([x], "log", nc, 0.1, want_iters=True, return_input=True)
    g_ref, words, env = _launch(e, N, x, gy, it.cpu().numpy(), "log", nc)
    gd = torch.from_numpy(gy.astype(np.float32)).to(e.device)
    g = e.true_envelope_backward(xin, it, gd, H, "log", nc)
    assert np.array_equal(g[:, :H].cpu().numpy(), g_ref)
    g2, d2, env2 = e.true_envelope_backward(xin, it, gd, H, "log", nc, want_decisions=True, want_env=True, ticket=False)
    assert np.array_equal(g2[:, :H].cpu().numpy(), g_ref) and np.array_equal(d2.cpu().numpy(), words)
    assert torch.equal(torch.nan_to_num(env2[:, :H], nan=-7.0), torch.nan_to_num(out[:, :H], nan=-7.0))


def _batch_inputs(dev, dtype):
    import torch

    xa = tam.spectra(9, 1025, 5)
    xb = tam.spectra(4, 1025, 6)
    xb[2, 100] = 0.0                               # an all-NaN envelope row: zero gradient
    mk = lambda m: torch.from_numpy(m.astype(np.float32)).to(dev).to(dtype).requires_grad_(True)   # noqa: E731
    return mk(xa), mk(xb)


@pytest.mark.parametrize("dtype_name", ["float32", "bfloat16"])
def test_true_envelope_batch_carries_gradients(dtype_name):
    import torch

    e = _engine()
    dtype = getattr(torch, dtype_name)
    xa, xb = _batch_inputs(e.device, dtype)
    H = xa.shape[1]
    host = tam.spectra(3, H, 8)
    plain = la.true_envelope_batch([xa.detach(), host, xb.detach()], ncoeffs=60, return_device=True, return_iters=True)
    (ya, yh, yb), its = la.true_envelope_batch([xa, host, xb], ncoeffs=60, return_device=True, return_iters=True)
    assert ya.grad_fn is not None and yb.grad_fn is not None and not its[0].requires_grad
    for u, v in zip((ya, yh, yb) + tuple(its), plain[0] + plain[1]):     # the forward values: bit for bit
        assert torch.equal(torch.nan_to_num(u.detach(), nan=-7.0), torch.nan_to_num(v, nan=-7.0))
    assert plain[0][0].grad_fn is None
    ra = torch.from_numpy(np.random.default_rng(1).normal(size=tuple(ya.shape)).astype(np.float32)).to(e.device)
    rb = torch.from_numpy(np.random.default_rng(2).normal(size=tuple(yb.shape)).astype(np.float32)).to(e.device)
    ((ya * ra).sum() + (torch.nan_to_num(yb, nan=0.0) * rb).sum()).backward()
    assert xa.grad.dtype == dtype and xa.grad.shape == xa.shape and xb.grad.dtype == dtype
    assert bool(torch.all(xb.grad[2] == 0)) and bool(torch.isfinite(xa.grad).all()) and bool(torch.isfinite(xb.grad).all())
    # against the engine's own backward on the float32 image of the rows (the kernel itself is tested above)
    for x, r, it in ((xa, ra, its[0]), (xb, rb, its[2])):
        x32 = x.detach().to(torch.float32).contiguous()
        g = e.true_envelope_backward(x32, it.contiguous(), r, H, "abs", 60)[:, :H]
        if dtype == torch.float32:
            assert torch.equal(x.grad, g)
        else:
            assert torch.equal(x.grad, g.to(dtype))
    # no grad mode, return_device=False and host arrays: as before
    with torch.no_grad():
        assert la.true_envelope_batch([xa], ncoeffs=60, return_device=True)[0].grad_fn is None
    assert isinstance(la.true_envelope_batch([xa.detach().to(torch.float32)], ncoeffs=60)[0], np.ndarray)


def test_no_double_backward():
    import torch

    e = _engine()
    xa, _ = _batch_inputs(e.device, torch.float32)
    (ya,) = la.true_envelope_batch([xa], return_device=True)
    (g,) = torch.autograd.grad(ya.sum(), xa, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


def test_poisoned_allocator_gives_the_same_gradients(monkeypatch):
    import torch

    e = _engine()
    xa, xb = _batch_inputs(e.device, torch.float32)
    ya, yb = la.true_envelope_batch([xa, xb], ncoeffs=600, return_device=True)
    (ya.sum() + torch.nan_to_num(yb, nan=0.0).sum()).backward()
    clean = [xa.grad.clone(), xb.grad.clone()]
    xa, xb = _batch_inputs(e.device, torch.float32)
    ya, yb = la.true_envelope_batch([xa, xb], ncoeffs=600, return_device=True)
    loss = ya.sum() + torch.nan_to_num(yb, nan=0.0).sum()
    real_empty = e.empty

    def poisoned(shape, dtype=None):
        t = real_empty(shape, dtype)
        return t.fill_(float("nan")) if t.is_floating_point() else t

    monkeypatch.setattr(e, "empty", poisoned)
    loss.backward()
    monkeypatch.undo()
    assert all(bool(torch.isfinite(x.grad).all()) for x in (xa, xb))
    assert torch.equal(xa.grad, clean[0]) and torch.equal(xb.grad, clean[1])
