"""GPU: tensor.backward() through synthesis_from_lossless_batch / synthesis_from_lossless_const_rate_batch
(magphase_amd/autograd.py, k_synth_lossless_bwd, k_rows_lerp_adjoint) against the float64 model of
tests/lossless_autograd_model.py, and the properties the feature promises: the forward's samples do not change, utterances
do not leak into one another, every input dtype and stride gets its own gradient, the result is deterministic."""
import numpy as np
import pytest
import torch

import lossless_autograd_model as model
from _tol import within
from magphase_amd import magphase as mp

pytestmark = pytest.mark.gpu

FS = 16000
# max |device - model| / max |model| per gradient matrix of a batch.  Stated at <= 3 x the worst case measured on an MI355X
# (profiles/r11_lossless_autograd_tolerances.json): 2.27e-7 / 1.54e-7 / 2.75e-7 at the variable
# rate, 1.16e-6 / 1.12e-5 / 1.07e-5 for constant-rate rows (the interpolated p = real + j imag can come out much shorter
# than its two rows, and the gradient with respect to p scales with mag / |p|: the float32 interpolation's rounding, and
# the float32 weight, weigh more there).
TOL = {"d_mag": 6.0e-7, "d_real": 4.5e-7, "d_imag": 8.0e-7, "cr_d_mag": 3.4e-6, "cr_d_real": 3.3e-5, "cr_d_imag": 3.2e-5}
NAMES = ("d_mag", "d_real", "d_imag")


def _engine():
    from magphase_amd.engine import get_engine
    return get_engine()


def _features(rng, F, H, n_zeros=10):
    """float32 [F x H] mag (log-normal), real / imag (unit circle times a factor in [0.25, 4]) with about n_zeros exact
    zeros of p = real + j imag and of mag planted (as many as the matrix has room for)."""
    mag = np.exp(rng.randn(F, H)).astype(np.float32)
    ang, rad = rng.uniform(-np.pi, np.pi, (F, H)), rng.uniform(0.25, 4.0, (F, H))
    real, imag = (rad * np.cos(ang)).astype(np.float32), (rad * np.sin(ang)).astype(np.float32)
    for _ in range(n_zeros if F else 0):
        i, k = rng.randint(F), rng.randint(H)
        real[i, k] = imag[i, k] = 0.0
        mag[rng.randint(F), rng.randint(H)] = 0.0
    if F:
        real[0, 0] = imag[0, 0] = 0.0              # ... and at the bins whose imaginary part the forward drops
        real[F - 1, H - 1] = imag[F - 1, H - 1] = 0.0
    return mag, real, imag


_BATCH = {}


def _batch(N):
    """The gradient test's batch for fft_len N, with its model gradients (computed once, never modified): three
    utterances of 2 (v_f0 = [0, 0]: 241 samples < fft_len), 37 and 70 frames, v_f0 from {0, 55, 400} Hz; for 1024 a fourth
    that starts with 30 Hz -- a first shift beyond fft_len/2, ola_plan's negative-start case: no frame reaches the few
    samples that are kept, its gradients are zero."""
    if N not in _BATCH:
        rng = np.random.RandomState(N)
        H = N // 2 + 1
        f0s = [np.zeros(2)] + [rng.choice([0.0, 55.0, 400.0], F) for F in (37, 70)]
        if N == 1024:
            f0s.append(np.r_[30.0, rng.choice([0.0, 55.0, 400.0], 8)])
        feats = [_features(rng, f0.size, H) for f0 in f0s]
        v_pms = [model.v_pm_of(f0, FS) for f0 in f0s]
        from magphase_amd import hostmath as hm
        gys = [rng.randn(hm.ola_plan(v, N)[2]).astype(np.float32) for v in v_pms]
        assert gys[0].size == 241
        ref = [model.grads_autograd(m, r, i, gy, v, N) for (m, r, i), gy, v in zip(feats, gys, v_pms)]
        for r in ref:
            for a in r:
                a.setflags(write=False)
        _BATCH[N] = (f0s, feats, gys, ref)
    return _BATCH[N]


def _leaves(feats, dev, requires_grad=(True, True, True)):
    return [tuple(torch.from_numpy(x).to(dev).requires_grad_(rg) for x, rg in zip(f, requires_grad)) for f in feats]


def _call(leaves, f0s, **kw):
    return mp.synthesis_from_lossless_batch([l + (f0, FS) for l, f0 in zip(leaves, f0s)], return_device=True, **kw)


def _dev_gys(gys, dev):
    return [torch.from_numpy(g).to(dev) for g in gys]


@pytest.mark.parametrize("N", [1024, 2048, 4096])
def test_gradients_match_the_float64_model(N):
    dev = _engine().device
    f0s, feats, gys, ref = _batch(N)
    leaves = _leaves(feats, dev)
    sigs = _call(leaves, f0s)
    assert [int(s.numel()) for s in sigs] == [g.size for g in gys]
    torch.autograd.backward(sigs, _dev_gys(gys, dev))
    for k, name in enumerate(NAMES):
        got = np.concatenate([l[k].grad.cpu().numpy() for l in leaves])
        want = np.concatenate([r[k] for r in ref])
        assert got.dtype == np.float32 and np.all(np.isfinite(got))
        err = model.rel_err(got, want)
        print("fft_len %d %s: %.4g" % (N, name, err))
        within(err, TOL[name], "autograd_lossless_%s" % name)
    if N == 1024:       # the utterance no frame of which reaches the kept samples
        assert all(not l.grad.any() for l in leaves[3])
    zero_p = (feats[2][1] == 0) & (feats[2][2] == 0)
    assert zero_p.sum() >= 2 and not leaves[2][0].grad.cpu().numpy()[zero_p].any()


def test_forward_is_unchanged_and_carries_grad_fn_only_when_asked():
    N = 2048
    dev = _engine().device
    f0s, feats, _gys, _ref = _batch(N)
    a = _call(_leaves(feats, dev), f0s)
    with torch.no_grad():
        b = _call(_leaves(feats, dev), f0s)
    c = _call(_leaves(feats, dev, (False, False, False)), f0s)
    host = mp.synthesis_from_lossless_batch([f + (f0, FS) for f, f0 in zip(feats, f0s)])
    for x, y, z, h in zip(a, b, c, host):
        assert x.grad_fn is not None and x.requires_grad and x.dtype == torch.float32
        assert y.grad_fn is None and not y.requires_grad and z.grad_fn is None and not z.requires_grad
        assert x.numel() > 0 and torch.equal(x.detach(), y) and torch.equal(y, z)
        assert isinstance(h, np.ndarray) and h.dtype == np.float64
        assert np.array_equal(x.detach().cpu().numpy().astype(np.float64), h)
    # a host return stays a detached numpy array, whatever the inputs require
    d = mp.synthesis_from_lossless_batch([l + (f0, FS) for l, f0 in zip(_leaves(feats, dev), f0s)])
    assert all(isinstance(x, np.ndarray) and np.array_equal(x, h) for x, h in zip(d, host))


def test_gradient_of_one_utterance_stays_inside_it():
    N = 1024
    dev = _engine().device
    f0s, feats, gys, _ref = _batch(N)
    leaves = _leaves(feats, dev)
    sigs = _call(leaves, f0s)
    gy = [torch.zeros_like(s) for s in sigs]
    gy[1] = torch.from_numpy(gys[1]).to(dev)
    torch.autograd.backward(sigs, gy)
    for u, l in enumerate(leaves):
        for t in l:
            assert t.grad is not None and t.grad.shape == t.shape
            assert bool(t.grad.any()) == (u == 1)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float64])
def test_dtypes_and_strides_get_their_own_gradients(dtype):
    N = 1024
    H = N // 2 + 1
    dev = _engine().device
    rng = np.random.RandomState(7)
    f0s = [rng.choice([0.0, 55.0, 400.0], F) for F in (5, 9)]
    wides = [torch.from_numpy(np.concatenate(_features(rng, f0.size, H, n_zeros=3), axis=1)).to(dev).to(dtype)
             for f0 in f0s]          # [F x 3H]; what the dtype holds is exactly representable in float32
    gys = None
    grads = {}
    for kind in ("wide", "f32"):
        if kind == "wide":
            roots = [w.clone().requires_grad_(True) for w in wides]
            leaves = [(w[:, :H], w[:, H:2 * H], w[:, 2 * H:]) for w in roots]
        else:
            leaves = [tuple(w[:, k * H:(k + 1) * H].float().contiguous().requires_grad_(True) for k in range(3))
                      for w in wides]
            roots = None
        sigs = _call(leaves, f0s)
        if gys is None:
            gys = [torch.from_numpy(rng.randn(s.numel()).astype(np.float32)).to(dev) for s in sigs]
        grads[kind + "_sig"] = [s.detach() for s in sigs]
        torch.autograd.backward(sigs, gys)
        grads[kind] = [r.grad for r in roots] if roots else [torch.cat([t.grad for t in l], dim=1) for l in leaves]
    for w, gw, g32, sw, s32 in zip(wides, grads["wide"], grads["f32"], grads["wide_sig"], grads["f32_sig"]):
        assert torch.equal(sw, s32)
        assert gw.dtype == dtype and gw.shape == w.shape and g32.dtype == torch.float32
        assert bool(g32.any()) and torch.equal(gw, g32.to(dtype))


def test_one_float32_utterance_taken_without_a_copy():
    """A batch of one float32 utterance is not packed: the kernels read the caller's rows where they lie (column slices of
    a wide tensor: row pitch 3H).  Same gradients as for the same utterance packed with a second one."""
    N = 1024
    H = N // 2 + 1
    dev = _engine().device
    rng = np.random.RandomState(9)
    f0s = [rng.choice([0.0, 55.0, 400.0], F) for F in (9, 4)]
    wide = torch.from_numpy(np.concatenate(_features(rng, 9, H, n_zeros=3), axis=1)).to(dev)
    other = _leaves([_features(rng, 4, H, n_zeros=3)], dev)[0]
    grads = []
    gy = None
    for batch_of in (1, 2):
        root = wide.clone().requires_grad_(True)
        leaves = [(root[:, :H], root[:, H:2 * H], root[:, 2 * H:])] + ([other] if batch_of == 2 else [])
        sigs = _call(leaves, f0s[:batch_of])
        if gy is None:
            gy = torch.from_numpy(rng.randn(sigs[0].numel()).astype(np.float32)).to(dev)
        torch.autograd.backward([sigs[0]], [gy])
        grads.append(root.grad)
    assert grads[0].shape == wide.shape and bool(grads[0].any()) and torch.equal(grads[0], grads[1])


def test_partial_gradients_and_determinism():
    N = 2048
    dev = _engine().device
    f0s, feats, gys, _ref = _batch(N)
    leaves = _leaves(feats, dev)
    sigs = _call(leaves, f0s)
    flat = [t for l in leaves for t in l]
    g1 = torch.autograd.grad(sigs, flat, _dev_gys(gys, dev), retain_graph=True)
    g2 = torch.autograd.grad(sigs, flat, _dev_gys(gys, dev), retain_graph=True)
    assert all(torch.equal(a, b) for a, b in zip(g1, g2)) and any(bool(a.any()) for a in g1)
    only_mag = _leaves(feats, dev, (True, False, False))
    sigs = _call(only_mag, f0s)
    torch.autograd.backward(sigs, _dev_gys(gys, dev))
    for u, l in enumerate(only_mag):
        assert l[1].grad is None and l[2].grad is None
        assert torch.equal(l[0].grad, g1[3 * u])


@pytest.mark.parametrize("rate_ms, f0_scale", [(5.0, 1.0), (7.5, 1.5)])
def test_constant_rate_gradients_match_the_float64_model(rate_ms, f0_scale):
    from magphase_amd.plans import LosslessConstRateSynthesisPlan

    N = 2048
    H = N // 2 + 1
    e = _engine()
    rng = np.random.RandomState(11)
    f0s = [f0_scale * rng.choice([0.0, 110.0, 180.0], n) for n in (1, 30, 0, 45)]      # rows at 5 ms; one without rows
    feats = [_features(rng, f0.size, H) for f0 in f0s]
    leaves = _leaves(feats, e.device)
    sigs = mp.synthesis_from_lossless_const_rate_batch([l + (f0, FS) for l, f0 in zip(leaves, f0s)],
                                                       const_rate_ms=rate_ms, return_device=True)
    assert sigs[2].numel() == 0 and all(s.grad_fn is not None for s in sigs)
    gys = [torch.from_numpy(rng.randn(s.numel()).astype(np.float32)).to(e.device) for s in sigs]
    torch.autograd.backward(sigs, gys)
    assert all(t.grad is not None and t.grad.shape == (0, H) for t in leaves[2])
    # the model, driven by the plan's own host tables
    plan = LosslessConstRateSynthesisPlan(e, f0s, [FS] * len(f0s), N, const_rate_ms=rate_ms)
    assert plan.live == [0, 1, 3]
    v_pms = plan.inner.v_pm
    frame_off = np.concatenate(([0], np.cumsum([len(v) for v in v_pms])))
    rows = [np.concatenate([f[k] for f in feats]).astype(np.float64) for k in range(3)]
    ref = model.const_rate_grads(rows, [gys[u].cpu().numpy() for u in plan.live],
                                 (plan.row0_host, plan.row1_host, plan.rowt_host), v_pms, frame_off, N)
    for k, name in enumerate(NAMES):
        got = np.concatenate([l[k].grad.cpu().numpy() for l in leaves])
        assert np.all(np.isfinite(got))
        err = model.rel_err(got, ref[k])
        print("const rate %.1f ms %s: %.4g" % (rate_ms, name, err))
        within(err, TOL["cr_" + name], "autograd_lossless_cr_%s" % name)
    with torch.no_grad():
        plain = mp.synthesis_from_lossless_const_rate_batch([l + (f0, FS) for l, f0 in zip(leaves, f0s)],
                                                            const_rate_ms=rate_ms, return_device=True)
    assert all(p.grad_fn is None and torch.equal(p, s.detach()) for p, s in zip(plain, sigs))
