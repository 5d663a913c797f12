"""GPU: device waveforms into analysis_lossless_batch and tensor.backward() through it (magphase_amd/autograd.py,
k_analysis_lossless_bwd, k_analysis_bwd_gather) against the float64 model of tests/lossless_analysis_autograd_model.py,
and the properties the feature promises: the forward's rows do not change, utterances do not leak into one another, every
input dtype and stride gets its own gradient, partial gradients and repeated passes are exact, and the analysis composes
with the synthesis' backward pass."""
import numpy as np
import pytest
import torch

import lossless_analysis_autograd_model as model
import lossless_autograd_model as synth_model
from _tol import within
from magphase_amd import magphase as mp

pytestmark = pytest.mark.gpu

FS = model.FS
# max |device - model| / max |model| per utterance gradient, no sample left out.  Stated at <= 3 x the worst case measured on
# an MI355X (profiles/r12_analysis_autograd_tolerances.json).  "kernel": against the closed form
# evaluated in float64 from the device's own rows -- only the backward kernels' float32 arithmetic is left: 2.49e-7 (2.52e-7
# for the m_mag gradient alone).  "e2e": against the model's float64 forward from the samples -- the float32 forward's
# rounding of real / imag is divided by mag on the way back: 8.94e-5; the m_mag gradient alone does not divide: 1.49e-6.
# "roundtrip": analysis + synthesis against the two float64 models chained: 2.90e-7.
TOL = {"kernel": 7.4e-7, "e2e": 2.6e-4, "gm_kernel": 7.5e-7, "gm_e2e": 4.4e-6, "roundtrip": 8.7e-7}


def _engine():
    from magphase_amd.engine import get_engine
    return get_engine()


def _utt(rng, n_frames, spacings):
    """One utterance of n_frames epochs whose spacings are drawn from `spacings` = [(samples, voiced)], a tone plus white
    noise at -10 dB in float32."""
    pick = [spacings[i] for i in rng.randint(len(spacings), size=n_frames)]
    pm = np.cumsum([s for s, _v in pick])
    n = int(np.ceil(pm[-1] + pick[-1][0])) + 2
    return (model.tone_and_noise(rng, n).astype(np.float32), pm / FS, np.asarray([1.0 if v else 0.0 for _s, v in pick]))


MIX = [(FS / 55.0, True), (FS / 400.0, True), (0.005 * FS, False)]
_BATCH = {}


def _batch(N):
    """The gradient test's batch for fft_len N with its model gradients (computed once, never modified): three utterances
    of 2, 37 and 70 frames (55 Hz, 400 Hz and unvoiced 5 ms spacing mixed), standard normal upstream gradients."""
    if N not in _BATCH:
        rng = np.random.RandomState(N + 1)
        H = N // 2 + 1
        utts = [_utt(rng, F, MIX) for F in (2, 37, 70)]
        tabs = [model.frames_of(pm_sec, voi, sig.size)[:3] for sig, pm_sec, voi in utts]
        assert [t[0].size for t in tabs] == [2, 37, 70]
        grads = [tuple(rng.randn(t[0].size, H).astype(np.float32) for _k in range(3)) for t in tabs]
        ref = [model.grads_autograd(u[0], g, t[0], t[1], t[2], N) for u, g, t in zip(utts, grads, tabs)]
        ref_gm = [model.grads_autograd(u[0], (g[0], None, None), t[0], t[1], t[2], N) for u, g, t in zip(utts, grads, tabs)]
        for a in ref + ref_gm:
            a.setflags(write=False)
        _BATCH[N] = (utts, tabs, grads, ref, ref_gm)
    return _BATCH[N]


def _leaves(utts, dev, requires_grad=True):
    return [torch.from_numpy(u[0]).to(dev).requires_grad_(requires_grad) for u in utts]


def _call(sigs, utts, N, **kw):
    kw.setdefault("return_device", True)
    return mp.analysis_lossless_batch([(s, FS, u[1], u[2]) for s, u in zip(sigs, utts)], fft_len=N, **kw)


def _backward(out, grads, dev, which=(True, True, True)):
    outs = [o[k] for o in out for k in range(3) if which[k]]
    gs = [torch.from_numpy(g[k]).to(dev) for g in grads for k in range(3) if which[k]]
    torch.autograd.backward(outs, gs)


def _compare(leaves, out, utts, tabs, grads, ref, N, label, which=(True, True, True)):
    """Both measurements per utterance: against the closed form from the device's own rows, and against the model's
    forward from the samples."""
    for u, x in enumerate(leaves):
        got = x.grad.cpu().numpy()
        assert got.dtype == np.float32 and got.shape == utts[u][0].shape and np.all(np.isfinite(got))
        rows = [out[u][k].detach().cpu().numpy() for k in range(3)]
        g = tuple(grads[u][k] if which[k] else None for k in range(3))
        closed = model.grads_closed(rows[0], rows[1], rows[2], g, tabs[u][0], tabs[u][1], tabs[u][2], got.size, N)
        e_k, e_e = model.rel_err(got, closed), model.rel_err(got, ref[u])
        print("fft_len %d utterance %d %s: kernel %.4g, end to end %.4g" % (N, u, label or "all", e_k, e_e))
        within(e_k, TOL[label + "kernel"], "autograd_lossless_analysis_%skernel" % label)
        within(e_e, TOL[label + "e2e"], "autograd_lossless_analysis_%se2e" % label)


@pytest.mark.parametrize("N", [1024, 2048, 4096])
def test_gradients_match_the_float64_model(N):
    dev = _engine().device
    utts, tabs, grads, ref, ref_gm = _batch(N)
    leaves = _leaves(utts, dev)
    out = _call(leaves, utts, N)
    assert [int(o[0].shape[0]) for o in out] == [2, 37, 70]
    assert all(isinstance(o[3], np.ndarray) and isinstance(o[5], np.ndarray) for o in out)   # v_f0, v_shift: host, no grad_fn
    _backward(out, grads, dev)
    _compare(leaves, out, utts, tabs, grads, ref, N, "")
    leaves = _leaves(utts, dev)
    out = _call(leaves, utts, N)
    _backward(out, grads, dev, (True, False, False))
    _compare(leaves, out, utts, tabs, grads, ref_gm, N, "gm_", (True, False, False))


def _special(kind, rng):
    if kind == "long":              # 12 Hz spacing: every frame is longer than fft_len = 1024
        pm_sec, voi, n = model.epochs(4, FS / 12.0, True)
    elif kind == "silence":
        pm_sec, voi, n = model.epochs(12, FS / 100.0, True)
    else:                           # two epochs that round to the same sample
        pm_sec, voi, n = model.epochs(8, FS / 100.0, True)
        pm_sec = np.sort(np.r_[pm_sec, pm_sec[4] + 0.3 / FS])
        voi = np.ones(pm_sec.size)
    sig = model.tone_and_noise(rng, n).astype(np.float32)
    if kind == "silence":           # three consecutive frames of exact silence
        pm = np.round(pm_sec * FS).astype(int)
        sig[pm[3]:pm[7] + 1] = 0.0
    return sig, pm_sec, voi


@pytest.mark.parametrize("kind", ["long", "silence", "equal_epochs"])
def test_special_cases(kind):
    N = 1024
    dev = _engine().device
    rng = np.random.RandomState(len(kind))
    # a plain utterance in front: the special one does not start at sample 0 of the batch
    utts = [_utt(rng, 5, MIX), _special(kind, rng)]
    tabs = [model.frames_of(pm_sec, voi, sig.size)[:3] for sig, pm_sec, voi in utts]
    grads = [tuple(rng.randn(t[0].size, N // 2 + 1).astype(np.float32) for _k in range(3)) for t in tabs]
    ref = [model.grads_autograd(u[0], g, t[0], t[1], t[2], N) for u, g, t in zip(utts, grads, tabs)]
    leaves = _leaves(utts, dev)
    if kind == "long":
        assert np.all(tabs[1][1] + tabs[1][2] + 1 > N)
        with pytest.warns(UserWarning, match="fft_len"):
            out = _call(leaves, utts, N)
    else:
        out = _call(leaves, utts, N)
    if kind == "silence":
        silent = ~out[1][0].detach().cpu().numpy().any(axis=1)
        assert silent.sum() == 3 and not out[1][1].detach().cpu().numpy()[silent].any()
    if kind == "equal_epochs":
        assert np.sum(tabs[1][1] == 0) == 1 and np.sum(tabs[1][2] == 0) == 1
    _backward(out, grads, dev)
    _compare(leaves, out, utts, tabs, grads, ref, N, "")


def test_forward_is_unchanged_and_carries_grad_fn_only_when_asked():
    N = 2048
    dev = _engine().device
    utts, _tabs, _grads, _ref, _ref_gm = _batch(N)
    a = _call(_leaves(utts, dev), utts, N)
    with torch.no_grad():
        b = _call(_leaves(utts, dev), utts, N)
    c = _call(_leaves(utts, dev, False), utts, N)
    d = _call([u[0] for u in utts], utts, N)                              # host arrays, device rows
    h = _call([u[0] for u in utts], utts, N, return_device=False)         # host arrays, host rows
    e = _call(_leaves(utts, dev), utts, N, return_device=False)           # a host return stays detached numpy
    for u in range(len(utts)):
        for k in range(3):
            x = a[u][k]
            assert x.grad_fn is not None and x.requires_grad and x.dtype == torch.float32 and x.numel() > 0
            for y in (b[u][k], c[u][k], d[u][k]):
                assert y.grad_fn is None and not y.requires_grad and torch.equal(x.detach(), y)
            assert isinstance(h[u][k], np.ndarray) and h[u][k].dtype == np.float64
            assert np.array_equal(x.detach().cpu().numpy().astype(np.float64), h[u][k])
            assert isinstance(e[u][k], np.ndarray) and np.array_equal(e[u][k], h[u][k])
        for k in (3, 5):
            assert isinstance(a[u][k], np.ndarray) and np.array_equal(a[u][k], h[u][k])


def test_a_tensor_on_another_device_is_refused_and_a_cpu_tensor_is_a_host_array():
    N = 1024
    utts = _batch(N)[0]
    host = _call([u[0] for u in utts], utts, N)
    cpu = _call([torch.from_numpy(u[0]).requires_grad_(True) for u in utts], utts, N)
    assert all(c[0].grad_fn is None and torch.equal(c[0], h[0]) for c, h in zip(cpu, host))
    meta = torch.empty(utts[1][0].size, device="meta")
    with pytest.raises(ValueError, match=r"utts\[1\]"):
        _call([torch.from_numpy(utts[0][0]).to(_engine().device), meta, utts[2][0]], utts, N)
    with pytest.raises(ValueError, match=r"utts\[0\]"):
        _call([torch.zeros(utts[0][0].size, dtype=torch.int16, device=_engine().device)] + [u[0] for u in utts[1:]], utts, N)


def test_gradient_of_one_utterance_stays_inside_it():
    N = 1024
    dev = _engine().device
    utts, _tabs, grads, _ref, _ref_gm = _batch(N)
    leaves = _leaves(utts, dev)
    out = _call(leaves, utts, N)
    _backward(out[1:2], grads[1:2], dev)
    for u, x in enumerate(leaves):
        assert x.grad is not None and x.grad.shape == x.shape
        assert bool(x.grad.any()) == (u == 1)


@pytest.mark.parametrize("kind", ["bfloat16", "float16", "float64", "strided"])
def test_dtypes_and_strides_get_their_own_gradients(kind):
    N = 1024
    dev = _engine().device
    rng = np.random.RandomState(7)
    utts = [_utt(rng, F, MIX) for F in (5, 9)]
    dtype = torch.float32 if kind == "strided" else getattr(torch, kind)
    # what the dtype holds is exactly representable in float32
    vals = [torch.from_numpy(u[0]).to(dev).to(dtype) for u in utts]
    if kind == "strided":
        roots = [torch.stack((v, -v), dim=1).reshape(-1) for v in vals]      # the samples are every second element
        wide = [r[::2].requires_grad_(True) for r in roots]
        assert all(w.stride(0) == 2 for w in wide)
    else:
        wide = [v.clone().requires_grad_(True) for v in vals]
    f32 = [v.float().contiguous().requires_grad_(True) for v in vals]
    res, gup = {}, None
    for name, xs in (("wide", wide), ("f32", f32)):
        out = _call(xs, utts, N)
        if gup is None:
            gup = [tuple(torch.from_numpy(rng.randn(*o[k].shape).astype(np.float32)).to(dev) for k in range(3)) for o in out]
        res[name + "_rows"] = [o[0].detach() for o in out]
        torch.autograd.backward([o[k] for o in out for k in range(3)], [g[k] for g in gup for k in range(3)])
        res[name] = [x.grad for x in xs]
    for w, gw, g32, rw, r32 in zip(wide, res["wide"], res["f32"], res["wide_rows"], res["f32_rows"]):
        assert torch.equal(rw, r32)
        assert gw.dtype == dtype and gw.shape == w.shape and g32.dtype == torch.float32
        assert bool(g32.any()) and torch.equal(gw, g32.to(dtype))


def test_partial_gradients_and_determinism():
    N = 2048
    dev = _engine().device
    utts, _tabs, grads, _ref, _ref_gm = _batch(N)
    leaves = _leaves(utts, dev)
    out = _call(leaves, utts, N)
    outs = [o[k] for o in out for k in range(3)]
    gs = [torch.from_numpy(g[k]).to(dev) for g in grads for k in range(3)]
    g1 = torch.autograd.grad(outs, leaves, gs, retain_graph=True)
    g2 = torch.autograd.grad(outs, leaves, gs, retain_graph=True)
    assert all(torch.equal(a, b) for a, b in zip(g1, g2)) and all(bool(a.any()) for a in g1)
    # a loss on m_mag alone == the three-output call with zero gradients for m_real and m_imag
    zeroed = [g if i % 3 == 0 else torch.zeros_like(g) for i, g in enumerate(gs)]
    g3 = torch.autograd.grad(outs, leaves, zeroed, retain_graph=True)
    g4 = torch.autograd.grad(outs[0::3], leaves, gs[0::3])
    assert all(torch.equal(a, b) for a, b in zip(g3, g4)) and all(bool(a.any()) for a in g4)


def test_composes_with_the_synthesis_backward():
    """loss = sum((synthesis(analysis(x)) - target)^2): backward() reaches x through both backward passes."""
    N = 1024
    dev = _engine().device
    rng = np.random.RandomState(21)
    utts = [_utt(rng, F, MIX) for F in (6, 11)]
    tabs = [model.frames_of(pm_sec, voi, sig.size) for sig, pm_sec, voi in utts]
    leaves = _leaves(utts, dev)
    feats = _call(leaves, utts, N)
    ys = mp.synthesis_from_lossless_batch([f[:5] for f in feats], return_device=True)
    targets = [rng.randn(int(y.numel())).astype(np.float32) for y in ys]
    loss = sum(((y - torch.from_numpy(t).to(dev)) ** 2).sum() for y, t in zip(ys, targets))
    assert all(y.grad_fn is not None for y in ys)
    loss.backward()
    for u, x in enumerate(leaves):
        pm, left, right, _voi = tabs[u]
        xm = torch.tensor(utts[u][0].astype(np.float64), requires_grad=True)
        m, r, i = model.forward_torch(xm, pm, left, right, N)
        y = synth_model.forward_torch(m, r, i, synth_model.v_pm_of(feats[u][3], FS), N)
        assert y.numel() == targets[u].size
        ((y - torch.from_numpy(targets[u].astype(np.float64))) ** 2).sum().backward()
        got = x.grad.cpu().numpy()
        assert np.all(np.isfinite(got))
        err = model.rel_err(got, xm.grad.numpy())
        print("round trip utterance %d: %.4g" % (u, err))
        within(err, TOL["roundtrip"], "autograd_lossless_analysis_roundtrip")
