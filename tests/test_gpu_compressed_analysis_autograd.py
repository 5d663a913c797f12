"""GPU: k_mel_warp_bwd on its own (Engine.mel_warp_backward) against the float64 product within a derived bound, and
tensor.backward() through analysis_compressed_batch (magphase_amd/autograd.py, CompressedAnalysisPlan.run_backward)
against the float64 model of tests/compressed_analysis_autograd_model.py, at both frame rates, with the properties the
feature promises: the forward's values do not change, device-tensor input equals host-array input, partial gradients
and repeated passes are exact, every input dtype and stride gets its own gradient, unvoiced and silent frames give zeros
and finite values, uninitialised scratch is never read, and the analysis composes with the synthesis' backward pass."""
import numpy as np
import pytest
import torch

import compressed_analysis_autograd_model as model
import lossless_autograd_model as synth_model
from _tol import within
from magphase_amd import magphase as mp
from magphase_amd.plans import CompressedAnalysisPlan

pytestmark = pytest.mark.gpu

FS = model.FS
# max |device - model| / max |model| per utterance gradient, no sample left out.  Stated at <= 3 x the worst case measured on
# an MI355X (profiles/r15_compressed_analysis_autograd_tolerances.json).  "kernel": against the
# closed form evaluated in float64 from the device's own recomputed rows, outputs, float32 tables and matrices -- only the
# float32 arithmetic of the backward kernels is left: 3.72e-7.  "e2e": against the model's float64 forward from the
# samples: 3.72e-7 (the recomputed rows are the correctly rounded float64-transform rows, so the forward adds next to
# nothing).  "compose": lossless synthesis + compressed analysis against the two float64 models chained -- the float32
# synthesis' waveform goes through the analysis' 1 / mag: 2.35e-5.
TOL = {"kernel": 1.1e-6, "e2e": 1.1e-6, "compose": 7.0e-5}


def _engine():
    from magphase_amd.engine import get_engine
    return get_engine()


# ----------------------------------------------------------------------------------------------------------------------
# the kernel alone
# ----------------------------------------------------------------------------------------------------------------------
def _padded(dev, rows, H, pad, fill=None):
    """A [rows x H] view of a buffer with row pitch H + pad, NaN everywhere (fill: the values of the view)."""
    buf = torch.full((rows, H + pad), float("nan"), dtype=torch.float32, device=dev)
    view = buf[:, :H]
    if fill is not None:
        view.copy_(torch.from_numpy(np.ascontiguousarray(fill, dtype=np.float32)))
    return buf, view


def _lerp_f32(x, tabs):
    """fma(x[row1] - x[row0], t, x[row0]) as the kernels form it in float32 (the product a * t is exact in float64)."""
    r0, r1, t = tabs
    a = (x[r1] - x[r0]).astype(np.float32)
    return (a.astype(np.float64) * t.astype(np.float64)[:, None] + x[r0].astype(np.float64)).astype(np.float32)


def _check_job(name, got, pad_cols, g, w, xt, mode, live=None):
    """Every element written, the padding untouched, and |got - ref| <= (n_out + 8) 2^-24 |d| sum_i |g_i W_ik| per element:
    n_out roundings of the sum in any order, and a few for d, the operand's interpolation and the last product."""
    got = got.cpu().numpy().astype(np.float64)
    assert np.all(np.isnan(pad_cols.cpu().numpy())), name
    assert np.all(np.isfinite(got)), name
    g64, w64, x64 = g.astype(np.float64), w.astype(np.float64), xt.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = 2.0 * x64 / (x64 * x64 + 1.0e-8) if mode == 0 else 2.0 - 2.0e-8 * np.exp(-2.0 * x64)
    ref, mass = d * (g64 @ w64), np.abs(d) * (np.abs(g64) @ np.abs(w64))
    if live is not None:
        ref[live == 0], mass[live == 0] = 0.0, 0.0
        assert not got[live == 0].any(), name
    bound = (g.shape[1] + 8) * 2.0 ** -24 * mass
    err = np.abs(got - ref)
    assert np.all(err <= bound), (name, float(np.max(err - bound)))
    frac = float(np.max(err[bound > 0] / bound[bound > 0])) if np.any(bound > 0) else 0.0
    within(frac, 1.0, "autograd_compressed_analysis_mel_warp_bwd_fraction_of_bound")
    return frac


def _kernel_case(rows, H, n_mag, n_ph, interp, which=(True, True, True), pad=7, dead_tile=False, seed=0):
    e = _engine()
    dev = e.device
    rng = np.random.RandomState(seed + 7 * rows + H + n_mag)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)   # noqa: E731
    rows_p = rows + 3 if interp else rows      # the phase jobs have their own row count
    mag = phase = None
    bufs = [None, None, None]
    views = [None, None, None]
    checks = []
    if which[0]:
        n_src = rows // 2 + 2 if interp else rows
        x = np.abs(rng.randn(n_src, H)).astype(np.float32)
        x[rng.rand(n_src, H) < 0.02] = 0.0            # exact zeros: d = 0
        x[rng.rand(n_src, H) < 0.02] *= 1.0e-5        # at the floor of the logarithm
        g = rng.randn(rows, n_mag).astype(np.float32)
        w = rng.randn(n_mag, H).astype(np.float32)
        tabs = None
        xt = x
        if interp:
            r0 = np.sort(rng.randint(0, n_src - 1, size=rows))
            r1 = r0 + 1
            r1[0] = r0[0]                             # the duplicated first row: row0 == row1
            t = rng.rand(rows).astype(np.float32)
            tabs_host = (r0, r1, t)
            xt = _lerp_f32(x, tabs_host)
            tabs = (torch.from_numpy(r0.astype(np.int32)).to(dev), torch.from_numpy(r1.astype(np.int32)).to(dev), up(t))
        _xb, xv = _padded(dev, n_src, H, pad, x)
        bufs[0], views[0] = _padded(dev, rows, H, pad)
        mag = (up(g), up(w), xv, tabs)
        checks.append(("mag", 0, g, w, xt, 0, None))
    if which[1] or which[2]:
        w = rng.randn(n_ph, H).astype(np.float32)
        live = None
        if dead_tile:
            live = (rng.rand(rows_p) < 0.7).astype(np.float32)
            live[64:128] = 0.0                        # a 64-row tile without a live row
        hs, xs = [None, None], [None, None]
        for k in (0, 1):
            if not which[1 + k]:
                continue
            x = rng.uniform(-1.0, 1.0, size=(rows_p, H)).astype(np.float32)
            h = rng.randn(rows_p, n_ph).astype(np.float32)
            if live is not None:
                h[live == 0] = 0.0                    # by construction
                x[live == 0] = np.nan                 # ... and the operand rows there are not to be used
            _xb, xs[k] = _padded(dev, rows_p, H, pad, x)
            hs[k] = up(h)
            bufs[1 + k], views[1 + k] = _padded(dev, rows_p, H, pad)
            checks.append(("real" if k == 0 else "imag", 1 + k, h, w, np.nan_to_num(x), 1, live))
        phase = (hs[0], hs[1], up(w), xs[0], xs[1], up(live) if live is not None else None)
    out = e.mel_warp_backward(H, mag=mag, phase=phase, out=tuple(views))
    torch.cuda.synchronize()
    worst = 0.0
    for name, k, g, w, xt, mode, live in checks:
        assert out[k] is views[k]
        worst = max(worst, _check_job("%s rows %d H %d" % (name, rows, H), views[k], bufs[k][:, H:], g, w, xt, mode, live))
    for k in range(3):
        assert (out[k] is None) == (not which[k])
    return worst


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("H,n_mag,n_ph", [(513, 60, 45), (1025, 64, 1), (2049, 17, 64), (513, 1, 17), (2049, 45, 60)])
def test_mel_warp_backward_kernel(rows, H, n_mag, n_ph):
    """Tile edges in the rows, a lone tail bin in every H, n_out from 1 to 64, a row pitch greater than H, the magnitude job
    with and without row tables (with: a duplicated first row), NaN around every output row."""
    for interp in (False, True):
        frac = _kernel_case(rows, H, n_mag, n_ph, interp)
        print("rows %d H %d n_out %d/%d tables %s: %.3f of the bound" % (rows, H, n_mag, n_ph, interp, frac))


@pytest.mark.parametrize("which", [(True, False, False), (False, True, False), (False, False, True), (True, False, True),
                                   (False, True, True)])
def test_mel_warp_backward_one_and_two_jobs(which):
    _kernel_case(65, 513, 60, 45, True, which=which)


def test_mel_warp_backward_tile_without_a_live_row():
    """Rows whose flag is 0 are zeros whatever their operands hold (NaN here), a whole tile of them reads nothing."""
    _kernel_case(130, 1025, 60, 45, False, dead_tile=True)
    _kernel_case(127, 513, 60, 10, True, which=(False, True, True), dead_tile=True)


def test_mel_warp_backward_refuses_and_skips():
    e = _engine()
    dev = e.device
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)   # noqa: E731
    with pytest.raises(Exception, match="1..64"):
        e.mel_warp_backward(513, mag=(z(4, 65), z(65, 513), z(4, 513), None))
    out = e.mel_warp_backward(513, mag=(z(0, 60), z(60, 513), z(0, 513), None))      # zero rows: nothing launched
    assert out[0].shape == (0, 513) and out[1] is None and out[2] is None


# ----------------------------------------------------------------------------------------------------------------------
# end to end
# ----------------------------------------------------------------------------------------------------------------------
_BATCH = {}


def _prepare(utts, N, cr, pd, ap, seed):
    """Tables, float64 model outputs, float32 upstream gradients with the tie rule applied, model gradients."""
    rng = np.random.RandomState(seed)
    wm, wp = model.warps(N, phase_dim=pd, alpha_phase=ap)
    tabs = [model.tables(pm_sec, voi, sig.size, cr) for sig, pm_sec, voi in utts]
    outs = [model.forward_numpy(u[0], t, N, wm, wp) for u, t in zip(utts, tabs)]
    grads = []
    for o, t in zip(outs, tabs):
        g = [rng.randn(*o[k].shape).astype(np.float32) for k in range(3)]
        for k, m in enumerate(model.tie_mask(o[3], o[4], t), start=1):
            g[k][m] = 0.0
        grads.append(tuple(g))
    ref = [model.grads_autograd(u[0], g, t, N, wm, wp) for u, g, t in zip(utts, grads, tabs)]
    for a in ref:
        a.setflags(write=False)
    return {"utts": utts, "tabs": tabs, "grads": grads, "ref": ref, "wm": wm, "wp": wp}


def _batch(N, cr, pd):
    """The gradient tests' batch (computed once, never modified): three utterances of 2, 37 and 70 frames."""
    key = (N, cr, pd)
    if key not in _BATCH:
        _BATCH[key] = _prepare(model.batch_utts(N), N, cr, pd, False if pd == 10 else None, N + pd)
    return _BATCH[key]


def _kw(N, cr, pd):
    return dict(fft_len=N, mag_dim=60, phase_dim=pd, b_const_rate=cr, alpha_phase=False if pd == 10 else None)


def _leaves(utts, dev, requires_grad=True):
    return [torch.from_numpy(u[0]).to(dev).requires_grad_(requires_grad) for u in utts]


def _call(sigs, utts, **kw):
    kw.setdefault("return_device", True)
    return mp.analysis_compressed_batch([(s, FS, u[1], u[2]) for s, u in zip(sigs, utts)], **kw)


def _backward(out, grads, dev, which=(True, True, True)):
    outs = [o[k] for o in out for k in range(3) if which[k]]
    gs = [torch.from_numpy(g[k]).to(dev) for g in grads for k in range(3) if which[k]]
    torch.autograd.backward(outs, gs)


def _device_rows(utts, kw):
    """The lossless rows the backward pass recomputes (the float64-transform rows of a plan of the same batch), per
    utterance, and the plan."""
    e = _engine()
    plan = CompressedAnalysisPlan(e, [(u[0], FS, u[1], u[2]) for u in utts], **kw)
    rows = [r.cpu().numpy() for r in plan.lossless.run(precise=True, rows_in_use=None)]
    fo = np.asarray(plan.lossless.frame_off)
    return [tuple(r[fo[u]:fo[u + 1]] for r in rows) for u in range(len(utts))], plan


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _compare(b, leaves, out, N, kw, label, tol_kernel="kernel", tol_e2e="e2e"):
    rows, plan = _device_rows(b["utts"], kw)
    voi_dev = plan.voi.cpu().numpy() != 0
    o_off = np.asarray(plan.out_off)
    wm32, wp32 = _f32(b["wm"]), _f32(b["wp"])
    for u, x in enumerate(leaves):
        tab = b["tabs"][u]
        assert np.array_equal(voi_dev[o_off[u]:o_off[u + 1]], tab["voi"])
        got = x.grad.cpu().numpy()
        assert got.dtype == np.float32 and got.shape == b["utts"][u][0].shape and np.all(np.isfinite(got))
        dev_out = [out[u][k].detach().cpu().numpy() for k in range(3)]
        tab32 = dict(tab, rowt=_f32(tab["rowt"]))
        closed = model.grads_closed(rows[u][0], rows[u][1], rows[u][2], dev_out[1], dev_out[2], b["grads"][u], tab32,
                                    got.size, N, wm32, wp32)
        e_k, e_e = model.rel_err(got, closed), model.rel_err(got, b["ref"][u])
        print("%s utterance %d: kernel %.4g, end to end %.4g" % (label, u, e_k, e_e))
        within(e_k, TOL[tol_kernel], "autograd_compressed_analysis_kernel")
        within(e_e, TOL[tol_e2e], "autograd_compressed_analysis_e2e")


@pytest.mark.parametrize("pd", [10, 45])
@pytest.mark.parametrize("cr", [False, True])
@pytest.mark.parametrize("N", [1024, 2048, 4096])
def test_gradients_match_the_float64_model(N, cr, pd):
    dev = _engine().device
    b = _batch(N, cr, pd)
    kw = _kw(N, cr, pd)
    leaves = _leaves(b["utts"], dev)
    out = _call(leaves, b["utts"], **kw)
    for o, t in zip(out, b["tabs"]):
        assert all(o[k].grad_fn is not None and o[k].dtype == torch.float32 for k in range(3))
        assert tuple(o[0].shape) == (t["voi"].size, 60) and tuple(o[1].shape) == tuple(o[2].shape) == (t["voi"].size, pd)
        assert isinstance(o[3], np.ndarray) and isinstance(o[4], np.ndarray)      # v_lf0_smth, v_shift: host, no grad_fn
    _backward(out, b["grads"], dev)
    _compare(b, leaves, out, N, kw, "fft_len %d const_rate %s phase_dim %d" % (N, cr, pd))


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("cr", [False, True])
def test_forward_is_unchanged_and_device_input_equals_host_input(cr, fused, monkeypatch):
    if not fused:
        monkeypatch.setenv("MAGPHASE_COMP_FUSED", "0")
    N, pd = 2048, 45
    dev = _engine().device
    utts = _batch(N, cr, pd)["utts"]
    kw = _kw(N, cr, pd)
    a = _call(_leaves(utts, dev), utts, **kw)
    with torch.no_grad():
        b = _call(_leaves(utts, dev), utts, **kw)
    c = _call(_leaves(utts, dev, False), utts, **kw)
    d = _call([u[0] for u in utts], utts, **kw)                                     # host arrays, device rows
    h = _call([u[0] for u in utts], utts, return_device=False, as_float32=True, **kw)
    s = _call([torch.stack((x, -x), dim=1).reshape(-1)[::2] for x in _leaves(utts, dev, False)], utts, **kw)   # strided
    w = _call([x.double() for x in _leaves(utts, dev, False)], utts, **kw)          # float64 of the same values
    for u in range(len(utts)):
        for k in range(3):
            x = a[u][k]
            assert x.grad_fn is not None and x.requires_grad and x.dtype == torch.float32 and x.numel() > 0
            for y in (b[u][k], c[u][k], d[u][k], s[u][k], w[u][k]):
                assert y.grad_fn is None and not y.requires_grad and torch.equal(x.detach(), y)
            assert np.array_equal(x.detach().cpu().numpy(), h[u][k])
        assert np.array_equal(a[u][3], h[u][3]) and np.array_equal(a[u][4], h[u][4])
    with pytest.raises(ValueError, match="async_out"):
        _call(_leaves(utts, dev), utts, async_out=True, as_float32=True, **kw)


@pytest.mark.parametrize("cr", [False, True])
def test_partial_gradients_and_determinism(cr):
    N, pd = 2048, 45
    dev = _engine().device
    b = _batch(N, cr, pd)
    utts, kw = b["utts"], _kw(N, cr, pd)
    leaves = _leaves(utts, dev)
    out = _call(leaves, utts, **kw)
    outs = [o[k] for o in out for k in range(3)]
    gs = [torch.from_numpy(g[k]).to(dev) for g in b["grads"] for k in range(3)]
    g1 = torch.autograd.grad(outs, leaves, gs, retain_graph=True)
    # a second forward and a second backward pass: identical bits
    leaves2 = _leaves(utts, dev)
    out2 = _call(leaves2, utts, **kw)
    g2 = torch.autograd.grad([o[k] for o in out2 for k in range(3)], leaves2, gs)
    assert all(torch.equal(x, y) for x, y in zip(g1, g2)) and all(bool(x.any()) for x in g1)
    # only m_mag_mel_log differentiated == the three-output call with zero gradients for the phase streams
    only_mag = [g if i % 3 == 0 else torch.zeros_like(g) for i, g in enumerate(gs)]
    g3 = torch.autograd.grad(outs, leaves, only_mag, retain_graph=True)
    g4 = torch.autograd.grad(outs[0::3], leaves, gs[0::3], retain_graph=True)
    assert all(torch.equal(x, y) for x, y in zip(g3, g4)) and all(bool(x.any()) for x in g4)
    # only the phase streams differentiated
    only_ph = [torch.zeros_like(g) if i % 3 == 0 else g for i, g in enumerate(gs)]
    g5 = torch.autograd.grad(outs, leaves, only_ph, retain_graph=True)
    g6 = torch.autograd.grad([o for i, o in enumerate(outs) if i % 3], leaves, [g for i, g in enumerate(gs) if i % 3])
    assert all(torch.equal(x, y) for x, y in zip(g5, g6)) and bool(g6[1].any())
    # an utterance whose v_sig does not require grad gets None, its neighbours' gradients are unchanged
    mixed = _leaves(utts, dev)
    mixed[1] = mixed[1].detach()
    out3 = _call(mixed, utts, **kw)
    torch.autograd.backward([o[k] for o in out3 for k in range(3)], gs)
    assert mixed[1].grad is None
    assert torch.equal(mixed[0].grad, g1[0]) and torch.equal(mixed[2].grad, g1[2])


@pytest.mark.parametrize("kind", ["bfloat16", "float16", "float64", "strided"])
def test_dtypes_and_strides_get_their_own_gradients(kind):
    N, pd = 1024, 10
    dev = _engine().device
    rng = np.random.RandomState(7)
    utts = [model.utterance(rng, F, model.MIX) for F in (5, 9)]
    kw = _kw(N, True, pd)
    dtype = torch.float32 if kind == "strided" else getattr(torch, kind)
    vals = [torch.from_numpy(u[0]).to(dev).to(dtype) for u in utts]     # what the dtype holds is exact in float32
    if kind == "strided":
        wide = [torch.stack((v, -v), dim=1).reshape(-1)[::2].requires_grad_(True) for v in vals]
        assert all(w.stride(0) == 2 for w in wide)
    else:
        wide = [v.clone().requires_grad_(True) for v in vals]
    f32 = [v.float().contiguous().requires_grad_(True) for v in vals]
    res, gup = {}, None
    for name, xs in (("wide", wide), ("f32", f32)):
        out = _call(xs, utts, **kw)
        if gup is None:
            gup = [tuple(torch.from_numpy(rng.randn(*o[k].shape).astype(np.float32)).to(dev) for k in range(3)) for o in out]
        res[name + "_rows"] = [o[0].detach() for o in out]
        torch.autograd.backward([o[k] for o in out for k in range(3)], [g[k] for g in gup for k in range(3)])
        res[name] = [x.grad for x in xs]
    for w, gw, g32, rw, r32 in zip(wide, res["wide"], res["f32"], res["wide_rows"], res["f32_rows"]):
        assert torch.equal(rw, r32)
        assert gw.dtype == dtype and gw.shape == w.shape and g32.dtype == torch.float32
        assert bool(g32.any()) and torch.equal(gw, g32.to(dtype))


def test_an_unvoiced_utterance_has_no_phase_gradient():
    N, pd = 1024, 45
    dev = _engine().device
    rng = np.random.RandomState(11)
    utts = [model.utterance(rng, 9, model.MIX[:2]), model.utterance(rng, 70, model.MIX[2:]),
            model.utterance(rng, 5, model.MIX[:2])]
    kw = _kw(N, False, pd)
    leaves = _leaves(utts, dev)
    out = _call(leaves, utts, **kw)
    assert not out[1][1].detach().any() and not out[1][2].detach().any() and bool(out[0][1].detach().any())
    gs = [[torch.from_numpy(rng.randn(*o[k].shape).astype(np.float32)).to(dev) for k in range(3)] for o in out]
    ph = torch.autograd.grad([o[k] for o in out for k in (1, 2)], leaves, [g[k] for g in gs for k in (1, 2)],
                             retain_graph=True)
    assert not ph[1].any() and bool(ph[0].any()) and bool(ph[2].any())      # exactly zero
    full = torch.autograd.grad([o[k] for o in out for k in range(3)], leaves, [g[k] for g in gs for k in range(3)],
                               retain_graph=True)
    mag = torch.autograd.grad([o[0] for o in out], leaves, [g[0] for g in gs])
    assert torch.equal(full[1], mag[1]) and bool(mag[1].any())


def _silent_utt(rng):
    pm_sec, voi, n = model.lossless.epochs(12, FS / 100.0, True)
    sig = model.tone_and_noise(rng, n).astype(np.float32)
    pm = np.round(pm_sec * FS).astype(int)
    sig[pm[3]:pm[7] + 1] = 0.0          # three consecutive frames of exact silence
    return sig, pm_sec, voi


@pytest.mark.parametrize("cr", [False, True])
def test_silent_frames_give_finite_gradients(cr):
    N, pd = 1024, 45
    dev = _engine().device
    rng = np.random.RandomState(13)
    utts = [model.utterance(rng, 5, model.MIX), _silent_utt(rng)]
    kw = _kw(N, cr, pd)
    b = _prepare(utts, N, cr, pd, None, 13)
    leaves = _leaves(utts, dev)
    out = _call(leaves, utts, **kw)
    rows, _plan = _device_rows(utts, kw)
    assert np.sum(~rows[1][0].any(axis=1)) == 3
    _backward(out, b["grads"], dev)
    _compare(b, leaves, out, N, kw, "silence const_rate %s" % cr)


def test_uninitialised_scratch_is_never_read(monkeypatch):
    """Constant rate, a long unvoiced stretch: the forward leaves the phase rows nobody reads unwritten.  The backward pass
    recomputes every row; with every allocation of the engine poisoned with NaN the gradient is finite, equals the model's
    and equals the unpoisoned pass bit for bit."""
    N, pd = 1024, 45
    e = _engine()
    dev = e.device
    rng = np.random.RandomState(17)
    sig, pm_sec, voi = model.utterance(rng, 9, model.MIX[:2])
    u_sig, u_pm, u_voi = model.utterance(rng, 80, model.MIX[2:])        # 80 unvoiced frames, 5 ms apart
    t_sig, t_pm, t_voi = model.utterance(rng, 9, model.MIX[:2])
    long = (np.concatenate((sig, u_sig, t_sig)),
            np.concatenate((pm_sec, sig.size / FS + u_pm, (sig.size + u_sig.size) / FS + t_pm)),
            np.concatenate((voi, u_voi, t_voi)))
    utts = [model.utterance(rng, 5, model.MIX), long]
    kw = _kw(N, True, pd)
    b = _prepare(utts, N, True, pd, None, 17)
    plan = CompressedAnalysisPlan(e, [(u[0], FS, u[1], u[2]) for u in utts], **kw)
    assert plan.rows_in_use is not None and int((plan.rows_in_use == 0).sum()) >= 64     # rows the forward does not write
    leaves = _leaves(utts, dev)
    out = _call(leaves, utts, **kw)
    _backward(out, b["grads"], dev)
    clean = [x.grad.clone() for x in leaves]
    leaves = _leaves(utts, dev)
    out = _call(leaves, utts, **kw)
    real_empty = e.empty

    def poisoned(shape, dtype=None):
        t = real_empty(shape, dtype)
        return t.fill_(float("nan")) if t.is_floating_point() else t

    monkeypatch.setattr(e, "empty", poisoned)
    _backward(out, b["grads"], dev)
    monkeypatch.undo()
    assert all(torch.equal(x.grad, c) for x, c in zip(leaves, clean))
    _compare(b, leaves, out, N, kw, "poisoned scratch")


def test_composes_with_the_synthesis_backward():
    """analysis_compressed_batch(synthesis_from_lossless_batch(feats)): backward() reaches m_mag, m_real and m_imag."""
    N, pd = 1024, 45
    dev = _engine().device
    rng = np.random.RandomState(21)
    utts = [model.utterance(rng, F, model.MIX) for F in (6, 11)]
    wm, wp = model.warps(N, phase_dim=pd)
    host = mp.analysis_lossless_batch([(u[0], FS, u[1], u[2]) for u in utts], fft_len=N)
    feats = [tuple(torch.from_numpy(f[k].astype(np.float32)).to(dev).requires_grad_(True) for k in range(3)) for f in host]
    ys = mp.synthesis_from_lossless_batch([ft + (f[3], FS) for ft, f in zip(feats, host)], return_device=True)
    assert all(y.grad_fn is not None for y in ys)
    out = _call(ys, utts, **_kw(N, False, pd))
    tabs, gup, pre = [], [], []
    for u, (y, o) in enumerate(zip(ys, out)):
        tab = model.tables(utts[u][1], utts[u][2], int(y.numel()), False)
        m = [torch.tensor(ft.detach().cpu().numpy().astype(np.float64), requires_grad=True) for ft in feats[u]]
        ym = synth_model.forward_torch(m[0], m[1], m[2], synth_model.v_pm_of(host[u][3], FS), N)
        assert ym.numel() == y.numel()
        om = model.forward_torch(ym, tab, N, wm, wp)
        g = [rng.randn(*o[k].shape).astype(np.float32) for k in range(3)]
        for k, msk in enumerate(model.tie_mask(om[3].detach().numpy(), om[4].detach().numpy(), tab), start=1):
            g[k][msk] = 0.0
        sum((om[k] * torch.from_numpy(g[k].astype(np.float64))).sum() for k in range(3)).backward()
        tabs.append(tab), gup.append(g), pre.append(m)
    torch.autograd.backward([o[k] for o in out for k in range(3)],
                            [torch.from_numpy(g[k]).to(dev) for g in gup for k in range(3)])
    for u in range(len(utts)):
        for k, name in enumerate(("m_mag", "m_real", "m_imag")):
            got = feats[u][k].grad.cpu().numpy()
            assert np.all(np.isfinite(got)) and got.any()
            err = model.rel_err(got, pre[u][k].grad.numpy())
            print("composition utterance %d %s: %.4g" % (u, name, err))
            within(err, TOL["compose"], "autograd_compressed_analysis_compose")
