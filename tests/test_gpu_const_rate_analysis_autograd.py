"""GPU: tensor.backward() through analysis_lossless_const_rate_batch (magphase_amd/autograd.py: analyze_const_rate;
k_analysis_lossless_bwd<P, CR = true>, k_analysis_bwd_gather).  The fused backward equals the
staged one (k_rows_lerp_adjoint, then the CR = false kernel) bit for bit; both are held to the float64 model of
tests/const_rate_analysis_autograd_model.py; and the properties the feature promises: the forward's rows do not change,
utterances do not leak into one another, every input dtype and stride gets its own gradient, silence gives zeros, and the
analysis composes with the constant-rate synthesis' backward pass at the same period and at another (a time-stretch).

The metric is max |device - model| / max |model| per utterance gradient, no frame or sample left out; the figures measured
on an MI355X stand at TOL below."""
import itertools

import numpy as np
import pytest
import torch

import const_rate_analysis_autograd_model as model
import lossless_autograd_model as synth_model
from _tol import note, within
from magphase_amd import hostmath as hm
from magphase_amd import hostplan
from magphase_amd import magphase as mp
from magphase_amd import synthetic as syn
from magphase_amd.plans import LosslessConstRateAnalysisPlan

pytestmark = pytest.mark.gpu

base = model.base
RATES = [(8000, 1024), (16000, 2048), (48000, 4096)]      # P = 8, 16, 32
PERIODS = [1.0, 5.0, 20.0]
# Stated at <= 3 x the worst case measured on an MI355X against the float64 model (never against the other device form;
# profiles/r28_const_rate_analysis_autograd_tolerance_report.json; DESIGN.md section 3.3i, "Constant rate").
# "kernel": the closed form in float64 from the device's own variable-rate rows -- the backward kernels' float32
# arithmetic alone: 3.06e-7 (2.95e-7 for the m_mag gradient alone, "gm_"), at every rate.
# "e2e": the model's float64 forward from the samples, per sample rate: 4.43e-6 / 8.26e-4 / 1.13 at 8 / 16 / 48 kHz
# (m_mag alone: 1.38e-6 / 1.92e-4 / 1.86e-2).  The figures at 16 and 48 kHz are the inputs', not this arm's: most bins of
# these synthetic utterances (pulse trains through resonators below 2.6 kHz, 16-bit) lie 60 dB and more under the frame's
# peak, their float32 phase is noise, and the gradient through it is divided by their magnitude.  The unfused
# variable-rate backward on the same utterances, measured in the same run (_counterpart), gives 4.8e-6 / 6.7e-4 / 0.84
# (9.1e-7 / 1.9e-4 / 2.3e-2).  At 48 kHz the end-to-end bound checks nothing; the kernel bound is the check there.
# "compose": synthesis_const_rate(analysis_const_rate(x)) against the two float64 models chained, at the analysis' period
# and stretched 2 x: 1.07e-6.
TOL = {"kernel": 9.1e-7, "gm_kernel": 8.8e-7, "compose": 3.2e-6,
       "e2e": {8000: 1.3e-5, 16000: 1.8e-3, 48000: 3.3}, "gm_e2e": {8000: 4.1e-6, 16000: 5.7e-4, 48000: 5.5e-2}}


def _engine():
    from magphase_amd.engine import get_engine
    return get_engine()


def _utts(fs):
    """Three ragged synthetic utterances of 0.25 / 0.28 / 0.3 s (131 or 132 variable-rate frames in all), float32."""
    out = []
    for u, dur in ((0, 0.25), (1, 0.28), (2, 0.3)):
        pcm, pm_sec, voi = syn.make_utterance(u, dur_s=dur, fs=fs)
        out.append((syn.pcm_to_float(pcm).astype(np.float32), pm_sec, voi))
    return out


_BATCH = {}


def _batch(fs, N, cr):
    """The batch of (fs, N) at period cr with its tables, upstream gradients and model gradients (computed once, never
    modified)."""
    key = (fs, N, cr)
    if key not in _BATCH:
        rng = np.random.RandomState(N + int(cr))
        H = N // 2 + 1
        utts = _utts(fs)
        ft = [model.frames_and_tables(pm_sec, voi, sig.size, fs, cr) for sig, pm_sec, voi in utts]
        grads = [tuple(rng.randn(t[1][0].size, H).astype(np.float32) for _k in range(3)) for t in ft]
        ref = [model.grads_autograd(u[0], g, t[0], t[1], N) for u, g, t in zip(utts, grads, ft)]
        ref_gm = [model.grads_autograd(u[0], (g[0], None, None), t[0], t[1], N) for u, g, t in zip(utts, grads, ft)]
        for a in ref + ref_gm:
            a.setflags(write=False)
        _BATCH[key] = (utts, ft, grads, ref, ref_gm)
    return _BATCH[key]


def _table_stats(ft):
    """(most constant-rate rows one variable frame is read by, entries with row0 == row1, frames no row reads)."""
    most = same = unread = 0
    for frames, tabs, _f0 in ft:
        rg = hm.lerp_adjoint_table(tabs[0], tabs[1], tabs[2], frames[0].size)
        n = [len(set(range(a0, a1)) | set(range(b0, b1))) for a0, a1, b0, b1 in rg.tolist()]
        most, same, unread = max([most] + n), same + int(np.sum(tabs[0] == tabs[1])), unread + n.count(0)
    return most, same, unread


def test_the_batches_hold_the_cases_they_are_chosen_for():
    for fs, N in RATES:
        n_var = sum(t[0][0].size for t in _batch(fs, N, 5.0)[1])
        assert 125 <= n_var <= 150
        most, same, _unread = _table_stats(_batch(fs, N, 1.0)[1])
        assert most >= 19 and same >= 15                  # many rows per frame, entries of weight exactly 1
        assert _table_stats(_batch(fs, N, 20.0)[1])[2] > 50   # frames no constant-rate row reads


def _plan(utts, fs, N, cr):
    return LosslessConstRateAnalysisPlan(_engine(), [(u[0], fs, u[1], u[2]) for u in utts], fft_len=N, const_rate_ms=cr)


def _dev_grads(plan, rng, which=(True, True, True)):
    dev, shp = plan.engine.device, (plan.total_out_frames, plan.fft_len // 2 + 1)
    return tuple(torch.from_numpy(rng.randn(*shp).astype(np.float32)).to(dev) if w else None for w in which)


def _both(plan, grads):
    """(fused, staged), the fused form run twice: two runs of the same call give the same bits."""
    a, b, c = plan.run_backward(grads), plan.run_backward_staged(grads), plan.run_backward(grads)
    total = int(plan.lossless.total_smpls)
    assert a.dtype == torch.float32 and tuple(a.shape) == tuple(b.shape) == (total,)
    assert torch.equal(a, c)
    assert bool(torch.isfinite(a).all())
    return a, b


# ---------------------------------------------------------------------------------------------------- fused == staged
@pytest.mark.parametrize("cr", PERIODS)
@pytest.mark.parametrize("fs,N", RATES)
def test_fused_equals_staged_bit_for_bit(fs, N, cr):
    utts = _batch(fs, N, cr)[0]
    plan = _plan(utts, fs, N, cr)
    rng = np.random.RandomState(N + int(cr) + 1)
    full = _dev_grads(plan, rng)
    for which in itertools.product((True, False), repeat=3):          # every subset of None gradient streams
        grads = tuple(g if w else None for g, w in zip(full, which))
        a, b = _both(plan, grads)
        assert torch.equal(a, b), which
        assert bool(a.any()) == any(which)                               # (no gradients: zeros)


@pytest.mark.parametrize("fs,N", RATES)
def test_one_hot_gradients(fs, N):
    """One constant-rate row, one bin: bins 0, 1, N/2 - 1, N/2 (the paired layout's edges: lane 0 of the first group, the
    last mirror, the handover bin), rows with row0 == row1 and with two different rows among them."""
    cr = 1.0
    utts, ft = _batch(fs, N, cr)[:2]
    plan = _plan(utts, fs, N, cr)
    H, dev = N // 2 + 1, plan.engine.device
    same = np.flatnonzero(plan.row0_host == plan.row1_host)
    rows = [0, int(same[0]), int(same[-1]) + 1, plan.total_out_frames // 2, plan.total_out_frames - 1]
    assert plan.row0_host[rows[2]] != plan.row1_host[rows[2]]
    for k, (c, b) in enumerate(itertools.product(rows, (0, 1, N // 2 - 1, N // 2))):
        g = torch.zeros((plan.total_out_frames, H), dtype=torch.float32, device=dev)
        g[c, b] = 1.0
        grads = tuple(g if s == k % 3 else None for s in range(3))
        a, b_ = _both(plan, grads)
        assert torch.equal(a, b_), (c, b, k % 3)
        if k % 3 == 0:
            assert bool(a.any())           # (a magnitude gradient at a live bin always reaches the samples)


def _short_batch(n_frames_list, fs=16000):
    """Utterances of n voiced epochs 160 samples apart (100 Hz), a tone plus noise in float32."""
    rng = np.random.RandomState(sum(n_frames_list))
    out = []
    for n in n_frames_list:
        pm_sec, voi, n_smpls = base.epochs(n, 160.0, True, fs=fs)
        out.append((base.tone_and_noise(rng, n_smpls, fs=fs).astype(np.float32), pm_sec, voi))
    return out


@pytest.mark.parametrize("N", [1024, 4096])        # 12 and 8 waves per workgroup
def test_frame_counts_around_the_workgroup_size(N):
    fs = 16000
    for F in (1, 7, 8, 9, 11, 12, 13, 16, 23, 24, 25):
        plan = _plan(_short_batch([F]), fs, N, 5.0)
        assert int(plan.lossless.total_frames) == F and plan.total_out_frames > 0
        a, b = _both(plan, _dev_grads(plan, np.random.RandomState(F)))
        assert torch.equal(a, b) and bool(a.any()), F


def test_an_utterance_without_rows_inside_a_batch():
    """The middle utterance is shorter than one 20 ms step: it has frames but no constant-rate row, and gets zeros."""
    fs, N, cr = 16000, 1024, 20.0
    utts = _short_batch([9, 1, 12])
    plan = _plan(utts, fs, N, cr)
    assert np.diff(plan.out_off).tolist()[1] == 0 and plan.lossless.n_frames[1] == 1 and plan.total_out_frames > 0
    a, b = _both(plan, _dev_grads(plan, np.random.RandomState(4)))
    assert torch.equal(a, b)
    n = plan.lossless.n_smpls
    assert bool(a[:n[0]].any()) and not bool(a[n[0]:n[0] + n[1]].any()) and bool(a[n[0] + n[1]:].any())
    # ... and a batch that has no rows at all: zeros from both forms, nothing launched
    empty = _plan(utts[1:2], fs, N, cr)
    assert empty.total_out_frames == 0
    g = tuple(torch.zeros((0, N // 2 + 1), device=plan.engine.device) for _k in range(3))
    for out in (empty.run_backward(g), empty.run_backward_staged(g)):
        assert tuple(out.shape) == (n[1],) and not bool(out.any())


# -------------------------------------------------------------------------------------------- against the float64 model
def _leaves(utts, dev, requires_grad=True):
    return [torch.from_numpy(u[0]).to(dev).requires_grad_(requires_grad) for u in utts]


def _call(sigs, utts, fs, N, cr, **kw):
    kw.setdefault("return_device", True)
    return mp.analysis_lossless_const_rate_batch([(s, fs, u[1], u[2]) for s, u in zip(sigs, utts)], fft_len=N,
                                                 const_rate_ms=cr, **kw)


def _backward(out, grads, dev, which=(True, True, True)):
    outs = [o[k] for o in out for k in range(3) if which[k]]
    gs = [torch.from_numpy(g[k]).to(dev) for g in grads for k in range(3) if which[k]]
    torch.autograd.backward(outs, gs)


def _compare(leaves, var_rows, utts, ft, grads, ref, fs, N, label, tag, which=(True, True, True)):
    """Both figures per utterance, all printed before anything is asserted: against the closed form from the device's own
    variable-rate rows, and against the model's forward from the samples."""
    figs = []
    for u, x in enumerate(leaves):
        got = x.grad.cpu().numpy()
        assert got.dtype == np.float32 and got.shape == utts[u][0].shape and np.all(np.isfinite(got))
        g = tuple(grads[u][k] if which[k] else None for k in range(3))
        rows = [var_rows[u][k].cpu().numpy() for k in range(3)]
        closed = model.grads_closed(rows[0], rows[1], rows[2], g, ft[u][0], ft[u][1], got.size, N)
        figs.append((model.rel_err(got, closed), model.rel_err(got, ref[u])))
        print("%s utterance %d %s: kernel %.4g, end to end %.4g" % (tag, u, label or "all", figs[-1][0], figs[-1][1]))
    for e_k, e_e in figs:
        within(e_k, TOL[label + "kernel"], "autograd_const_rate_analysis_%skernel" % label)
        within(e_e, TOL[label + "e2e"][fs], "autograd_const_rate_analysis_%se2e_%d" % (label, fs))


_COUNTERPART = {}


def _counterpart(fs, N, dev):
    """The end-to-end figures of the VARIABLE-rate analysis' backward pass (analysis_lossless_batch, the unfused
    k_analysis_lossless_bwd<P>) on the same utterances, all three streams and m_mag alone: what the float32 forward costs on
    these inputs before any interpolation.  Measured once per rate, printed and recorded; not asserted on."""
    if (fs, N) not in _COUNTERPART:
        rng = np.random.RandomState(N + 7)
        utts, ft = _batch(fs, N, 5.0)[:2]
        worst = []
        for which in ((True, True, True), (True, False, False)):
            leaves = _leaves(utts, dev)
            out = mp.analysis_lossless_batch([(x, fs, u[1], u[2]) for x, u in zip(leaves, utts)], fft_len=N, return_device=True)
            grads = [tuple(rng.randn(*o[k].shape).astype(np.float32) for k in range(3)) for o in out]
            _backward(out, grads, dev, which)
            errs = []
            for u, x in enumerate(leaves):
                g = tuple(grads[u][k] if which[k] else None for k in range(3))
                fr = ft[u][0]
                errs.append(base.rel_err(x.grad.cpu().numpy(), base.grads_autograd(utts[u][0], g, fr[0], fr[1], fr[2], N)))
            worst.append(max(errs))
        _COUNTERPART[(fs, N)] = tuple(worst)
        print("fs %d fft_len %d variable-rate counterpart, end to end: all %.4g, m_mag alone %.4g" % ((fs, N) + tuple(worst)))
        note("autograd_var_rate_analysis_e2e_%d" % fs, worst[0])
        note("autograd_var_rate_analysis_gm_e2e_%d" % fs, worst[1])
    return _COUNTERPART[(fs, N)]


@pytest.mark.parametrize("cr", PERIODS)
@pytest.mark.parametrize("fs,N", RATES)
def test_gradients_match_the_float64_model(fs, N, cr):
    dev = _engine().device
    utts, ft, grads, ref, ref_gm = _batch(fs, N, cr)
    tag = "fs %d fft_len %d period %g ms" % (fs, N, cr)
    _counterpart(fs, N, dev)
    # the device's own variable-rate rows (k_analysis, the launch the backward pass repeats)
    var_rows = [r[:3] for r in mp.analysis_lossless_batch([(torch.from_numpy(u[0]).to(dev), fs, u[1], u[2]) for u in utts],
                                                          fft_len=N, return_device=True)]
    leaves = _leaves(utts, dev)
    out = _call(leaves, utts, fs, N, cr)
    assert [int(o[0].shape[0]) for o in out] == [t[1][0].size for t in ft]
    for o, t in zip(out, ft):
        assert isinstance(o[3], np.ndarray) and o[3].dtype == np.float64 and np.array_equal(o[3], t[2])   # v_f0: host
    _backward(out, grads, dev)
    leaves_gm = _leaves(utts, dev)
    out_gm = _call(leaves_gm, utts, fs, N, cr)
    _backward(out_gm, grads, dev, (True, False, False))
    _compare(leaves_gm, var_rows, utts, ft, grads, ref_gm, fs, N, "gm_", tag, (True, False, False))
    _compare(leaves, var_rows, utts, ft, grads, ref, fs, N, "", tag)


# ------------------------------------------------------------------------------------------------------- the interface
def test_forward_is_unchanged_and_carries_grad_fn_only_when_asked():
    fs, N, cr = 16000, 2048, 5.0
    dev = _engine().device
    utts = _batch(fs, N, cr)[0]
    a = _call(_leaves(utts, dev), utts, fs, N, cr)
    with torch.no_grad():
        b = _call(_leaves(utts, dev), utts, fs, N, cr)
    c = _call(_leaves(utts, dev, False), utts, fs, N, cr)
    d = _call([u[0] for u in utts], utts, fs, N, cr)                            # host arrays, device rows
    h = _call([u[0] for u in utts], utts, fs, N, cr, return_device=False)       # host arrays, host rows
    e = _call(_leaves(utts, dev), utts, fs, N, cr, return_device=False)         # a host return stays detached numpy
    for u in range(len(utts)):
        for k in range(3):
            x = a[u][k]
            assert x.grad_fn is not None and x.requires_grad and x.dtype == torch.float32 and x.numel() > 0
            for y in (b[u][k], c[u][k], d[u][k]):
                assert y.grad_fn is None and not y.requires_grad and torch.equal(x.detach(), y)
            assert isinstance(h[u][k], np.ndarray) and h[u][k].dtype == np.float64
            assert np.array_equal(x.detach().cpu().numpy().astype(np.float64), h[u][k])
            assert isinstance(e[u][k], np.ndarray) and np.array_equal(e[u][k], h[u][k])
        assert isinstance(a[u][3], np.ndarray) and np.array_equal(a[u][3], h[u][3])


def test_a_tensor_on_another_device_is_refused_and_a_cpu_tensor_is_a_host_array():
    fs, N, cr = 8000, 1024, 5.0
    utts = _batch(fs, N, cr)[0]
    host = _call([u[0] for u in utts], utts, fs, N, cr)
    cpu = _call([torch.from_numpy(u[0]).requires_grad_(True) for u in utts], utts, fs, N, cr)
    assert all(c[0].grad_fn is None and torch.equal(c[0], h[0]) for c, h in zip(cpu, host))
    meta = torch.empty(utts[1][0].size, device="meta")
    with pytest.raises(ValueError, match=r"utts\[1\]"):
        _call([torch.from_numpy(utts[0][0]).to(_engine().device), meta, utts[2][0]], utts, fs, N, cr)


def test_gradient_of_one_utterance_stays_inside_it():
    fs, N, cr = 8000, 1024, 5.0
    dev = _engine().device
    utts, _ft, grads = _batch(fs, N, cr)[:3]
    leaves = _leaves(utts, dev)
    out = _call(leaves, utts, fs, N, cr)
    _backward(out[1:2], grads[1:2], dev)
    for u, x in enumerate(leaves):
        assert x.grad is not None and x.grad.shape == x.shape
        assert bool(x.grad.any()) == (u == 1)


@pytest.mark.parametrize("kind", ["bfloat16", "float16", "float64", "strided"])
def test_dtypes_and_strides_get_their_own_gradients(kind):
    fs, N, cr = 16000, 1024, 5.0
    dev = _engine().device
    rng = np.random.RandomState(7)
    utts = _short_batch([9, 14], fs)
    dtype = torch.float32 if kind == "strided" else getattr(torch, kind)
    vals = [torch.from_numpy(u[0]).to(dev).to(dtype) for u in utts]      # what the dtype holds is exact in float32
    if kind == "strided":
        roots = [torch.stack((v, -v), dim=1).reshape(-1) for v in vals]      # the samples are every second element
        wide = [r[::2].requires_grad_(True) for r in roots]
        assert all(w.stride(0) == 2 for w in wide)
    else:
        wide = [v.clone().requires_grad_(True) for v in vals]
    host = _call([v.float().cpu().numpy() for v in vals], utts, fs, N, cr)
    f32 = [v.float().contiguous().clone().requires_grad_(True) for v in vals]
    res, gup = {}, None
    for name, xs in (("wide", wide), ("f32", f32)):
        out = _call(xs, utts, fs, N, cr)
        if gup is None:
            gup = [tuple(torch.from_numpy(rng.randn(*o[k].shape).astype(np.float32)).to(dev) for k in range(3)) for o in out]
        res[name + "_rows"] = [[o[k].detach() for k in range(3)] for o in out]
        torch.autograd.backward([o[k] for o in out for k in range(3)], [g[k] for g in gup for k in range(3)])
        res[name] = [x.grad for x in xs]
    for u, (w, gw, g32) in enumerate(zip(wide, res["wide"], res["f32"])):
        for k in range(3):   # bit-identical to the host-array call on the same float32 samples
            assert torch.equal(res["wide_rows"][u][k], host[u][k]) and torch.equal(res["f32_rows"][u][k], host[u][k])
        assert gw.dtype == dtype and gw.shape == w.shape and g32.dtype == torch.float32
        assert bool(g32.any()) and torch.equal(gw, g32.to(dtype))


def test_a_silent_utterance_gives_zeros_never_nan():
    fs, N, cr = 16000, 1024, 5.0
    dev = _engine().device
    utts = _short_batch([9, 12, 8], fs)
    utts[1] = (np.zeros_like(utts[1][0]), utts[1][1], utts[1][2])
    leaves = _leaves(utts, dev)
    out = _call(leaves, utts, fs, N, cr)
    assert out[1][0].shape[0] > 0 and not bool(out[1][0].any())
    rng = np.random.RandomState(2)
    grads = [tuple(rng.randn(*o[k].shape).astype(np.float32) for k in range(3)) for o in out]
    _backward(out, grads, dev)
    for u, x in enumerate(leaves):
        assert bool(torch.isfinite(x.grad).all()) and bool(x.grad.any()) == (u != 1)


# --------------------------------------------------------------------------------------------------------- composition
def _steady_utt(rng, n_frames, fs, spacing, noise_db=-50.0):
    """Voiced only, epochs on even samples `spacing` apart, and a signal of that period: every harmonic below the Nyquist
    frequency at 1 / h with a random phase, white noise noise_db below, a DC offset and a Nyquist component.  All frames
    see (nearly) the same spectrum, so every interpolated unit phasor keeps a length near 1: the synthesis divides by that
    length, and where two rows of unrelated phase meet near t = 0.5 the composition is as ill-conditioned as the length is
    small -- for the DC and Nyquist phasors (real = +-1, a sign flip) it is discontinuous (last
    paragraph).  A tone plus noise at -10 dB gave lengths down to 1e-4 in its noise bins, and the float32 forward's error
    there, divided by the length squared, 1e-2 of the largest gradient."""
    assert spacing % 2 == 0
    pm_sec, voi, n = base.epochs(n_frames, float(spacing), True, fs=fs)
    t = np.arange(n)
    x = sum(np.cos(2 * np.pi * h * t / spacing + rng.uniform(0, 2 * np.pi)) / h for h in range(1, spacing // 2))
    x = x / np.sqrt(np.mean(x * x))
    sig = 0.1 * (x + 10.0 ** (noise_db / 20.0) * rng.randn(n)) + 0.05 + 0.05 * (-1.0) ** t
    return sig.astype(np.float32), pm_sec, voi


@pytest.mark.parametrize("cr_syn", [5.0, 10.0])      # the analysis' own period, and a 2 x time-stretch
def test_composes_with_the_constant_rate_synthesis(cr_syn):
    """loss = sum((synthesis_const_rate(analysis_const_rate(x)) - target)^2): backward() reaches x through both passes."""
    fs, N, cr = 16000, 1024, 5.0
    dev = _engine().device
    rng = np.random.RandomState(31)
    utts = [_steady_utt(rng, 14, fs, 160), _steady_utt(rng, 21, fs, 114)]
    ft = [model.frames_and_tables(pm_sec, voi, sig.size, fs, cr) for sig, pm_sec, voi in utts]
    leaves = _leaves(utts, dev)
    feats = _call(leaves, utts, fs, N, cr)
    assert all(f[0].grad_fn is not None for f in feats)
    ys = mp.synthesis_from_lossless_const_rate_batch([f[:5] for f in feats], const_rate_ms=cr_syn, return_device=True)
    targets = [rng.randn(int(y.numel())).astype(np.float32) for y in ys]
    loss = sum(((y - torch.from_numpy(t).to(dev)) ** 2).sum() for y, t in zip(ys, targets))
    assert all(y.grad_fn is not None and y.numel() > 0 for y in ys)
    loss.backward()
    for u, x in enumerate(leaves):
        frames, tabs, f0_c = ft[u]
        assert np.array_equal(f0_c, feats[u][3]) and np.all(f0_c > 1.0)
        xm = torch.tensor(utts[u][0].astype(np.float64), requires_grad=True)
        rows_c = model.forward_torch(xm, frames, tabs, N)
        host = hostplan.plan_const_rate_synthesis([f0_c], [fs], cr_syn)
        W = torch.from_numpy(synth_model.lerp_matrix(host["row0"], host["row1"], host["rowt"], f0_c.size))
        var = [W @ r for r in rows_c]
        for p in (rows_c, var):             # no interpolated phasor near 0 at either interpolation: DC / Nyquist
            assert float(p[1].detach()[:, [0, -1]].abs().min()) > 1e-3                   # (the issue's condition)
            assert float((p[1] ** 2 + p[2] ** 2).detach().min()) > 0.25                  # ... and every other bin
        y = synth_model.forward_torch(var[0], var[1], var[2], synth_model.v_pm_of(host["v_f0"][0], fs), N)
        assert y.numel() == targets[u].size
        ((y - torch.from_numpy(targets[u].astype(np.float64))) ** 2).sum().backward()
        got = x.grad.cpu().numpy()
        assert np.all(np.isfinite(got))
        err = model.rel_err(got, xm.grad.numpy())
        print("composition at %g ms, utterance %d: %.4g" % (cr_syn, u, err))
        within(err, TOL["compose"], "autograd_const_rate_analysis_compose")
