"""GPU: tensor.backward() through analysis_lossless_type2_batch and analysis_compressed_type2_batch
(magphase_amd/autograd.py, Type2AnalysisPlan.run_backward, Type2CompressedAnalysisPlan.run_backward) against the float64
chain model of tests/type2_analysis_autograd_model.py, which replays the envelope kernel's own decisions: the gradient is
compared as the adjoint of the passes the device ran, per utterance, no sample left out.  Also: device-tensor input gives
the rows of the host-array input bit for bit, the forward does not change under grad, partial gradients, b_norm_mag, and
the refusal of more than 64 coefficient columns.

Tolerances: max |device - model| / max |model| per utterance, <= 3 x the worst value measured on the MI355X
(profiles/r18_type2_analysis_autograd_tolerance_report.json)."""
import warnings

import numpy as np
import pytest
import torch

import compressed_analysis_autograd_model as cmodel
import type2_analysis_autograd_model as t2m
from _tol import within
from magphase_amd import magphase as mp
from magphase_amd.plans import Type2AnalysisPlan, Type2CompressedAnalysisPlan

pytestmark = pytest.mark.gpu

T2_LOSSLESS_GRAD_TOL = 1.2e-6     # analysis_lossless_type2_batch, all three outputs (measured 4.7e-7)
T2_COMPRESSED_GRAD_TOL = 4.0e-6   # analysis_compressed_type2_batch (measured 1.5e-6)
T2_FORWARD_TOL = 3.0e-6           # the compressed outputs against the model's, relative to each matrix' largest element
#                                   (measured 1.1e-6)

SHAPES = ((20, 16, True), (30, 16, False), (24, 26, False))   # (voiced, unvoiced, gap) epochs: 0.3 .. 0.4 s each


def _engine():
    from magphase_amd.engine import get_engine
    return get_engine()


def _utts(fs, N):
    rng = np.random.RandomState(N + fs // 1000)
    out = []
    for nv, nu, gap in SHAPES:
        sig, pm_sec, voi = t2m.utterance(rng, fs, N, nv, nu, gap=gap)
        out.append((sig, fs, pm_sec, voi))
    return out


def _quiet(fn, *a, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")      # the truncated two-period frame warns, as the reference does
        return fn(*a, **kw)


def _leaves(utts, dev, dtype=torch.float32):
    return [torch.from_numpy(u[0]).to(dev).to(dtype).requires_grad_(True) for u in utts]


def _decisions(t2, iters, H):
    """The envelope kernel's decision words for the plan's two-period rows (they depend on the forward only)."""
    import true_envelope_autograd_model as tam

    F = t2.total_frames
    ones = torch.ones((F, H), dtype=torch.float32, device=t2.engine.device)
    _g, words = t2.run_backward((ones, None, None), iters, want_decisions=True)
    return tam.unpack_decisions(words.cpu().numpy(), H)


def _per_utt_err(leaves, ref, tab):
    so = tab["smpl_off"]
    return max(cmodel.rel_err(x.grad.double().cpu().numpy(), ref[a:b]) for x, a, b in zip(leaves, so[:-1], so[1:]))


@pytest.mark.parametrize("fs,N", [(16000, 1024), (16000, 2048), (48000, 4096)])
def test_lossless_type2_gradients_against_the_chain_model(fs, N):
    e = _engine()
    H = N // 2 + 1
    utts = _utts(fs, N)
    tab = t2m.batch_tables(utts)
    assert np.max(tab["left2"] + tab["right2"] + 1) > N        # the unvoiced gap: a two-period frame longer than fft_len
    leaves = _leaves(utts, e.device)
    res = _quiet(mp.analysis_lossless_type2_batch, [(x,) + u[1:] for x, u in zip(leaves, utts)], fft_len=N,
                 return_device=True, return_iters=True)
    ref = _quiet(mp.analysis_lossless_type2_batch, utts, fft_len=N, return_device=True)
    rng = np.random.RandomState(3)
    loss, ups = 0.0, []
    for r, rr in zip(res, ref):
        assert all(t.grad_fn is not None for t in r[:3]) and not r[6].requires_grad and r[6].dtype == torch.float64
        for k in range(3):                                       # device-tensor input: the host-array call's rows, bit for bit
            assert torch.equal(r[k].detach(), rr[k]) and rr[k].grad_fn is None
        assert torch.equal(r[6], rr[6])
        g = [torch.from_numpy(rng.randn(*r[k].shape).astype(np.float32)).to(e.device) for k in range(3)]
        ups.append(g)
        loss = loss + sum((r[k] * g[k]).sum() for k in range(3))
    loss.backward()
    # ---- the model with the device's pass counts and decisions
    t2 = Type2AnalysisPlan(e, utts, fft_len=N)
    _env, _re, _im, _gain, iters = t2.run(want_iters=True)
    dec = _decisions(t2, iters, H)
    rows = t2m.out_rows(tab)
    F = tab["pos"].size
    full = [np.zeros((F, H)) for _ in range(3)]
    for k in range(3):
        full[k][rows] = np.concatenate([g[k].cpu().numpy() for g in ups])
    it = iters.cpu().numpy()
    sig = np.concatenate([u[0] for u in utts]).astype(np.float64)
    for which, label in (((0, 1, 2), "all"),):
        gref = t2m.grads_of(sig, lambda x: t2m.forward_torch(x, tab, N, it, dec)[:3], full)
        err = _per_utt_err(leaves, gref, tab)
        print("type2 lossless grad fs=%d N=%d %s: %.3g" % (fs, N, label, err))
        within(err, T2_LOSSLESS_GRAD_TOL, "T2_LOSSLESS_GRAD_TOL")
    # ---- the plan's own backward gives the same bits, and the envelope alone / the phase alone add up to it
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(e.device)   # noqa: E731
    g_all = t2.run_backward(tuple(up(f) for f in full), iters)
    assert torch.equal(g_all, torch.cat([x.grad for x in leaves]))
    g_env = t2.run_backward((up(full[0]), None, None), iters)
    g_ph = t2.run_backward((None, up(full[1]), up(full[2])), iters)
    assert torch.equal(g_env + g_ph, g_all)
    assert bool(torch.isfinite(g_all).all())


@pytest.mark.parametrize("rate,phase_dim,norm,which", [(-1.0, 45, False, (0, 1, 2)), (5.0, 10, True, (0, 1, 2)),
                                                       (7.5, 45, True, (0,)), (5.0, 45, False, (1,)),
                                                       (-1.0, 10, True, (2,)), (7.5, 10, False, (0, 1, 2))])
def test_compressed_type2_gradients_against_the_chain_model(rate, phase_dim, norm, which):
    e = _engine()
    fs, N, mag_dim = 16000, 1024, 60
    H = N // 2 + 1
    utts = _utts(fs, N)
    tab = t2m.batch_tables(utts)
    leaves = _leaves(utts, e.device)
    kw = dict(fft_len=N, mag_dim=mag_dim, phase_dim=phase_dim, b_norm_mag=norm, const_rate_ms=rate, return_device=True)
    res = _quiet(mp.analysis_compressed_type2_batch, [(x,) + u[1:] for x, u in zip(leaves, utts)], **kw)
    ref = _quiet(mp.analysis_compressed_type2_batch, utts, **kw)
    for r, rr in zip(res, ref):
        for k in range(3):
            assert r[k].grad_fn is not None and torch.equal(r[k].detach(), rr[k])
        assert np.array_equal(r[7], rr[7]) and np.array_equal(r[3], rr[3])
    # ---- the model on the plan's row tables, with the device's pass counts and decisions
    plan = Type2CompressedAnalysisPlan(e, utts, fft_len=N, mag_dim=mag_dim, phase_dim=phase_dim, const_rate_ms=rate)
    _outs, _gain, iters = plan.run(want_iters=True)
    dec = _decisions(plan.t2, iters, H)
    r0, r1, rt = plan._rows_host
    rows_tab = {"row0": np.asarray(r0, dtype=np.int64), "row1": np.asarray(r1, dtype=np.int64),
                "rowt": np.asarray(rt, dtype=np.float64), "voi": plan.voi.cpu().numpy() > 0}
    wm, wp = cmodel.warps(N, fs, mag_dim, phase_dim)
    it = iters.cpu().numpy()
    sig = np.concatenate([u[0] for u in utts]).astype(np.float64)
    fn = lambda x: t2m.compressed_torch(x, tab, rows_tab, N, it, dec, wm, wp, b_norm_mag=norm)   # noqa: E731
    with torch.no_grad():
        model_out = [t.numpy() for t in fn(torch.from_numpy(sig))]
    got = [torch.cat([r[k].detach() for r in res]).double().cpu().numpy() for k in range(3)]
    fwd = max(cmodel.rel_err(got[k], model_out[k]) for k in range(3))
    rng = np.random.RandomState(11)
    ups = [rng.randn(*got[k].shape).astype(np.float32) if k in which else None for k in range(3)]
    ties = cmodel.tie_mask(model_out[3], model_out[4], rows_tab)
    for k in (1, 2):
        if ups[k] is not None:
            ups[k][ties[k - 1]] = 0.0        # a coefficient within 1e-3 of the clip: float32 may land on its other side
    off = np.concatenate(([0], np.cumsum([int(r[0].shape[0]) for r in res])))
    loss = 0.0
    for u, r in enumerate(res):
        for k in which:
            loss = loss + (r[k] * torch.from_numpy(ups[k][off[u]:off[u + 1]]).to(e.device)).sum()
    loss.backward()
    gref = t2m.grads_of(sig, lambda x: fn(x)[:3], ups)
    err = _per_utt_err(leaves, gref, tab)
    print("type2 compressed rate=%g phase_dim=%d norm=%s which=%s: forward %.3g, grad %.3g"
          % (rate, phase_dim, norm, which, fwd, err))
    within(fwd, T2_FORWARD_TOL, "T2_FORWARD_TOL")
    within(err, T2_COMPRESSED_GRAD_TOL, "T2_COMPRESSED_GRAD_TOL")
    assert all(bool(torch.isfinite(x.grad).all()) for x in leaves)


def test_bfloat16_waveform_gets_a_bfloat16_gradient_and_no_grad_runs_as_before():
    e = _engine()
    fs, N = 16000, 1024
    utts = _utts(fs, N)[:2]
    leaves = _leaves(utts, e.device, torch.bfloat16)
    res = _quiet(mp.analysis_compressed_type2_batch, [(x,) + u[1:] for x, u in zip(leaves, utts)], fft_len=N,
                 const_rate_ms=5.0, return_device=True)
    sum(r[0].sum() + r[1].sum() for r in res).backward()
    assert all(x.grad.dtype == torch.bfloat16 and x.grad.shape == x.shape and bool(torch.isfinite(x.grad).all())
               for x in leaves)
    with torch.no_grad():
        res = _quiet(mp.analysis_compressed_type2_batch, [(x,) + u[1:] for x, u in zip(leaves, utts)], fft_len=N,
                     return_device=True)
    assert all(r[0].grad_fn is None for r in res)
    host = _quiet(mp.analysis_lossless_type2_batch, [(x,) + u[1:] for x, u in zip(leaves, utts)], fft_len=N)
    assert isinstance(host[0][0], np.ndarray)


def test_more_than_64_columns_raise_before_the_forward():
    e = _engine()
    fs, N = 16000, 1024
    utts = _utts(fs, N)[:1]
    leaves = _leaves(utts, e.device)
    with pytest.raises(NotImplementedError, match="mag_dim"):
        _quiet(mp.analysis_compressed_type2_batch, [(leaves[0],) + utts[0][1:]], fft_len=N, mag_dim=65, return_device=True)

T2_CYCLE_GRAD_TOL = 9.0e-5   # the cycle with the type-2 synthesis, per gradient matrix (measured 3.3e-5)


@pytest.mark.parametrize("rate", [-1.0, 5.0])
def test_cycle_with_the_type2_synthesis_against_the_composed_model(rate):
    """analysis_compressed_type2_batch(synthesis_from_compressed_type2_batch(x)): backward() reaches the coefficient
    matrices, and their gradients equal those of the two float64 models composed -- the synthesis model of
    tests/type2_synthesis_autograd_model.py, then the chain model replaying the envelope kernel's decisions on the
    device's waveform.  Per gradient matrix, no element left out."""
    import test_gpu_type2_synthesis_autograd as syn_t
    import type2_synthesis_autograd_model as smodel

    e = _engine()
    N, pd, fs, mag_dim = 1024, 45, 16000, 60
    H = N // 2 + 1
    b = syn_t._make_batch(N, -1.0, pd, 1.0, True, 61, kinds=("mixed", "voiced"), n_rows=(18, 14))
    assert b["fs"] == fs
    leaves = syn_t._leaves(b, e.device)
    ys = syn_t._call(b, leaves)
    assert all(y.grad_fn is not None and y.dtype == torch.float64 for y in ys)
    epochs = []
    for u in b["utts"]:
        t = u["tab"]
        pm = t["v_pm"] - t["start"]
        keep = (pm > 0) & (pm < t["out_len"] - 1)
        epochs.append((pm[keep] / float(fs), np.asarray(t["voiced"][keep], dtype=np.float64)))
    kw = dict(fft_len=N, mag_dim=mag_dim, phase_dim=pd, const_rate_ms=rate, return_device=True)
    out = _quiet(mp.analysis_compressed_type2_batch, [(y, fs, pm_sec, voi) for y, (pm_sec, voi) in zip(ys, epochs)], **kw)
    assert all(o[k].grad_fn is not None for o in out for k in range(3))
    wm, wp = cmodel.warps(N, fs, mag_dim, pd)
    rng = np.random.RandomState(63)
    gup, pre = [], []
    for u, y, o, (pm_sec, voi) in zip(b["utts"], ys, out, epochs):
        # the device's pass counts, decisions and row tables for this utterance's waveform (one-utterance plan: the
        # kernels treat every frame on its own, so these are the batch call's)
        plan = _quiet(Type2CompressedAnalysisPlan, e, [(y.detach(), fs, pm_sec, voi)], fft_len=N, mag_dim=mag_dim,
                      phase_dim=pd, const_rate_ms=rate)
        _o, _g, iters = plan.run(want_iters=True)
        dec = _decisions(plan.t2, iters, H)
        r0, r1, rt = plan._rows_host
        rows_tab = {"row0": np.asarray(r0, dtype=np.int64), "row1": np.asarray(r1, dtype=np.int64),
                    "rowt": np.asarray(rt, dtype=np.float64), "voi": plan.voi.cpu().numpy() > 0}
        m = [torch.tensor(x, requires_grad=True) for x in u["feats"]]
        ym = smodel.forward_torch(m[0], m[1], m[2], u["tab"], b["cst"], u["ns"], u["inv"])
        tab = t2m.batch_tables([(np.zeros(int(ym.numel())), fs, pm_sec, voi)])
        om = t2m.compressed_torch(ym, tab, rows_tab, N, iters.cpu().numpy(), dec, wm, wp)
        g = [rng.randn(*o[j].shape).astype(np.float32) for j in range(3)]
        for j, msk in enumerate(cmodel.tie_mask(om[3].detach().numpy(), om[4].detach().numpy(), rows_tab), start=1):
            g[j][msk] = 0.0
        sum((om[j] * torch.from_numpy(g[j].astype(np.float64))).sum() for j in range(3)).backward()
        gup.append(g), pre.append(m)
    torch.autograd.backward([o[j] for o in out for j in range(3)],
                            [torch.from_numpy(g[j]).to(e.device) for g in gup for j in range(3)])
    for u in range(len(b["utts"])):
        for j, name in enumerate(("m_mag_mel_log", "m_real_mel", "m_imag_mel")):
            got = leaves[u][j].grad.cpu().numpy()
            assert np.all(np.isfinite(got)) and got.any()
            err = smodel.rel_err(got, pre[u][j].grad.numpy())
            print("type2 cycle rate=%g utterance %d %s: %.4g" % (rate, u, name, err))
            within(err, T2_CYCLE_GRAD_TOL, "T2_CYCLE_GRAD_TOL")


@pytest.mark.parametrize("rate", [-1.0, 5.0])
def test_digital_silence_gives_nan_rows_and_finite_gradients(rate):
    """A stretch of exact zeros: the envelope rows of its frames are NaN, as in the reference, and so are the log-mel rows
    that read them.  With those rows masked out of the loss, every sample gradient is finite -- also on the grid, where an
    output frame interpolates between a NaN row and a finite one."""
    e = _engine()
    fs, N = 16000, 1024
    sig, _fs, pm_sec, voi = _utts(fs, N)[0]
    sig = sig.copy()
    sig[2300:3300] = 0.0                     # inside the unvoiced stretch: two-period frames of 320 samples
    x = torch.from_numpy(sig).to(e.device).requires_grad_(True)
    (r,) = _quiet(mp.analysis_compressed_type2_batch, [(x, fs, pm_sec, voi)], fft_len=N, const_rate_ms=rate,
                  return_device=True)
    bad = ~torch.isfinite(r[0]).all(dim=1)
    assert 0 < int(bad.sum()) < int(bad.numel())
    assert bool(torch.isfinite(r[1]).all()) and bool(torch.isfinite(r[2]).all())
    g = torch.from_numpy(np.random.RandomState(9).randn(*r[0].shape).astype(np.float32)).to(e.device)
    (torch.where(bad[:, None], torch.zeros_like(r[0]), r[0]) * g).sum().backward()
    assert bool(torch.isfinite(x.grad).all()) and bool(x.grad.any())
