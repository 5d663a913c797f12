"""GPU: k_synth_comp_bwd and k_mel_unwarp_bwd on their own against float64 closed forms, and tensor.backward() through
synthesis_from_compressed_batch (magphase_amd/autograd.py, CompressedSynthesisPlan.run_backward) against torch autograd of
the float64 model of tests/compressed_synthesis_autograd_model.py, at both frame rates, with the properties the feature
promises: the forward's samples do not change, partial gradients and repeated passes are exact, every input dtype and
stride gets its own gradient, unvoiced and silent frames give zeros and finite values, uninitialised scratch is never read,
what has no backward pass says so, and the synthesis composes with the compressed analysis' backward pass."""
import numpy as np
import pytest
import torch

import compressed_analysis_autograd_model as ana_model
import compressed_synthesis_autograd_model as model
from _tol import within
from magphase_amd import magphase as mp

pytestmark = pytest.mark.gpu

# max |device - model| / max |model| per gradient matrix, no element left out (model.rel_err), against the float64 model.
# Stated at <= 3 x the worst case measured on an MI355X (profiles/r16_compressed_synthesis_autograd_tolerance_report.json;
# DESIGN.md section 3.3k):
#   "kernel"   k_synth_comp_bwd alone against the closed form on the device's own float32 inputs: 9.05e-7;
#   "e2e"      synthesis_from_compressed_batch against the model's autograd: 9.41e-6 (the float32 forward rows, the
#              float32 noise gains and the float32 adjoint of the output high-pass are in it);
#   "compose"  compressed synthesis + compressed analysis against the two float64 models chained: 4.61e-6.
TOL = {"kernel": 2.7e-6, "e2e": 2.8e-5, "compose": 1.38e-5}


def _engine():
    from magphase_amd.engine import get_engine
    return get_engine()


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _up(dev, a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)


# ----------------------------------------------------------------------------------------------------------------------
# kernel 1 alone
# ----------------------------------------------------------------------------------------------------------------------
def _noise_spectrum(noise, pos, L, R, wt, N):
    """FFT_N of the windowed frame noise[pos - L .. pos + R] with its epoch at index 0 (the forward's Ns), float64."""
    seg = noise[pos - L:pos + R + 1] * model._half_windows(L, R, bool(wt))
    m = np.zeros(N)
    m[N // 2 - L:N // 2 - L + seg.size] = seg
    return np.fft.fft(np.fft.fftshift(m))[:N // 2 + 1]


def _kernel1_case(N, which=(True, True, True), seed=0):
    e = _engine()
    dev = e.device
    H, M = N // 2 + 1, N // 2
    rng = np.random.RandomState(100 + N + seed)
    F = 21                                   # three workgroups at 8 waves, six at 4
    n_per = int(0.37 * H)                    # not a multiple of 64
    n_phase = min((n_per + 63) // 64 * 64, H)
    ld = int(e.lib.mpx_spec_ld(H))
    # noise frames: random extents within what the planner allows (left <= N/2, right + 1 <= N/2), both windows
    nleft = rng.randint(1, M + 1, size=F)
    nright = rng.randint(1, M, size=F)
    nleft[3], nright[3] = M, M - 1           # the widest frame
    nleft[4], nright[4] = 1, 1               # the narrowest
    npos = np.cumsum(nleft + rng.randint(0, 40, size=F))
    noise = rng.uniform(-1, 1, int(npos[-1] + M + 8)).astype(np.float32)
    wtype = rng.randint(0, 2, size=F)
    voiced = (rng.rand(F) < 0.7).astype(np.int32)
    voiced[0], voiced[1], voiced[2] = 1, 0, 1            # an unvoiced frame for sure
    wtype = wtype * voiced
    inv_gain = rng.uniform(0.05, 0.2, size=F).astype(np.float32)
    win_l = rng.randint(1, M + 1, size=F)
    win_r = rng.randint(1, M, size=F)
    win_l[2] = 0                                          # win_l == 0: the single rising sample weighs 1
    win_l[5], win_r[5] = M, M - 1
    # the gradient buffer: frame 0 starts before it, the last frame ends after it, frame 6 is wider than what is kept of it
    total = 5 * N
    gpos = rng.randint(0, total - N, size=F).astype(np.int64)
    glo, ghi = np.zeros(F, dtype=np.int32), np.full(F, N, dtype=np.int32)
    gpos[0], glo[0] = -(M // 3), M // 3
    gpos[F - 1], ghi[F - 1] = total - M - 7, M + 7
    gpos[6], glo[6], ghi[6] = 1000 - 70, 70, 70 + 301
    gpos[7], glo[7], ghi[7] = 17, M + 3, M + 3                 # nothing kept at all
    gy = rng.randn(total).astype(np.float32)
    # features: NaN where the forward writes nothing (row padding, phase rows of unvoiced frames, bins from n_per on)
    m = np.exp(rng.randn(F, H)).astype(np.float32)
    a, b = rng.randn(F, H).astype(np.float32), rng.randn(F, H).astype(np.float32)
    a[0, 3:40] = b[0, 3:40] = 0.0                         # a voiced frame with a == b == 0 at some bins
    a[2, 0] = b[2, 0] = 0.0
    per_v = np.abs(rng.randn(H)).astype(np.float32)
    per_v[n_per:] = 0.0
    ap_v, ap_u = np.abs(rng.randn(H)).astype(np.float32), np.abs(rng.randn(H)).astype(np.float32)
    a_dev, b_dev = a.copy(), b.copy()
    a_dev[:, n_per:] = b_dev[:, n_per:] = np.nan
    a_dev[voiced == 0] = b_dev[voiced == 0] = np.nan

    def padded(x):
        buf = torch.full((F, ld), float("nan"), dtype=torch.float32, device=dev)
        buf[:, :H] = _up(dev, x)
        return buf

    d_m, d_a, d_b = padded(m), padded(a_dev), padded(b_dev)
    outs = [torch.full((F + 2, ld), float("nan"), dtype=torch.float32, device=dev) if w else None for w in which]
    rows = [o[1:F + 1] if o is not None else None for o in outs]
    i32, i64 = np.int32, np.int64
    e.launch("mpx_synthesis_compressed_backward", N, e.tables(N), _up(dev, gy), total, _up(dev, gpos, i64), _up(dev, glo, i32),
             _up(dev, ghi, i32), F, d_m, d_a, d_b, ld, _up(dev, noise), _up(dev, npos, i64), _up(dev, nleft, i32),
             _up(dev, nright, i32), _up(dev, wtype, i32), _up(dev, voiced, i32), _up(dev, inv_gain), _up(dev, win_l, i32),
             _up(dev, win_r, i32), _up(dev, per_v), _up(dev, ap_v), _up(dev, ap_u), n_per, rows[0], rows[1], rows[2], ld)
    torch.cuda.synchronize()
    # the closed form in float64 on the same float32 inputs
    ns = np.stack([_noise_spectrum(noise.astype(np.float64), int(npos[f]), int(nleft[f]), int(nright[f]), wtype[f], N)
                   for f in range(F)])
    v = voiced[:, None] != 0
    P = np.where(v, per_v[None, :].astype(np.float64), 0.0)
    A = np.where(v, ap_v[None, :], ap_u[None, :]).astype(np.float64)
    gwin = np.zeros((F, N))
    for f in range(F):
        lo, hi = int(glo[f]), int(ghi[f])
        w = np.zeros(N)
        w[M - win_l[f]:M + win_r[f] + 1] = model._half_windows(int(win_l[f]), int(win_r[f]), False)
        gwin[f, lo:hi] = gy[gpos[f] + lo:gpos[f] + hi].astype(np.float64) * w[lo:hi]
    ref = model.frame_grads_closed(m.astype(np.float64), np.where(v, a, 0.0).astype(np.float64),
                                   np.where(v, b, 0.0).astype(np.float64), P,
                                   A * ns * inv_gain[:, None].astype(np.float64), gwin, N)
    worst = 0.0
    for k, name in enumerate(("grad m", "grad a", "grad b")):
        if not which[k]:
            continue
        full = outs[k].cpu().numpy()
        width = H if k == 0 else n_phase
        got = full[1:F + 1, :width].astype(np.float64)
        assert np.all(np.isnan(full[0])) and np.all(np.isnan(full[F + 1])), name      # sentinel rows
        assert np.all(np.isnan(full[1:F + 1, width:])), name                            # nothing beyond the written bins
        assert np.all(np.isfinite(got)), name
        if k > 0:
            assert not got[voiced == 0].any() and not got[:, n_per:].any(), name        # exact zeros
        assert not got[7].any(), name                                                   # a frame with nothing kept
        err = model.rel_err(got, ref[k][:, :width])
        print("fft_len %d %s: %.4g" % (N, name, err))
        within(err, TOL["kernel"], "autograd_compressed_synthesis_kernel")
        worst = max(worst, err)
        # the den == 0 convention on the bins that were set to zero: m P gS
        if k == 1:
            assert np.any(got[0, 3:40] != 0.0)
    return worst


@pytest.mark.parametrize("N", [1024, 2048, 4096])
def test_frame_kernel_against_the_closed_form(N):
    """Random rows and noise; the first and the last frame of a buffer, a frame wider than the kept output and one with
    nothing kept; win_l == 0; a voiced frame with a == b == 0 at some bins; unvoiced frames; NaN wherever the forward
    writes nothing, NaN sentinel rows around every output and beyond the written phase bins."""
    _kernel1_case(N)


@pytest.mark.parametrize("which", [(False, True, True), (True, False, True), (True, True, False), (True, False, False)])
def test_frame_kernel_null_outputs(which):
    _kernel1_case(1024, which=which, seed=1)
    _kernel1_case(4096, which=which, seed=1)


# ----------------------------------------------------------------------------------------------------------------------
# kernel 2 alone
# ----------------------------------------------------------------------------------------------------------------------
def _kernel2_case(rows, H, n_out, which=(True, True, True), n_phase_bins=None, seed=0):
    """Each element within (K + 8) 2^-24 sum_k |A[r, k] B[c, k]|: K roundings of the sum in any order and a few for the
    operand's product and the chunk totals."""
    e = _engine()
    dev = e.device
    rng = np.random.RandomState(seed + 3 * rows + H + n_out)
    n_pb = n_phase_bins if n_phase_bins is not None else min(H, 64 * ((int(0.4 * H) + 63) // 64))
    n_ph_out = n_out
    rows_p = rows + 5                               # the phase jobs have their own row count
    pad = 7

    def padded(r, x):
        buf = torch.full((r, H + pad), float("nan"), dtype=torch.float32, device=dev)
        buf[:, :x.shape[1]] = _up(dev, x)
        return buf

    E = np.exp(0.5 * rng.randn(rows, H)).astype(np.float32)
    gE = rng.randn(rows, H).astype(np.float32)
    u_mag = rng.randn(n_out, H).astype(np.float32)
    ga, gb = rng.randn(rows_p, n_pb).astype(np.float32), rng.randn(rows_p, n_pb).astype(np.float32)
    u_ph = rng.randn(n_ph_out, H).astype(np.float32)
    d_E, d_gE, d_ga, d_gb = padded(rows, E), padded(rows, gE), padded(rows_p, ga), padded(rows_p, gb)

    def sentinel(r, c):
        return torch.full((r + 2, c), float("nan"), dtype=torch.float32, device=dev) if r is not None else None

    o = [sentinel(rows, n_out) if which[0] else None, sentinel(rows_p, n_ph_out) if which[1] else None,
         sentinel(rows_p, n_ph_out) if which[2] else None]
    v = [x[1:-1] if x is not None else None for x in o]
    e.launch("mpx_mel_unwarp_backward", H, d_E, H + pad, d_gE, H + pad, _up(dev, u_mag), n_out, rows, v[0], d_ga, d_gb,
             H + pad, n_pb, _up(dev, u_ph), n_ph_out, rows_p, v[1], v[2])
    torch.cuda.synchronize()
    jobs = [(E.astype(np.float64) * gE.astype(np.float64), u_mag, H), (ga, u_ph[:, :n_pb], n_pb), (gb, u_ph[:, :n_pb], n_pb)]
    worst = 0.0
    for k, (A, B, K) in enumerate(jobs):
        if not which[k]:
            continue
        full = o[k].cpu().numpy()
        assert np.all(np.isnan(full[0])) and np.all(np.isnan(full[-1])), k
        got = full[1:-1].astype(np.float64)
        A64, B64 = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
        ref, mass = A64 @ B64.T, np.abs(A64) @ np.abs(B64).T
        bound = (K + 8) * 2.0 ** -24 * mass
        err = np.abs(got - ref)
        assert np.all(np.isfinite(got)) and np.all(err <= bound), (k, float(np.max(err - bound)))
        frac = float(np.max(err[bound > 0] / bound[bound > 0]))
        within(frac, 1.0, "autograd_compressed_synthesis_mel_unwarp_bwd_fraction_of_bound")
        worst = max(worst, frac)
    return worst


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("H,n_out", [(513, 60), (1025, 1), (2049, 64), (2049, 45)])
def test_mel_unwarp_backward_kernel(rows, H, n_out):
    """Tile edges in the rows, a lone tail bin in every H, n_out from 1 to 64, row pitches greater than the widths, NaN in
    every operand's padding and around every output."""
    frac = _kernel2_case(rows, H, n_out)
    print("rows %d H %d n_out %d: %.3f of the bound" % (rows, H, n_out, frac))


@pytest.mark.parametrize("which", [(True, False, False), (False, True, False), (False, False, True), (True, False, True),
                                   (False, True, True)])
def test_mel_unwarp_backward_one_and_two_jobs(which):
    _kernel2_case(65, 513, 60, which=which)


@pytest.mark.parametrize("n_pb", [1, 63, 100, 200, 513])
def test_mel_unwarp_backward_phase_bins_not_a_multiple_of_64(n_pb):
    _kernel2_case(70, 513, 45, n_phase_bins=n_pb)


# ----------------------------------------------------------------------------------------------------------------------
# end to end
# ----------------------------------------------------------------------------------------------------------------------
_BATCH = {}
_KINDS = ("mixed", "unvoiced", "voiced")


def _fs_of(N):
    return 48000 if N == 4096 else 16000


def _make_batch(N, cr, pd, hpf, seed, kinds=_KINDS, n_rows=(22, 16, 20), ap_win=True, fbank=False, mag_level=None):
    fs = _fs_of(N)
    rng = np.random.RandomState(seed)
    cst = model.constants(fs, N, 60, pd, b_fbank_mel=fbank)
    utts = []
    for kind, n in zip(kinds, n_rows):
        lf0 = model.lf0_track(rng, n, kind, fs)
        feats = [_f32(x) for x in model.features(rng, n, 60, pd)]
        if mag_level is not None:
            feats[0][:] = mag_level
        tab = model.tables(lf0, fs, N, cr, ap_win)
        noise = _f32(rng.uniform(-1, 1, tab["ns_len"]))
        ns, inv = model.noise_spectra(noise, tab, N)
        gy = rng.randn(tab["out_len"]).astype(np.float32)
        utts.append(dict(lf0=lf0, feats=feats, tab=tab, noise=noise, ns=ns, inv=inv, gy=gy))
    return dict(fs=fs, N=N, cr=cr, pd=pd, hpf=hpf, cst=cst, utts=utts, ap_win=ap_win, fbank=fbank)


def _batch(N, cr, pd, hpf):
    """The gradient tests' batch (computed once, never modified): three utterances -- mixed, all unvoiced, all voiced --
    of 22, 16 and 20 rows, and the model's gradients."""
    key = (N, cr, pd, hpf)
    if key not in _BATCH:
        b = _make_batch(N, cr, pd, hpf, N + pd + 7 * cr + hpf)
        _reference(b)
        _BATCH[key] = b
    return _BATCH[key]


def _reference(b):
    b["ref"] = [model.grads_autograd(*u["feats"], u["gy"], u["tab"], b["cst"], u["ns"], u["inv"], b["hpf"])
                for u in b["utts"]]
    for r in b["ref"]:
        for x in r:
            x.setflags(write=False)


def _leaves(b, dev, requires_grad=True, dtype=torch.float32):
    return [[torch.from_numpy(x).to(dev).to(dtype).requires_grad_(requires_grad) for x in u["feats"]] for u in b["utts"]]


def _call(b, leaves, **kw):
    kw.setdefault("return_device", True)
    kw.setdefault("noise", [u["noise"] for u in b["utts"]])
    utts = [tuple(lv) + (u["lf0"],) for lv, u in zip(leaves, b["utts"])]
    return mp.synthesis_from_compressed_batch(utts, b["fs"], fft_len=b["N"], b_voi_ap_win=b["ap_win"], b_const_rate=b["cr"],
                                              b_out_hpf=b["hpf"], b_fbank_mel=b["fbank"], **kw)


def _gys(b, dev):
    return [torch.from_numpy(u["gy"]).to(dev) for u in b["utts"]]


def _backward(b, wavs, dev):
    torch.autograd.backward(wavs, [g.to(w.dtype) for g, w in zip(_gys(b, dev), wavs)])


def _compare(b, leaves, label, tol="e2e", name="autograd_compressed_synthesis_e2e"):
    for u, lv in enumerate(leaves):
        for k, nm in enumerate(("m_mag_mel_log", "m_real_mel", "m_imag_mel")):
            got = lv[k].grad.cpu().numpy()
            ref = b["ref"][u][k]
            assert got.dtype == np.float32 and got.shape == ref.shape and np.all(np.isfinite(got))
            err = model.rel_err(got, ref)
            print("%s utterance %d %s: %.4g" % (label, u, nm, err))
            within(err, TOL[tol], name)


@pytest.mark.parametrize("hpf", [False, True])
@pytest.mark.parametrize("pd", [10, 45])
@pytest.mark.parametrize("cr", [False, True])
@pytest.mark.parametrize("N", [1024, 2048, 4096])
def test_gradients_match_the_float64_model(N, cr, pd, hpf):
    dev = _engine().device
    b = _batch(N, cr, pd, hpf)
    leaves = _leaves(b, dev)
    wavs = _call(b, leaves)
    for w, u in zip(wavs, b["utts"]):
        assert w.grad_fn is not None and w.dtype == (torch.float64 if hpf else torch.float32)
        assert int(w.numel()) == u["tab"]["out_len"]
    _backward(b, wavs, dev)
    _compare(b, leaves, "fft_len %d const_rate %s phase_dim %d hpf %s" % (N, cr, pd, hpf))
    assert not leaves[1][1].grad.any() and not leaves[1][2].grad.any()       # the unvoiced utterance: exactly zero
    assert bool(leaves[0][1].grad.any()) and bool(leaves[2][2].grad.any())


@pytest.mark.parametrize("variant", ["no_voi_ap_win", "fbank", "device_noise"])
def test_variants_in_scope(variant):
    """b_voi_ap_win off and the filter-bank unwarp against the model; noise_mode='device' (whose samples the model does
    not know) against the model evaluated on the noise the plan generated."""
    dev = _engine().device
    N, cr, pd, hpf = 1024, True, 45, True
    b = _make_batch(N, cr, pd, hpf, 31, ap_win=(variant != "no_voi_ap_win"), fbank=(variant == "fbank"))
    kw = {}
    if variant == "device_noise":
        from magphase_amd.plans import CompressedSynthesisPlan

        e = _engine()
        plan = CompressedSynthesisPlan(e, [tuple(u["feats"]) + (u["lf0"],) for u in b["utts"]], b["fs"], fft_len=N,
                                       b_const_rate=cr, noise_mode="device", noise_seeds=[5, 6, 7])
        noise = plan.noise.cpu().numpy().astype(np.float64)
        for k, u in enumerate(b["utts"]):
            u["noise"] = noise[int(plan.noise_off_host[k]):int(plan.noise_off_host[k + 1])]
            u["ns"], u["inv"] = model.noise_spectra(u["noise"], u["tab"], N)
        kw = dict(noise=None, noise_mode="device", noise_seeds=[5, 6, 7])
    _reference(b)
    leaves = _leaves(b, dev)
    wavs = _call(b, leaves, **kw)
    _backward(b, wavs, dev)
    _compare(b, leaves, variant)


def test_forward_is_unchanged():
    """Samples from a grad-requiring call are bit-identical to the plain device-tensor call and to the host-array call."""
    dev = _engine().device
    for cr, hpf in ((False, True), (True, False)):
        b = _batch(2048, cr, 45, hpf)
        a = _call(b, _leaves(b, dev))
        with torch.no_grad():
            c = _call(b, _leaves(b, dev))
        d = _call(b, _leaves(b, dev, False))
        h = _call(b, [[x.astype(np.float32) for x in u["feats"]] for u in b["utts"]], return_device=False)
        for u in range(len(a)):
            assert a[u].grad_fn is not None and a[u].requires_grad and a[u].numel() > 0
            for y in (c[u], d[u]):
                assert y.grad_fn is None and not y.requires_grad and torch.equal(a[u].detach(), y)
            assert np.array_equal(a[u].detach().cpu().numpy().astype(np.float64), h[u])
        hh = _call(b, _leaves(b, dev), return_device=False)          # a host return stays a detached numpy array
        assert all(isinstance(x, np.ndarray) for x in hh) and all(np.array_equal(x, y) for x, y in zip(hh, h))


@pytest.mark.parametrize("kind", ["bfloat16", "float16", "float64", "strided", "columns"])
def test_dtypes_and_strides_get_their_own_gradients(kind):
    dev = _engine().device
    b = _make_batch(1024, True, 10, True, 41, n_rows=(9, 7, 8))
    dtype = torch.float32 if kind in ("strided", "columns") else getattr(torch, kind)
    vals = [[torch.from_numpy(x).to(dev).to(dtype) for x in u["feats"]] for u in b["utts"]]   # what the dtype holds is
    f32 = [[v.float().clone().requires_grad_(True) for v in vs] for vs in vals]              # exact in float32
    if kind == "strided":
        wide = [[torch.stack((v, -v), dim=1).reshape(2 * v.shape[0], v.shape[1])[::2].requires_grad_(True) for v in vs]
                for vs in vals]
        assert all(w.stride(0) == 2 * w.shape[1] for ws in wide for w in ws)
        call_w = wide
    elif kind == "columns":      # column slices of one [F x 80] tensor: the gradient arrives in the wide tensor
        wide = [torch.cat(vs, dim=1).requires_grad_(True) for vs in vals]
        call_w = [[w[:, :60], w[:, 60:70], w[:, 70:80]] for w in wide]
    else:
        wide = [[v.clone().requires_grad_(True) for v in vs] for vs in vals]
        call_w = wide
    res = {}
    for name, xs in (("wide", call_w), ("f32", f32)):
        wavs = _call(b, xs)
        res[name + "_wav"] = [w.detach() for w in wavs]
        _backward(b, wavs, dev)
    for u in range(len(vals)):
        assert torch.equal(res["wide_wav"][u], res["f32_wav"][u])
        g32 = [x.grad for x in f32[u]]
        assert all(g.dtype == torch.float32 and bool(g.any()) for g in g32[:1])
        if kind == "columns":
            gw = wide[u].grad
            assert gw.dtype == torch.float32 and gw.shape == wide[u].shape
            assert torch.equal(gw, torch.cat(g32, dim=1))
        else:
            for w, g in zip(wide[u], g32):
                assert w.grad.dtype == dtype and w.grad.shape == w.shape and torch.equal(w.grad, g.to(dtype))


def test_partial_gradients_and_determinism():
    dev = _engine().device
    b = _batch(2048, True, 45, True)
    gs = [g.double() for g in _gys(b, dev)]
    leaves = _leaves(b, dev)
    flat = [x for lv in leaves for x in lv]
    wavs = _call(b, leaves)
    g1 = torch.autograd.grad(wavs, flat, gs, retain_graph=True)
    g1b = torch.autograd.grad(wavs, flat, gs, retain_graph=True)               # a second backward pass: identical bits
    leaves2 = _leaves(b, dev)
    g2 = torch.autograd.grad(_call(b, leaves2), [x for lv in leaves2 for x in lv], gs)   # ... and a second forward
    assert all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(g1, g1b, g2)) and bool(g1[0].any())
    # magnitudes only: None elsewhere, the same bits
    mag_only = [[x.detach().requires_grad_(k == 0) for k, x in enumerate(lv)] for lv in leaves]
    torch.autograd.backward(_call(b, mag_only), gs)
    for u, lv in enumerate(mag_only):
        assert lv[1].grad is None and lv[2].grad is None and torch.equal(lv[0].grad, g1[3 * u])
    # one utterance only
    one = [[x.detach().requires_grad_(u == 2) for x in lv] for u, lv in enumerate(leaves)]
    torch.autograd.backward(_call(b, one), gs)
    assert all(x.grad is None for lv in one[:2] for x in lv)
    assert all(torch.equal(x.grad, g1[6 + k]) for k, x in enumerate(one[2]))


def test_silence_gives_finite_gradients():
    """m_mag_mel_log = -20 everywhere (no -inf): magnitudes of e^-20, finite gradients that match the model."""
    dev = _engine().device
    b = _make_batch(1024, False, 45, True, 43, mag_level=-20.0)
    _reference(b)
    leaves = _leaves(b, dev)
    wavs = _call(b, leaves)
    _backward(b, wavs, dev)
    _compare(b, leaves, "silence")


def test_uninitialised_scratch_is_never_read(monkeypatch):
    """Constant rate, an unvoiced utterance and unvoiced stretches: the forward leaves the phase rows nobody reads
    unwritten.  With every allocation of the engine poisoned with NaN during the backward pass the gradients are finite
    and equal the unpoisoned pass bit for bit."""
    e = _engine()
    dev = e.device
    b = _batch(1024, True, 45, True)
    leaves = _leaves(b, dev)
    _backward(b, _call(b, leaves), dev)
    clean = [x.grad.clone() for lv in leaves for x in lv]
    leaves = _leaves(b, dev)
    wavs = _call(b, leaves)
    real_empty = e.empty

    def poisoned(shape, dtype=None):
        t = real_empty(shape, dtype)
        return t.fill_(float("nan")) if t.is_floating_point() else t

    monkeypatch.setattr(e, "empty", poisoned)
    _backward(b, wavs, dev)
    monkeypatch.undo()
    got = [x.grad for lv in leaves for x in lv]
    assert all(bool(torch.isfinite(g).all()) for g in got)
    assert all(torch.equal(g, c) for g, c in zip(got, clean))


def test_what_has_no_backward_pass_says_so(monkeypatch):
    dev = _engine().device
    b = _batch(1024, False, 10, True)
    for kw, word in ((dict(per_phase_type="min_phase"), "per_phase_type"), (dict(per_phase_type="linear"), "per_phase_type"),
                     (dict(b_post_filter=True), "b_post_filter"), (dict(b_post_filter="merlin"), "b_post_filter"),
                     (dict(pcm16_norm=0.98), "pcm16_norm"), (dict(pcm16_norm=None), "pcm16_norm"),
                     (dict(prepared=object()), "prepared")):
        with pytest.raises(NotImplementedError, match=word):
            _call(b, _leaves(b, dev), **kw)
    # ... and only then: without grad the same calls run as before
    with torch.no_grad():
        w = _call(b, _leaves(b, dev), per_phase_type="linear")
    assert w[0].grad_fn is None
    w = _call(b, _leaves(b, dev, False), pcm16_norm=0.98)
    assert w[0].dtype == torch.int16
    # stored noise spectra are ignored by the backward pass: the same gradients, bit for bit
    b4 = _batch(4096, False, 10, True)
    lv = _leaves(b4, dev)
    _backward(b4, _call(b4, lv), dev)
    monkeypatch.setenv("MAGPHASE_NOISE_SPECTRA", "store")
    lv2 = _leaves(b4, dev)
    _backward(b4, _call(b4, lv2), dev)
    assert all(bool(torch.isfinite(y.grad).all()) for ys in lv2 for y in ys)
    _compare(b4, lv2, "stored noise spectra")


def test_composes_with_the_compressed_analysis_backward():
    """analysis_compressed_batch(synthesis_from_compressed_batch(x)): backward() reaches the three coefficient matrices."""
    N, pd, fs = 1024, 45, ana_model.FS
    dev = _engine().device
    b = _make_batch(N, False, pd, True, 51, kinds=("mixed", "voiced"), n_rows=(18, 14))
    assert b["fs"] == fs
    rng = np.random.RandomState(53)
    leaves = _leaves(b, dev)
    ys = _call(b, leaves)
    assert all(y.grad_fn is not None for y in ys)
    epochs = []
    for u in b["utts"]:
        t = u["tab"]
        pm = t["v_pm"] - t["start"]
        keep = (pm > 0) & (pm < t["out_len"] - 1)
        epochs.append((pm[keep] / float(fs), t["voiced"][keep]))
    out = mp.analysis_compressed_batch([(y, fs, pm_sec, voi) for y, (pm_sec, voi) in zip(ys, epochs)], fft_len=N, mag_dim=60,
                                       phase_dim=pd, return_device=True)
    wm, wp = ana_model.warps(N, phase_dim=pd)
    gup, pre = [], []
    for k, (u, o, (pm_sec, voi)) in enumerate(zip(b["utts"], out, epochs)):
        m = [torch.tensor(x, requires_grad=True) for x in u["feats"]]
        ym = model.forward_torch(m[0], m[1], m[2], u["tab"], b["cst"], u["ns"], u["inv"], True)
        tab = ana_model.tables(pm_sec, voi, int(ym.numel()), False)
        om = ana_model.forward_torch(ym, tab, N, wm, wp)
        g = [rng.randn(*o[j].shape).astype(np.float32) for j in range(3)]
        for j, msk in enumerate(ana_model.tie_mask(om[3].detach().numpy(), om[4].detach().numpy(), tab), start=1):
            g[j][msk] = 0.0
        sum((om[j] * torch.from_numpy(g[j].astype(np.float64))).sum() for j in range(3)).backward()
        gup.append(g), pre.append(m)
    torch.autograd.backward([o[j] for o in out for j in range(3)], [torch.from_numpy(g[j]).to(dev) for g in gup for j in range(3)])
    for u in range(len(b["utts"])):
        for j, name in enumerate(("m_mag_mel_log", "m_real_mel", "m_imag_mel")):
            got = leaves[u][j].grad.cpu().numpy()
            assert np.all(np.isfinite(got)) and got.any()
            err = model.rel_err(got, pre[u][j].grad.numpy())
            print("composition utterance %d %s: %.4g" % (u, name, err))
            within(err, TOL["compose"], "autograd_compressed_synthesis_compose")
