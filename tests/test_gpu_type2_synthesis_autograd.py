"""GPU: k_synth_comp_bwd's type-2 arm on its own against the float64 closed form, and tensor.backward() through
synthesis_from_compressed_type2_batch (magphase_amd/autograd.py, Type2SynthesisPlan.run_backward) against torch autograd of
the float64 model of tests/type2_synthesis_autograd_model.py, at the variable rate and on two grids, with the properties
the feature promises: the forward's samples do not change, partial gradients and repeated passes are exact, every input
dtype and stride gets its own gradient, unvoiced and silent frames give zeros and finite values, uninitialised scratch is
never read, pcm16_norm under grad says so, a type-1 plan on the same engine is not disturbed, and the synthesis composes
with the compressed analysis' backward pass."""
import numpy as np
import pytest
import torch

import compressed_analysis_autograd_model as ana_model
import compressed_synthesis_autograd_model as model1
import type2_synthesis_autograd_model as model
from _tol import within
from magphase_amd import magphase as mp

pytestmark = pytest.mark.gpu

# max |device - model| / max |model| per gradient matrix, no element left out (model.rel_err), against the float64 model.
# Stated at <= 3 x the worst case measured on an MI355X (profiles/r17_type2_synthesis_autograd_tolerance_report.json;
# DESIGN.md section 3.3l):
#   "kernel"   k_synth_comp_bwd<P, T2> alone against the closed form on the device's own float32 inputs: 4.14e-7 (the
#              project's tolerance for this kernel is type 1's 2.7e-6; the measurement came in 6.5 x below it, so it is
#              restated at 3 x measured);
#   "vs_type1" grad m of the type-2 entry against the type-1 entry's where the two agree in exact arithmetic (the bins
#              between the ends; the modulus at the ends of unvoiced frames): 7.68e-8;
#   "e2e"      synthesis_from_compressed_type2_batch against the model's autograd: 1.40e-5 (the float32 forward rows, the
#              float32 noise gain and the float32 adjoint of the elliptic filter are in it; the worst element is a phase
#              gradient, which carries 1 / |a + j b| of the float32 rows);
#   "compose"  type-2 synthesis + compressed analysis against the two float64 models chained: 3.00e-5.
TOL = {"kernel": 1.24e-6, "vs_type1": 2.3e-7, "e2e": 4.1e-5, "compose": 9.0e-5}


def _engine():
    from magphase_amd.engine import get_engine
    return get_engine()


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _up(dev, a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)


# ----------------------------------------------------------------------------------------------------------------------
# the frame kernel alone
# ----------------------------------------------------------------------------------------------------------------------
def _noise_spectrum(noise, pos, L, R, wt, N):
    """FFT_N of the windowed frame noise[pos - L .. pos + R] with its epoch at index 0 (the forward's Ns), float64."""
    seg = noise[pos - L:pos + R + 1] * model1._half_windows(L, R, bool(wt))
    m = np.zeros(N)
    m[N // 2 - L:N // 2 - L + seg.size] = seg
    return np.fft.fft(np.fft.fftshift(m))[:N // 2 + 1]


def _kernel_case(N, which=(True, True, True), seed=0):
    """The synthetic case of the type-1 kernel test (its shape: F = 21, a frame starting before the buffer and one ending
    after it, one with nothing kept, win_l == 0, a == b == 0 at bins including bin 0, unvoiced frames; NaN wherever the
    forward writes nothing, NaN sentinel rows and columns around every output) through
    mpx_synthesis_compressed_type2_backward.  Returns (worst error, grad m [F x H] of the type-2 entry, of the type-1
    entry on the same inputs, voiced)."""
    e = _engine()
    dev = e.device
    H, M = N // 2 + 1, N // 2
    rng = np.random.RandomState(200 + N + seed)
    F = 21                                   # three workgroups at 8 waves, six at 4
    n_per = int(0.37 * H)                    # not a multiple of 64
    n_phase = min((n_per + 63) // 64 * 64, H)
    ld = int(e.lib.mpx_spec_ld(H))
    nleft = rng.randint(1, M + 1, size=F)
    nright = rng.randint(1, M, size=F)
    nleft[3], nright[3] = M, M - 1           # the widest frame
    nleft[4], nright[4] = 1, 1               # the narrowest
    npos = np.cumsum(nleft + rng.randint(0, 40, size=F))
    noise = rng.uniform(-1, 1, int(npos[-1] + M + 8)).astype(np.float32)
    wtype = rng.randint(0, 2, size=F)
    voiced = (rng.rand(F) < 0.7).astype(np.int32)
    voiced[0], voiced[1], voiced[2] = 1, 0, 1
    wtype = wtype * voiced
    inv_gain = rng.uniform(0.05, 0.2, size=F).astype(np.float32)
    win_l = rng.randint(1, M + 1, size=F)
    win_r = rng.randint(1, M, size=F)
    win_l[2] = 0                                          # win_l == 0: the single rising sample weighs 1
    win_l[5], win_r[5] = M, M - 1
    total = 5 * N
    gpos = rng.randint(0, total - N, size=F).astype(np.int64)
    glo, ghi = np.zeros(F, dtype=np.int32), np.full(F, N, dtype=np.int32)
    gpos[0], glo[0] = -(M // 3), M // 3                         # starts before the buffer
    gpos[F - 1], ghi[F - 1] = total - M - 7, M + 7              # ends after it
    gpos[6], glo[6], ghi[6] = 1000 - 70, 70, 70 + 301
    gpos[7], glo[7], ghi[7] = 17, M + 3, M + 3                 # nothing kept at all
    gy = rng.randn(total).astype(np.float32)
    m = np.exp(rng.randn(F, H)).astype(np.float32)
    a, b = rng.randn(F, H).astype(np.float32), rng.randn(F, H).astype(np.float32)
    a[0, 3:40] = b[0, 3:40] = 0.0                         # a voiced frame with a == b == 0 at some bins
    a[2, 0] = b[2, 0] = 0.0                               # ... and at bin 0
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
    i32, i64 = np.int32, np.int64
    fixed = (N, e.tables(N), _up(dev, gy), total, _up(dev, gpos, i64), _up(dev, glo, i32), _up(dev, ghi, i32), F, d_m, d_a,
             d_b, ld, _up(dev, noise), _up(dev, npos, i64), _up(dev, nleft, i32), _up(dev, nright, i32),
             _up(dev, wtype, i32), _up(dev, voiced, i32), _up(dev, inv_gain), _up(dev, win_l, i32), _up(dev, win_r, i32),
             _up(dev, per_v), _up(dev, ap_v), _up(dev, ap_u), n_per)

    def launch(entry, which_):
        outs = [torch.full((F + 2, ld), float("nan"), dtype=torch.float32, device=dev) if w else None for w in which_]
        rows = [o[1:F + 1] if o is not None else None for o in outs]
        e.launch(entry, *fixed, rows[0], rows[1], rows[2], ld)
        torch.cuda.synchronize()
        return [o.cpu().numpy() if o is not None else None for o in outs]

    outs = launch("mpx_synthesis_compressed_type2_backward", which)
    type1_m = launch("mpx_synthesis_compressed_backward", (True, False, False))[0][1:F + 1, :H].astype(np.float64)
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
        w[M - win_l[f]:M + win_r[f] + 1] = model1._half_windows(int(win_l[f]), int(win_r[f]), False)
        gwin[f, lo:hi] = gy[gpos[f] + lo:gpos[f] + hi].astype(np.float64) * w[lo:hi]
    ref = model.frame_grads_closed(m.astype(np.float64), np.where(v, a, 0.0).astype(np.float64),
                                   np.where(v, b, 0.0).astype(np.float64), P,
                                   A * ns * inv_gain[:, None].astype(np.float64), gwin, N)
    worst, got_m = 0.0, None
    for k, name in enumerate(("grad m", "grad a", "grad b")):
        if not which[k]:
            assert outs[k] is None
            continue
        full = outs[k]
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
        within(err, TOL["kernel"], "autograd_type2_synthesis_kernel")
        worst = max(worst, err)
        if k == 0:
            got_m = got
        if k == 1:      # the den == 0 convention on the bins that were set to zero: m P gS
            assert np.any(got[0, 3:40] != 0.0)
        if k == 2:      # the phase gradient at bin 0 is not shortcut to zero
            nz = ref[2][:, 0] != 0.0      # (voiced, a_0 != 0, some windowed gradient under the frame)
            assert nz.sum() >= 5 and np.all(got[nz, 0] != 0.0) and not got[~nz, 0].any()
    return worst, got_m, type1_m, voiced


@pytest.mark.parametrize("N", [1024, 2048, 4096])
def test_frame_kernel_against_the_closed_form(N):
    """... and the arm does something: the grad m column at bin 0 and at bin N/2 is not what the type-1 entry returns on
    the same inputs.  Type 1 keeps |S| there and returns |T| sign(m) Re gS, type 2 keeps Re S and returns Re T Re gS: they
    differ wherever T is not a positive real -- in every voiced frame at bin 0 (P u is complex), and at bin N/2, where the
    noise spectrum is real and P is zero, in the frames whose Re T is negative.  Between the ends the two agree."""
    _, got_m, type1_m, voiced = _kernel_case(N)
    H = N // 2 + 1
    # (frame 2: a == b == 0 at bin 0, T is real; a frame whose window misses what is kept of it has a zero gradient)
    v0 = (voiced != 0) & (np.arange(voiced.size) != 2) & (got_m[:, 0] != 0.0)
    assert v0.sum() >= 5 and np.all(got_m[v0, 0] != type1_m[v0, 0])
    for k in (0, H - 1):
        assert not np.array_equal(got_m[:, k], type1_m[:, k]), k
        # unvoiced frames: T is real there, the two differ by the sign of Re T only
        within(model.rel_err(np.abs(got_m[voiced == 0, k]), np.abs(type1_m[voiced == 0, k])), TOL["vs_type1"],
               "autograd_type2_synthesis_kernel_vs_type1")
    within(model.rel_err(got_m[:, 1:-1], type1_m[:, 1:-1]), TOL["vs_type1"], "autograd_type2_synthesis_kernel_vs_type1")


@pytest.mark.parametrize("which", [(False, True, True), (True, False, True), (True, True, False), (True, False, False)])
def test_frame_kernel_null_outputs(which):
    _kernel_case(1024, which=which, seed=1)
    _kernel_case(4096, which=which, seed=1)


# ----------------------------------------------------------------------------------------------------------------------
# end to end
# ----------------------------------------------------------------------------------------------------------------------
_BATCH = {}
_KINDS = ("mixed", "unvoiced", "voiced")
_SEEDS = [5, 6, 7]


def _fs_of(N):
    return 48000 if N == 4096 else 16000


def _make_batch(N, rate, pd, hf, ap_win, seed, kinds=_KINDS, n_rows=(18, 14, 16), mag_dim=60, mag_level=None):
    fs = _fs_of(N)
    rng = np.random.RandomState(seed)
    cst = model.constants(fs, N, mag_dim, pd, hf)
    utts = []
    for kind, n in zip(kinds, n_rows):
        lf0 = model.lf0_track(rng, n, kind, fs)
        feats = [_f32(x) for x in model.features(rng, n, mag_dim, pd)]
        if mag_level is not None:
            feats[0][:] = mag_level
        tab = model.tables(lf0, fs, N, rate, ap_win)
        noise = _f32(rng.uniform(-1, 1, tab["ns_len"]))
        ns, inv = model.noise_spectra(noise, tab, N)
        gy = rng.randn(tab["out_len"]).astype(np.float32)
        utts.append(dict(lf0=lf0, feats=feats, tab=tab, noise=noise, ns=ns, inv=inv, gy=gy))
    return dict(fs=fs, N=N, rate=rate, pd=pd, hf=hf, cst=cst, utts=utts, ap_win=ap_win, device_noise=False)


def _use_device_noise(b):
    """noise_mode='device' (whose samples the model does not know): the model is evaluated on the noise the plan makes."""
    from magphase_amd.plans import Type2SynthesisPlan

    plan = Type2SynthesisPlan(_engine(), [tuple(u["feats"]) + (u["lf0"],) for u in b["utts"]], b["fs"], fft_len=b["N"],
                              hf_slope_coeff=b["hf"], b_voi_ap_win=b["ap_win"], const_rate_ms=b["rate"],
                              noise_mode="device", noise_seeds=_SEEDS)
    noise = plan.noise.cpu().numpy().astype(np.float64)
    for k, u in enumerate(b["utts"]):
        u["noise"] = noise[int(plan.noise_off_host[k]):int(plan.noise_off_host[k + 1])]
        u["ns"], u["inv"] = model.noise_spectra(u["noise"], u["tab"], b["N"])
    b["device_noise"] = True


def _reference(b):
    b["ref"] = [model.grads_autograd(*u["feats"], u["gy"], u["tab"], b["cst"], u["ns"], u["inv"]) for u in b["utts"]]
    for r in b["ref"]:
        for x in r:
            x.setflags(write=False)


def _batch(N, rate, pd, hf, ap_win, device_noise=False):
    """The gradient tests' batch (computed once, never modified): three utterances -- mixed, all unvoiced, all voiced --
    of 18, 14 and 16 rows, and the model's gradients."""
    key = (N, rate, pd, hf, ap_win, device_noise)
    if key not in _BATCH:
        b = _make_batch(N, rate, pd, hf, ap_win, N + pd + int(7 * rate) + int(10 * hf) + ap_win)
        if device_noise:
            _use_device_noise(b)
        _reference(b)
        _BATCH[key] = b
    return _BATCH[key]


def _leaves(b, dev, requires_grad=True, dtype=torch.float32):
    return [[torch.from_numpy(x).to(dev).to(dtype).requires_grad_(requires_grad) for x in u["feats"]] for u in b["utts"]]


def _call(b, leaves, **kw):
    kw.setdefault("return_device", True)
    if b["device_noise"]:
        kw.setdefault("noise_mode", "device")
        kw.setdefault("noise_seeds", _SEEDS)
    else:
        kw.setdefault("noise", [u["noise"] for u in b["utts"]])
    utts = [tuple(lv) + (u["lf0"],) for lv, u in zip(leaves, b["utts"])]
    return mp.synthesis_from_compressed_type2_batch(utts, b["fs"], fft_len=b["N"], hf_slope_coeff=b["hf"],
                                                    b_voi_ap_win=b["ap_win"], const_rate_ms=b["rate"], **kw)


def _gys(b, dev):
    return [torch.from_numpy(u["gy"]).to(dev) for u in b["utts"]]


def _backward(b, wavs, dev):
    torch.autograd.backward(wavs, [g.to(w.dtype) for g, w in zip(_gys(b, dev), wavs)])


def _compare(b, leaves, label, tol="e2e", name="autograd_type2_synthesis_e2e"):
    for u, lv in enumerate(leaves):
        for k, nm in enumerate(("m_mag_mel_log", "m_real_mel", "m_imag_mel")):
            got = lv[k].grad.cpu().numpy()
            ref = b["ref"][u][k]
            assert got.dtype == np.float32 and got.shape == ref.shape and np.all(np.isfinite(got))
            err = model.rel_err(got, ref)
            print("%s utterance %d %s: %.4g" % (label, u, nm, err))
            within(err, TOL[tol], name)


# fft_len (16 kHz for 1024 / 2048, 48 kHz for 4096), const_rate_ms, phase_dim (mag_dim 60), hf_slope_coeff, b_voi_ap_win,
# device noise: every value of every axis, every fft_len at every rate
_E2E = [(1024, -1.0, 45, 1.0, True, False), (1024, 5.0, 10, 1.7, True, False), (1024, 4.0, 60, 1.0, False, False),
        (1024, 5.0, 64, 1.7, True, False), (2048, -1.0, 10, 1.7, False, False), (2048, 5.0, 45, 1.0, True, True),
        (2048, 4.0, 45, 1.7, True, False), (4096, -1.0, 45, 1.7, True, True), (4096, 5.0, 45, 1.0, False, False),
        (4096, 4.0, 10, 1.0, True, False), (4096, -1.0, 64, 1.0, True, False)]


@pytest.mark.parametrize("N,rate,pd,hf,ap_win,device_noise", _E2E)
def test_gradients_match_the_float64_model(N, rate, pd, hf, ap_win, device_noise):
    dev = _engine().device
    b = _batch(N, rate, pd, hf, ap_win, device_noise)
    leaves = _leaves(b, dev)
    wavs = _call(b, leaves)
    for w, u in zip(wavs, b["utts"]):
        assert w.grad_fn is not None and w.dtype == torch.float64
        assert int(w.numel()) == u["tab"]["out_len"]
    _backward(b, wavs, dev)
    _compare(b, leaves, "fft_len %d rate %g phase_dim %d hf %g ap_win %s device noise %s" % (N, rate, pd, hf, ap_win,
                                                                                             device_noise))
    assert not leaves[1][1].grad.any() and not leaves[1][2].grad.any()       # the unvoiced utterance: exactly zero
    assert bool(leaves[0][1].grad.any()) and bool(leaves[2][2].grad.any())
    if pd > 60:     # phase_dim > mag_dim: u_phase has zero rows there, the gradient columns are exact zeros
        for lv in leaves:
            assert not lv[1].grad[:, 60:].any() and not lv[2].grad[:, 60:].any()
        assert bool(leaves[2][1].grad[:, :60].any())


def test_forward_is_unchanged():
    """Samples from a grad-requiring call are bit-identical to the plain device-tensor call and to the host-array call."""
    dev = _engine().device
    for rate in (-1.0, 5.0):
        b = _batch(2048, rate, 45, 1.0 if rate > 0 else 1.7, True, rate > 0)
        a = _call(b, _leaves(b, dev))
        with torch.no_grad():
            c = _call(b, _leaves(b, dev))
        d = _call(b, _leaves(b, dev, False))
        h = _call(b, [[x.astype(np.float32) for x in u["feats"]] for u in b["utts"]], return_device=False)
        for u in range(len(a)):
            assert a[u].grad_fn is not None and a[u].requires_grad and a[u].numel() > 0
            for y in (c[u], d[u]):
                assert y.grad_fn is None and not y.requires_grad and torch.equal(a[u].detach(), y)
            assert np.array_equal(a[u].detach().cpu().numpy(), h[u])
        hh = _call(b, _leaves(b, dev), return_device=False)          # a host return stays a detached numpy array
        assert all(isinstance(x, np.ndarray) for x in hh) and all(np.array_equal(x, y) for x, y in zip(hh, h))


@pytest.mark.parametrize("kind", ["bfloat16", "float16", "float64", "strided", "columns"])
def test_dtypes_and_strides_get_their_own_gradients(kind):
    dev = _engine().device
    b = _make_batch(1024, 5.0, 45, 1.0, True, 41, n_rows=(9, 7, 8))
    dtype = torch.float32 if kind in ("strided", "columns") else getattr(torch, kind)
    vals = [[torch.from_numpy(x).to(dev).to(dtype) for x in u["feats"]] for u in b["utts"]]   # what the dtype holds is
    f32 = [[v.float().clone().requires_grad_(True) for v in vs] for vs in vals]              # exact in float32
    if kind == "strided":
        wide = [[torch.stack((v, -v), dim=1).reshape(2 * v.shape[0], v.shape[1])[::2].requires_grad_(True) for v in vs]
                for vs in vals]
        assert all(w.stride(0) == 2 * w.shape[1] for ws in wide for w in ws)
        call_w = wide
    elif kind == "columns":      # column slices of one [F x 151] tensor: the gradient arrives in the wide tensor
        wide = [torch.cat(vs + [vs[0][:, :1]], dim=1).requires_grad_(True) for vs in vals]
        assert all(w.shape[1] == 151 for w in wide)
        call_w = [[w[:, :60], w[:, 60:105], w[:, 105:150]] for w in wide]
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
            assert torch.equal(gw[:, :150], torch.cat(g32, dim=1)) and not gw[:, 150].any()
        else:
            for w, g in zip(wide[u], g32):
                assert w.grad.dtype == dtype and w.grad.shape == w.shape and torch.equal(w.grad, g.to(dtype))


def test_partial_gradients_and_determinism():
    dev = _engine().device
    b = _batch(2048, 5.0, 45, 1.0, True, True)
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
    # no double backward
    lv3 = _leaves(b, dev)
    (g3,) = torch.autograd.grad(_call(b, lv3), [lv3[0][0]], gs, create_graph=True)
    assert g3.grad_fn is None and not g3.requires_grad and torch.equal(g3, g1[0])


def test_silence_gives_finite_gradients():
    """m_mag_mel_log = -20 everywhere (no -inf): magnitudes of e^-20, finite gradients that match the model."""
    dev = _engine().device
    b = _make_batch(1024, -1.0, 45, 1.0, True, 43, mag_level=-20.0)
    _reference(b)
    leaves = _leaves(b, dev)
    wavs = _call(b, leaves)
    _backward(b, wavs, dev)
    _compare(b, leaves, "silence")


def test_uninitialised_scratch_is_never_read(monkeypatch):
    """A grid, an unvoiced utterance and unvoiced stretches: the forward leaves the phase rows nobody reads unwritten.
    With every allocation of the engine poisoned with NaN during the backward pass the gradients are finite and equal the
    unpoisoned pass bit for bit."""
    e = _engine()
    dev = e.device
    b = _batch(1024, 5.0, 10, 1.7, True)
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


def test_what_has_no_backward_pass_says_so():
    dev = _engine().device
    b = _batch(1024, -1.0, 45, 1.0, True)
    for norm in (0.98, None):
        with pytest.raises(NotImplementedError, match="pcm16_norm"):
            _call(b, _leaves(b, dev), pcm16_norm=norm)
    # ... and only then: without grad the same call runs as before
    w = _call(b, _leaves(b, dev, False), pcm16_norm=0.98)
    assert w[0].dtype == torch.int16
    with torch.no_grad():
        w = _call(b, _leaves(b, dev), pcm16_norm=0.98)
    assert w[0].dtype == torch.int16
    with torch.no_grad():
        w = _call(b, _leaves(b, dev))
    assert w[0].grad_fn is None and w[0].dtype == torch.float64
    # more than 64 columns: k_mel_unwarp_bwd's limit, said by name before anything is launched
    wide = [[torch.zeros(u["feats"][0].shape[0], d, device=dev, requires_grad=True) for d in (60, 65, 65)]
            for u in b["utts"]]
    with pytest.raises(NotImplementedError, match="phase_dim"):
        _call(b, wide)


def test_type_1_plan_is_not_disturbed():
    """A type-1 backward pass after a type-2 one on the same engine gives the bits it gave before: the cached constants
    (unwarp matrices, curves, n_per, filter tables) are keyed apart."""
    dev = _engine().device
    N, pd = 1024, 45
    rng = np.random.RandomState(61)
    fs = _fs_of(N)
    utts1 = []
    for kind, n in zip(_KINDS, (12, 9, 10)):
        lf0 = model1.lf0_track(rng, n, kind, fs)
        feats = [np.asarray(x, dtype=np.float32) for x in model1.features(rng, n, 60, pd)]
        tab = model1.tables(lf0, fs, N, True, True)
        utts1.append(dict(lf0=lf0, feats=feats, noise=rng.uniform(-1, 1, tab["ns_len"])))

    def type1():
        lv = [[torch.from_numpy(x).to(dev).requires_grad_(True) for x in u["feats"]] for u in utts1]
        wavs = mp.synthesis_from_compressed_batch([tuple(l) + (u["lf0"],) for l, u in zip(lv, utts1)], fs, fft_len=N,
                                                  b_const_rate=True, noise=[u["noise"] for u in utts1], return_device=True)
        torch.autograd.backward(wavs, [torch.ones_like(w) for w in wavs])
        return [w.detach().clone() for w in wavs] + [x.grad for l in lv for x in l]

    before = type1()
    b = _batch(N, 5.0, pd, 1.7, True)
    leaves = _leaves(b, dev)
    _backward(b, _call(b, leaves), dev)
    assert bool(leaves[0][0].grad.any())
    after = type1()
    assert all(torch.equal(x, y) for x, y in zip(before, after)) and bool(before[-1].any())


def test_composes_with_the_compressed_analysis_backward():
    """analysis_compressed_batch(synthesis_from_compressed_type2_batch(x)): backward() reaches the coefficient matrices."""
    N, pd, fs = 1024, 45, ana_model.FS
    dev = _engine().device
    b = _make_batch(N, -1.0, pd, 1.0, True, 51, kinds=("mixed", "voiced"), n_rows=(18, 14))
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
        ym = model.forward_torch(m[0], m[1], m[2], u["tab"], b["cst"], u["ns"], u["inv"])
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
            within(err, TOL["compose"], "autograd_type2_synthesis_compose")
