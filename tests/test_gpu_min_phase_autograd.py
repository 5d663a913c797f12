"""GPU: k_min_phase_bwd on its own (mpx_min_phase_backward) against the float64 model of
tests/min_phase_autograd_model.py fed the device's own float32 rows; synthesis_from_mag_batch's samples against
synthesis_from_compressed_batch(per_phase_type='min_phase' / 'linear'), bit for bit; tensor.backward() through it against
torch autograd of the float64 model (tests/compressed_synthesis_autograd_model.py with the min-phase stage in front), for
both phases, both frame rates, with and without the output high-pass, every input dtype and a column slice; uninitialised
scratch is never read; la.build_min_phase_from_mag_spec_batch against the single call and its gradients against the model;
what has no backward pass says so."""
import numpy as np
import pytest
import torch

import compressed_synthesis_autograd_model as cs_model
import min_phase_autograd_model as model
from _tol import within
from magphase_amd import libaudio as la
from magphase_amd import magphase as mp

pytestmark = pytest.mark.gpu

# Against the float64 model, no row or bin left out.  Stated at <= 3 x the worst case measured on an MI355X
# (profiles/r23_min_phase_autograd_tolerance_report.json):
#   "kernel"  k_min_phase_bwd alone, per row max |device - model| / max |model| of the row (model.rel_err_rows), the model
#             fed the device's own float32 rows: 4.91e-6 (the worst of 2 051 log-normal rows at fft_len 1024, where a row's
#             largest |g_mag| sits on a bin with a small magnitude; 4.1e-6 for one-hot phase gradients, 2.1e-7 to 7.8e-7
#             for the handful of dense rows of the small cases);
#   "e2e"     synthesis_from_mag_batch against the model's autograd, max |device - model| / max |model| per gradient
#             matrix (the float32 forward rows, the float32 noise gains and the float32 adjoint of the output high-pass
#             are in it): 4.47e-7;
#   "la"      la.build_min_phase_from_mag_spec_batch's gradients against the model on the float32 magnitudes, per row as
#             "kernel" (the forward's float32 phase is in it): 9.60e-7.
TOL = {"kernel": 1.47e-5, "e2e": 1.34e-6, "la": 2.88e-6}


def _engine():
    from magphase_amd.engine import get_engine
    return get_engine()


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _up(dev, a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)


# ----------------------------------------------------------------------------------------------------------------------
# the kernel alone
# ----------------------------------------------------------------------------------------------------------------------
def _padded(dev, x, rows, ld, row0=0):
    """x in rows [row0, row0 + len(x)) of a NaN-filled [rows x ld] buffer."""
    buf = torch.full((rows, ld), float("nan"), dtype=torch.float32, device=dev)
    buf[row0:row0 + x.shape[0], :x.shape[1]] = _up(dev, x)
    return buf


def _forward_rows(e, N, m):
    """mpx_min_phase on the float32 rows m -> the three [F x ld] device buffers (NaN beyond column H) and ld."""
    dev = e.device
    F, H = m.shape
    ld = int(e.lib.mpx_spec_ld(H))
    src = _padded(dev, m, F, ld)
    outs = [torch.full((F, ld), float("nan"), dtype=torch.float32, device=dev) for _ in range(3)]
    ident = torch.arange(F, dtype=torch.int32, device=dev)
    e.launch("mpx_min_phase", N, e.tables(N), src, ident, ident, torch.zeros(F, dtype=torch.float32, device=dev), F,
             outs[0], outs[1], outs[2], ld)
    return outs, ld


def _kernel_case(N, F, kind="dense", n_phase=None, null=(), in_place=False, seed=0):
    e = _engine()
    dev = e.device
    H, M = N // 2 + 1, N // 2
    n_phase = H if n_phase is None else n_phase
    rng = np.random.RandomState(1000 + N + 7 * F + seed)
    m = np.exp(2.0 * rng.randn(F, H)).astype(np.float32)
    if kind == "zero_mag":
        m[F // 2, 37] = 0.0
    rows, ld = _forward_rows(e, N, m)
    g = [rng.randn(F, H).astype(np.float32) for _ in range(3)]
    if kind == "onehot":          # frame f: g_a / g_b one-hot at one interior bin
        bins = [1, 63, 64, M - 1]
        for k in (1, 2):
            v = np.zeros((F, H), dtype=np.float32)
            for f in range(F):
                v[f, bins[f % 4]] = g[k][f, bins[f % 4]]
            g[k] = v
    elif kind == "ends":          # one-hot at bins 0 and M: the phase there is 0 whatever the magnitude
        for k in (1, 2):
            v = np.zeros((F, H), dtype=np.float32)
            v[0::3, 0] = g[k][0::3, 0]
            v[1::3, M] = g[k][1::3, M]
            v[2::3, 0], v[2::3, M] = g[k][2::3, 0], g[k][2::3, M]
            g[k] = v
    ldg = ld + 8
    g_dev = []
    for k in range(3):
        x = g[k].copy()
        if k > 0:
            x[:, n_phase:] = np.nan                         # not read
        g_dev.append(None if k in null else _padded(dev, x, F, ldg))
    ref_g = [None if k in null else g[k] for k in range(3)]
    if in_place:
        ldo = ldg
        out = _padded(dev, g[0], F + 2, ldg, row0=1)        # g_m inside sentinel rows, and the output
        g_dev[0] = out[1:F + 1]
    else:
        ldo = ld + 4
        out = torch.full((F + 2, ldo), float("nan"), dtype=torch.float32, device=dev)

    def launch():
        e.launch("mpx_min_phase_backward", N, e.tables(N), rows[0], rows[1], rows[2], ld, g_dev[0], g_dev[1], g_dev[2], ldg,
                 n_phase, F, out[1:F + 1], ldo)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    full = launch()
    if not in_place:
        assert np.array_equal(full, launch(), equal_nan=True)               # deterministic
    assert np.all(np.isnan(full[0])) and np.all(np.isnan(full[F + 1]))      # sentinel rows
    assert np.all(np.isnan(full[1:F + 1, H:]))                              # nothing beyond column H - 1
    got = full[1:F + 1, :H]
    assert np.all(np.isfinite(got))
    dr = [r.cpu().numpy()[:, :H].astype(np.float64) for r in rows]
    assert np.array_equal(dr[0], m.astype(np.float64))
    ref = model.backward_rows(dr[0], dr[1], dr[2], ref_g[0], ref_g[1], ref_g[2], n_phase=n_phase)
    err = model.rel_err_rows(got, ref)
    print("fft_len %d frames %d %s n_phase %d null %s in_place %s: %.4g" % (N, F, kind, n_phase, null, in_place, err))
    within(err, TOL["kernel"], "autograd_min_phase_kernel")
    if kind == "ends" or 1 in null and 2 in null or n_phase <= 1:
        assert np.array_equal(got, g[0] if 0 not in null else np.zeros_like(got))      # g_m bit for bit
    if kind == "zero_mag":
        assert got[F // 2, 37] == g[0][F // 2, 37] and np.any(got[F // 2] != g[0][F // 2])
    if kind == "onehot":
        assert np.all(np.any(got != g[0], axis=1))                                     # every frame got a phase term
    return err


def _second_trip_frames(e):
    """One more than a workgroup's 8 waves times the largest grid (one workgroup per compute unit), and a bit."""
    return 8 * torch.cuda.get_device_properties(e.device).multi_processor_count + 3


@pytest.mark.parametrize("F", [1, 3, 4, 5])
@pytest.mark.parametrize("N", [1024, 2048, 4096])
def test_kernel_dense_gradients(N, F):
    _kernel_case(N, F)


@pytest.mark.parametrize("N", [1024, 2048, 4096])
def test_kernel_second_trip_of_the_grid_stride_loop(N):
    _kernel_case(N, _second_trip_frames(_engine()))


@pytest.mark.parametrize("kind", ["onehot", "ends", "zero_mag"])
@pytest.mark.parametrize("N", [1024, 2048, 4096])
def test_kernel_special_gradients(N, kind):
    _kernel_case(N, 9, kind=kind)


@pytest.mark.parametrize("N", [1024, 2048, 4096])
def test_kernel_columns_from_n_phase_on_are_not_read(N):
    H = N // 2 + 1
    for n_phase in (0, 1, 64, 100, min((int(0.37 * H) + 63) // 64 * 64, H), H - 1):
        _kernel_case(N, 5, n_phase=n_phase, seed=n_phase)


@pytest.mark.parametrize("null", [(1, 2), (0,), (1,), (2,), (0, 1, 2)])
def test_kernel_null_gradient_pointers(null):
    _kernel_case(1024, 5, null=null)
    _kernel_case(4096, 3, null=null)


@pytest.mark.parametrize("N", [1024, 2048, 4096])
def test_kernel_in_place(N):
    """grad_mag == grad_m: the same bits as the separate output."""
    a = _kernel_case(N, 11, in_place=True)
    b = _kernel_case(N, 11, in_place=False)
    assert a == b


# ----------------------------------------------------------------------------------------------------------------------
# the forward: the samples of the compressed synthesis with that per_phase_type
# ----------------------------------------------------------------------------------------------------------------------
_KINDS = ("mixed", "unvoiced")
_ROWS = (12, 7)
_BATCH = {}


def _fs_of(N):
    return 48000 if N == 4096 else 16000


def _make_batch(N, cr, hpf, seed):
    fs = _fs_of(N)
    rng = np.random.RandomState(seed)
    cst = cs_model.constants(fs, N, 60, 10)
    utts = []
    for kind, n in zip(_KINDS, _ROWS):
        lf0 = cs_model.lf0_track(rng, n, kind, fs)
        a_mag, a_real, a_imag = (_f32(x) for x in cs_model.features(rng, n, 60, 10))
        tab = cs_model.tables(lf0, fs, N, cr, True)
        noise = _f32(rng.uniform(-1, 1, tab["ns_len"]))
        ns, inv = cs_model.noise_spectra(noise, tab, N)
        gy = rng.randn(tab["out_len"]).astype(np.float32)
        utts.append(dict(lf0=lf0, a_mag=a_mag, a_real=a_real, a_imag=a_imag, tab=tab, noise=noise, ns=ns, inv=inv, gy=gy))
    return dict(fs=fs, N=N, cr=cr, hpf=hpf, cst=cst, utts=utts, ref={})


def _batch(N, cr, hpf):
    """Two utterances of 12 and 7 rows -- voiced and unvoiced stretches, all unvoiced -- computed once, never modified."""
    key = (N, cr, hpf)
    if key not in _BATCH:
        _BATCH[key] = _make_batch(N, cr, hpf, 5 + N + 7 * cr + hpf)
    return _BATCH[key]


def _reference(b, phase):
    if phase not in b["ref"]:
        r = [model.grads_autograd(u["a_mag"], u["gy"], u["tab"], b["cst"], u["ns"], u["inv"], phase, b["hpf"])
             for u in b["utts"]]
        for x in r:
            x.setflags(write=False)
        b["ref"][phase] = r
    return b["ref"][phase]


def _leaves(b, dev, requires_grad=True, dtype=torch.float32):
    return [torch.from_numpy(u["a_mag"]).to(dev).to(dtype).requires_grad_(requires_grad) for u in b["utts"]]


def _call(b, mags, phase, **kw):
    kw.setdefault("return_device", True)
    if kw.get("noise_mode") != "device":
        kw.setdefault("noise", [u["noise"] for u in b["utts"]])
    return mp.synthesis_from_mag_batch([(m, u["lf0"]) for m, u in zip(mags, b["utts"])], b["fs"], fft_len=b["N"], phase=phase,
                                       b_const_rate=b["cr"], b_out_hpf=b["hpf"], **kw)


def _call_compressed(b, phase, dev, **kw):
    kw.setdefault("return_device", True)
    if kw.get("noise_mode") != "device":
        kw.setdefault("noise", [u["noise"] for u in b["utts"]])
    utts = [(_up(dev, u["a_mag"]), _up(dev, u["a_real"]), _up(dev, u["a_imag"]), u["lf0"]) for u in b["utts"]]
    return mp.synthesis_from_compressed_batch(utts, b["fs"], fft_len=b["N"], b_const_rate=b["cr"], b_out_hpf=b["hpf"],
                                              per_phase_type={"min_phase": "min_phase", "zero": "linear"}[phase], **kw)


@pytest.mark.parametrize("phase", ["min_phase", "zero"])
@pytest.mark.parametrize("N,cr,hpf", [(1024, False, True), (1024, True, True), (1024, False, False), (1024, True, False),
                                      (4096, True, True)])
def test_forward_is_the_compressed_synthesis_with_that_phase_type(N, cr, hpf, phase):
    dev = _engine().device
    b = _batch(N, cr, hpf)
    with torch.no_grad():
        ref = _call_compressed(b, phase, dev)                                     # arbitrary phase matrices
        got = _call(b, _leaves(b, dev, False), phase)
        ref_d = _call_compressed(b, phase, dev, noise_mode="device", noise_seeds=[11, 12])
        got_d = _call(b, _leaves(b, dev, False), phase, noise_mode="device", noise_seeds=[11, 12])
    for u, utt in enumerate(b["utts"]):
        assert got[u].dtype == (torch.float64 if hpf else torch.float32) and int(got[u].numel()) == utt["tab"]["out_len"]
        assert torch.equal(got[u], ref[u]) and bool(got[u].any())
        assert torch.equal(got_d[u], ref_d[u]) and not torch.equal(got_d[u], got[u])
    # host arrays in, host arrays out; the grad-requiring call: the same samples
    host = _call(b, [u["a_mag"] for u in b["utts"]], phase, return_device=False)
    grad = _call(b, _leaves(b, dev), phase)
    for u in range(len(host)):
        assert isinstance(host[u], np.ndarray) and host[u].dtype == np.float64
        assert np.array_equal(host[u], got[u].cpu().numpy().astype(np.float64))
        assert grad[u].grad_fn is not None and torch.equal(grad[u].detach(), got[u])
    if N == 1024 and cr and hpf:
        one = mp.synthesis_from_mag(b["utts"][0]["a_mag"], b["utts"][0]["lf0"], b["fs"], fft_len=N, phase=phase,
                                    b_const_rate=cr)
        assert isinstance(one, np.ndarray) and one.shape == host[0].shape and np.all(np.isfinite(one))


# ----------------------------------------------------------------------------------------------------------------------
# end-to-end gradients
# ----------------------------------------------------------------------------------------------------------------------
def _gys(b, dev):
    return [torch.from_numpy(u["gy"]).to(dev) for u in b["utts"]]


def _backward(b, wavs, dev):
    torch.autograd.backward(wavs, [g.to(w.dtype) for g, w in zip(_gys(b, dev), wavs)])


def _compare(b, leaves, phase, label):
    ref = _reference(b, phase)
    for u, lv in enumerate(leaves):
        got = lv.grad.cpu().numpy()
        assert got.dtype == np.float32 and got.shape == ref[u].shape and np.all(np.isfinite(got)) and got.any()
        err = cs_model.rel_err(got, ref[u])
        print("%s utterance %d: %.4g" % (label, u, err))
        within(err, TOL["e2e"], "autograd_min_phase_e2e")


@pytest.mark.parametrize("phase", ["min_phase", "zero"])
@pytest.mark.parametrize("N,cr,hpf", [(1024, False, True), (1024, True, True), (1024, False, False), (1024, True, False),
                                      (4096, True, True), (2048, False, True)])
def test_gradients_match_the_float64_model(N, cr, hpf, phase):
    dev = _engine().device
    b = _batch(N, cr, hpf)
    leaves = _leaves(b, dev)
    wavs = _call(b, leaves, phase)
    for w, u in zip(wavs, b["utts"]):
        assert w.grad_fn is not None and w.dtype == (torch.float64 if hpf else torch.float32)
    _backward(b, wavs, dev)
    _compare(b, leaves, phase, "fft_len %d const_rate %s hpf %s %s" % (N, cr, hpf, phase))


def test_min_phase_gradient_is_not_the_zero_phase_one():
    """The phase term is there: on the voiced utterance the two phases' gradients differ by far more than the tolerance."""
    dev = _engine().device
    b = _batch(1024, False, True)
    a, z = _reference(b, "min_phase")[0], _reference(b, "zero")[0]
    assert cs_model.rel_err(a, z) > 100 * TOL["e2e"]
    lv = _leaves(b, dev)
    _backward(b, _call(b, lv, "min_phase"), dev)
    assert cs_model.rel_err(lv[0].grad.cpu().numpy(), z) > 100 * TOL["e2e"]


@pytest.mark.parametrize("cr", [False, True])
def test_zero_phase_gradient_is_the_magphase_path_with_a_unit_phasor(cr):
    """CompressedSynthesisPlan(per_phase_type='magphase') with its unwarped phase rows overwritten by 1 + 0j:
    run_backward's magnitude gradient is the 'zero' plan's."""
    from magphase_amd.plans import CompressedSynthesisPlan, MagnitudeSynthesisPlan

    e = _engine()
    dev = e.device
    b = _batch(1024, cr, False)
    noise = [u["noise"] for u in b["utts"]]
    pc = CompressedSynthesisPlan(e, [(u["a_mag"], u["a_real"], u["a_imag"], u["lf0"]) for u in b["utts"]], b["fs"],
                                 fft_len=1024, b_const_rate=cr, noise=noise)
    pm = MagnitudeSynthesisPlan(e, [(u["a_mag"], u["lf0"]) for u in b["utts"]], b["fs"], fft_len=1024, phase="zero",
                                b_const_rate=cr, noise=noise)
    pc.run()
    pm.run()
    pc._buf["spec"][1].fill_(1.0)
    pc._buf["spec"][2].fill_(0.0)
    g = torch.cat(_gys(b, dev)).contiguous()
    ref = pc.run_backward(g, need=(True, False, False))[0]
    got = pm.run_backward(g)
    assert got.shape == ref.shape and bool(got.any())
    err = cs_model.rel_err(got.cpu().numpy(), ref.cpu().numpy())
    print("zero phase against the magphase path, const_rate %s: %.4g" % (cr, err))
    within(err, TOL["e2e"], "autograd_min_phase_e2e")


@pytest.mark.parametrize("phase", ["min_phase", "zero"])
@pytest.mark.parametrize("kind", ["bfloat16", "float16", "float64", "columns"])
def test_dtypes_and_column_slices_get_their_own_gradients(kind, phase):
    dev = _engine().device
    b = _batch(1024, True, True)
    dtype = torch.float32 if kind == "columns" else getattr(torch, kind)
    vals = [torch.from_numpy(u["a_mag"]).to(dev).to(dtype) for u in b["utts"]]     # what the dtype holds is exact in float32
    f32 = [v.float().clone().requires_grad_(True) for v in vals]
    if kind == "columns":        # columns 3 .. 62 of a [F x 70] tensor: the gradient arrives in the wide tensor
        wide = [torch.cat((torch.ones_like(v[:, :3]), v, torch.ones_like(v[:, :7])), dim=1).requires_grad_(True) for v in vals]
        call_w = [w[:, 3:63] for w in wide]
    else:
        wide = [v.clone().requires_grad_(True) for v in vals]
        call_w = wide
    wav = {}
    for name, xs in (("wide", call_w), ("f32", f32)):
        wavs = _call(b, xs, phase)
        wav[name] = [w.detach() for w in wavs]
        _backward(b, wavs, dev)
    for u in range(len(vals)):
        assert torch.equal(wav["wide"][u], wav["f32"][u])
        g32 = f32[u].grad
        assert g32.dtype == torch.float32 and bool(g32.any())
        gw = wide[u].grad
        assert gw.dtype == dtype and gw.shape == wide[u].shape
        if kind == "columns":
            assert torch.equal(gw[:, 3:63], g32) and not gw[:, :3].any() and not gw[:, 63:].any()
        else:
            assert torch.equal(gw, g32.to(dtype))


@pytest.mark.parametrize("phase", ["min_phase", "zero"])
def test_uninitialised_scratch_is_never_read(monkeypatch, phase):
    """With every allocation of the engine poisoned with NaN during the backward pass the gradients are finite and equal
    the unpoisoned pass bit for bit (which is also: two passes give the same bits)."""
    e = _engine()
    dev = e.device
    b = _batch(1024, True, True)
    leaves = _leaves(b, dev)
    _backward(b, _call(b, leaves, phase), dev)
    clean = [x.grad.clone() for x in leaves]
    leaves = _leaves(b, dev)
    wavs = _call(b, leaves, phase)
    real_empty = e.empty

    def poisoned(shape, dtype=None):
        t = real_empty(shape, dtype)
        return t.fill_(float("nan")) if t.is_floating_point() else t

    monkeypatch.setattr(e, "empty", poisoned)
    _backward(b, wavs, dev)
    monkeypatch.undo()
    got = [x.grad for x in leaves]
    assert all(bool(torch.isfinite(g).all()) for g in got)
    assert all(torch.equal(g, c) for g, c in zip(got, clean))


# ----------------------------------------------------------------------------------------------------------------------
# la.build_min_phase_from_mag_spec_batch
# ----------------------------------------------------------------------------------------------------------------------
def test_min_phase_batch_equals_the_single_call():
    rng = np.random.RandomState(77)
    mats = [np.exp(rng.randn(n, 513)) for n in (3, 1, 6)]
    out = la.build_min_phase_from_mag_spec_batch(mats)
    for m, o in zip(mats, out):
        one = la.build_min_phase_from_mag_spec(m)
        assert o.dtype == np.complex128 and o.shape == m.shape and np.array_equal(o, one)
    dev = _engine().device
    pairs = la.build_min_phase_from_mag_spec_batch([_up(dev, m) for m in mats], return_device=True)
    for (re, im), o in zip(pairs, out):
        assert re.dtype == torch.float32 and re.grad_fn is None
        assert np.allclose(re.cpu().numpy(), o.real, rtol=1e-6, atol=0) and np.allclose(im.cpu().numpy(), o.imag, rtol=1e-6, atol=1e-12)
    assert la.build_min_phase_from_mag_spec_batch([]) == []


@pytest.mark.parametrize("H", [513, 2049])
def test_min_phase_batch_gradients_match_the_model(H):
    dev = _engine().device
    rng = np.random.RandomState(H)
    mats = [np.exp(rng.randn(n, H)).astype(np.float32) for n in (4, 2)]
    w = [(rng.randn(*m.shape).astype(np.float32), rng.randn(*m.shape).astype(np.float32)) for m in mats]
    leaves = [_up(dev, m).requires_grad_(True) for m in mats[:1]] + [_up(dev, mats[1]).double().requires_grad_(True)]
    pairs = la.build_min_phase_from_mag_spec_batch(leaves, return_device=True)
    loss = sum((re * _up(dev, wr).to(re.dtype)).sum() + (im * _up(dev, wi).to(im.dtype)).sum() for (re, im), (wr, wi) in zip(pairs, w))
    assert all(re.grad_fn is not None for re, _ in pairs)
    loss.backward()
    for m, (wr, wi), lv in zip(mats, w, leaves):
        m64, wr, wi = m.astype(np.float64), wr.astype(np.float64), wi.astype(np.float64)
        mm, c, s = model.min_phase_rows(m64)
        ref = wr * c + wi * s + model.backward_rows(mm, c, s, None, wr * m64, wi * m64)
        got = lv.grad
        assert got.dtype == lv.dtype and got.shape == lv.shape
        err = model.rel_err_rows(got.cpu().numpy(), ref)
        print("H %d rows %d: %.4g" % (H, m.shape[0], err))
        within(err, TOL["la"], "autograd_min_phase_la_batch")


# ----------------------------------------------------------------------------------------------------------------------
# refusals
# ----------------------------------------------------------------------------------------------------------------------
def test_what_has_no_backward_pass_says_so():
    dev = _engine().device
    b = _batch(1024, False, True)
    for kw, word in ((dict(b_post_filter=True), "b_post_filter"), (dict(b_post_filter="merlin"), "b_post_filter"),
                     (dict(pcm16_norm=0.98), "pcm16_norm"), (dict(pcm16_norm=None), "pcm16_norm")):
        with pytest.raises(NotImplementedError, match=word):
            _call(b, _leaves(b, dev), "min_phase", **kw)
    wide = [torch.zeros((u["a_mag"].shape[0], 65), device=dev, requires_grad=True) for u in b["utts"]]
    with pytest.raises(NotImplementedError, match="mag_dim"):
        _call(b, wide, "zero")
    for bad in ("linear", "magphase", ""):
        with pytest.raises(ValueError, match="phase"):
            _call(b, _leaves(b, dev), bad)
    # ... and only then: without grad the same calls run
    w = _call(b, _leaves(b, dev, False), "min_phase", pcm16_norm=0.98)
    assert w[0].dtype == torch.int16
    with torch.no_grad():
        w = _call(b, _leaves(b, dev), "zero", b_post_filter=True)
    assert w[0].grad_fn is None
    # the compressed synthesis keeps its refusal
    utts = [(lv, _up(dev, u["a_real"]), _up(dev, u["a_imag"]), u["lf0"]) for lv, u in zip(_leaves(b, dev), b["utts"])]
    for ppt in ("min_phase", "linear"):
        with pytest.raises(NotImplementedError, match="per_phase_type"):
            mp.synthesis_from_compressed_batch(utts, b["fs"], fft_len=1024, per_phase_type=ppt, return_device=True,
                                               noise=[u["noise"] for u in b["utts"]])
