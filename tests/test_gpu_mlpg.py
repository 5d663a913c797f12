"""GPU: k_mlpg_solve / k_mlpg_apply (mpx_mlpg_solve, mpx_mlpg_apply) and mp.mlpg_batch / dynamic_features_batch /
mlpg_streams_batch with their autograd, against tests/mlpg_model.py.

The solve is held to a DERIVED bound, for every system of every batch: with A and b formed in longdouble from the operands
as the kernel received them,
    backward error  eta = |b - A c|_inf / (|A|_inf |c|_inf + |b|_inf)  <=  16 x 2^-53
                    (at most 7 rounded terms per band entry, the bandwidth-2 factorisation, two substitutions)
    forward error   |c - c_model|_inf / |c_model|_inf                   <=  2 kappa_inf(A) x 16 x 2^-53
and the stencil to 4 x 2^-53 of sum |terms| per element (one product, two fused multiply-adds, one division).  The
fractions of these bounds that the MI355X reached are recorded through _tol.within (profiles/r21_mlpg_tolerance_report.json).

Gradients: the float64 gradient of the device (Engine.mlpg_streams_backward: the right-hand-side solve and the stencil) is
held, per system and relative to its largest element, to the forward-error bound plus the stencil bound against the float64
torch model; a leaf's .grad must then be exactly that gradient cast to the leaf's dtype (float32 leaves cannot be held to a
2^-53 bound themselves, and no wider one is used).

Shapes: frame counts 1, 2, 3, 4, 5, 63, 64, 65, 257 and an empty utterance in every batch (F = 1 next to F = 257, so that
for D = 10 utterance boundaries fall inside a wave), widths 1, 10, 60, 64, 65; every dimension has its own static-to-dynamic
variance ratio between 1e-8 and 1e8."""
import ctypes

import numpy as np
import pytest
import torch

import mlpg_model as mm
from _tol import within
from magphase_amd import libaudio as la
from magphase_amd import magphase as mp

pytestmark = pytest.mark.gpu

FRAMES = (1, 257, 2, 0, 3, 4, 5, 63, 64, 65)
NON_DEFAULT = ((0.25, -0.5, 0.75),)
SENT = -77.25
# D, windows, mean dtype, var dtype, per-frame variances, columns left / right of the slice in a wider mean matrix
CASES = (
    (1, mm.WINDOWS, np.float64, np.float64, False, 0),
    (10, mm.WINDOWS, np.float32, np.float32, True, 0),
    (60, mm.WINDOWS, np.float32, np.float64, False, 7),
    (64, mm.WINDOWS[:1], np.float64, np.float32, False, 0),
    (65, NON_DEFAULT, np.float64, np.float64, True, 3),
)


def _engine():
    from magphase_amd.engine import get_engine
    return get_engine()


def _operands(D, K, mdt, vdt, per_frame, seed, frames=FRAMES):
    """Means [total x K D] and variances ([K D] or [total x K D]) as float64 arrays holding values of mdt / vdt, and the
    frame offsets.  Dimension d has the static-to-dynamic variance ratio 10^r_d, r_d spread over [-8, 8]."""
    rng = np.random.default_rng(seed)
    offs = np.concatenate(([0], np.cumsum(frames))).astype(np.int64)
    total = int(offs[-1])
    mean = rng.normal(size=(total, K * D)).astype(mdt).astype(np.float64)
    var = np.exp(rng.normal(size=(total if per_frame else 1, K * D)))
    ratio = 10.0 ** (np.linspace(-8, 8, D) if D > 1 else np.array([3.0]))
    var[:, :D] *= rng.permutation(ratio)
    var = var.astype(vdt).astype(np.float64)
    return mean, (var if per_frame else var[0]), offs


def _per_system(mean, var, offs, D, K, u):
    """[F x K x D] means and variances of utterance u."""
    a, b = int(offs[u]), int(offs[u + 1])
    mu = mean[a:b].reshape(b - a, K, D)
    v = var[a:b].reshape(b - a, K, D) if var.ndim == 2 else np.broadcast_to(var.reshape(1, K, D), (b - a, K, D))
    return mu, v


def _tdt(dt):
    return torch.float64 if dt == np.float64 else torch.float32


def _guarded(e, rows, cols, ld, guard=64):
    buf = torch.full((guard + rows * ld + guard,), SENT, dtype=torch.float64, device=e.device)
    return buf, buf[guard:guard + rows * ld].view(rows, ld)[:, :cols]


def _check_guarded(buf, rows, cols, ld, what, guard=64):
    h = buf.cpu().numpy()
    assert np.all(h[:guard] == SENT) and np.all(h[guard + rows * ld:] == SENT), what + ": written outside the buffer"
    body = h[guard:guard + rows * ld].reshape(rows, ld)
    assert np.all(body[:, cols:] == SENT), what + ": written beyond a row's last column"
    return body[:, :cols]


def _launch_solve(e, mean, var, offs, D, windows, mdt, vdt, pad, rhs=False):
    """mpx_mlpg_solve on a column slice of a wider NaN-padded mean matrix, the output and the workspace inside
    sentinel-filled buffers -> c [total x D]; asserts that nothing outside was written."""
    w = np.asarray(windows, dtype=np.float64).reshape(-1, 3)
    K, total = w.shape[0] + 1, int(offs[-1])
    width = D if rhs else K * D
    wide = torch.full((total, pad + width + pad + 1), float("nan"), dtype=_tdt(mdt), device=e.device)
    wide[:, pad:pad + width] = torch.from_numpy(mean).to(e.device).to(_tdt(mdt))
    if var.ndim == 2:
        vd = torch.full((total, K * D + 2), float("nan"), dtype=_tdt(vdt), device=e.device)
        vd[:, :K * D] = torch.from_numpy(var).to(e.device).to(_tdt(vdt))
        vview, ld_v = vd[:, :K * D], K * D + 2
    else:
        vview, ld_v = torch.from_numpy(var).to(e.device).to(_tdt(vdt)), 0
    offs_dev = torch.from_numpy(offs.astype(np.int32)).to(e.device)
    ld_o = D + 3
    obuf, out = _guarded(e, total, D, ld_o)
    need = int(e.lib.mpx_mlpg_work_doubles(total, D))
    assert need == 2 * total * D
    wbuf = torch.full((64 + need + 64,), SENT, dtype=torch.float64, device=e.device)
    wins = (ctypes.c_double * w.size)(*w.reshape(-1))
    e.launch("mpx_mlpg_solve", wide[:, pad:], int(mdt == np.float64), wide.stride(0), vview, int(vdt == np.float64), ld_v,
             offs_dev, len(offs) - 1, total, D, K - 1, wins, int(rhs), out, ld_o, wbuf[64:])
    torch.cuda.synchronize()
    hw = wbuf.cpu().numpy()
    assert np.all(hw[:64] == SENT) and np.all(hw[64 + need:] == SENT), "workspace: written outside"
    return _check_guarded(obuf, total, D, ld_o, "out").copy()


def _hold_to_bounds(c, mean, var, offs, D, K, windows, label, rhs=False):
    worst = [0.0, 0.0]
    for u in range(len(offs) - 1):
        a, b = int(offs[u]), int(offs[u + 1])
        if b == a:
            continue
        mu, v = _per_system(np.zeros((int(offs[-1]), K * D)) if rhs else mean, var, offs, D, K, u)
        eta, fwd, _, _ = mm.band_errors(c[a:b], None if rhs else mu, v, windows, rhs=mean[a:b] if rhs else None)
        assert np.all(np.isfinite(c[a:b]))
        worst = [max(worst[0], float(eta.max())), max(worst[1], float(fwd.max()))]
    print("%s: eta %.3f of 16 u, forward error %.3f of 2 kappa 16 u" % (label, worst[0], worst[1]))
    within(worst[0], 1.0, "mlpg_solve_eta_fraction_of_bound")
    within(worst[1], 1.0, "mlpg_solve_forward_fraction_of_bound")


@pytest.mark.parametrize("case", CASES, ids=lambda c: "D%d" % c[0])
def test_solve_every_system_within_the_derived_bounds(case):
    D, windows, mdt, vdt, per_frame, pad = case
    e, K = _engine(), len(windows) + 1
    mean, var, offs = _operands(D, K, mdt, vdt, per_frame, 100 + D)
    c = _launch_solve(e, mean, var, offs, D, windows, mdt, vdt, pad)
    _hold_to_bounds(c, mean, var, offs, D, K, windows, "solve D=%d" % D)


@pytest.mark.parametrize("case", (CASES[1], CASES[4]), ids=lambda c: "D%d" % c[0])
def test_solve_with_the_right_hand_side_given(case):
    """rhs_direct (the backward pass' z = A^-1 g): the same bounds, b = the matrix handed in."""
    D, windows, mdt, vdt, per_frame, pad = case
    e, K = _engine(), len(windows) + 1
    _, var, offs = _operands(D, K, mdt, vdt, per_frame, 200 + D)
    g = np.random.default_rng(D).normal(size=(int(offs[-1]), D)).astype(mdt).astype(np.float64)
    z = _launch_solve(e, g, var, offs, D, windows, mdt, vdt, pad, rhs=True)
    _hold_to_bounds(z, g, var, offs, D, K, windows, "rhs solve D=%d" % D, rhs=True)


def _launch_apply(e, x, var, offs, D, windows, xdt, vdt):
    w = np.asarray(windows, dtype=np.float64).reshape(-1, 3)
    K, total = w.shape[0] + 1, int(offs[-1])
    xw = torch.full((total, D + 2), float("nan"), dtype=_tdt(xdt), device=e.device)
    xw[:, :D] = torch.from_numpy(x).to(e.device).to(_tdt(xdt))
    if var is None:
        vview, ld_v = None, 0
    elif var.ndim == 2:
        vview, ld_v = torch.from_numpy(var).to(e.device).to(_tdt(vdt)).contiguous(), K * D
    else:
        vview, ld_v = torch.from_numpy(var).to(e.device).to(_tdt(vdt)), 0
    ld_y = K * D + 5
    ybuf, y = _guarded(e, total, K * D, ld_y)
    wins = (ctypes.c_double * w.size)(*w.reshape(-1))
    e.launch("mpx_mlpg_apply", xw, int(xdt == np.float64), xw.stride(0), vview, int(vdt == np.float64), ld_v,
             torch.from_numpy(offs.astype(np.int32)).to(e.device), len(offs) - 1, total, D, K - 1, wins, y, ld_y)
    torch.cuda.synchronize()
    return _check_guarded(ybuf, total, K * D, ld_y, "y").copy()


def _apply_model(x, var, offs, D, K, windows, dtype=np.longdouble):
    """(model [total x K D] in dtype, sum |terms| likewise in float64)."""
    total = int(offs[-1])
    ref, mag = np.zeros((total, K * D), dtype=dtype), np.zeros((total, K * D))
    for u in range(len(offs) - 1):
        a, b = int(offs[u]), int(offs[u + 1])
        for d in range(D if b > a else 0):
            v = None
            if var is not None:
                v = _per_system(np.zeros((total, K * D)), var, offs, D, K, u)[1][:, :, d]
            ref[a:b, d::D] = mm.apply(x[a:b, d], v, windows, dtype)
            mag[a:b, d::D] = mm.apply_abs_terms(x[a:b, d], v, windows)
    return ref, mag


@pytest.mark.parametrize("case", CASES, ids=lambda c: "D%d" % c[0])
@pytest.mark.parametrize("with_var", (False, True))
def test_apply_against_the_model(case, with_var):
    D, windows, xdt, vdt, per_frame, _ = case
    e, K = _engine(), len(windows) + 1
    frames = FRAMES if D <= 10 else (1, 65, 0, 2, 3)
    _, var, offs = _operands(D, K, xdt, vdt, per_frame, 300 + D, frames)
    x = np.random.default_rng(D).normal(size=(int(offs[-1]), D)).astype(xdt).astype(np.float64)
    y = _launch_apply(e, x, var if with_var else None, offs, D, windows, xdt, vdt)
    ref, mag = _apply_model(x, var if with_var else None, offs, D, K, windows)
    err = np.abs(y.astype(np.longdouble) - ref).astype(np.float64)
    assert np.all(err[mag == 0] == 0)          # F = 1: the only tap of a dynamic window inside the utterance may be a zero
    within(float(np.max(err[mag > 0] / mag[mag > 0])) / mm.APPLY_BOUND, 1.0, "mlpg_apply_fraction_of_bound")


def test_apply_one_hot_matches_bit_for_bit():
    """x = one 1 per column: every output is one tap (divided by one variance), no sum is rounded."""
    e, D, K = _engine(), 10, 3
    frames = (1, 5, 0, 2, 66)
    _, var, offs = _operands(D, K, np.float64, np.float64, True, 7, frames)
    total = int(offs[-1])
    x = np.zeros((total, D))
    for d in range(D):
        x[(7 * d) % total, d] = 1.0
    for v in (None, var):
        y = _launch_apply(e, x, v, offs, D, mm.WINDOWS, np.float64, np.float64)
        ref, _ = _apply_model(x, v, offs, D, K, mm.WINDOWS, np.float64)
        assert np.array_equal(y, ref)


def _utt_list(mean, offs):
    return [mean[int(a):int(b)] for a, b in zip(offs[:-1], offs[1:])]


def test_batching_and_repetition_are_bit_identical():
    D, K = 10, 3
    mean, var, offs = _operands(D, K, np.float32, np.float64, True, 11)
    means, vars_ = _utt_list(mean.astype(np.float32), offs), _utt_list(var, offs)
    first = mp.mlpg_batch(means, vars_)
    again = mp.mlpg_batch(means, vars_)
    assert [c.shape for c in first] == [(f, D) for f in FRAMES] and all(c.dtype == np.float64 for c in first)
    for c1, c2 in zip(first, again):
        assert np.array_equal(c1, c2)
    for u in (0, 1, 4, 8):
        alone = mp.mlpg_batch([means[u]], [vars_[u]])[0]
        assert np.array_equal(alone, first[u]), u
    assert np.array_equal(mp.mlpg(means[1], vars_[1]), first[1])
    g = _operands(D, K, np.float32, np.float64, False, 12)[1]
    assert np.array_equal(mp.mlpg(means[1], g), mp.mlpg_batch(means, g)[1])
    assert mp.mlpg_batch([means[3]], g)[0].shape == (0, D)         # a batch without a frame: no launch
    assert mp.mlpg_batch([means[3]], g, return_device=True)[0].shape == (0, D)


def test_dynamic_features_then_mlpg_returns_the_static_input():
    e, D = _engine(), 10
    rng = np.random.default_rng(5)
    for windows in (mm.WINDOWS, NON_DEFAULT):
        K = len(windows) + 1
        xs = [rng.normal(size=(f, D)) for f in FRAMES]
        dyn = mp.dynamic_features_batch(xs, windows=windows)
        assert [m.shape for m in dyn] == [(f, K * D) for f in FRAMES]
        assert np.array_equal(mp.dynamic_features(xs[1], windows), dyn[1])
        _, var, offs = _operands(D, K, np.float64, np.float64, True, 21)
        back = mp.mlpg_batch(dyn, _utt_list(var, offs), windows=windows)
        worst = 0.0
        for u, (x, c) in enumerate(zip(xs, back)):
            if len(x) == 0:
                continue
            mu, v = _per_system(np.concatenate(dyn), var, offs, D, K, u)
            kappa = mm.band_errors(c, mu, v, windows)[2]
            frac = np.max(np.abs(c - x), axis=0) / np.max(np.abs(x), axis=0) / (2 * kappa * mm.SOLVE_BACKWARD_BOUND)
            worst = max(worst, float(frac.max()))
        within(worst, 1.0, "mlpg_of_dynamic_features_fraction_of_forward_bound")


# ------------------------------------------------------------------------------------------------------- autograd
def _grad_model(g, var, offs, D, K, windows):
    """float64 torch-free model of dL/dmean [total x K D] for g = dL/dc [total x D], and per (utterance, dimension) the
    allowance relative to the system's largest gradient element: 2 kappa 16 u + 4 u."""
    total = int(offs[-1])
    ref, allow = np.zeros((total, K * D)), np.zeros((len(offs) - 1, D))
    for u in range(len(offs) - 1):
        a, b = int(offs[u]), int(offs[u + 1])
        if b == a:
            continue
        _, v = _per_system(np.zeros((total, K * D)), var, offs, D, K, u)
        kappa = mm.band_errors(np.zeros((b - a, D)), None, v, windows, rhs=g[a:b])[2]
        allow[u] = 2 * kappa * mm.SOLVE_BACKWARD_BOUND + mm.APPLY_BOUND
        for d in range(D):
            ref[a:b, d::D] = mm.backward(g[a:b, d], v[:, :, d], windows)
    return ref, allow


@pytest.mark.parametrize("ldt", (torch.float32, torch.float64), ids=("f32", "f64"))
@pytest.mark.parametrize("per_frame", (False, True), ids=("global", "per_frame"))
def test_autograd_gradients_of_mlpg_batch(ldt, per_frame):
    e, D, K, pad = _engine(), 10, 3, 4
    frames = (1, 65, 2, 0, 5)
    ndt = np.float32 if ldt == torch.float32 else np.float64
    mean, var, offs = _operands(D, K, ndt, np.float64, per_frame, 31, frames)
    total = int(offs[-1])
    # leaves: wider matrices, the means a column slice of them
    leaves = [torch.zeros((f, pad + K * D + pad), dtype=ldt, device=e.device).requires_grad_(True) for f in frames]
    with torch.no_grad():
        for lf, m in zip(leaves, _utt_list(mean, offs)):
            lf[:, pad:pad + K * D] = torch.from_numpy(m).to(e.device).to(ldt)
    slices = [lf[:, pad:pad + K * D] for lf in leaves]
    if per_frame:
        v_arg = [torch.from_numpy(v).to(e.device).requires_grad_(True) for v in _utt_list(var, offs)]
    else:
        v_arg = torch.from_numpy(var).to(e.device).requires_grad_(True)
    out = mp.mlpg_batch(slices, v_arg, return_device=True)
    assert all(o.grad_fn is not None and o.dtype == torch.float64 for o in out)
    with torch.no_grad():
        plain = mp.mlpg_batch(slices, v_arg, return_device=True)
    host = mp.mlpg_batch([s.detach().cpu().numpy() for s in slices], var if not per_frame else _utt_list(var, offs))
    for o, p, h in zip(out, plain, host):
        assert p.grad_fn is None and torch.equal(o.detach(), p) and np.array_equal(p.cpu().numpy(), h)
    g = np.random.default_rng(3).normal(size=(total, D))
    gs = [torch.from_numpy(x).to(e.device) for x in _utt_list(g, offs)]
    torch.autograd.backward(out, gs)
    for v in (v_arg if per_frame else [v_arg]):
        assert v.grad is None                                   # variances get no gradient
    # the device's float64 gradient against the model, per system
    w = np.asarray(mm.WINDOWS, dtype=np.float64)
    vd = torch.from_numpy(var).to(e.device)
    g64 = e.mlpg_streams_backward(torch.from_numpy(g).to(e.device), vd, torch.from_numpy(offs.astype(np.int32)).to(e.device),
                                  [(0, D)], w, K * D)
    ref, allow = _grad_model(g, var, offs, D, K, mm.WINDOWS)
    h64 = g64.cpu().numpy()
    worst = 0.0
    for u in range(len(frames)):
        a, b = int(offs[u]), int(offs[u + 1])
        for d in range(D if b > a else 0):
            err = np.max(np.abs(h64[a:b, d::D] - ref[a:b, d::D])) / np.max(np.abs(ref[a:b, d::D]))
            worst = max(worst, err / allow[u, d])
    within(worst, 1.0, "mlpg_gradient_fraction_of_allowance")
    # every leaf: its own dtype and shape, exactly that gradient in the slice's columns, zero beside them
    for u, lf in enumerate(leaves):
        a, b = int(offs[u]), int(offs[u + 1])
        assert lf.grad is not None and lf.grad.dtype == ldt and lf.grad.shape == lf.shape
        assert torch.equal(lf.grad[:, pad:pad + K * D], g64[a:b].to(ldt))
        assert not lf.grad[:, :pad].any() and not lf.grad[:, pad + K * D:].any()


# ------------------------------------------------------------------------------------------------------- streams
_LAYOUT = (("mag", 60), ("real", 10), ("imag", 10), ("lf0", 1))


def _cmp_batch(frames, seed, fs=16000):
    """Acoustic-model-like rows [F x 244] (float64 values): consistent static / delta / acc means of plausible
    trajectories plus a little noise, the voicing column in stretches of 1 and 0, and one global variance."""
    import compressed_synthesis_autograd_model as csm

    rng = np.random.RandomState(seed)
    K, cmps, voiced = 3, [], []
    for f in frames:
        lf0 = csm.lf0_track(rng, f, "mixed", fs)
        voi = lf0 > 0
        stat = list(csm.features(rng, f, 60, 10)) + [np.where(voi, lf0, np.log(150.0))[:, None]]
        cols = []
        for s in stat:
            dyn = np.stack([mm.apply(s[:, d], None) for d in range(s.shape[1])], axis=2)      # [F x K x dim]
            cols.append((dyn + 0.01 * rng.randn(*dyn.shape)).reshape(f, K * s.shape[1]))
        cmps.append(np.concatenate(cols + [np.where(voi, 0.9, 0.1)[:, None]], axis=1))
        voiced.append(voi)
    var = np.exp(0.3 * rng.randn(K * 81 + 1))
    return cmps, var, voiced


def test_streams_equal_separate_mlpg_batches_and_threshold_lf0():
    e = _engine()
    frames = (9, 0, 33)
    cmps, var, voiced = _cmp_batch(frames, 1)
    res = mp.mlpg_streams_batch(cmps, var)
    dev = mp.mlpg_streams_batch([torch.from_numpy(c).to(e.device) for c in cmps], torch.from_numpy(var).to(e.device),
                                return_device=True)
    col = 0
    for s, (name, d) in enumerate(_LAYOUT):
        sep = mp.mlpg_batch([c[:, col:col + 3 * d] for c in cmps], var[col:col + 3 * d])
        for u, f in enumerate(frames):
            got = res[u][s]
            assert torch.is_tensor(dev[u][s]) and np.array_equal(dev[u][s].cpu().numpy(), got)   # host and device calls agree
            if name == "lf0":
                assert got.shape == (f,)
                want = np.where(voiced[u], sep[u][:, 0], la.f0_to_lf0(np.zeros(1))[0])      # -1e10 exactly where unvoiced
                assert np.array_equal(got, want) and (f == 0 or np.any(got == -1.0e10))
            else:
                assert got.shape == (f, d) and np.array_equal(got, sep[u])
        col += 3 * d
    # the threshold is "<=": a voicing value equal to it is unvoiced
    c2 = [c.copy() for c in cmps]
    c2[0][:, -1] = 0.5
    assert np.all(mp.mlpg_streams_batch(c2, var)[0][3] == -1.0e10)
    assert np.all(mp.mlpg_streams_batch(c2, var, vuv_thres=0.25)[0][3] > 0)
    # the tuples are what the synthesis takes, host arrays and device tensors alike
    keep = [0, 2]
    y_host = mp.synthesis_from_compressed_batch([res[u] for u in keep], 16000, fft_len=1024, noise_mode="device")
    y_dev = mp.synthesis_from_compressed_batch([dev[u] for u in keep], 16000, fft_len=1024, noise_mode="device",
                                               return_device=True)
    for yh, yd in zip(y_host, y_dev):
        assert len(yh) > 0 and np.all(np.isfinite(yh)) and yd.shape[0] == len(yh)


def test_end_to_end_gradient_through_mlpg_and_compressed_synthesis():
    """mlpg_streams_batch -> synthesis_from_compressed_batch -> backward(): finite, non-zero gradients on the means, equal
    to the model of the MLPG stage applied to the gradients the synthesis gave its own inputs."""
    e, K = _engine(), 3
    frames = (24, 17)
    cmps, var, _ = _cmp_batch(frames, 2)
    leaves = [torch.from_numpy(c).to(e.device).requires_grad_(True) for c in cmps]
    tuples = mp.mlpg_streams_batch(leaves, var, return_device=True)
    for t in tuples:
        for x in t[:3]:
            assert x.grad_fn is not None
            x.retain_grad()
    ys = mp.synthesis_from_compressed_batch(tuples, 16000, fft_len=1024, noise_mode="device", return_device=True)
    assert all(y.grad_fn is not None for y in ys)
    rng = np.random.default_rng(9)
    loss = sum((y * torch.from_numpy(rng.normal(size=y.shape[0])).to(y)).sum() for y in ys)
    loss.backward()
    worst = 0.0
    for u, (lf, t) in enumerate(zip(leaves, tuples)):
        got = lf.grad.cpu().numpy()
        assert lf.grad.dtype == torch.float64 and got.shape == cmps[u].shape
        assert np.all(np.isfinite(got)) and np.any(got != 0)
        offs = np.array([0, frames[u]], dtype=np.int64)
        col = 0
        for s, (name, d) in enumerate(_LAYOUT[:3]):
            g = t[s].grad.cpu().numpy()
            assert np.any(g != 0)
            ref, allow = _grad_model(g, var[col:col + K * d], offs, d, K, mm.WINDOWS)
            for dd in range(d):
                err = np.max(np.abs(got[:, col + dd:col + K * d:d] - ref[:, dd::d])) / np.max(np.abs(ref[:, dd::d]))
                worst = max(worst, err / allow[0, dd])
            col += K * d
        assert not got[:, col:].any()          # lf0 (not differentiable in the synthesis) and the voicing column
    within(worst, 1.0, "mlpg_end_to_end_gradient_fraction_of_allowance")
