"""GPU: the MLPG variance gradients and the trajectory likelihood -- k_mlpg_var_bwd, the column pass, k_mlpg_nll and
k_mlpg_nll_bwd through their C entries, and mp.mlpg_batch / mlpg_streams_batch(var_grad=True) and
mp.mlpg_trajectory_nll_batch with their autograd -- against tests/mlpg_variance_model.py (longdouble, every system of every
batch, fed the operands as the kernel received them; tests/test_mlpg_variance_host.py holds that model to torch autograd).

Tolerances.
  k_mlpg_var_bwd      DERIVED, per element: with Sz = sum_j |w_k[j] z[t + j]| and Sc likewise, both stencils carry at most
                      mm.APPLY_BOUND of those sums, mu - W_k c one rounding, p^2 three, the two outer products two:
                          |error| <= p^2 Sz (|mu| + Sc) (2 mm.APPLY_BOUND + 6 u).
                      Through the API z and c are themselves computed: their forward bounds 2 kappa mm.SOLVE_BACKWARD_BOUND
                      (relative to the largest element of the system) carry through the product of the two stencils,
                          + p^2 |w_k|_1 (dz (|mu| + Sc) + Sz dc),   dz = 2 kappa 16 u max|z|,   dc = 2 kappa 16 u max|c|.
  the column pass     exact: partial sums of 128 rows in ascending order, then the partials in ascending order, are plain
                      float64 additions, which numpy reproduces bit for bit.
  NLL, its gradients  MEASURED on an MI355X against the longdouble model, per system, in units of kappa_inf(A) 2^-53 |NLL|
                      (the gradients: of kappa_inf(A) 2^-53 times the largest element of the system's model gradient), and
                      held at <= 3 x the worst case (the *_CONSTANT below; profiles/r26_mlpg_variance_tolerance_report.json).
                      The C entries are compared on the trajectory c they received (of a preceding mpx_mlpg_solve launch),
                      the API against the model's own trajectory.

Shapes: frame counts 0, 1, 2, 3, 4, 5, 8, 9, 16, 17, 63, 64, 65, 257 in every batch (the truncated windows, the last two rows
of the recursion, the chunk-ahead edges; an empty utterance), widths 1, 3, 60, 64, 65 (the wave edge of lane-per-system),
one and two windows, float32 / float64 operands, column slices of wider NaN-padded matrices, global and per-frame
variances; dimension d has its own static-to-dynamic variance ratio between 1e-8 and 1e8 (D = 3: 1e-8, 1, 1e8)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mlpg_model as mm
import mlpg_variance_model as vm
from _tol import within
from magphase_amd import magphase as mp

pytestmark = pytest.mark.gpu

FRAMES = (1, 257, 2, 0, 3, 4, 5, 8, 9, 16, 17, 63, 64, 65)
NON_DEFAULT = ((0.25, -0.5, 0.75),)
SENT = -77.25
# D, windows, mean dtype, var dtype, target dtype, per-frame variances, columns left / right of the slice in a wider matrix
CASES = (
    (1, mm.WINDOWS, np.float64, np.float64, np.float64, False, 0),
    (3, mm.WINDOWS, np.float32, np.float32, np.float32, True, 0),
    (60, mm.WINDOWS, np.float32, np.float64, np.float64, False, 7),
    (64, mm.WINDOWS[:1], np.float64, np.float32, np.float32, False, 0),
    (65, NON_DEFAULT, np.float64, np.float64, np.float32, True, 3),
)
_ids = lambda c: "D%d" % c[0]
# measured worst cases on an MI355X (see the module docstring), each constant <= 3 x its measurement
NLL_CONSTANT = 140.0              # measured 48.4
NLL_G_MEAN_CONSTANT = 7.0         # measured 2.41
NLL_G_VAR_CONSTANT = 90.0         # measured 31.6
NLL_API_CONSTANT = 4600.0         # measured 1542: the trajectory's own forward error enters through |A e|, and the terms of
#                                   the NLL (the quadratic form, the log-determinant) cancel in some systems
NLL_API_G_MEAN_CONSTANT = 360.0   # measured 121.4
NLL_API_G_VAR_CONSTANT = 119.0    # measured 39.8


def _engine():
    from magphase_amd.engine import get_engine
    return get_engine()


def _t(a):
    return torch.from_numpy(np.array(a))      # (a copy: the shared operands are read-only)


def _tdt(dt):
    return torch.float64 if dt == np.float64 else torch.float32


@functools.lru_cache(maxsize=None)
def _operands(D, K, mdt, vdt, xdt, per_frame, seed, frames=FRAMES):
    """Means [total x K D], variances ([K D] or [total x K D]), static targets, dL/dc and trajectory-like z, c [total x D] as
    float64 arrays holding values of their dtypes, the frame offsets and the upstream gradient of the NLL [n_utts x D].
    Dimension d has the static-to-dynamic variance ratio 10^r_d, r_d spread over [-8, 8]."""
    rng = np.random.default_rng(seed)
    offs = np.concatenate(([0], np.cumsum(frames))).astype(np.int64)
    total = int(offs[-1])
    mean = rng.normal(size=(total, K * D)).astype(mdt).astype(np.float64)
    var = np.exp(rng.normal(size=(total if per_frame else 1, K * D)))
    ratio = 10.0 ** (np.linspace(-8, 8, D) if D > 1 else np.array([3.0]))
    var[:, :D] *= rng.permutation(ratio)
    var = var.astype(vdt).astype(np.float64)
    x = (mean[:, :D] + 0.5 * rng.normal(size=(total, D))).astype(xdt).astype(np.float64)
    g, z, c = (rng.normal(size=(total, D)) for _ in range(3))
    go = rng.normal(size=(len(frames), D))
    for a in (mean, var, x, g, z, c, offs, go):
        a.setflags(write=False)
    return mean, (var if per_frame else var[0]), x, g, z, c, offs, go


def _sys(a, offs, u, K, D):
    """Rows of utterance u of a [total x K D] (or global [K D]) array as [F x K x D]."""
    lo, hi = int(offs[u]), int(offs[u + 1])
    if a.ndim == 1:
        return np.broadcast_to(a.reshape(1, K, D), (hi - lo, K, D))
    return a[lo:hi].reshape(hi - lo, K, D)


def _utts(offs):
    return [(u, int(offs[u]), int(offs[u + 1])) for u in range(len(offs) - 1) if offs[u + 1] > offs[u]]


def _fenced(e, a, dt, pad, tail=2):
    """A device view of `a` inside a wider NaN-filled matrix (pad columns left, pad + tail right)."""
    rows, cols = a.shape
    wide = torch.full((rows, pad + cols + pad + tail), float("nan"), dtype=_tdt(dt), device=e.device)
    wide[:, pad:pad + cols] = _t(np.ascontiguousarray(a)).to(e.device).to(_tdt(dt))
    return wide[:, pad:pad + cols]


def _dev_var(e, var, vdt, pad=0):
    return _fenced(e, var, vdt, pad) if var.ndim == 2 else _t(np.array(var)).to(e.device).to(_tdt(vdt))


def _guarded(e, rows, cols, ld, guard=64):
    buf = torch.full((guard + rows * ld + guard,), SENT, dtype=torch.float64, device=e.device)
    return buf, buf[guard:guard + rows * ld].view(rows, ld)[:, :cols]


def _check_guarded(buf, rows, cols, ld, what, guard=64):
    h = buf.cpu().numpy()
    assert np.all(h[:guard] == SENT) and np.all(h[guard + rows * ld:] == SENT), what + ": written outside the buffer"
    body = h[guard:guard + rows * ld].reshape(rows, ld)
    assert np.all(body[:, cols:] == SENT), what + ": written beyond a row's last column"
    return body[:, :cols].copy()


def _wins(windows):
    w = np.asarray(windows, dtype=np.float64).reshape(-1)
    return (ctypes.c_double * w.size)(*w)


def _offs_dev(e, offs):
    return _t(offs.astype(np.int32)).to(e.device)


def _colsum_emulation(x):
    """The column pass on a host float64 matrix, bit for bit."""
    total, width = x.shape
    sums = np.zeros(width)
    for a in range(0, total, 128):
        part = np.zeros(width)
        for r in range(a, min(a + 128, total)):
            part = part + x[r]
        sums = sums + part
    return sums


# ------------------------------------------------------------------------------------------------------- the C entries
def _launch_var_bwd(e, case, seed):
    D, windows, mdt, vdt, xdt, per_frame, pad = case
    K = len(windows) + 1
    mean, var, _, _, z, c, offs, _ = _operands(D, K, mdt, vdt, xdt, per_frame, seed)
    total = int(offs[-1])
    md, vd = _fenced(e, mean, mdt, pad), _dev_var(e, var, vdt)
    zd, cd = _fenced(e, z, np.float64, 1), _fenced(e, c, np.float64, 2)
    ld_g = K * D + 5
    gbuf, g = _guarded(e, total, K * D, ld_g)
    sbuf, gsum = _guarded(e, 1, K * D, K * D)
    need = int(e.lib.mpx_mlpg_colsum_work_doubles(total, K * D))
    assert need == (total + 127) // 128 * K * D
    wbuf, work = _guarded(e, 1, need, need)
    e.launch("mpx_mlpg_var_backward", zd, zd.stride(0), cd, cd.stride(0), md, int(mdt == np.float64), md.stride(0), vd,
             int(vdt == np.float64), vd.stride(0) if per_frame else 0, _offs_dev(e, offs), len(offs) - 1, total, D, K - 1,
             _wins(windows), g, ld_g, None if per_frame else gsum, None if per_frame else work)
    torch.cuda.synchronize()
    got = _check_guarded(gbuf, total, K * D, ld_g, "g")
    sums = _check_guarded(sbuf, 1, K * D, K * D, "gsum")[0]
    _check_guarded(wbuf, 1, need, need, "work")
    return got, sums


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_var_backward_entry_within_the_derived_allowance(case):
    D, windows, mdt, vdt, xdt, per_frame, pad = case
    e, K = _engine(), len(windows) + 1
    mean, var, _, _, z, c, offs, _ = _operands(D, K, mdt, vdt, xdt, per_frame, 400 + D)
    got, sums = _launch_var_bwd(e, case, 400 + D)
    worst = 0.0
    for u, lo, hi in _utts(offs):
        ref, allow = vm.var_bwd_entry_model(z[lo:hi], c[lo:hi], _sys(mean, offs, u, K, D), _sys(var, offs, u, K, D), windows)
        err = np.abs(got[lo:hi].reshape(hi - lo, K, D).astype(np.longdouble) - ref).astype(np.float64)
        assert np.all(err[allow == 0] == 0)
        worst = max(worst, float(np.max(err[allow > 0] / allow[allow > 0])))
    print("var_bwd D=%d: %.3f of the allowance" % (D, worst))
    within(worst, 1.0, "mlpg_var_bwd_fraction_of_allowance")
    if per_frame:
        assert np.all(sums == SENT)                              # no column pass for per-frame variances
    else:
        assert np.array_equal(sums, _colsum_emulation(got))      # the global row: the column sums of g, bit for bit
        again = _launch_var_bwd(e, case, 400 + D)
        assert np.array_equal(again[0], got) and np.array_equal(again[1], sums)


@pytest.mark.parametrize("total", (1, 127, 128, 129, 514))
def test_column_sums_are_the_fixed_order_sums(total):
    e, width, ld = _engine(), 5, 7
    x = np.random.default_rng(total).normal(size=(total, width)) * 10.0 ** np.arange(-8, 12, 4)
    xd = _fenced(e, x, np.float64, 1, tail=0)
    assert xd.stride(0) == ld
    need = int(e.lib.mpx_mlpg_colsum_work_doubles(total, width))
    runs = []
    for _ in range(2):
        sbuf, sums = _guarded(e, 1, width, width)
        wbuf, work = _guarded(e, 1, need, need)
        e.launch("mpx_mlpg_column_sums", xd, ld, total, width, sums, work)
        torch.cuda.synchronize()
        _check_guarded(wbuf, 1, need, need, "work")
        runs.append(_check_guarded(sbuf, 1, width, width, "sums")[0])
    assert np.array_equal(runs[0], _colsum_emulation(x)) and np.array_equal(runs[0], runs[1])
    assert np.array_equal(e.mlpg_column_sums(xd).cpu().numpy(), runs[0])


def _solve_on_device(e, md, vd, offs, D, windows):
    return e.mlpg_solve(md, vd, _offs_dev(e, offs), D, np.asarray(windows, dtype=np.float64).reshape(-1, 3))


def _launch_nll(e, case, seed):
    """-> (nll [n_utts x D], the trajectory the kernel received [total x D])."""
    D, windows, mdt, vdt, xdt, per_frame, pad = case
    K = len(windows) + 1
    mean, var, x, _, _, _, offs, _ = _operands(D, K, mdt, vdt, xdt, per_frame, seed)
    total, n = int(offs[-1]), len(offs) - 1
    md, vd, xd = _fenced(e, mean, mdt, pad), _dev_var(e, var, vdt), _fenced(e, x, xdt, pad)
    c = _solve_on_device(e, md, vd, offs, D, windows)
    cd = _fenced(e, c.cpu().numpy(), np.float64, 1)
    nbuf, nll = _guarded(e, n, D, D)
    e.launch("mpx_mlpg_trajectory_nll", cd, cd.stride(0), xd, int(xdt == np.float64), xd.stride(0), vd,
             int(vdt == np.float64), vd.stride(0) if per_frame else 0, _offs_dev(e, offs), n, total, D, K - 1,
             _wins(windows), nll)
    torch.cuda.synchronize()
    return _check_guarded(nbuf, n, D, D, "nll"), c.cpu().numpy()


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_trajectory_nll_entry_against_the_longdouble_model(case):
    D, windows, mdt, vdt, xdt, per_frame, pad = case
    e, K = _engine(), len(windows) + 1
    mean, var, x, _, _, _, offs, _ = _operands(D, K, mdt, vdt, xdt, per_frame, 500 + D)
    nll, c = _launch_nll(e, case, 500 + D)
    assert np.all(np.isfinite(nll)) and np.all(nll[FRAMES.index(0)] == 0)          # an utterance without frames: zeros
    worst = 0.0
    for u, lo, hi in _utts(offs):
        m = vm.band_model(_sys(mean, offs, u, K, D), _sys(var, offs, u, K, D), x=x[lo:hi], windows=windows, c=c[lo:hi])
        ref = m["nll"].astype(np.float64)
        err = np.abs(nll[u].astype(np.longdouble) - m["nll"]).astype(np.float64)
        worst = max(worst, float(np.max(err / (m["kappa"] * vm.U * np.abs(ref)))))
    print("nll D=%d: %.4g of kappa u |NLL|" % (D, worst))
    within(worst, NLL_CONSTANT, "mlpg_nll_over_kappa_u_nll")
    assert np.array_equal(_launch_nll(e, case, 500 + D)[0], nll)


def _launch_nll_bwd(e, case, seed, want=(True, True)):
    D, windows, mdt, vdt, xdt, per_frame, pad = case
    K = len(windows) + 1
    mean, var, x, _, _, _, offs, go = _operands(D, K, mdt, vdt, xdt, per_frame, seed)
    total, n = int(offs[-1]), len(offs) - 1
    md, vd, xd = _fenced(e, mean, mdt, pad), _dev_var(e, var, vdt), _fenced(e, x, xdt, pad)
    c = _solve_on_device(e, md, vd, offs, D, windows)
    cd = _fenced(e, c.cpu().numpy(), np.float64, 1)
    ld_gm, ld_gv = K * D + 1, K * D + 4
    mbuf, gm = _guarded(e, total, K * D, ld_gm)
    vbuf, gv = _guarded(e, total, K * D, ld_gv)
    need = int(e.lib.mpx_mlpg_nll_work_doubles(total, D))
    assert need == 3 * total * D
    wbuf, work = _guarded(e, 1, need, need)
    e.launch("mpx_mlpg_trajectory_nll_backward", md, int(mdt == np.float64), md.stride(0), vd, int(vdt == np.float64),
             vd.stride(0) if per_frame else 0, cd, cd.stride(0), xd, int(xdt == np.float64), xd.stride(0),
             _t(np.ascontiguousarray(go)).to(e.device), _offs_dev(e, offs), n, total, D, K - 1, _wins(windows),
             gm if want[0] else None, ld_gm, gv if want[1] else None, ld_gv, work if want[1] else None)
    torch.cuda.synchronize()
    _check_guarded(wbuf, 1, need, need, "work")
    return (_check_guarded(mbuf, total, K * D, ld_gm, "g_mean"), _check_guarded(vbuf, total, K * D, ld_gv, "g_var"),
            c.cpu().numpy())


def _hold_nll_grads(gm, gv, c, mean, var, x, go, offs, D, K, windows, labels, constants):
    worst = [0.0, 0.0]
    for u, lo, hi in _utts(offs):
        m = vm.band_model(_sys(mean, offs, u, K, D), _sys(var, offs, u, K, D), x=x[lo:hi], go=go[u], windows=windows,
                          c=None if c is None else c[lo:hi])
        for j, (got, key) in enumerate(((gm, "nll_g_mean"), (gv, "nll_g_var"))):
            if got is None:
                continue
            ref = m[key]
            err = np.max(np.abs(got[lo:hi].reshape(hi - lo, K, D).astype(np.longdouble) - ref), axis=(0, 1)).astype(np.float64)
            top = np.max(np.abs(ref), axis=(0, 1)).astype(np.float64)
            assert np.all(err[top == 0] == 0)
            ok = top > 0
            worst[j] = max(worst[j], float(np.max(err[ok] / (m["kappa"][ok] * vm.U * top[ok]))) if np.any(ok) else 0.0)
    print("%s %.4g, %s %.4g (of kappa u max|gradient|)" % (labels[0], worst[0], labels[1], worst[1]))
    if gm is not None:
        within(worst[0], constants[0], labels[0])
    if gv is not None:
        within(worst[1], constants[1], labels[1])


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_trajectory_nll_backward_entry_against_the_longdouble_model(case):
    D, windows, mdt, vdt, xdt, per_frame, pad = case
    e, K = _engine(), len(windows) + 1
    mean, var, x, _, _, _, offs, go = _operands(D, K, mdt, vdt, xdt, per_frame, 600 + D)
    gm, gv, c = _launch_nll_bwd(e, case, 600 + D)
    assert np.all(np.isfinite(gm)) and np.all(np.isfinite(gv))
    _hold_nll_grads(gm, gv, c, mean, var, x, go, offs, D, K, windows,
                    ("mlpg_nll_g_mean_over_kappa_u_max", "mlpg_nll_g_var_over_kappa_u_max"),
                    (NLL_G_MEAN_CONSTANT, NLL_G_VAR_CONSTANT))
    # either output alone: the same bits, the other buffer and (without g_var) the workspace untouched
    gm1, gv1, _ = _launch_nll_bwd(e, case, 600 + D, want=(True, False))
    assert np.array_equal(gm1, gm) and np.all(gv1 == SENT)
    gm2, gv2, _ = _launch_nll_bwd(e, case, 600 + D, want=(False, True))
    assert np.array_equal(gv2, gv) and np.all(gm2 == SENT)


# ------------------------------------------------------------------------------------------------------------ the API
def _utt_list(a, offs):
    return [a[int(lo):int(hi)] for lo, hi in zip(offs[:-1], offs[1:])]


def _traj_allowance(m, mu, var, windows):
    """The allowance of the variance gradient of <g, c> through the API (module docstring), [F x K x S] float64, for the
    model m = vm.band_model(..., g=...) of one utterance."""
    w = mm.taps(windows)
    z, c = m["z"].astype(np.float64), m["c"].astype(np.float64)
    _, entry = vm.var_bwd_entry_model(z, c, mu, var, windows)
    fwd = 2 * m["kappa"] * mm.SOLVE_BACKWARD_BOUND
    dz, dc = fwd * np.max(np.abs(z), axis=0), fwd * np.max(np.abs(c), axis=0)
    allow = np.zeros(np.shape(var))
    for k in range(w.shape[0]):
        p2 = 1.0 / np.asarray(var[:, k], dtype=np.float64) ** 2
        sz, sc = vm._stencil(np.abs(w[k]), np.abs(z)), vm._stencil(np.abs(w[k]), np.abs(c))
        allow[:, k] = p2 * np.sum(np.abs(w[k])) * (dz * (np.abs(mu[:, k]) + sc) + sz * dc)
    return allow + entry


@pytest.mark.parametrize("ldt", (torch.float32, torch.float64), ids=("f32", "f64"))
@pytest.mark.parametrize("per_frame", (False, True), ids=("global", "per_frame"))
@pytest.mark.parametrize("mean_grad", (False, True), ids=("var_only", "mean_and_var"))
def test_var_grad_of_mlpg_batch(ldt, per_frame, mean_grad):
    e, D, K, pad = _engine(), 10, 3, 4
    frames = (1, 65, 2, 0, 5, 129)
    ndt = np.float32 if ldt == torch.float32 else np.float64
    mean, var, _, g, _, _, offs, _ = _operands(D, K, ndt, ndt, ndt, per_frame, 31, frames)
    total = int(offs[-1])
    leaves = [torch.zeros((f, pad + K * D + pad), dtype=ldt, device=e.device).requires_grad_(mean_grad) for f in frames]
    with torch.no_grad():
        for lf, m in zip(leaves, _utt_list(mean, offs)):
            lf[:, pad:pad + K * D] = _t(m).to(e.device).to(ldt)
    slices = [lf[:, pad:pad + K * D] for lf in leaves]

    def variances():
        if per_frame:
            return [_t(v).to(e.device).to(ldt).requires_grad_(True) for v in _utt_list(var, offs)]
        return _t(np.array(var)).to(e.device).to(ldt).requires_grad_(True)

    gs = [_t(x).to(e.device) for x in _utt_list(g, offs)]
    # var_grad=False: today's behaviour -- the variances get no gradient, the same forward bits
    v_off = variances()
    plain = mp.mlpg_batch(slices, v_off, return_device=True)
    if mean_grad:
        torch.autograd.backward(plain, gs)
        for lf in leaves:
            lf.grad = None
    else:
        assert all(o.grad_fn is None for o in plain)
    assert all(v.grad is None for v in (v_off if per_frame else [v_off]))
    # var_grad=True
    v_arg = variances()
    out = mp.mlpg_batch(slices, v_arg, return_device=True, var_grad=True)
    assert all(o.grad_fn is not None and o.dtype == torch.float64 for o in out)
    for o, p in zip(out, plain):
        assert torch.equal(o.detach(), p.detach())
    with torch.no_grad():
        assert all(o.grad_fn is None for o in mp.mlpg_batch(slices, v_arg, return_device=True, var_grad=True))
    torch.autograd.backward(out, gs)
    # the device's float64 gradient against the model, every element
    w = np.asarray(mm.WINDOWS, dtype=np.float64)
    vd = _t(np.array(var)).to(e.device).to(ldt)
    buf = _t(mean).to(e.device).to(ldt)
    offs_dev = _offs_dev(e, offs)
    c_dev = e.mlpg_streams(buf, vd, offs_dev, [(0, D)], w)
    g_mean64, gv64 = e.mlpg_streams_var_backward(_t(g).to(e.device), buf, c_dev, vd, offs_dev, [(0, D)], w,
                                                 K * D, need_mean=mean_grad)
    plane = gv64 if per_frame else e.mlpg_var_backward(
        e.mlpg_solve(_t(g).to(e.device), vd, offs_dev, D, w, rhs=True), c_dev, buf, vd, offs_dev, D, w)[0]
    h = plane.cpu().numpy()
    worst, ref_all, allow_all = 0.0, np.zeros((total, K * D), dtype=np.longdouble), np.zeros((total, K * D))
    for u, lo, hi in _utts(offs):
        mu_u, var_u = _sys(mean, offs, u, K, D), _sys(var, offs, u, K, D)
        m = vm.band_model(mu_u, var_u, g=g[lo:hi])
        allow = _traj_allowance(m, mu_u, var_u, mm.WINDOWS)
        err = np.abs(h[lo:hi].reshape(hi - lo, K, D).astype(np.longdouble) - m["traj_g_var"]).astype(np.float64)
        assert np.all(err[allow == 0] == 0)
        worst = max(worst, float(np.max(err[allow > 0] / allow[allow > 0])))
        ref_all[lo:hi], allow_all[lo:hi] = m["traj_g_var"].reshape(hi - lo, K * D), allow.reshape(hi - lo, K * D)
    print("var_grad (%s): %.3f of the allowance" % ("per frame" if per_frame else "global", worst))
    within(worst, 1.0, "mlpg_var_grad_fraction_of_allowance")
    if per_frame:
        for u, v in enumerate(v_arg):
            lo, hi = int(offs[u]), int(offs[u + 1])
            assert v.grad is not None and v.grad.dtype == ldt and v.grad.shape == v.shape
            assert torch.equal(v.grad, gv64[lo:hi].to(ldt))
    else:
        # the global row: the column sums of the plane in the fixed order (exact), each element within its allowance plus
        # the summation's (128 + tiles) u sum |terms|
        assert np.array_equal(gv64.cpu().numpy(), _colsum_emulation(h))
        slack = np.sum(allow_all, axis=0) + (128 + (total + 127) // 128) * vm.U * np.sum(np.abs(ref_all), axis=0)
        err = np.abs(gv64.cpu().numpy().astype(np.longdouble) - np.sum(ref_all, axis=0)).astype(np.float64)
        within(float(np.max(err / slack.astype(np.float64))), 1.0, "mlpg_global_var_grad_fraction_of_allowance")
        assert v_arg.grad.dtype == ldt and v_arg.grad.shape == v_arg.shape and torch.equal(v_arg.grad, gv64.to(ldt))
        # two runs: the same bits
        v2 = variances()
        torch.autograd.backward(mp.mlpg_batch([s.detach() for s in slices], v2, return_device=True, var_grad=True), gs)
        assert torch.equal(v2.grad, v_arg.grad)
    for u, lf in enumerate(leaves):
        if mean_grad:
            lo, hi = int(offs[u]), int(offs[u + 1])
            assert lf.grad.dtype == ldt and torch.equal(lf.grad[:, pad:pad + K * D], g_mean64[lo:hi].to(ldt))
        else:
            assert lf.grad is None


def test_an_utterance_alone_and_in_a_batch_gives_the_same_bits():
    """Per-frame variance gradients (of a trajectory loss and of the likelihood) and NLL values."""
    e, D, K = _engine(), 10, 3
    frames = (1, 65, 2, 0, 5, 129)
    mean, var, x, g, _, _, offs, go = _operands(D, K, np.float32, np.float64, np.float32, True, 41, frames)
    dev = lambda a, dt: _t(np.ascontiguousarray(a)).to(e.device).to(dt)

    def run(us):
        ms = [dev(mean[offs[u]:offs[u + 1]], torch.float32) for u in us]
        xs = [dev(x[offs[u]:offs[u + 1]], torch.float32) for u in us]
        v1 = [dev(var[offs[u]:offs[u + 1]], torch.float64).requires_grad_(True) for u in us]
        out = mp.mlpg_batch(ms, v1, return_device=True, var_grad=True)
        torch.autograd.backward(out, [dev(g[offs[u]:offs[u + 1]], torch.float64) for u in us])
        v2 = [dev(var[offs[u]:offs[u + 1]], torch.float64).requires_grad_(True) for u in us]
        nll = mp.mlpg_trajectory_nll_batch(ms, v2, xs, return_device=True)
        (nll * dev(go[list(us)], torch.float64)).sum().backward()
        return [v.grad for v in v1], [v.grad for v in v2], nll.detach()

    b1, b2, bn = run(range(len(frames)))
    for u in (0, 1, 2, 5):             # (utterance 3 has no frames: alone it is a batch without a launch)
        a1, a2, an = run([u])
        assert torch.equal(a1[0], b1[u]) and torch.equal(a2[0], b2[u]) and torch.equal(an[0], bn[u]), u


@pytest.mark.parametrize("case", (CASES[1], CASES[2], CASES[3]), ids=_ids)
def test_trajectory_nll_batch_and_its_gradients(case):
    D, windows, mdt, vdt, xdt, per_frame, _ = case
    e, K = _engine(), len(windows) + 1
    frames = (1, 17, 2, 0, 3, 64)
    mean, var, x, _, _, _, offs, go = _operands(D, K, mdt, vdt, xdt, per_frame, 700 + D, frames)
    cast = lambda a, dt: np.ascontiguousarray(a).astype(dt)
    means_h, xs_h = [cast(m, mdt) for m in _utt_list(mean, offs)], [cast(t, xdt) for t in _utt_list(x, offs)]
    var_h = [cast(v, vdt) for v in _utt_list(var, offs)] if per_frame else cast(var, vdt)
    host = mp.mlpg_trajectory_nll_batch(means_h, var_h, xs_h, windows=windows)
    assert host.shape == (len(frames), D) and host.dtype == np.float64 and np.all(host[3] == 0)
    assert np.array_equal(mp.mlpg_trajectory_nll(means_h[1], var_h[1] if per_frame else var_h, xs_h[1], windows), host[1])
    dev = lambda a: _t(a).to(e.device)
    means_d = [dev(m).requires_grad_(True) for m in means_h]
    xs_d = [dev(t).requires_grad_(True) for t in xs_h]
    var_d = [dev(v).requires_grad_(True) for v in var_h] if per_frame else dev(var_h).requires_grad_(True)
    nll = mp.mlpg_trajectory_nll_batch(means_d, var_d, xs_d, windows=windows, return_device=True)
    assert nll.grad_fn is not None and nll.dtype == torch.float64 and np.array_equal(nll.detach().cpu().numpy(), host)
    with torch.no_grad():
        plain = mp.mlpg_trajectory_nll_batch(means_d, var_d, xs_d, windows=windows, return_device=True)
    assert plain.grad_fn is None and torch.equal(plain, nll.detach())
    (nll * dev(np.ascontiguousarray(go))).sum().backward()
    assert all(t.grad is None for t in xs_d)                                    # the targets get no gradient
    worst = 0.0
    for u, lo, hi in _utts(offs):
        m = vm.band_model(_sys(mean, offs, u, K, D), _sys(var, offs, u, K, D), x=x[lo:hi], windows=windows)
        err = np.abs(host[u].astype(np.longdouble) - m["nll"]).astype(np.float64)
        worst = max(worst, float(np.max(err / (m["kappa"] * vm.U * np.abs(m["nll"].astype(np.float64))))))
    print("nll through the API D=%d: %.4g of kappa u |NLL|" % (D, worst))
    within(worst, NLL_API_CONSTANT, "mlpg_nll_api_over_kappa_u_nll")
    # the gradients: float64 on the device against the model; a leaf's .grad is that gradient cast to its dtype
    offs_dev, w = _offs_dev(e, offs), np.asarray(windows, dtype=np.float64).reshape(-1, 3)
    buf, vd = dev(cast(mean, mdt)), dev(cast(var, vdt))
    c = e.mlpg_solve(buf, vd, offs_dev, D, w)
    xd = dev(cast(x, xdt))
    gm64, gv64 = e.mlpg_trajectory_nll_backward(buf, vd, c, xd, dev(np.ascontiguousarray(go)), offs_dev, D, w)
    plane = gv64
    if not per_frame:
        plane = torch.empty((int(offs[-1]), K * D), dtype=torch.float64, device=e.device)
        e.launch("mpx_mlpg_trajectory_nll_backward", buf, int(mdt == np.float64), K * D, vd, int(vdt == np.float64), 0, c, D,
                 xd, int(xdt == np.float64), D, dev(np.ascontiguousarray(go)), offs_dev, len(frames), int(offs[-1]), D,
                 K - 1, _wins(windows), None, K * D, plane, K * D,
                 torch.empty(int(e.lib.mpx_mlpg_nll_work_doubles(int(offs[-1]), D)), dtype=torch.float64, device=e.device))
        assert np.array_equal(gv64.cpu().numpy(), _colsum_emulation(plane.cpu().numpy()))
    _hold_nll_grads(gm64.cpu().numpy(), plane.cpu().numpy(), None, mean, var, x, go, offs, D, K, windows,
                    ("mlpg_nll_api_g_mean_over_kappa_u_max", "mlpg_nll_api_g_var_over_kappa_u_max"),
                    (NLL_API_G_MEAN_CONSTANT, NLL_API_G_VAR_CONSTANT))
    for u, md in enumerate(means_d):
        lo, hi = int(offs[u]), int(offs[u + 1])
        assert md.grad.dtype == md.dtype and md.grad.shape == md.shape and torch.equal(md.grad, gm64[lo:hi].to(md.dtype))
        if per_frame:
            v = var_d[u]
            assert v.grad.dtype == v.dtype and v.grad.shape == v.shape and torch.equal(v.grad, gv64[lo:hi].to(v.dtype))
    if not per_frame:
        assert var_d.grad.dtype == var_d.dtype and torch.equal(var_d.grad, gv64.to(var_d.dtype))


# ------------------------------------------------------------------------------------------------------- end to end
_LAYOUT = (("mag", 60), ("real", 10), ("imag", 10), ("lf0", 1))


def _cmp_batch(frames, seed, fs=16000):
    """Acoustic-model-like rows [F x 244] (float64): consistent static / delta / acc means of plausible trajectories plus a
    little noise, the voicing column in stretches, and per-frame variances."""
    import compressed_synthesis_autograd_model as csm

    rng = np.random.RandomState(seed)
    K, cmps, vars_ = 3, [], []
    for f in frames:
        lf0 = csm.lf0_track(rng, f, "mixed", fs)
        voi = lf0 > 0
        stat = list(csm.features(rng, f, 60, 10)) + [np.where(voi, lf0, np.log(150.0))[:, None]]
        cols = []
        for s in stat:
            dyn = np.stack([mm.apply(s[:, d], None) for d in range(s.shape[1])], axis=2)      # [F x K x dim]
            cols.append((dyn + 0.01 * rng.randn(*dyn.shape)).reshape(f, K * s.shape[1]))
        cmps.append(np.concatenate(cols + [np.where(voi, 0.9, 0.1)[:, None]], axis=1))
        vars_.append(np.exp(0.3 * rng.randn(f, K * 81 + 1)))
    return cmps, vars_


def test_end_to_end_variance_gradient_through_compressed_synthesis():
    """mlpg_streams_batch(var_grad=True) -> synthesis_from_compressed_batch -> backward(): the per-frame variances' gradient
    is the model of the MLPG stage applied to the gradients the synthesis gave its own inputs (the two-step product)."""
    e, K = _engine(), 3
    frames = (24, 17)
    cmps, vars_ = _cmp_batch(frames, 2)
    leaves = [_t(c).to(e.device).requires_grad_(True) for c in cmps]
    v_leaves = [_t(v).to(e.device).requires_grad_(True) for v in vars_]
    plain = mp.mlpg_streams_batch(leaves, v_leaves, return_device=True)
    tuples = mp.mlpg_streams_batch(leaves, v_leaves, return_device=True, var_grad=True)
    for t, p in zip(tuples, plain):
        for a, b in zip(t, p):
            assert torch.equal(a.detach(), b.detach())
        for a in t[:3]:
            a.retain_grad()
    ys = mp.synthesis_from_compressed_batch(tuples, 16000, fft_len=1024, noise_mode="device", return_device=True)
    rng = np.random.default_rng(9)
    loss = sum((y * _t(rng.normal(size=y.shape[0])).to(y)).sum() for y in ys)
    loss.backward()
    worst = 0.0
    for u, (v, t) in enumerate(zip(v_leaves, tuples)):
        got = v.grad.cpu().numpy()
        assert v.grad.dtype == torch.float64 and got.shape == vars_[u].shape
        assert np.all(np.isfinite(got)) and np.any(got != 0)
        col = 0
        for s, (name, d) in enumerate(_LAYOUT[:3]):
            g = t[s].grad.cpu().numpy()
            assert np.any(g != 0)
            mu_u = cmps[u][:, col:col + K * d].reshape(frames[u], K, d)
            var_u = vars_[u][:, col:col + K * d].reshape(frames[u], K, d)
            m = vm.band_model(mu_u, var_u, g=g)
            allow = _traj_allowance(m, mu_u, var_u, mm.WINDOWS)
            err = np.abs(got[:, col:col + K * d].reshape(frames[u], K, d).astype(np.longdouble) - m["traj_g_var"])
            err = err.astype(np.float64)
            assert np.all(err[allow == 0] == 0)
            worst = max(worst, float(np.max(err[allow > 0] / allow[allow > 0])))
            col += K * d
        assert not got[:, col:].any()          # lf0 (not differentiable in the synthesis) and the voicing column: zeros
    within(worst, 1.0, "mlpg_end_to_end_var_grad_fraction_of_allowance")
