"""CPU: the mathematics of the MLPG variance gradients and of the trajectory likelihood (tests/mlpg_variance_model.py against
torch autograd, torch.distributions and a longdouble inverse), the argument checks of the new public functions and the
argument-error branches of the new C entries (none of them needs a GPU)."""
import ctypes

import numpy as np
import pytest
import torch

import mlpg_model as mm
import mlpg_variance_model as vm
from _tol import within
from magphase_amd import _lib
from magphase_amd import magphase as mp

ONE_WINDOW = ((0.25, -0.5, 0.75),)
FRAMES = (1, 2, 3, 4, 9)
# The float64 emulation of the band recursion against the longdouble inverse, in units of kappa_inf(A) 2^-53 max |Z|:
# measured 0.47 at worst over the systems below (numpy float64 on the host), held at 3 x that.
Z_BAND_CONSTANT = 1.4


def _system(F, K, seed, spread=1.0):
    rng = np.random.default_rng(seed)
    mu = rng.normal(size=(F, K))
    var = np.exp(spread * rng.normal(size=(F, K)))
    return mu, var, rng.normal(size=F), rng.normal(size=F)


@pytest.mark.parametrize("windows", (mm.WINDOWS, ONE_WINDOW), ids=("two_windows", "one_window"))
@pytest.mark.parametrize("F", FRAMES)
def test_closed_forms_against_torch_autograd(F, windows):
    K = len(windows) + 1
    mu, var, x, g = _system(F, K, 10 * F + K)
    _, _, tv = vm.torch_grads(mu, var, g=g, windows=windows)
    nll, nm, nv = vm.torch_grads(mu, var, x=x, windows=windows)
    scale = lambda r: max(np.max(np.abs(r)), 1e-300)
    cv = vm.var_grad_closed(mu, var, g, windows)
    assert np.max(np.abs(cv - tv)) <= 1e-11 * scale(tv)
    gm, gv = vm.nll_grads_closed(mu, var, x, windows)
    assert np.max(np.abs(gm - nm)) <= 1e-11 * scale(nm)
    assert np.max(np.abs(gv - nv)) <= 1e-11 * scale(nv)
    assert abs(vm.nll_dense(mu, var, x, windows) - nll) <= 1e-12 * max(abs(nll), 1.0)
    assert abs(float(vm.nll_longdouble(mu, var, x, windows)) - nll) <= 1e-11 * max(abs(nll), 1.0)


@pytest.mark.parametrize("F", FRAMES)
def test_nll_against_multivariate_normal(F):
    mu, var, x, _ = _system(F, 3, 100 + F)
    ref = vm.torch_mvn_nll(mu, var, x)
    assert abs(vm.nll_dense(mu, var, x) - ref) <= 1e-11 * max(abs(ref), 1.0)


@pytest.mark.parametrize("F", FRAMES)
def test_band_recursion_against_the_longdouble_inverse(F):
    worst = 0.0
    for windows in (mm.WINDOWS, ONE_WINDOW):
        K = len(windows) + 1
        for seed, spread in ((1, 1.0), (2, 3.0), (3, 6.0)):
            _, var, _, _ = _system(F, K, 1000 * seed + F, spread)
            A, _, Ws, _ = mm.dense_system(None, var, windows, np.longdouble)
            Zl = vm.dense_inverse(A)
            kappa = np.linalg.cond(A.astype(np.float64), np.inf)
            d, Z, s = vm.recursion_emulation(var, windows)
            zmax = float(np.max(np.abs(Zl)))
            for j in range(3):
                ref = np.array([Zl[i, i + j] if i + j < F else 0.0 for i in range(F)], dtype=np.longdouble)
                worst = max(worst, float(np.max(np.abs(Z[:, j] - ref))) / (kappa * vm.U * zmax))
            sref = np.stack([np.diag(W @ Zl @ W.T) for W in Ws], axis=1)
            worst = max(worst, float(np.max(np.abs(s - sref))) / (kappa * vm.U * float(np.max(np.abs(sref)))))
            assert np.all(d > 0)
    print("band of Z, F = %d: %.3f of kappa u max|Z|" % (F, worst))
    within(worst, Z_BAND_CONSTANT, "mlpg_z_band_emulation_over_kappa_u_zmax")


@pytest.mark.parametrize("F", FRAMES)
def test_band_model_equals_the_dense_forms(F):
    """What the GPU tests compare against (banded, every system at once, longdouble) is the dense model."""
    Ld = np.longdouble
    S, K = 3, 3
    sys_ = [_system(F, K, 50 * F + s, 2.0) for s in range(S)]
    mu = np.stack([t[0] for t in sys_], axis=2)
    var = np.stack([t[1] for t in sys_], axis=2)
    x = np.stack([t[2] for t in sys_], axis=1)
    g = np.stack([t[3] for t in sys_], axis=1)
    go = np.array([1.0, -2.5, 0.5])
    m = vm.band_model(mu, var, x=x, g=g, go=go)
    for s in range(S):
        A, _, _, _ = mm.dense_system(mu[:, :, s], var[:, :, s], mm.WINDOWS, Ld)
        tol = 1e-15 * np.linalg.cond(A.astype(np.float64), np.inf)
        rel = lambda got, ref: float(np.max(np.abs(got - ref)) / max(np.max(np.abs(ref)), 1e-300))
        assert rel(m["nll"][s], vm.nll_longdouble(mu[:, :, s], var[:, :, s], x[:, s])) <= tol
        gm, gv = vm.nll_grads_closed(mu[:, :, s], var[:, :, s], x[:, s], dtype=Ld)
        assert rel(m["nll_g_mean"][:, :, s], go[s] * gm) <= tol and rel(m["nll_g_var"][:, :, s], go[s] * gv) <= tol
        assert rel(m["traj_g_var"][:, :, s], vm.var_grad_closed(mu[:, :, s], var[:, :, s], g[:, s], dtype=Ld)) <= tol
        Zl = vm.dense_inverse(A)
        for j in range(3):
            ref = np.array([Zl[i, i + j] if i + j < F else 0.0 for i in range(F)], dtype=Ld)
            assert float(np.max(np.abs(m["Z"][:, j, s] - ref))) <= tol * float(np.max(np.abs(Zl)))


# --------------------------------------------------------------------------------------------------- the public functions
def _args(F=4, D=2, K=3):
    rng = np.random.default_rng(0)
    return [rng.normal(size=(F, K * D))], np.ones(K * D), [rng.normal(size=(F, D))]


def test_var_grad_argument_checks():
    means, var, _ = _args()
    with pytest.raises(ValueError, match="return_device"):
        mp.mlpg_batch(means, var, var_grad=True)
    with pytest.raises(ValueError, match="device tensors"):
        mp.mlpg_batch(means, var, var_grad=True, return_device=True)
    with pytest.raises(ValueError, match="device tensors"):
        mp.mlpg_batch(means, [np.ones((4, 6))], var_grad=True, return_device=True)
    with pytest.raises(ValueError, match="device tensors"):      # a CPU tensor is a host array to every path
        mp.mlpg_batch(means, torch.ones(6, dtype=torch.float64, requires_grad=True), var_grad=True, return_device=True)
    cmps = [np.zeros((3, 244))]
    with pytest.raises(ValueError, match="return_device"):
        mp.mlpg_streams_batch(cmps, np.ones(244), var_grad=True)
    with pytest.raises(ValueError, match="device tensors"):
        mp.mlpg_streams_batch(cmps, np.ones(244), var_grad=True, return_device=True)


def test_trajectory_nll_argument_checks():
    means, var, targets = _args()
    bad = [
        (means, var, targets[0], "list"),                                    # not a list
        (means, var, targets + targets, "one target matrix per utterance"),
        (means, var, [targets[0][:3]], "rows"),
        (means, var, [targets[0][:, :1]], "columns"),
        (means, var, [np.full((4, 2), np.nan)], "finite"),
        (means, var, [targets[0].astype(np.complex128)], "real matrix"),
        (means, var, [targets[0][0]], "2-D"),
        (means, -var, targets, "finite and > 0"),
        (means, var[:5], targets, "vector of 6"),
        (means, [np.ones((3, 6))], targets, "rows"),
        (means[0], var, targets, "list"),
        ([means[0][:, :5]], var[:5], targets, "blocks"),
    ]
    for m, v, t, msg in bad:
        with pytest.raises(ValueError, match=msg):
            mp.mlpg_trajectory_nll_batch(m, v, t)
    with pytest.raises(ValueError, match="windows"):
        mp.mlpg_trajectory_nll_batch(means, var, targets, windows=((1.0, 2.0),))
    assert mp.mlpg_trajectory_nll_batch([], var, []).shape == (0, 0)


# ------------------------------------------------------------------------------------------------------ the C entries
def _wins(n_win=2):
    w = np.asarray(mm.WINDOWS[:n_win], dtype=np.float64).reshape(-1)
    return (ctypes.c_double * w.size)(*w)


def _err(lib, rc, word):
    assert rc == -1 and word.encode() in lib.mpx_last_error(), lib.mpx_last_error()


P = 64   # a non-null pointer value that is never dereferenced: every call below fails (or returns) before a launch


def test_var_backward_argument_errors():
    lib, w = _lib.load(), _wins()

    def call(z=P, ld_z=2, c=P, ld_c=2, mean=P, ld_mean=6, var=P, ld_var=6, off=P, n_utts=1, total=4, D=2, n_win=2, wins=w,
             g=P, ld_g=6, gsum=P, work=P):
        return lib.mpx_mlpg_var_backward(None, z, ld_z, c, ld_c, mean, 1, ld_mean, var, 1, ld_var, off, n_utts, total, D,
                                         n_win, wins, g, ld_g, gsum, work)

    _err(lib, call(D=0), "D must be")
    _err(lib, call(n_win=3), "n_win")
    _err(lib, call(total=-1), "negative total_frames")
    _err(lib, call(n_utts=-1), "negative n_utts")
    _err(lib, call(total=2 ** 31), "2^31")
    _err(lib, call(ld_z=1), "ld_z")
    _err(lib, call(ld_c=1), "ld_z or ld_c")
    _err(lib, call(ld_mean=5), "ld_mean")
    _err(lib, call(ld_var=5), "ld_var")
    _err(lib, call(ld_g=5), "ld_g")
    _err(lib, call(wins=None), "windows")
    bad = (ctypes.c_double * 6)(*([float("nan")] * 6))
    _err(lib, call(wins=bad), "not finite")
    for name in ("z", "c", "mean", "var", "off", "g"):
        _err(lib, call(**{name: None}), "null pointer")
    _err(lib, call(n_utts=2 ** 31 - 1, D=2 ** 20, ld_z=2 ** 20, ld_c=2 ** 20), "too many systems")
    _err(lib, call(total=2 ** 31 - 1, D=2 ** 20, ld_z=2 ** 20, ld_c=2 ** 20, ld_mean=2 ** 22, ld_var=2 ** 22, ld_g=2 ** 22),
         "too many elements")
    _err(lib, call(ld_var=0, gsum=None), "gsum")
    _err(lib, call(ld_var=0, work=None), "gsum")
    assert call(total=0, z=None, g=None) == 0 and call(n_utts=0, mean=None) == 0      # no frames: no launch


def test_column_sums_argument_errors():
    lib = _lib.load()
    f = lib.mpx_mlpg_column_sums
    _err(lib, f(None, P, 4, 3, 0, P, P), "width")
    _err(lib, f(None, P, 4, -1, 4, P, P), "negative")
    _err(lib, f(None, P, 4, 2 ** 31, 4, P, P), "2^31")
    _err(lib, f(None, P, 3, 3, 4, P, P), "ld_x")
    _err(lib, f(None, P, 2 ** 40, 2 ** 31 - 1, 2 ** 40, P, P), "too many elements")
    for a in ((None, P, P), (P, None, P), (P, P, None)):
        _err(lib, f(None, a[0], 4, 3, 4, a[1], a[2]), "null pointer")
    assert f(None, None, 4, 0, 4, None, None) == 0
    assert lib.mpx_mlpg_colsum_work_doubles(127, 5) == 5 and lib.mpx_mlpg_colsum_work_doubles(128, 5) == 5
    assert lib.mpx_mlpg_colsum_work_doubles(129, 5) == 10 and lib.mpx_mlpg_colsum_work_doubles(0, 5) == 0
    assert lib.mpx_mlpg_colsum_work_doubles(-1, 5) == 0 and lib.mpx_mlpg_colsum_work_doubles(5, 0) == 0


def test_trajectory_nll_argument_errors():
    lib, w = _lib.load(), _wins()

    def call(c=P, ld_c=2, x=P, ld_x=2, var=P, ld_var=6, off=P, n_utts=1, total=4, D=2, n_win=2, wins=w, nll=P):
        return lib.mpx_mlpg_trajectory_nll(None, c, ld_c, x, 0, ld_x, var, 1, ld_var, off, n_utts, total, D, n_win, wins, nll)

    _err(lib, call(D=0), "D must be")
    _err(lib, call(n_win=0), "n_win")
    _err(lib, call(total=-1), "negative total_frames")
    _err(lib, call(n_utts=-1), "negative n_utts")
    _err(lib, call(ld_c=1), "ld_c")
    _err(lib, call(ld_x=1), "ld_c or ld_x")
    _err(lib, call(ld_var=5), "ld_var")
    _err(lib, call(wins=None), "windows")
    _err(lib, call(wins=(ctypes.c_double * 6)(*([float("inf")] * 6))), "not finite")
    _err(lib, call(n_utts=2 ** 31 - 1, D=2 ** 20, ld_c=2 ** 20, ld_x=2 ** 20), "too many systems")
    for name in ("c", "x", "var", "off", "nll"):
        _err(lib, call(**{name: None}), "null pointer")
    assert call(total=0, c=None) == 0 and call(n_utts=0, nll=None) == 0


def test_trajectory_nll_backward_argument_errors():
    lib, w = _lib.load(), _wins(1)

    def call(mean=P, ld_mean=4, var=P, ld_var=0, c=P, ld_c=2, x=P, ld_x=2, go=P, off=P, n_utts=1, total=4, D=2, n_win=1,
             wins=w, g_mean=P, ld_gm=4, g_var=P, ld_gv=4, work=P):
        return lib.mpx_mlpg_trajectory_nll_backward(None, mean, 0, ld_mean, var, 0, ld_var, c, ld_c, x, 1, ld_x, go, off,
                                                    n_utts, total, D, n_win, wins, g_mean, ld_gm, g_var, ld_gv, work)

    _err(lib, call(D=0), "D must be")
    _err(lib, call(n_win=3), "n_win")
    _err(lib, call(total=-1), "negative total_frames")
    _err(lib, call(ld_mean=3), "ld_mean")
    _err(lib, call(ld_var=3), "ld_var")
    _err(lib, call(ld_c=1), "ld_c")
    _err(lib, call(ld_x=1), "ld_c or ld_x")
    _err(lib, call(ld_gm=3), "ld_gm")
    _err(lib, call(ld_gv=3), "ld_gm or ld_gv")
    _err(lib, call(wins=None), "windows")
    _err(lib, call(wins=(ctypes.c_double * 3)(*([float("nan")] * 3))), "not finite")
    _err(lib, call(n_utts=2 ** 31 - 1, D=2 ** 20, ld_c=2 ** 20, ld_x=2 ** 20), "too many systems")
    _err(lib, call(n_utts=-1), "negative n_utts")
    _err(lib, call(g_mean=None, g_var=None), "nothing to compute")
    for name in ("mean", "var", "c", "x", "go", "off"):
        _err(lib, call(**{name: None}), "null pointer")
    _err(lib, call(work=None), "work")
    assert call(total=0, mean=None) == 0 and call(n_utts=0, go=None) == 0
    assert lib.mpx_mlpg_nll_work_doubles(7, 3) == 63 and lib.mpx_mlpg_nll_work_doubles(-1, 3) == 0
    assert lib.mpx_mlpg_nll_work_doubles(7, 0) == 0
