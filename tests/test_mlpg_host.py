"""CPU: the numpy model of the MLPG kernels (tests/mlpg_model.py) against independent formulations, the float64 emulation
of k_mlpg_solve's banded LDL^T against the derived backward-error bound, and every argument check of the public functions
and of the two C entries -- none of which needs a GPU."""
import ctypes

import numpy as np
import pytest

import mlpg_model as mm
from _tol import within
from magphase_amd import _lib
from magphase_amd import hostmath as hm

FRAMES = (1, 2, 3, 4, 5, 17, 64)
NON_DEFAULT = ((0.25, -0.5, 0.75),)


def _system(F, K, seed, ratio=1.0, per_frame=True):
    rng = np.random.default_rng(seed)
    mu = rng.normal(size=(F, K))
    var = np.exp(rng.normal(size=(F if per_frame else 1, K)))
    var[:, 0] *= ratio
    return mu, np.broadcast_to(var, (F, K)).copy()


def _windows(K):
    return mm.WINDOWS[:K - 1]


@pytest.mark.parametrize("F", FRAMES)
@pytest.mark.parametrize("K", (2, 3))
def test_model_is_the_weighted_least_squares_solution(F, K):
    mu, var = _system(F, K, 10 * F + K)
    _, _, Ws, ps = mm.dense_system(mu, var, _windows(K))
    M = np.vstack([np.sqrt(p)[:, None] * W for W, p in zip(Ws, ps)])
    rhs = np.concatenate([np.sqrt(p) * mu[:, k] for k, p in enumerate(ps)])
    ref = np.linalg.lstsq(M, rhs, rcond=None)[0]
    c = mm.solve_dense(mu, var, _windows(K))
    within(np.max(np.abs(c - ref)) / np.max(np.abs(ref)), 1e-10, "mlpg_model_vs_lstsq")


@pytest.mark.parametrize("F", FRAMES)
def test_model_matches_solveh_banded(F):
    scipy_linalg = pytest.importorskip("scipy.linalg")
    mu, var = _system(F, 3, 7 * F)
    A, b, _, _ = mm.dense_system(mu, var)
    ab = np.zeros((3, F))
    for k in range(3):
        ab[k, :F - k] = np.diagonal(A, k)
    assert np.allclose(A, A.T) and np.all(np.abs(np.triu(A, 3)) == 0)     # symmetric, pentadiagonal
    ref = scipy_linalg.solveh_banded(ab[:min(3, F)], b, lower=True)
    within(np.max(np.abs(mm.solve_dense(mu, var) - ref)) / np.max(np.abs(ref)), 1e-11, "mlpg_model_vs_solveh_banded")
    within(np.max(np.abs(mm.solve_dense(mu, var, dtype=np.longdouble).astype(np.float64) - ref)) / np.max(np.abs(ref)),
           1e-11, "mlpg_longdouble_model_vs_solveh_banded")


@pytest.mark.parametrize("F", FRAMES)
@pytest.mark.parametrize("windows", (mm.WINDOWS, mm.WINDOWS[:1], NON_DEFAULT))
def test_band_form_of_the_model_is_the_dense_one(F, windows):
    """band_system / band_solve / band_dense (what the GPU tests hold every system to) against dense_system."""
    K, S = len(windows) + 1, 3
    rng = np.random.default_rng(F + K)
    mu, var = rng.normal(size=(F, K, S)), np.exp(rng.normal(size=(F, K, S)))
    a, e, f, b = mm.band_system(mu, var, windows)
    Ad = mm.band_dense(a, e, f)
    for s in range(S):
        A, bd, _, _ = mm.dense_system(mu[:, :, s], var[:, :, s], windows, np.longdouble)
        within(np.max(np.abs(Ad[s] - A.astype(np.float64))) / np.max(np.abs(A)).astype(np.float64), 4 * 2.0 ** -53,
               "mlpg_band_vs_dense_A")
        within(float(np.max(np.abs(b[:, s] - bd)) / np.max(np.abs(bd))), 16 * 2.0 ** -64, "mlpg_band_vs_dense_b")
        c = mm.gauss_solve(A, bd)
        kappa = mm.errors(c, mu[:, :, s], var[:, :, s], windows)[2]
        within(float(np.max(np.abs(mm.band_solve(a, e, f, b)[:, s] - c)) / np.max(np.abs(c))) / kappa, 256 * 2.0 ** -64,
               "mlpg_band_solve_vs_dense_over_kappa")
        within(float(np.max(np.abs(mm.band_matvec(a, e, f, b)[:, s] - A @ bd)) / np.max(np.abs(A @ bd))), 64 * 2.0 ** -64,
               "mlpg_band_matvec_vs_dense")


@pytest.mark.parametrize("F", FRAMES)
@pytest.mark.parametrize("windows", (mm.WINDOWS, mm.WINDOWS[:1], NON_DEFAULT))
def test_consistent_means_return_the_static_trajectory(F, windows):
    """mu_k = W_k s for every k  =>  c = s, whatever the variances."""
    rng = np.random.default_rng(F)
    s = rng.normal(size=F)
    K = len(windows) + 1
    mu = mm.apply(s, None, windows, np.longdouble)    # in longdouble: a float64 W_k s is itself rounded at 2^-53
    for ratio in (1e-6, 1.0, 1e6):
        _, var = _system(F, K, F + 1, ratio)
        c = mm.solve_dense(mu, var, windows, np.longdouble).astype(np.float64)
        kappa = mm.errors(c, mu, var, windows)[2]
        within(np.max(np.abs(c - s)) / np.max(np.abs(s)) / kappa, 256 * 2.0 ** -64, "mlpg_model_consistent_means_over_kappa")


@pytest.mark.parametrize("F", (1, 2, 3, 9))
@pytest.mark.parametrize("K", (2, 3))
def test_backward_formulas_match_torch_autograd(F, K):
    import torch

    mu, var = _system(F, K, 3 * F + K)
    g = np.random.default_rng(F).normal(size=F)
    tp = torch.from_numpy(mm.taps(_windows(K)))
    mu_t = torch.from_numpy(mu).requires_grad_(True)
    p = 1.0 / torch.from_numpy(var)
    Ws = [torch.from_numpy(mm.dense_w(F, tp[k].numpy())) for k in range(K)]
    A = sum(W.T @ (p[:, k, None] * W) for k, W in enumerate(Ws))
    b = sum(W.T @ (p[:, k] * mu_t[:, k]) for k, W in enumerate(Ws))
    c = torch.linalg.solve(A, b)
    c.backward(torch.from_numpy(g))
    ref = mu_t.grad.numpy()
    within(np.max(np.abs(mm.backward(g, var, _windows(K)) - ref)) / np.max(np.abs(ref)), 1e-11, "mlpg_model_backward_vs_torch")


@pytest.mark.parametrize("F", FRAMES + (257,))
@pytest.mark.parametrize("ratio", (1e-8, 1e-4, 1.0, 1e4, 1e8))
def test_kernel_order_ldl_stays_within_half_the_backward_error_bound(F, ratio):
    """The float64 emulation of k_mlpg_solve (forming A and b included) against A, b in longdouble: eta <= 0.5 x 16 x 2^-53,
    and the forward error within its kappa bound."""
    for K, per_frame in ((3, True), (3, False), (2, True)):
        mu, var = _system(F, K, F + K, ratio, per_frame)
        c = mm.ldl_emulation(mu, var, _windows(K))
        eta, fwd, _ = mm.errors(c, mu, var, _windows(K))
        within(eta, 0.5, "mlpg_emulation_eta_fraction_of_bound")
        within(fwd, 1.0, "mlpg_emulation_forward_fraction_of_bound")


def test_emulation_handles_one_and_two_frames_exactly():
    for F in (1, 2):
        mu, var = _system(F, 3, F)
        assert np.allclose(mm.ldl_emulation(mu, var), mm.solve_dense(mu, var), rtol=1e-13, atol=0)


# ------------------------------------------------------------------------------------------------ argument checks
def _no_engine(monkeypatch):
    from magphase_amd import magphase as mp

    def boom(*a, **k):
        raise AssertionError("an engine was asked for before the argument checks finished")
    monkeypatch.setattr(mp, "get_engine", boom)
    return mp


def test_mlpg_batch_argument_checks_raise_before_an_engine_exists(monkeypatch):
    mp = _no_engine(monkeypatch)
    ok, v = np.zeros((4, 6)), np.ones(6)
    bad = [
        (np.zeros((4, 6)), v, {}),                                   # means: not a list
        ([np.zeros(6)], v, {}),                                      # 1-D
        ([np.zeros((4, 7))], np.ones(7), {}),                        # 7 columns are no 3 streams
        ([ok, np.zeros((3, 9))], v, {}),                             # two widths
        ([ok], np.ones(5), {}),                                      # var length
        ([ok], np.zeros(6), {}),                                     # var == 0
        ([ok], -v, {}),                                              # var < 0
        ([ok], np.full(6, np.inf), {}),                              # var not finite
        ([ok], np.full(6, np.nan), {}),
        ([ok], [np.ones((3, 6))], {}),                               # per-frame var: rows differ
        ([ok], [np.ones((4, 6)), np.ones((4, 6))], {}),              # per-frame var: count differs
        ([ok], [np.zeros((4, 6))], {}),                              # per-frame var: not positive
        ([ok], v, {"windows": ()}),                                  # n_win 0
        ([ok], v, {"windows": mp.MLPG_WINDOWS + ((1.0, 0.0, 0.0),)}),   # n_win 3
        ([ok], v, {"windows": ((1.0, 2.0),)}),                       # two taps
        ([ok], v, {"windows": ((1.0, np.nan, 0.0),)}),
        ([ok.astype(complex)], v, {}),
    ]
    for means, var, kw in bad:
        with pytest.raises(ValueError):
            mp.mlpg_batch(means, var, **kw)
    import torch
    with pytest.raises(ValueError):
        mp.mlpg_batch([torch.zeros((4, 6), dtype=torch.float16)], v)
    with pytest.raises(ValueError):
        mp.mlpg(np.zeros((4, 6)), np.zeros(6))
    assert mp.mlpg_batch([], v) == []


def test_dynamic_features_argument_checks_raise_before_an_engine_exists(monkeypatch):
    mp = _no_engine(monkeypatch)
    for mats, kw in ((np.zeros((4, 2)), {}), ([np.zeros(4)], {}), ([np.zeros((4, 2)), np.zeros((4, 3))], {}),
                     ([np.zeros((4, 0))], {}), ([np.zeros((4, 2))], {"windows": ((1.0,),)})):
        with pytest.raises(ValueError):
            mp.dynamic_features_batch(mats, **kw)
    with pytest.raises(ValueError):
        mp.dynamic_features(np.zeros(4))
    assert mp.dynamic_features_batch([]) == []


def test_mlpg_streams_argument_checks_raise_before_an_engine_exists(monkeypatch):
    mp = _no_engine(monkeypatch)
    W = 3 * 81 + 1
    ok, v = np.zeros((4, W)), np.ones(W)
    bad = [
        ([np.zeros((4, W - 1))], np.ones(W - 1), {}),                      # width against the layout
        ([ok], v, {"layout": ()}),
        ([ok], v, {"layout": (("mag", 0),)}),
        ([ok], v, {"layout": (("mag", 81),)}),                             # vuv without an lf0 stream
        ([ok], v, {"layout": (("mag", 60), ("lf0", 21))}),                 # lf0 wider than 1
        ([ok], v, {"layout": (("a", 40), ("a", 40), ("lf0", 1))}),         # a name twice
        ([ok], v, {"layout": "mag"}),
        ([ok], v, {"vuv_thres": np.nan}),
        ([ok], v, {"vuv_thres": "0.5"}),
        ([ok], np.concatenate((np.zeros(1), np.ones(W - 1))), {}),         # a stream variance of 0
        ([ok], v, {"windows": ()}),
    ]
    for cmps, var, kw in bad:
        with pytest.raises(ValueError):
            mp.mlpg_streams_batch(cmps, var, **kw)
    # the voicing column's variance is not used, and not checked; the check itself must get past it to the engine
    vv = v.copy()
    vv[-1] = 0.0
    with pytest.raises(AssertionError, match="engine"):
        mp.mlpg_streams_batch([ok], vv)
    assert mp.mlpg_streams_batch([], v) == []


def test_c_entries_argument_errors_without_gpu():
    lib = _lib.load()
    win = (ctypes.c_double * 6)(-0.5, 0.0, 0.5, 1.0, -2.0, 1.0)
    one = ctypes.c_void_p(8)   # a non-null pointer that is never followed: every call below returns before a launch

    def solve(mean=one, ld_mean=30, var=one, ld_var=0, off=one, n_utts=1, total=5, D=10, n_win=2, w=win, rhs=0, out=one,
              ld_out=10, work=one):
        return lib.mpx_mlpg_solve(None, mean, 0, ld_mean, var, 1, ld_var, off, n_utts, total, D, n_win, w, rhs, out, ld_out,
                                  work)

    def app(x=one, ld_x=10, var=one, ld_var=0, off=one, n_utts=1, total=5, D=10, n_win=2, w=win, y=one, ld_y=30):
        return lib.mpx_mlpg_apply(None, x, 0, ld_x, var, 1, ld_var, off, n_utts, total, D, n_win, w, y, ld_y)

    for fn, name in ((solve, b"mpx_mlpg_solve"), (app, b"mpx_mlpg_apply")):
        for kw, word in (({"D": 0}, b"D must"), ({"n_win": 0}, b"n_win"), ({"n_win": 3}, b"n_win"),
                         ({"total": -1}, b"negative"), ({"n_utts": -1}, b"negative"), ({"w": None}, b"null"),
                         ({"off": None}, b"null"), ({"ld_var": 7}, b"ld_var")):
            assert fn(**kw) == -1, (name, kw)
            err = lib.mpx_last_error()
            assert name in err and word in err, (kw, err)
        assert fn(total=0) == 0 and fn(n_utts=0) == 0          # an empty batch: no launch, no error
    for kw in ({"mean": None}, {"var": None}, {"out": None}, {"work": None}):
        assert solve(**kw) == -1 and b"null" in lib.mpx_last_error(), kw
    for kw, word in (({"ld_mean": 29}, b"ld_mean"), ({"ld_out": 9}, b"ld_out"), ({"rhs": 1, "ld_mean": 9}, b"ld_mean")):
        assert solve(**kw) == -1 and word in lib.mpx_last_error(), kw
    for kw in ({"x": None}, {"y": None}):
        assert app(**kw) == -1 and b"null" in lib.mpx_last_error(), kw
    for kw, word in (({"ld_x": 9}, b"ld_x"), ({"ld_y": 29}, b"ld_y")):
        assert app(**kw) == -1 and word in lib.mpx_last_error(), kw
    assert lib.mpx_mlpg_work_doubles(1000, 60) == 2 * 1000 * 60
    assert lib.mpx_mlpg_work_doubles(-1, 60) == 0 and lib.mpx_mlpg_work_doubles(5, 0) == 0


def test_windows_and_layout_helpers():
    w = hm.mlpg_windows(((-0.5, 0, 0.5),))
    assert w.shape == (1, 3) and w.dtype == np.float64
    lay, streams, need = hm.mlpg_layout((("mag", 60), ("real", 10), ("imag", 10), ("lf0", 1)), True, 3)
    assert streams == [(0, 60), (180, 10), (210, 10), (240, 1)] and need == 244
    assert hm.mlpg_layout((("x", 2),), False, 2)[1:] == ([(0, 2)], 4)
