"""CPU: the float64 model of the compressed analysis (tests/compressed_analysis_autograd_model.py) against the oracle, the
closed form of its backward pass (what k_phase_grad_mask, k_mel_warp_bwd and k_rows_lerp_adjoint implement ahead of the
lossless analysis' backward kernels) against torch float64 autograd and against central
differences, the share of phase outputs that lie too close to the clip to be compared, the adjoint's frame ranges at the
width of the phase features, and the argument checks of mpx_mel_warp_backward.  Needs no GPU."""
import numpy as np
import pytest

import _tol
import compressed_analysis_autograd_model as model
from magphase_amd import hostmath as hm
from oracle import magphase_oracle as orc

FS = model.FS
TOL = 1.0e-11      # of the largest gradient: float64 round-off of two different orders of the same sums
TIE_CAP = 0.01     # of the voiced phase elements of a batch


def _upstream(rng, out, tab, tie=True):
    """Standard normal upstream gradients of the three outputs, zero at the tie elements (model.tie_mask)."""
    g = [rng.randn(*out[k].shape) for k in range(3)]
    if tie:
        for k, m in enumerate(model.tie_mask(out[3], out[4], tab), start=1):
            g[k][m] = 0.0
    return tuple(g)


@pytest.mark.parametrize("b_const_rate", [False, True])
def test_model_forward_matches_the_oracle(b_const_rate):
    """The oracle's mcep reads and writes float32 files: its input carries a relative 2^-24 (2 * 2^-24 on each log bin, summed
    by |W|'s rows), its n cepstral coefficients a relative 2^-24 each (|mc_n| <= max |out| n summed by the cosine matrix is
    bounded by n * max |out|).  The constant-rate phase streams are interpolated after the warp, the oracle's before it:
    below 1e-8 per bin."""
    N, pd = 1024, 45
    sig, pm_sec, voi = model.batch_utts(N)[1]
    wm, wp = model.warps(N, phase_dim=pd)
    tab = model.tables(pm_sec, voi, sig.size, b_const_rate)
    out = model.forward_numpy(sig, tab, N, wm, wp)
    ref = orc.analysis_compressed_from_epochs(sig.astype(np.float64), FS, pm_sec, voi, fft_len=N, mag_dim=60, phase_dim=pd,
                                              b_const_rate=b_const_rate)
    cf, _ = hm.define_crossfade_params(FS)
    k_full = hm.get_num_full_mel_coeffs_from_num_phase_coeffs(cf, pd, hm.define_alpha(FS), FS)
    u = 2.0 ** -24
    for k, (w, n_coef) in enumerate(((wm, 60), (wp, k_full), (wp, k_full))):
        assert out[k].shape == ref[k].shape and np.all(np.isfinite(out[k]))
        bound = u * (2.0 * np.abs(w).sum(axis=1).max() + n_coef * np.max(np.abs(ref[k])))
        if k and b_const_rate:
            bound += 1.0e-8 * np.abs(w).sum(axis=1).max()
        err = np.max(np.abs(out[k] - ref[k]))
        print("output %d const_rate %s: %.3g (bound %.3g)" % (k, b_const_rate, err, bound))
        assert err <= bound
    assert np.any(np.abs(out[1][tab["voi"]]) == 1.0)      # the clip is exercised
    if not b_const_rate:
        assert np.any(~tab["voi"]) and not out[1][~tab["voi"]].any()


@pytest.mark.parametrize("b_const_rate", [False, True])
@pytest.mark.parametrize("N,pd,alpha_phase", [(1024, 45, None), (2048, 10, False), (4096, 45, None)])
def test_closed_form_equals_autograd(N, pd, alpha_phase, b_const_rate):
    rng = np.random.RandomState(N + pd)
    wm, wp = model.warps(N, phase_dim=pd, alpha_phase=alpha_phase)
    for sig, pm_sec, voi in model.batch_utts(N)[:2]:
        tab = model.tables(pm_sec, voi, sig.size, b_const_rate)
        out = model.forward_numpy(sig, tab, N, wm, wp)
        rows = model.lossless.forward_numpy(sig, tab["pm"], tab["left"], tab["right"], N)
        for which in ((True, True, True), (True, False, False), (False, True, True)):
            g = tuple(x if w else None for x, w in zip(_upstream(rng, out, tab), which))
            want = model.grads_autograd(sig, g, tab, N, wm, wp)
            got = model.grads_closed(rows[0], rows[1], rows[2], out[1], out[2], g, tab, sig.size, N, wm, wp)
            assert np.all(np.isfinite(got)) and np.any(want != 0)
            assert model.rel_err(got, want) <= TOL, model.rel_err(got, want)


def test_autograd_equals_central_differences():
    """One utterance of 6 frames, float64, directional derivatives with step h = 1e-6: the truncation error is h^2 times
    a third derivative (the samples are ~0.1, no magnitude near the 1e-8 floor), the round-off 1e-16 / h of the loss --
    both far below 1e-5 of the derivative."""
    N, pd, h = 1024, 45, 1.0e-6
    rng = np.random.RandomState(6)
    sig, pm_sec, voi = model.utterance(rng, 6, model.MIX[:2])
    sig = sig.astype(np.float64)
    wm, wp = model.warps(N, phase_dim=pd)
    for b_const_rate in (False, True):
        tab = model.tables(pm_sec, voi, sig.size, b_const_rate)
        out = model.forward_numpy(sig, tab, N, wm, wp)
        g = _upstream(rng, out, tab)
        grad = model.grads_autograd(sig, g, tab, N, wm, wp)

        def loss(x):
            o = model.forward_numpy(x, tab, N, wm, wp)
            return sum(float(np.sum(o[k] * g[k])) for k in range(3))

        for _ in range(4):
            v = rng.randn(sig.size)
            fd = (loss(sig + h * v) - loss(sig - h * v)) / (2.0 * h)
            assert abs(fd - float(grad @ v)) <= 1.0e-5 * abs(fd), (fd, float(grad @ v))


@pytest.mark.parametrize("N", [1024, 2048, 4096])
def test_few_phase_outputs_lie_at_the_clip(N):
    """The tie rule zeroes the upstream gradient where the float64 pre-clip magnitude is within 1e-3 of 1: at most 1 % of
    the voiced phase elements of every batch of the GPU tests."""
    for b_const_rate in (False, True):
        for pd, alpha_phase in ((45, None), (10, False)):
            wm, wp = model.warps(N, phase_dim=pd, alpha_phase=alpha_phase)
            ties = voiced = clipped = 0
            for sig, pm_sec, voi in model.batch_utts(N):
                tab = model.tables(pm_sec, voi, sig.size, b_const_rate)
                out = model.forward_numpy(sig, tab, N, wm, wp)
                ties += sum(int(m.sum()) for m in model.tie_mask(out[3], out[4], tab))
                voiced += 2 * int(tab["voi"].sum()) * pd
                clipped += sum(int(np.sum(np.abs(out[k][tab["voi"]]) == 1.0)) for k in (1, 2))
            assert voiced > 0 and clipped > 0
            _tol.note("autograd_compressed_analysis_tie_fraction_%d_%s_%d" % (N, "cr" if b_const_rate else "vr", pd),
                      ties / voiced)
            assert ties <= TIE_CAP * voiced, (ties, voiced)


def test_lerp_adjoint_table_at_the_width_of_the_phase_features():
    N, pd = 1024, 10
    rng = np.random.RandomState(2)
    row0, row1, rowt, base = [], [], [], 0
    for sig, pm_sec, voi in model.batch_utts(N):
        tab = model.tables(pm_sec, voi, sig.size, True)
        row0.append(tab["row0"] + base), row1.append(tab["row1"] + base), rowt.append(tab["rowt"])
        base += tab["pm"].size
    tab = {"row0": np.concatenate(row0), "row1": np.concatenate(row1), "rowt": np.concatenate(rowt)}
    assert np.any(tab["row0"] == tab["row1"])          # the duplicated first row
    g = rng.randn(tab["row0"].size, pd)
    ranges = hm.lerp_adjoint_table(tab["row0"], tab["row1"], tab["rowt"], base)
    assert ranges.shape == (base, 4) and ranges.dtype == np.int32
    got = model.lerp_adjoint_by_table(g, ranges, tab["rowt"])
    want = model.lerp_adjoint(g, tab, base)
    assert got.shape == (base, pd) and np.max(np.abs(got - want)) <= 1e-12 and np.any(want != 0)


def test_argument_errors_without_gpu():
    from magphase_amd import _lib

    lib = _lib.load()
    p = 64     # any non-null address: the arguments are refused before anything is dereferenced

    def call(n_bins=513, mag_dim=60, n_mag=5, rows=(None, None, None), grad_mag=p, phase_dim=45, n_ph=5, grad_real=p,
             grad_imag=p, ld=513, ld_grad=513, g_mag=p):
        return lib.mpx_mel_warp_backward(None, n_bins, g_mag, p, mag_dim, p, n_mag, rows[0], rows[1], rows[2], grad_mag, p, p,
                                         p, phase_dim, p, p, n_ph, None, grad_real, grad_imag, ld, ld_grad)

    for kw, word in (({"mag_dim": 65}, b"1..64"), ({"phase_dim": 65}, b"1..64"), ({"mag_dim": 0}, b"1..64"),
                     ({"ld": 512}, b"pitch"), ({"ld_grad": 100}, b"pitch"), ({"n_bins": 0}, b"size"),
                     ({"n_mag": -1}, b"size"), ({"rows": (p, None, p)}, b"row0"), ({"g_mag": None}, b"null")):
        assert call(**kw) == -1 and word in lib.mpx_last_error(), kw
    # nothing to do: zero rows, or every job null (whose n_out is then not looked at) -- 0, nothing launched
    assert call(n_mag=0, n_ph=0) == 0
    assert call(grad_mag=None, grad_real=None, grad_imag=None, mag_dim=99, phase_dim=99) == 0
    assert call(grad_mag=None, mag_dim=99, n_ph=0) == 0
    assert lib.mpx_phase_grad_mask(None, -1, 45, p, p, p, p, p, p, p) == -1 and b"size" in lib.mpx_last_error()
    assert lib.mpx_phase_grad_mask(None, 5, 45, None, p, p, p, p, p, p) == -1 and b"null" in lib.mpx_last_error()
    assert lib.mpx_phase_grad_mask(None, 0, 45, None, None, None, None, None, None, None) == 0
