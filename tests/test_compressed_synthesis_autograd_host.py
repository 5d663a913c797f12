"""CPU: the float64 model of the compressed synthesis (tests/compressed_synthesis_autograd_model.py) against the oracle, its
closed-form gradients against torch autograd of its forward, the reversed-filter adjoint of the output high-pass against
a dense filter matrix, and the argument checks of mpx_synthesis_compressed_backward / mpx_mel_unwarp_backward.  Needs no
GPU."""
import numpy as np
import pytest
from scipy import signal

import compressed_synthesis_autograd_model as model
from oracle import magphase_oracle as orc


def _case(fs, N, cr, pd, ap_win, kind, seed, n_rows=24):
    rng = np.random.RandomState(seed)
    lf0 = model.lf0_track(rng, n_rows, kind, fs)
    a_mag, a_real, a_imag = model.features(rng, n_rows, 60, pd)
    tab = model.tables(lf0, fs, N, cr, ap_win)
    cst = model.constants(fs, N, 60, pd)
    noise = rng.uniform(-1, 1, tab["ns_len"])
    ns, inv = model.noise_spectra(noise, tab, N)
    return dict(lf0=lf0, feats=(a_mag, a_real, a_imag), tab=tab, cst=cst, noise=noise, ns=ns, inv=inv, rng=rng)


_FORWARD_CASES = [(fs, N, cr, pd, ap, kind)
                  for fs, N in ((16000, 2048), (48000, 4096))
                  for cr in (False, True)
                  for pd, ap, kind in ((10, True, "mixed"), (45, False, "voiced"), (45, True, "unvoiced"),
                                       (10, False, "mixed"))]


@pytest.mark.parametrize("fs,N,cr,pd,ap_win,kind", _FORWARD_CASES)
@pytest.mark.parametrize("b_out_hpf", [False, True])
def test_model_forward_matches_the_oracle(fs, N, cr, pd, ap_win, kind, b_out_hpf):
    """Two float64 statements of one formula: the difference is rounding in another order.  Calibrated here, each stated
    figure <= 3 x the worst case measured over these cases:
      before the high-pass (and b_out_hpf=False)   1.55e-15 of the peak, stated 4.5e-15;
      after it, 16 kHz                             1.24e-9, stated 3.7e-9;
      after it, 48 kHz                             4.79e-8, stated 1.4e-7.
    The expected 1e-11 holds before the high-pass and not after it: scipy's lfilter runs the fourth-order Butterworth in
    direct form, whose four poles lie within 0.005 (48 kHz) / 0.016 (16 kHz) of z = 1, and its own rounding, fed back
    through 1 / A(z), is of this size -- two inputs that agree to 1e-15 come out 1e-8 apart.  That is the reference's own
    error, not the model's: the waveforms before the filter are compared at 4.5e-15 in the same test."""
    import torch

    c = _case(fs, N, cr, pd, ap_win, kind, 3)
    want, dbg = orc.synthesis_from_compressed(*c["feats"], c["lf0"], fs, fft_len=N, b_voi_ap_win=ap_win, b_const_rate=cr,
                                              b_out_hpf=b_out_hpf, v_noise=c["noise"], return_debug=True)
    t = [torch.from_numpy(x) for x in c["feats"]]
    got = model.forward_torch(t[0], t[1], t[2], c["tab"], c["cst"], c["ns"], c["inv"], b_out_hpf).numpy()
    pre = model.forward_torch(t[0], t[1], t[2], c["tab"], c["cst"], c["ns"], c["inv"], b_out_hpf, return_pre=True).numpy()
    assert got.shape == want.shape and np.max(np.abs(want)) > 0
    assert np.array_equal(dbg["v_voi"], c["tab"]["voiced"]) and np.array_equal(dbg["v_pm"], c["tab"]["v_pm"])
    err_pre = float(np.max(np.abs(pre - dbg["v_pre_hpf"])) / np.max(np.abs(dbg["v_pre_hpf"])))
    err = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
    print("fs %d N %d cr %s pd %d ap_win %s %s hpf %s: %.3g of the peak (%.3g before the high-pass)"
          % (fs, N, cr, pd, ap_win, kind, b_out_hpf, err, err_pre))
    assert err_pre <= 4.5e-15
    assert err <= ((1.4e-7 if fs == 48000 else 3.7e-9) if b_out_hpf else 4.5e-15)


@pytest.mark.parametrize("fs,N,cr,pd,kind,b_out_hpf", [(16000, 1024, False, 10, "mixed", True),
                                                       (16000, 1024, True, 45, "mixed", False),
                                                       (16000, 2048, True, 10, "voiced", True),
                                                       (48000, 4096, False, 45, "mixed", True),
                                                       (48000, 4096, True, 10, "unvoiced", True)])
def test_closed_form_equals_autograd(fs, N, cr, pd, kind, b_out_hpf):
    c = _case(fs, N, cr, pd, True, kind, 5, n_rows=16)
    a_mag, a_real, a_imag = c["feats"]
    if kind != "unvoiced":   # a voiced bin with a == b == 0 needs whole zero rows of coefficients: one such row
        v_row = int(c["tab"]["row0"][np.flatnonzero(c["tab"]["voiced"])[0]])
        a_real[v_row] = a_imag[v_row] = 0.0
    gy = c["rng"].randn(c["tab"]["out_len"])
    args = (a_mag, a_real, a_imag, gy, c["tab"], c["cst"], c["ns"], c["inv"], b_out_hpf)
    ref = model.grads_autograd(*args)
    got = model.grads_closed(*args)
    for k, name in enumerate(("a_mag", "a_real", "a_imag")):
        err = model.rel_err(got[k], ref[k])
        print("%s: %.3g" % (name, err))
        assert err <= 1.0e-9
        if kind == "unvoiced" and k > 0:
            assert not ref[k].any() and not got[k].any()
        else:
            assert ref[k].any()


def test_ends_and_zero_phase_conventions():
    """|S| at bins 0 and N/2 with S == 0, and den == 0: the closed form's conventions are the model's (where-before-sqrt)."""
    N, H = 1024, 513
    rng = np.random.RandomState(9)
    F = 3
    m = np.abs(rng.randn(F, H)) + 0.1
    a, b = rng.randn(F, H), rng.randn(F, H)
    a[0, 5:9] = b[0, 5:9] = 0.0
    P = np.abs(rng.randn(F, H))
    ns = rng.randn(F, H) + 1j * rng.randn(F, H)
    ns[1, 0] = 0.0
    P[1, 0] = 0.0                      # S_0 == 0 in frame 1
    gwin = rng.randn(F, N)
    gm, ga, gb = model.frame_grads_closed(m, a, b, P, ns, gwin, N)
    assert np.all(np.isfinite(gm)) and np.all(np.isfinite(ga)) and np.all(np.isfinite(gb))
    assert gm[1, 0] == 0.0 and ga[1, 0] == 0.0
    G = np.fft.fft(np.fft.ifftshift(gwin, axes=1), axis=1)[:, :H] * (2.0 / N)
    assert np.allclose(ga[0, 5:9], (m * P * G.real)[0, 5:9]) and np.allclose(gb[0, 5:9], (m * P * G.imag)[0, 5:9])


@pytest.mark.parametrize("fs", [16000, 48000])
def test_reversed_filter_is_the_adjoint_of_the_high_pass(fs):
    """The dense lower-triangular Toeplitz matrix of the filter's impulse response against the filter, and its transpose
    against the reversed filter.  A filter that is not the adjoint misses by O(1); what is left here is the direct form's
    own rounding (see test_model_forward_matches_the_oracle) -- measured 2.1e-10 / 2.0e-10 of the peak at 16 kHz and
    3.6e-9 / 2.4e-9 at 48 kHz over 300 samples, stated at 3 x that."""
    n = 300
    b, a = model.hpf_coefficients(fs)
    imp = signal.lfilter(b, a, np.r_[1.0, np.zeros(n - 1)])
    Hm = np.zeros((n, n))
    for j in range(n):
        Hm[j:, j] = imp[:n - j]
    rng = np.random.RandomState(1)
    x, g = rng.randn(n), rng.randn(n)
    tol_f, tol_a = (1.1e-8, 7.2e-9) if fs == 48000 else (6.3e-10, 6.0e-10)
    e_f = np.max(np.abs(Hm @ x - model.hpf(x, fs))) / np.max(np.abs(x))
    got, want = model.hpf_adjoint(g, fs), Hm.T @ g
    e_a = np.max(np.abs(got - want)) / np.max(np.abs(want))
    print("fs %d: forward %.3g, adjoint %.3g" % (fs, e_f, e_a))
    assert e_f <= tol_f and e_a <= tol_a
    assert np.max(np.abs(model.hpf(g, fs) - want)) > 1e-2 * np.max(np.abs(want))     # the filter itself is not its adjoint


def test_argument_errors_without_gpu():
    from magphase_amd import _lib

    lib = _lib.load()
    p = 64     # any non-null address: the arguments are refused before anything is dereferenced

    def bwd(fft_len=1024, total=100, n_frames=4, ld=513, ld_grad=513, n_per=100, tables=p, noise=p, grads=(p, p, p),
            grad_out=p):
        return lib.mpx_synthesis_compressed_backward(None, fft_len, tables, grad_out, total, p, p, p, n_frames, p, p, p, ld,
                                                     noise, p, p, p, p, p, p, p, p, p, p, p, n_per, grads[0], grads[1],
                                                     grads[2], ld_grad)

    for kw, word in (({"fft_len": 1000}, b"fft_len"), ({"n_frames": -1}, b"negative"), ({"total": -1}, b"negative"),
                     ({"ld": 512}, b"ld"), ({"ld_grad": 100}, b"ld"), ({"n_per": -1}, b"n_per"), ({"n_per": 514}, b"n_per"),
                     ({"tables": None}, b"null"), ({"noise": None}, b"null"), ({"grad_out": None}, b"null")):
        assert bwd(**kw) == -1 and word in lib.mpx_last_error(), kw
    assert bwd(n_frames=0, tables=None) == 0                    # no frames: nothing launched
    assert bwd(grads=(None, None, None), tables=None) == 0      # nothing asked for

    def unw(n_bins=513, ld_e=513, ld_g=513, mag_dim=60, n_mag=5, o_mag=p, ld_ph=513, n_ph_bins=192, phase_dim=45, n_ph=5,
            o_real=p, o_imag=p, e_mag=p, g_real=p, u_phase=p):
        return lib.mpx_mel_unwarp_backward(None, n_bins, e_mag, ld_e, p, ld_g, p, mag_dim, n_mag, o_mag, g_real, p, ld_ph,
                                           n_ph_bins, u_phase, phase_dim, n_ph, o_real, o_imag)

    for kw, word in (({"n_bins": 0}, b"size"), ({"n_mag": -1}, b"size"), ({"n_ph": -1}, b"size"), ({"ld_e": 512}, b"pitch"),
                     ({"ld_g": 100}, b"pitch"), ({"mag_dim": 65}, b"1..64"), ({"phase_dim": 0}, b"1..64"),
                     ({"n_ph_bins": 514}, b"n_phase_bins"), ({"n_ph_bins": -1}, b"n_phase_bins"),
                     ({"ld_ph": 100}, b"n_phase_bins"), ({"e_mag": None}, b"null"), ({"g_real": None}, b"null"),
                     ({"u_phase": None}, b"null")):
        assert unw(**kw) == -1 and word in lib.mpx_last_error(), kw
    assert unw(n_mag=0, n_ph=0) == 0
    assert unw(o_mag=None, o_real=None, o_imag=None, mag_dim=99, phase_dim=99) == 0
    assert unw(o_mag=None, mag_dim=99, n_ph=0) == 0
