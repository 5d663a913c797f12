"""CPU: the float64 model of the type-2 synthesis (tests/type2_synthesis_autograd_model.py) against the numpy restatement
that is pinned to golden g17 (tests/type2_synthesis_model.py), its closed-form gradients against torch autograd of its
forward, the reversed elliptic filter against a dense filter matrix, the type-2 end bins against type 1's, and the
argument checks of mpx_synthesis_compressed_type2_backward and of the plan.  Needs no GPU."""
import inspect

import numpy as np
import pytest
from scipy import signal

import compressed_synthesis_autograd_model as model1
import type2_synthesis_autograd_model as model
import type2_synthesis_model as t2


def _case(fs, N, rate, pd, ap_win, kind, hf, seed, n_rows=24, mag_dim=60):
    rng = np.random.RandomState(seed)
    lf0 = model.lf0_track(rng, n_rows, kind, fs)
    a_mag, a_real, a_imag = model.features(rng, n_rows, mag_dim, pd)
    tab = model.tables(lf0, fs, N, rate, ap_win)
    cst = model.constants(fs, N, mag_dim, pd, hf)
    noise = rng.uniform(-1, 1, tab["ns_len"])
    ns, inv = model.noise_spectra(noise, tab, N)
    return dict(lf0=lf0, feats=(a_mag, a_real, a_imag), tab=tab, cst=cst, noise=noise, ns=ns, inv=inv, rng=rng)


# every value of every axis the issue names, each pair (size, rate) and each voicing with each rate
_FORWARD_CASES = [(fs, N, rate, pd, ap, kind, hf)
                  for fs, N in ((16000, 2048), (48000, 4096))
                  for rate, pd, ap, kind, hf in ((-1.0, 45, True, "mixed", 1.0), (-1.0, 10, False, "unvoiced", 1.7),
                                                 (5.0, 45, False, "voiced", 1.7), (5.0, 60, True, "mixed", 1.0),
                                                 (4.0, 45, True, "mixed", 1.7), (4.0, 64, False, "voiced", 1.0),
                                                 (4.0, 10, True, "unvoiced", 1.0), (-1.0, 45, True, "voiced", 1.0))]


@pytest.mark.parametrize("fs,N,rate,pd,ap_win,kind,hf", _FORWARD_CASES)
def test_model_forward_matches_the_pinned_restatement(fs, N, rate, pd, ap_win, kind, hf):
    """Two float64 statements of one formula on the same explicit noise: the difference is rounding in another order.
    Before the filter the bound is the one the type-1 host test states for the same comparison, 4.5e-15 of the peak
    (measured here: 1.48e-15).  After the elliptic filter, calibrated here over these cases, each stated figure 3 x the
    worst case measured:
      16 kHz   measured 2.31e-10, stated 6.9e-10;
      48 kHz   measured 9.39e-9, stated 2.8e-8.
    The reason is the one DESIGN.md section 3.3k gives for the Butterworth: scipy's lfilter runs the fourth-order filter in
    direct form, its poles lie close to z = 1 (closer at 48 kHz), and its own rounding, fed back through 1 / A(z), is of
    this size -- inputs that agree to 1e-15 come out this far apart.  That is the reference's own error: the waveforms
    before the filter are compared at 4.5e-15 in the same test."""
    import torch

    c = _case(fs, N, rate, pd, ap_win, kind, hf, 3)
    want, dbg = t2.synthesis(*c["feats"], c["lf0"], fs, fft_len=N, hf_slope_coeff=hf, b_voi_ap_win=ap_win,
                             const_rate_ms=rate, v_noise=c["noise"])
    t = [torch.from_numpy(x) for x in c["feats"]]
    got = model.forward_torch(t[0], t[1], t[2], c["tab"], c["cst"], c["ns"], c["inv"]).numpy()
    pre = model.forward_torch(t[0], t[1], t[2], c["tab"], c["cst"], c["ns"], c["inv"], return_pre=True).numpy()
    assert got.shape == want.shape and np.max(np.abs(want)) > 0
    assert np.array_equal(dbg["v_voi"], c["tab"]["voiced"]) and np.array_equal(dbg["v_pm"], c["tab"]["v_pm"])
    assert abs(1.0 / c["inv"][0] - dbg["rms_spec"]) <= 1e-14 * dbg["rms_spec"]
    err_pre = float(np.max(np.abs(pre - dbg["v_pre_hpf"])) / np.max(np.abs(dbg["v_pre_hpf"])))
    err = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
    print("fs %d N %d rate %g pd %d ap_win %s %s hf %g: %.3g of the peak (%.3g before the filter)"
          % (fs, N, rate, pd, ap_win, kind, hf, err, err_pre))
    assert err_pre <= 4.5e-15
    assert err <= (2.8e-8 if fs == 48000 else 6.9e-10)


@pytest.mark.parametrize("fs,N,rate,pd,kind,hf", [(16000, 1024, -1.0, 10, "mixed", 1.0),
                                                   (16000, 1024, 5.0, 45, "mixed", 1.7),
                                                   (16000, 2048, 4.0, 60, "voiced", 1.0),
                                                   (16000, 1024, 4.0, 64, "mixed", 1.7),
                                                   (48000, 4096, -1.0, 45, "mixed", 1.7),
                                                   (48000, 4096, 5.0, 10, "unvoiced", 1.0)])
def test_closed_form_equals_autograd(fs, N, rate, pd, kind, hf):
    c = _case(fs, N, rate, pd, True, kind, hf, 5, n_rows=16)
    a_mag, a_real, a_imag = c["feats"]
    if kind != "unvoiced":   # a voiced bin with a == b == 0 needs whole zero rows of coefficients: one such row
        v_row = int(c["tab"]["row0"][np.flatnonzero(c["tab"]["voiced"])[0]])
        a_real[v_row] = a_imag[v_row] = 0.0
    gy = c["rng"].randn(c["tab"]["out_len"])
    args = (a_mag, a_real, a_imag, gy, c["tab"], c["cst"], c["ns"], c["inv"])
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
        if k > 0 and pd > 60:     # phase_dim > mag_dim: the forward never reads the columns from mag_dim on
            assert not ref[k][:, 60:].any() and not got[k][:, 60:].any() and got[k][:, :60].any()


def test_end_bins_are_type_2s_not_type_1s():
    """Re S at bins 0 and N/2: where Im T_end != 0 the closed form differs from type 1's |S| there and nowhere else, the
    phase gradient at the ends is not zero, and den == 0 keeps the m P gS convention."""
    N, H = 1024, 513
    rng = np.random.RandomState(9)
    F = 3
    m = np.abs(rng.randn(F, H)) + 0.1
    a, b = rng.randn(F, H), rng.randn(F, H)
    a[0, 5:9] = b[0, 5:9] = 0.0
    a[2, 0] = b[2, 0] = 0.0
    P = np.abs(rng.randn(F, H))
    ns = rng.randn(F, H) + 1j * rng.randn(F, H)        # Im Ns != 0 at the ends: Im T_end != 0
    ns[1, 0] = 0.0
    P[1, 0] = 0.0                                      # S_0 == 0 in frame 1
    gwin = rng.randn(F, N)
    g2 = model.frame_grads_closed(m, a, b, P, ns, gwin, N)
    g1 = model1.frame_grads_closed(m, a, b, P, ns, gwin, N)
    assert all(np.all(np.isfinite(x)) for x in g2)
    G = np.fft.fft(np.fft.ifftshift(gwin, axes=1), axis=1)[:, :H]
    T = P * (a + 1j * b) / np.where(a * a + b * b == 0, 1.0, np.sqrt(a * a + b * b)) + ns
    for k in (0, H - 1):
        assert np.allclose(g2[0][:, k], T[:, k].real * G[:, k].real / N, rtol=1e-12, atol=0)     # grad m = Re T Re gS
        big = np.abs(g2[0][:, k]) > 1e-6
        assert np.all(np.abs(g1[0][:, k] - g2[0][:, k])[big] > 1e-3 * np.abs(g2[0][:, k])[big]) and big.any()
        nz = (a[:, k] != 0) & (P[:, k] != 0)
        assert np.all(g2[2][nz, k] != 0.0)             # grad b at the ends: -(m P / den) u_i u_r Re gS
    for x1, x2 in zip(g1, g2):
        assert np.array_equal(x1[:, 1:-1], x2[:, 1:-1])
    assert g2[0][1, 0] == 0.0 and g2[1][1, 0] == 0.0   # T_0 == 0 and P_0 == 0 in frame 1
    assert np.allclose(g2[1][0, 5:9], (m * P * G.real * 2 / N)[0, 5:9]) and np.allclose(g2[2][0, 5:9],
                                                                                       (m * P * G.imag * 2 / N)[0, 5:9])
    assert np.isclose(g2[1][2, 0], (m * P * G.real / N)[2, 0]) and g2[2][2, 0] == 0.0


@pytest.mark.parametrize("fs", [16000, 48000])
def test_reversed_filter_is_the_adjoint_of_the_elliptic_high_pass(fs):
    """The dense lower-triangular Toeplitz matrix of the filter's impulse response against the filter, and its transpose
    against the reversed filter.  A filter that is not the adjoint misses by O(1); what is left is the direct form's own
    rounding (see test_model_forward_matches_the_pinned_restatement) -- measured 4.63e-11 / 8.86e-11 of the peak at 16 kHz
    and 2.97e-10 / 2.37e-9 at 48 kHz over 300 samples, stated at 3 x that."""
    n = 300
    b, a = model.hpf_coefficients(fs)
    imp = signal.lfilter(b, a, np.r_[1.0, np.zeros(n - 1)])
    Hm = np.zeros((n, n))
    for j in range(n):
        Hm[j:, j] = imp[:n - j]
    rng = np.random.RandomState(1)
    x, g = rng.randn(n), rng.randn(n)
    tol_f, tol_a = (8.9e-10, 7.1e-9) if fs == 48000 else (1.4e-10, 2.7e-10)
    assert np.array_equal(model.hpf(x, fs), t2.output_filter(x, fs))         # the pinned restatement's filter
    e_f = np.max(np.abs(Hm @ x - model.hpf(x, fs))) / np.max(np.abs(x))
    got, want = model.hpf_adjoint(g, fs), Hm.T @ g
    e_a = np.max(np.abs(got - want)) / np.max(np.abs(want))
    print("fs %d: forward %.3g, adjoint %.3g" % (fs, e_f, e_a))
    assert e_f <= tol_f and e_a <= tol_a
    assert np.max(np.abs(model.hpf(g, fs) - want)) > 1e-2 * np.max(np.abs(want))     # the filter itself is not its adjoint
    assert np.max(np.abs(model1.hpf_adjoint(g, fs) - want)) > 1e-2 * np.max(np.abs(want))   # nor is type 1's Butterworth


def test_argument_errors_without_gpu():
    from magphase_amd import _lib, plans

    lib = _lib.load()
    p = 64     # any non-null address: the arguments are refused before anything is dereferenced

    def bwd(fft_len=1024, total=100, n_frames=4, ld=513, ld_grad=513, n_per=100, tables=p, noise=p, grads=(p, p, p),
            grad_out=p):
        return lib.mpx_synthesis_compressed_type2_backward(None, fft_len, tables, grad_out, total, p, p, p, n_frames, p, p,
                                                           p, ld, noise, p, p, p, p, p, p, p, p, p, p, p, n_per, grads[0],
                                                           grads[1], grads[2], ld_grad)

    for kw, word in (({"fft_len": 1000}, b"fft_len"), ({"n_frames": -1}, b"negative"), ({"total": -1}, b"negative"),
                     ({"ld": 512}, b"ld"), ({"ld_grad": 100}, b"ld"), ({"n_per": -1}, b"n_per"), ({"n_per": 514}, b"n_per"),
                     ({"tables": None}, b"null"), ({"noise": None}, b"null"), ({"grad_out": None}, b"null")):
        assert bwd(**kw) == -1, kw
        msg = lib.mpx_last_error()
        assert word in msg and msg.startswith(b"mpx_synthesis_compressed_type2_backward:"), (kw, msg)
    assert bwd(n_frames=0, tables=None) == 0                    # no frames: nothing launched
    assert bwd(grads=(None, None, None), tables=None) == 0      # nothing asked for
    # the type-1 entry still speaks under its own name
    assert lib.mpx_synthesis_compressed_backward(None, 1000, p, p, 100, p, p, p, 4, p, p, p, 513, *([p] * 12), 100, p, p, p,
                                                 513) == -1
    assert lib.mpx_last_error().startswith(b"mpx_synthesis_compressed_backward:")

    # the plans name their backward entries; more than 64 columns are refused by name before any launch
    assert plans.CompressedSynthesisPlan._bwd_entry == "mpx_synthesis_compressed_backward"
    assert plans.Type2SynthesisPlan._bwd_entry == "mpx_synthesis_compressed_type2_backward"
    assert plans.Type2SynthesisPlan._bwd_entry in _lib.SYMBOLS
    assert _lib.PROTOTYPES[plans.Type2SynthesisPlan._bwd_entry] == _lib.PROTOTYPES[plans.CompressedSynthesisPlan._bwd_entry]
    plans.check_type2_grad_dims(64, 64)
    with pytest.raises(NotImplementedError, match="mag_dim"):
        plans.check_type2_grad_dims(65, 45)
    with pytest.raises(NotImplementedError, match="phase_dim"):
        plans.check_type2_grad_dims(60, 65)
    sig = inspect.signature(plans.CompressedSynthesisPlan.adjoint_hpf)
    assert sig.parameters["design"].default == "butter40"


def test_cpu_tensors_that_require_grad_take_the_host_path():
    """The predicate of the device path: CPU tensors, a host return and no_grad are not differentiated."""
    import torch

    from magphase_amd import hostmath as hm

    x = torch.zeros(4, 60, requires_grad=True)
    utts = [(x, torch.zeros(4, 45), torch.zeros(4, 45), np.zeros(4))]
    assert not hm.wants_grad(True, [m for u in utts for m in u[:3]])
    assert not hm.wants_grad(False, [m for u in utts for m in u[:3]])
