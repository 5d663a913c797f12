"""GPU: Griffin-Lim with the initial phase and the fold on the device -- k_gl_fold (mpx_griffin_lim_fold) directly against
the fp64 model (tests/griffin_lim_device_model.py), numpy's draws continued on the device, griffin_lim_batch(fold='device')
end to end against tests/griffin_lim_model.py with the measures of tests/test_gpu_griffin_lim.py, device-tensor inputs, and
griffin_lim_from_mag_batch against the oracle's unwarp + shifts + the Griffin-Lim model.

The kernel's bound.  The model and the kernel evaluate the same float64 expression on the same float32 inputs; they
differ by their sin / cos (each within one float64 ulp of the true value: 2^-53 for |value| <= 1, so 2 * 2^-53 between two
implementations) and by a few roundings of relative size 2^-53.  c = (cr, ci) is a half-sum of two such values per
component: |d cr|, |d ci| <= 2 * 2^-53, |d c| <= 2 sqrt(2) 2^-53.  The phasor c / |c| moves by at most |d c| / |c|, plus
three roundings (hypot, the division, the product) of 2^-53 each: <= 4 * 2^-53 / |c| for |c| <= 0.39, and below 2^-50 --
a 2^-26-th of the smallest float32 ulp near 1 -- otherwise.  mag' = M |c| moves by at most M |d c| <= M * 4 * 2^-53.  After
the single rounding to float32 an element therefore lies within ONE float32 ulp of the model's rounded value (the two
float64 values straddle at most one rounding boundary), except where that float64 term itself exceeds the ulp (a phasor
component that is tiny beside 1): there the bound is the term plus the ulp.  HALF has |c| = 1.  The tests choose phases
whose smallest |c| stays above 1e-6 (asserted on the model), where the term is at most 4.5e-10.

End-to-end tolerances are stated at <= 3 x the worst case measured on the MI355X against the float64 model
(tests/_tol.py records it; profiles/r27_griffin_lim_device_tolerance_report.json)."""
import contextlib
import io

import numpy as np
import pytest

import griffin_lim_device_model as gdm
import griffin_lim_model as glm
from _tol import within

pytestmark = pytest.mark.gpu

SEED = 2727
SENTINEL = -777.25
FRAME_COUNTS = (1, 2, 63, 64, 65, 257)
FORMS = {"half": gdm.HALF, "full": gdm.FULL, "words": gdm.WORDS}
TERM = 4.0 * 2.0 ** -53

# fold='device' end to end, beside the host fold's GL1_TOL 1e-6, GL_ITER_TOL {2: 1.1e-6, 3: 1.8e-6, 5: 4e-6} and
# GL_PHASE_TOL 2e-6 (tests/test_gpu_griffin_lim.py)
GLD1_TOL = 6e-7
GLD_ITER_TOL = {2: 9e-7, 3: 1.3e-6, 5: 3e-6}
GLD_PHASE_TOL = 2e-6
GLD_PHASE1_TOL = np.pi * 2.0 ** -24     # niters = 1: the kernel's float32 phase rows against the float64 draws (|phi| <= pi)
GLD_MINPH_SC_TOL = 0.075                # 'min_phase', niters > 1: the host fold's measure and reason
# griffin_lim_from_mag_batch against exp(oracle unwarp) -> oracle shifts / row interpolation -> the Griffin-Lim model
GLM1_TOL = 9e-7
GLM_ITER_TOL = 4e-6
GLM_MINPH1_TOL = 6e-7
# 'min_phase' beyond the first synthesis is set by rounding (tests/test_gpu_griffin_lim.py::test_min_phase_iterations).  Here
# the target itself carries the float32 unwarp's error, about 1e-6 of M: perturbing M by 1e-6 (relative, Gaussian) moves the
# float64 model's own spectral convergence at niters = 3 by up to 0.18 of its value on this file's inputs (three draws per
# input, all six modes; the figure is the model's alone, computed without the device).  The bound is that sensitivity.
GLM_MINPH_SC_TOL = 0.2


def _mp():
    from magphase_amd import magphase as mp
    return mp


def _engine():
    from magphase_amd.engine import get_engine
    return get_engine()


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------------ the kernel directly
def _operands(rs, F, N, form):
    """Random (float32 magnitudes [F x H], the phase operand of `form`)."""
    H = N // 2 + 1
    m = (rs.rand(F, H) * 3.0).astype(np.float32)
    if form == "half":
        ph = (2 * np.pi * (rs.rand(F, H) - 0.5)).astype(np.float32)   # junk (non-zero) in columns 0 and H - 1
    elif form == "full":
        ph = (2 * np.pi * (rs.rand(F, N) - 0.5)).astype(np.float32)
    else:
        ph = rs.randint(0, 2**32, size=2 * F * N, dtype=np.uint32)
    return m, ph


def _launch(N, form, m, ph, frame0=3, tail=2):
    """k_gl_fold on rows frame0 .. frame0 + F - 1 of pitched buffers: the outputs lie in sentinel-filled matrices, the
    magnitudes and the phase between NaN fences (the words, which have no NaN, between words of another draw).
    Returns the four output buffers (host, whole) and the row pitch."""
    import torch

    eng = _engine()
    F, H = m.shape
    ld = int(eng.lib.mpx_spec_ld(H))
    rows = frame0 + F + tail
    dev = eng.device
    mag = torch.full((rows, ld), float("nan"), dtype=torch.float32, device=dev)
    mag[frame0:frame0 + F, :H] = torch.from_numpy(m).to(dev)
    outs = [torch.full((rows, ld), SENTINEL, dtype=torch.float32, device=dev) for _ in range(4)]
    off = 0
    if form == "words":
        fence = np.random.RandomState(99).randint(0, 2**32, size=6, dtype=np.uint32)
        buf = np.concatenate((fence, ph, fence))
        phase = torch.from_numpy(buf.view(np.int32)).to(dev)
        off = 3   # samples: the words of the range start 6 words into the buffer
    else:
        w = ph.shape[1]
        full = torch.full((F + 2, w + 5), float("nan"), dtype=torch.float32, device=dev)
        full[1:1 + F, :w] = torch.from_numpy(ph).to(dev)
        phase = full[1:1 + F, :w]
    eng.griffin_lim_fold(N, form, mag[:, :H], phase, frame0, F, [o[:, :H] for o in outs[:3]], outs[3][:, :H],
                         phase_offset=off)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs], ld


def _compare(N, form, m, ph, label, frame0=3):
    F, H = m.shape
    outs, ld = _launch(N, form, m, ph, frame0=frame0)
    want = gdm.fold(m, ph, FORMS[form])
    mod = want[4]
    if form != "half":
        assert mod.min() > 1e-6, "the model's smallest |c| = %g: choose other phases" % mod.min()
    terms = (m.astype(np.float64) * TERM, TERM / mod, TERM / mod, np.zeros_like(mod))
    worst = 0.0
    for name, o, w, term in zip(("mag", "real", "imag", "phase"), outs, want[:4], terms):
        # nothing outside the range's H columns was written
        mask = np.ones(o.shape, dtype=bool)
        mask[frame0:frame0 + F, :H] = False
        assert np.all(o[mask] == np.float32(SENTINEL)), "%s: a store outside rows %d..%d x %d columns" % (name, frame0, frame0 + F, H)
        got = o[frame0:frame0 + F, :H].astype(np.float64)
        assert np.all(np.isfinite(got)), name     # (no fence was read, no sentinel left: every element was written)
        w32 = np.asarray(w, dtype=np.float32)
        ulp = gdm.ulp32(w32)
        tol = np.where(term > ulp, term + ulp, ulp)
        worst = max(worst, float(np.max(np.abs(got - w32.astype(np.float64)) / tol)))
    within(worst, 1.0, label)
    return outs


@pytest.mark.parametrize("form", ["half", "full", "words"])
@pytest.mark.parametrize("N", [1024, 2048, 4096])
def test_kernel_against_model(N, form):
    for F in FRAME_COUNTS:
        rs = np.random.RandomState(SEED + N + F)
        m, ph = _operands(rs, F, N, form)
        _compare(N, form, m, ph, "GLD_FOLD_ULP:" + form, frame0=3 if F != 64 else 0)


@pytest.mark.parametrize("N", [1024, 4096])
def test_kernel_directed_rows(N):
    H = N // 2 + 1
    rs = np.random.RandomState(SEED + N)
    # M = 0 rows, one-hot rows at bins 0, 1, N/2 - 1, N/2
    m = np.zeros((6, H), dtype=np.float32)
    for r, k in enumerate((0, 1, N // 2 - 1, N // 2)):
        m[2 + r, k] = 1.5
    for form in ("half", "full", "words"):
        _, ph = _operands(rs, 6, N, form)
        outs = _compare(N, form, m, ph, "GLD_FOLD_ULP:directed")
        got = outs[0][3:9, :H]
        assert np.all(got[:2] == 0.0) and np.count_nonzero(got) <= 4
    # phases of magnitude 40 rad (HALF and FULL)
    m = (rs.rand(3, H) + 0.5).astype(np.float32)
    big = (np.where(rs.rand(3, H) < 0.5, -1.0, 1.0) * (40.0 + rs.rand(3, H))).astype(np.float32)
    _compare(N, "half", m, big, "GLD_FOLD_ULP:directed")
    bigf = (np.where(rs.rand(3, N) < 0.5, -1.0, 1.0) * (40.0 + 0.01 * rs.rand(3, N))).astype(np.float32)
    _compare(N, "full", m, bigf, "GLD_FOLD_ULP:directed")
    # a FULL row with phi_{N-k} = phi_k: c = cos phi is real
    half = (2 * np.pi * (rs.rand(3, H) - 0.5)).astype(np.float32)
    sym = np.hstack((half, half[:, -2:0:-1]))
    outs = _compare(N, "full", m, sym, "GLD_FOLD_ULP:directed")
    assert np.all(outs[2][3:6, :H] == 0.0)
    want = np.cos(half.astype(np.float64))
    assert np.all(np.sign(outs[1][3:6, :H]) == np.sign(want * np.where(np.arange(H) % 2 == 0, 1.0, -1.0)))


# ------------------------------------------------------------------------------------------------ the draws
@pytest.mark.parametrize("N,F", [(1024, 65), (4096, 80)])   # one workgroup; more than one segment of 624 * 512 words
def test_random_draws_continue_numpys_stream(N, F):
    H = N // 2 + 1
    rs = np.random.RandomState(SEED)
    sizes = (F - 7, 3, 7, 2)       # 'random', 'linear', 'random', 'linear': the two draws are one contiguous stretch
    inits = ["random", "linear", "random", "linear"]
    utts = [(rs.rand(n, H) + 0.1, np.full(n, 150.0)) for n in sizes]
    assert (2 * F * N > 624 * 512) == (N == 4096)
    np.random.seed(SEED)
    host = [2 * np.pi * (np.random.rand(n, N) - 0.5)[:, :H] if i == "random" else None for n, i in zip(sizes, inits)]
    after = np.random.rand()
    np.random.seed(SEED)
    out = _quiet(_mp().griffin_lim_batch, utts, phase_init=inits, niters=1, fold="device")
    assert np.random.rand() == after
    lin = np.where(np.arange(H) % 2 == 0, 0.0, np.pi)
    for (v, ph), h, (m, _) in zip(out, host, utts):
        assert ph.dtype == np.float64 and ph.shape == m.shape and np.all(np.isfinite(v))
        if h is None:
            assert np.max(np.abs(np.abs(ph) - lin)) <= GLD_PHASE1_TOL
        else:
            within(np.max(np.abs(ph - h)), GLD_PHASE1_TOL, "GLD_PHASE1_TOL:random")


# ------------------------------------------------------------------------------------------------ end to end
def _golden(golden_dir):
    return np.load(golden_dir + "/g13_griffin_lim.npz")


def _ndarray_init(shape, fs):
    return _f32(2 * np.pi * (np.random.RandomState(SEED + fs).rand(*shape) - 0.5))   # (exact in float32: one input for both)


def _circ(a, b, w):
    d = np.angle(np.exp(1j * (np.asarray(a, np.float64) - np.asarray(b, np.float64))))
    return float(np.sum(w * np.abs(d)) / np.sum(w))


_MODEL = {}


def _model(g, tag, fs, init, niters):
    """The float64 model's (signal, phase, generator cursor), computed once per case and left unchanged."""
    key = (tag, init, niters)
    if key not in _MODEL:
        m, sh = g[tag + "_mag"], g[tag + "_shift"]
        np.random.seed(SEED)
        ref, ph = glm.griffin_lim(m, sh, _ndarray_init(m.shape, fs) if init == "ndarray" else init, niters)
        _MODEL[key] = (ref, ph, np.random.rand())
    return _MODEL[key]


@pytest.mark.parametrize("niters", [1, 2, 3, 5])
@pytest.mark.parametrize("init", ["random", "linear", "ndarray"])
def test_device_fold_against_model(golden_dir, niters, init):
    g = _golden(golden_dir)
    for tag, fs in (("16k", 16000), ("48k", 48000)):
        m, sh = g[tag + "_mag"], g[tag + "_shift"]
        ref, ref_ph, after = _model(g, tag, fs, init, niters)
        arg = _ndarray_init(m.shape, fs) if init == "ndarray" else init
        if init == "ndarray":
            arg[:, 0], arg[:, -1] = 0.3, -0.4     # the reference zeroes them in place; so does this
        np.random.seed(SEED)
        v, ph = _quiet(_mp().griffin_lim_batch, [(m, sh)], phase_init=[arg], niters=niters, fold="device")[0]
        assert np.random.rand() == after
        assert v.dtype == np.float64 and v.shape == ref.shape and ph.shape == m.shape
        err = np.max(np.abs(v - ref)) / np.max(np.abs(ref))
        if niters == 1:
            within(err, GLD1_TOL, "GLD1_TOL:sig")
            within(np.max(np.abs(np.angle(np.exp(1j * (ph - ref_ph))))), GLD_PHASE1_TOL, "GLD_PHASE1_TOL:" + init)
        else:
            within(err, GLD_ITER_TOL[niters], "GLD_ITER_TOL:%d" % niters)
        if niters == 5:
            within(_circ(ph, ref_ph, m), GLD_PHASE_TOL, "GLD_PHASE_TOL")
        if init == "ndarray":
            assert np.all(arg[:, 0] == 0) and np.all(arg[:, -1] == 0)


@pytest.mark.parametrize("niters", [1, 2, 5])
def test_device_fold_min_phase(golden_dir, niters):
    """'min_phase' keeps the mpx_min_phase route.  niters = 1: the signal per sample; beyond, the model's spectral
    convergence only, for the reason given in tests/test_gpu_griffin_lim.py::test_min_phase_iterations."""
    g = _golden(golden_dir)
    mp = _mp()
    for tag in ("16k", "48k"):
        m, sh = g[tag + "_mag"], g[tag + "_shift"]
        v, ph = _quiet(mp.griffin_lim_batch, [(m, sh)], phase_init="min_phase", niters=niters, fold="device")[0]
        vh, phh = _quiet(mp.griffin_lim_batch, [(m, sh)], phase_init="min_phase", niters=niters, fold="host")[0]
        assert v.shape == vh.shape and np.all(np.isfinite(v)) and np.all(np.abs(ph) <= np.float32(np.pi))
        if niters == 1:   # the same launches on the same rows
            assert np.array_equal(v, vh) and np.array_equal(ph, phh)
            continue
        ref, _ = glm.griffin_lim(m, sh, "min_phase", niters)
        v1, _ = _quiet(mp.griffin_lim_batch, [(m, sh)], phase_init="min_phase", niters=1, fold="device")[0]
        sc, sc1, sc_ref = (glm.spectral_convergence(x, m, sh) for x in (v, v1, ref))
        assert sc < sc1
        within(abs(sc - sc_ref) / sc_ref, GLD_MINPH_SC_TOL, "GLD_MINPH_SC_TOL")


# ------------------------------------------------------------------------------------------------ device tensors
@pytest.mark.parametrize("dtype", ["float16", "bfloat16", "float64"])
def test_device_tensor_inputs(golden_dir, dtype):
    import torch

    g = _golden(golden_dir)
    mp, eng = _mp(), _engine()
    m, sh = g["16k_mag"][:40], g["16k_shift"][:40]
    F, H = m.shape
    tdt = getattr(torch, dtype)
    wide = torch.zeros((F, H + 11), dtype=tdt, device=eng.device)
    wide[:, 4:4 + H] = torch.from_numpy(m).to(eng.device).to(tdt)
    m_dev = wide[:, 4:4 + H]
    assert m_dev.stride(0) == H + 11
    m_host = m_dev.float().cpu().numpy() if dtype != "float64" else _f32(m_dev.cpu().numpy())
    if dtype == "float64":   # the same float32 values on both sides
        wide[:, 4:4 + H] = torch.from_numpy(m_host).to(eng.device)
    init_host = _ndarray_init(m.shape, 16000).astype(np.float32)
    init_dev = torch.from_numpy(init_host).to(eng.device)
    keep_m, keep_i = wide.clone(), init_dev.clone()
    for niters in (1, 3):
        for init in ("random", "array"):
            np.random.seed(SEED)
            a = _quiet(mp.griffin_lim_batch, [(m_dev, sh)], phase_init=[init_dev] if init == "array" else "random",
                       niters=niters)[0]
            np.random.seed(SEED)
            b = _quiet(mp.griffin_lim_batch, [(m_host, sh)], phase_init=[init_host.copy()] if init == "array" else "random",
                       niters=niters, fold="device")[0]
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert torch.equal(wide, keep_m) and torch.equal(init_dev, keep_i)     # device tensors are never written
    assert init_dev[0, 0] != 0 and init_dev[0, -1] != 0
    # return_device: float32 views on the device, the same values
    np.random.seed(SEED)
    d = _quiet(mp.griffin_lim_batch, [(m_dev, sh)], phase_init="random", niters=3, return_device=True)[0]
    np.random.seed(SEED)
    h = _quiet(mp.griffin_lim_batch, [(m_dev, sh)], phase_init="random", niters=3)[0]
    assert d[0].device == eng.device and d[0].dtype == torch.float32 and tuple(d[1].shape) == (F, H)
    assert np.array_equal(d[0].double().cpu().numpy(), h[0]) and np.array_equal(d[1].double().cpu().numpy(), h[1])


def test_host_fold_keyword_changes_nothing(golden_dir):
    g = _golden(golden_dir)
    mp = _mp()
    m, sh = g["16k_mag"][:30], g["16k_shift"][:30]
    for init in ("random", "linear", "min_phase", "ndarray"):
        for niters in (1, 2):
            res = []
            for kw in ({}, {"fold": "host"}):
                arg = _ndarray_init(m.shape, 16000) + 0.1 if init == "ndarray" else init
                np.random.seed(SEED)
                res.append(_quiet(mp.griffin_lim_batch, [(m, sh)], phase_init=[arg], niters=niters, **kw)[0]
                           + (np.random.rand(),))
                if init == "ndarray":
                    assert np.all(arg[:, 0] == 0) and np.all(arg[:, -1] == 0)
            assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1]) and res[0][2] == res[1][2]


# ------------------------------------------------------------------------------------------------ from mel-log magnitudes
def _mel_utt(fs, rows, seed, mag_dim=60):
    """A few tens of rows of smooth mel-log magnitudes and an lf0 contour with an unvoiced stretch."""
    rs = np.random.RandomState(seed)
    k = np.arange(mag_dim)[None, :] / mag_dim
    t = np.arange(rows)[:, None] / rows
    mml = -3.0 + 1.5 * np.cos(2 * np.pi * (k * (1.5 + t) + 0.3 * seed)) * np.exp(-2 * k) + 0.05 * rs.randn(rows, mag_dim)
    f0 = 110.0 + 60.0 * np.sin(2 * np.pi * (0.7 * t[:, 0] + 0.1 * seed)) ** 2
    lf0 = np.log(f0)
    lf0[rows // 2:rows // 2 + 5] = -1e10
    return mml, lf0


_MEL_MODES = {"variable": {}, "const_rate": {"b_const_rate": True}, "fbank": {"b_fbank_mel": True}}


@pytest.mark.parametrize("mode", sorted(_MEL_MODES))
@pytest.mark.parametrize("fs", [16000, 48000])
def test_from_mag_against_model(fs, mode):
    import torch

    mp, eng = _mp(), _engine()
    kw = _MEL_MODES[mode]
    N = 2048 if fs == 16000 else 4096
    utts = [_mel_utt(fs, 30, 1), _mel_utt(fs, 41, 2)]
    for init, niters in (("linear", 1), ("linear", 3), ("random", 1), ("random", 3), ("min_phase", 1), ("min_phase", 3)):
        np.random.seed(SEED)
        refs = [gdm.from_mag(mml, lf0, fs, N, init, niters, **kw) for mml, lf0 in utts]
        after = np.random.rand()
        np.random.seed(SEED)
        sigs = _quiet(mp.griffin_lim_from_mag_batch, utts, fs, phase_init=init, niters=niters, **kw)
        assert np.random.rand() == after
        for v, (ref, m_mag, v_shift) in zip(sigs, refs):
            assert v.dtype == np.float64 and v.shape == ref.shape
            err = np.max(np.abs(v - ref)) / np.max(np.abs(ref))
            if init == "min_phase" and niters > 1:
                sc, sc_ref = (glm.spectral_convergence(x, m_mag, v_shift) for x in (v, ref))
                within(abs(sc - sc_ref) / sc_ref, GLM_MINPH_SC_TOL, "GLM_MINPH_SC_TOL")
            elif init == "min_phase":
                within(err, GLM_MINPH1_TOL, "GLM_MINPH1_TOL")
            else:
                within(err, GLM1_TOL if niters == 1 else GLM_ITER_TOL, "GLM1_TOL" if niters == 1 else "GLM_ITER_TOL")
    # device tensors (a column slice of a wider model output), return_device: the same samples
    wide = [torch.from_numpy(np.hstack((mml, np.zeros((mml.shape[0], 5))))).to(eng.device) for mml, _ in utts]
    dev_utts = [(w[:, :60], torch.from_numpy(lf0).to(eng.device)) for w, (_, lf0) in zip(wide, utts)]
    d = _quiet(mp.griffin_lim_from_mag_batch, dev_utts, fs, phase_init="linear", niters=2, return_device=True, **kw)
    h = _quiet(mp.griffin_lim_from_mag_batch, utts, fs, phase_init="linear", niters=2, **kw)
    for a, b in zip(d, h):
        assert a.device == eng.device and a.dtype == torch.float32
        assert np.array_equal(a.double().cpu().numpy(), b)


@pytest.mark.parametrize("b_const_rate", [False, True])
def test_from_mag_length_state_and_domain(b_const_rate):
    mp = _mp()
    fs = 16000
    utts = [_mel_utt(fs, 33, 3), _mel_utt(fs, 24, 4)]
    np.random.seed(SEED)
    state = np.random.get_state()
    sigs = _quiet(mp.griffin_lim_from_mag_batch, utts, fs, phase_init="min_phase", niters=2, b_const_rate=b_const_rate)
    st = np.random.get_state()
    assert st[2] == state[2] and np.array_equal(st[1], state[1])     # nothing drawn: no noise, no random init
    syn = mp.synthesis_from_mag_batch(utts, fs, b_const_rate=b_const_rate)
    assert [len(a) for a in sigs] == [len(b) for b in syn]
    one = _quiet(mp.griffin_lim_from_mag, utts[1][0], utts[1][1], fs, niters=2, b_const_rate=b_const_rate)
    assert one.dtype == np.float64 and one.shape == sigs[1].shape and np.all(np.isfinite(one))
    low = utts[1][1].copy()
    low[7] = np.log(10.0)
    np.random.seed(SEED)
    with pytest.raises(ValueError, match=r"utts\[1\]"):
        mp.griffin_lim_from_mag_batch([utts[0], (utts[1][0], low)], fs, b_const_rate=b_const_rate)
    assert np.random.get_state()[2] == state[2]
