"""GPU: griffin_lim / griffin_lim_batch (k_synth_ola_pair for the first synthesis, k_griffin_lim_pair per iteration)
against the reference's golden (tests/golden/g13_griffin_lim.npz) and the fp64 model (tests/griffin_lim_model.py).
Tolerances are <= 3 x the worst case measured on the MI355X (tests/_tol.py records it)."""
import contextlib
import io

import numpy as np
import pytest

import griffin_lim_model as glm
from _tol import within
from magphase_amd import synthetic as syn
from oracle import magphase_oracle as orc

pytestmark = pytest.mark.gpu

SEED = 1313
GL1_TOL = 1e-6       # niters = 1: the lossless synthesis' PCM_TOL (tests/test_gpu_lossless.py)
GL_ITER_TOL = {2: 1.1e-6, 3: 1.8e-6, 5: 4e-6}   # per-sample error / peak after n syntheses
GL_SC30_TOL = 1.5e-6   # niters = 30, 'random': |SC_dev - SC_model| / SC_model
GL_PHASE_TOL = 2e-6  # magnitude-weighted mean circular error of the returned phase (rad), niters 5
GL_MINPH_SC_TOL = 0.075  # 'min_phase', niters 2 / 5: |SC_dev - SC_model| / SC_model (see test_min_phase_iterations)
GL_BATCH_TOL = 1.8e-6  # batch (many runs, head strips) vs one call per utterance, / peak


def _mp():
    from magphase_amd import magphase as mp
    return mp


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _golden(golden_dir):
    return np.load(golden_dir + "/g13_griffin_lim.npz")


def _ndarray_init(shape, fs):
    return 2 * np.pi * (np.random.RandomState(SEED + fs).rand(*shape) - 0.5)


def _circ(a, b, w):
    d = np.angle(np.exp(1j * (np.asarray(a, np.float64) - np.asarray(b, np.float64))))
    return float(np.sum(w * np.abs(d)) / np.sum(w))


def _utt(fs, dur, u, fft_len=None, n_frames=None):
    pcm, pm_sec, voi = syn.make_utterance(u, dur_s=dur, fs=fs)
    m, _, _, _, _, sh = orc.analysis_lossless_from_epochs(syn.pcm_to_float(pcm), fs, pm_sec, voi, fft_len=fft_len)
    if n_frames:
        m, sh = m[:n_frames], sh[:n_frames]
    N = 2 * (m.shape[1] - 1)
    return m, np.minimum(sh, N // 2 - 1).astype(np.float64)


@pytest.mark.parametrize("init", ["random", "linear", "min_phase", "ndarray"])
def test_niters1_against_golden(golden_dir, init):
    g = _golden(golden_dir)
    m, sh = g["16k_mag"], g["16k_shift"]
    key = "16k_%s_1" % init
    np.random.seed(SEED)
    arg = _ndarray_init(m.shape, 16000) if init == "ndarray" else init
    v, ph = _quiet(_mp().griffin_lim, m, sh, phase_init=arg, niters=1)
    ref = g[key + "_sig"]
    assert v.dtype == np.float64 and v.shape == ref.shape and ph.shape == m.shape
    within(np.max(np.abs(v - ref)) / np.max(np.abs(ref)), GL1_TOL, "GL1_TOL:sig")
    within(_circ(ph, g[key + "_phase"], m), 1.8e-6 if init == "min_phase" else 1e-7, "GL1_TOL:phase-" + init)
    if init == "random":
        assert np.random.get_state()[2] == int(g[key + "_rng_pos"])
    if init == "ndarray":
        np.testing.assert_array_equal(arg, g[key + "_init_after"])


@pytest.mark.parametrize("niters", [2, 3, 5])
@pytest.mark.parametrize("init", ["random", "linear", "ndarray"])
def test_iterations_against_model(golden_dir, niters, init):
    g = _golden(golden_dir)
    for tag, fs in (("16k", 16000), ("48k", 48000)):
        m, sh = g[tag + "_mag"], g[tag + "_shift"]
        arg = (lambda: _ndarray_init(m.shape, fs)) if init == "ndarray" else (lambda: init)
        np.random.seed(SEED)
        ref, ref_ph = glm.griffin_lim(m, sh, arg(), niters)
        state = np.random.get_state()[2]
        np.random.seed(SEED)
        v, ph = _quiet(_mp().griffin_lim, m, sh, phase_init=arg(), niters=niters)
        assert np.random.get_state()[2] == state
        within(np.max(np.abs(v - ref)) / np.max(np.abs(ref)), GL_ITER_TOL[niters], "GL_ITER_TOL:%d" % niters)
        key = "%s_%s_%d" % (tag, init, niters)
        if key + "_sig" in g.files:   # the model is the reference here (test_griffin_lim_host); the golden directly too
            gs = g[key + "_sig"]
            within(np.max(np.abs(v - gs)) / np.max(np.abs(gs)), GL_ITER_TOL[niters], "GL_ITER_TOL:%d" % niters)
        if niters == 5:
            within(_circ(ph, ref_ph, m), GL_PHASE_TOL, "GL_PHASE_TOL")


@pytest.mark.parametrize("niters", [2, 5])
def test_min_phase_iterations(golden_dir, niters):
    """'min_phase' beyond the first synthesis is not held to the model sample by sample: its frames are minimum-phase
    responses that start N/2 before their epochs, so most analysis windows see only their residue (|X| ~ 1e-7 of the
    peak or exactly 0 in fp64) and the phase the next synthesis takes from them is set by rounding.  Perturbing the first
    synthesis by 1e-7 of its peak moves the model's phase by 0.85 rad (magnitude-weighted mean); M perturbed by 1e-7
    moves the model's niters = 2 output by 0.9 of its peak -- but its spectral convergence by at most 23 % (16 kHz,
    niters 5).  Checked: finite output of the right length, phases in [-pi, pi], the iterations converge (SC below the
    first synthesis'), and SC within GL_MINPH_SC_TOL (relative) of the model's."""
    g = _golden(golden_dir)
    for tag in ("16k", "48k"):
        m, sh = g[tag + "_mag"], g[tag + "_shift"]
        v, ph = _quiet(_mp().griffin_lim, m, sh, phase_init="min_phase", niters=niters)
        v1, _ = _quiet(_mp().griffin_lim, m, sh, phase_init="min_phase", niters=1)
        ref, _ = glm.griffin_lim(m, sh, "min_phase", niters)
        assert v.shape == ref.shape and np.all(np.isfinite(v))
        assert np.all(np.abs(ph) <= np.float32(np.pi))
        sc, sc1, sc_ref = (glm.spectral_convergence(x, m, sh) for x in (v, v1, ref))
        assert sc < sc1
        within(abs(sc - sc_ref) / sc_ref, GL_MINPH_SC_TOL, "GL_MINPH_SC_TOL")


def test_niters30_spectral_convergence():
    m, sh = _utt(48000, 0.4, 5)
    np.random.seed(SEED)
    ref, _ = glm.griffin_lim(m, sh, "random", 30)
    np.random.seed(SEED)
    v, _ = _quiet(_mp().griffin_lim, m, sh, phase_init="random", niters=30)
    sc_ref = glm.spectral_convergence(ref, m, sh)
    sc_dev = glm.spectral_convergence(v, m, sh)
    np.random.seed(SEED)
    v1, _ = _quiet(_mp().griffin_lim, m, sh, phase_init="random", niters=1)
    assert sc_dev < glm.spectral_convergence(v1, m, sh)   # the iterations converge
    within(abs(sc_dev - sc_ref) / sc_ref, GL_SC30_TOL, "GL_SC30_TOL")
    within(np.max(np.abs(v - ref)) / np.max(np.abs(ref)), 2.5e-4, "GL_SC30_TOL:per-sample-drift-30")


def test_batch_equals_per_utterance_calls(monkeypatch):
    utts = [_utt(48000, d, u) for u, d in ((1, 0.3), (2, 0.15), (3, 0.25))]
    utts.append((utts[0][0][:1], np.array([700.0])))   # a lone frame
    inits = [_ndarray_init(m.shape, 48000 + i) for i, (m, _) in enumerate(utts)]
    np.random.seed(SEED)
    singles = [_quiet(_mp().griffin_lim, m, s, phase_init="random", niters=4) for m, s in utts]
    state = np.random.get_state()[2]
    monkeypatch.setenv("MAGPHASE_OLA_FRAMES_PER_RUN", "3")   # many runs and head strips
    np.random.seed(SEED)
    batch = _quiet(_mp().griffin_lim_batch, utts, phase_init="random", niters=4)
    assert np.random.get_state()[2] == state
    for (v1, p1), (v2, p2), (m, _) in zip(singles, batch, utts):
        assert v1.shape == v2.shape and p1.shape == p2.shape
        within(np.max(np.abs(v1 - v2)) / np.max(np.abs(v1)), GL_BATCH_TOL, "GL_BATCH_TOL")
    # a list of ndarray inits, each mutated as the reference mutates it
    b2 = _quiet(_mp().griffin_lim_batch, utts, phase_init=inits, niters=2)
    assert all(np.all(a[:, 0] == 0) and np.all(a[:, -1] == 0) for a in inits)
    assert len(b2) == len(utts)


def test_zero_magnitudes_give_exact_zeros():
    m, sh = _utt(16000, 0.2, 4)
    z = np.zeros_like(m)
    for init in ("random", "min_phase", "linear"):
        v, ph = _quiet(_mp().griffin_lim, z, sh, phase_init=init, niters=3)
        assert np.all(v == 0.0) and not np.any(np.isnan(ph)) and np.all(ph == 0.0)


@pytest.mark.parametrize("fs,fft_len", [(48000, 4096), (16000, 2048), (16000, 1024)])
def test_fft_lengths(fs, fft_len):
    m, sh = _utt(fs, 0.25, 6, fft_len=fft_len)
    assert m.shape[1] == fft_len // 2 + 1
    np.random.seed(SEED)
    ref, ref_ph = glm.griffin_lim(m, sh, "random", 3)
    np.random.seed(SEED)
    v, ph = _quiet(_mp().griffin_lim, m, sh, phase_init="random", niters=3)
    within(np.max(np.abs(v - ref)) / np.max(np.abs(ref)), GL_ITER_TOL[3], "GL_ITER_TOL:3")
