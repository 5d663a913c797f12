"""CPU: the model of the device fold of Griffin-Lim (tests/griffin_lim_device_model.py) against numpy's own draws and
hostmath.griffin_lim_fold, the argument checks of mpx_griffin_lim_fold (no device needed), the ValueErrors of
griffin_lim_batch's device path and of griffin_lim_from_mag_batch (raised before any device call), and header / binding /
INTEGRATION.md agreement."""
import os
import re

import numpy as np
import pytest

import griffin_lim_device_model as gdm
from magphase_amd import _lib
from magphase_amd import hostmath as hm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("seed,F,N", [(0, 3, 1024), (1313, 5, 2048), (7, 2, 4096)])
def test_words_are_numpys_rand(seed, F, N):
    np.random.seed(seed)
    words = np.random.randint(0, 2**32, size=2 * F * N, dtype=np.uint32)
    after_words = np.random.get_state()[2]
    np.random.seed(seed)
    r = np.random.rand(F, N)
    assert np.random.get_state()[2] == after_words     # the same stretch of the stream
    assert np.array_equal(gdm.words_to_rand(words).reshape(F, N), r)
    assert np.array_equal(gdm.words_to_phase(words, F, N), 2 * np.pi * (r - 0.5))


@pytest.mark.parametrize("N", [1024, 2048, 4096])
def test_model_fold_is_hostmaths(N):
    rs = np.random.RandomState(N)
    F, H = 7, N // 2 + 1
    m = rs.rand(F, H).astype(np.float32)
    m[2] = 0.0
    full = (2 * np.pi * (rs.rand(F, N) - 0.5)).astype(np.float32)
    half = (80 * (rs.rand(F, H) - 0.5)).astype(np.float32)      # |phi| up to 40 rad, junk in the end columns
    for form, ph, is_full in ((gdm.FULL, full, True), (gdm.HALF, half, False)):
        want = hm.griffin_lim_fold(m, ph.astype(np.float64), is_full)
        got = gdm.fold(m, ph, form)
        for w, g in zip(want, got[:3]):
            assert np.max(np.abs(w - g)) <= 1e-15
    assert np.array_equal(gdm.fold(m, half, gdm.HALF)[3][:, [0, -1]], np.zeros((F, 2)))
    words = rs.randint(0, 2**32, size=2 * F * N, dtype=np.uint32)
    want = hm.griffin_lim_fold(m, gdm.words_to_phase(words, F, N), True)
    for w, g in zip(want, gdm.fold(m, words, gdm.WORDS)[:3]):
        assert np.max(np.abs(w - g)) <= 1e-15


@pytest.mark.parametrize("N", [1024, 2048, 4096])
def test_linear_folds_to_the_magnitude_and_one(N):
    F, H = 3, N // 2 + 1
    m = np.random.RandomState(3).rand(F, H)
    ph, full = hm.griffin_lim_initial_phase("linear", m)
    assert full and set(np.unique(ph)) <= {0.0, np.pi}
    for fold in (hm.griffin_lim_fold(m, ph, True), gdm.fold(m, ph, gdm.FULL)[:3]):
        assert np.array_equal(fold[0], m) and np.all(fold[1] == 1.0) and np.all(fold[2] == 0.0)


# ------------------------------------------------------------------------------------------------ the C entry
def _fold(lib, fft_len=2048, form=0, mag=1, phase=1, ld_phase=None, frame0=0, n=4, outs=(1, 1, 1), ld=None):
    H = fft_len // 2 + 1
    p = lambda x: 4096 if x else None   # noqa: E731  (never dereferenced: every case returns before a launch)
    return lib.mpx_griffin_lim_fold(None, fft_len, form, p(mag), p(phase), fft_len if ld_phase is None else ld_phase, frame0, n,
                                    p(outs[0]), p(outs[1]), p(outs[2]), None, lib.mpx_spec_ld(H) if ld is None else ld)


def test_argument_errors_without_gpu():
    lib = _lib.load()
    err = lambda: lib.mpx_last_error()   # noqa: E731
    for kw in (dict(mag=0), dict(phase=0), dict(outs=(0, 1, 1)), dict(outs=(1, 0, 1)), dict(outs=(1, 1, 0))):
        assert _fold(lib, **kw) == -1 and b"null" in err()
    assert _fold(lib, form=3) == -1 and b"form" in err()
    assert _fold(lib, form=-1) == -1 and b"form" in err()
    assert _fold(lib, fft_len=1000) == -1 and b"fft_len" in err()
    assert _fold(lib, fft_len=512) == -1 and b"fft_len" in err()
    for kw in (dict(n=-1), dict(frame0=-2), dict(ld=-5), dict(ld_phase=-1)):
        assert _fold(lib, **kw) == -1 and b"negative" in err()
    assert _fold(lib, ld=1024) == -1 and b"ld smaller than H" in err()
    assert _fold(lib, form=0, ld_phase=1024) == -1 and b"ld_phase" in err()
    assert _fold(lib, form=1, ld_phase=2047) == -1 and b"ld_phase" in err()
    # zero rows: MPX_OK without a launch, whatever the pointers
    assert _fold(lib, n=0, mag=0, phase=0, outs=(0, 0, 0)) == 0
    for form in (0, 1, 2):
        assert _fold(lib, form=form, n=0) == 0


def test_header_binding_and_integration_agree():
    hdr = open(os.path.join(ROOT, "include", "magphase_hip.h")).read()
    assert re.search(r"\bint mpx_griffin_lim_fold\(void\* stream, int fft_len, int32_t form,", hdr)
    for name, val in (("HALF", 0), ("FULL", 1), ("WORDS", 2)):
        assert re.search(r"#define MPX_GL_FOLD_%s %d\b" % (name, val), hdr)
    restype, argtypes = _lib.PROTOTYPES["mpx_griffin_lim_fold"]
    decl = hdr[hdr.index("int mpx_griffin_lim_fold("):]
    decl = decl[:decl.index(";")]
    assert len(argtypes) == decl.count(",") + 1 == 13
    names = list(_lib.PROTOTYPES)
    assert names.index("mpx_griffin_lim_fold") == names.index("mpx_griffin_lim_ola") + 1   # the header's order
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "| `mpx_griffin_lim_fold` |" in doc and "griffin_lim_from_mag_batch" in doc
    from magphase_amd.engine import Engine
    assert Engine.GL_FOLD_FORMS == {"half": gdm.HALF, "full": gdm.FULL, "words": gdm.WORDS}
    assert 1 << 26 <= Engine.GL_WORDS_GROUP_SAMPLES <= 1 << 27
    from magphase_amd import build
    assert "magphase_gl.hip" in build.UNITS


# ------------------------------------------------------------------------------------------------ the Python checks
class _NoDevice:
    """An engine that has a device name and nothing else: any use of it is a device call, which these checks precede."""

    def __init__(self, device):
        self.__dict__["device"] = device

    def __getattr__(self, name):
        raise AssertionError("device call before the argument checks were done: engine.%s" % name)


def _gl_args(F=4, N=1024):
    H = N // 2 + 1
    return np.random.RandomState(1).rand(F, H), np.full(F, 100.0)


def test_griffin_lim_batch_value_errors_precede_device_calls():
    import torch

    from magphase_amd import magphase as mp

    eng = _NoDevice(torch.device("cuda", 0))
    m, sh = _gl_args()
    elsewhere = torch.zeros(m.shape, device="meta")
    np.random.seed(5)
    state = np.random.get_state()
    cases = [
        (dict(fold="gpu"), "fold"),
        (dict(fold="host", utts=[(elsewhere, sh)]), "fold='host' with a device tensor"),
        (dict(fold="host", phase_init=[elsewhere]), "fold='host' with a device tensor"),
        (dict(utts=[(elsewhere, sh)]), "is on meta"),
        (dict(fold="device", phase_init=[elsewhere]), "is on meta"),
        (dict(utts=[(torch.zeros(m.shape, dtype=torch.int32), sh)]), "dtype"),
        (dict(utts=[(torch.zeros(m.shape, dtype=torch.bool), sh)]), "dtype"),
        (dict(utts=[(torch.zeros(m.shape, dtype=torch.complex64), sh)]), "dtype"),
        (dict(fold="device", phase_init=[torch.zeros(m.shape, dtype=torch.int64)]), "dtype"),
        (dict(utts=[(torch.zeros((2,) + m.shape), sh)]), "2-D"),
        (dict(fold="device", phase_init=[torch.zeros((m.shape[0], 7), device="meta")]), "shape"),
        (dict(fold="device", phase_init="warm"), "unknown phase_init"),
        (dict(fold="device", niters=0), "niters"),
        (dict(fold="device", utts=[(m, np.full(m.shape[0], 600.0))]), "domain"),
        (dict(fold="device", utts=[(m, sh), (np.ones((2, 1025)), np.full(2, 100.0))]), "fft_len"),
        (dict(fold="device", utts=[(elsewhere, sh[:-1])]), "len(v_shift)"),
    ]
    for kw, what in cases:
        kw = dict(dict(utts=[(m, sh)], phase_init="random", niters=2, engine=eng), **kw)
        with pytest.raises(ValueError) as ei:
            mp.griffin_lim_batch(kw.pop("utts"), **kw)
        assert what in str(ei.value), (what, str(ei.value))
    st = np.random.get_state()
    assert st[2] == state[2] and np.array_equal(st[1], state[1])    # nothing was drawn


def test_griffin_lim_from_mag_value_errors_precede_device_calls():
    import torch

    from magphase_amd import magphase as mp

    eng = _NoDevice(torch.device("cuda", 0))
    rs = np.random.RandomState(2)
    mml = rs.randn(12, 60) * 0.1
    lf0 = np.log(np.full(12, 120.0))
    low = lf0.copy()
    low[5] = np.log(10.0)    # a 1600-sample shift at 16 kHz: beyond fft_len / 2 - 1 = 1023
    np.random.seed(6)
    state = np.random.get_state()
    cases = [
        (dict(phase_init="zero"), "unknown phase_init"),
        (dict(phase_init=np.zeros((12, 1025))), "unknown phase_init"),
        (dict(niters=0), "niters"),
        (dict(fft_len=512), "fft_len 512"),
        (dict(fs=12345), "Sample rate"),
        (dict(utts=[(mml, lf0), (mml, low)]), "utts[1]"),
        (dict(utts=[(mml, lf0), (mml, low)], b_const_rate=True), "utts[1]"),
        (dict(utts=[(mml, lf0), (mml[:, :40], lf0)]), "utts[1]"),
        (dict(utts=[(mml, lf0[:-1])]), "utts[0]"),
        (dict(utts=[(mml, lf0, lf0)]), "(m_mag_mel_log, v_lf0)"),
        (dict(utts=[(torch.zeros((12, 60), dtype=torch.int32), lf0)]), "dtype"),
        (dict(utts=[(torch.zeros((12, 60), device="meta"), lf0)]), "is on meta"),
    ]
    for kw, what in cases:
        kw = dict(dict(utts=[(mml, lf0)], fs=16000, engine=eng), **kw)
        with pytest.raises(ValueError) as ei:
            mp.griffin_lim_from_mag_batch(kw.pop("utts"), kw.pop("fs"), **kw)
        assert what in str(ei.value), (what, str(ei.value))
    st = np.random.get_state()
    assert st[2] == state[2] and np.array_equal(st[1], state[1])
    assert "autograd" in mp.griffin_lim_from_mag_batch.__doc__
    assert mp.griffin_lim_from_mag_batch([], 16000, engine=eng) == []
