"""
No GPU: what the round-trip kernel's direct arm rests on (csrc/magphase_comp.hip, k_roundtrip_pair's DIRECT).

The synthesis half of the one-launch round trip is given the spectrum its analysis half has just computed, so the frame it
rebuilds is fftshift(IFFT(hermitian(FFT(y)))) of the windowed, rotated, zero-padded (or truncated) frame y: fftshift(y).  In
float64, the oracle's copy synthesis against the plain overlap-add of fftshift(y), on the edge batch of the round-trip tests
and on a train of periods 300 / 700 / 1100: 1e-12 of the peak (measured: 5.6e-16).  Then the row map of the arm -- row q of
the shifted frame is gathered row (q + P/2) mod P, and a class-4 frame's rows are what hostmath.roundtrip_frame_extents says
the launch adds -- and the switch: the flag bit at the two C entries that take the flags word, the environment variable at
plan build.
"""
import numpy as np
import pytest

import _rt_direct as rtd
import _seams
from magphase_amd import hostmath as hm

N, P = 4096, 32
IDENTITY_TOL = 1e-12     # of the peak, float64; measured 5.6e-16
MPX_RT_INVERSE_TRANSFORM = 32


@pytest.fixture(scope="module")
def orc():
    from oracle import magphase_oracle as o
    return o


@pytest.fixture(scope="module")
def lib():
    from magphase_amd import _lib
    return _lib.load()


def _identity_error(orc, utt):
    pcm, fs, pm, voi = utt
    x = np.asarray(pcm, dtype=np.float64) / 32768.0
    ref = rtd.quiet(rtd.oracle_copy_synthesis, orc, x, fs, pm, voi)
    got = rtd.quiet(rtd.direct_copy_synthesis, orc, x, fs, pm, voi)
    assert got.shape == ref.shape
    peak = float(np.max(np.abs(ref), initial=0.0))
    if peak == 0.0:
        assert not np.any(got)
        return 0.0
    return float(np.max(np.abs(got - ref))) / peak


def test_copy_synthesis_is_the_overlap_add_of_the_shifted_windowed_frames(orc):
    utts = rtd.edge_batch() + [rtd.period_train()]
    kinds = set()
    for pcm, fs, pm, voi in utts:
        _, left, right, _ = orc.frame_bounds(orc.clean_epochs(pm, voi, len(pcm), fs)[0] * fs, len(pcm))
        kinds |= rtd.frame_kinds(left, right)
    assert kinds == {"class-4", "full-class", "second-tile", "truncated", "L=0"}
    _, left, right, _ = orc.frame_bounds(rtd.period_train()[2] * rtd.FS, len(rtd.period_train()[0]))
    assert 0.3 < np.mean(hm.roundtrip_support_classes(left, right, N) != 4) < 0.8     # about half outside class 4
    errs = [_identity_error(orc, u) for u in utts]
    print("copy synthesis against ola(fftshift(windowed rotated frames)), of the peak: " + " ".join("%.2g" % e for e in errs))
    assert max(errs) <= IDENTITY_TOL


def test_identity_at_the_other_transform_lengths(orc):
    from magphase_amd import synthetic as syn
    for fs in (16000, 8000):
        pcm, pm, voi = syn.make_utterance(41, dur_s=0.5, fs=fs)
        assert _identity_error(orc, (pcm, fs, pm, voi)) <= IDENTITY_TOL


def test_row_map_and_class_rows_against_the_extents(orc):
    """Row q of the shifted frame is row (q + P/2) mod P = q ^ (P/2) of the gathered frame (what ring_add_plane's natural,
    rotated form reads); a class-4 frame is zero outside the gathered rows j < 4 and j >= 28, whose images are the rows
    12 ... 19 -- the samples hostmath.roundtrip_frame_extents says such a frame adds."""
    q = np.arange(P)
    assert np.array_equal((q + P // 2) % P, q ^ (P // 2))
    pcm, fs, pm, voi = rtd.period_train()
    x = np.asarray(pcm, dtype=np.float64) / 32768.0 + 1.0      # no sample of a frame is zero but its window's ends
    y, v_shift, _ = rtd.windowed_rotated_frames(orc, x, fs, pm, voi)
    _, left, right, _ = orc.frame_bounds(orc.clean_epochs(pm, voi, len(x), fs)[0] * fs, len(x))
    ext = hm.roundtrip_frame_extents(left, right, N)
    cls = hm.roundtrip_support_classes(left, right, N)
    assert (cls == 4).any() and (cls != 4).any()
    shifted = np.fft.fftshift(y, axes=1).reshape(-1, P, 128)
    assert np.array_equal(shifted, y.reshape(-1, P, 128)[:, q ^ (P // 2), :])
    for f in range(y.shape[0]):
        rows_in = np.flatnonzero(np.any(y[f].reshape(P, 128) != 0.0, axis=1))
        rows_out = np.flatnonzero(np.any(shifted[f] != 0.0, axis=1))
        assert np.array_equal(np.sort(rows_in ^ (P // 2)), rows_out)
        assert 128 * rows_out.min() >= ext[f, 0] and 128 * rows_out.max() + 128 <= ext[f, 1]
        if cls[f] == 4:
            assert tuple(ext[f]) == _seams.NARROW
            assert set(rows_in) <= set(range(4)) | set(range(28, 32)) and set(rows_out) <= set(range(12, 20))
    narrow_in = [j for j in range(P) if 12 <= (j ^ (P // 2)) < 20]
    assert narrow_in == [0, 1, 2, 3, 28, 29, 30, 31]


def _empty_launch(lib, n_fft, flags):
    return lib.mpx_roundtrip_lossless_ola_flags(*([None, n_fft] + [None] * 5 + [0, None, 0, None, None, 0] + [None] * 6
                                                  + [n_fft // 2 + 1, flags]))


def test_the_flag_at_the_c_entries(lib):
    left = np.asarray([300, 600, 0], dtype=np.int32)
    right = np.asarray([200, 100, 511], dtype=np.int32)
    for n_fft in (4096, 2048, 1024):
        for base in (0, 1, 4, 8):
            ref = np.zeros((3, 2), dtype=np.int32)
            ext = np.full((3, 2), -1, dtype=np.int32)
            assert lib.mpx_roundtrip_frame_extents(n_fft, left.ctypes.data, right.ctypes.data, 3, base, ref.ctypes.data) == 0
            assert lib.mpx_roundtrip_frame_extents(n_fft, left.ctypes.data, right.ctypes.data, 3,
                                                   base | MPX_RT_INVERSE_TRANSFORM, ext.ctypes.data) == 0
            assert np.array_equal(ext, ref)                     # accepted and ignored
            assert _empty_launch(lib, n_fft, base | MPX_RT_INVERSE_TRANSFORM) == 0
    for bad in (2, 16, 64, 1 << 31, MPX_RT_INVERSE_TRANSFORM | 64, MPX_RT_INVERSE_TRANSFORM | 4 | 8):
        assert _empty_launch(lib, N, bad) != 0
    assert lib.mpx_roundtrip_frame_extents(N, None, None, 0, 64, None) != 0


def test_the_environment_variable_at_plan_build(monkeypatch):
    from magphase_amd import _lib
    from magphase_amd.plans import LosslessRoundTripPlan
    eng = _seams.HostEngine(6)
    assert _lib.RT_INVERSE_FLAGS == {"direct": 0, "transform": MPX_RT_INVERSE_TRANSFORM}
    monkeypatch.delenv("MAGPHASE_RT_INVERSE", raising=False)
    assert LosslessRoundTripPlan(eng, []).inverse == "direct"
    for name in ("direct", "transform"):
        monkeypatch.setenv("MAGPHASE_RT_INVERSE", name)
        assert LosslessRoundTripPlan(eng, []).inverse == name
    for bad in ("bogus", "Direct", "0"):
        monkeypatch.setenv("MAGPHASE_RT_INVERSE", bad)
        with pytest.raises(ValueError):
            LosslessRoundTripPlan(eng, [])
