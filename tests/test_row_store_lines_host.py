"""
CPU: the line-aligned store shape of the round-trip kernel's feature rows (csrc/mpx_common.hpp, "Row stores by line").
mpx_roundtrip_store_map answers from the functions the kernel takes its per-lane bases and predicates from; here it is held
to its numpy twin and to what the shape promises, for every phase a row can have in its 128-byte line.
"""
import numpy as np
import pytest

from magphase_amd import _lib
from magphase_amd import hostmath as hm

N = 4096
M = N // 2          # bin M is the row's last float
HP = N // 256       # steps per frame: the lane holds bin lane + 64 q and its mirror at step q
STORES = 2 * HP + 2
PHASES = range(32)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def store_map(lib, phase, fft_len=N):
    out = np.full((STORES, 64), -7, dtype=np.int32)
    rc = lib.mpx_roundtrip_store_map(fft_len, phase, out.ctypes.data)
    return rc, out


def parent_shape():
    """The row-relative shape, written out from the kernel's description of it: ascending 256-byte blocks of the own bins in
    natural q order; the mirrors of step q regrouped into aligned blocks [M - 64 q - 64, M - 64 q - 1] whose lowest float is
    lane 0's mirror of step q + 1 (bin M/2 for the last block); bin M alone from lane 0.  In issue order, with the empty
    store the by-line shape has at phase 0 (the ascending tail)."""
    lane = np.arange(64)
    rows = []
    for q in range(HP):
        rows.append(lane + 64 * q)                                   # own bins of step q
        if q == 0:
            rows.append(np.where(lane == 0, M, -1))                  # bin M alone
        else:                                                        # block [M - 64 q, M - 64 q + 63]: mirrors of step q - 1 ...
            rows.append(np.where(lane == 0, M - 64 * q, M - 64 * (q - 1) - lane))   # ... lane 0: its mirror of step q
    rows.append(np.full(64, -1))
    rows.append(np.where(lane == 0, M // 2, M - 64 * (HP - 1) - lane))
    return np.stack(rows).astype(np.int32)


@pytest.mark.parametrize("phase", PHASES)
def test_map_equals_numpy_twin(lib, phase):
    rc, got = store_map(lib, phase)
    assert rc == 0
    assert np.array_equal(got, hm.roundtrip_store_map(N, phase))


@pytest.mark.parametrize("phase", PHASES)
def test_every_row_float_exactly_once(lib, phase):
    _, got = store_map(lib, phase)
    live = got[got >= 0]
    assert got.min() >= -1 and got.max() <= M
    assert live.size == M + 1
    assert np.array_equal(np.sort(live), np.arange(M + 1))


@pytest.mark.parametrize("phase", PHASES)
def test_interior_stores_are_two_whole_lines(lib, phase):
    _, got = store_map(lib, phase)
    edge = {0: "B_0", 1: "B_32", 2 * HP: "middle, ascending part", 2 * HP + 1: "middle, mirror part"}
    for st in range(STORES):
        if st in edge:
            continue
        row = np.sort(got[st])
        assert row[0] >= 0, (phase, st)                                       # no lane masked
        assert np.array_equal(row, row[0] + np.arange(64)), (phase, st)       # 64 consecutive floats ...
        assert (row[0] + phase) % 32 == 0, (phase, st)                        # ... from a line boundary of memory
    # the four others: B_0 and B_32 clipped to the row, the middle block's two parts together one whole block
    assert np.array_equal(np.sort(got[0][got[0] >= 0]), np.arange(0, 64 - phase))
    assert np.array_equal(np.sort(got[1][got[1] >= 0]), np.arange(M - phase, M + 1))
    mid = np.sort(np.concatenate([got[2 * HP][got[2 * HP] >= 0], got[2 * HP + 1][got[2 * HP + 1] >= 0]]))
    assert np.array_equal(mid, M // 2 - phase + np.arange(64))


def test_phase_0_is_the_row_relative_shape(lib):
    _, got = store_map(lib, 0)
    assert np.array_equal(got, parent_shape())
    assert np.array_equal(hm.roundtrip_store_map(N, 0), parent_shape())


def test_store_order_is_ascending_then_mirror_per_step(lib):
    """Issue order: block B_q (ascending) and block B_{32 - q} (mirrors) at step q."""
    for phase in (0, 1, 17, 31):
        _, got = store_map(lib, phase)
        for q in range(1, HP):
            assert got[2 * q].min() == 64 * q - phase
            assert got[2 * q + 1].min() == M - 64 * q - phase


@pytest.mark.parametrize("fft_len", [2048, 1024, 1000])
def test_other_transform_lengths_are_rejected(lib, fft_len):
    rc, out = store_map(lib, 0, fft_len=fft_len)
    assert rc != 0 and b"4096" in lib.mpx_last_error()
    assert np.all(out == -7)
    with pytest.raises(ValueError):
        hm.roundtrip_store_map(fft_len, 0)


def test_bad_arguments_are_rejected(lib):
    out = np.zeros((STORES, 64), dtype=np.int32)
    assert lib.mpx_roundtrip_store_map(N, -1, out.ctypes.data) != 0
    assert lib.mpx_roundtrip_store_map(N, 32, out.ctypes.data) != 0
    assert lib.mpx_roundtrip_store_map(N, 0, None) != 0
    for bad in (-1, 32):
        with pytest.raises(ValueError):
            hm.roundtrip_store_map(N, bad)


def test_flags_of_the_launch_and_of_the_extents(lib):
    """The store bits are known to both entries that take the flags word (an empty launch: no device needed); both bits
    together and any other bit are refused."""
    left = np.asarray([300, 600], dtype=np.int32)
    right = np.asarray([200, 100], dtype=np.int32)
    ref = np.zeros((2, 2), dtype=np.int32)
    assert lib.mpx_roundtrip_frame_extents(N, left.ctypes.data, right.ctypes.data, 2, 0, ref.ctypes.data) == 0
    for flags in (4, 8):
        ext = np.zeros((2, 2), dtype=np.int32)
        assert lib.mpx_roundtrip_frame_extents(N, left.ctypes.data, right.ctypes.data, 2, flags, ext.ctypes.data) == 0
        assert np.array_equal(ext, ref)
        assert lib.mpx_roundtrip_lossless_ola_flags(*([None, N] + [None] * 5 + [0, None, 0, None, None, 0] + [None] * 6
                                                      + [M + 1, flags])) == 0
    for flags in (4 | 8, 2, 16):
        assert lib.mpx_roundtrip_lossless_ola_flags(*([None, N] + [None] * 5 + [0, None, 0, None, None, 0] + [None] * 6
                                                      + [M + 1, flags])) != 0
