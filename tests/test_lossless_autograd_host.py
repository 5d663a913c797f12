"""CPU: the math of the lossless synthesis' backward pass (tests/lossless_autograd_model.py) and the host tables its
kernels read (hostmath.lerp_adjoint_table, hostmath.lossless_backward_table).  No GPU, no library."""
import numpy as np
import pytest

import lossless_autograd_model as model
from magphase_amd import hostmath as hm


def _case(seed, N, f0, fs=16000):
    """Features of one utterance with planted zeros of p = real + j imag and of mag, and an upstream gradient."""
    rng = np.random.RandomState(seed)
    F, H = len(f0), N // 2 + 1
    mag = np.exp(rng.randn(F, H))
    ang = rng.uniform(-np.pi, np.pi, (F, H))
    rad = rng.uniform(0.25, 4.0, (F, H))
    real, imag = rad * np.cos(ang), rad * np.sin(ang)
    for _ in range(10):
        real[rng.randint(F), rng.randint(H)] = 0.0          # only one part zero: |p| > 0
        i, k = rng.randint(F), rng.randint(H)
        real[i, k] = imag[i, k] = 0.0                        # p == 0: the divisor is the constant 1
        mag[rng.randint(F), rng.randint(H)] = 0.0
    real[0, 0] = imag[0, 0] = 0.0                            # ... at the two bins whose imaginary part is dropped, too
    real[F - 1, H - 1] = imag[F - 1, H - 1] = 0.0
    v_pm = model.v_pm_of(f0, fs)
    gy = rng.randn(hm.ola_plan(v_pm, N)[2])
    return mag, real, imag, gy, v_pm


@pytest.mark.parametrize("f0", [[0, 120, 130, 0, 0, 400, 55], [30, 0, 200, 210], [0, 0], [100]])
def test_closed_form_equals_float64_autograd(f0):
    """Mixed voicing; 30 Hz first: the first pitch mark lies beyond fft_len/2 (ola_plan's negative-start case)."""
    N = 1024
    mag, real, imag, gy, v_pm = _case(len(f0), N, f0)
    ref = model.grads_autograd(mag, real, imag, gy, v_pm, N)
    got = model.grads_closed(mag, real, imag, gy, v_pm, N)
    reached = f0[0] != 30       # with the 30 Hz start no frame reaches the kept output: all gradients are zero
    for g, r in zip(got, ref):
        assert np.all(np.isfinite(r)) and np.all(np.isfinite(g))
        assert (np.max(np.abs(r)) > 0) == reached
        assert model.rel_err(g, r) <= 1e-12
    zero_p = (real == 0) & (imag == 0)
    assert zero_p.sum() >= 2 and np.all(got[0][zero_p] == 0)      # d mag = 0 where p == 0


def test_backward_table_is_the_transpose_of_ola_plan():
    """lossless_backward_table against the forward's index arithmetic, utterance by utterance: the samples it reads are
    exactly those the overlap-add took from the frame, at the positions it put them."""
    N, fs = 1024, 16000
    f0s = [[0, 0], [30, 0, 200, 210, 0], [0, 120, 130, 0, 0, 400, 55], [100]]
    v_pms = [model.v_pm_of(f, fs) for f in f0s]
    plans = [hm.ola_plan(v, N) for v in v_pms]
    frame_off = np.concatenate(([0], np.cumsum([len(f) for f in f0s])))
    out_off = np.concatenate(([0], np.cumsum([p[2] for p in plans])))
    pos, lo, hi = hm.lossless_backward_table(np.concatenate([p[0] for p in plans]), frame_off, [p[1] for p in plans],
                                             [p[2] for p in plans], out_off, N)
    assert pos.dtype == np.int64 and lo.dtype == np.int32 and hi.dtype == np.int32
    assert any(N // 2 - int(v[0]) < 0 for v in v_pms)             # ola_plan's negative-start case is among them
    empty = 0
    for u, (rel, start, out_len) in enumerate(plans):
        for i in range(rel.size):
            f = frame_off[u] + i
            t0 = int(rel[i]) - start
            want = [n for n in range(N) if 0 <= t0 + n < out_len]
            assert pos[f] == out_off[u] + t0
            assert list(range(lo[f], hi[f])) == want
            if want:
                assert out_off[u] <= pos[f] + lo[f] and pos[f] + hi[f] <= out_off[u + 1]
            empty += not want
    assert empty > 0                                               # ... and with it frames that reach no output sample


def _check_adjoint(row0, row1, rowt, n_rows, seed=0):
    table = hm.lerp_adjoint_table(row0, row1, rowt, n_rows)
    assert table.dtype == np.int32 and table.shape == (n_rows, 4)
    gv = np.random.RandomState(seed).randn(len(row0), 5)
    want = model.lerp_matrix(row0, row1, rowt, n_rows).T @ gv
    got = model.lerp_adjoint_by_table(table, rowt, gv)
    assert np.max(np.abs(got - want)) <= 1e-12 * max(1.0, np.max(np.abs(want)))
    return table, got


def test_lerp_adjoint_table_random_monotone_tables():
    rng = np.random.RandomState(4)
    for trial in range(20):
        n_rows, F = rng.randint(2, 30), rng.randint(1, 80)
        row0 = np.sort(rng.randint(0, n_rows - 1, F))
        row1 = np.minimum(row0 + rng.randint(0, 2, F), n_rows - 1)     # row0 or row0 + 1: non-decreasing or not
        row1 = np.maximum.accumulate(row1)
        rowt = rng.uniform(-0.2, 1.2, F)                               # the clipped ends extrapolate
        _check_adjoint(row0, row1, rowt, n_rows, seed=trial)


def test_lerp_adjoint_table_one_row_grid_and_untouched_rows():
    # a one-row grid: every frame takes the row itself (row0 == row1, t = 0): its gradient is the plain sum
    table, got = _check_adjoint(np.zeros(6, int), np.zeros(6, int), np.zeros(6), 1)
    assert table.tolist() == [[0, 6, 0, 6]]
    assert np.allclose(got[0], np.random.RandomState(0).randn(6, 5).sum(axis=0), rtol=0, atol=1e-12)
    # rows no frame touches (0, 3 and 6) and an utterance boundary between rows 2 and 4
    row0, row1 = np.array([1, 1, 1, 4, 4, 5]), np.array([2, 2, 2, 5, 5, 5])
    table, got = _check_adjoint(row0, row1, np.array([0.0, 0.25, 1.0, 0.5, 0.75, 0.0]), 7)
    for r in (0, 3, 6):
        assert table[r, 0] == table[r, 1] and table[r, 2] == table[r, 3] and not got[r].any()
    # no frames at all
    assert hm.lerp_adjoint_table([], [], [], 3).tolist() == [[0, 0, 0, 0]] * 3


def test_lerp_adjoint_table_refuses_what_the_kernel_cannot_take():
    with pytest.raises(ValueError):
        hm.lerp_adjoint_table([1, 0], [1, 1], [0.0, 0.0], 2)          # decreasing
    with pytest.raises(ValueError):
        hm.lerp_adjoint_table([0, 2], [1, 2], [0.0, 0.0], 2)          # outside the rows
    with pytest.raises(ValueError):
        hm.lerp_adjoint_table([0, 1], [1, 1], [0.0], 2)               # lengths
