"""CPU: the closed form of the lossless analysis' backward pass (what k_analysis_lossless_bwd / k_analysis_bwd_gather
implement) against torch float64 autograd through the forward, and the host tables of the gather
(hostmath.analysis_backward_table) against a brute-force scatter.  Needs neither a GPU nor the library."""
import numpy as np
import pytest

import lossless_analysis_autograd_model as model
from magphase_amd import hostmath as hm

FS = model.FS
TOL = 1.0e-12      # of the largest gradient: float64 round-off of two different orders of the same sums


def _case(kind, rng):
    """(sig, pm, left, right) of one utterance."""
    if kind in ("f0_55", "f0_400", "unvoiced"):
        spacing = {"f0_55": FS / 55.0, "f0_400": FS / 400.0, "unvoiced": 0.005 * FS}[kind]
        pm_sec, voi, n = model.epochs(9, spacing, kind != "unvoiced")
        sig = model.tone_and_noise(rng, n)
    elif kind == "long":            # 12 Hz spacing: every frame is longer than fft_len = 1024
        pm_sec, voi, n = model.epochs(4, FS / 12.0, True)
        sig = model.tone_and_noise(rng, n)
    elif kind == "silence":         # three consecutive frames of exact silence
        pm_sec, voi, n = model.epochs(12, FS / 100.0, True)
        sig = model.tone_and_noise(rng, n)
        pm = np.round(pm_sec * FS).astype(int)
        sig[pm[3]:pm[7] + 1] = 0.0          # frames 4, 5, 6 span pm[3] .. pm[7]
    elif kind == "equal_epochs":    # two epochs that round to the same sample: R == 0, then L == 0
        pm_sec, voi, n = model.epochs(8, FS / 100.0, True)
        pm_sec = np.sort(np.r_[pm_sec, pm_sec[4] + 0.3 / FS])
        voi = np.ones(pm_sec.size)
        sig = model.tone_and_noise(rng, n)
    else:
        raise KeyError(kind)
    pm, left, right, _voi = model.frames_of(pm_sec, voi, n)
    return sig, pm, left, right


def _check(sig, pm, left, right, N, rng, which=(True, True, True)):
    mag, real, imag = model.forward_numpy(sig, pm, left, right, N)
    assert np.all(np.isfinite(mag)) and np.all(np.isfinite(real)) and np.all(np.isfinite(imag))
    grads = tuple(rng.randn(*mag.shape) if w else None for w in which)
    want = model.grads_autograd(sig, grads, pm, left, right, N)
    got = model.grads_closed(mag, real, imag, grads, pm, left, right, sig.size, N)
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(want)) and np.any(want != 0)
    assert model.rel_err(got, want) <= TOL, model.rel_err(got, want)
    return mag, got


@pytest.mark.parametrize("N", [1024, 2048, 4096])
@pytest.mark.parametrize("kind", ["f0_55", "f0_400", "unvoiced", "silence", "equal_epochs"])
def test_closed_form_equals_autograd(kind, N):
    rng = np.random.RandomState(N + len(kind))
    sig, pm, left, right = _case(kind, rng)
    mag, _g = _check(sig, pm, left, right, N, rng)
    if kind == "silence":
        assert np.sum(~mag.any(axis=1)) == 3          # all-zero rows, and no NaN anywhere (checked above)
    if kind == "equal_epochs":
        assert np.sum(left == 0) == 1 and np.sum(right == 0) == 1


def test_frames_longer_than_fft_len():
    rng = np.random.RandomState(5)
    sig, pm, left, right = _case("long", rng)
    assert np.all(left + right + 1 > 1024) and np.all(left >= 1024)
    _check(sig, pm, left, right, 1024, rng)
    # ... and a frame that is too long with its centre still inside the transform (rot = L < fft_len)
    pm_sec, voi, n = model.epochs(4, 700.0, True)
    pm, left, right, _voi = model.frames_of(pm_sec, voi, n)
    assert np.all(left + right + 1 > 1024) and np.all(left < 1024)
    _check(model.tone_and_noise(rng, n), pm, left, right, 1024, rng)


@pytest.mark.parametrize("which", [(True, False, False), (False, True, False), (False, False, True)])
def test_one_output_at_a_time(which):
    rng = np.random.RandomState(17)
    sig, pm, left, right = _case("f0_400", rng)
    _check(sig, pm, left, right, 1024, rng, which)


def test_backward_table_against_a_scatter():
    rng = np.random.RandomState(3)
    N = 1024
    pos, left, right, total = [], [], [], 0
    for kind in ("f0_400", "long", "equal_epochs", "unvoiced"):
        sig, pm, l, r = _case(kind, rng)
        pos.append(pm + total), left.append(l), right.append(r)
        total += sig.size + 7          # utterances follow one another; a few samples no frame covers in between
    pos, left, right = (np.concatenate(x) for x in (pos, left, right))
    start, off = hm.analysis_backward_table(pos, left, right, N, total)
    n = np.minimum(left + right + 1, N)
    assert start.dtype == np.int64 and off.dtype == np.int64 and off[0] == 0
    assert np.array_equal(start, pos - left) and np.array_equal(np.diff(off), n) and n.max() == N
    per_frame = rng.randn(int(off[-1]))
    want = np.zeros(total)
    for f in range(pos.size):
        np.add.at(want, start[f] + np.arange(n[f]), per_frame[off[f]:off[f + 1]])
    got = model.gather_by_table(per_frame, start, off, total)
    assert np.allclose(got, want, rtol=0, atol=1e-12) and np.any(want == 0) and np.any(want != 0)
    e_start, e_off = hm.analysis_backward_table([], [], [], N, 0)
    assert e_start.size == 0 and e_off.tolist() == [0]


def test_backward_table_refuses_malformed_tables():
    ok = ([10, 20, 30], [5, 10, 10], [10, 10, 5], 1024, 40)
    hm.analysis_backward_table(*ok)
    bad = [
        ([10, 20], [5, 10, 10], [10, 10, 5], 1024, 40),        # lengths differ
        ([10, 20, 30], [5, -1, 10], [10, 10, 5], 1024, 40),    # negative left
        ([10, 20, 30], [5, 10, 10], [10, -2, 5], 1024, 40),    # negative right
        ([3, 20, 30], [5, 10, 10], [10, 10, 5], 1024, 40),     # starts before the buffer
        ([10, 20, 30], [5, 10, 10], [10, 10, 50], 1024, 40),   # ends after it
        ([20, 10, 30], [5, 10, 10], [3, 3, 5], 1024, 40),      # starts decrease
        ([10, 12, 30], [5, 6, 10], [30, 3, 5], 1024, 45),      # ends decrease
        ([10, 20, 30], [5, 10, 10], [10, 10, 5], 0, 40),       # fft_len
        ([10, 20, 30], [5, 10, 10], [10, 10, 5], 1024, -1),    # total
    ]
    for args in bad:
        with pytest.raises(ValueError):
            hm.analysis_backward_table(*args)


def test_signal_tensor_check():
    import torch

    hm.check_signal_tensor(torch.zeros(4, dtype=torch.bfloat16)[::2], "x")
    for t in (torch.zeros(4, dtype=torch.int16), torch.zeros(2, 2), torch.zeros(3, dtype=torch.complex64)):
        with pytest.raises(ValueError):
            hm.check_signal_tensor(t, "utts[0]: v_sig")
