"""
Shared by the tests of the round-trip kernel's direct arm (MAGPHASE_RT_INVERSE=direct, csrc/magphase_comp.hip: the windowed
frame is overlap-added as gathered, without the Hermitian merge and the inverse transform of its own spectrum): the float64
model of that arm on the oracle's own functions, and the test batches.
"""
import warnings

import numpy as np

import _seams

FS = 48000


def windowed_rotated_frames(orc, x, fs, v_pm_sec, v_voi, fft_len=None):
    """What the kernel's gather holds per frame, in float64: the oracle's windowed frames (Hann halves around the epoch),
    zero-padded or truncated to fft_len and rotated left by the frame's left length (oracle.analysis_frames up to its FFT,
    with its slicing rule: a left length >= fft_len rotates nothing).  Returns (y [F x N], v_shift, v_voi of the cleaned
    epochs)."""
    pm, voi = orc.clean_epochs(v_pm_sec, v_voi, check_len_smpls=len(x), fs=fs)
    N = fft_len or orc.define_fft_len(fs)
    frames, lens, _, v_shift, _ = orc.windowing(x, pm * fs)
    y = np.zeros((len(frames), N))
    for f, fr in enumerate(frames):
        row = np.zeros(N)
        n = min(int(lens[f]), N)
        row[:n] = fr[:n]
        s = int(v_shift[f])
        y[f] = np.concatenate((row[s:], row[:s]))
    return y, v_shift, voi


def direct_copy_synthesis(orc, x, fs, v_pm_sec, v_voi):
    """Copy synthesis without a transform: ola(fftshift(y), v_pm) with the synthesis positions of the oracle's own f0."""
    y, v_shift, voi = windowed_rotated_frames(orc, x, fs, v_pm_sec, v_voi)
    v_f0 = orc.shift_to_f0(v_shift, voi, fs)
    v_pm = orc.shift_to_pm(orc.f0_to_shift(v_f0, fs))
    return orc.ola(np.fft.fftshift(y, axes=1), v_pm)


def oracle_copy_synthesis(orc, x, fs, v_pm_sec, v_voi):
    o = orc.analysis_lossless_from_epochs(x, fs, v_pm_sec, v_voi)
    return orc.synthesis_from_lossless(o[0], o[1], o[2], o[3], fs)


def edge_batch():
    """The batch of tests/test_gpu_lossless.py::test_round_trip_launch_edge_frames: frames of 11 520 + 6 240 samples truncated
    at N, a first epoch at sample 0 (L = 0) with an unvoiced stretch, silence, an utterance of two frames."""
    fs = FS
    rng = np.random.RandomState(5)
    x = (rng.uniform(-0.5, 0.5, 30000) * 32767).astype(np.int16)
    pm_long = np.array([0.0, 0.01, 0.02, 0.15, 0.16, 0.4]) + 1e-4
    pm0 = np.array([0.0, 0.004, 0.009, 0.015, 0.02])
    return [(x, fs, pm_long, np.ones(pm_long.size)), (x[:2000], fs, pm0, np.array([1.0, 1, 0, 0, 1])),
            (np.zeros(4000, dtype=np.int16), fs, np.arange(1, 16) * 0.005, np.zeros(15)),
            (x[:1500], fs, np.array([0.005, 0.012]), np.ones(2))]


def period_train():
    """One utterance at 48 kHz with periods of 300, 700 and 1100 samples (class 4; L > 512: the full class; frames of 1401 and
    2201 samples: a second sample tile) and one gap of 4300 samples (the frames on either side are truncated at N)."""
    gaps = [300] * 6 + [700] * 5 + [1100] * 5 + [4300] + [300] * 4 + [1100] * 2 + [700] * 3 + [300] * 5
    return _seams.utt_from_gaps(np.asarray(gaps), 11, first=150)


def direct_batch():
    """Four utterances of 0.2 - 0.4 s at 48 kHz whose frames are of every kind the kernel's arms tell apart: periods around
    155 and 240 samples (class 4), around 800 (L > 512: the full class; frames of ~1 600 samples: a second sample tile), a
    pause of 4300 samples (the frames on either side are truncated at N), a first epoch at sample 0 (L = 0), a stretch of
    unvoiced epochs 300 samples apart (synthesised 240 apart: the synthesis positions leave the analysis positions), and an
    utterance of digital silence."""
    rng = np.random.RandomState(2024)

    def hi(n):
        return list(rng.randint(225, 256, n))

    def lo(n):
        return list(rng.randint(760, 840, n))

    def sh(n):
        return list(rng.randint(140, 171, n))

    a = _seams.utt_from_gaps(np.asarray(sh(3) + hi(10) + lo(3) + [4300] + hi(8) + lo(2) + hi(7)), 61, first=0)
    gb = hi(9) + [300] * 8 + lo(2) + hi(12)
    pcm, fs, pm, voi = _seams.utt_from_gaps(np.asarray(gb), 62, first=44)
    voi = voi.copy()
    voi[10:18] = 0.0                       # the epochs of the 300-sample stretch
    b = (pcm, fs, pm, voi)
    c = _seams.utt_from_gaps(np.asarray(sh(4) + hi(6) + lo(2) + hi(11) + lo(1) + sh(9) + hi(5) + lo(2) + hi(6)), 63, first=29)
    d = (np.zeros(9600, dtype=np.int16), FS, np.arange(1, 38) * 0.005, np.zeros(37))
    return [a, b, c, d]


def frame_kinds(left, right, n_fft=4096):
    """The kinds of frames in host tables of left / right lengths, as a set of names."""
    left, right = np.asarray(left), np.asarray(right)
    ln = left + right + 1
    kinds = set()
    if ((left <= 512) & (right <= 511)).any():
        kinds.add("class-4")
    if (left > 512).any():
        kinds.add("full-class")
    if ((ln > 1024) & (ln <= n_fft)).any():
        kinds.add("second-tile")
    if (ln > n_fft).any():
        kinds.add("truncated")
    if (left == 0).any():
        kinds.add("L=0")
    return kinds


def quiet(fn, *a, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with np.errstate(all="ignore"):
            return fn(*a, **kw)
