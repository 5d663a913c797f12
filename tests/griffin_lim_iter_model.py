"""
fp64 model of ONE Griffin-Lim iteration (reference magphase.py:3355-3370, the loop body after a synthesis) composed from
oracle.magphase_oracle primitives, the error bound of the float32 kernel that performs it (k_griffin_lim_pair,
csrc/magphase_comp.hip) and the batches of tests/test_gpu_griffin_lim_kernel.py.  tests/test_griffin_lim_iter_host.py holds
the model to tests/griffin_lim_model.py and the reference's golden, and the batches to what they claim.

The bound, u = 2^-24, L = log2 N + 8 (the project's (K + 8) 2^-24 style: log2 N butterfly levels, 8 for the window weight,
the product with the sample, the split and the table twiddles):

  spectrum    |X_dev - X| <= delta_f = L u S_f per bin, S_f = sum_n |windowed frame f|
  phasor      |X_dev/|X_dev| - X/|X|| <= e_k = min(2, delta_f / max(|X_k| - delta_f, tiny)): two unit vectors are never more
              than 2 apart, which is what holds for a bin whose |X_k| is within delta_f of zero.  No bin is left out.
  frame       |y_dev - y| <= (1/N) sum_k w_k T_k (e_k + (L + 4) u) per sample, w_k = 1 at DC and Nyquist and 2 elsewhere
              (L u for the inverse transform and the merge, 4 u for |u|^2, the reciprocal square root and two products)
  signal      the frames' bounds overlap-added as the frames are, + u sum |contributions| for the accumulation
  phase rows  |phi_dev - phi| (circular) <= e_k + 4 u pi (the arctangent and its result's rounding near +-pi)
"""
import numpy as np

from oracle import magphase_oracle as orc

U = 2.0 ** -24
TINY = 1e-300
FFT_LENS = (1024, 2048, 4096)
SCALE_EXPS = (-40, -62, -90)     # sig_in scaled by 2^e: below, across and far below the kernel's 2^-60 threshold
FRAMES_PER_RUN = (1, 3, None)
# Share of non-zero samples of the white noise.  The bound adds the bins' errors in one direction while the signal adds
# them with random phases, so bound / peak grows with sqrt(non-zero samples per frame): dense noise under frames of N - 1
# samples misses COND (measured on the model alone: 2.8e-3 at N = 4096), sparse noise of the same spectrum meets it.  The
# shortest frames of a sparse signal are all zeros now and then: X == 0 inside a loud utterance, one more case.
DENSITY = {1024: 0.25, 2048: 0.25, 4096: 0.125}
COND = 1e-3                      # every batch: bound <= COND x the utterance's peak at every sample


def iterate(sig, v_shift, target):
    """One iteration on one utterance: sig float64 [pm_{F-1} + last shift + 1] (what ola returns), v_shift int [F], target
    magnitudes [F x H].  Returns (sig_out, phase [F x H], X [F x H], S [F])."""
    sig = np.asarray(sig, dtype=np.float64)
    target = np.asarray(target, dtype=np.float64)
    v_shift = np.asarray(v_shift).astype(int)
    H = target.shape[1]
    N = 2 * (H - 1)
    v_pm = np.cumsum(v_shift)
    frames = orc.windowing(sig, v_pm)[0]
    m_frm = orc.frm_list_to_matrix(frames, v_shift, N)
    X = np.fft.fft(m_frm)
    phase = np.angle(X)                      # angle(0) = 0
    Y = orc.add_hermitian_half_real(target) * np.exp(1j * phase)
    sig_out = orc.ola(np.fft.ifft(Y).real, v_pm)
    return sig_out, phase[:, :H], X[:, :H], np.sum(np.abs(m_frm), axis=1)


def phasor_error(X, S):
    """e_k [F x H] of the module's docstring."""
    H = X.shape[1]
    N = 2 * (H - 1)
    delta = ((np.log2(N) + 8) * U * np.asarray(S, dtype=np.float64))[:, None]
    return np.minimum(2.0, delta / np.maximum(np.abs(X) - delta, TINY))


def bound(v_shift, target, phase, X, S):
    """Per-output-sample bound of one utterance's iteration (aligned with iterate()'s sig_out) and the per-bin bound of
    its phase rows [F x H]."""
    target = np.asarray(target, dtype=np.float64)
    F, H = target.shape
    N = 2 * (H - 1)
    L = np.log2(N) + 8
    v_pm = np.cumsum(np.asarray(v_shift).astype(int))
    e = phasor_error(X, S)
    w = np.full(H, 2.0)
    w[0] = w[-1] = 1.0
    per_frame = np.sum(w * target * (e + (L + 4) * U), axis=1) / N
    ph_full = np.hstack((phase, -phase[:, -2:0:-1]))
    contrib = np.abs(np.fft.ifft(orc.add_hermitian_half_real(target) * np.exp(1j * ph_full)).real)
    sig_bound = orc.ola(np.repeat(per_frame[:, None], N, axis=1), v_pm) + U * orc.ola(contrib, v_pm)
    return sig_bound, e + 4 * U * np.pi


def circular(a, b):
    """|a - b| on the circle, float64."""
    d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) % (2 * np.pi)
    return np.minimum(d, 2 * np.pi - d)


# ====================================================================================================== the batches
def shifts(N):
    """The utterances' shifts of the batch of fft_len N: every kind of frame_kinds() in one launch of at most 150 frames.
    Utterance 1 is the one of digital silence (between two loud ones)."""
    rng = np.random.RandomState(N)
    half = N // 2
    wide = [512, 513] if half - 1 >= 513 else []

    def around(c, n):
        return list(rng.randint(c - 8, c + 9, n))

    a = [half, 63, 64, 65] + around(155, 5) + wide + around(240, 5) + [half - 1, 155, half - 1]   # right of the last: half - 1
    silence = around(155, 6) + around(240, 8)      # longer than N/2: the responses' peaks lie N/2 before the epochs
    c = [0, 1, 0, 2, 65, 64, 63, 1] + around(155, 6) + [0, 0] + around(240, 4)     # first epoch at sample 0, doubled epochs
    lone = [200]
    two = [half, half - 1]
    f = around(240, 6) + wide[::-1] + around(155, 8) + [63, 64, 65] + around(240, 6)
    return [np.asarray(v, dtype=np.int64) for v in (a, silence, c, lone, two, f)]


SILENT = 1
ONE_HOT_UTT = 5          # the utterance that carries the one-hot target rows ...
ONE_HOT_FRAME0 = 3       # ... from this frame on, one row per bin of one_hot_bins()


def one_hot_bins(N):
    """DC, bin 1, the kernel's handover bin M/2 = N/4, the last bin below Nyquist, Nyquist."""
    return (0, 1, N // 4, N // 2 - 1, N // 2)


def frame_kinds(shift_list, N):
    """The kinds of frames and utterances in a list of shift vectors, as a set of names (with the frame tables of
    hostmath.griffin_lim_plan's convention: left = the frame's shift, right = the next one's, the last frame's its own)."""
    half = N // 2
    kinds = set()
    for v in shift_list:
        v = np.asarray(v)
        right = np.append(v[1:], v[-1])
        if v[0] == half:
            kinds.add("first-left=N/2")
        if np.any(right == half - 1):
            kinds.add("right=N/2-1")
        if np.any(v == 0):
            kinds.add("smallest-shift")
        if v.size == 1:
            kinds.add("lone-frame")
        if v.size == 2:
            kinds.add("two-frame")
        for s in (63, 64, 65, 512, 513, half - 1):
            if np.any(v == s):
                kinds.add("shift-%d" % s)
        if np.any(np.abs(v - 155) <= 8):
            kinds.add("around-155")
        if np.any(np.abs(v - 240) <= 8):
            kinds.add("around-240")
    return kinds


def claimed_kinds(N):
    kinds = {"first-left=N/2", "right=N/2-1", "smallest-shift", "lone-frame", "two-frame", "shift-63", "shift-64", "shift-65",
             "shift-%d" % (N // 2 - 1), "around-155", "around-240"}
    if N // 2 - 1 >= 513:
        kinds |= {"shift-512", "shift-513"}
    return kinds


def out_len(v_shift):
    """Length of ola's output (= of the signal the iteration analyses) in the Griffin-Lim domain (first shift <= N/2)."""
    v = np.asarray(v_shift).astype(int)
    return int(np.sum(v) + v[-1] + 1)


_CACHE = {}


def batch(N):
    """The batch of fft_len N, computed once and not to be modified: dict of
         shifts    list of int64 shift vectors            sig      list of float32 signals (white noise, a share DENSITY
         target    list of float32 [F_u x H] magnitudes             of the samples non-zero, those 2^-10 <= |x| < 1;
                                                                    utterance SILENT: zeros)
         model     list of iterate()'s tuples of the float32 inputs' float64 values
         bound     list of bound()'s pairs."""
    if N in _CACHE:
        return _CACHE[N]
    rng = np.random.RandomState(1000 + N)
    H = N // 2 + 1
    sh = shifts(N)
    sigs, targets = [], []
    for u, v in enumerate(sh):
        n = out_len(v)
        x = rng.uniform(2.0 ** -10, 1.0, n) * np.where(rng.rand(n) < 0.5, -1.0, 1.0) * (rng.rand(n) < DENSITY[N])
        sigs.append((np.zeros(n) if u == SILENT else x).astype(np.float32))
        t = rng.uniform(0.5, 1.5, (v.size, H))
        for row in t:                              # a few exact zeros per row
            row[rng.randint(0, H, 3)] = 0.0
        t[:, 0][::4] = 0.0                         # ... DC, Nyquist and the handover bin among them
        t[:, -1][1::4] = 0.0
        t[:, N // 4][2::4] = 0.0
        if u == ONE_HOT_UTT:
            for i, k in enumerate(one_hot_bins(N)):
                t[ONE_HOT_FRAME0 + i] = 0.0
                t[ONE_HOT_FRAME0 + i, k] = 1.0
        targets.append(t.astype(np.float32))
    model = [iterate(x, v, t) for x, v, t in zip(sigs, sh, targets)]
    bnd = [bound(v, t, m[1], m[2], m[3]) for v, t, m in zip(sh, targets, model)]
    _CACHE[N] = dict(shifts=sh, sig=sigs, target=targets, model=model, bound=bnd)
    return _CACHE[N]
