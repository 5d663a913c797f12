"""
A plain numpy model of every kernel of csrc/magphase_epochs.hip, one utterance at a time, in a precision `dt` of the
caller's choice (np.float64 or np.longdouble).  tests/test_epochs_model_host.py pins it on the CPU against independent forms
(avg_pool1d, brute-force window loops, cumsum(diff)); tests/test_gpu_epoch_kernels.py compares the kernels with it.

Nothing here shares code with the device path: sums run one after the other (np.cumsum, np.sum), where the kernels use
trees and tiles, so the two differ by rounding only -- the float64 model against the longdouble model is the yardstick of
that difference.  The second half of the file holds the inputs both test files use, so that what the host test proves
about them (decision margins, crossings next to the ends) holds for the arrays the GPU test uploads.
"""
import numpy as np

from magphase_amd.epochs import _geometry

EPS = 2.0 ** -53
MARGIN_MIN = 1.0e-9      # an NCCF frame whose lag decision sits closer than this to its threshold is not compared
DENOM_MIN = 1.0e-6       # ... nor one whose parabola is this flat


# ----------------------------------------------------------------------------------------------------------------------
# stage 1
# ----------------------------------------------------------------------------------------------------------------------
def mean(x, dt):
    x = np.asarray(x, dtype=dt)
    return dt(np.sum(x) / dt(x.size)) if x.size else dt(0)


def n_decimated(n, dec):
    return max((n + 2 * (dec // 2) - 2 * dec) // dec + 1, 0)


def n_frames(nd, hop, span):
    return (max(nd, span + hop) - span) // hop + 1


def decimate(x, dec, dt, m=None):
    """xd[j] = sum of (x - m) over [j dec - dec//2, j dec - dec//2 + 2 dec), zeros outside the utterance, over 2 dec.
    m: the utterance mean (default: mean(x, dt))."""
    x = np.asarray(x, dtype=dt)
    n = x.size
    m = mean(x, dt) if m is None else dt(m)
    nd = n_decimated(n, dec)
    out = np.zeros(nd, dtype=dt)
    for j in range(nd):
        a = j * dec - dec // 2
        out[j] = np.sum(x[max(a, 0):min(a + 2 * dec, n)] - m) / dt(2 * dec)
    return out


def decimate_bound_terms(x, dec, m):
    """sum |x - m| over each window / (2 dec), longdouble: what the float64 error of xd is measured against."""
    x = np.asarray(x, dtype=np.longdouble)
    n = x.size
    nd = n_decimated(n, dec)
    out = np.zeros(nd, dtype=np.longdouble)
    for j in range(nd):
        a = j * dec - dec // 2
        out[j] = np.sum(np.abs(x[max(a, 0):min(a + 2 * dec, n)] - np.longdouble(m))) / (2 * dec)
    return out


def nccf(xd, hop, win, l_min, n_lags, fs_d, dt, m=None):
    """The normalised cross-correlation of every frame -> dict of arrays [T]: first (shortest lag index within 0.06 of the
    best), f0, peak, energy, margin (min over lags of |r - (best - 0.06)|), denom (of the parabola) and delta."""
    xd = np.asarray(xd, dtype=dt)
    nd = xd.size
    l_max = l_min + n_lags - 1
    span = win + l_max
    T = n_frames(nd, hop, span)
    m = mean(xd, dt) if m is None else dt(m)
    z = np.zeros(max(nd, (T - 1) * hop + span) + 1, dtype=dt)       # zeros past the end
    z[:nd] = xd - m
    out = {k: np.zeros(T, dtype=dt) for k in ("f0", "peak", "energy", "margin", "denom", "delta")}
    out["first"] = np.zeros(T, dtype=np.int64)
    tiny = dt(1.0e-20)
    for t in range(T):
        s0 = t * hop
        a = z[s0:s0 + win]
        W = np.lib.stride_tricks.sliding_window_view(z[s0 + l_min:s0 + l_max + win], win)   # [n_lags, win]
        num = np.sum(W * a, axis=1)
        e_sh = np.sum(W * W, axis=1)
        e_ref = np.sum(a * a)
        r = num / (np.sqrt(e_ref * e_sh) + tiny)
        best = r.max()
        thr = best - dt(0.06)
        first = int(np.argmax(r >= thr))
        li = min(max(first, 1), n_lags - 2)
        denom = r[li - 1] - dt(2.0) * r[li] + r[li + 1] - tiny
        delta = min(max(dt(0.5) * (r[li - 1] - r[li + 1]) / denom, dt(-1.0)), dt(1.0))
        out["first"][t] = first
        out["f0"][t] = dt(fs_d) / (dt(li + l_min) + delta)
        out["peak"][t] = r[first]
        out["energy"][t] = e_ref
        out["margin"][t] = np.min(np.abs(r - thr))
        out["denom"][t] = denom
        out["delta"][t] = delta
    return out


# ----------------------------------------------------------------------------------------------------------------------
# stage 2
# ----------------------------------------------------------------------------------------------------------------------
def scan(x, mode, dt):
    """mode 0: inclusive cumsum(x).  mode 1: x is float32 PCM, cumsum(dx) with dx[0] = 0, dx[i] = x[i] - x[i-1].
    mode 2: cumsum(dx^2)."""
    if mode == 0:
        return np.cumsum(np.asarray(x, dtype=dt))
    x = np.asarray(np.asarray(x, dtype=np.float32), dtype=dt)
    d = np.zeros(x.size, dtype=dt)
    d[1:] = x[1:] - x[:-1]
    return np.cumsum(d if mode == 1 else d * d)


def movmean(y, h, dt):
    """y[i] - (sum of y over [i - h, i + h], replicate padding) / (2 h + 1), from y's own prefix sums; any h >= 0."""
    y = np.asarray(y, dtype=dt)
    n = y.size
    if n == 0:
        return y.copy()
    S = np.concatenate((np.zeros(1, dtype=dt), np.cumsum(y)))          # S[k] = sum of y[:k]
    i = np.arange(n, dtype=np.int64)
    lo, hi = i - int(h), i + int(h)
    lo_c, hi_c = np.maximum(lo, 0), np.minimum(hi, n - 1)
    w = S[hi_c + 1] - S[lo_c]
    w = w + np.maximum(-lo, 0).astype(dt) * y[0] + np.maximum(hi - (n - 1), 0).astype(dt) * y[n - 1]
    return y - w / dt(2 * int(h) + 1)


def zff(x, h, dt):
    """The chain of mpx_epoch_zff on float32 PCM x -> (C, A, B): A the filtered signal whose zero crossings are listed
    (buf_a), C the signal one mean removal earlier (buf_c), B the prefix sums of dx^2 (buf_b)."""
    A = scan(scan(x, 1, dt), 0, dt)
    C = movmean(A, h, dt)
    C = scan(scan(C, 0, dt), 0, dt)
    A = movmean(C, h, dt)
    C = movmean(A, h, dt)
    A = movmean(C, h, dt)
    B = scan(x, 2, dt)
    return C, A, B


def crossing_score_indices(i, n, w):
    """The three indices into the inclusive prefix sums c of dx^2 (index -1 reads 0) of a crossing at sample i: the centre
    q of the two windows of w samples is moved inwards so that both fit, [w, n - w - 1]; an utterance shorter than
    2 w + 1 samples has no such centre, q = i, and the windows are cut at its ends."""
    q = i
    if n >= 2 * w + 1:
        q = min(max(i, w), n - w - 1)
    return tuple(min(max(k, -1), n - 1) for k in (q - 1, q + w - 1, q - w - 1))


def crossings(A, B, w):
    """Zero crossings of A (float64) in both directions -> two lists (p = 0: a > 0 and b <= 0; p = 1: a < 0 and b >= 0) of
    (idx, slope, frac, score), float64, in the order of idx.  score = (c[q+w] - c[q]) - (c[q] - c[q-w]) on B."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    n = A.size
    a, b = A[:-1], A[1:]
    lists = []
    c = np.concatenate((B, np.zeros(1)))                                # c[-1] = 0
    for p in (0, 1):
        sel = (a > 0) & (b <= 0) if p == 0 else (a < 0) & (b >= 0)
        rows = []
        for i in np.flatnonzero(sel) + 1:
            i = int(i)
            iq, ip, im = crossing_score_indices(i, n, w)
            av, bv = A[i - 1], A[i]
            rows.append((i, abs(bv - av), bv / (bv - av), (c[ip] - c[iq]) - (c[iq] - c[im])))
        lists.append(rows)
    return lists


def track(x, fs, dt):
    """The whole front end on one utterance with the model in place of the kernels and the package's own host functions:
    float32 where the device rounds to float32 -> (pm, voi) as epochs.track_epochs returns them."""
    from magphase_amd import epochs
    x = np.asarray(x, dtype=np.float32)
    dec, fs_d, hop, win, l_min, l_max = _geometry(fs)
    n_lags = l_max - l_min + 1
    xd = decimate(x, dec, dt)
    r = nccf(xd, hop, win, l_min, n_lags, fs_d, dt)
    as32 = lambda v: np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)   # noqa: E731
    f0_h, half = epochs._voicing_from_candidates(as32(r["f0"]), as32(r["peak"]), as32(r["energy"]), fs)
    w = max(2, int(round(0.001 * fs)))
    cap = x.size // 16 + 64
    _C, A, B = zff(x, half, dt)
    lists = crossings(np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64), w)
    cnt = np.array([len(lists[0]), len(lists[1])])
    idx_h = np.zeros((2, cap), dtype=np.int32)
    slope_h, score_h, frac_h = (np.zeros((2, cap)) for _ in range(3))
    for p in (0, 1):
        for k, (i, sl, fr, sc) in enumerate(lists[p][:cap]):
            idx_h[p, k], slope_h[p, k], frac_h[p, k], score_h[p, k] = i, as32(sl), as32(fr), as32(sc)
    return epochs._epochs_from_crossings(x.size, fs, f0_h, cnt, idx_h, slope_h, score_h, frac_h, cap, hop / fs_d, win / fs_d)


# ----------------------------------------------------------------------------------------------------------------------
# the inputs of tests/test_gpu_epoch_kernels.py (and of the host test's statements about them)
# ----------------------------------------------------------------------------------------------------------------------
SIGNALS = ("utt", "noise", "zeros", "const", "impulse")
F0_RATES = (8000, 16000, 22050, 44100, 48000)
ZFF_RATES = (16000, 48000)
E2E_CASE = (3, 16000, 1.0)         # (utterance, fs, seconds) of the end-to-end comparison
_CACHE = {}


def make_signal(kind, n, fs, start=0):
    """float32 [n].  utt: synthetic utterance 3 (1 s at fs) / 32768 from sample `start`; noise: RandomState(0) white noise
    at 0.1; zeros; const: 0.25; impulse: 0.5 at n // 2."""
    if kind == "utt":
        if ("utt", fs) not in _CACHE:
            from magphase_amd import synthetic
            _CACHE["utt", fs] = (synthetic.make_utterance(3, 1.0, fs)[0] / 32768.0).astype(np.float32)
        u = _CACHE["utt", fs]
        assert start + n <= u.size
        return u[start:start + n].copy()
    if kind == "noise":
        if "noise" not in _CACHE:
            _CACHE["noise"] = (0.1 * np.random.RandomState(0).randn(65536)).astype(np.float32)
        assert start + n <= 65536
        return _CACHE["noise"][start:start + n].copy()
    x = np.zeros(n, dtype=np.float32)
    if kind == "const":
        x[:] = 0.25
    elif kind == "impulse" and n:
        x[n // 2] = 0.5
    elif kind not in ("zeros", "impulse"):
        raise ValueError(kind)
    return x


def f0_lengths(fs):
    """Utterance lengths of the ragged mpx_epoch_f0_track batch at fs: nd in {255, 256, 257} (the block edge of
    k_epoch_decimate), T % 4 in {0, 1, 2, 3} (four frames per workgroup of k_epoch_nccf), n < dec (nd = 0), nd < span
    (every frame runs past the end) and n = 1."""
    dec, _fs_d, hop, win, _l_min, l_max = _geometry(fs)
    span = win + l_max

    def n_for(nd):      # the shortest utterance with nd decimated samples
        return (nd - 1) * dec + 2 * dec - 2 * (dec // 2)

    lens = [n_for(255), 1, n_for(span + 7 * hop), n_for(256), dec - 1, n_for(span + 4 * hop) + dec - 1, n_for(257),
            n_for(span - 1), n_for(span + 5 * hop), n_for(span + 6 * hop)]
    nds = [n_decimated(n, dec) for n in lens]
    Ts = [n_frames(nd, hop, span) for nd in nds]
    assert {255, 256, 257} <= set(nds) and 0 in nds and span - 1 in nds
    assert {T % 4 for T in Ts} == {0, 1, 2, 3}
    return lens


F0_KINDS = ("utt", "noise", "utt", "zeros", "noise", "utt", "const", "utt", "noise", "utt")   # per utterance of f0_lengths


def f0_batch(fs):
    """[(kind, float32 signal)] of the f0 batch at fs.  The slices of the synthetic utterance start inside its first
    voiced stretch; the impulse is left to the zero-frequency filter's tests: away from it every lag of a frame correlates
    alike, and the parabola of such a frame is flat (denom -> 0: nothing to compare)."""
    key = ("f0", fs)
    if key not in _CACHE:
        out, s_n = [], 0
        for n, kind in zip(f0_lengths(fs), F0_KINDS):
            out.append((kind, make_signal(kind, n, fs, start=s_n if kind == "noise" else int(0.05 * fs))))
            s_n += n if kind == "noise" else 0
        _CACHE[key] = out
    return _CACHE[key]


def zff_w(fs):
    return max(2, int(round(0.001 * fs)))


def zff_lengths(fs):
    """Short utterances first, last and in the middle: a read past an utterance's ends lands once before the buffer, once
    after it and once in a neighbour."""
    w = zff_w(fs)
    lens = [1, w + 1, 2 * w - 1, 255, 4095, 8192, 2, w, 2 * w, 256, 4096, 12289 + 5, 8193, 4097, 257, 2 * w + 1, w + 2, 3]
    assert sorted(lens) == sorted([1, 2, 3, w, w + 1, w + 2, 2 * w - 1, 2 * w, 2 * w + 1, 255, 256, 257, 4095, 4096, 4097,
                                   8192, 8193, 12289 + 5])
    return lens


def zff_half_wins(fs):
    lens = zff_lengths(fs)
    return [(1, 7, 85 if fs == 16000 else 257, n, 3 * n)[u % 5] for u, n in enumerate(lens)]


def zff_batch(fs, kind):
    """[float32 signal] per utterance of zff_lengths(fs).  utt: slices from 50 ms into the synthetic utterance (voiced);
    noise: consecutive slices."""
    key = ("zff", fs, kind)
    if key not in _CACHE:
        out, s_n = [], 0
        for n in zff_lengths(fs):
            out.append(make_signal(kind, n, fs, start=s_n if kind == "noise" else int(0.05 * fs)))
            s_n += n if kind == "noise" else 0
        _CACHE[key] = out
    return _CACHE[key]


def zff_models(fs, kind):
    """[(C, A, B) float64, (C, A, B) longdouble] per utterance of zff_batch(fs, kind), computed once."""
    key = ("zffm", fs, kind)
    if key not in _CACHE:
        _CACHE[key] = [(zff(x, h, np.float64), zff(x, h, np.longdouble))
                       for x, h in zip(zff_batch(fs, kind), zff_half_wins(fs))]
    return _CACHE[key]
