"""
Float64 numpy restatement of what mpx_synthesis_compressed_ola, mpx_synthesis_compressed_ola_spectra and
mpx_synthesis_compressed_type2_ola are documented to compute (include/magphase_hip.h; oracle.magphase_oracle
.synthesis_from_compressed from the crossfade mask to the overlap-add), written from those two texts and not from the kernel,
together with the operand sets tests/test_gpu_synth_comp_kernel.py launches (tests/test_synth_comp_model_host.py holds the
model to the oracle and checks every operand set on the CPU).

Per frame f:

  noise frame   type2_kernels_model.noise_frame(noise, pos, L, R, wtype) -- the windowed samples noise[pos - L .. pos + R] --
                placed circularly with the epoch at index 0, np.fft.rfft at N -> Ns
  row           with row tables x[row0] + (x[row1] - x[row0]) row_t for mag, real and imag, in float64 on the float32
                inputs; otherwise row f
  X_k           m_k (apc_k inv_gain_f Ns_k + voiced_f per_v_k (a_k + j b_k) / |a_k + j b_k|), apc = ap_v for a voiced frame
                and ap_u otherwise; the periodic term is zero where a_k == b_k == 0 and from bin n_per on
  bins 0, N/2   |X| (type 1) or Re X (type 2), imaginary part zero
  frame         fftshift(irfft(X)) under the centred window: half_windows(win_l, win_r) at N/2 - win_l, zero outside
  waveform      lossless_kernels_model.ola_gather's sum in float64

and per output sample n of a frame the norm the GPU test states its bounds in,

  B[n] = w[n] sum_k c_k m_k (|apc_k inv_gain| ||noise frame||_1 + voiced per_v_k [k < n_per]) / N,   c_k = 1 at bins 0 and N/2, else 2,

summed over the frames that reach a sample.  With row tables the float32 interpolation fma(x1 - x0, t, x0) adds, in units of
u = 2^-24,

  B_lerp[n] = w[n] sum_k c_k ((|m1 - m0| t + |m|) (|apc inv_gain| ||noise frame||_1 + voiced per_v)
                              + m voiced per_v ((|a1 - a0| t + |a|) + (|b1 - b0| t + |b|)) / |a + j b|) / N

(the difference and the fused multiply-add round once each; an error dv of the phase vector v = a + j b moves the unit
phasor by at most |dv| / |v|).

phase_read_set(N, n_per_bins) is the header's n_per_bins contract as a mask over the bins: what a caller must fill.
"""
import numpy as np

import compressed_kernels_model as ck
import lossless_kernels_model as lk
import type2_kernels_model as t2k
from magphase_amd import hostmath as hm

U = lk.U
FFT_LENS = (1024, 2048, 4096)


def eff_n_per(n_per_bins, N):
    """n_per_bins as the entries take it: 0 (or less) and more than H mean no promise."""
    H = N // 2 + 1
    return H if (n_per_bins <= 0 or n_per_bins > H) else int(n_per_bins)


def phase_read_set(N, n_per_bins):
    """bool [H]: the bins of a voiced frame's real / imag rows the one-row-per-frame form reads (include/magphase_hip.h,
    n_per_bins): whole 64-bin groups -- [64 q, 64 q + 63] below N/4 with 64 q < n_per; [N/4, N/4 + 63] when n_per > N/4;
    [N/4 + 1 + 64 j, N/4 + 64 + 64 j] with N/4 + 1 + 64 j < n_per."""
    H, Q = N // 2 + 1, N // 4
    n_per = eff_n_per(n_per_bins, N)
    read = np.zeros(H, dtype=bool)
    for q0 in range(0, Q, 64):
        if q0 < n_per:
            read[q0:q0 + 64] = True
    if n_per > Q:
        read[Q:Q + 64] = True
    for lo in range(Q + 1, H, 64):
        if lo < n_per:
            read[lo:lo + 64] = True
    return read


class Case:
    """One launch's operands (host arrays as the entry takes them) and the utterance layout of its output."""

    def __init__(self, **kw):
        self.row0 = self.row1 = self.row_t = None
        self.type2 = False
        self.n_per_bins = 0
        self.frames_per_run = 1
        self.__dict__.update(kw)

    @property
    def H(self):
        return self.N // 2 + 1

    @property
    def F(self):
        return int(self.npos.size)

    @property
    def frame_off(self):
        return np.concatenate(([0], np.cumsum([len(r) for r in self.pm_rel]))).astype(np.int64)

    @property
    def out_off(self):
        return np.concatenate(([0], np.cumsum(self.out_len))).astype(np.int64)

    @property
    def pm_rel_cat(self):
        return np.concatenate(self.pm_rel).astype(np.int32)

    def lerp(self):
        return self.row0 is not None


def noise_spectrum(noise, pos, L, R, wtype, N):
    """(Ns complex [N/2 + 1], ||windowed frame||_1)."""
    frm = t2k.noise_frame(noise, int(pos), int(L), int(R), int(wtype))
    assert frm.size == L + R + 1 <= N
    c = np.zeros(N)
    c[(np.arange(frm.size) - int(L)) % N] = frm
    return np.fft.rfft(c), float(np.sum(np.abs(frm)))


def frame_rows(c, f):
    """(m, a, b float64 [H], lerp terms (dm, da, db) or None)."""
    x = [np.asarray(v, dtype=np.float64) for v in (c.mag, c.real, c.imag)]
    if not c.lerp():
        return x[0][f], x[1][f], x[2][f], None
    r0, r1, t = int(c.row0[f]), int(c.row1[f]), float(c.row_t[f])
    y = [v[r0] + (v[r1] - v[r0]) * t for v in x]
    d = [np.abs(v[r1] - v[r0]) * abs(t) + np.abs(yy) for v, yy in zip(x, y)]
    return y[0], y[1], y[2], d


def window(N, wl, wr):
    w = np.zeros(N)
    w[N // 2 - wl:N // 2 + wr + 1] = t2k.half_windows(int(wl), int(wr))
    return w


def frame_spectrum(c, f):
    """(X complex [H] after the DC / Nyquist rule, per-bin norm, per-bin lerp norm)."""
    N, H = c.N, c.H
    Ns, l1 = noise_spectrum(c.noise, c.npos[f], c.nleft[f], c.nright[f], c.wtype[f], N)
    m, a, b, d = frame_rows(c, f)
    v = bool(c.voiced[f])
    apc = np.asarray(c.ap_v if v else c.ap_u, dtype=np.float64)
    ig = float(c.inv_gain[f])
    per = np.asarray(c.per_v, dtype=np.float64) * (np.arange(H) < eff_n_per(c.n_per_bins, N)) * (1.0 if v else 0.0)
    per_term = np.zeros(H, dtype=complex)
    if v:
        with np.errstate(invalid="ignore"):      # real / imag the contract leaves unread may be NaN where per == 0
            den = np.hypot(a, b)
        on = (per != 0.0) & (den > 0.0)
        per_term[on] = per[on] * (a[on] + 1j * b[on]) / den[on]
        per = np.where(np.nan_to_num(den, nan=1.0) > 0.0, per, 0.0)
    X = m * (apc * ig * Ns + per_term)
    X[0] = X[0].real if c.type2 else abs(X[0])
    X[-1] = X[-1].real if c.type2 else abs(X[-1])
    ck_ = np.full(H, 2.0)
    ck_[0] = ck_[-1] = 1.0
    amp = np.abs(apc * ig) * l1 + per
    norm = ck_ * np.abs(m) * amp
    lerp = np.zeros(H)
    if d is not None:
        lerp = ck_ * d[0] * amp
        on = per != 0.0
        lerp[on] += (ck_ * np.abs(m) * per)[on] * ((d[1] + d[2])[on] / np.hypot(a, b)[on])
    return X, norm, lerp


def frame(c, f):
    """(windowed frame float64 [N], B [N], B_lerp [N], window support bool [N])."""
    N = c.N
    X, norm, lerp = frame_spectrum(c, f)
    w = window(N, c.win_l[f], c.win_r[f])
    y = np.fft.fftshift(np.fft.irfft(X, n=N)) * w
    sup = np.zeros(N, dtype=bool)
    sup[N // 2 - c.win_l[f]:N // 2 + c.win_r[f] + 1] = True
    return y, w * (norm.sum() / N), w * (lerp.sum() / N), sup


def synthesis(c):
    """-> dict: pcm (float64 [total_out]), B, B_lerp (the norms summed over the frames that reach a sample), count (how many
    frames' window supports reach it), frames [F x N]."""
    rows = [frame(c, f) for f in range(c.F)]
    out = {}
    for key, i in (("pcm", 0), ("B", 1), ("B_lerp", 2), ("count", 3)):
        m = np.array([r[i] for r in rows], dtype=np.float64).reshape(c.F, c.N)
        out[key] = lk.ola_gather(m, c.frame_off, c.pm_rel_cat, c.out_start, c.out_off, c.N, dtype=np.float64)
    out["frames"] = np.array([r[0] for r in rows]).reshape(c.F, c.N)
    return out


def derived_units(N, lerp=False):
    """The derived bound of one frame's sample in units of u B[n] (tests/test_gpu_synth_comp_kernel.py's docstring)."""
    return 10 * np.log2(N) + 46


# ---------------------------------------------------------------------------------------------------------------------
# operand sets shared by the CPU and GPU tests
# ---------------------------------------------------------------------------------------------------------------------
def win_values(N):
    """win_l / win_r of the single-frame cases: the row boundaries of the overlap-add (128 samples per register row) and the
    largest values hostplan.plan_synthesis_numpy accepts (win_l <= N/2, win_r + 1 <= N/2)."""
    return (0, 1, 63, 64, 65, 127, 128, N // 2), (0, 1, 63, 64, 65, 127, 128, N // 2 - 1)


def tile_lengths(N):
    """Frame lengths around the two staging tiles (32 P and 64 P samples, P = N / 128)."""
    return [t + d for t in (N // 4, N // 2) for d in (-1, 0, 1)]


def frame_shapes(N):
    """(L, R): compressed_kernels_model.noise_shapes, then every tile length split three ways (L == 0, R == 0, uneven)."""
    s = list(ck.noise_shapes(N))
    for n in tile_lengths(N):
        for L in (0, n - 1, n // 3):
            if (L, n - 1 - L) not in s:
                s.append((L, n - 1 - L))
    return s


def _f32(x):
    return np.asarray(x, dtype=np.float32)


def _away_from_zero(x):
    """|x| >= 2e-3 (1e-3 with room for the float32 rounding), the sign kept."""
    return np.where(np.abs(x) < 2e-3, np.where(x < 0, -2e-3, 2e-3), x)


def _phase(rs, shape):
    """normal values with |x| >= 1e-3."""
    return _away_from_zero(rs.normal(size=shape))


def _mags(rs, F, H):
    """120 dB across the bins: falling, rising or with the peak inside, per row; a factor in [0.7, 1.4] per element."""
    k = np.arange(H) / (H - 1.0)
    prof = np.stack([10.0 ** (-6.0 * k), 10.0 ** (-6.0 * (1 - k)), 10.0 ** (-12.0 * np.abs(k - 0.37))])
    return prof[np.arange(F) % 3] * rs.uniform(0.7, 1.4, size=(F, H))


def _curves(rs, N, n_per):
    """Synthetic curves: per_v in [0.5, 1.5] exactly below n_per and 0 from there on, ap_v and ap_u in [0.25, 1]."""
    H = N // 2 + 1
    per_v = rs.uniform(0.5, 1.5, H) * (np.arange(H) < n_per)
    return _f32(per_v), _f32(rs.uniform(0.25, 1.0, H)), _f32(rs.uniform(0.25, 1.0, H))


def _lay_noise(rs, left, right):
    """Every frame's samples in a segment of its own (alternating parity of the first sample), NaN everywhere else."""
    pos, total = t2k.layout(np.asarray(left), np.asarray(right), np.arange(len(left)) % 2)
    gap = 3
    pos = pos + gap * (np.arange(len(left)) + 1)
    noise = np.full(total + gap * (len(left) + 1), np.nan, dtype=np.float32)
    for p, L, R in zip(pos, left, right):
        n = L + R + 1
        noise[p - L:p + R + 1] = _f32(rs.uniform(0.05, 1.0, n) * np.where(rs.randint(0, 2, n) == 1, 1.0, -1.0))
    return noise, pos.astype(np.int64)


def _single_layout(N, F):
    """F utterances of one frame each: the output is the frame itself, out_start 0, N samples."""
    return dict(pm_rel=[np.zeros(1, np.int64) for _ in range(F)], out_start=np.zeros(F, np.int32),
                out_len=np.full(F, N, dtype=np.int64))


def _poison(c):
    """NaN in every real / imag element the contract leaves unread (one-row form): every bin of an unvoiced frame, the
    complement of phase_read_set of a voiced one."""
    assert not c.lerp()
    dead = ~phase_read_set(c.N, c.n_per_bins)
    for x in (c.real, c.imag):
        x[np.asarray(c.voiced) == 0] = np.nan
        x[:, dead] = np.nan
    return c


def single_frame_case(N, lerp, type2, n_per_bins, seed=0):
    """Every frame shape x both noise windows x voiced / unvoiced, one frame per utterance; win_l / win_r, inv_gain (three
    decades) and the row tables cycle through their values with periods coprime to the shapes'."""
    rs = np.random.RandomState(1000 + seed + N + 7 * lerp + 13 * type2 + n_per_bins)
    H = N // 2 + 1
    rows = [(L, R, w, v) for (L, R) in frame_shapes(N) for w in (0, 1) for v in (1, 0)]
    F = len(rows)
    left, right, wtype, voiced = (np.array([r[i] for r in rows], dtype=np.int32) for i in range(4))
    wls, wrs = win_values(N)
    i = np.arange(F)
    win_l = np.array(wls, dtype=np.int32)[(i // 4 + i) % len(wls)]
    win_r = np.array(wrs, dtype=np.int32)[(3 * (i // 4) + i // 2) % len(wrs)]
    inv_gain = _f32(10.0 ** rs.uniform(-2.0, 1.0, F))
    noise, npos = _lay_noise(rs, left, right)
    per_v, ap_v, ap_u = _curves(rs, N, eff_n_per(n_per_bins, N))
    c = Case(N=N, type2=type2, n_per_bins=n_per_bins, noise=noise, npos=npos, nleft=left, nright=right, wtype=wtype,
             voiced=voiced, inv_gain=inv_gain, win_l=win_l, win_r=win_r, per_v=per_v, ap_v=ap_v, ap_u=ap_u,
             **_single_layout(N, F))
    if not lerp:
        c.mag, c.real, c.imag = _f32(_mags(rs, F, H)), _f32(_phase(rs, (F, H))), _f32(_phase(rs, (F, H)))
        zero = np.flatnonzero(voiced)[::3]                 # a == b == 0 on some bins of every third voiced frame
        for x in (c.real, c.imag):
            x[np.ix_(zero, [0, 5, 64, 70, N // 4, H - 2, H - 1])] = 0.0
        c.real[zero, 71], c.imag[zero, 72] = 0.0, 0.0      # (one of the two: still a phasor)
        return _poison(c)
    # row tables: R rows, two of them named by no entry (NaN); t at 0, at 1, interior; row0 == row1 with t != 0
    R = F // 2 + 4
    ang = rs.uniform(-np.pi, np.pi, (1, H)) + rs.uniform(-0.5, 0.5, (R, H))      # rows within 1 rad of each other
    rad = rs.uniform(0.5, 2.0, (R, H))
    c.mag = _f32(_mags(rs, 1, H) * rs.uniform(0.7, 1.4, (R, H)))
    c.real, c.imag = _f32(_away_from_zero(rad * np.cos(ang))), _f32(_away_from_zero(rad * np.sin(ang)))
    for x in (c.real, c.imag):
        x[:, [0, 64, H - 1]] = np.where(np.arange(R)[:, None] % 4 == 0, 0.0, x[:, [0, 64, H - 1]])
    row0 = (i // 2) % (R - 2)
    row1 = np.where(i % 5 == 0, row0, np.minimum(row0 + 1 + (i % 3 == 0), R - 3))
    c.row0, c.row1 = row0.astype(np.int32), row1.astype(np.int32)
    c.row_t = _f32(np.choose(i % 6, [0.0, 1.0, 0.37, 0.5, 2.0 ** -24, 1.0 - 2.0 ** -24]))
    c.row_t[(i % 5 == 0) & (c.row_t == 0)] = 0.61          # row0 == row1 with a weight that is not 0
    for x in (c.mag, c.real, c.imag):
        x[R - 2:] = np.nan
    return c


ONE_HOT_ANGLES = (0.3, 2.0, np.pi, -1.2, 0.0, -np.pi / 2)


def one_hot_bins(N, n_per):
    M = N // 2
    want = (0, 1, 63, 64, n_per - 1, n_per, M // 2 - 1, M // 2, M // 2 + 1, M - 1, M)
    return sorted({k for k in want if 0 <= k <= M})


def one_hot_case(N, lerp, type2, n_per_bins, seed=0):
    """mag one-hot at one_hot_bins, the phase a unit phasor at ONE_HOT_ANGLES (in every bin: only the hot one counts):
    voiced frames with ap_v == 0 (the periodic term alone; the hot bins from n_per on give exact silence) and one unvoiced
    frame per bin with an arbitrary per_v.  With row tables: row0 == row1 == f, row_t 0."""
    rs = np.random.RandomState(2000 + seed + N + 7 * lerp + 13 * type2 + n_per_bins)
    H = N // 2 + 1
    n_per = eff_n_per(n_per_bins, N)
    bins = one_hot_bins(N, n_per)
    spec = [(k, a, 1) for k in bins for a in ONE_HOT_ANGLES] + [(k, 0.7, 0) for k in bins]
    F = len(spec)
    hot = np.array([s[0] for s in spec])
    voiced = np.array([s[2] for s in spec], dtype=np.int32)
    mag = np.zeros((F, H))
    mag[np.arange(F), hot] = rs.uniform(0.5, 2.0, F)
    ang = np.array([s[1] for s in spec])[:, None] * np.ones((1, H))
    real, imag = np.cos(ang), np.sin(ang)
    real[np.abs(real) < 1e-6], imag[np.abs(imag) < 1e-6] = 0.0, 0.0      # cos(pi / 2), sin(pi): exact zeros
    left = np.full(F, 40, dtype=np.int32) + (np.arange(F) % 7).astype(np.int32)
    right = np.full(F, 55, dtype=np.int32) - (np.arange(F) % 5).astype(np.int32)
    noise, npos = _lay_noise(rs, left, right)
    per_v, _, ap_u = _curves(rs, N, n_per)
    c = Case(N=N, type2=type2, n_per_bins=n_per_bins, noise=noise, npos=npos, nleft=left, nright=right,
             wtype=(np.arange(F) % 2).astype(np.int32), voiced=voiced, inv_gain=_f32(rs.uniform(0.5, 2.0, F)),
             win_l=np.full(F, N // 2, dtype=np.int32), win_r=np.full(F, N // 2 - 1, dtype=np.int32), per_v=per_v,
             ap_v=np.zeros(H, dtype=np.float32), ap_u=ap_u, mag=_f32(mag), real=_f32(real), imag=_f32(imag),
             hot=hot, angle=np.array([s[1] for s in spec]), **_single_layout(N, F))
    if lerp:
        c.row0 = c.row1 = np.arange(F, dtype=np.int32)
        c.row_t = np.zeros(F, dtype=np.float32)
        return c
    return _poison(c)


def n_per_values(N):
    """The sweep of the issue, where the value exists for the fft_len: (n_per_bins, ...); 0 and H + 7 mean no promise."""
    M = N // 2
    H = M + 1
    want = (1, 63, 64, 65, 511, 512, 513, M // 2, M // 2 + 1, M // 2 + 2, M // 2 + 64, M // 2 + 65, M - 63, M - 1, M, M + 1)
    return sorted({v for v in want if 1 <= v <= H}) + [0, H + 7]


def n_per_case(N, type2, n_per_bins, seed=0):
    """Six voiced and two unvoiced single-frame utterances; per_v nonzero exactly below n_per; real / imag finite random
    (large where per_v == 0: they must not enter) on the documented read set and NaN on its complement."""
    rs = np.random.RandomState(3000 + seed + N + 13 * type2 + n_per_bins)
    H = N // 2 + 1
    F = 8
    voiced = np.array([1, 1, 0, 1, 1, 1, 0, 1], dtype=np.int32)
    left = np.array([3, 100, 64, N // 4, 0, 511, 31, 200], dtype=np.int32)
    right = np.array([100, 3, 64, N // 4 - 1, 77, 511, 32, 0], dtype=np.int32)
    noise, npos = _lay_noise(rs, left, right)
    n_per = eff_n_per(n_per_bins, N)
    per_v, ap_v, ap_u = _curves(rs, N, n_per)
    real, imag = _phase(rs, (F, H)), _phase(rs, (F, H))
    real[:, n_per:] *= 1e3
    imag[:, n_per:] *= 1e3
    wls, wrs = win_values(N)
    c = Case(N=N, type2=type2, n_per_bins=n_per_bins, noise=noise, npos=npos, nleft=left, nright=right,
             wtype=(np.arange(F) % 2).astype(np.int32), voiced=voiced, inv_gain=_f32(rs.uniform(0.1, 3.0, F)),
             win_l=np.array([wls[-1], 128, 65, 64, 200, wls[-1], 1, 300], dtype=np.int32),
             win_r=np.array([wrs[-1], 127, 64, 300, 65, 0, wrs[-1], 128], dtype=np.int32), per_v=per_v, ap_v=ap_v, ap_u=ap_u,
             mag=_f32(_mags(rs, F, H)), real=_f32(real), imag=_f32(imag), **_single_layout(N, F))
    return _poison(c)


MULTI_UTT_FRAMES = (2, 23, 41, 1, 57, 30)
MULTI_SEQUENCES = ("short_long_short", "long_short", "all_long", "alternating")


def multi_frame_case(N, lerp, type2, n_per_bins, frames_per_run=9, seed=0):
    """Six utterances (2, 23, 41, 1, 57 and 30 frames; shifts between N/32 and N/6, so a run of frames_per_run frames spans
    more than N) whose noise-frame lengths follow MULTI_SEQUENCES around the staging tile; the anti-ringing windows are
    the reference's (the two shifts on either side)."""
    rs = np.random.RandomState(4000 + seed + N + 7 * lerp + 13 * type2 + n_per_bins)
    H, tile = N // 2 + 1, N // 4
    left, right, wtype, voiced, win_l, win_r, pm_rel, starts, lens = [], [], [], [], [], [], [], [], []
    short, long_ = (20, tile // 2 - 30), (tile // 2 + 3, N // 2 - 1)
    for u, n in enumerate(MULTI_UTT_FRAMES):
        seq = MULTI_SEQUENCES[u % len(MULTI_SEQUENCES)]
        i = np.arange(n)
        if seq == "short_long_short":
            big = (i >= n // 3) & (i < 2 * n // 3)
        elif seq == "long_short":
            big = i < max(1, n // 2)
        elif seq == "all_long":
            big = np.ones(n, dtype=bool)
        else:
            big = i % 2 == 0
        lo = np.where(big, long_[0], short[0])
        hi = np.where(big, long_[1], short[1])
        L = rs.randint(0, 1 << 30, n) % (hi - lo + 1) + lo
        Rr = rs.randint(0, 1 << 30, n) % (hi - lo + 1) + lo
        left.append(L), right.append(Rr)
        alt = seq == "alternating"
        voiced.append(np.where(alt, i % 2, rs.randint(0, 2, n)))
        wtype.append(np.where(alt, (i // 2) % 2, rs.randint(0, 2, n)))
        shift = rs.randint(N // 32, N // 6 + 1, n)
        v_pm = np.cumsum(shift)
        rel, start, out_len = hm.ola_plan(v_pm, N) if n > 1 else (np.zeros(1, np.int64), 0, N)
        pm_rel.append(rel), starts.append(start), lens.append(out_len)
        se = np.r_[shift[0], shift, shift[-1], shift[-1]]
        win_l.append(se[:n] + se[1:n + 1]), win_r.append(se[2:n + 2] + se[3:n + 3])
    cat = lambda xs: np.concatenate(xs).astype(np.int32)   # noqa: E731
    left, right, wtype, voiced, win_l, win_r = (cat(x) for x in (left, right, wtype, voiced, win_l, win_r))
    F = left.size
    noise, npos = _lay_noise(rs, left, right)
    per_v, ap_v, ap_u = _curves(rs, N, eff_n_per(n_per_bins, N))
    c = Case(N=N, type2=type2, n_per_bins=n_per_bins, noise=noise, npos=npos, nleft=left, nright=right, wtype=wtype,
             voiced=voiced, inv_gain=_f32(10.0 ** rs.uniform(-1.0, 0.5, F)), win_l=win_l, win_r=win_r, per_v=per_v,
             ap_v=ap_v, ap_u=ap_u, pm_rel=pm_rel, out_start=np.array(starts, dtype=np.int32),
             out_len=np.array(lens, dtype=np.int64), frames_per_run=frames_per_run)
    if not lerp:
        c.mag, c.real, c.imag = _f32(_mags(rs, F, H)), _f32(_phase(rs, (F, H))), _f32(_phase(rs, (F, H)))
        return _poison(c)
    R = F // 2 + 2
    ang = rs.uniform(-np.pi, np.pi, (1, H)) + rs.uniform(-0.5, 0.5, (R, H))
    rad = rs.uniform(0.5, 2.0, (R, H))
    c.mag = _f32(_mags(rs, 1, H) * rs.uniform(0.7, 1.4, (R, H)))
    c.real, c.imag = _f32(_away_from_zero(rad * np.cos(ang))), _f32(_away_from_zero(rad * np.sin(ang)))
    i = np.arange(F)
    c.row0 = (i // 2).astype(np.int32)
    c.row1 = np.minimum(c.row0 + (i % 2), R - 1).astype(np.int32)
    c.row_t = _f32(np.where(i % 2, rs.uniform(0.05, 0.95, F), 0.0))
    return c


def identity_tables(c):
    """The one-row case c as a row-table case: row0 == row1 == f, row_t == 0 (real / imag the one-row form leaves unread are
    read by this form: they become 1, 0)."""
    d = Case(**c.__dict__)
    d.real, d.imag = np.where(np.isnan(c.real), np.float32(1.0), c.real), np.where(np.isnan(c.imag), np.float32(0.0), c.imag)
    d.row0 = d.row1 = np.arange(c.F, dtype=np.int32)
    d.row_t = np.zeros(c.F, dtype=np.float32)
    return d


def check_case(c):
    """The self-consistency every operand set must have before it is launched; raises AssertionError."""
    N, H, F = c.N, c.H, c.F
    for name in ("nleft", "nright", "wtype", "voiced", "inv_gain", "win_l", "win_r"):
        assert len(getattr(c, name)) == F, name
    assert np.all(c.nleft >= 0) and np.all(c.nright >= 0) and np.all(c.nleft + c.nright + 1 <= N)
    assert np.all(c.win_l >= 0) and np.all(c.win_r >= 0) and np.all(c.win_l <= N // 2) and np.all(c.win_r + 1 <= N // 2)
    assert set(np.unique(c.wtype)) <= {0, 1} and set(np.unique(c.voiced)) <= {0, 1}
    assert np.all(np.isfinite(c.inv_gain)) and np.all(c.inv_gain > 0)
    for p, L, R in zip(c.npos, c.nleft, c.nright):          # every frame inside the noise, its samples finite
        assert 0 <= p - L and p + R < c.noise.size and np.all(np.isfinite(c.noise[p - L:p + R + 1]))
    for x in (c.per_v, c.ap_v, c.ap_u):
        assert x.shape == (H,) and x.dtype == np.float32 and np.all(np.isfinite(x)) and np.all(x >= 0)
    n_per = eff_n_per(c.n_per_bins, N)
    assert not c.per_v[n_per:].any(), "the caller's promise: per_v == 0 from n_per on"
    rows = c.mag.shape[0]
    assert c.mag.shape == c.real.shape == c.imag.shape == (rows, H) and c.mag.dtype == np.float32
    if c.lerp():
        assert len(c.row0) == len(c.row1) == len(c.row_t) == F
        assert np.all(c.row0 >= 0) and np.all(c.row1 >= 0) and max(c.row0.max(), c.row1.max()) < rows
        assert np.all((c.row_t >= 0) & (c.row_t <= 1))
        named = np.unique(np.concatenate((c.row0, c.row1)))
        for x in (c.mag, c.real, c.imag):
            assert np.all(np.isfinite(x[named]))
        phase = [c.real[named], c.imag[named]]
    else:
        assert rows == F and np.all(np.isfinite(c.mag))
        read = phase_read_set(N, c.n_per_bins)
        v = np.asarray(c.voiced) == 1
        for x in (c.real, c.imag):
            assert np.all(np.isfinite(x[np.ix_(v, read)])), "a bin of the documented read set is not finite"
            assert np.all(np.isnan(x[~v])) and np.all(np.isnan(x[:, ~read])), "the complement of the read set is poisoned"
        phase = [c.real[np.ix_(v, read)], c.imag[np.ix_(v, read)]]
    for x in phase:
        assert np.all((x == 0) | (np.abs(x) >= 1e-3)), "|real|, |imag| are exactly 0 or >= 1e-3"
    assert np.all(c.mag[np.isfinite(c.mag)] >= 0)
    # the utterance layout: ascending positions, every kept sample inside the overlap-add buffer
    assert len(c.pm_rel) == len(c.out_start) == len(c.out_len) and sum(len(r) for r in c.pm_rel) == F
    for rel, s, n in zip(c.pm_rel, c.out_start, c.out_len):
        assert rel[0] == 0 and np.all(np.diff(rel) >= 0) and s >= 0 and n > 0
    return True
