"""
float64 model of the lossless analysis and of its backward pass, for
tests/test_lossless_analysis_autograd_host.py and tests/test_gpu_lossless_analysis_autograd.py.  Needs neither a GPU nor
the library.

forward_torch is the forward of k_analysis (magphase.py:74-119, :266-334, :457-476) restated in plain torch float64, so
that torch's autograd gives the gradients; grads_closed is the closed form the HIP kernels implement, in numpy.
"""
import numpy as np
import torch

from magphase_amd import hostmath as hm

FS = 16000
TINY = 1.0e-37      # mag^2 below this: the forward's clamp region, the gradient is defined as zero there


def frames_of(v_pm_sec, v_voi, n_smpls, fs=FS):
    """(pm, left, right, voi) of one utterance, as LosslessAnalysisPlan's numpy path builds them."""
    pm_sec, voi = hm.clean_epochs(v_pm_sec, v_voi, check_len_smpls=n_smpls, fs=fs)
    pm, left, right = hm.frame_bounds(pm_sec * fs, n_smpls)
    return pm, left, right, voi


def window(L, R, n):
    """float64 weights w(k), 0 <= k < n, of a frame with L samples before and R after its centre: the rising Hann half
    np.hanning(2 L + 1)[:L + 1] (1 at the centre; [1.] for L == 0), then the falling half of np.hanning(2 R + 1)."""
    k = np.arange(n, dtype=np.float64)
    up = np.sin(0.5 * np.pi * k / L) ** 2 if L > 0 else np.ones(n)
    down = np.sin(0.5 * np.pi * (L + R - k) / R) ** 2 if R > 0 else np.zeros(n)
    return np.where(k <= L, up, down)


def _geom(L, R, N):
    n = min(L + R + 1, N)
    rot = L if L < N else 0
    return n, (np.arange(n) - rot) % N


def forward_torch(sig, pm, left, right, fft_len):
    """One utterance: sig torch float64 [n] -> (mag, real, imag) [F x H] (differentiable).  The zero branch is taken
    BEFORE the square root (X == 0 -> all three outputs 0 with zero gradient), so autograd sees no sqrt'(0)."""
    N = int(fft_len)
    rows = []
    for p, L, R in zip(np.asarray(pm).tolist(), np.asarray(left).tolist(), np.asarray(right).tolist()):
        n, idx = _geom(L, R, N)
        frm = sig[p - L:p - L + n] * torch.from_numpy(window(L, R, n))
        buf = torch.zeros(N, dtype=sig.dtype).index_add(0, torch.from_numpy(idx), frm)
        rows.append(torch.fft.rfft(buf))
    X = torch.stack(rows) if rows else torch.zeros((0, N // 2 + 1), dtype=torch.complex128)
    s = X.real * X.real + X.imag * X.imag
    zero = s == 0
    den = torch.sqrt(torch.where(zero, torch.ones_like(s), s))
    z = torch.zeros_like(s)
    return torch.where(zero, z, den), torch.where(zero, z, X.real / den), torch.where(zero, z, X.imag / den)


def forward_numpy(sig, pm, left, right, fft_len):
    with torch.no_grad():
        return tuple(t.numpy() for t in forward_torch(torch.as_tensor(np.asarray(sig, dtype=np.float64)), pm, left, right,
                                                      fft_len))


def grads_autograd(sig, grads, pm, left, right, fft_len):
    """d sig float64 numpy of sum_k sum(grads[k] * forward[k]) by torch autograd; grads[k] None: output k not used."""
    x = torch.tensor(np.asarray(sig, dtype=np.float64), requires_grad=True)
    out = forward_torch(x, pm, left, right, fft_len)
    loss = sum((o * torch.as_tensor(np.asarray(g, dtype=np.float64))).sum() for o, g in zip(out, grads) if g is not None)
    if not (torch.is_tensor(loss) and loss.requires_grad):
        return np.zeros(x.shape)
    loss.backward()
    return x.grad.numpy()


def grads_closed(mag, real, imag, grads, pm, left, right, n_smpls, fft_len):
    """The closed form, numpy float64, from the forward's OUTPUTS mag / real / imag [F x H]: pointwise gX -> Y -> the
    unnormalised inverse real transform -> rotation, window -> scatter-add."""
    N = int(fft_len)
    mag, real, imag = (np.asarray(a, dtype=np.float64) for a in (mag, real, imag))
    gm, gr, gi = (np.zeros(mag.shape) if g is None else np.asarray(g, dtype=np.float64) for g in grads)
    live = mag * mag >= TINY
    inv = np.where(live, 1.0 / np.where(live, mag, 1.0), 0.0)
    d = real * gr + imag * gi
    gX = (np.where(live, gm, 0.0) * real + (gr - real * d) * inv) + 1j * (np.where(live, gm, 0.0) * imag + (gi - imag * d) * inv)
    Y = 0.5 * gX
    Y[:, 0] = gX[:, 0].real
    Y[:, -1] = gX[:, -1].real
    b = N * np.fft.irfft(Y, n=N, axis=1)
    gsig = np.zeros(int(n_smpls))
    for f, (p, L, R) in enumerate(zip(np.asarray(pm).tolist(), np.asarray(left).tolist(), np.asarray(right).tolist())):
        n, idx = _geom(L, R, N)
        gsig[p - L:p - L + n] += b[f, idx] * window(L, R, n)
    return gsig


def gather_by_table(per_frame, start, scratch_off, n_smpls):
    """What k_analysis_bwd_gather computes from hostmath.analysis_backward_table's tables: per sample the frames that
    cover it, found as the kernel finds them (the first frame that ends after the sample, then on while frames start at or
    before it), added in ascending frame order.  per_frame: the compact scratch, frame f at scratch_off[f]."""
    start, off = np.asarray(start), np.asarray(scratch_off)
    end = start + np.diff(off)
    out = np.zeros(int(n_smpls))
    for t in range(int(n_smpls)):
        f = int(np.searchsorted(end, t, side="right"))
        while f < start.size and start[f] <= t:
            if t - start[f] < off[f + 1] - off[f]:
                out[t] += per_frame[off[f] + t - start[f]]
            f += 1
    return out


def tone_and_noise(rng, n, f0=140.0, fs=FS, noise_db=-10.0):
    """A harmonic tone (8 partials, random phases) plus white noise noise_db below it: no bin lies far below the rest
    (the phase gradients scale with 1 / mag)."""
    t = np.arange(n) / fs
    x = sum(np.cos(2 * np.pi * f0 * h * t + rng.uniform(0, 2 * np.pi)) / h for h in range(1, 9))
    x = x / np.sqrt(np.mean(x * x))
    return 0.1 * (x + 10.0 ** (noise_db / 20.0) * rng.randn(n))


def epochs(n_frames, spacing_smpls, voiced, fs=FS, first=None):
    """n_frames epochs `spacing_smpls` apart (seconds), all voiced or all unvoiced; the signal length that leaves one more
    period after the last."""
    first = spacing_smpls if first is None else first
    pm = first + spacing_smpls * np.arange(n_frames)
    return pm / fs, np.full(n_frames, 1.0 if voiced else 0.0), int(np.ceil(pm[-1] + spacing_smpls)) + 2


def rel_err(got, ref):
    """max |got - ref| / max |ref| over a whole vector (no sample left out); the plain max |got - ref| where the reference
    is all zero."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape
    if ref.size == 0:
        return 0.0
    scale = np.max(np.abs(ref))
    return float(np.max(np.abs(got - ref)) / (scale if scale > 0 else 1.0))
