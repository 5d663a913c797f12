"""
float64 models of the true envelope's backward pass (k_true_envelope_bwd), in the formulation of
tests/true_envelope_model.py: forced pass counts K per frame, and optionally GIVEN decisions of the max updates -- the
device's own, unpacked from its decision words -- so that a gradient is compared as the adjoint of the passes as the device
decided them.

    envelope_torch    differentiable torch model: (y, decisions used, margins |s - a| of every decision)
    envelope_np       the same forward in numpy
    envelope_grad_np  the hand-written reverse recursion with S^T g = D^-1 S (D g): the kernel's specification
    pack_decisions / unpack_decisions   bool [F x max_iters x H] <-> int32 [F x max_iters x ceil(H / 32)]
"""
import numpy as np
import torch

import true_envelope_model as tem
from magphase_amd import hostmath as hm

LN10_20 = np.log(10.0) / 20.0


def spectra(F, H, seed, noise_only=(), comb=()):
    """Magnitude rows: harmonic peaks over a tilted floor, times log-normal noise (3 dB).  The rows in noise_only are the
    magnitudes of complex Gaussian noise under a 20 dB tilt (about 25 passes at 60 coefficients and thres_db 0.1).  The rows
    in comb are a line spectrum 120 dB above its floor (a line every 37 bins, 1 dB of noise): at 60 coefficients such a row
    is still rising after 100 passes, at every supported size -- white noise does that only from a spread of 40 dB on, far
    outside the range of the spectra the forward kernel's tolerance was measured on."""
    rng = np.random.default_rng(seed)
    b = np.arange(H) / (H - 1.0)
    rows = []
    for f in range(F):
        if f in noise_only:
            rows.append(20.0 * np.log10(np.abs(rng.normal(size=H) + 1j * rng.normal(size=H))) - 20.0 * b)
            continue
        if f in comb:
            db = np.full(H, -60.0)
            db[::37] = 60.0
            rows.append(db + rng.normal(0.0, 1.0, H))
            continue
        f0 = 0.012 + 0.004 * (f % 5)
        db = -20.0 * b + 6.0 * np.sin(2 * np.pi * (1.5 + f % 3) * b + f) + 18.0 * np.cos(np.pi * b / f0) ** 8
        rows.append(db + rng.normal(0.0, 3.0, H))
    return 10.0 ** (np.array(rows) / 20.0)


def smooth_torch(v, w):
    """tem.smooth on a float64 tensor [F x H], w a float64 tensor [N]."""
    c = torch.fft.ifft(torch.cat((v, v[:, 1:-1].flip(1)), dim=1)).real
    return torch.fft.fft(c * w).real[:, :v.shape[1]]


def _to_db_torch(x, in_type):
    return 20.0 * torch.log10(x) if in_type == "abs" else (x if in_type == "db" else x / LN10_20)


def _from_db_torch(v, in_type):
    return 10.0 ** (v / 20.0) if in_type == "abs" else (v if in_type == "db" else v * LN10_20)


def envelope_torch(x, in_type, ncoeffs, forced, decisions=None, max_iters=hm.TRUE_ENV_MAX_ITERS, fade=0.7):
    """x: float64 tensor [F x H] (may require grad); forced: K per frame.  decisions (optional): bool [F x max_iters x H],
    m_k = decisions[:, k - 1]; without it the model decides itself (s > a).  -> (y [F x H], the decisions used as a bool
    array [F x max_iters x H], zero for k >= K, and the margins |s_k - a_k| in dB as an array of the same shape, inf where
    no decision is made)."""
    F, H = x.shape
    K = np.clip(np.asarray(forced, dtype=np.int64), 1, max_iters)
    w = torch.from_numpy(hm.true_envelope_lifter(2 * (H - 1), ncoeffs, fade))
    a = _to_db_torch(x, in_type)
    out = torch.zeros_like(a)
    used = np.zeros((F, max_iters, H), dtype=bool)
    margin = np.full((F, max_iters, H), np.inf)
    for k in range(1, int(K.max()) + 1):
        s = smooth_torch(a, w)
        last = torch.from_numpy(K == k)[:, None]
        out = torch.where(last, s, out)
        go = K > k
        if not go.any():
            break
        m = (s > a).detach().numpy() if decisions is None else np.asarray(decisions[:, k - 1], dtype=bool)
        m = m & go[:, None]
        used[:, k - 1] = m
        margin[go, k - 1] = np.abs((s - a).detach().numpy())[go]
        a = torch.where(torch.from_numpy(m), s, a)
    return _from_db_torch(out, in_type), used, margin


def envelope_np(x, in_type, ncoeffs, forced, decisions, max_iters=hm.TRUE_ENV_MAX_ITERS, fade=0.7):
    """The forward with given decisions in numpy -> y [F x H] float64."""
    x = np.asarray(x, dtype=np.float64)
    F, H = x.shape
    K = np.clip(np.asarray(forced, dtype=np.int64), 1, max_iters)
    w = hm.true_envelope_lifter(2 * (H - 1), ncoeffs, fade)
    a = tem._TO_DB[in_type](x).copy()
    out = np.zeros_like(a)
    for k in range(1, int(K.max()) + 1):
        s = tem.smooth(a, w)
        out[K == k] = s[K == k]
        m = np.asarray(decisions[:, k - 1], dtype=bool) & (K > k)[:, None]
        a = np.where(m, s, a)
    return tem._FROM_DB[in_type](out)


def smooth_adjoint_np(g, w):
    """S^T g for the smoothing pass S = tem.smooth(., w), as D^-1 S (D g) with D = diag(2, 1, ..., 1, 2)."""
    d = np.array(g, dtype=np.float64)
    d[:, 0] *= 2.0
    d[:, -1] *= 2.0
    t = tem.smooth(d, w)
    t[:, 0] *= 0.5
    t[:, -1] *= 0.5
    return t


def envelope_grad_np(x, gy, in_type, ncoeffs, forced, decisions, max_iters=hm.TRUE_ENV_MAX_ITERS, fade=0.7):
    """The reverse recursion of the issue, per frame with its own K:
        g_s = g_y dy/ds_K;  g_a = 0;  for k = K .. 1:  g_a += S^T g_s;  if k > 1: (g_s, g_a) = m_{k-1} ? (g_a, 0) : (0, g_a)
        g_x = g_a da_1/dx
    -> g_x [F x H] float64."""
    x = np.asarray(x, dtype=np.float64)
    gy = np.asarray(gy, dtype=np.float64)
    F, H = x.shape
    K = np.clip(np.asarray(forced, dtype=np.int64), 1, max_iters)
    w = hm.true_envelope_lifter(2 * (H - 1), ncoeffs, fade)
    y = envelope_np(x, in_type, ncoeffs, K, decisions, max_iters, fade)
    g_s = gy * (y * LN10_20 if in_type == "abs" else (1.0 if in_type == "db" else LN10_20))
    g_a = np.zeros_like(g_s)
    for k in range(int(K.max()), 0, -1):
        run = K >= k                     # frames whose pass k exists (the others have not started yet: g_s waits)
        t = smooth_adjoint_np(np.where(run[:, None], g_s, 0.0), w)
        g_a = g_a + t
        if k > 1:
            m = np.asarray(decisions[:, k - 2], dtype=bool) & run[:, None]
            keep = ~run[:, None]
            g_s = np.where(keep, g_s, np.where(m, g_a, 0.0))
            g_a = np.where(keep, g_a, np.where(m, 0.0, g_a))
    return g_a * ((1.0 / (LN10_20 * x)) if in_type == "abs" else (1.0 if in_type == "db" else 1.0 / LN10_20))


def pack_decisions(m):
    """bool [F x max_iters x H] -> int32 [F x max_iters x ceil(H / 32)]: bit b % 32 of word b / 32 is m[..., b]."""
    m = np.asarray(m, dtype=bool)
    H = m.shape[-1]
    nw = (H + 31) // 32
    pad = np.zeros(m.shape[:-1] + (nw * 32,), dtype=np.uint64)
    pad[..., :H] = m
    words = (pad.reshape(m.shape[:-1] + (nw, 32)) << np.arange(32, dtype=np.uint64)).sum(axis=-1)
    return words.astype(np.uint32).view(np.int32)


def unpack_decisions(words, H):
    """int32 [F x max_iters x ceil(H / 32)] -> bool [F x max_iters x H]."""
    u = np.ascontiguousarray(words, dtype=np.int32).view(np.uint32)
    bits = (u[..., None] >> np.arange(32, dtype=np.uint32)) & 1
    return bits.reshape(u.shape[:-1] + (u.shape[-1] * 32,))[..., :H].astype(bool)
