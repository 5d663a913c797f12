"""
numpy / torch float64 model of the acoustic-composition kernels (magphase_amd/csrc/magphase_cmp.hip, DESIGN.md section
3.3q), one function per kernel:

    voiced_neighbours     k_cmp_neighbours: per frame the nearest voiced frame at or before / at or after it (-1: none)
    carried               the statics of the carried stream as k_cmp_compose reads them (cmp_static)
    compose               k_cmp_compose: one utterance's [F x W] row matrix in float64, the kernel's expressions in the
                          kernel's order (numpy has no fused multiply-add and the kernel unit uses none: bit for bit)
    compose_backward      k_cmp_compose_bwd in the kernel's order
    compose_torch         the composition in torch float64, for autograd
    column_moments        k_cmp_moment_tiles / k_cmp_moment_final: count, column sums, centred sums of squares in the
                          device's order (tiles of 128 rows ascending, then the tiles ascending)
    chan_merge, finalize  the host side of mp.AcousticStats

An utterance's statics: x [F x SD], the streams side by side in layout order; dims = the streams' dimensions; interp = the
index of the carried stream ('lf0') or -1.  Voiced: value > 0 (NaN: unvoiced).
"""
import numpy as np

WINDOWS = ((-0.5, 0.0, 0.5), (1.0, -2.0, 1.0))
TILE = 128


def taps(windows):
    w = np.asarray(windows, dtype=np.float64).reshape(-1, 3)
    return np.vstack([[0.0, 1.0, 0.0], w]) if w.size else np.array([[0.0, 1.0, 0.0]])


def voiced_mask(v):
    with np.errstate(invalid="ignore"):
        return np.asarray(v, dtype=np.float64) > 0.0


def voiced_neighbours(v):
    """(prev, next) int32 [F] of one utterance's voicing source v [F]."""
    m = voiced_mask(v)
    F = m.size
    idx = np.arange(F)
    prev = np.maximum.accumulate(np.where(m, idx, -1)) if F else np.zeros(0, dtype=np.int64)
    nxt = np.minimum.accumulate(np.where(m, idx, F)[::-1])[::-1] if F else np.zeros(0, dtype=np.int64)
    nxt = np.where(nxt == F, -1, nxt)
    return prev.astype(np.int32), nxt.astype(np.int32)


def carried(x, prev, nxt, zeros=False, fill=0.0):
    """x [F] or [F x D] (float64) with the unvoiced frames replaced; the unvoiced entries of x are never read."""
    x = np.asarray(x, dtype=np.float64)
    F = x.shape[0]
    t = np.arange(F)
    voiced = prev == t
    out = np.empty_like(x)
    tail = (slice(None),) * (x.ndim - 1)
    for i in range(F):
        p, n = int(prev[i]), int(nxt[i])
        if voiced[i]:
            out[i] = x[i]
        elif zeros:
            out[i] = 0.0
        elif p < 0 and n < 0:
            out[i] = fill
        elif p < 0:
            out[i] = x[n]
        elif n < 0:
            out[i] = x[p]
        else:
            lo, hi = x[(p,) + tail], x[(n,) + tail]
            slope = (hi - lo) / np.float64(n - p)
            out[i] = slope * np.float64(i - p) + lo
    return out


def offsets(dims):
    return np.concatenate(([0], np.cumsum(dims))).astype(int)


def compose(x, dims, interp=-1, vuv=False, windows=WINDOWS, mean=None, std=None, fill=0.0, zeros=False, nb=None):
    """One utterance: x [F x SD] -> float64 [F x W]; round with .astype(np.float32) for the device's stored value."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, int(np.sum(dims)))
    F = x.shape[0]
    w = taps(windows)
    K = w.shape[0]
    s0 = offsets(dims)
    W = K * s0[-1] + (1 if vuv else 0)
    y = np.zeros((F, W))
    if interp >= 0:
        prev, nxt = voiced_neighbours(x[:, s0[interp]]) if nb is None else nb
    for s, D in enumerate(dims):
        xs = x[:, s0[s]:s0[s] + D]
        if s == interp:
            xs = carried(xs, prev, nxt, zeros, fill)
        for k in range(K):
            c = K * s0[s] + k * D
            if k == 0:
                y[:, c:c + D] = xs
                continue
            acc = np.zeros((F, D))
            acc[1:] = w[k, 0] * xs[:-1]
            acc = acc + w[k, 1] * xs
            acc[:-1] = acc[:-1] + w[k, 2] * xs[1:]
            y[:, c:c + D] = acc
    if vuv:
        y[:, W - 1] = (prev == np.arange(F)).astype(np.float64)
    if mean is not None:
        y = (y - np.asarray(mean, dtype=np.float64)) / np.asarray(std, dtype=np.float64)
    return y


def _gx(g, std, t, F, c0, D, w):
    K = w.shape[0]
    acc = 0.0
    for k in range(K):
        c = c0 + k * D
        sd = 1.0 if std is None else std[c]
        if k == 0:
            acc = np.float64(g[t, c]) / sd
            continue
        if t > 0:
            acc = acc + w[k, 2] * (np.float64(g[t - 1, c]) / sd)
        acc = acc + w[k, 1] * (np.float64(g[t, c]) / sd)
        if t + 1 < F:
            acc = acc + w[k, 0] * (np.float64(g[t + 1, c]) / sd)
    return acc


def compose_backward(g, x, dims, interp=-1, vuv=False, windows=WINDOWS, std=None):
    """One utterance: g [F x W] (the float32 values the kernel reads) -> gx float64 [F x SD], the kernel's order."""
    g = np.asarray(g)
    F = g.shape[0]
    w = taps(windows)
    K = w.shape[0]
    s0 = offsets(dims)
    std = None if std is None else np.asarray(std, dtype=np.float64)
    gx = np.zeros((F, s0[-1]))
    if interp >= 0:
        prev, nxt = voiced_neighbours(np.asarray(x, dtype=np.float64).reshape(F, -1)[:, s0[interp]])
    for s, D in enumerate(dims):
        for d in range(D):
            c0, sc = K * s0[s] + d, s0[s] + d
            for v in range(F):
                if s != interp:
                    gx[v, sc] = _gx(g, std, v, F, c0, D, w)
                    continue
                if prev[v] != v:
                    continue
                p = int(prev[v - 1]) if v > 0 else -1
                n = int(nxt[v + 1]) if v + 1 < F else -1
                lo, hi = (0 if p < 0 else p + 1), (F - 1 if n < 0 else n - 1)
                acc = 0.0
                for t in range(lo, hi + 1):
                    wt = 1.0
                    if t < v and p >= 0:
                        wt = np.float64(t - p) / np.float64(v - p)
                    if t > v and n >= 0:
                        wt = 1.0 - np.float64(t - v) / np.float64(n - v)
                    acc = acc + wt * _gx(g, std, t, F, c0, D, w)
                gx[v, sc] = acc
    return gx


def compose_torch(x, dims, interp=-1, vuv=False, windows=WINDOWS, mean=None, std=None, fill=0.0):
    """The composition of one utterance in torch float64 (x: a [F x SD] float64 tensor, may require grad)."""
    import torch

    F = int(x.shape[0])
    w = taps(windows)
    K = w.shape[0]
    s0 = offsets(dims)
    cols = []
    voiced = None
    for s, D in enumerate(dims):
        xs = x[:, s0[s]:s0[s] + D]
        if s == interp:
            prev, nxt = voiced_neighbours(x[:, s0[s]].detach().cpu().numpy())
            t = np.arange(F)
            voiced = torch.from_numpy(prev == t).to(x.device)
            clean = torch.where(voiced[:, None], xs, torch.zeros((), dtype=x.dtype, device=x.device))
            p = torch.from_numpy(np.maximum(prev, 0).astype(np.int64)).to(x.device)
            n = torch.from_numpy(np.maximum(nxt, 0).astype(np.int64)).to(x.device)
            has_p = torch.from_numpy(prev >= 0).to(x.device)[:, None]
            has_n = torch.from_numpy(nxt >= 0).to(x.device)[:, None]
            lo, hi = clean[p], clean[n]
            span = torch.from_numpy(np.maximum(nxt - prev, 1).astype(np.float64)).to(x.device)[:, None]
            dt = torch.from_numpy((t - prev).astype(np.float64)).to(x.device)[:, None]
            line = (hi - lo) / span * dt + lo
            held = torch.where(has_p, lo, hi)
            val = torch.where(has_p & has_n, line, held)
            val = torch.where(has_p | has_n, val, torch.full_like(val, float(fill)))
            xs = torch.where(voiced[:, None], clean, val)
        blocks = [xs]
        for k in range(1, K):
            acc = w[k, 1] * xs
            if F > 1:
                acc = acc + torch.cat([torch.zeros_like(xs[:1]), w[k, 0] * xs[:-1]], 0)
                acc = acc + torch.cat([w[k, 2] * xs[1:], torch.zeros_like(xs[:1])], 0)
            blocks.append(acc)
        cols += blocks
    if vuv:
        cols.append(voiced.to(x.dtype)[:, None])
    y = torch.cat(cols, 1)
    if mean is not None:
        y = (y - torch.as_tensor(mean, dtype=x.dtype, device=x.device)) / torch.as_tensor(std, dtype=x.dtype,
                                                                                       device=x.device)
    return y


def column_moments(x):
    """(count, sums [W], centred sums of squares [W]) of x [total x W] (float32 or float64 values) in the device's order."""
    x = np.asarray(x)
    total, W = x.shape
    n_tiles = (total + TILE - 1) // TILE

    def tiled(fn):
        part = np.zeros((n_tiles, W))
        for i in range(n_tiles):
            s = np.zeros(W)
            for r in range(i * TILE, min((i + 1) * TILE, total)):
                s = s + fn(x[r].astype(np.float64))
            part[i] = s
        out = np.zeros(W)
        for i in range(n_tiles):
            out = out + part[i]
        return out

    sums = tiled(lambda row: row)
    m = sums / np.float64(total) if total else sums

    def sq(row):
        dv = row - m
        return dv * dv

    return float(total), sums, tiled(sq)


def chan_merge(a, b):
    """(n, sums, m2) of two batches merged (Chan et al.): m2 = m2_a + m2_b + delta^2 n_a n_b / n."""
    (na, sa, ma), (nb, sb, mb) = a, b
    if na == 0:
        return nb, np.array(sb, dtype=np.float64), np.array(mb, dtype=np.float64)
    if nb == 0:
        return na, np.array(sa, dtype=np.float64), np.array(ma, dtype=np.float64)
    n = na + nb
    delta = sb / nb - sa / na
    return n, sa + sb, ma + mb + delta * delta * (na * nb / n)


def finalize(n, sums, m2):
    mean = sums / n
    std = np.sqrt(m2 / n)
    return mean, np.where(std > 0, std, 1.0)
