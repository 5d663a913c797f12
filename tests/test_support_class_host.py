"""
CPU: the support classes of the round-trip kernel (csrc/mpx_common.hpp: frame_support_class) and the pruned in-register
passes they select (csrc/wave_fft.hpp: fft_inreg_pruned_stage).

A frame the round-trip kernel rebuilds is the windowed frame it has just analysed.  Class W promises that the frame's
samples lie in the register rows j < W or j >= P - W of the rotated analysis input and in the rows P/2 - W <= q < P/2 + W
of the rebuilt (fftshifted) frame; the kernel then neither gathers, transforms nor overlap-adds the other rows.  Checked
here: (1) the promise, by placing every sample of every (L, R) and looking at the rows it lands in; (2) the numpy twin
against the library's host entry; (3) a float32 numpy model of the pruned DIF passes against the full pass.
"""
import ctypes

import numpy as np
import pytest

from magphase_amd import _lib, hostmath as hm


def _brev(i, bits):
    r = 0
    for b in range(bits):
        r |= ((i >> b) & 1) << (bits - 1 - b)
    return r


def _row_masks(L, N, r_max):
    """Bit sets of the 128-sample rows that hold a sample of the frame (L, R), R = 0..r_max, by placing the samples one by
    one: sample k of the frame (k < len = min(L + R + 1, N)) sits at n = (k - rot) mod N of the rotated analysis input
    (rot = L if L < N else 0: noise_fft's gather) and at m = (n + N/2) mod N of the rebuilt frame (the fftshift:
    ring_add_plane's ROT).  -> (analysis masks, rebuilt masks), uint64 [r_max + 1]."""
    rot = L if L < N else 0
    k_left = np.arange(min(L + 1, N), dtype=np.int64)            # samples 0..L: present for every R (R = 0: len = L + 1)
    n_left = (k_left - rot) % N
    base_a = np.bitwise_or.reduce(np.uint64(1) << (n_left >> 7).astype(np.uint64))
    base_s = np.bitwise_or.reduce(np.uint64(1) << (((n_left + N // 2) % N) >> 7).astype(np.uint64))
    k_new = L + np.arange(r_max + 1, dtype=np.int64)              # the sample that R adds (none once the frame is cut at N)
    n_new = (k_new - rot) % N
    present = k_new < N
    bit_a = np.where(present, np.uint64(1) << (n_new >> 7).astype(np.uint64), np.uint64(0))
    bit_s = np.where(present, np.uint64(1) << (((n_new + N // 2) % N) >> 7).astype(np.uint64), np.uint64(0))
    return base_a | np.bitwise_or.accumulate(bit_a), base_s | np.bitwise_or.accumulate(bit_s)


def _class_masks(W, P):
    a = sum(1 << j for j in range(P) if j < W or j >= P - W)
    s = sum(1 << q for q in range(P) if P // 2 - W <= q < P // 2 + W)
    return np.uint64(a), np.uint64(s)


@pytest.mark.parametrize("N,step", [(4096, 1), (2048, 7), (1024, 7)])
def test_class_rows_contain_every_sample(N, step):
    P = N // 128
    r = np.arange(N + 201, dtype=np.int64)
    masks = {W: _class_masks(W, P) for W in (4, 8, P // 2) if W <= P // 2}
    seen = set()
    for L in range(0, N + 201, step):
        cls = hm.roundtrip_support_classes(np.full(r.size, L), r, N)
        occ_a, occ_s = _row_masks(L, N, r.size - 1)
        for W in np.unique(cls):
            ca, cs = masks[int(W)]
            m = cls == W
            assert not np.any(occ_a[m] & ~ca), (N, L, int(W))
            assert not np.any(occ_s[m] & ~cs), (N, L, int(W))
            seen.add(int(W))
    assert seen == ({4, 16} if N == 4096 else {P // 2})
    # the narrow class is exactly the stated box (and nothing truncated or unrotated is in it)
    if N == 4096:
        for L, R, W in [(512, 511, 4), (513, 511, 16), (512, 512, 16), (0, 0, 4), (0, 511, 4), (0, 512, 16), (4096, 0, 16),
                        (5000, 100, 16), (2047, 2048, 16), (-1, 10, 16), (10, -1, 16)]:
            assert int(hm.roundtrip_support_classes([L], [R], N)[0]) == W, (L, R)


@pytest.mark.parametrize("N", [4096, 2048, 1024])
def test_numpy_twin_equals_the_native_function(N):
    lib = _lib.load()
    r = np.arange(-3, N + 201, dtype=np.int32)
    out = np.empty(r.size, dtype=np.int32)
    for L in list(range(-3, N + 201, 1 if N == 4096 else 5)):
        left = np.full(r.size, L, dtype=np.int32)
        rc = lib.mpx_roundtrip_support_classes(N, left.ctypes.data, r.ctypes.data, r.size, out.ctypes.data)
        assert rc == 0
        assert np.array_equal(out, hm.roundtrip_support_classes(left, r, N)), (N, L)
    assert lib.mpx_roundtrip_support_classes(1000, None, None, 0, None) != 0
    assert lib.mpx_roundtrip_support_classes(N, None, None, 0, None) == 0
    assert lib.mpx_roundtrip_support_classes(N, None, None, 4, None) != 0


# ---------------------------------------------------------------------------------------------------------------------
# float32 model of wave_fft.hpp's in-register DIF pass and of its pruned stages (the same case analysis, the same order of
# float32 operations; numpy does not fuse multiply-adds, and neither form does in this model)
# ---------------------------------------------------------------------------------------------------------------------
F = np.float32


def _tw(t, sign):
    c = F(np.cos(2 * np.pi * t / 32))
    s = F(np.sin(2 * np.pi * t / 32))
    return c, (F(-s) if sign < 0 else s)


def _zero_after(P, s, z):
    o = 0
    for g in range(0, P, 2 * s):
        for k in range(s):
            i0, i1 = g + k, g + k + s
            if (z >> i0) & 1 and (z >> i1) & 1:
                o |= (1 << i0) | (1 << i1)
    return o


def _need_after(P, s, out):
    need, t = out, 1
    while t < s:
        n2 = 0
        for g in range(0, P, 2 * t):
            for k in range(t):
                i0, i1 = g + k, g + k + t
                if ((need >> i0) | (need >> i1)) & 1:
                    n2 |= (1 << i0) | (1 << i1)
        need, t = n2, t << 1
    return need


def _stage(re, im, P, sign, s, zin=0, out=None):
    """One stage (stride s) of fft_inreg_pruned_stage on [P, lanes] float32 arrays, in place.  Registers in zin are never
    read; registers not needed afterwards are not written."""
    allr = (1 << P) - 1
    need = allr if out is None else _need_after(P, s, out)
    for g in range(0, P, 2 * s):
        for k in range(s):
            i0, i1 = g + k, g + k + s
            t = k * (16 // s) * (32 // P)     # W_{2s}^k as a 32nd root (P = 32: k * 16 / s)
            za, zb = (zin >> i0) & 1, (zin >> i1) & 1
            n0, n1 = (need >> i0) & 1, (need >> i1) & 1
            if (za and zb) or not (n0 or n1):
                continue
            if zb:
                tr, ti = re[i0].copy(), im[i0].copy()
            elif za:
                tr, ti = -re[i1], -im[i1]
                re[i0], im[i0] = re[i1].copy(), im[i1].copy()
            else:
                ar, ai, br, bi = re[i0].copy(), im[i0].copy(), re[i1].copy(), im[i1].copy()
                tr, ti = ar - br, ai - bi
                if n0:
                    re[i0], im[i0] = ar + br, ai + bi
            if not n1:
                continue
            if t == 0:
                re[i1], im[i1] = tr, ti
            elif t == 8:
                re[i1], im[i1] = (ti, -tr) if sign < 0 else (-ti, tr)
            else:
                c, sn = _tw(t, sign)
                re[i1], im[i1] = tr * c - ti * sn, tr * sn + ti * c
    return _zero_after(P, s, zin)


def _pass(re, im, P, sign, zin=0, out=None):
    s, z = P // 2, zin
    while s >= 1:
        z = _stage(re, im, P, sign, s, z, out)
        s >>= 1


def _clear_stride(P, z):
    s = P // 2
    while s >= 1 and z:
        z = _zero_after(P, s, z)
        s >>= 1
    return s


def _prune_stride(P, out):
    allr, s, t = (1 << P) - 1, 0, 1
    while t <= P // 2:
        if _need_after(P, t, out) != allr:
            s = t
        t <<= 1
    return s


@pytest.mark.parametrize("W", [4, 8, 16])
def test_pruned_first_pass_equals_the_full_pass_on_class_inputs(W):
    """Forward side: inputs that are zero outside the class's rows -- the pruned pass never reads those registers (they
    hold garbage here) and gives exactly what the full pass gives on the zero-filled input."""
    P = 32
    rng = np.random.RandomState(W)
    live = np.array([j < W or j >= P - W for j in range(P)])
    zin = sum(1 << j for j in range(P) if not live[j])
    x = (rng.randn(2, P, 64) * np.array([1.0, 1e-3, 1e3, 1e-20])[rng.randint(0, 4, (1, P, 64))]).astype(F)
    x[:, :, 0] = F(-0.0)                      # a lane of negative zeros: the copy keeps the sign, a + 0 drops it, == holds
    full_r, full_i = x[0].copy(), x[1].copy()
    full_r[~live] = 0
    full_i[~live] = 0
    _pass(full_r, full_i, P, -1)
    pr, pi = x[0].copy(), x[1].copy()
    pr[~live] = np.nan                        # never read
    pi[~live] = np.nan
    _pass(pr, pi, P, -1, zin=zin)
    assert np.array_equal(pr, full_r) and np.array_equal(pi, full_i)
    # the kernel's form: pruned stages down to stride 2 S0, the full stages from S0 on
    s0 = _clear_stride(P, zin)
    assert s0 == {4: 4, 8: 8, 16: 16}[W]
    kr, ki = x[0].copy(), x[1].copy()
    kr[~live] = np.nan
    ki[~live] = np.nan
    s, z = P // 2, zin
    while s > s0:
        z = _stage(kr, ki, P, -1, s, z)
        s >>= 1
    assert z == 0
    while s >= 1:
        _stage(kr, ki, P, -1, s)
        s >>= 1
    assert np.array_equal(kr, full_r) and np.array_equal(ki, full_i)


@pytest.mark.parametrize("W", [4, 8, 16])
def test_pruned_last_pass_equals_the_full_pass_on_class_outputs(W):
    """Inverse side: the registers that hold the rows P/2 - W <= q < P/2 + W of the fftshifted frame (register i <-> output
    row brev(i), frame row q = output row (q + P/2) mod P) come out exactly as from the full pass."""
    P, LB = 32, 5
    rng = np.random.RandomState(100 + W)
    out = 0
    for q in range(P):
        if P // 2 - W <= q < P // 2 + W:
            out |= 1 << _brev((q + P // 2) % P, LB)
    x = rng.randn(2, P, 64).astype(F)
    fr, fi = x[0].copy(), x[1].copy()
    _pass(fr, fi, P, +1)
    s1 = _prune_stride(P, out)
    assert s1 == {4: 2, 8: 1, 16: 0}[W]
    pr, pi = x[0].copy(), x[1].copy()
    s = P // 2
    while s > s1:
        _stage(pr, pi, P, +1, s)
        s >>= 1
    while s >= 1:
        _stage(pr, pi, P, +1, s, 0, out)
        s >>= 1
    regs = [i for i in range(P) if (out >> i) & 1]
    assert len(regs) == 2 * W
    assert np.array_equal(pr[regs], fr[regs]) and np.array_equal(pi[regs], fi[regs])
    # and the full pass of the model is the DFT (register i <-> index brev(i))
    z = (x[0] + 1j * x[1]).astype(np.complex128)
    ref = np.fft.ifft(z, axis=0) * P
    got = np.stack([fr[_brev(k, LB)] + 1j * fi[_brev(k, LB)] for k in range(P)])
    assert np.max(np.abs(got - ref)) < 1e-4 * np.max(np.abs(ref))
