"""
numpy model of k_rows_pack (magphase_amd/csrc/magphase_pack.hip) on CPU tensors, and the views the tests pack.

The model works from the descriptor table alone, as the kernel does: for every entry it reads HOST memory at
base + (r * row_stride + c) * itemsize, converts the element to float32 (f32: bits unchanged; f16 / bf16: widened; f64:
round to nearest even) and writes it to row out_row0 + r of its stream's output.
"""
import ctypes

import numpy as np
import torch

from magphase_amd import hostmath as hm

STORAGE = {0: np.uint32, 1: np.uint16, 2: np.uint16, 3: np.float64}   # element type code -> how the bytes are read
DTYPES = (torch.float32, torch.float16, torch.bfloat16, torch.float64)


def to_f32_bits(raw, code):
    """Elements read as STORAGE[code] -> the uint32 bit patterns of their float32 values."""
    if code == 0:
        return raw.astype(np.uint32)
    if code == 1:
        return raw.view(np.float16).astype(np.float32).view(np.uint32)
    if code == 2:
        return raw.astype(np.uint32) << np.uint32(16)
    with np.errstate(over="ignore", invalid="ignore"):
        return raw.astype(np.float32).view(np.uint32)


def pack_model(streams, lds=None):
    """streams: lists of CPU tensors as Engine.pack_rows takes them -> per stream a uint32 array [rows x ld] holding the
    float32 bit patterns (columns >= width, when ld > width, keep the fill value 0xFFFFFFFF)."""
    table, widths, rows = hm.rows_pack_table(streams)
    U = len(streams[0])
    outs = []
    for s in range(len(streams)):
        w = widths[s]
        ld = w if lds is None else lds[s]
        out = np.full((rows[s], ld), 0xFFFFFFFF, dtype=np.uint32)
        for u in range(U):
            e = table[s * U + u]
            n, stride, code = int(e["n_rows"]), int(e["row_stride"]), int(e["dtype"])
            if n == 0 or w == 0:
                continue
            st = np.dtype(STORAGE[code])
            n_el = (n - 1) * stride + w
            buf = (ctypes.c_char * (n_el * st.itemsize)).from_address(int(e["base"]))
            flat = np.frombuffer(buf, dtype=st)
            src = np.lib.stride_tricks.as_strided(flat, shape=(n, w), strides=(stride * st.itemsize, st.itemsize))
            r0 = int(e["out_row0"])
            out[r0:r0 + n, :w] = to_f32_bits(np.array(src), code)
        outs.append(out)
    return outs


def bits(t):
    """float32 tensor (any device) -> uint32 numpy array of its bit patterns."""
    return t.detach().cpu().contiguous().view(torch.int32).numpy().view(np.uint32)


def special_values(dtype):
    """Values whose conversion is worth pinning: signed zeros, denormals, the extremes, infinities, a NaN; for float64
    the ties of the narrowing (round to nearest EVEN), values that overflow / underflow float32 and float32 denormals."""
    if dtype == torch.float32:
        b = np.array([0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000,
                      0x7FC00000, 0x7FA12345, 0xFFC0BEEF, 0x3F800001], dtype=np.uint32)   # (NaN payloads: copied as bits)
        return torch.from_numpy(b.view(np.float32).copy())
    if dtype == torch.float16:
        b = np.array([0x0000, 0x8000, 0x0001, 0x83FF, 0x0400, 0x7BFF, 0xFBFF, 0x7C00, 0xFC00, 0x7E00, 0x3C01, 0x3555],
                     dtype=np.uint16)
        return torch.from_numpy(b.view(np.float16).copy())
    if dtype == torch.bfloat16:
        b = np.array([0x0000, 0x8000, 0x0001, 0x807F, 0x0080, 0x7F7F, 0xFF7F, 0x7F80, 0xFF80, 0x7FC0, 0x3F81, 0xD015],
                     dtype=np.uint16)   # (0xD015 = -1e10 rounded to bfloat16: the unvoiced marker)
        return torch.from_numpy(b.view(np.int16).copy()).view(torch.bfloat16)
    v = np.array([0.0, -0.0, 1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -50, -(1.0 + 2.0 ** -24),
                  2.0 ** -149, 2.0 ** -150, 1.5 * 2.0 ** -150, 2.0 ** -126 - 2.0 ** -150, 3.4028235677973366e38, 1e39,
                  -1e39, np.inf, -np.inf, np.nan, -1e10, 0.1, 2.0 ** -1074], dtype=np.float64)
    return torch.from_numpy(v)


def wide_tensor(n_rows, width, dtype, seed):
    """A [n_rows x width] CPU tensor of `dtype`: random values with the special values sprinkled in."""
    g = torch.Generator().manual_seed(seed)
    t = (torch.randn(n_rows, width, generator=g, dtype=torch.float64) * 3.0).to(dtype)
    sp = special_values(dtype)
    flat = t.view(-1)
    if flat.numel():
        idx = torch.randint(0, flat.numel(), (min(sp.numel(), flat.numel()),), generator=g)
        flat[idx] = sp[:idx.numel()]
    return t


def column_slices(wide, mag_dim=60, phase_dim=45):
    """mag | real | imag (| lf0 column) cut from one [F x (mag_dim + 2 phase_dim + 1)] tensor: views, no copy."""
    a, b = mag_dim, mag_dim + phase_dim
    return wide[:, :a], wide[:, a:b], wide[:, b:b + phase_dim], wide[:, b + phase_dim]
