"""CPU: the descriptor table of mpx_rows_pack, the numpy model of its kernel, the C entry's argument errors and the
argument checks of the batch API that need no device."""
import ctypes

import numpy as np
import pytest
import torch

import rows_pack_model as model
from magphase_amd import _lib, hostmath as hm
from magphase_amd import magphase as mp

SIZE = {torch.float32: 4, torch.float16: 2, torch.bfloat16: 2, torch.float64: 8}
CODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2, torch.float64: 3}


def _entry(table, i):
    e = table[i]
    return int(e["base"]), int(e["row_stride"]), int(e["dtype"]), int(e["n_rows"]), int(e["out_row0"])


def test_record_layout_matches_the_c_struct():
    assert hm.ROWS_PACK_DTYPE.itemsize == 32
    assert [hm.ROWS_PACK_DTYPE.fields[k][1] for k in ("base", "row_stride", "dtype", "n_rows", "out_row0")] == [0, 8, 16, 20, 24]


def test_table_contiguous():
    a, b = torch.zeros(7, 60), torch.zeros(5, 60)
    ra, rb = torch.zeros(7, 45), torch.zeros(5, 45)
    table, widths, rows = hm.rows_pack_table([[a, b], [ra, rb]])
    assert widths == [60, 45] and rows == [12, 12] and table.shape == (4,)
    assert _entry(table, 0) == (a.data_ptr(), 60, 0, 7, 0)
    assert _entry(table, 1) == (b.data_ptr(), 60, 0, 5, 7)
    assert _entry(table, 2) == (ra.data_ptr(), 45, 0, 7, 0)
    assert _entry(table, 3) == (rb.data_ptr(), 45, 0, 5, 7)


@pytest.mark.parametrize("dtype", model.DTYPES)
def test_table_column_slices_of_one_wide_tensor(dtype):
    wides = [torch.zeros(9, 151, dtype=dtype), torch.zeros(4, 151, dtype=dtype)]
    cuts = [model.column_slices(w) for w in wides]
    table, widths, rows = hm.rows_pack_table([[c[k] for c in cuts] for k in range(3)])
    assert widths == [60, 45, 45] and rows == [13, 13, 13]
    sz, code = SIZE[dtype], CODE[dtype]
    for s, col0 in enumerate((0, 60, 105)):
        for u, (n, row0) in enumerate(((9, 0), (4, 9))):
            base, stride, dt, n_rows, out_row0 = _entry(table, s * 2 + u)
            assert base - wides[u].data_ptr() == col0 * sz      # the slice is read where it lies
            assert (stride, dt, n_rows, out_row0) == (151, code, n, row0)


def test_table_row_strided_views_and_a_zero_row_utterance():
    w0, w1, w2 = torch.zeros(9, 151), torch.zeros(6, 151), torch.zeros(8, 151)
    mags = [w0[::2, :60], w1[0:0, :60], w2[1::2, :60]]          # 5 rows, none, 4 rows
    table, widths, rows = hm.rows_pack_table([mags])
    assert widths == [60] and rows == [9]
    assert _entry(table, 0) == (w0.data_ptr(), 302, 0, 5, 0)
    assert _entry(table, 1) == (0, 60, 0, 0, 5)                 # nothing to read: no pointer, rows 5 .. 5
    assert _entry(table, 2) == (w2.data_ptr() + 151 * 4, 302, 0, 4, 5)


def test_table_refuses_what_the_kernel_cannot_read():
    with pytest.raises(ValueError, match="dtype"):
        hm.rows_pack_table([[torch.zeros(3, 4, dtype=torch.int32)]])
    with pytest.raises(ValueError, match="column stride"):
        hm.rows_pack_table([[torch.zeros(3, 8)[:, ::2]]])
    with pytest.raises(ValueError, match="columns"):
        hm.rows_pack_table([[torch.zeros(3, 8), torch.zeros(3, 7)]])
    with pytest.raises(ValueError, match="2-D|-D"):
        hm.rows_pack_table([[torch.zeros(3)]])


def _streams(dtype, n_utts, seed, strided=False):
    """mag | real | imag column slices of `n_utts` wide tensors (utterance 1 has no rows when there are three or more)."""
    wides = []
    for u in range(n_utts):
        n = 0 if (u == 1 and n_utts >= 3) else 3 + (5 * u + seed) % 11
        wides.append(model.wide_tensor(2 * n if strided else n, 151, dtype, 100 * seed + u))
    cuts = [model.column_slices(w[::2] if strided else w) for w in wides]
    return wides, [[c[k] for c in cuts] for k in range(3)]


@pytest.mark.parametrize("dtype", model.DTYPES)
@pytest.mark.parametrize("strided", (False, True))
def test_model_equals_torch_cat(dtype, strided):
    """The model (descriptor table + the kernel's conversions) against torch's own conversion and concatenation: f32
    bit for bit (NaN payloads, -0), f16 / bf16 widened exactly, f64 narrowed round-to-nearest-even (ties, overflow to
    inf, float32 denormals)."""
    _keep, streams = _streams(dtype, 4, 3, strided)
    outs = model.pack_model(streams)
    for st, out in zip(streams, outs):
        ref = torch.cat([t.float() for t in st])
        assert out.shape == tuple(ref.shape)
        if dtype == torch.float64:   # a NaN's payload is not pinned by the narrowing: NaN where NaN, bits elsewhere
            nan = np.isnan(ref.numpy())
            assert np.array_equal(np.isnan(out.view(np.float32)), nan)
            assert np.array_equal(out[~nan], model.bits(ref)[~nan])
        else:
            assert np.array_equal(out, model.bits(ref))


def test_model_f64_ties_round_to_even():
    v = model.special_values(torch.float64)
    out = model.pack_model([[v.reshape(1, -1)]])[0].view(np.float32)[0]
    assert out[2] == np.float32(1.0)                          # 1 + 2^-24: tie, to the even mantissa below
    assert out[3] == np.float32(1.0 + 2.0 ** -22)             # 1 + 3 * 2^-24: tie, to the even mantissa above
    assert out[4] == np.float32(1.0 + 2.0 ** -23)             # just above the tie: up
    assert out[6] == np.float32(2.0 ** -149) and out[7] == 0.0 and out[8] == np.float32(2.0 ** -149)
    assert np.isinf(out[11]) and out[11] > 0 and np.isinf(out[12]) and out[12] < 0
    assert np.signbit(out[1]) and out[1] == 0.0


def test_model_pitched_output_leaves_the_padding_alone():
    _keep, streams = _streams(torch.float32, 2, 1)
    out = model.pack_model(streams[:1], lds=[64])[0]
    assert out.shape[1] == 64 and np.all(out[:, 60:] == 0xFFFFFFFF)
    assert np.array_equal(out[:, :60], model.bits(torch.cat(streams[0])))


# ---------------------------------------------------------------------------------------------------------------------
# the C entry: argument errors are found on the host, without a device
# ---------------------------------------------------------------------------------------------------------------------
def _call(lib, table, host, n_utts, n_streams, s0=(None, 0, 0, 0), s1=(None, 0, 0, 0), s2=(None, 0, 0, 0)):
    return lib.mpx_rows_pack(None, table, host, n_utts, n_streams, *s0, *s1, *s2)


def test_c_entry_argument_errors_without_gpu():
    lib = _lib.load()
    out = ctypes.c_void_p(0x1000)                   # never dereferenced: every call below fails (or returns) before a launch
    assert _call(lib, None, None, 1, 1, (out, 10, 10, 5)) == -1 and b"null" in lib.mpx_last_error()
    assert _call(lib, None, None, -1, 1, (out, 10, 10, 5)) == -1 and b"n_utts" in lib.mpx_last_error()
    assert _call(lib, None, None, 1, 4) == -1 and b"n_streams" in lib.mpx_last_error()
    assert _call(lib, None, None, 1, 1, (out, -10, 10, 5)) == -1 and b"negative" in lib.mpx_last_error()
    assert _call(lib, None, None, 1, 1, (out, 10, 10, -5)) == -1 and b"negative" in lib.mpx_last_error()
    assert _call(lib, None, None, 1, 1, (out, 10, 8, 5)) == -1 and b"pitch" in lib.mpx_last_error()
    # U == 0 and zero-row batches are no-ops
    assert _call(lib, None, None, 0, 3) == 0
    assert _call(lib, None, None, 0, 1, (None, 10, 10, 0)) == 0
    assert _call(lib, None, None, 0, 1, (out, 10, 10, 5)) == -1 and b"without utterances" in lib.mpx_last_error()
    # the host image of the table is checked entry by entry
    t = np.zeros(2, dtype=hm.ROWS_PACK_DTYPE)
    t["base"], t["row_stride"], t["n_rows"], t["out_row0"] = 0x2000, 10, [3, 2], [0, 3]
    p = t.ctypes.data
    t["dtype"] = [0, 4]
    assert _call(lib, p, p, 2, 1, (out, 10, 10, 5)) == -1 and b"type code" in lib.mpx_last_error()
    t["dtype"] = [0, -1]
    assert _call(lib, p, p, 2, 1, (out, 10, 10, 5)) == -1 and b"type code" in lib.mpx_last_error()
    t["dtype"] = [0, 3]
    t["n_rows"] = [3, -2]
    assert _call(lib, p, p, 2, 1, (out, 10, 10, 5)) == -1 and b"negative" in lib.mpx_last_error()
    t["n_rows"] = [3, 2]
    t["out_row0"] = [0, 4]
    assert _call(lib, p, p, 2, 1, (out, 10, 10, 5)) == -1 and b"follow" in lib.mpx_last_error()
    t["out_row0"] = [0, 3]
    assert _call(lib, p, p, 2, 1, (out, 10, 10, 6)) == -1 and b"do not fill" in lib.mpx_last_error()
    assert _call(lib, p, None, 2, 1, (out, 10, 10, 5)) == -1 and b"null" in lib.mpx_last_error()
    t["n_rows"] = [0, 0]
    t["out_row0"] = [0, 0]
    assert _call(lib, p, p, 2, 1, (None, 10, 10, 0)) == 0      # utterances without rows: nothing is launched


# ---------------------------------------------------------------------------------------------------------------------
# argument checks of the batch API that are made before the engine (and so before a device) is touched
# ---------------------------------------------------------------------------------------------------------------------
def _utt(lf0_dtype=torch.float32, mag_dtype=torch.float32, rows=6):
    return (torch.zeros(rows, 60, dtype=mag_dtype), torch.zeros(rows, 45), torch.zeros(rows, 45),
            torch.zeros(rows, dtype=lf0_dtype))


def test_float16_lf0_is_rejected():
    for fn in (mp.synthesis_from_compressed_batch, mp.synthesis_from_compressed_type2_batch):
        with pytest.raises(ValueError, match=r"utts\[0\]: v_lf0.*float16"):
            fn([_utt(lf0_dtype=torch.float16)], 48000)
    with pytest.raises(ValueError, match=r"v_lf0.*float16"):
        mp.synthesis_from_compressed(*_utt(lf0_dtype=torch.float16), 48000)


@pytest.mark.parametrize("dtype", (torch.int32, torch.int64, torch.bool, torch.complex64))
def test_non_float_tensors_are_rejected(dtype):
    for fn in (mp.synthesis_from_compressed_batch, mp.synthesis_from_compressed_type2_batch):
        with pytest.raises(ValueError, match=r"utts\[1\]: m_mag_mel_log: dtype"):
            fn([_utt(), _utt(mag_dtype=dtype)], 48000)
    feats = (torch.zeros(4, 2049), torch.zeros(4, 2049, dtype=dtype), torch.zeros(4, 2049), np.zeros(4), 48000)
    for fn in (mp.synthesis_from_lossless_batch, mp.synthesis_from_lossless_const_rate_batch):
        with pytest.raises(ValueError, match=r"utts\[0\]: m_real: dtype"):
            fn([feats])


def test_prepared_with_tensors_is_rejected():
    with pytest.raises(ValueError, match="prepared"):
        mp.synthesis_from_compressed_batch([_utt()], 48000, prepared=object())


def test_return_device_excludes_async_out():
    with pytest.raises(ValueError, match="return_device"):
        mp.synthesis_from_compressed_batch([_utt()], 48000, pcm16_norm=0.98, async_out=True, return_device=True)
    sig = (np.zeros(4800, dtype=np.float32), 48000, np.array([0.01, 0.02]), np.array([1.0, 1.0]))
    with pytest.raises(ValueError, match="return_device"):
        mp.analysis_compressed_batch([sig], as_float32=True, async_out=True, return_device=True)
