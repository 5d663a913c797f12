"""GPU: feature matrices that live on the device go in (Engine.pack_rows / mpx_rows_pack) and results stay there
(return_device).  The feature only changes where the float32 values come from, so every comparison is bit for bit."""
import os
import warnings

import numpy as np
import pytest
import torch

import rows_pack_model as model
from magphase_amd import libutils as lu
from magphase_amd import magphase as mp
from magphase_amd import synthetic as syn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRED = os.path.join(ROOT, "demos", "data_48k", "params_predicted")
MAG, PH = 60, 45


def _engine():
    from magphase_amd.engine import get_engine
    return get_engine()


def _predicted():
    """The four bundled predicted utterances (48 kHz; 60 / 45 / 45 / 1) as [F x 151] float32 host matrices."""
    out = []
    for t in ("hvd_704", "hvd_705", "hvd_706", "hvd_708"):
        parts = [np.asarray(lu.read_binfile(os.path.join(PRED, t + e), dim=k), dtype=np.float32).reshape(-1, k)
                 for e, k in ((".mag", MAG), (".real", PH), (".imag", PH), (".lf0", 1))]
        out.append(np.ascontiguousarray(np.concatenate(parts, axis=1)))
    return out


_SYN16 = {}


def _synthetic16(b_const_rate):
    """Synthetic utterances at 16 kHz analysed at fft_len 2048 (60 / 45 / 45), as [F x 151] float32 host matrices."""
    if b_const_rate not in _SYN16:
        utts = []
        for u in range(3):
            pcm, pm, voi = syn.make_utterance(40 + u, dur_s=0.6 + 0.2 * u, fs=16000)
            utts.append((syn.pcm_to_float(pcm), 16000, pm, voi))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res = mp.analysis_compressed_batch(utts, fft_len=2048, mag_dim=MAG, phase_dim=PH, b_const_rate=b_const_rate,
                                               as_float32=True)
        _SYN16[b_const_rate] = (utts, [np.ascontiguousarray(np.concatenate(
            [r[0], r[1], r[2], np.asarray(r[3], dtype=np.float32)[:, None]], axis=1)) for r in res])
    return _SYN16[b_const_rate]


def _dev_utts(wides, dtype=None, lf0_dtype=None):
    """Per utterance ONE device tensor [F x 151]; mag / real / imag / lf0 are column slices of it (views)."""
    dev = _engine().device
    out = []
    for w in wides:
        t = torch.from_numpy(w).to(dev)
        lf0 = t[:, MAG + 2 * PH]
        if dtype is not None:
            t = t.to(dtype)
        m, r, i, _l = model.column_slices(t, MAG, PH)
        out.append((m, r, i, lf0 if lf0_dtype is None else lf0.to(lf0_dtype)))
    return out


def _host_utts(dev_utts, widen=False):
    """The same call's host inputs: tensor.cpu().numpy() (widen: tensor.float().cpu().numpy() for the matrices)."""
    return [tuple((x.float() if widen and k < 3 else x).cpu().numpy() for k, x in enumerate(u)) for u in dev_utts]


def _noise(plan_cls, utts_host, fs, seed, **kw):
    """A fixed noise list of the lengths the plan asks for."""
    ns_len = plan_cls(_engine(), utts_host, fs, noise_mode="device", **kw).ns_len
    rng = np.random.RandomState(seed)
    return [rng.uniform(-1, 1, n) for n in ns_len]


def _same(a, b, dtypes=True):
    """Every element of a equals its partner in b, sample for sample (device tensors through .cpu().numpy());
    dtypes=False: the values only (a float32 device signal against its exactly widened float64 host return)."""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        x = x.cpu().numpy() if torch.is_tensor(x) else x
        y = y.cpu().numpy() if torch.is_tensor(y) else y
        assert (x.dtype == y.dtype or not dtypes) and x.shape == y.shape and x.size > 0
        assert np.array_equal(x, y)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernel against its model
# ---------------------------------------------------------------------------------------------------------------------
def _pack_case(dtype, n_utts, width, strided, zero_mid, seed, pitched=False):
    e = _engine()
    cpu_wide, cpu, dev = [], [[], []], [[], []]
    for u in range(n_utts):
        n = 0 if (zero_mid and u == n_utts // 2) else 1 + (7 * u + seed) % 13
        w = model.wide_tensor(2 * n if strided else n, 2 * width + 3, dtype, 1000 * seed + u)
        cpu_wide.append(w)
        d = w.to(e.device)
        for src, dst in ((w, cpu), (d, dev)):
            v = src[::2] if strided else src
            dst[0].append(v[:, 1:1 + width])               # two streams cut from one tensor, at odd element offsets
            dst[1].append(v[:, 2 + width:2 + 2 * width])
    rows = sum(int(t.shape[0]) for t in cpu[0])
    outs, bufs = [], []
    for _ in range(2):
        ld = int(e.empty_feats(1, width).stride(0)) if pitched else width
        buf = torch.full((max(rows, 1), ld), -1, dtype=torch.int32, device=e.device)
        bufs.append(buf)
        outs.append(buf.view(torch.float32)[:rows, :width])
    e.pack_rows(dev, outs)
    ref = model.pack_model(cpu, lds=[int(b.shape[1]) for b in bufs])
    for b, r in zip(bufs, ref):
        got = b[:rows].cpu().numpy().view(np.uint32)
        if dtype == torch.float64:      # (a NaN's payload is not pinned by the narrowing)
            nan = np.isnan(r[:, :width].view(np.float32))
            assert np.array_equal(np.isnan(got[:, :width].view(np.float32)), nan)
            got, r = got.copy(), r.copy()
            got[:, :width][nan] = 0
            r[:, :width][nan] = 0
        assert np.array_equal(got, r), (dtype, n_utts, width, strided)


@pytest.mark.parametrize("dtype", model.DTYPES)
@pytest.mark.parametrize("strided", (False, True))
def test_pack_rows_every_dtype(dtype, strided):
    for n_utts in (1, 4, 64):
        _pack_case(dtype, n_utts, 45, strided, zero_mid=n_utts > 1, seed=n_utts)


@pytest.mark.parametrize("width", (10, 45, 60, 2049))
def test_pack_rows_widths(width):
    for dtype in (torch.float32, torch.bfloat16):
        _pack_case(dtype, 4, width, False, True, seed=width, pitched=(width == 2049))
        _pack_case(dtype, 64, width, True, True, seed=width + 1, pitched=(width == 2049))


def test_pack_rows_no_utterances_and_no_rows():
    e = _engine()
    out = e.empty((0, 45))
    assert e.pack_rows([[]], [out]) == [out]
    assert e.pack_rows([[torch.zeros(0, 45, device=e.device)]], [out]) == [out]


# ---------------------------------------------------------------------------------------------------------------------
# 2. compressed synthesis: device inputs (column slices of one [F x 151] tensor) equal host inputs
# ---------------------------------------------------------------------------------------------------------------------
def _inputs(which, b_const_rate):
    if which == 48000:
        return 48000, 4096, _predicted()
    return 16000, 2048, _synthetic16(b_const_rate)[1]


@pytest.mark.parametrize("which", (48000, 16000))
@pytest.mark.parametrize("b_const_rate", (False, True))
def test_compressed_synthesis_device_equals_host(which, b_const_rate):
    from magphase_amd.plans import CompressedSynthesisPlan
    fs, N, wides = _inputs(which, b_const_rate)
    d = _dev_utts(wides)
    h = _host_utts(d)
    noise = _noise(CompressedSynthesisPlan, h, fs, 3, fft_len=N, b_const_rate=b_const_rate)
    kw = dict(fft_len=N, b_const_rate=b_const_rate, noise=noise)
    _same(mp.synthesis_from_compressed_batch(d, fs, **kw), mp.synthesis_from_compressed_batch(h, fs, **kw))


@pytest.mark.parametrize("kw", (dict(per_phase_type="magphase"), dict(per_phase_type="min_phase"),
                                dict(per_phase_type="linear"), dict(b_post_filter="magphase"),
                                dict(b_post_filter="merlin"), dict(pcm16_norm=0.98), dict(b_out_hpf=False)))
def test_compressed_synthesis_options_device_equals_host(kw):
    from magphase_amd.plans import CompressedSynthesisPlan
    wides = _predicted()
    d = _dev_utts(wides)
    h = _host_utts(d)
    noise = _noise(CompressedSynthesisPlan, h, 48000, 4, b_const_rate=True)
    kw = dict(kw, b_const_rate=True, noise=noise)
    _same(mp.synthesis_from_compressed_batch(d, 48000, **kw), mp.synthesis_from_compressed_batch(h, 48000, **kw))


def test_compressed_synthesis_device_noise_device_equals_host():
    d = _dev_utts(_predicted())
    kw = dict(b_const_rate=True, noise_mode="device", noise_seeds=[11, 12, 13, 14])
    _same(mp.synthesis_from_compressed_batch(d, 48000, **kw), mp.synthesis_from_compressed_batch(_host_utts(d), 48000, **kw))


def test_single_utterance_wrapper_forwards_tensors():
    d = _dev_utts(_predicted()[:1])
    h = _host_utts(d)
    np.random.seed(2)
    a = mp.synthesis_from_compressed(*d[0], 48000, b_const_rate=True)
    np.random.seed(2)
    b = mp.synthesis_from_compressed(*h[0], 48000, b_const_rate=True)
    _same([a], [b])


# ---------------------------------------------------------------------------------------------------------------------
# 3. the reference noise stream (numpy's global generator)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (0, 7))
def test_reference_noise_stream_device_equals_host(k):
    d = _dev_utts(_predicted())
    h = _host_utts(d)
    np.random.seed(k)
    a = mp.synthesis_from_compressed_batch(d, 48000, b_const_rate=True)
    sa = np.random.get_state()
    np.random.seed(k)
    b = mp.synthesis_from_compressed_batch(h, 48000, b_const_rate=True)
    sb = np.random.get_state()
    _same(a, b)
    assert sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]


# ---------------------------------------------------------------------------------------------------------------------
# 4. bfloat16 / float16 matrices (float32 lf0)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (torch.bfloat16, torch.float16, torch.float64))
def test_half_precision_matrices(dtype):
    from magphase_amd.plans import CompressedSynthesisPlan
    wides = _predicted()
    d = _dev_utts(wides, dtype=dtype)
    assert d[0][0].dtype == dtype and d[0][3].dtype == torch.float32
    h = _host_utts(d, widen=True)
    assert h[0][0].dtype == np.float32
    noise = _noise(CompressedSynthesisPlan, h, 48000, 5, b_const_rate=True)
    kw = dict(b_const_rate=True, noise=noise)
    _same(mp.synthesis_from_compressed_batch(d, 48000, **kw), mp.synthesis_from_compressed_batch(h, 48000, **kw))


def test_device_lf0_dtypes_reach_the_planner_as_their_float64_values():
    e = _engine()
    wides = _predicted()
    for dt in (torch.float32, torch.bfloat16, torch.float64):
        d = _dev_utts(wides, lf0_dtype=dt)
        got = e.lf0_to_host([u[3] for u in d])
        for g, u in zip(got, d):
            assert g.dtype == np.float64 and np.array_equal(g, u[3].double().cpu().numpy())


# ---------------------------------------------------------------------------------------------------------------------
# 5. no host staging
# ---------------------------------------------------------------------------------------------------------------------
def test_device_inputs_do_not_touch_host_staging(monkeypatch):
    from magphase_amd.engine import Engine
    from magphase_amd.plans import CompressedSynthesisPlan
    d = _dev_utts(_predicted())
    h = _host_utts(d)
    noise = _noise(CompressedSynthesisPlan, h, 48000, 6, b_const_rate=True)
    ref = mp.synthesis_from_compressed_batch(h, 48000, b_const_rate=True, noise=noise)

    def boom(*a, **k):
        raise AssertionError("host staging used for device inputs")

    for name in ("stage_rows", "host_staging", "upload_staged"):
        monkeypatch.setattr(Engine, name, boom)
    with pytest.raises(AssertionError):      # the patch bites: the host path does stage
        mp.synthesis_from_compressed_batch([tuple(np.ascontiguousarray(x) for x in u) for u in h], 48000,
                                           b_const_rate=True, noise=noise, engine=_NoPrepare(_engine()))
    _same(mp.synthesis_from_compressed_batch(d, 48000, b_const_rate=True, noise=noise), ref)


class _NoPrepare:
    """The engine without its native planner: the plan takes the generic path (the one device inputs take)."""

    def __init__(self, e):
        self._e = e

    def __getattr__(self, name):
        if name == "prepare_synthesis":
            raise AttributeError(name)
        return getattr(self._e, name)


# ---------------------------------------------------------------------------------------------------------------------
# 6. synthesis return_device
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw, dtype", ((dict(), torch.float64), (dict(b_out_hpf=False), torch.float32),
                                       (dict(pcm16_norm=0.98), torch.int16),
                                       (dict(pcm16_norm=0.98, b_out_hpf=False), torch.int16)))
def test_synthesis_return_device(kw, dtype):
    from magphase_amd.plans import CompressedSynthesisPlan
    e = _engine()
    d = _dev_utts(_predicted())
    h = _host_utts(d)
    noise = _noise(CompressedSynthesisPlan, h, 48000, 8, b_const_rate=True)
    kw = dict(kw, b_const_rate=True, noise=noise)
    for inputs in (d, h):
        dev = mp.synthesis_from_compressed_batch(inputs, 48000, return_device=True, **kw)
        assert all(torch.is_tensor(t) and t.device == e.device and t.dtype == dtype for t in dev)
        _same(dev, mp.synthesis_from_compressed_batch(h, 48000, **kw), dtypes=False)


# ---------------------------------------------------------------------------------------------------------------------
# 7. analysis return_device
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b_const_rate", (False, True))
def test_analysis_return_device(b_const_rate):
    e = _engine()
    utts = _synthetic16(b_const_rate)[0]
    kw = dict(fft_len=2048, mag_dim=MAG, phase_dim=PH, b_const_rate=b_const_rate)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        dev = mp.analysis_compressed_batch(utts, return_device=True, **kw)
        ref = mp.analysis_compressed_batch(utts, as_float32=True, **kw)
    for a, b in zip(dev, ref):
        for k in range(3):
            assert a[k].device == e.device and a[k].dtype == torch.float32
        _same(a[:3], b[:3])
        assert isinstance(a[3], np.ndarray) and np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])
        assert a[5:] == b[5:]


@pytest.mark.parametrize("const_rate_ms", (-1.0, 5.0))
def test_analysis_type2_return_device(const_rate_ms):
    e = _engine()
    utts = _synthetic16(False)[0]
    kw = dict(fft_len=2048, mag_dim=MAG, phase_dim=PH, const_rate_ms=const_rate_ms)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        dev = mp.analysis_compressed_type2_batch(utts, return_device=True, **kw)
        ref = mp.analysis_compressed_type2_batch(utts, **kw)
    for a, b in zip(dev, ref):
        for k in range(3):
            assert a[k].device == e.device and a[k].dtype == torch.float32
            assert np.array_equal(a[k].cpu().numpy().astype(np.float64), b[k]) and b[k].size > 0
        assert np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4]) and np.array_equal(a[7], b[7], equal_nan=True)
        assert a[5:7] == b[5:7]


# ---------------------------------------------------------------------------------------------------------------------
# 8. model in the loop: analysis -> one [F x 151] device tensor per utterance -> slices -> synthesis, all on the device
# ---------------------------------------------------------------------------------------------------------------------
def test_model_in_the_loop():
    from magphase_amd.plans import CompressedSynthesisPlan
    e = _engine()
    utts = _synthetic16(True)[0]
    kw = dict(fft_len=2048, mag_dim=MAG, phase_dim=PH, b_const_rate=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        dev = mp.analysis_compressed_batch(utts, return_device=True, **kw)
        ref = mp.analysis_compressed_batch(utts, as_float32=True, **kw)
    d_in, h_in = [], []
    for a, b in zip(dev, ref):
        lf0 = torch.from_numpy(a[3]).to(e.device).float()
        wide = torch.cat([a[0], a[1], a[2], lf0[:, None]], dim=1)        # [F x (60 + 45 + 45 + 1)]
        assert wide.shape[1] == MAG + 2 * PH + 1
        d_in.append(model.column_slices(wide, MAG, PH))
        hw = np.concatenate([b[0], b[1], b[2], b[3].astype(np.float32)[:, None]], axis=1)
        h_in.append(model.column_slices(hw, MAG, PH))
    noise = _noise(CompressedSynthesisPlan, h_in, 16000, 9, fft_len=2048, b_const_rate=True)
    skw = dict(fft_len=2048, b_const_rate=True, noise=noise)
    out = mp.synthesis_from_compressed_batch(d_in, 16000, return_device=True, **skw)
    assert all(t.device == e.device for t in out)
    _same(out, mp.synthesis_from_compressed_batch(h_in, 16000, **skw))


# ---------------------------------------------------------------------------------------------------------------------
# 9. type 2
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("const_rate_ms", (-1.0, 5.0))
def test_type2_synthesis_device_equals_host(const_rate_ms):
    from magphase_amd.plans import Type2SynthesisPlan
    e = _engine()
    utts = _synthetic16(False)[0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = mp.analysis_compressed_type2_batch(utts, fft_len=2048, mag_dim=MAG, phase_dim=PH, const_rate_ms=const_rate_ms)
    wides = [np.ascontiguousarray(np.concatenate([r[0], r[1], r[2], r[3][:, None]], axis=1).astype(np.float32)) for r in res]
    d = _dev_utts(wides)
    h = _host_utts(d)
    noise = _noise(Type2SynthesisPlan, h, 16000, 10, fft_len=2048, const_rate_ms=const_rate_ms)
    kw = dict(fft_len=2048, const_rate_ms=const_rate_ms, noise=noise)
    ref = mp.synthesis_from_compressed_type2_batch(h, 16000, **kw)
    _same(mp.synthesis_from_compressed_type2_batch(d, 16000, **kw), ref)
    dev = mp.synthesis_from_compressed_type2_batch(d, 16000, return_device=True, **kw)
    assert all(t.device == e.device and t.dtype == torch.float64 for t in dev)
    _same(dev, ref)
    bad = [(u[0], u[1], u[2], torch.full_like(u[3], float("nan"))) for u in d]
    with pytest.raises(ValueError, match="non-finite"):     # the finite-lf0 check sees device lf0 too
        mp.synthesis_from_compressed_type2_batch(bad, 16000, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# 10. lossless
# ---------------------------------------------------------------------------------------------------------------------
def _lossless_utts(n):
    out = []
    for u in range(n):
        pcm, pm, voi = syn.make_utterance(60 + u, dur_s=0.4 + 0.1 * u, fs=16000)
        out.append((syn.pcm_to_float(pcm), 16000, pm, voi))
    return out


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16))
def test_lossless_synthesis_device_equals_host(dtype):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        feats = mp.analysis_lossless_batch(_lossless_utts(3), fft_len=2048, return_device=True)
    d = [tuple(x.to(dtype) for x in f[:3]) + (f[3], f[4]) for f in feats]
    h = [tuple(x.float().cpu().numpy() for x in f[:3]) + (f[3], f[4]) for f in d]
    _same(mp.synthesis_from_lossless_batch(d), mp.synthesis_from_lossless_batch(h))


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16))
def test_lossless_const_rate_synthesis_device_equals_host(dtype):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        feats = mp.analysis_lossless_const_rate_batch(_lossless_utts(3), fft_len=2048, return_device=True)
    d = [tuple(x.to(dtype) for x in f[:3]) + (f[3], f[4]) for f in feats]
    h = [tuple(x.float().cpu().numpy() for x in f[:3]) + (f[3], f[4]) for f in d]
    _same(mp.synthesis_from_lossless_const_rate_batch(d), mp.synthesis_from_lossless_const_rate_batch(h))


def test_lossless_single_float32_utterance_is_taken_without_a_copy(monkeypatch):
    from magphase_amd import plans
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        f = mp.analysis_lossless_batch(_lossless_utts(1), fft_len=2048, return_device=True)[0]
        fc = mp.analysis_lossless_const_rate_batch(_lossless_utts(1), fft_len=2048, return_device=True)[0]
    seen = []
    for cls in (plans.LosslessSynthesisPlan, plans.LosslessConstRateSynthesisPlan):
        run = cls.run

        def spy(self, mag, real, imag, *a, _run=run, **k):
            seen.append((mag.data_ptr(), real.data_ptr(), imag.data_ptr()))
            return _run(self, mag, real, imag, *a, **k)

        monkeypatch.setattr(cls, "run", spy)
    mp.synthesis_from_lossless_batch([f[:5]])
    mp.synthesis_from_lossless_const_rate_batch([fc[:5]])
    assert seen == [tuple(x.data_ptr() for x in f[:3]), tuple(x.data_ptr() for x in fc[:3])]


# ---------------------------------------------------------------------------------------------------------------------
# 11. errors
# ---------------------------------------------------------------------------------------------------------------------
def test_tensor_on_a_second_device_is_rejected():
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU")
    e = _engine()
    other = torch.device("cuda", (e.device.index + 1) % torch.cuda.device_count())
    d = _dev_utts(_predicted()[:2])
    bad = [d[0], (d[1][0], d[1][1].to(other), d[1][2], d[1][3])]
    with pytest.raises(ValueError, match="m_real_mel"):
        mp.synthesis_from_compressed_batch(bad, 48000, b_const_rate=True)
    with pytest.raises(ValueError, match="m_real"):
        mp.synthesis_from_lossless_batch([(torch.zeros(4, 1025, device=e.device), torch.zeros(4, 1025, device=other),
                                           torch.zeros(4, 1025, device=e.device), np.full(4, 100.0), 16000)])


def test_complex_dtype_is_rejected():
    d = _dev_utts(_predicted()[:1])
    bad = [(d[0][0], d[0][1].to(torch.complex64), d[0][2], d[0][3])]
    with pytest.raises(ValueError, match="m_real_mel"):
        mp.synthesis_from_compressed_batch(bad, 48000)


def test_mismatched_row_count_raises_the_existing_error():
    d = _dev_utts(_predicted()[:2])
    bad = [d[0], (d[1][0], d[1][1][:-1], d[1][2], d[1][3])]
    n = int(d[1][0].shape[0])
    with pytest.raises(ValueError, match=r"utterance 1: mag / real / imag / lf0 have %d / %d / %d / %d frames" % (n, n - 1, n, n)):
        mp.synthesis_from_compressed_batch(bad, 48000)
    with pytest.raises(ValueError, match=r"utts\[1\]: mag / real / imag / lf0 have"):
        mp.synthesis_from_compressed_type2_batch(bad, 48000)


def test_non_unit_column_stride_is_accepted():
    from magphase_amd.plans import CompressedSynthesisPlan
    d = _dev_utts(_predicted()[:2])
    h = _host_utts(d)
    noise = _noise(CompressedSynthesisPlan, h, 48000, 12, b_const_rate=True)
    spread = []
    for u in d:
        parts = []
        for x in u[:3]:
            w = torch.zeros(x.shape[0], 2 * x.shape[1], device=x.device)
            w[:, ::2] = x
            parts.append(w[:, ::2])
            assert parts[-1].stride(1) == 2
        spread.append(tuple(parts) + (u[3],))
    kw = dict(b_const_rate=True, noise=noise)
    _same(mp.synthesis_from_compressed_batch(spread, 48000, **kw), mp.synthesis_from_compressed_batch(d, 48000, **kw))


def test_host_arrays_mixed_into_a_device_batch():
    from magphase_amd.plans import CompressedSynthesisPlan
    d = _dev_utts(_predicted())
    h = _host_utts(d)
    noise = _noise(CompressedSynthesisPlan, h, 48000, 13, b_const_rate=True)
    mixed = [d[0], h[1], (d[2][0], h[2][1].astype(np.float64), d[2][2], h[2][3]), d[3]]
    kw = dict(b_const_rate=True, noise=noise)
    _same(mp.synthesis_from_compressed_batch(mixed, 48000, **kw), mp.synthesis_from_compressed_batch(h, 48000, **kw))
