"""GPU: the three kernels of magphase_type2.hip through Engine.launch, each against its reference of
tests/type2_kernels_model.py (checked on the CPU by tests/test_type2_kernels_host.py), and the elliptic 60 Hz output
filter against scipy.signal.lfilter at the scan's block and carry edges.  No frame, sample or utterance is left out of any
comparison.

The bounds are derived, not measured (eps = 2^-53, n = left + right + 1 samples, N = fft_len):
  T2K_POWER     |P_dev - P_ref| <= 4 N eps P_ref: first-order error of summing <= N float64 terms one after the other.  The
                three terms of the identity are non-negative and (sum |x|)^2 <= N sum x^2 bounds the cancelling sums against
                the first.  A frame of zeros gives exactly 0.
  T2K_GAIN_VOI  relative 8 eps: the device cos, one product, the float32 -> float64 conversion.
  T2K_GAIN_UNV  |d g| <= 2 n eps sqrt(mean((x w)^2)); a one-sample frame and a frame of zeros give exactly 0.
  T2K_RMS       relative 64 eps against the float64 rms of the device's own power vector; inv_gain = float32(1 / rms)
                within one float32 ulp.
  T2K_ELLIP     1e-6 max(1, peak), test_device_output_hpf_matches_lfilter's bound for the Butterworth design.
within() records the worst value of each as a fraction of its bound (tolerance 1).
"""
import numpy as np
import pytest

import type2_kernels_model as t2k
from _tol import note, within

pytestmark = pytest.mark.gpu
EPS = t2k.EPS
GAIN_WAVES = 8           # frames per workgroup of k_frame_gain / k_noise_power (kGainWaves)
DEFAULT_BLOCKS_PER_CU = 3   # kGainBlocksPerCu


def _engine():
    from magphase_amd.engine import get_engine
    return get_engine()


def _cus(e):
    import torch
    return int(torch.cuda.get_device_properties(e.device).multi_processor_count)


def _frames(e, N, blocks_per_cu, gain):
    """More frames than one pass of the grid-stride loop takes, and no multiple of the frames per workgroup."""
    n = blocks_per_cu * _cus(e) * GAIN_WAVES + 13
    assert n % GAIN_WAVES != 0
    left, right, flag, parity = t2k.frame_table(N, n, gain)
    pos, total = t2k.layout(left, right, parity)
    return left, right, flag, pos, total


def _upload_frames(e, x, pos, left, right):
    assert np.min(pos - left) >= 0 and np.max(pos + right) < x.size   # every read inside the buffer
    return (e.to_device(x, np.float32), e.to_device(pos, np.int64), e.to_device(left, np.int32),
            e.to_device(right, np.int32))


@pytest.mark.parametrize("kind", t2k.SIGNALS)
@pytest.mark.parametrize("N", t2k.FFT_LENS)
def test_frame_gain_against_the_longdouble_reference(N, kind):
    import torch
    e = _engine()
    note("T2K_excluded", 0)
    for bpc_arg, bpc in ((1, 1), (0, DEFAULT_BLOCKS_PER_CU)):
        left, right, voi, pos, total = _frames(e, N, bpc, gain=True)
        x = t2k.make_signal(kind, total)
        d_x, d_pos, d_l, d_r = _upload_frames(e, x, pos, left, right)
        d_voi = e.to_device(voi.astype(np.float32), np.float32)
        F = left.size
        gain = torch.full((F,), -1.0, dtype=torch.float64, device=e.device)
        e.launch("mpx_frame_gain", N, d_x, d_pos, d_l, d_r, d_voi, F, gain, bpc_arg)
        got = gain.cpu().numpy()
        worst_v = worst_u = 0.0
        for f in range(F):
            L, R, v = int(left[f]), int(right[f]), bool(voi[f])
            ref = t2k.frame_gain_ref(x, int(pos[f]), L, R, v, N)
            d = abs(np.longdouble(got[f]) - ref)
            if ref == 0.0 or L + R == 0 and not v:
                assert got[f] == 0.0, (L, R, v, got[f])
                assert ref == 0.0
                continue
            if v:
                worst_v = max(worst_v, float(d / ref) / (8 * EPS))
            else:
                n = L + R + 1
                frm = np.asarray(x[pos[f] - L:pos[f] + R + 1], dtype=np.longdouble) * t2k.half_windows(L, R)
                worst_u = max(worst_u, float(d / np.sqrt(np.mean(frm * frm))) / (2 * n * EPS))
        print("k_frame_gain N %d %s blocks_per_cu %d: %d frames, voiced %.3g, unvoiced %.3g of the bound"
              % (N, kind, bpc, F, worst_v, worst_u))
        within(worst_v, 1.0, "T2K_GAIN_VOI")
        within(worst_u, 1.0, "T2K_GAIN_UNV")


@pytest.mark.parametrize("kind", t2k.SIGNALS)
@pytest.mark.parametrize("N", t2k.FFT_LENS)
def test_noise_power_of_every_frame_against_the_rfft_reference(N, kind):
    import torch
    e = _engine()
    left, right, wtype, pos, total = _frames(e, N, DEFAULT_BLOCKS_PER_CU, gain=False)
    x = t2k.make_signal(kind, total)
    d_x, d_pos, d_l, d_r = _upload_frames(e, x, pos, left, right)
    d_wt = e.to_device(wtype, np.int32)
    F = left.size
    power = torch.full((F,), -1.0, dtype=torch.float64, device=e.device)
    e.launch("mpx_noise_power", N, d_x, d_pos, d_l, d_r, d_wt, F, power)
    got = power.cpu().numpy()
    worst, n_ext = 0.0, 0
    for f in range(F):
        L, R = int(left[f]), int(right[f])
        ext = not t2k.noise_in_domain(L, R, N)
        n_ext += ext
        ref = t2k.noise_power_ref(x, int(pos[f]), L, R, int(wtype[f]), N, extended=ext)
        if ref == 0.0:
            assert got[f] == 0.0, (L, R, got[f])
        else:
            worst = max(worst, abs(got[f] - ref) / ref / t2k.noise_power_bound(N))
    assert n_ext == 20   # five shapes outside the reference's domain, each at two offsets and with both windows
    if kind == "zeros":
        assert np.all(got == 0.0)
    print("k_noise_power N %d %s: %d frames, %.3g of the bound" % (N, kind, F, worst))
    within(worst, 1.0, "T2K_POWER")


RMS_LENS = [1, 2, 0, 255, 256, 257, 513]   # around the strided load (256 threads) and the shared-memory tree
SENTINEL = -7.0


def _noise_rms(e, N, power, off, tail=0):
    import torch
    n_utts = len(off) - 1
    d_power = e.to_device(power if power.size else np.ones(1), np.float64)
    d_off = e.to_device(np.asarray(off), np.int32)
    inv = torch.full((max(int(off[-1]), 1) + tail,), SENTINEL, dtype=torch.float32, device=e.device)
    rms = torch.full((n_utts,), SENTINEL, dtype=torch.float64, device=e.device)
    e.launch("mpx_noise_rms", N, d_power, d_off, n_utts, inv, rms)
    return inv.cpu().numpy(), rms.cpu().numpy()


@pytest.mark.parametrize("N", t2k.FFT_LENS)
def test_noise_rms_at_the_edges_of_its_load_and_tree(N):
    e = _engine()
    off = np.concatenate(([0], np.cumsum(RMS_LENS)))
    total = int(off[-1])
    # powers as k_noise_power gives them for frames of about 10 .. 140 samples, over five decades
    power = np.exp(np.random.RandomState(N).uniform(np.log(1e1), np.log(1e6), total))
    inv, rms = _noise_rms(e, N, power, off, tail=9)
    ref = t2k.noise_rms_ref(power, off, N)
    assert np.all(inv[total:] == SENTINEL), "inv_gain written past the last utterance"
    worst = 0.0
    for u, n in enumerate(RMS_LENS):
        a, b = int(off[u]), int(off[u + 1])
        one_inv, one_rms = _noise_rms(e, N, power[a:b], [0, n], tail=9)
        assert np.array_equal(one_rms, rms[u:u + 1], equal_nan=True), "utterance %d depends on its batch" % u
        assert np.array_equal(one_inv[:n], inv[a:b]) and np.all(one_inv[n:] == SENTINEL)
        if n == 0:
            assert np.isnan(rms[u]) and np.isnan(ref[u])
            continue
        worst = max(worst, abs(rms[u] / ref[u] - 1.0) / (64 * EPS))
        want = np.float32(1.0 / rms[u])
        assert np.all(np.abs(inv[a:b] - want) <= np.spacing(want)), u
    print("k_noise_rms N %d: %.3g of the bound" % (N, worst))
    within(worst, 1.0, "T2K_RMS")


@pytest.mark.parametrize("fs", [48000, 16000])
def test_device_output_hpf_ellip60_matches_lfilter(fs):
    """test_device_output_hpf_matches_lfilter's ragged lengths with the elliptic design (zeros on the unit circle), on
    noise and on stop-band input: a constant and a 20 Hz tone, where an error of the carry across blocks shows best."""
    from scipy import signal
    e = _engine()
    rng = np.random.RandomState(2)
    lens = [1, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 16383, 16384, 16385, 50000, 3000, 240001]
    off = np.concatenate(([0], np.cumsum(lens)))
    b_, a_ = signal.ellip(4, 0.5, 80, 60 / (fs / 2.0), btype="highpass")
    for kind in ("noise", "stop_band"):
        if kind == "noise":
            sigs = [rng.uniform(-1, 1, n).astype(np.float32) for n in lens]
        else:
            sigs = [(0.5 + 0.4 * np.sin(2 * np.pi * 20.0 * np.arange(n) / fs)
                     + rng.uniform(-1e-3, 1e-3, n).astype(np.float32)).astype(np.float32) for n in lens]
        y = e.output_hpf(e.to_device(np.concatenate(sigs), np.float32), off, fs, design="ellip60").cpu().numpy()
        worst = 0.0
        for u, x in enumerate(sigs):
            ref = signal.lfilter(b_, a_, x.astype(np.float64))
            worst = max(worst, np.max(np.abs(y[off[u]:off[u + 1]] - ref)) / (1e-6 * max(1.0, np.max(np.abs(ref)))))
        print("ellip60 @ %d Hz, %s: %.3g of the bound" % (fs, kind, worst))
        within(worst, 1.0, "T2K_ELLIP")
