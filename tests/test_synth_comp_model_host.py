"""
CPU: tests/synth_comp_model.py (the float64 model tests/test_gpu_synth_comp_kernel.py holds k_synth_comp_pair to) against
oracle.magphase_oracle.synthesis_from_compressed and tests/type2_synthesis_model.synthesis -- the assembled spectra
(m_syn) and the waveform before the output filter (v_pre_hpf) to 1e-12 of their peaks, from the oracle's own unwarped
rows, gains, shifts and epochs and the same noise --, the documented read set of the n_per_bins contract against the
column count the plan fills (hostmath.synth_comp_phase_columns), the argument rejections of the three C entries that return
before any launch, and the self-consistency of every operand set the GPU file launches.
"""
import ctypes

import numpy as np
import pytest

import synth_comp_model as scm
import type2_synthesis_model as t2s
from magphase_amd import _lib
from magphase_amd import hostmath as hm
from oracle import magphase_oracle as orc

TOL = 1e-12


def _features(fs, rows, seed):
    """Random compressed features with voiced and unvoiced stretches; f0 between 90 and 250 Hz."""
    rs = np.random.RandomState(seed)
    mag = 0.3 * rs.randn(rows, 60) / (1.0 + np.arange(60))[None, :] ** 0.5
    mag[:, 0] += -2.0
    real, imag = 0.4 * rs.randn(rows, 45), 0.4 * rs.randn(rows, 45)
    f0 = 90.0 + 160.0 * rs.rand(rows)
    lf0 = np.log(f0)
    lf0[rows // 3:rows // 3 + 7] = -1e10
    lf0[-5:] = -1e10
    return mag, real, imag, lf0


def _case_from(N, v_shift, v_pm, v_voi, ns_len, b_voi_ap_win, noise, m_mag, m_real, m_imag, inv_gain, curves, type2):
    n = v_pm.size
    _, lft, rgt = hm.frame_bounds(v_pm, ns_len)
    se = np.r_[v_shift[0], v_shift, v_shift[-1], v_shift[-1]]
    rel, start, out_len = hm.ola_plan(v_pm, N)
    return scm.Case(N=N, type2=type2, n_per_bins=0, noise=noise, npos=v_pm.astype(np.int64), nleft=lft.astype(np.int32),
                    nright=rgt.astype(np.int32), wtype=(v_voi & bool(b_voi_ap_win)).astype(np.int32),
                    voiced=v_voi.astype(np.int32), inv_gain=inv_gain, win_l=(se[:n] + se[1:n + 1]).astype(np.int32),
                    win_r=(se[2:n + 2] + se[3:n + 3]).astype(np.int32), per_v=curves[0], ap_v=curves[1], ap_u=curves[2],
                    mag=m_mag, real=m_real, imag=m_imag, pm_rel=[rel], out_start=np.array([start], np.int32),
                    out_len=np.array([out_len], np.int64))


# every combination for 'magphase'; the min-phase and linear branches differ from it in the phase rows only: once per rate
ORACLE_CASES = [(fs, cr, vw, "magphase") for fs in (48000, 16000) for cr in (False, True) for vw in (True, False)] + \
               [(fs, False, True, pt) for fs in (48000, 16000) for pt in ("min_phase", "linear")]


@pytest.mark.parametrize("fs,const_rate,voi_win,phase_type", ORACLE_CASES)
def test_model_against_the_oracle_type1(fs, const_rate, voi_win, phase_type):
    feats = _features(fs, 46, fs // 1000 + 2 * const_rate + voi_win)
    N = orc.define_fft_len(fs)
    # the noise length is known only after the oracle has placed its epochs: a first call with its own draw tells it
    np.random.seed(5)
    _, d0 = orc.synthesis_from_compressed(*feats, fs, b_voi_ap_win=voi_win, b_const_rate=const_rate,
                                          per_phase_type=phase_type, return_debug=True)
    noise = np.random.RandomState(9).uniform(-1, 1, d0["ns_len"])
    _, d = orc.synthesis_from_compressed(*feats, fs, b_voi_ap_win=voi_win, b_const_rate=const_rate,
                                         per_phase_type=phase_type, v_noise=noise, return_debug=True)
    v_voi = d["v_voi"]
    assert v_voi.any() and (~v_voi).any()
    m_real, m_imag = d["m_real"], d["m_imag"]
    if phase_type == "min_phase":
        mp_ = orc.build_min_phase_from_mag_spec(d["m_mag"])
        m_real, m_imag = mp_.real, mp_.imag
    elif phase_type == "linear":
        m_real, m_imag = np.ones_like(d["m_mag"]), np.zeros_like(d["m_mag"])
    inv_gain = np.where(v_voi, 1.0 / d["g_voi"], 1.0 / d["g_unv"])
    c = _case_from(N, d["v_shift"], d["v_pm"], v_voi, d["ns_len"], voi_win, noise, d["m_mag"], m_real, m_imag, inv_gain,
                   hm.synthesis_bin_curves(fs, N), False)
    X = np.array([scm.frame_spectrum(c, f)[0] for f in range(c.F)])
    ref = d["m_syn"]
    assert X.shape == ref.shape
    assert np.max(np.abs(X - ref)) <= TOL * np.max(np.abs(ref))
    out = scm.synthesis(c)
    assert out["pcm"].shape == d["v_pre_hpf"].shape
    assert np.max(np.abs(out["pcm"] - d["v_pre_hpf"])) <= TOL * np.max(np.abs(d["v_pre_hpf"]))
    # the norm really bounds the frames it is stated for
    assert np.all(np.abs(out["pcm"]) <= out["B"] * (1 + 1e-9))


@pytest.mark.parametrize("fs,rate,voi_win,hf", [(48000, -1.0, True, 1.0), (16000, 5.0, True, 2.0), (16000, -1.0, False, 0.5)])
def test_model_against_the_type2_model(fs, rate, voi_win, hf):
    mag, real, imag, lf0 = _features(fs, 40, 77 + fs // 1000)
    N = orc.define_fft_len(fs)
    half, alpha = N // 2 + 1, orc.define_alpha(fs)
    v_shift, v_pm, v_voi, v_locs, ns_len = t2s.frame_tables(lf0, fs, rate)
    noise = np.random.RandomState(3).uniform(-1, 1, ns_len)
    _, d = t2s.synthesis(mag, real, imag, lf0, fs, hf_slope_coeff=hf, b_voi_ap_win=voi_win, const_rate_ms=rate, v_noise=noise)
    m_mag = np.exp(orc.sp_mel_unwarp(mag, half, alpha=alpha, in_type="log"))
    m_real, m_imag = t2s.phase_unwarp(real, imag, mag.shape[1], half, alpha)
    if v_locs is not None:
        m_mag, m_real, m_imag = (orc.interp_from_const_to_variable_rate(x, v_locs, rate, fs) for x in (m_mag, m_real, m_imag))
    assert v_voi.any() and (~v_voi).any()
    c = _case_from(N, v_shift, v_pm, v_voi, ns_len, voi_win, noise, m_mag, m_real, m_imag,
                   np.full(v_pm.size, 1.0 / d["rms_spec"]), hm.type2_synthesis_bin_curves(fs, N, hf), True)
    out = scm.synthesis(c)
    assert out["pcm"].shape == d["v_pre_hpf"].shape
    assert np.max(np.abs(out["pcm"] - d["v_pre_hpf"])) <= TOL * np.max(np.abs(d["v_pre_hpf"]))
    # type 1 on the same operands differs: the DC / Nyquist rule is what the flag selects
    c.type2 = False
    assert np.max(np.abs(scm.synthesis(c)["pcm"] - d["v_pre_hpf"])) > 1e-6 * np.max(np.abs(d["v_pre_hpf"]))


def test_row_tables_are_the_oracles_interpolation():
    """x[row0] + (x[row1] - x[row0]) row_t on hostmath.const_to_variable_rows' tables is
    oracle.interp_from_const_to_variable_rate."""
    fs, rate, rows = 16000, 5.0, 30
    rs = np.random.RandomState(1)
    x = rs.randn(rows, 513)
    shift_c = orc.f0_to_shift(np.full(rows, 140.0), fs)
    _, v_locs = orc.get_shifts_and_frm_locs_from_const_shifts(shift_c, rate, fs)
    lo, hi, t, _ = hm.const_to_variable_rows(np.ones(rows, dtype=bool), v_locs, rate, fs)
    F = lo.size
    c = scm.Case(N=1024, mag=x, real=x, imag=x, row0=lo.astype(np.int32), row1=hi.astype(np.int32), row_t=t,
                 npos=np.zeros(F, np.int64))
    got = np.array([scm.frame_rows(c, f)[0] for f in range(F)])
    want = orc.interp_from_const_to_variable_rate(x, v_locs, rate, fs)
    assert got.shape == want.shape and np.max(np.abs(got - want)) <= 1e-12


@pytest.mark.parametrize("N", scm.FFT_LENS)
def test_read_set_and_the_columns_the_plan_fills(N):
    """The header's n_per_bins contract as a mask: whole 64-bin groups; the plan fills the leading
    hostmath.synth_comp_phase_columns(N, n_per) columns (the unwarp rounds that up to a multiple of 64), which cover it."""
    H, Q = N // 2 + 1, N // 4
    for n_per in range(0, H + 2):
        read = scm.phase_read_set(N, n_per)
        eff = scm.eff_n_per(n_per, N)
        assert read[:eff].all(), "every bin that can carry a periodic component is read"
        cols = hm.synth_comp_phase_columns(N, n_per)
        assert cols == (int(np.flatnonzero(read)[-1]) + 1 if read.any() else 0) <= H
        if eff <= Q + 1:
            assert cols == min((eff + 63) // 64 * 64, H)          # what the plan passed before: unchanged where it was right
        else:
            assert cols == min(Q + 1 + (eff - Q - 1 + 63) // 64 * 64, H)
    # the case the direct test exposed: n_per just above N/4 + 1 reads bin N/4 + 64, one past roundup64(n_per)
    read = scm.phase_read_set(N, Q + 2)
    assert read[Q + 64] and (Q + 2 + 63) // 64 * 64 == Q + 64 and hm.synth_comp_phase_columns(N, Q + 2) == Q + 65
    # every supported rate stays below N/4: the plan's column count is what it always was
    for fs in (16000, 48000):
        n = hm.define_fft_len(fs)
        for curves in (hm.synthesis_bin_curves(fs, n), hm.type2_synthesis_bin_curves(fs, n)):
            n_per = hm._first_all_zero_from(np.asarray(curves[0], dtype=np.float32))
            assert n_per <= n // 4 + 1 and hm.synth_comp_phase_columns(n, n_per) == (n_per + 63) // 64 * 64


def _entry_args(n_runs=7, n_slots=7, fft_len=4096, rows=(None, None, None), spectra=False):
    """Non-null host addresses for every pointer (never dereferenced: the entries return before any launch)."""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    args = [None, fft_len, p] + [p] * 10 + list(rows) + [p] * 7 + [n_runs, p, p, n_slots, p, p, 2112, 0]
    return (args + [p] if spectra else args), buf


def test_c_entries_reject_before_any_launch():
    lib = _lib.load()
    one = ctypes.addressof(ctypes.create_string_buffer(16))
    entries = ("mpx_synthesis_compressed_ola", "mpx_synthesis_compressed_type2_ola", "mpx_synthesis_compressed_ola_spectra")
    for name in entries:
        fn, spectra = getattr(lib, name), name.endswith("_spectra")
        # row tables given only in part
        for mask in range(1, 7):
            rows = tuple(one if mask >> i & 1 else None for i in range(3))
            args, keep = _entry_args(rows=rows, spectra=spectra)
            assert fn(*args) == -1, (name, mask)
            msg = lib.mpx_last_error()
            assert b"row0 / row1 / row_t must be given together" in msg and msg.startswith(name.encode()), msg
        # negative counts (before the null-pointer test: every pointer may be null)
        for n_runs, n_slots in ((-1, 7), (7, -1), (-3, -3)):
            args, keep = _entry_args(n_runs=n_runs, n_slots=n_slots, spectra=spectra)
            assert fn(*args) == -1 and b"negative count" in lib.mpx_last_error(), name
            assert fn(*([None, 4096] + [None] * 21 + [n_runs, None, None, n_slots, None, None, 2112, 0] + [None] * spectra)) == -1
        # nothing to do: no run or no slot
        for n_runs, n_slots in ((0, 7), (7, 0)):
            args, keep = _entry_args(n_runs=n_runs, n_slots=n_slots, spectra=spectra)
            assert fn(*args) == 0
    fn = lib.mpx_synthesis_compressed_ola_spectra
    for n in (1024, 2048):                                      # stored spectra exist at 4096 only
        args, keep = _entry_args(fft_len=n, spectra=True)
        assert fn(*args) == -1 and b"fft_len 4096 and one row per frame only" in lib.mpx_last_error()
    args, keep = _entry_args(rows=(one, one, one), spectra=True)   # ... and in the one-row form only
    assert fn(*args) == -1 and b"fft_len 4096 and one row per frame only" in lib.mpx_last_error()
    args, keep = _entry_args(spectra=True)
    args[-1] = None                                             # the spectra themselves missing
    assert fn(*args) == -1 and b"null pointer" in lib.mpx_last_error()
    assert lib.mpx_noise_stats_spectra(None, 2048, one, one, one, one, one, one, 3, one, one) == -1
    assert b"fft_len must be 4096" in lib.mpx_last_error()
    assert lib.mpx_noise_spectra_floats(2048, 5) == 0 and lib.mpx_noise_spectra_floats(4096, 5) == 5 * 17 * 64 * 4


def _all_cases():
    for N in scm.FFT_LENS:
        for lerp in (False, True):
            for type2 in (False, True):
                yield "single", scm.single_frame_case(N, lerp, type2, 0)
                yield "onehot", scm.one_hot_case(N, lerp, type2, 0)
                yield "onehot", scm.one_hot_case(N, lerp, type2, 200)
                yield "multi", scm.multi_frame_case(N, lerp, type2, 0)
        for type2 in (False, True):
            for n_per in scm.n_per_values(N):
                yield "n_per", scm.n_per_case(N, type2, n_per)
    for n_per in (449, 512, 513, 700):
        yield "single", scm.single_frame_case(4096, False, False, n_per)
        yield "multi", scm.multi_frame_case(4096, False, False, n_per)
        yield "onehot", scm.one_hot_case(4096, False, False, n_per)


def test_every_gpu_operand_set_is_self_consistent():
    kinds = {}
    for kind, c in _all_cases():
        assert scm.check_case(c), kind
        assert c.F <= 220
        kinds[kind] = kinds.get(kind, 0) + 1
        if kind == "single":
            shapes = set(zip(c.nleft.tolist(), c.nright.tolist()))
            assert shapes == set(scm.frame_shapes(c.N))
            lens = {L + R + 1 for L, R in shapes}
            assert set(scm.tile_lengths(c.N)) <= lens and any(L == 0 for L, _ in shapes) and any(R == 0 for _, R in shapes)
            wls, wrs = scm.win_values(c.N)
            for v in (0, 1):                       # every window value on both sides, for voiced and unvoiced frames
                assert set(c.win_l[c.voiced == v].tolist()) == set(wls) and set(c.win_r[c.voiced == v].tolist()) == set(wrs)
            for w in (0, 1):
                assert {0, 1} == set(c.voiced[c.wtype == w].tolist())
            assert c.inv_gain.max() / c.inv_gain.min() > 500
            m = c.mag[np.isfinite(c.mag).all(axis=1)]
            assert (m.max(axis=1) / m.min(axis=1)).min() > 1e5          # 120 dB across the bins of every row
            if c.lerp():
                t = c.row_t
                assert (t == 0).any() and (t == 1).any() and ((t > 0.1) & (t < 0.9)).any()
                assert ((c.row0 == c.row1) & (t != 0)).any() and (c.row0 != c.row1).any()
            else:
                v = c.voiced == 1
                assert ((c.real[v] == 0) & (c.imag[v] == 0)).any()
        if kind == "multi":
            per_run = [len(r) for r in c.pm_rel]
            assert min(per_run) == 1 and max(per_run) > 40
    assert set(kinds) == {"single", "onehot", "multi", "n_per"}


def test_the_model_honours_the_documented_rules():
    """Small hand cases: DC / Nyquist under both types, a == b == 0, n_per, the window's placement."""
    N, H = 1024, 513
    rs = np.random.RandomState(0)
    noise = rs.uniform(-1, 1, 400).astype(np.float32)
    base = dict(N=N, noise=noise, npos=np.array([200], np.int64), nleft=np.array([50], np.int32),
                nright=np.array([60], np.int32), wtype=np.array([0], np.int32), voiced=np.array([1], np.int32),
                inv_gain=np.array([0.5], np.float32), win_l=np.array([3], np.int32), win_r=np.array([0], np.int32),
                per_v=np.ones(H, np.float32), ap_v=np.zeros(H, np.float32), ap_u=np.ones(H, np.float32),
                mag=np.ones((1, H), np.float32), real=-np.ones((1, H), np.float32), imag=np.zeros((1, H), np.float32),
                pm_rel=[np.zeros(1, np.int64)], out_start=np.zeros(1, np.int32), out_len=np.array([N], np.int64))
    X1 = scm.frame_spectrum(scm.Case(**base), 0)[0]
    X2 = scm.frame_spectrum(scm.Case(type2=True, **base), 0)[0]
    assert X1[0] == 1 and X1[-1] == 1 and X2[0] == -1 and X2[-1] == -1 and np.all(X1[1:-1] == -1)
    c = scm.Case(n_per_bins=100, **base)
    X = scm.frame_spectrum(c, 0)[0]
    assert np.all(X[:100] != 0) and not X[100:].any()
    c = scm.Case(**base)
    c.real = c.real.copy()
    c.real[0, 7] = 0.0
    assert scm.frame_spectrum(c, 0)[0][7] == 0
    y, B, _, sup = scm.frame(scm.Case(**base), 0)
    assert np.flatnonzero(sup).tolist() == [509, 510, 511, 512] and not y[:510].any() and not y[513:].any()
    assert y[512] != 0 and B[512] > 0 and B[509] == 0
    c = scm.Case(**dict(base, voiced=np.array([0], np.int32)))
    Xu = scm.frame_spectrum(c, 0)[0]
    Ns, l1 = scm.noise_spectrum(noise, 200, 50, 60, 0, N)
    assert np.allclose(Xu[1:-1], 0.5 * Ns[1:-1], rtol=1e-15, atol=0) and l1 > 0
