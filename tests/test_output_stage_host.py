"""
CPU: the references of the output-stage kernel tests (tests/output_stage_model.py) against what the rest of the suite
already trusts, and the figures the GPU tolerances of tests/test_gpu_output_stage.py are judged against.

  hpf_blocked vs hpf_cascade   the error the blocked scan itself owns, per (design, fs, input): printed and recorded
                               (_tol.note); a device figure more than 10 x its row is a finding, not a tolerance
  hpf_cascade vs lfilter b, a  the direct-form lfilter of magphase._output_hpf (and the elliptic b, a) stays within the old
                               1e-6 -- and is printed: it is 1e-8 .. 1e-6 of round-off noise, the reason the old reference
                               could not hold a tighter bound
  hpf_tables                   G = the impulse response of the state recursion, pmat = G continued to n = block, entries
                               below 120 (what magphase_output.hip's comment promises)
  merlin_stages vs the oracle  at the dims, rates and pf_coef the GPU tests launch
  pcm16 vs la.write_audio_file read back with the wave module: normal, norm=None, over-range, silent, every exact tie
"""
import wave

import numpy as np
import pytest

import output_stage_model as osm
from _tol import note, within
from magphase_amd import hostmath as hm
from magphase_amd import libaudio as la
from magphase_amd import magphase as mp
from oracle import magphase_oracle as orc

LD = osm.LD


# ---------------------------------------------------------------------------------------------------------------------
# high-pass
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("design", hm.HPF_DESIGNS)
@pytest.mark.parametrize("fs", osm.HPF_HOST_FS)
def test_blocked_scan_against_the_longdouble_cascade(design, fs):
    """The algorithm of mpx_output_hpf in float64 against the longdouble cascade, on every batch the GPU tests launch.
    Of the input's peak (1).  The bound: every block hands its state over through P, and the hand-over's float64 rounding
    comes back multiplied by the free response, both at most T = the tables' largest entry -- 2^-53 T^2 per block, summed
    over the longest utterance's 193 blocks without crediting the decay, for the two sections."""
    sos, pm, g = hm.hpf_tables(fs, osm.HPF_BLOCK, design)
    t_max = max(float(np.max(np.abs(pm))), float(np.max(np.abs(g))))
    bound = 2.0 ** -53 * t_max ** 2 * ((max(osm.HPF_LENS) + osm.HPF_BLOCK - 1) // osm.HPF_BLOCK) * 2
    print("hpf_blocked bound %s fs %d: %.3g (T = %.4g)" % (design, fs, bound, t_max))
    for name in osm.HPF_INPUTS:
        sigs, refs = osm.hpf_reference(design, fs, name)
        worst = 0.0
        for x, ref in zip(sigs, refs):
            y = osm.hpf_blocked(sos, pm, g, x)
            assert y.shape == x.shape and y.dtype == np.float64
            if x.size:
                worst = max(worst, float(np.max(np.abs(y.astype(LD) - ref))))
        print("hpf_blocked vs hpf_cascade %s fs %d %-12s %.3g" % (design, fs, name, worst))
        note("OS_HPF_BLOCKED_F64/%s/%d/%s" % (design, fs, name), worst)
        within(worst, bound, "OS_HPF_BLOCKED_F64_%s_%d" % (design, fs))


def test_cascade_loop_and_lfilter_forms_agree():
    """hpf_cascade's fast path (lfilter on longdouble arrays) against the plain loop in the kernel's operation order."""
    for design, fs in (("butter40", 48000), ("ellip60", 8000)):
        sos = hm.hpf_tables(fs, osm.HPF_BLOCK, design)[0]
        x = osm.hpf_input("dc_noise", design, fs, lens=(3000,))[0]
        a, b = osm.hpf_cascade(sos, x), osm.hpf_cascade(sos, x, loop=True)
        assert a.dtype == b.dtype == np.dtype(LD)
        assert float(np.max(np.abs(a - b))) <= 1e-15


@pytest.mark.parametrize("design", hm.HPF_DESIGNS)
@pytest.mark.parametrize("fs", osm.HPF_HOST_FS)
def test_direct_form_lfilter_is_the_noisy_side(design, fs):
    """scipy's lfilter in b, a form (magphase._output_hpf; for the elliptic design the same call with ellip's b, a) against
    the longdouble cascade: within the 1e-6 the old device test allows, but orders of magnitude above the blocked scan."""
    from scipy import signal
    sos = hm.hpf_tables(fs, osm.HPF_BLOCK, design)[0]
    if design == "ellip60":
        b_, a_ = signal.ellip(4, 0.5, 80, 60 / (fs / 2.0), btype="highpass")
    for name in ("noise", "dc", "corner_sine"):
        x = osm.hpf_input(name, design, fs, lens=(3000,))[0].astype(np.float64)
        ref = osm.hpf_cascade(sos, x)
        y = mp._output_hpf(x, fs) if design == "butter40" else signal.lfilter(b_, a_, x)
        d = float(np.max(np.abs(y.astype(LD) - ref)))
        print("lfilter b, a vs hpf_cascade %s fs %d %-12s %.3g" % (design, fs, name, d))
        note("OS_HPF_LFILTER_BA/%s/%d/%s" % (design, fs, name), d)
        within(d, 1e-6, "OS_HPF_LFILTER_BA_%s" % design)


@pytest.mark.parametrize("design", hm.HPF_DESIGNS)
@pytest.mark.parametrize("fs", osm.HPF_HOST_FS)
def test_hpf_tables_are_the_state_recursion(design, fs):
    block = osm.HPF_BLOCK
    sos, pm, g = hm.hpf_tables(fs, block, design)
    assert sos.shape == (2, 6) and pm.shape == (2, 4) and g.shape == (2, block, 2)
    for sec in range(2):
        a1, a2 = LD(sos[sec, 4]) / LD(sos[sec, 3]), LD(sos[sec, 5]) / LD(sos[sec, 3])
        # the free response: y[n] of the section with x = 0 from z = (1, 0) and from z = (0, 1); one step further, the state
        # itself after `block` samples = A^block
        for col, z in enumerate(((LD(1), LD(0)), (LD(0), LD(1)))):
            z0, z1 = z
            resp = np.empty(block, dtype=LD)
            for n in range(block):
                y = z0
                resp[n] = y
                z0, z1 = z1 - a1 * y, -a2 * y
            scale = max(1.0, float(np.max(np.abs(resp))))
            assert float(np.max(np.abs(g[sec, :, col].astype(LD) - resp))) <= 1e-12 * scale, (design, fs, sec, col)
            # column `col` of A^block = the state reached from the unit state e_col
            assert abs(float(LD(pm[sec, col]) - z0)) <= 1e-12 * scale and abs(float(LD(pm[sec, 2 + col]) - z1)) <= 1e-12 * scale
        # "G continued": row `block` of [1, 0] A^n is pmat's first row
        cont = g[sec, block - 1] @ np.array([[-float(a1), 1.0], [-float(a2), 0.0]])
        assert np.max(np.abs(cont - pm[sec, :2])) <= 1e-12 * max(1.0, np.max(np.abs(pm[sec])))
    big = max(float(np.max(np.abs(pm))), float(np.max(np.abs(g))))
    print("hpf_tables %s fs %d: largest |pmat|, |G| entry %.4g" % (design, fs, big))
    note("OS_HPF_TABLE_MAX/%s/%d" % (design, fs), big)
    assert big < 120.0


# ---------------------------------------------------------------------------------------------------------------------
# Merlin post-filter
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs", osm.MERLIN_FS)
@pytest.mark.parametrize("dim", osm.MERLIN_DIMS)
def test_merlin_stages_match_the_oracle(dim, fs):
    """merlin_stages (tables, float32 where the device stores float32) against the oracle's tool-by-tool chain, at the bound
    of test_host_form_matches_the_independent_oracle (one float32 flip of a pipe value)."""
    assert osm.MAGIC == la.MAGIC
    x = osm.merlin_input(dim)[osm.MERLIN_UNIQUE - 12:osm.MERLIN_UNIQUE]      # eight formant rows and the four silent ones
    for pf in (1.0, 1.4, 1.25):
        want = orc.post_filter_merlin(x, fs, pf_coef=pf)
        st = osm.merlin_stages(x, hm.merlin_tables(dim, fs, pf))
        assert st["out"].shape == want.shape and np.all(np.isfinite(st["out"]))
        d = float(np.max(np.abs(st["out"] - want)))
        print("merlin_stages vs oracle D %d fs %d pf %.2f: %.3g" % (dim, fs, pf, d))
        within(d, 2e-6, "OS_MERLIN_STAGES_VS_ORACLE")
        for k in ("mcep", "mcep_w", "mcep_pf"):
            assert st[k].shape == x.shape
        assert st["r0"].shape == st["p_r0"].shape == (x.shape[0],) and np.all(st["r0"] > 0) and np.all(st["p_r0"] > 0)


def test_merlin_stages_and_oracle_turn_bad_rows_into_magic():
    x = osm.merlin_input(24)[:6].copy()
    x[1, :] = np.nan
    x[4, 7] = -np.inf
    with np.errstate(all="ignore"):
        want = orc.post_filter_merlin(x, 48000)
        st = osm.merlin_stages(x, hm.merlin_tables(24, 48000))
    for out in (want, st["out"]):
        assert np.all(out[[1, 4]] == la.MAGIC) and np.all(np.isfinite(out))
    good = [0, 2, 3, 5]
    assert np.array_equal(want[good], orc.post_filter_merlin(x[good], 48000))


# ---------------------------------------------------------------------------------------------------------------------
# 16-bit PCM
# ---------------------------------------------------------------------------------------------------------------------
def _written(tmp_path, y, norm):
    path = str(tmp_path / "x.wav")
    with np.errstate(invalid="ignore", divide="ignore"):
        la.write_audio_file(path, y, 16000, norm=norm)
    with wave.open(path, "rb") as fh:
        assert fh.getsampwidth() == 2 and fh.getnchannels() == 1
        return np.frombuffer(fh.readframes(fh.getnframes()), dtype="<i2")


@pytest.mark.parametrize("norm", [0.98, None])
def test_pcm16_model_is_what_write_audio_file_stores(tmp_path, norm):
    rs = np.random.RandomState(4)
    over = rs.uniform(-3, 3, 5000)
    over[-1] = -3.5
    cases = {"normal": rs.uniform(-0.7, 0.7, 5000), "over-range": over, "silent": np.zeros(300),
             "float32": rs.uniform(-1, 1, 777).astype(np.float32)}
    for what, y in cases.items():
        got = _written(tmp_path, y, norm)
        assert np.array_equal(got, osm.pcm16(y, norm)), (what, norm)
    assert np.all(_written(tmp_path, np.zeros(300), norm) == 0)          # silence is written as silence
    if norm is None:
        assert osm.pcm16(over, None).min() == -32768 and osm.pcm16(over, None).max() == 32767


def test_pcm16_exact_ties_round_half_to_even(tmp_path):
    k, y = osm.pcm16_ties()
    assert k.size == 65535 and np.array_equal(y * 32767.0, k + 0.5)     # exact ties, every one of them
    want = np.where(k % 2 == 0, k, k + 1)                              # the even neighbour of k + 0.5
    got = osm.pcm16(y, None)
    assert np.array_equal(got.astype(np.float64), want)
    assert np.array_equal(_written(tmp_path, y, None), got)


def test_pcm16_to_f32_model_is_exact():
    p = np.arange(-32768, 32768).astype(np.int16)
    f = osm.pcm16_to_f32(p)
    assert f.dtype == np.float32 and np.array_equal(f.astype(np.float64) * 32768.0, p.astype(np.float64))
