"""
TEST INFRASTRUCTURE ONLY -- writes tests/golden/g14_const_rate_lossless.npz from the REAL reference (imported in memory
through oracle/ref_shim.py):

    python tools/gen_golden_const_rate_lossless.py

Inputs: three short synthetic utterances (magphase_amd.synthetic): "16k" (fft_len 1024, voiced and unvoiced stretches,
205-222 Hz), "16k_low" (108-126 Hz) and "48k" (4096, 163-174 Hz).  Per
utterance, the reference's analysis_lossless (magphase.py:2869-2906) on the wav with the epochs registered, then the
constant-rate block of analysis_compressed (:2967-2980) at 5 ms: every row of mag / real / imag at every COL_STEP-th
bin, the last bin included (float32), and f0 (float64) -- whole float32 rows would make the file 1.8 MB.  The synthesis
below runs on the reference's full float64 rows; a test feeds the oracle's rows of the stored utterance, which
equal these at the stored columns.  Synthesis: the reference's composition from the 5 ms rows (f0_to_shift :2210,
get_shifts_and_frm_locs_from_const_shifts :1426, interp_from_const_to_variable_rate :2242 of the rows and of the
voicing > 0.5, shift_to_f0 :2198 with b_smooth=False, synthesis_from_lossless :1759) at 5 ms and, for the two
utterances whose f0 stays under 200 Hz, time-stretched at 10 ms; with the frame locations and shifts.  Every scan stays
under the reference's 2n-slot cap (asserted here: above 200 Hz -- or unvoiced, 5 ms -- a 10 ms scan reaches it).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402
from magphase_amd import synthetic as syn  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g14_const_rate_lossless.npz")
# (tag, fs, synthetic utterance, seconds, synthesis frame periods in ms)
UTTS = (("16k", 16000, 7, 0.2, (5.0,)), ("16k_low", 16000, 2, 0.2, (5.0, 10.0)), ("48k", 48000, 6, 0.15, (5.0, 10.0)))
CR = 5.0
COL_STEP = 8   # stored bins 0, 8, ..., H - 1 (H - 1 = fft_len / 2 is a multiple of 8)


def const_rate(mp, la, m_mag, m_real, m_imag, v_f0, v_shift, fs, cr):
    """magphase.py:2967-2980 with the reference's own functions (const_rate_ms = cr)."""
    v_pm = la.shift_to_pm(v_shift)
    rows = [mp.interp_from_variable_to_const_frm_rate(m, v_pm, cr, fs) for m in (m_mag, m_real, m_imag)]
    v_voi = v_f0 > 1.0
    v_f0_c = mp.interp_from_variable_to_const_frm_rate(
        np.r_[v_f0[v_voi][0], v_f0[v_voi], v_f0[v_voi][-1]], np.r_[0, v_pm[v_voi], v_pm[-1]], cr, fs).squeeze()
    v_voi_c = mp.interp_from_variable_to_const_frm_rate(v_voi, v_pm, cr, fs).squeeze() > 0.5
    return rows + [v_f0_c * v_voi_c]


def synthesis(mp, m_mag_c, m_real_c, m_imag_c, v_f0_c, fs, cr):
    """The reference's constant -> variable rate composition followed by synthesis_from_lossless."""
    v_shift_c = mp.f0_to_shift(v_f0_c, fs)
    v_shift, v_locs = mp.get_shifts_and_frm_locs_from_const_shifts(v_shift_c, cr, fs, interp_type="linear")
    n = np.size(v_f0_c)
    assert v_shift.size < 2 * n, "the scan reached the reference's 2n-slot cap: choose another f0 range"
    rows = [mp.interp_from_const_to_variable_rate(m, v_locs, cr, fs) for m in (m_mag_c, m_real_c, m_imag_c)]
    v_voi = mp.interp_from_const_to_variable_rate(v_f0_c > 1.0, v_locs, cr, fs) > 0.5
    v_f0 = mp.shift_to_f0(v_shift, v_voi, fs, b_smooth=False)
    v_syn = mp.synthesis_from_lossless(rows[0], rows[1], rows[2], v_f0, fs)
    return np.asarray(v_syn, dtype=np.float64), v_shift, v_locs


def main():
    mp, la, _ = ref_shim.load_reference()
    d = {"const_rate_ms": np.float64(CR), "tags": np.asarray([u[0] for u in UTTS]), "col_step": np.int64(COL_STEP)}
    for tag, fs, u, dur, rates in UTTS:
        pcm, pm_sec, voi = syn.make_utterance(u, dur_s=dur, fs=fs)
        wav = os.path.abspath("g14_%s.wav" % tag)
        ref_shim._wav_write(wav, pcm / 32768.0, fs)
        ref_shim.set_epochs(wav, pm_sec, voi)
        try:
            m_mag, m_real, m_imag, v_f0, fs_out, v_shift = mp.analysis_lossless(wav)
        finally:
            os.remove(wav)
        mag_c, real_c, imag_c, f0_c = const_rate(mp, la, m_mag, m_real, m_imag, v_f0, v_shift, fs, CR)
        d.update({tag + "_fs": np.int64(fs), tag + "_pcm": pcm, tag + "_pm_sec": pm_sec, tag + "_voi": voi,
                  tag + "_mag": mag_c[:, ::COL_STEP].astype(np.float32),
                  tag + "_real": real_c[:, ::COL_STEP].astype(np.float32),
                  tag + "_imag": imag_c[:, ::COL_STEP].astype(np.float32), tag + "_f0": np.asarray(f0_c, dtype=np.float64)})
        d[tag + "_rates"] = np.asarray(rates)
        for rate in rates:   # 10 ms: the 5 ms rows time-stretched by two
            v_syn, v_sh, v_locs = synthesis(mp, mag_c, real_c, imag_c, f0_c, fs, rate)
            key = "%s_syn%g" % (tag, rate)
            d[key], d[key + "_shift"], d[key + "_locs"] = v_syn, v_sh, v_locs
    np.savez_compressed(OUT, **d)
    print("wrote %s (%.0f KB)" % (OUT, os.path.getsize(OUT) / 1024))


if __name__ == "__main__":
    main()
