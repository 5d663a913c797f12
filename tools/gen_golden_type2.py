"""
TEST INFRASTRUCTURE ONLY -- writes tests/golden/g16_type2.npz from the REAL reference's analysis_lossless_type2
(magphase.py:2793-2866) and analysis_compressed_type2 (:3123-3196), imported in memory through oracle/ref_shim.py
(epochs registered with set_epochs, wavs written with the shim's 16-bit writer):

    python tools/gen_golden_type2.py

Utterances (magphase_amd.synthetic, edited): at 48 kHz and 16 kHz, "a" has its first epoch later than fft_len samples,
an unvoiced gap whose two-period frame (and one-period frame) exceeds fft_len, and an all-zero stretch (zero gains,
all-NaN envelope rows: lossless only); "b" has an epoch count of the other parity and only finite features (compressed
cases: variable rate, 5 ms and 4 ms, b_norm_mag off and on).  Stored: the inputs, every STEP-th bin of the lossless
matrices (envelope in dB), the full f0 / shift / gain vectors, the reference's envelope passes per frame (its
spectral_smoothing_rceps calls, counted per row), the compressed matrices and the lf0 / lgain vectors.  The SPTK leg of
format_for_modelling is the oracle's restatement (ref_shim), as for G8: parity of that leg is unpinned (pinned = 0).
"""
import os
import sys
import tempfile
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402
from magphase_amd import synthetic as syn  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g16_type2.npz")
STEP = {48000: 16, 16000: 8}
# (tag, fs, synthetic utterance, duration, first epoch at or after, gap (start, end) or None, zero stretch or None)
UTTS = (("48k_a", 48000, 21, 0.5, 0.1, (0.22, 0.31), (0.38, 0.44)),
        ("48k_b", 48000, 22, 0.45, 0.0, None, None),
        ("16k_a", 16000, 23, 0.6, 0.15, (0.3, 0.45), (0.48, 0.53)),
        ("16k_b", 16000, 24, 0.45, 0.0, None, None))
COMP = ((-1.0, False), (-1.0, True), (5.0, False), (5.0, True), (4.0, False))


def utterance(fs, u, dur, t_first, gap, zero):
    pcm, pm, voi = syn.make_utterance(u, dur_s=dur, fs=fs)
    keep = pm >= t_first
    if gap is not None:
        keep &= ~((pm > gap[0]) & (pm < gap[1]))
    pm, voi = pm[keep], voi[keep].copy()
    if gap is not None:   # the epochs on both sides of the gap are unvoiced
        j = int(np.searchsorted(pm, gap[0]))
        voi[max(j - 1, 0):j + 1] = 0.0
    if zero is not None:
        pcm = pcm.copy()
        pcm[int(zero[0] * fs):int(zero[1] * fs)] = 0
    return pcm, pm, voi


def main():
    mp, la, _ = ref_shim.load_reference()
    orig_te = la.true_envelope
    orig_sm = la.spectral_smoothing_rceps
    passes = []

    def counted_te(m_sp, **kw):   # the reference's loop is per row: count its smoothing calls row by row
        count = [0]

        def counted(*a, **k):
            count[0] += 1
            return orig_sm(*a, **k)

        la.spectral_smoothing_rceps = counted
        rows, it = [], []
        try:
            for f in range(m_sp.shape[0]):
                count[0] = 0
                with np.errstate(divide="ignore", invalid="ignore"):
                    rows.append(orig_te(m_sp[f:f + 1].copy(), **kw)[0])
                it.append(count[0])
        finally:
            la.spectral_smoothing_rceps = orig_sm
        passes.append(np.asarray(it, dtype=np.int32))
        return np.array(rows).reshape(m_sp.shape)

    la.true_envelope = counted_te
    d = {"tags": np.asarray([u[0] for u in UTTS]), "pinned": np.int64(0),
         "comp_cases": np.asarray([[r, float(b)] for r, b in COMP])}
    tmp = tempfile.mkdtemp()
    try:
        for tag, fs, u, dur, t_first, gap, zero in UTTS:
            pcm, pm, voi = utterance(fs, u, dur, t_first, gap, zero)
            wav = os.path.join(tmp, "g16_%s.wav" % tag)
            ref_shim._wav_write(wav, pcm / 32768.0, fs)
            ref_shim.set_epochs(wav, pm, voi)
            step = STEP[fs]
            passes.clear()
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter("always")
                m_env, m_real, m_imag, v_f0, fs_o, v_shift, v_gain = mp.analysis_lossless_type2(wav)
            with np.errstate(divide="ignore", invalid="ignore"):
                env_db = 20.0 * np.log10(m_env)
            d.update({tag + "_fs": np.int64(fs), tag + "_pcm": pcm, tag + "_pm_sec": pm, tag + "_voi": voi,
                      tag + "_step": np.int64(step), tag + "_env_db": env_db[:, ::step].astype(np.float32),
                      tag + "_real": m_real[:, ::step].astype(np.float32),
                      tag + "_imag": m_imag[:, ::step].astype(np.float32), tag + "_f0": np.asarray(v_f0, np.float64),
                      tag + "_shift": np.asarray(v_shift, np.float64), tag + "_gain": np.asarray(v_gain, np.float64),
                      tag + "_passes": passes[0].copy(), tag + "_n_warn": np.int64(len(w))})
            print("%s: %d epochs, %d rows, %d NaN rows, %d warnings, passes %.1f per frame"
                  % (tag, pm.size, m_env.shape[0], int(np.isnan(m_env).all(axis=1).sum()), len(w), passes[0].mean()))
            if tag.endswith("_b"):
                for k, (rate, norm) in enumerate(COMP):
                    with warnings.catch_warnings():
                        warnings.simplefilter("ignore")
                        r = mp.analysis_compressed_type2(wav, mag_dim=60, phase_dim=45, b_norm_mag=norm,
                                                         const_rate_ms=rate)
                    key = "%s_c%d" % (tag, k)
                    for name, x in zip(("mag", "real", "imag", "lf0", "shift"), r[:5]):
                        d[key + "_" + name] = np.asarray(x, dtype=np.float32 if name in ("mag", "real", "imag") else np.float64)
                    d[key + "_fft_len"] = np.int64(r[6])
                    d[key + "_lgain"] = np.asarray(r[7], dtype=np.float64)
                    assert np.all(np.isfinite(r[0])), key
                    print("  %s: rate %g, b_norm_mag %s: %d rows" % (key, rate, norm, r[0].shape[0]))
            os.remove(wav)
    finally:
        la.true_envelope = orig_te
        os.rmdir(tmp)
    np.savez_compressed(OUT, **d)
    print("wrote %s (%.0f KB)" % (OUT, os.path.getsize(OUT) / 1024))


if __name__ == "__main__":
    main()
