"""
TEST INFRASTRUCTURE ONLY -- writes tests/golden/g17_type2_synthesis.npz from the REAL reference's
synthesis_from_compressed_type2 (magphase.py:1452-1606), imported in memory through oracle/ref_shim.py:

    python tools/gen_golden_type2_synthesis.py

Inputs are the compressed type-2 rows of tests/golden/g16_type2.npz (utterances "48k_b" and "16k_b", cases c0 = variable
rate, c2 = 5 ms, c4 = 4 ms); they are read from g16 at test time, not stored twice.  Cases, each with a seed of its own
for numpy's global generator: both sample rates x (variable rate, 5 ms, 4 ms); at 16 kHz only: hf_slope_coeff = 2,
b_voi_ap_win off, fft_len 4096 and 1024 given explicitly.  b_norm_mag=True with a v_lgain is run too and must give the
plain case's signal bit for bit (the reference ignores both): asserted here, stored as a flag only.
Stored per case: the float64 signal, rms_noise and the frame count (read off la.remove_hermitian_half's argument) and the
number of voiced frames (the row count la.spectral_crossfade is first called with).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402

G16 = os.path.join(ROOT, "tests", "golden", "g16_type2.npz")
OUT = os.path.join(ROOT, "tests", "golden", "g17_type2_synthesis.npz")
RATE_CASE = {-1.0: 0, 5.0: 2, 4.0: 4}   # const_rate_ms -> g16's compressed case (b_norm_mag off)
# (name, g16 utterance, const_rate_ms, keyword arguments)
CASES = (("48k_var", "48k_b", -1.0, {}),
         ("48k_5ms", "48k_b", 5.0, {}),
         ("48k_4ms", "48k_b", 4.0, {}),
         ("16k_var", "16k_b", -1.0, {}),
         ("16k_5ms", "16k_b", 5.0, {}),
         ("16k_4ms", "16k_b", 4.0, {}),
         ("16k_hf2", "16k_b", -1.0, {"hf_slope_coeff": 2.0}),
         ("16k_nowin", "16k_b", -1.0, {"b_voi_ap_win": False}),
         ("16k_n4096", "16k_b", -1.0, {"fft_len": 4096}),
         ("16k_n1024", "16k_b", -1.0, {"fft_len": 1024}))
SEED0 = 5


def g16_inputs(g, utt, rate):
    key = "%s_c%d" % (utt, RATE_CASE[float(rate)])
    return tuple(np.asarray(g[key + "_" + n], dtype=np.float64) for n in ("mag", "real", "imag", "lf0"))


def main():
    mp, la, _ = ref_shim.load_reference()
    g = np.load(G16)
    seen = {}
    orig_rhh, orig_cf = la.remove_hermitian_half, la.spectral_crossfade

    def spy_rhh(m):
        r = orig_rhh(m)
        seen["ns"] = r
        return r

    def spy_cf(l, r, *a, **k):
        seen.setdefault("n_voiced", int(l.shape[0]))
        return orig_cf(l, r, *a, **k)

    def run(utt, rate, seed, **kw):
        mag, real, imag, lf0 = g16_inputs(g, utt, rate)
        fs = int(g[utt + "_fs"])
        seen.clear()
        np.random.seed(seed)
        la.remove_hermitian_half, la.spectral_crossfade = spy_rhh, spy_cf
        try:
            sig = mp.synthesis_from_compressed_type2(mag.copy(), real.copy(), imag.copy(), lf0.copy(), fs,
                                                     const_rate_ms=rate, **kw)
        finally:
            la.remove_hermitian_half, la.spectral_crossfade = orig_rhh, orig_cf
        ns = seen["ns"]
        return np.asarray(sig, dtype=np.float64), float(np.sqrt(np.mean(np.absolute(ns) ** 2))), ns.shape[0], seen["n_voiced"]

    d = {"names": np.asarray([c[0] for c in CASES]), "utts": np.asarray([c[1] for c in CASES]),
         "rates": np.asarray([c[2] for c in CASES]), "seeds": np.asarray([SEED0 + i for i in range(len(CASES))])}
    for i, (name, utt, rate, kw) in enumerate(CASES):
        sig, rms, nfrm, nvoi = run(utt, rate, SEED0 + i, **kw)
        assert np.all(np.isfinite(sig)), name
        assert nvoi >= 10 and nfrm - nvoi >= 10, (name, nfrm, nvoi)
        d.update({name + "_sig": sig, name + "_rms": np.float64(rms), name + "_nfrm": np.int64(nfrm),
                  name + "_nvoi": np.int64(nvoi), name + "_hf_slope": np.float64(kw.get("hf_slope_coeff", 1.0)),
                  name + "_voi_ap_win": np.int64(kw.get("b_voi_ap_win", True)),
                  name + "_fft_len": np.int64(kw.get("fft_len", 0))})
        print("%s: %d samples, peak %.3f, rms_noise %.6f, %d frames (%d voiced)"
              % (name, sig.size, np.max(np.abs(sig)), rms, nfrm, nvoi))
    # b_norm_mag / v_lgain are dead arguments of the reference: the same seed gives the plain case's signal
    j = [c[0] for c in CASES].index("16k_var")
    lgain = np.asarray(g["16k_b_c1_lgain"], dtype=np.float64)
    sig_n = run("16k_b", -1.0, SEED0 + j, b_norm_mag=True, v_lgain=lgain)[0]
    assert np.array_equal(sig_n, d["16k_var_sig"]), "b_norm_mag / v_lgain changed the reference's signal"
    d["norm_mag_equals"] = np.asarray("16k_var")
    np.savez_compressed(OUT, **d)
    print("wrote %s (%.0f KB)" % (OUT, os.path.getsize(OUT) / 1024))


if __name__ == "__main__":
    main()
