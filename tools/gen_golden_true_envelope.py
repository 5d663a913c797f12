"""
TEST INFRASTRUCTURE ONLY -- writes tests/golden/g15_true_envelope.npz from the REAL reference's la.true_envelope
(libaudio.py:295-340), la.spectral_smoothing_rceps (:203-238), la.rceps (:252-270) and la.rceps_to_min_phase_rceps
(:190-197), imported in memory through oracle/ref_shim.py:

    python tools/gen_golden_true_envelope.py

Inputs: lossless magnitudes of short synthetic utterances (magphase_amd.synthetic -> the oracle's lossless analysis) at
8 kHz (fft_len 1024), 16 kHz (2048) and 48 kHz (4096), rounded to float32 (what the device reads) and stored so.
true_envelope cases (tag_intype_ncoeffs_thres): the envelope in dB (20 log10 for 'abs', (20 / ln 10) x for 'log'), float64
at every 4th bin, and the reference's passes per frame (calls of spectral_smoothing_rceps, counted by wrapping it while the
reference runs one frame at a time).  The 16 kHz 'zero' case has one zero bin in row 2.  Also: spectral_smoothing_rceps
of the 16 kHz log magnitudes at two fade_to_total values (every 4th bin), rceps in each in_type / out_type mode and
rceps_to_min_phase_rceps (full rows).  Prints the reference's time per frame (one CPU core): the probe's baseline.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import magphase_oracle as orc  # noqa: E402
from oracle import ref_shim  # noqa: E402
from magphase_amd import synthetic as syn  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g15_true_envelope.npz")
STEP = 4   # bins kept of each output row
# (tag, fs, frames, [(in_type, ncoeffs, thres_db), ...])
SETS = (("8k", 8000, 6, [("abs", 60, 0.1), ("abs", 600, 0.1), ("log", 60, 0.1)]),
        ("16k", 16000, 6, [("abs", 60, 0.1), ("abs", 600, 0.1), ("abs", 1500, 0.1), ("log", 60, 0.0),
                           ("db", 600, 1e3)]),
        ("48k", 48000, 6, [("abs", 60, 0.1), ("abs", 600, 0.1), ("db", 60, 0.1), ("log", 600, 0.1), ("abs", 60, 1e3),
                           ("abs", 60, 0.0)]))


def magnitudes(fs, n_frames, u=5):
    pcm, pm_sec, voi = syn.make_utterance(u, dur_s=0.3, fs=fs)
    m_mag = orc.analysis_lossless_from_epochs(syn.pcm_to_float(pcm), fs, pm_sec, voi)[0]
    return m_mag[:n_frames].astype(np.float32).astype(np.float64)


def to_input(m_mag, in_type):
    if in_type == "abs":
        return m_mag
    if in_type == "log":
        return np.log(m_mag)
    return 20.0 * np.log10(m_mag)


def to_db(y, in_type):
    if in_type == "abs":
        with np.errstate(invalid="ignore", divide="ignore"):
            return 20.0 * np.log10(y)
    return (20.0 / np.log(10.0)) * y if in_type == "log" else y


def run_counted(la, x, **kw):
    """la.true_envelope one frame at a time: (output rows, passes per frame, seconds)."""
    orig = la.spectral_smoothing_rceps
    count = [0]

    def counted(*a, **k):
        count[0] += 1
        return orig(*a, **k)

    la.spectral_smoothing_rceps = counted
    rows, iters = [], []
    t0 = time.perf_counter()
    try:
        for f in range(x.shape[0]):
            count[0] = 0
            with np.errstate(divide="ignore", invalid="ignore"):
                rows.append(la.true_envelope(x[f:f + 1].copy(), **kw)[0])
            iters.append(count[0])
    finally:
        la.spectral_smoothing_rceps = orig
    return np.array(rows), np.array(iters, dtype=np.int32), time.perf_counter() - t0


def main():
    _mp, la, _lu = ref_shim.load_reference()
    d = {"step": np.int64(STEP)}
    cases = []
    for tag, fs, nf, todo in SETS:
        m = magnitudes(fs, nf)
        d[tag + "_mag"] = m.astype(np.float32)
        for in_type, nc, thres in todo:
            key = "%s_%s_%d_%g" % (tag, in_type, nc, thres)
            x = to_input(m, in_type)
            y, iters, sec = run_counted(la, x, in_type=in_type, ncoeffs=nc, thres_db=thres)
            d[key + "_env_db"] = to_db(y, in_type)[:, ::STEP]
            d[key + "_iters"] = iters
            cases.append(key)
            print("%-22s passes %3d..%3d  %.2f ms per frame" % (key, iters.min(), iters.max(), 1e3 * sec / nf))
    # a zero bin: the whole row is NaN in the reference, the other rows are unaffected
    mz = d["16k_mag"].astype(np.float64).copy()
    mz[2, 100] = 0.0
    d["16k_zero_mag"] = mz.astype(np.float32)
    y, iters, _ = run_counted(la, mz, in_type="abs", ncoeffs=60, thres_db=0.1)
    d["16k_zero_env_db"], d["16k_zero_iters"] = to_db(y, "abs")[:, ::STEP], iters
    # spectral_smoothing_rceps on log magnitudes
    lg = np.log(d["16k_mag"].astype(np.float64))
    for nc, fade in ((60, 0.2), (600, 0.7)):
        d["smooth_%d_%g" % (nc, fade)] = la.spectral_smoothing_rceps(lg.copy(), nc_total=nc, fade_to_total=fade)[:, ::STEP]
    # rceps in each mode, rceps_to_min_phase_rceps
    m8 = d["8k_mag"].astype(np.float64)[:2]
    m8[0, 7] = 0.0   # the protected log's floor ('abs')
    d["rceps_in"] = m8
    for in_type in ("abs", "log"):
        x = m8 if in_type == "abs" else np.log(m8 + 1e-3)
        for out_type in ("compact", "whole"):
            with np.errstate(divide="ignore"):
                d["rceps_%s_%s" % (in_type, out_type)] = la.rceps(x.copy(), in_type=in_type, out_type=out_type)
    c = np.random.RandomState(15).randn(3, 16)
    d["minph_in"] = c.copy()
    d["minph_out"] = la.rceps_to_min_phase_rceps(c)
    d["minph_in_after"] = c
    # time per frame at 48 kHz, ncoeffs 60 and 600, thres_db 0.1 (the probe's CPU baseline)
    m48 = magnitudes(48000, 40, u=7)
    for nc in (60, 600):
        _, it, sec = run_counted(la, m48, in_type="abs", ncoeffs=nc, thres_db=0.1)
        d["ref_ms_per_frame_48k_%d" % nc] = np.float64(1e3 * sec / m48.shape[0])
        d["ref_mean_passes_48k_%d" % nc] = np.float64(it.mean())
        print("reference, 48 kHz, ncoeffs %d: %.2f ms per frame, %.1f passes per frame (one CPU core)"
              % (nc, 1e3 * sec / m48.shape[0], it.mean()))
    d["cases"] = np.asarray(cases)
    np.savez_compressed(OUT, **d)
    print("wrote %s (%d cases, %.0f KB)" % (OUT, len(cases), os.path.getsize(OUT) / 1024))


if __name__ == "__main__":
    main()
