"""
TEST INFRASTRUCTURE ONLY -- writes tests/golden/g13_griffin_lim.npz from the REAL reference's griffin_lim
(magphase.py:3320-3372, imported in memory through oracle/ref_shim.py):

    python tools/gen_golden_griffin_lim.py

Inputs: magnitudes and shifts of short synthetic utterances (magphase_amd.synthetic -> the oracle's lossless analysis),
at 16 kHz (fft_len 1024) and 48 kHz (4096), with the first shift set to N/2 and one more to N/2 - 1 (the edges of the
reference's domain).  Cases: every phase_init ('random' with a fixed numpy seed) x niters in {1, 2, 5} at 16 kHz, and
every phase_init at niters 2 plus 'random' at 5 at 48 kHz.  Per case: v_sig float64 and, for 'random', numpy's RNG
position after the call; the phase (float32, to keep the file small) at niters 1 and 5; the ndarray init after the
16 kHz niters = 1 call (the reference zeroes its columns 0 and H - 1 in place).  The ndarray init itself is
2 pi (RandomState(seed + fs).rand(F, H) - 0.5) (ndarray_init below), not stored.
"""
import contextlib
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import magphase_oracle as orc  # noqa: E402
from oracle import ref_shim  # noqa: E402
from magphase_amd import synthetic as syn  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g13_griffin_lim.npz")
SEED = 1313
INITS = ("random", "linear", "min_phase", "ndarray")


def utterance(fs, n_frames, u):
    pcm, pm_sec, voi = syn.make_utterance(u, dur_s=0.3, fs=fs)
    m_mag, _, _, _, _, v_shift = orc.analysis_lossless_from_epochs(syn.pcm_to_float(pcm), fs, pm_sec, voi)
    N = 2 * (m_mag.shape[1] - 1)
    v_shift = v_shift[:n_frames].astype(np.float64) + 0.25   # fractional: round_to_int is part of the contract
    v_shift[0] = N // 2
    v_shift[n_frames // 2] = N // 2 - 1
    return m_mag[:n_frames], v_shift


def ndarray_init(shape, fs, seed=SEED):
    return 2 * np.pi * (np.random.RandomState(seed + fs).rand(*shape) - 0.5)


def main():
    mp = ref_shim.load_reference()[0]
    d = {"seed": np.int64(SEED)}
    cases = []
    for tag, fs, nf, niters_list in (("16k", 16000, 8, (1, 2, 5)), ("48k", 48000, 4, (2,))):
        m_mag, v_shift = utterance(fs, nf, 3)
        d[tag + "_mag"], d[tag + "_shift"] = m_mag, v_shift
        init = ndarray_init(m_mag.shape, fs)
        todo = [(i, n) for n in niters_list for i in INITS]
        if tag == "48k":
            todo.append(("random", 5))
        for init_name, niters in todo:
            key = "%s_%s_%d" % (tag, init_name, niters)
            np.random.seed(SEED)
            arg = init.copy() if init_name == "ndarray" else init_name
            with contextlib.redirect_stdout(io.StringIO()):
                v_sig, m_phase = mp.griffin_lim(m_mag.copy(), v_shift.copy(), phase_init=arg, niters=niters)
            d[key + "_sig"] = np.asarray(v_sig, dtype=np.float64)
            if niters != 2:
                d[key + "_phase"] = np.asarray(m_phase, dtype=np.float32)
            if init_name == "ndarray" and niters == 1:
                d[key + "_init_after"] = arg
            if init_name == "random":
                d[key + "_rng_pos"] = np.int64(np.random.get_state()[2])
            cases.append(key)
    d["cases"] = np.asarray(cases)
    np.savez_compressed(OUT, **d)
    print("wrote %s (%d cases, %.0f KB)" % (OUT, len(cases), os.path.getsize(OUT) / 1024))


if __name__ == "__main__":
    main()
