"""
TEST INFRASTRUCTURE ONLY -- writes tests/golden/g18_interp_unv.npz from the REAL reference's la.interp_unv_regions
(libaudio.py:273-291), imported in memory through oracle/ref_shim.py:

    python tools/gen_golden_interp_unv.py

Cases (c<i>_data, c<i>_voi, c<i>_out; conds[i], kinds[i], vector[i]): [F x n] matrices and vectors (the reference indexes
two axes, so a vector goes in as [F x 1] and its result is stored as [F]), voicing patterns with leading, trailing and
inner gaps, a gap of one frame, two voiced frames only, the interpolation kinds 'linear', 'slinear' and 'zeros', and
voi_cond other than the default.  The unvoiced rows hold finite values (the reference multiplies them by 0 for 'zeros').
Left out on purpose: one voiced frame (the reference gives NaN there, a 0 / 0 in scipy) and none (it raises IndexError).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g18_interp_unv.npz")
#        name                voicing pattern (1 = voiced)                      n   cond     kind
CASES = (("lead_trail_inner", "00011100001101000", 3, ">0", "linear"),
         ("lead_trail_inner", "00011100001101000", 3, ">0", "slinear"),
         ("lead_trail_inner", "00011100001101000", 3, ">0", "zeros"),
         ("one_frame_gap", "1101011", 2, ">0", "linear"),
         ("two_voiced", "00100000100", 1, ">0", "linear"),
         ("two_voiced_ends", "10000000001", 1, ">0", "slinear"),
         ("two_adjacent", "0001100", 4, ">0", "linear"),
         ("all_voiced", "11111", 2, ">0", "linear"),
         ("vector", "01100011000110", 0, ">0", "linear"),
         ("vector_zeros", "01100011000110", 0, ">0", "zeros"),
         ("cond_half", "0110001100", 3, ">0.5", "linear"),
         ("cond_eq", "0110001101", 2, "==1", "linear"),
         ("cond_lt", "0110001101", 1, "<0.5", "slinear"),
         ("long_gap", "1" + "0" * 70 + "11" + "0" * 9, 2, ">0", "linear"))


def main():
    _mp, la, _lu = ref_shim.load_reference()
    rng = np.random.RandomState(18)
    d, conds, kinds, vector = {}, [], [], []
    for i, (name, pat, n, cond, kind) in enumerate(CASES):
        m = np.array([int(c) for c in pat], dtype=np.float64)
        F = m.size
        voi = m * rng.uniform(0.6, 1.0, F) if cond == ">0.5" else m.copy()
        if cond == ">0.5":
            voi = voi + (1 - m) * rng.uniform(0.0, 0.4, F)
        data = 5.0 + rng.normal(size=(F, max(n, 1)))
        out = la.interp_unv_regions(data.copy(), voi.copy(), voi_cond=cond, interp_type=kind)
        assert np.all(np.isfinite(out)), name
        d["c%d_data" % i] = data[:, 0] if n == 0 else data
        d["c%d_voi" % i] = voi
        d["c%d_out" % i] = np.asarray(out, dtype=np.float64)[:, 0] if n == 0 else np.asarray(out, dtype=np.float64)
        conds.append(cond)
        kinds.append(kind)
        vector.append(n == 0)
        print("%-18s F %3d n %d %-5s %-8s" % (name, F, n, cond, kind))
    d["ncases"] = np.int64(len(CASES))
    d["conds"], d["kinds"], d["vector"] = np.asarray(conds), np.asarray(kinds), np.asarray(vector)
    d["names"] = np.asarray([c[0] for c in CASES])
    np.savez_compressed(OUT, **d)
    print("wrote %s (%d cases, %.1f KB)" % (OUT, len(CASES), os.path.getsize(OUT) / 1024))


if __name__ == "__main__":
    main()
