"""
Type-2 analysis on the headline batch (64 synthetic 5 s utterances at 48 kHz: magphase_amd.synthetic, fft_len 4096).
Median launch times over --reps rounds (HIP events, warmed up; every round times each variant once, in turn, in this
process).  Prints one JSON line (and writes it to --out):
  lossless_ms                 one lossless analysis launch of the batch (k_analysis, float32: LosslessAnalysisPlan.run)
  lossless_f64_ms             the same frames through k_analysis_f64 (what analysis_compressed runs)
  type2_analysis_ms           the type-2 analysis without the envelope: k_analysis_f64 over the one-period frames,
                              k_analysis_f64 over the two-period frames (magnitudes only), k_frame_gain
  type2_vs_lossless           type2_analysis_ms / lossless_ms (target <= 2.5)
  gain_ms_bpc<k>              k_frame_gain alone with k workgroups of 8 waves per CU
  env_<nc>_ms, ns_per_frame_pass_<nc>
                              k_true_envelope on the batch's two-period magnitudes at 600 and 60 coefficients, and the
                              launch time / (frames x mean passes); env_600_vs_60 = the ratio of the two per-pass figures
  passes_600_hist             passes per frame at 600 coefficients: {passes: frames}, NaN rows (no pass) left out
    python tools/type2_probe.py [--reps 10] [--utts 64] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--utts", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from magphase_amd import _lib
    from magphase_amd import hostmath as hm
    from magphase_amd import synthetic as syn
    from magphase_amd.engine import LosslessAnalysisPlan, Type2AnalysisPlan, get_engine

    fs, dur, N = 48000, 5.0, 4096
    H = N // 2 + 1
    utts = []
    for i in range(args.utts):
        pcm, pm, voi = syn.make_utterance(i, dur_s=dur, fs=fs)
        utts.append((pcm, fs, pm, voi))
    e = get_engine()
    pl = LosslessAnalysisPlan(e, utts)
    t2 = Type2AnalysisPlan(e, utts)
    p1 = t2.lossless
    F = t2.total_frames
    ld = t2.ld
    feats = tuple(e.empty((F, ld))[:, :H] for _ in range(3))
    feats32 = tuple(e.empty_feats(pl.total_frames, H) for _ in range(3))
    gain = torch.empty(F, dtype=torch.float64, device=e.device)
    env = e.empty((F, ld))
    iters = torch.empty(F, dtype=torch.int32, device=e.device)
    tk = torch.empty(1, dtype=torch.int32, device=e.device)

    def lossless():
        pl.run(out=feats32)

    def lossless_f64():
        p1.run(out=feats, precise=True)

    def gain_k(bpc):
        def fn():
            _lib.check(e.lib.mpx_frame_gain(e.stream_ptr(), N, p1.sig.data_ptr(), p1.pos.data_ptr(), p1.left.data_ptr(),
                                            p1.right.data_ptr(), t2.voi.data_ptr(), F, gain.data_ptr(), bpc),
                       "mpx_frame_gain")
        return fn

    def type2_analysis():
        p1.run(out=feats, precise=True)
        e.analysis_frames(N, p1.sig, p1.pos, t2.left2, t2.right2, out=feats, precise=True, rows_in_use=t2.mag_only)
        gain_k(0)()

    def envelope(nc):
        w = e.constant(("true_env_w", N, nc, 0.7), lambda: hm.true_envelope_lifter(N, nc, 0.7))

        def fn():
            _lib.check(e.lib.mpx_true_envelope(e.stream_ptr(), N, e.tables(N).data_ptr(), w.data_ptr(),
                                               feats[0].data_ptr(), ld, F, 0, 0.1, hm.TRUE_ENV_MAX_ITERS, env.data_ptr(),
                                               ld, iters.data_ptr(), None, tk.data_ptr()), "mpx_true_envelope")
        return fn

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn):
        ev[0].record()
        fn()
        ev[1].record()
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1])

    with torch.cuda.device(e.device):
        type2_analysis()   # the two-period magnitudes the envelope variants read
        variants = {"lossless_ms": lossless, "lossless_f64_ms": lossless_f64, "type2_analysis_ms": type2_analysis,
                    "gain_ms_bpc1": gain_k(1), "gain_ms_bpc3": gain_k(3)}
        for _ in range(3):
            for fn in variants.values():
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(args.reps):
            for k, fn in variants.items():
                times[k].append(timed(fn))
        # the envelope variants last: they only read feats[0] (the two-period magnitudes left by type2_analysis)
        type2_analysis()
        env_fns = {nc: envelope(nc) for nc in (600, 60)}
        for fn in env_fns.values():
            fn()
        torch.cuda.synchronize()
        te = {nc: [] for nc in env_fns}
        passes = {}
        for _ in range(args.reps):
            for nc, fn in env_fns.items():
                te[nc].append(timed(fn))
                passes[nc] = iters.cpu().numpy().copy()
    res = {k: float(np.median(v)) for k, v in times.items()}
    res["type2_vs_lossless"] = res["type2_analysis_ms"] / res["lossless_ms"]
    res["frames"] = int(F)
    for nc in env_fns:
        it = passes[nc]
        ok = it > 0
        res["env_%d_ms" % nc] = float(np.median(te[nc]))
        res["passes_%d_mean" % nc] = float(it[ok].mean())
        res["passes_%d_max" % nc] = int(it.max())
        res["nan_rows_%d" % nc] = int(np.sum(~ok))
        res["ns_per_frame_pass_%d" % nc] = 1e6 * res["env_%d_ms" % nc] / float(it[ok].sum())
    res["env_600_vs_60"] = res["ns_per_frame_pass_600"] / res["ns_per_frame_pass_60"]
    h = np.bincount(passes[600][passes[600] > 0])
    res["passes_600_hist"] = {str(k): int(v) for k, v in enumerate(h) if v}
    res["reps"] = args.reps
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
