"""
The type-2 analysis' backward pass beside its forward, and the true envelope's backward kernel beside its forward kernel, on
the headline batch (64 synthetic 5 s utterances at
48 kHz: magphase_amd.synthetic -> analysis_lossless_batch, ~57 k frames, fft_len 4096), same rows, same process.  Prints
one JSON line (and writes it to --out, default profiles/r18_type2_analysis_autograd_probe.json):
  fwd_<nc>_ms / bwd_<nc>_ms     median launch time (HIP events, warmed up, alternated) of mpx_true_envelope ('abs', thres_db
                                0.1, ticket counter) and of mpx_true_envelope_backward with the forward's pass counts
  bwd_over_fwd_<nc>             their ratio: the backward kernel runs 2 K transforms pairs per frame where the forward runs K,
                                so 2 is its floor at equal occupancy
  waves_per_cu_fwd / _bwd       resident waves per compute unit (one workgroup each: 8 forward; 3 backward at fft_len 4096,
                                where the decision history of 100 passes takes 25.6 KB of LDS per wave)
  passes_<nc>_mean              passes per frame
  deterministic_<nc>            two backward launches give the same bits
  t2_lossless_fwd_ms / _bwd_ms  Type2AnalysisPlan.run(want_iters=True) and .run_backward (all three gradients) on the batch's
                                samples: the backward recomputes both sets of rows, runs k_true_envelope_bwd at 600
                                coefficients and the lossless analysis' backward kernels over both frame tables
  t2_comp_<rate>_fwd_ms / _bwd_ms   Type2CompressedAnalysisPlan.run(want_iters=True) and .run_backward (all three gradients,
                                mag_dim 60, phase_dim 45) at the variable rate ("var") and at const_rate_ms 5 ("5ms"): the
                                backward recomputes the type-2 rows with the pass counts forced, runs the type-1 compressed
                                tail, then the above
  ..._bwd_over_fwd              the ratios
    python tools/type2_analysis_autograd_probe.py [--reps 10] [--utts 64] [--out FILE]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_type2_analysis_autograd_probe.json"))
    args = ap.parse_args()
    import torch

    from magphase_amd import magphase as mp
    from magphase_amd import synthetic as syn
    from magphase_amd.engine import get_engine

    fs, dur, N = 48000, 5.0, 4096
    H = N // 2 + 1
    utts = []
    for i in range(args.utts):
        pcm, pm, voi = syn.make_utterance(i, dur_s=dur, fs=fs)
        utts.append((pcm, fs, pm, voi))
    mags = [f[0] for f in mp.analysis_lossless_batch(utts)]
    e = get_engine()
    dev = [torch.from_numpy(m.astype(np.float32)).to(e.device) for m in mags]
    F = sum(m.shape[0] for m in mags)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn):
        ev[0].record()
        fn()
        ev[1].record()
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1])

    res = {"frames": F, "utts": len(mags), "fft_len": N, "waves_per_cu_fwd": 8, "waves_per_cu_bwd": 3}
    for nc in (60, 600):
        out, _, it, x = e.true_envelope(dev, "abs", nc, 0.1, want_iters=True, return_input=True)
        gy = torch.randn_like(out)
        fns = {"fwd": lambda nc=nc: e.true_envelope(dev, "abs", nc, 0.1, want_iters=True),
               "bwd": lambda nc=nc: e.true_envelope_backward(x, it, gy, H, "abs", nc)}
        for fn in fns.values():
            for _ in range(2):
                timed(fn)
        t = {k: [] for k in fns}
        for _ in range(args.reps):
            for k, fn in fns.items():
                t[k].append(timed(fn))
        for k in fns:
            res["%s_%d_ms" % (k, nc)] = float(np.median(t[k]))
            res["%s_%d_ms_min" % (k, nc)] = float(np.min(t[k]))
        res["bwd_over_fwd_%d" % nc] = res["bwd_%d_ms" % nc] / res["fwd_%d_ms" % nc]
        nan_rows = torch.isnan(out[:, :H]).all(dim=1)
        res["nan_rows_%d" % nc] = int(nan_rows.sum())
        res["passes_%d_mean" % nc] = float(it[~nan_rows].float().mean())
        a = e.true_envelope_backward(x, it, gy, H, "abs", nc)
        b = e.true_envelope_backward(x, it, gy, H, "abs", nc)
        res["deterministic_%d" % nc] = bool(torch.equal(a[:, :H], b[:, :H]))
        res["finite_%d" % nc] = bool(torch.isfinite(a[:, :H]).all())
    # ---- the whole type-2 chain: backward beside forward, same process, same plans
    import warnings

    from magphase_amd.plans import Type2AnalysisPlan, Type2CompressedAnalysisPlan

    def bench(fwd, bwd, key):
        fns = {"fwd": fwd, "bwd": bwd}
        for fn in fns.values():
            for _ in range(2):
                timed(fn)
        t = {k: [] for k in fns}
        for _ in range(args.reps):
            for k, fn in fns.items():
                t[k].append(timed(fn))
        for k in fns:
            res["%s_%s_ms" % (key, k)] = float(np.median(t[k]))
            res["%s_%s_ms_min" % (key, k)] = float(np.min(t[k]))
        res["%s_bwd_over_fwd" % key] = res["%s_bwd_ms" % key] / res["%s_fwd_ms" % key]

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        t2 = Type2AnalysisPlan(e, utts, fft_len=N)
    env, real, imag, _gain, it2 = t2.run(want_iters=True)
    g3 = tuple(torch.randn((t2.total_frames, H), dtype=torch.float32, device=e.device) for _ in range(3))
    bench(lambda: t2.run(want_iters=True), lambda: t2.run_backward(g3, it2), "t2_lossless")
    res["t2_passes_mean"] = float(it2.float().mean())
    res["t2_lossless_finite"] = bool(torch.isfinite(t2.run_backward(g3, it2)).all())
    del env, real, imag, g3
    for rate, tag in ((-1.0, "var"), (5.0, "5ms")):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            pc = Type2CompressedAnalysisPlan(e, utts, fft_len=N, mag_dim=60, phase_dim=45, const_rate_ms=rate)
        outs, _gain, itc = pc.run(want_iters=True)
        gc = tuple(torch.randn_like(o) for o in outs)
        bench(lambda: pc.run(want_iters=True), lambda: pc.run_backward(outs, gc, itc), "t2_comp_" + tag)
        res["t2_comp_%s_out_frames" % tag] = int(pc.total_out_frames)
        res["t2_comp_%s_finite" % tag] = bool(torch.isfinite(pc.run_backward(outs, gc, itc)).all())
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
