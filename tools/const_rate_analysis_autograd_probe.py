"""
Backward pass of the constant-rate lossless analysis, fused and staged, beside its forward on the headline batch shape
(64 synthetic 5 s utterances at 48 kHz, fft_len 4096, const_rate_ms 5).  The waveforms are device tensors; the upstream
gradients of the constant-rate rows are random.  HIP events, three warm-up rounds, the variants interleaved in this
process.  Prints one JSON line and writes it to --out (default profiles/r28_const_rate_analysis_autograd_probe.json):
  fwd_ms                LosslessConstRateAnalysisPlan.run: k_analysis + k_rows_lerp
  rows_ms               k_analysis alone (the rows both backward forms recompute first; part of both figures below)
  fused_ms              run_backward: k_analysis, k_analysis_lossless_bwd<P, CR = true>, k_analysis_bwd_gather
  staged_ms             run_backward_staged: k_analysis, k_rows_lerp_adjoint, k_analysis_lossless_bwd<P>, k_analysis_bwd_gather
  *_bytes, *_tb_s       the bytes each form has to move by the algorithmic count (every buffer once per kernel that reads
                        or writes it; the constant-rate gradient rows count once although two frames read most of them)
                        and their rate at the median:
                          rows    4 n + 12 H F
                          fwd     rows + 12 H (F + Fc)
                          fused   rows + 12 H F + 12 H Fc + 8 S + 4 n
                          staged  rows + (12 H Fc + 12 H F) + (24 H F + 8 S + 4 n)    = fused + 2 x 12 H F
                        (n samples, F variable-rate frames, Fc constant-rate rows, S scratch floats, H bins)
  fused_vs_staged       fused_ms / staged_ms: the yardstick is the staged form in the same process, not a fixed figure
  equal_bits            the two forms' results compared with torch.equal
    python tools/const_rate_analysis_autograd_probe.py [--reps 20] [--utts 64] [--const-rate-ms 5] [--out FILE]
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--utts", type=int, default=64)
    ap.add_argument("--const-rate-ms", type=float, default=5.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r28_const_rate_analysis_autograd_probe.json"))
    args = ap.parse_args()
    import torch

    from magphase_amd import synthetic as syn
    from magphase_amd.engine import get_engine
    from magphase_amd.plans import LosslessConstRateAnalysisPlan

    fs, dur, N = 48000, 5.0, 4096
    H = N // 2 + 1
    e = get_engine()
    utts = []
    for i in range(args.utts):
        pcm, pm, voi = syn.make_utterance(i, dur_s=dur, fs=fs)
        x = torch.from_numpy(np.asarray(pcm).astype(np.float32) * np.float32(1.0 / 32768.0))   # int16 PCM -> [-1, 1)
        utts.append((x.to(e.device), fs, pm, voi))
    plan = LosslessConstRateAnalysisPlan(e, utts, fft_len=N, const_rate_ms=args.const_rate_ms)
    pl = plan.lossless
    out = plan.run()
    F, Fc, n = int(pl.total_frames), int(plan.total_out_frames), int(pl.total_smpls)
    grads = tuple(torch.randn(Fc, H, device=e.device, dtype=torch.float32) for _ in range(3))
    _soff, S = pl.backward_tables()
    equal = bool(torch.equal(plan.run_backward(grads), plan.run_backward_staged(grads)))

    variants = {
        "fwd": lambda: plan.run(out=out),
        "rows": lambda: pl.run(),
        "fused": lambda: plan.run_backward(grads),
        "staged": lambda: plan.run_backward_staged(grads),
    }
    times = {k: [] for k in variants}
    for rep in range(args.reps + 3):   # 3 warm-up rounds
        for k, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if rep >= 3:
                times[k].append(a.elapsed_time(b))
    med = {k: float(np.median(v)) for k, v in times.items()}

    rows_b = 4 * n + 12 * H * F
    nbytes = {"rows": rows_b, "fwd": rows_b + 12 * H * (F + Fc),
              "fused": rows_b + 12 * H * F + 12 * H * Fc + 8 * S + 4 * n}
    nbytes["staged"] = nbytes["fused"] + 2 * 12 * H * F
    res = {"utts": len(utts), "const_rate_ms": args.const_rate_ms, "frames": F, "const_rows": Fc, "H": H, "samples": n,
           "scratch_floats": S, "reps": args.reps, "audio_s": round(n / fs, 1)}
    res.update({k + "_ms": round(v, 4) for k, v in med.items()})
    res.update({k + "_min_max_ms": [round(min(v), 4), round(max(v), 4)] for k, v in times.items()})
    res.update({k + "_bytes": v for k, v in nbytes.items()})
    res.update({k + "_tb_s": round(nbytes[k] / (med[k] * 1e-3) / 1e12, 3) for k in nbytes})
    res.update(fused_vs_staged=round(med["fused"] / med["staged"], 3), equal_bits=equal,
               device=torch.cuda.get_device_name(e.device))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
