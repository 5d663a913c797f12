"""
Backward pass of the lossless analysis beside its forward on the headline batch shape (64 synthetic 5 s utterances at
48 kHz, fft_len 4096: bench.py's configs[1]).  The rows come from the analysis of the same utterances, given as device
tensors; the upstream gradients are random.  Prints one JSON line and writes it to --out (default
profiles/r12_analysis_autograd_probe.json):
  fwd_ms                      k_analysis, median per-launch time (HIP events, three warm-up rounds, the variants alternated
                              in this process)
  bwd_ms, bwd_mag_only_ms     the two launches of mpx_analysis_lossless_backward (k_analysis_lossless_bwd +
                              k_analysis_bwd_gather) with all three gradients / with the m_mag gradient only
  bwd_bytes, bwd_tb_s         the bytes the backward has to move -- 24 H F (six rows read) plus the scratch traffic (every
                              frame's samples written once and read once: 8 scratch floats) plus 4 n for the result -- and
                              their rate at bwd_ms; bwd_mag_only_bytes / _tb_s: 16 H F for the four rows that launch reads
  bwd_vs_fwd                  bwd_ms / fwd_ms
  autograd_step_ms            analysis_lossless_batch(return_device=True) on device waveforms + a sum-of-squares loss on the
                              three outputs + backward(), whole call with host planning, one synchronise at the end (host
                              clock)
    python tools/analysis_autograd_probe.py [--reps 20] [--utts 64] [--out FILE]
There is no gate: the feature has no parent to compare with.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--utts", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_analysis_autograd_probe.json"))
    args = ap.parse_args()
    import torch

    from magphase_amd import magphase as mp
    from magphase_amd import synthetic as syn
    from magphase_amd.engine import get_engine
    from magphase_amd.plans import LosslessAnalysisPlan

    fs, dur, N = 48000, 5.0, 4096
    H = N // 2 + 1
    e = get_engine()
    utts = []
    for i in range(args.utts):
        pcm, pm, voi = syn.make_utterance(i, dur_s=dur, fs=fs)
        x = torch.from_numpy(np.asarray(pcm).astype(np.float32) * np.float32(1.0 / 32768.0))   # int16 PCM -> [-1, 1)
        utts.append((x.to(e.device), fs, pm, voi))
    pa = LosslessAnalysisPlan(e, utts, fft_len=N)
    mag, real, imag = pa.run()
    F, n = pa.total_frames, pa.total_smpls
    gm, gr, gi = (torch.randn(F, H, device=e.device, dtype=torch.float32) for _ in range(3))
    _soff, scratch_floats = pa.backward_tables()

    variants = {
        "fwd": lambda: pa.run(out=(mag, real, imag)),
        "bwd": lambda: pa.run_backward(mag, real, imag, (gm, gr, gi)),
        "bwd_mag_only": lambda: pa.run_backward(mag, real, imag, (gm, None, None)),
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

    steps = []
    for rep in range(args.reps // 2 + 2):
        leaves = [u[0].detach().clone().requires_grad_(True) for u in utts]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = mp.analysis_lossless_batch([(x,) + u[1:] for x, u in zip(leaves, utts)], fft_len=N, return_device=True)
        sum(o[k].square().sum() for o in out for k in range(3)).backward()
        torch.cuda.synchronize()
        if rep >= 2:
            steps.append(1e3 * (time.perf_counter() - t0))
    extra = 8 * scratch_floats + 4 * n
    bwd_bytes, mag_bytes = 24 * H * F + extra, 16 * H * F + extra
    res = {"utts": len(utts), "frames": F, "H": H, "samples": n, "scratch_floats": scratch_floats, "reps": args.reps,
           "audio_s": round(n / fs, 1)}
    res.update({k + "_ms": round(v, 4) for k, v in med.items()})
    res.update({k + "_min_max_ms": [round(min(v), 4), round(max(v), 4)] for k, v in times.items()})
    res.update(bwd_bytes=bwd_bytes, bwd_tb_s=round(bwd_bytes / (med["bwd"] * 1e-3) / 1e12, 3),
               bwd_mag_only_bytes=mag_bytes, bwd_mag_only_tb_s=round(mag_bytes / (med["bwd_mag_only"] * 1e-3) / 1e12, 3),
               bwd_vs_fwd=round(med["bwd"] / med["fwd"], 3), autograd_step_ms=round(float(np.median(steps)), 3),
               device=torch.cuda.get_device_name(e.device))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
