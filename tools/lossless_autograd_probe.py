"""
Backward pass of the lossless synthesis beside its forward on the headline batch shape (64 synthetic 5 s utterances at
48 kHz, fft_len 4096: bench.py's configs[1]).  The features come from the lossless analysis of the same utterances, the
upstream gradient is random.  Prints one JSON line and writes it to --out (default
profiles/r11_lossless_autograd_probe.json):
  fwd_pair_ms, fwd_fixup_ms   median per-launch time (HIP events, warmed up, the variants alternated in this process) of
                              the forward's two launches, k_synth_ola_pair and k_ola_fixup
  bwd_ms, bwd_mag_only_ms     k_synth_lossless_bwd with all three gradients / with the m_mag gradient only
  bwd_bytes, bwd_tb_s         the bytes the backward kernel has to move, 24 H F (three rows read, three written), and
                              their rate at bwd_ms
  bwd_vs_fwd                  bwd_ms / (fwd_pair_ms + fwd_fixup_ms)
  autograd_step_ms            synthesis_from_lossless_batch(return_device=True) + a sum-of-squares loss + backward(), whole
                              call with host planning, one synchronise at the end (host clock)
    python tools/lossless_autograd_probe.py [--reps 20] [--utts 64] [--out FILE]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_lossless_autograd_probe.json"))
    args = ap.parse_args()
    import torch

    from magphase_amd import magphase as mp
    from magphase_amd import synthetic as syn
    from magphase_amd.engine import LosslessAnalysisPlan, LosslessSynthesisPlan, get_engine

    fs, dur, N = 48000, 5.0, 4096
    H = N // 2 + 1
    utts = []
    for i in range(args.utts):
        pcm, pm, voi = syn.make_utterance(i, dur_s=dur, fs=fs)
        utts.append((pcm, fs, pm, voi))
    e = get_engine()
    pa = LosslessAnalysisPlan(e, utts, fft_len=N)
    mag, real, imag = pa.run()
    U = len(utts)
    ps = LosslessSynthesisPlan(e, [pa.v_f0[u] for u in range(U)], pa.fs, N)
    F = ps.total_frames
    assert F == int(mag.shape[0])
    out = e.empty((ps.total_out,))
    strips = e.empty((max(ps.strip_floats, 1),))
    gy = torch.randn(ps.total_out, device=e.device, dtype=torch.float32)

    variants = {
        "fwd_pair": lambda: e.synthesis_lossless_ola(N, mag, real, imag, ps, strips, out),
        "fwd_fixup": lambda: e.ola_fixup(N, ps, strips, out),
        "bwd": lambda: ps.run_backward(gy, mag, real, imag),
        "bwd_mag_only": lambda: ps.run_backward(gy, mag, real, imag, need=(True, False, False)),
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

    fo = pa.frame_off
    feats = [(mag[int(fo[u]):int(fo[u + 1])], real[int(fo[u]):int(fo[u + 1])], imag[int(fo[u]):int(fo[u + 1])]) for u in range(U)]
    steps = []
    for rep in range(args.reps // 2 + 2):
        leaves = [tuple(x.detach().clone().requires_grad_(True) for x in f) for f in feats]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sigs = mp.synthesis_from_lossless_batch([l + (pa.v_f0[u], fs) for u, l in enumerate(leaves)], return_device=True)
        torch.cat(sigs).square().sum().backward()
        torch.cuda.synchronize()
        if rep >= 2:
            steps.append(1e3 * (time.perf_counter() - t0))
    bwd_bytes = 24 * H * F
    res = {"utts": U, "frames": F, "H": H, "reps": args.reps, "audio_s": round(sum(len(u[0]) for u in utts) / fs, 1)}
    res.update({k + "_ms": round(v, 4) for k, v in med.items()})
    res.update({k + "_min_max_ms": [round(min(v), 4), round(max(v), 4)] for k, v in times.items()})
    res.update(bwd_bytes=bwd_bytes, bwd_tb_s=round(bwd_bytes / (med["bwd"] * 1e-3) / 1e12, 3),
               bwd_vs_fwd=round(med["bwd"] / (med["fwd_pair"] + med["fwd_fixup"]), 3),
               autograd_step_ms=round(float(np.median(steps)), 3), device=torch.cuda.get_device_name(e.device))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
