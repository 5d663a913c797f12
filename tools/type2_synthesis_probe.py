"""
Type-2 synthesis on the headline batch (64 synthetic 5 s utterances at 48 kHz, 60 magnitude and 45 phase coefficients per
row on the 5 ms grid, rows built as bench.py builds its configs[2] features; the same arrays and the same device noise
feed both chains).  Median times over --reps rounds (HIP events, warmed up; every round times each variant once, in a
rotating order, in this process).  Prints one JSON line (and writes it to --out):
  t1_stat_ms / t2_stat_ms     the noise statistic alone: mpx_noise_stats + mpx_noise_gains (type 1) against
                              mpx_noise_power + mpx_noise_rms (type 2) on the same noise and frame tables
  stat_ratio                  t2_stat_ms / t1_stat_ms (expected well below 1: no transform)
  noise_power_ms, noise_power_gbps
                              mpx_noise_power alone and the bytes it must read (4 x the summed frame lengths) per second
  t1_chain_ms, t1_chain_again_ms, t2_chain_ms
                              the whole launch chain (unwarp, statistic, pair kernel, fix-up, output high-pass); type 1 is
                              timed twice per round: aa_spread = their ratio, what two runs of the same code show here
  chain_ratio                 t2_chain_ms / mean of the two type-1 figures (target <= 1.05)
The type-1 plan here is the repository's own (its launch sequence, entries and kernels are the parent commit's: the
refactoring moved them into methods, the instantiations' resource usage is unchanged -- DESIGN.md 3.3f).

    python tools/type2_synthesis_probe.py [--reps 20] [--utts 64] [--out FILE]
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
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-power", action="store_true",
                    help="warm up, then launch mpx_noise_power --reps times and exit (for a kernel trace of its own)")
    args = ap.parse_args()
    import torch
    from scipy import signal

    from magphase_amd import engine as em
    from magphase_amd import synthetic as syn

    fs = 48000
    utts = []
    for i in range(args.utts):
        pcm, pm, voi = syn.make_utterance(i, dur_s=5.0, fs=fs)
        utts.append((pcm, fs, pm, voi))
    e = em.get_engine()
    aplan = em.CompressedAnalysisPlan(e, utts, mag_dim=60, phase_dim=45, b_const_rate=True)
    H = aplan.fft_len // 2 + 1
    feats = None if getattr(aplan, "fused_cr", False) else tuple(
        e.empty_feats(aplan.lossless.total_frames, H) for _ in range(3))
    out = aplan.run(feats=feats)
    torch.cuda.synchronize()
    res = [t.cpu().numpy().astype(np.float64) for t in out]
    sutts = []
    for u in range(len(utts)):
        a, b = int(aplan.out_off[u]), int(aplan.out_off[u + 1])
        v_f0 = aplan.f0_out[u]
        with np.errstate(divide="ignore"):
            v_lf0 = np.log((v_f0 > 0).astype(float) * signal.medfilt(v_f0))
        v_lf0[np.isinf(v_lf0) | np.isnan(v_lf0)] = -1.0e10
        sutts.append((res[0][a:b], res[1][a:b], res[2][a:b], v_lf0))
    del aplan, feats, out
    seeds = np.arange(len(sutts))
    p1 = em.CompressedSynthesisPlan(e, sutts, fs, b_const_rate=True, noise_mode="device", noise_seeds=seeds)
    p2 = em.Type2SynthesisPlan(e, sutts, fs, const_rate_ms=5.0, noise_mode="device", noise_seeds=seeds)
    assert p1.total_frames == p2.total_frames and p1.ns_len == p2.ns_len
    N = p2.fft_len
    tab = e.tables(N)
    b1, b2 = p1._buffers(), p2._buffers()
    mark = lambda name: None   # noqa: E731

    def t1_stat():
        p1._launch_noise_statistic(tab, b1, mark)

    def t2_stat():
        p2._launch_noise_statistic(tab, b2, mark)

    def power():
        e.launch("mpx_noise_power", N, p2.noise, p2.npos, p2.nleft, p2.nright, p2.wtype, p2.total_frames, b2["power"])

    def t1_chain():
        e.output_hpf(p1.run(), p1.out_off_host, fs)

    def t2_chain():
        e.output_hpf(p2.run(), p2.out_off_host, fs, design="ellip60")

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn):
        ev[0].record()
        fn()
        ev[1].record()
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1])

    with torch.cuda.device(e.device):
        if args.only_power:
            for _ in range(3 + args.reps):
                power()
            torch.cuda.synchronize()
            return
        variants = [("t1_stat_ms", t1_stat), ("t2_stat_ms", t2_stat), ("noise_power_ms", power),
                    ("t1_chain_ms", t1_chain), ("t2_chain_ms", t2_chain), ("t1_chain_again_ms", t1_chain)]
        for _ in range(3):
            for _, fn in variants:
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k, _ in variants}
        for r in range(args.reps):
            order = variants[r % len(variants):] + variants[:r % len(variants)]
            for k, fn in order:
                times[k].append(timed(fn))
    res = {k: float(np.median(v)) for k, v in times.items()}
    nbytes = 4.0 * float(np.sum(p2._tabs["nleft"].astype(np.int64) + p2._tabs["nright"].astype(np.int64) + 1))
    res["stat_ratio"] = res["t2_stat_ms"] / res["t1_stat_ms"]
    res["noise_power_bytes"] = nbytes
    res["noise_power_gbps"] = nbytes / (res["noise_power_ms"] * 1e-3) / 1e9
    res["aa_spread"] = res["t1_chain_again_ms"] / res["t1_chain_ms"]
    res["chain_ratio"] = res["t2_chain_ms"] / (0.5 * (res["t1_chain_ms"] + res["t1_chain_again_ms"]))
    res["frames"] = int(p2.total_frames)
    res["utts"] = len(sutts)
    res["reps"] = args.reps
    res["rms_first"] = p2.rms[0]
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
