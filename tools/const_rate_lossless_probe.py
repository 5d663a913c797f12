"""
Constant-rate lossless analysis / synthesis on the headline batch shape (64 synthetic 5 s utterances at 48 kHz, fft_len
4096: bench.py's configs[1]; magphase_amd.synthetic's fully unvoiced utterances are skipped -- the constant-rate f0
needs a voiced frame -- and the next ones taken).  Prints one JSON line:
  ana_k_analysis_ms, ana_k_rows_lerp_ms   median per-launch time (HIP events, warmed up, the variants alternated in this
                                          process) of the two analysis launches; lerp_bytes and lerp_tb_s: the bytes
                                          k_rows_lerp moves, 12 H (F_var + F_const), and their rate
  syn_fused_ms                            the LERP arm of k_synth_ola_pair + k_ola_fixup on the constant-rate rows
  syn_staged_ms (+ _lerp_ms)              k_rows_lerp into variable-rate rows, then k_synth_ola_pair + k_ola_fixup
  syn_plain_ms                            k_synth_ola_pair + k_ola_fixup on the same variable-rate rows (already there)
  fused_vs_staged, fused_vs_plain         ratios of the medians
    python tools/const_rate_lossless_probe.py [--reps 20] [--out FILE] [--timing-only]
--timing-only: the timed loop alone (for a kernel trace: rocprofv3 --kernel-trace --stats -- python ...).
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
    ap.add_argument("--timing-only", action="store_true")
    args = ap.parse_args()
    import torch

    from magphase_amd import magphase as mp
    from magphase_amd import synthetic as syn
    from magphase_amd.engine import LosslessConstRateAnalysisPlan, LosslessConstRateSynthesisPlan, get_engine

    fs, dur, N, cr = 48000, 5.0, 4096, 5.0
    H = N // 2 + 1
    utts, i = [], 0
    while len(utts) < args.utts:
        pcm, pm, voi = syn.make_utterance(i, dur_s=dur, fs=fs)
        i += 1
        if np.any(np.asarray(voi) > 0):
            utts.append((pcm, fs, pm, voi))
    e = get_engine()
    pa = LosslessConstRateAnalysisPlan(e, utts, fft_len=N, const_rate_ms=cr)
    F_var, F_c = pa.lossless.total_frames, pa.total_out_frames
    var = pa.lossless.run()
    crow = tuple(e.empty_feats(F_c, H) for _ in range(3))
    ps = LosslessConstRateSynthesisPlan(e, pa.v_f0, pa.fs, N, const_rate_ms=cr)
    F_s = ps.total_frames
    srow = tuple(e.empty_feats(F_s, H) for _ in range(3))
    pcm_out = e.empty((ps.total_out,))
    strips = e.empty((max(ps.inner.strip_floats, 1),))
    e.rows_lerp(var, pa.rows, F_c, out=crow)
    e.rows_lerp(crow, ps.rows, F_s, out=srow)

    variants = {
        "ana_k_analysis": lambda: pa.lossless.run(out=var),
        "ana_k_rows_lerp": lambda: e.rows_lerp(var, pa.rows, F_c, out=crow),
        "syn_fused": lambda: ps.run(*crow, strips=strips, out=pcm_out),
        "syn_staged_lerp": lambda: e.rows_lerp(crow, ps.rows, F_s, out=srow),
        "syn_staged": lambda: ps.run_staged(*crow, rows_out=srow, out=pcm_out),
        "syn_plain": lambda: ps.inner.run(*srow, strips=strips, out=pcm_out),
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
    lerp_bytes = 12 * H * (F_var + F_c)
    out = {"utts": len(utts), "F_var": F_var, "F_const": F_c, "F_syn": F_s, "H": H, "reps": args.reps}
    out.update({k + "_ms": round(v, 4) for k, v in med.items()})
    out.update(lerp_bytes=lerp_bytes, lerp_tb_s=round(lerp_bytes / (med["ana_k_rows_lerp"] * 1e-3) / 1e12, 3),
               syn_lerp_tb_s=round(12 * H * (F_c + F_s) / (med["syn_staged_lerp"] * 1e-3) / 1e12, 3),
               fused_vs_staged=round(med["syn_fused"] / med["syn_staged"], 3),
               fused_vs_plain=round(med["syn_fused"] / med["syn_plain"], 3))
    if not args.timing_only:   # parity of the timed launches: fused vs staged signal, on this batch
        f = e.to_host_f64(ps.run(*crow))
        s = e.to_host_f64(ps.run_staged(*crow))
        out["fused_vs_staged_max_abs_over_peak"] = float(np.max(np.abs(f - s)) / np.max(np.abs(s)))
        out["audio_s"] = round(sum(len(u[0]) for u in utts) / fs, 1)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
