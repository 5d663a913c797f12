"""
Griffin-Lim with the initial phase built and folded on the device (griffin_lim_batch(fold='device'), k_gl_fold) beside the
host fold (fold='host': numpy draws and numpy fold, the path before the device fold existed), on the headline batch of
tools/griffin_lim_probe.py: 64 synthetic 5 s utterances at 48 kHz, ~57 k frames, fft_len 4096, niters 30.  One process,
the two folds alternated.  Prints one JSON line and writes it to --out:
  batch30_{random,ndarray}_{host,device}_s   griffin_lim_batch end to end, wall time (best of --reps after a warm-up call)
  fold_{half,full,words}_ms                  k_gl_fold alone on all frames (HIP events, median of --kernel-reps), the bytes
  fold_*_bytes, fold_*_gb_per_s              it moves by count (operands read once + rows written) and their rate
  draw_words_ms                              the generator's launches for one group's words (Engine.numpy_global_words)
    python tools/griffin_lim_device_probe.py [--utts 64] [--reps 2] [--out profiles/r27_griffin_lim_device_probe.json]
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=64)
    ap.add_argument("--niters", type=int, default=30)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from magphase_amd import hostmath as hm
    from magphase_amd import magphase as mp
    from magphase_amd import synthetic as syn
    from magphase_amd.engine import get_engine

    fs, dur, N = 48000, 5.0, 4096
    H = N // 2 + 1
    utts = []
    for i in range(args.utts):
        pcm, pm, voi = syn.make_utterance(i, dur_s=dur, fs=fs)
        utts.append((pcm, fs, pm, voi))
    feats = mp.analysis_lossless_batch(utts)
    gl = [(f[0], hm.f0_to_shift(f[3], fs)) for f in feats]
    del feats, utts
    e = get_engine()
    F = int(sum(m.shape[0] for m, _ in gl))
    res = {"utts": len(gl), "frames": F, "fft_len": N, "niters": args.niters}

    # ---- the fold kernel alone, on all frames
    ld = int(e.lib.mpx_spec_ld(H))
    rows = lambda: e.empty((F, ld))[:, :H]   # noqa: E731
    tgt, outs, ph_out = rows(), (rows(), rows(), rows()), rows()
    tgt.copy_(torch.from_numpy(np.concatenate([m for m, _ in gl]).astype(np.float32)))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn):
        ev[0].record()
        fn()
        ev[1].record()
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1])

    np.random.seed(3)
    t0 = time.perf_counter()
    words = e.numpy_global_words(F * N)
    torch.cuda.synchronize()
    res["draw_words_first_call_s"] = time.perf_counter() - t0    # (includes the jump polynomials, computed once)
    t0 = time.perf_counter()
    words = e.numpy_global_words(F * N)
    torch.cuda.synchronize()
    res["draw_words_ms"] = 1e3 * (time.perf_counter() - t0)
    operands = {"words": (words, 8 * N), "full": (e.empty((F, N)).uniform_(-3.14, 3.14), 4 * N),
                "half": (e.empty((F, H)).uniform_(-3.14, 3.14), 4 * H)}
    for form, (ph, row_bytes) in operands.items():
        fn = lambda: e.griffin_lim_fold(N, form, tgt, ph, 0, F, outs, ph_out)   # noqa: E731
        for _ in range(3):
            timed(fn)
        ms = float(np.median([timed(fn) for _ in range(args.kernel_reps)]))
        nbytes = F * (row_bytes + 4 * H + 4 * 4 * H)     # the phase operand + M read, four rows written
        res["fold_%s_ms" % form] = ms
        res["fold_%s_bytes" % form] = nbytes
        res["fold_%s_gb_per_s" % form] = nbytes / ms / 1e6
    del operands, words, outs, ph_out, tgt

    # ---- end to end: the two folds alternated, the same inputs and seed
    rng = np.random.RandomState(7)
    inits = [2 * np.pi * (rng.rand(*m.shape) - 0.5) for m, _ in gl]
    audio_s = None
    for name in ("ndarray", "random"):
        best = {"host": None, "device": None}
        for rep in range(args.reps + 1):          # (the first pass warms both up)
            for fold in ("host", "device"):
                arg = [x.copy() for x in inits] if name == "ndarray" else "random"
                np.random.seed(1)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()):
                    out = mp.griffin_lim_batch(gl, phase_init=arg, niters=args.niters, fold=fold)
                t = time.perf_counter() - t0
                audio_s = sum(len(v) for v, _ in out) / fs
                del out
                if rep and (best[fold] is None or t < best[fold]):
                    best[fold] = t
        for fold, t in best.items():
            res["batch30_%s_%s_s" % (name, fold)] = t
            res["batch30_%s_%s_x_real_time" % (name, fold)] = audio_s / t
    res["audio_s"] = audio_s
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
