"""
Griffin-Lim on the headline batch (64 synthetic 5 s utterances at 48 kHz: magphase_amd.synthetic -> analysis_lossless_batch
-> f0_to_shift, ~57 k frames, fft_len 4096).  Prints one JSON line:
  gl_iter_ms / rt_ms      median per-launch time (HIP events, warmed up, alternated in this process) of one Griffin-Lim
                          iteration (k_griffin_lim_pair + k_ola_fixup) and of the one-launch copy synthesis
                          (k_roundtrip_pair + k_ola_fixup) on the same frames, and their ratio
  batch30_*_s             griffin_lim_batch(niters=30) end to end (ndarray init / 'random'), host init + fold time
                          separately, and x real time (audio seconds / wall seconds)
  model_*                 max |device - fp64 model| / peak and the spectral convergence of both, two utterances
    python tools/griffin_lim_probe.py [--reps 20] [--out FILE] [--timing-only]
--timing-only: the first part alone, so that a kernel trace of the run (rocprofv3 --kernel-trace --stats) holds the
launches on the 57 k frames and nothing else (the end-to-end and model parts launch the same kernels on other sizes).
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--utts", type=int, default=64)
    ap.add_argument("--out", default=None)
    ap.add_argument("--timing-only", action="store_true")
    args = ap.parse_args()
    import torch

    from magphase_amd import hostmath as hm
    from magphase_amd import magphase as mp
    from magphase_amd import synthetic as syn
    from magphase_amd.engine import GriffinLimPlan, LosslessRoundTripPlan, get_engine

    fs, dur = 48000, 5.0
    utts = []
    for i in range(args.utts):
        pcm, pm, voi = syn.make_utterance(i, dur_s=dur, fs=fs)
        utts.append((pcm, fs, pm, voi))
    feats = mp.analysis_lossless_batch(utts)
    gl = [(f[0], hm.f0_to_shift(f[3], fs)) for f in feats]
    e = get_engine()
    N = 4096
    H = N // 2 + 1
    shifts = [hm.griffin_lim_shifts(m, s)[0] for m, s in gl]
    plan = GriffinLimPlan(e, shifts, N)
    F = plan.total_frames
    ld = int(e.lib.mpx_spec_ld(H))
    tgt = e.empty((F, ld))[:, :H]
    tgt.copy_(torch.from_numpy(np.concatenate([m for m, _ in gl]).astype(np.float32)))
    ones, zeros = e.empty((F, ld))[:, :H], e.empty((F, ld))[:, :H]
    ones.fill_(1.0), zeros.fill_(0.0)
    sig, _ = plan.run(tgt, [tgt, ones, zeros], 2)   # first synthesis + one iteration: buffers and strips in use
    rt = LosslessRoundTripPlan(e, utts)
    rt_feats = tuple(e.empty_feats(rt.total_frames, H) for _ in range(3))
    rt_out = e.empty((rt.total_out,))
    a, b = plan.bufs

    def gl_step():
        e.griffin_lim_ola(N, plan, tgt, a, b, plan.strips)
        e.ola_fixup(N, plan.iter, plan.strips, b)

    def rt_step():
        rt.run(feats=rt_feats, out=rt_out)

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn):
        ev[0].record()
        fn()
        ev[1].record()
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1])

    for _ in range(3):
        timed(gl_step), timed(rt_step)
    t_gl, t_rt = [], []
    for _ in range(args.reps):
        t_gl.append(timed(gl_step))
        t_rt.append(timed(rt_step))
    res = {"frames": F, "rt_frames": rt.total_frames, "utts": len(gl), "fft_len": N,
           "gl_iter_ms": float(np.median(t_gl)), "rt_ms": float(np.median(t_rt)),
           "gl_iter_ms_min": float(np.min(t_gl)), "rt_ms_min": float(np.min(t_rt))}
    res["gl_over_rt"] = res["gl_iter_ms"] / res["rt_ms"]
    audio_s = sum(int(x) for x in plan.out_len) / fs
    del rt, rt_feats, rt_out, ones, zeros, sig
    if args.timing_only:
        print(json.dumps(res))
        return

    # end to end, niters = 30: host init + fold measured on the same inputs beforehand
    rng = np.random.RandomState(7)
    inits = [2 * np.pi * (rng.rand(*m.shape) - 0.5) for m, _ in gl]
    for name, arg in (("ndarray", [x.copy() for x in inits]), ("random", "random")):
        t0 = time.perf_counter()
        np.random.seed(1)
        for (m, _), x in zip(gl, arg if name == "ndarray" else [name] * len(gl)):
            ph, full = hm.griffin_lim_initial_phase(x.copy() if name == "ndarray" else x, m)
            hm.griffin_lim_fold(m, ph, full)
        t_host = time.perf_counter() - t0
        torch.cuda.synchronize()
        np.random.seed(1)
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            out = mp.griffin_lim_batch(gl, phase_init=arg, niters=30)
        t_all = time.perf_counter() - t0
        res["batch30_%s_s" % name] = t_all
        res["batch30_%s_host_init_fold_s" % name] = t_host
        res["batch30_%s_x_real_time" % name] = audio_s / t_all
        del out
    res["audio_s"] = audio_s

    # accuracy against the fp64 model, niters = 30, 'random' seeded: two utterances
    import griffin_lim_model as glm
    errs, scs = [], []
    for u in (0, 1):
        m, s = gl[u]
        np.random.seed(11)
        ref, _ = glm.griffin_lim(m, s, "random", 30)
        np.random.seed(11)
        with contextlib.redirect_stdout(io.StringIO()):
            v, _ = mp.griffin_lim(m, s, phase_init="random", niters=30)
        errs.append(float(np.max(np.abs(v - ref)) / np.max(np.abs(ref))))
        scs.append((glm.spectral_convergence(v, m, s), glm.spectral_convergence(ref, m, s)))
    res["model_max_err_over_peak_niters30"] = errs
    res["model_sc_dev_vs_fp64"] = scs
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
