"""
Backward pass of the type-2 synthesis from compressed features beside its forward on 64 synthetic utterances at 48 kHz
(fft_len 4096, mag_dim 60, phase_dim 45, device noise): 1000 feature rows each -- 5 s on the 5 ms grid at const_rate_ms 5
("cr"); at the variable rate ("vr", const_rate_ms -1) the same rows are pitch-synchronous frames.  The coefficient rows are
device tensors, the upstream gradient random.  Prints one JSON line and writes it to --out (default
profiles/r17_type2_synthesis_autograd_probe.json).  Per rate, medians of HIP-event times between the marks of
Type2SynthesisPlan.run_backward / run:
  fwd_ms                Type2SynthesisPlan.run() (unwarp, noise power and rms, k_synth_comp_pair's type-2 arm, seam fix-up)
  hpf_adjoint_ms        the elliptic output filter run backwards in time (two index_select, Engine.output_hpf, two casts)
  k_synth_comp_bwd_ms   the frame kernel, type-2 arm, between run_backward's marks
  frame_kernel_t2_ms    the same launch on its own (mpx_synthesis_compressed_type2_backward) ...
  frame_kernel_t1_ms    ... and the type-1 instance (mpx_synthesis_compressed_backward) on the same tables and rows: the
                        arm only drops the end bins' projection, so the two should be equal
  lerp_adjoint_ms       k_rows_lerp_adjoint, width H (magnitudes) and width phase_dim (two streams); 0 at the variable rate
  unwarp_again_ms       the forward's unwarp at the rows' rate (E); 0 at the variable rate
  k_mel_unwarp_bwd_ms   the three jobs in one launch
  backward_ms           run_backward, all of the above but the filter, in one call
  autograd_step_ms      synthesis_from_compressed_type2_batch(return_device=True) + a sum-of-squares loss + backward(),
                        host clock
    python tools/type2_synthesis_autograd_probe.py [--reps 20] [--utts 64] [--rows 1000] [--out FILE]
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


def _timed(fn, reps, warm=3):
    import torch

    ts = []
    for rep in range(reps + warm):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if rep >= warm:
            ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def _marked(run, reps, warm=3):
    """run(mark) -> {label: median ms of the stretch that ends at mark(label)} (repeated labels are summed per pass)."""
    import torch

    acc = {}
    for rep in range(reps + warm):
        evs = []

        def mark(name):
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            evs.append((name, ev))

        run(mark)
        torch.cuda.synchronize()
        if rep < warm:
            continue
        one = {}
        for (_n0, e0), (n1, e1) in zip(evs[:-1], evs[1:]):
            one[n1] = one.get(n1, 0.0) + e0.elapsed_time(e1)
        for k, v in one.items():
            acc.setdefault(k, []).append(v)
    return {k: float(np.median(v)) for k, v in acc.items()}


def _frame_kernel(plan, entry, g, reps):
    """One entry of the frame kernel on the plan's own tables and unwarped rows, all three outputs."""
    e, N = plan.engine, plan.fft_len
    H = N // 2 + 1
    buf, t = plan._buffers(), plan.backward_tables()
    ld = buf["ld"]
    mag, real, imag = buf["spec"]
    outs = [e.empty((plan.total_frames, ld))[:, :H] for _ in range(3)]
    return _timed(lambda: e.launch(entry, N, e.tables(N), g, plan.total_out, t["pos"], t["lo"], t["hi"], plan.total_frames,
                                   mag, real, imag, ld, plan.noise, plan.npos, plan.nleft, plan.nright, plan.wtype,
                                   plan.voiced, buf["inv_gain"], plan.win_l, plan.win_r, plan.per_v, plan.ap_v, plan.ap_u,
                                   int(plan.n_per), outs[0], outs[1], outs[2], ld), reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--utts", type=int, default=64)
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_type2_synthesis_autograd_probe.json"))
    args = ap.parse_args()
    import torch

    from magphase_amd import magphase as mp
    from magphase_amd.engine import get_engine
    from magphase_amd.plans import Type2SynthesisPlan

    fs, N, md, pd = 48000, 4096, 60, 45
    e = get_engine()
    dev = e.device
    rng = np.random.RandomState(0)
    utts = []
    for i in range(args.utts):
        n = args.rows
        f0 = rng.uniform(90.0, 240.0) * np.exp(0.15 * np.sin(2 * np.pi * np.arange(n) / rng.uniform(150, 400)))
        voi = (np.arange(n) // rng.randint(60, 140)) % 3 != 2          # two thirds voiced, in stretches
        lf0 = np.where(voi, np.log(f0), -1.0e10)
        a_mag = (-3.0 + 0.8 * rng.randn(n, md) * np.linspace(1.0, 0.3, md)[None, :]).astype(np.float32)
        a_re, a_im = (np.clip(0.5 * rng.randn(n, pd), -1, 1).astype(np.float32) for _ in range(2))
        utts.append(tuple(torch.from_numpy(x).to(dev) for x in (a_mag, a_re, a_im)) + (lf0,))
    res = {"utts": len(utts), "rows_per_utt": args.rows, "fft_len": N, "mag_dim": md, "phase_dim": pd, "reps": args.reps,
           "device": torch.cuda.get_device_name(dev)}
    seeds = list(range(len(utts)))
    for tag, rate in (("vr", -1.0), ("cr", 5.0)):
        plan = Type2SynthesisPlan(e, utts, fs, fft_len=N, const_rate_ms=rate, noise_mode="device", noise_seeds=seeds)
        pcm = plan.run()
        g64 = torch.randn(plan.total_out, device=dev, dtype=torch.float64)
        g = plan.adjoint_hpf(g64, design="ellip60").contiguous()
        plan.run_backward(g)
        r = {"const_rate_ms": rate, "frames": int(plan.total_frames), "rows": int(plan.n_rows),
             "samples": int(plan.total_out)}
        r["fwd_ms"] = _timed(lambda: plan.run(out=pcm), args.reps)
        r["hpf_adjoint_ms"] = _timed(lambda: plan.adjoint_hpf(g64, design="ellip60"), args.reps)
        m = _marked(lambda mark: plan.run_backward(g, mark=mark), args.reps)
        r["k_synth_comp_bwd_ms"] = m.get("k_synth_comp_bwd", 0.0)
        r["frame_kernel_t2_ms"] = _frame_kernel(plan, "mpx_synthesis_compressed_type2_backward", g, args.reps)
        r["frame_kernel_t1_ms"] = _frame_kernel(plan, "mpx_synthesis_compressed_backward", g, args.reps)
        r["lerp_adjoint_ms"] = m.get("k_rows_lerp_adjoint", 0.0)
        r["unwarp_again_ms"] = m.get("k_mel_unwarp_mfma", 0.0)
        r["k_mel_unwarp_bwd_ms"] = m.get("k_mel_unwarp_bwd", 0.0)
        r["backward_ms"] = _timed(lambda: plan.run_backward(g), args.reps)
        steps = []
        for rep in range(args.reps // 4 + 2):
            leaves = [tuple(x.detach().clone().requires_grad_(True) for x in u[:3]) + (u[3],) for u in utts]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            wavs = mp.synthesis_from_compressed_type2_batch(leaves, fs, fft_len=N, const_rate_ms=rate, noise_mode="device",
                                                            noise_seeds=seeds, return_device=True)
            sum(w.square().sum() for w in wavs).backward()
            torch.cuda.synchronize()
            if rep >= 2:
                steps.append(1e3 * (time.perf_counter() - t0))
        r["autograd_step_ms"] = float(np.median(steps))
        res[tag] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}
        del plan, pcm, g, g64
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
