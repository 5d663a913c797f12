"""
Backward pass of the magnitude-only synthesis beside its forward on 64 synthetic utterances at 48 kHz (fft_len 4096,
mag_dim 60, phase 'min_phase', device noise): 1000 feature rows each -- at the variable rate ("vr") the rows are the
pitch-synchronous frames, so k_min_phase and k_min_phase_bwd both run on the same 64 x 1000 rows; at the constant rate
("cr") the rows are 5 s on the 5 ms grid and the two kernels run on the plan's frames.  Prints one JSON line and writes it
to --out (default profiles/r23_min_phase_autograd_probe.json).  Per rate, medians of HIP-event times between the marks of
MagnitudeSynthesisPlan.run / run_backward:
  fwd_ms                run() (unwarp, noise statistic, k_min_phase, k_synth_comp_pair, seam fix-up)
  k_min_phase_ms        the forward kernel inside run()
  k_synth_comp_bwd_ms   the frame kernel, three gradient rows per frame
  k_min_phase_bwd_ms    the new kernel, in place on the magnitude gradient rows
  bwd_over_fwd_kernel   k_min_phase_bwd_ms / k_min_phase_ms: the yardstick (the same two transforms, comparable row traffic:
                        the forward reads 1 row and writes 3, the backward reads 5 below n_phase + 2 and writes 1)
  lerp_adjoint_ms, unwarp_again_ms (0 at the variable rate), k_mel_unwarp_bwd_ms (the magnitude job alone)
  backward_ms           run_backward in one call;  backward_over_forward = backward_ms / fwd_ms
  zero_backward_ms      run_backward of the phase='zero' plan on the same utterances (no phase rows, no k_min_phase_bwd)
  autograd_step_ms      synthesis_from_mag_batch(return_device=True) + a sum-of-squares loss + backward(), host clock
    python tools/min_phase_autograd_probe.py [--reps 20] [--utts 64] [--rows 1000] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--utts", type=int, default=64)
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_min_phase_autograd_probe.json"))
    args = ap.parse_args()
    import torch

    from magphase_amd import magphase as mp
    from magphase_amd.engine import get_engine
    from magphase_amd.plans import MagnitudeSynthesisPlan

    fs, N, md = 48000, 4096, 60
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
        utts.append((torch.from_numpy(a_mag).to(dev), lf0))
    res = {"utts": len(utts), "rows_per_utt": args.rows, "fft_len": N, "mag_dim": md, "reps": args.reps,
           "device": torch.cuda.get_device_name(dev)}
    seeds = list(range(len(utts)))
    for tag, cr in (("vr", False), ("cr", True)):
        plan = MagnitudeSynthesisPlan(e, utts, fs, fft_len=N, phase="min_phase", b_const_rate=cr, noise_mode="device",
                                      noise_seeds=seeds)
        pcm = plan.run()
        g = plan.adjoint_hpf(torch.randn(plan.total_out, device=dev, dtype=torch.float64)).contiguous()
        plan.run_backward(g)
        r = {"frames": int(plan.total_frames), "rows": int(plan.n_rows), "samples": int(plan.total_out)}
        r["fwd_ms"] = _timed(lambda: plan.run(out=pcm), args.reps)
        r["k_min_phase_ms"] = _marked(lambda mark: plan.run(out=pcm, mark=mark), args.reps).get("k_min_phase", 0.0)
        m = _marked(lambda mark: plan.run_backward(g, mark=mark), args.reps)
        r["k_synth_comp_bwd_ms"] = m.get("k_synth_comp_bwd", 0.0)
        r["k_min_phase_bwd_ms"] = m.get("k_min_phase_bwd", 0.0)
        r["bwd_over_fwd_kernel"] = r["k_min_phase_bwd_ms"] / r["k_min_phase_ms"] if r["k_min_phase_ms"] else None
        r["lerp_adjoint_ms"] = m.get("k_rows_lerp_adjoint", 0.0)
        r["unwarp_again_ms"] = m.get("k_mel_unwarp_mfma", 0.0)
        r["k_mel_unwarp_bwd_ms"] = m.get("k_mel_unwarp_bwd", 0.0)
        r["backward_ms"] = _timed(lambda: plan.run_backward(g), args.reps)
        r["backward_over_forward"] = r["backward_ms"] / r["fwd_ms"]
        zero = MagnitudeSynthesisPlan(e, utts, fs, fft_len=N, phase="zero", b_const_rate=cr, noise_mode="device",
                                      noise_seeds=seeds)
        zero.run()
        zero.run_backward(g)
        r["zero_backward_ms"] = _timed(lambda: zero.run_backward(g), args.reps)
        del zero
        steps = []
        for rep in range(args.reps // 4 + 2):
            leaves = [(u[0].detach().clone().requires_grad_(True), u[1]) for u in utts]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            wavs = mp.synthesis_from_mag_batch(leaves, fs, fft_len=N, b_const_rate=cr, noise_mode="device",
                                               noise_seeds=seeds, return_device=True)
            sum(w.square().sum() for w in wavs).backward()
            torch.cuda.synchronize()
            if rep >= 2:
                steps.append(1e3 * (time.perf_counter() - t0))
        r["autograd_step_ms"] = float(np.median(steps))
        res[tag] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}
        del plan, pcm, g
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
