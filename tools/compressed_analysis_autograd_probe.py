"""
Backward pass of the compressed analysis beside its forward on 64 synthetic 5 s utterances at 48 kHz (fft_len 4096,
mag_dim 60, phase_dim 45), at the variable and the constant frame rate.  The waveforms are device tensors, the upstream
gradients random.  Prints one JSON line and writes it to --out (default
profiles/r15_compressed_analysis_autograd_probe.json).  Per rate ("vr" / "cr"), medians of HIP-event times:
  fwd_ms                CompressedAnalysisPlan.run()
  rows_ms               the recomputation of the lossless rows (LosslessAnalysisPlan.run, float64 transform, every row)
  mask_ms               k_phase_grad_mask
  warp_bwd_ms           k_mel_warp_bwd (the three jobs in one launch) on the recomputed rows
  warp_bwd_bytes, _tb_s the bytes it writes (3 rows x H x 4 -- at the constant rate the magnitude job writes per OUTPUT
                        frame) plus the bytes it reads (the operand rows, the magnitudes' twice where interpolated; g and W
                        are small), and their rate at warp_bwd_ms
  lerp_adjoint_ms       k_rows_lerp_adjoint: phase_dim wide (two streams) and H wide (magnitudes); 0 at the variable rate
  lossless_bwd_ms       mpx_analysis_lossless_backward on the three gradient rows
  backward_ms           CompressedAnalysisPlan.run_backward, all of the above in one call
  autograd_step_ms      analysis_compressed_batch(return_device=True) + a sum-of-squares loss + backward(), host clock
fill_tb_s: the device's streaming fill rate (mpx_bw_probe, best shape) -- the ceiling of a kernel made of its stores;
warp_fwd_ms: k_mel_warp_mfma (staged forward warp of the same constant-rate batch, the parent's kernel) for scale.
    python tools/compressed_analysis_autograd_probe.py [--reps 20] [--utts 64] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--utts", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_compressed_analysis_autograd_probe.json"))
    args = ap.parse_args()
    import torch

    from magphase_amd import _lib, hostmath as hm, magphase as mp
    from magphase_amd import synthetic as syn
    from magphase_amd.engine import get_engine
    from magphase_amd.plans import CompressedAnalysisPlan

    fs, dur, N, md, pd = 48000, 5.0, 4096, 60, 45
    H = N // 2 + 1
    e = get_engine()
    dev = e.device
    utts = []
    for i in range(args.utts):
        pcm, pm, voi = syn.make_utterance(i, dur_s=dur, fs=fs)
        x = torch.from_numpy(np.asarray(pcm).astype(np.float32) * np.float32(1.0 / 32768.0))
        utts.append((x.to(dev), fs, pm, voi))
    res = {"utts": len(utts), "H": H, "mag_dim": md, "phase_dim": pd, "reps": args.reps,
           "device": torch.cuda.get_device_name(dev)}

    # the device's fill rate: the ceiling of a kernel that is made of its stores
    n_fill = 1 << 28
    buf, one = e.empty((n_fill,)), e.empty((4,))
    best = 0.0
    for shape in range(int(e.lib.mpx_bw_probe_shapes())):
        ms = _timed(lambda: _lib.check(e.lib.mpx_bw_probe(e.stream_ptr(), 1 + 16 * shape, buf.data_ptr(), one.data_ptr(),
                                                          n_fill), "mpx_bw_probe"), 5, 2)
        best = max(best, 4.0 * n_fill / (ms * 1e-3) / 1e12)
    res["fill_tb_s"] = round(best, 3)
    del buf

    for tag, cr in (("vr", False), ("cr", True)):
        plan = CompressedAnalysisPlan(e, utts, fft_len=N, mag_dim=md, phase_dim=pd, b_const_rate=cr)
        pl = plan.lossless
        Fo, n_var = plan.total_out_frames, int(pl.total_frames)
        outs = plan.run()
        g = (torch.randn(Fo, md, device=dev), torch.randn(Fo, pd, device=dev), torch.randn(Fo, pd, device=dev))
        rows = pl.run(precise=True, rows_in_use=None)
        h = e.phase_grad_mask(outs[1], outs[2], plan.voi, g[1], g[2])
        tabs = live = None
        if cr:
            adj = e.to_device(hm.lerp_adjoint_table(*plan._rows_host, n_var).reshape(-1), np.int32)
            tabs, live = (plan.row0, plan.row1, plan.rowt), plan.rows_in_use
            hv = e.rows_lerp_adjoint((None,) + h, adj, plan.rowt, n_var)[1:]
        else:
            live, hv = plan.voi, h
        g_rows = e.mel_warp_backward(H, mag=(g[0], plan.w_mag, rows[0], tabs), phase=(hv[0], hv[1], plan.w_ph, rows[1], rows[2], live))
        r = {"frames": n_var, "out_frames": Fo}
        r["fwd_ms"] = _timed(lambda: plan.run(out=outs), args.reps)
        r["rows_ms"] = _timed(lambda: pl.run(out=rows, precise=True, rows_in_use=None), args.reps)
        r["mask_ms"] = _timed(lambda: e.phase_grad_mask(outs[1], outs[2], plan.voi, g[1], g[2]), args.reps)
        r["warp_bwd_ms"] = _timed(lambda: e.mel_warp_backward(H, mag=(g[0], plan.w_mag, rows[0], tabs),
                                                              phase=(hv[0], hv[1], plan.w_ph, rows[1], rows[2], live),
                                                              out=g_rows), args.reps)
        nbytes = 4 * H * ((Fo + 2 * n_var) + ((2 * Fo if cr else Fo) + 2 * n_var))
        r["warp_bwd_bytes"] = nbytes
        r["warp_bwd_tb_s"] = round(nbytes / (r["warp_bwd_ms"] * 1e-3) / 1e12, 3)
        if cr:
            r["lerp_adjoint_ms"] = (_timed(lambda: e.rows_lerp_adjoint((None,) + h, adj, plan.rowt, n_var), args.reps)
                                    + _timed(lambda: e.rows_lerp_adjoint((g_rows[0], None, None), adj, plan.rowt, n_var),
                                             args.reps))
            gl = (e.rows_lerp_adjoint((g_rows[0], None, None), adj, plan.rowt, n_var)[0], g_rows[1], g_rows[2])
            # the staged forward warp of the same batch, for scale
            wout = tuple(torch.empty_like(o) for o in outs)
            warp = (Fo, H, rows[0], rows[1], rows[2], plan.row0, plan.row1, plan.rowt, plan.w_mag, md, plan.w_ph, pd, plan.voi,
                    wout[0], wout[1], wout[2], e.feat_ld(*rows), 0, n_var, plan.rows_in_use, *plan._phase_rows_tmp())
            res["warp_fwd_ms"] = round(_timed(lambda: e.launch("mpx_mel_warp_rows", *warp), args.reps), 4)
        else:
            r["lerp_adjoint_ms"], gl = 0.0, g_rows
        r["lossless_bwd_ms"] = _timed(lambda: pl.run_backward(rows[0], rows[1], rows[2], gl), args.reps)
        r["backward_ms"] = _timed(lambda: plan.run_backward(outs, g), args.reps)
        del rows, g_rows, gl
        steps = []
        for rep in range(args.reps // 4 + 2):
            leaves = [u[0].detach().clone().requires_grad_(True) for u in utts]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = mp.analysis_compressed_batch([(x,) + u[1:] for x, u in zip(leaves, utts)], fft_len=N, mag_dim=md,
                                               phase_dim=pd, b_const_rate=cr, return_device=True)
            sum(o[k].square().sum() for o in out for k in range(3)).backward()
            torch.cuda.synchronize()
            if rep >= 2:
                steps.append(1e3 * (time.perf_counter() - t0))
        r["autograd_step_ms"] = float(np.median(steps))
        res[tag] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
