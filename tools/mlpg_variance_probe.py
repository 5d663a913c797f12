#!/usr/bin/env python
"""
What the MLPG variance entries cost beside the solve they follow (64 utterances x 1000 frames, D = 60, two dynamic windows,
float32 means and targets, float64 variances), all in one process: one JSON under profiles/.

    python tools/mlpg_variance_probe.py

  solve          ONE mpx_mlpg_solve launch (k_mlpg_solve), as tools/mlpg_probe.py times it
  var_backward   ONE mpx_mlpg_var_backward call (k_mlpg_var_bwd; global variances: and the two column-pass kernels)
  nll            ONE mpx_mlpg_trajectory_nll launch (k_mlpg_nll)
  nll_backward   ONE mpx_mlpg_trajectory_nll_backward launch (k_mlpg_nll_bwd), both gradients / the means' alone

each for per-frame variances and for one global row.  Every figure is the median of --repeats runs after --warmup
(microseconds between two HIP events), with its spread.  There is no gate: the entries have no parent to compare with.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
N_UTTS, FRAMES, D, K = 64, 1000, 60, 3


def stat(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def timed(torch, fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(1e3 * a.elapsed_time(b))
    return stat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "r26_mlpg_variance_probe.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(HERE))
    import torch

    from magphase_amd import hostmath as hm
    from magphase_amd import magphase as mp
    from magphase_amd.engine import get_engine

    e = get_engine()
    w = hm.mlpg_windows(mp.MLPG_WINDOWS)
    wins = (ctypes.c_double * w.size)(*w.reshape(-1))
    total = N_UTTS * FRAMES
    f64 = dict(dtype=torch.float64, device=e.device)
    offs = e.to_device(np.arange(N_UTTS + 1, dtype=np.int32) * FRAMES, np.int32)
    torch.manual_seed(26)
    mean = torch.randn((total, K * D), device=e.device)
    x = mean[:, :D].contiguous() + 0.3 * torch.randn((total, D), device=e.device)
    g = torch.randn((total, D), **f64)
    go = torch.ones((N_UTTS, D), **f64)
    c, z = torch.empty((total, D), **f64), torch.empty((total, D), **f64)
    work = torch.empty(int(e.lib.mpx_mlpg_work_doubles(total, D)), **f64)
    nwork = torch.empty(int(e.lib.mpx_mlpg_nll_work_doubles(total, D)), **f64)
    cwork = torch.empty(int(e.lib.mpx_mlpg_colsum_work_doubles(total, K * D)), **f64)
    gm, gv = torch.empty((total, K * D), **f64), torch.empty((total, K * D), **f64)
    gsum, nll = torch.empty(K * D, **f64), torch.empty((N_UTTS, D), **f64)
    res = {"device": torch.cuda.get_device_name(e.device), "utterances": N_UTTS, "frames": FRAMES, "D": D,
           "warmup": a.warmup, "repeats": a.repeats}
    for name, var in (("per_frame", torch.rand((total, K * D), **f64) + 0.5), ("global", torch.rand(K * D, **f64) + 0.5)):
        ld_v = 0 if var.dim() == 1 else K * D
        e.mlpg_solve(mean, var, offs, D, w, out=c, work=work)
        e.mlpg_solve(g, var, offs, D, w, rhs=True, out=z, work=work)

        def nll_bwd(g_mean, g_var):
            e.launch("mpx_mlpg_trajectory_nll_backward", mean, 0, K * D, var, 1, ld_v, c, D, x, 0, D, go, offs, N_UTTS, total,
                     D, K - 1, wins, g_mean, K * D, g_var, K * D, nwork if g_var is not None else None)

        res[name] = {
            "solve_us": timed(torch, lambda: e.mlpg_solve(mean, var, offs, D, w, out=c, work=work), a.warmup, a.repeats),
            "var_backward_us": timed(torch, lambda: e.launch(
                "mpx_mlpg_var_backward", z, D, c, D, mean, 0, K * D, var, 1, ld_v, offs, N_UTTS, total, D, K - 1, wins, gv,
                K * D, gsum if ld_v == 0 else None, cwork if ld_v == 0 else None), a.warmup, a.repeats),
            "nll_us": timed(torch, lambda: e.launch(
                "mpx_mlpg_trajectory_nll", c, D, x, 0, D, var, 1, ld_v, offs, N_UTTS, total, D, K - 1, wins, nll),
                a.warmup, a.repeats),
            "nll_backward_us": timed(torch, lambda: nll_bwd(gm, gv), a.warmup, a.repeats),
            "nll_backward_means_only_us": timed(torch, lambda: nll_bwd(gm, None), a.warmup, a.repeats),
        }
        if ld_v == 0:
            res[name]["column_sums_us"] = timed(torch, lambda: e.launch("mpx_mlpg_column_sums", gv, K * D, total, K * D, gsum,
                                                                        cwork), a.warmup, a.repeats)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
