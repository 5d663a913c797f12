#!/usr/bin/env python
"""
What MLPG costs beside the synthesis it feeds (64 utterances x 1000 frames of 5 ms, 60 / 10 / 10 / 1 coefficients, 48 kHz):
one JSON under profiles/.

    python tools/mlpg_probe.py

  solve     ONE mpx_mlpg_solve launch (k_mlpg_solve: one lane per (utterance, dimension), two dynamic windows, float32
            means, one global float64 variance row) at D = 60, 10 and 1, HIP events
  streams   mp.mlpg_streams_batch(..., return_device=True) on the [1000 x 244] device matrices: the four launches, the
            packing and the voicing threshold
  synthesis the forward of mp.synthesis_from_compressed_batch(..., b_const_rate=True, noise_mode='device',
            return_device=True) on the trajectories of that batch

Every figure is the median of --repeats runs after --warmup (microseconds between two HIP events), with its spread.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
N_UTTS, FRAMES, FS = 64, 1000, 48000
LAYOUT = (("mag", 60), ("real", 10), ("imag", 10), ("lf0", 1))


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


def cmp_rows(mp, rng):
    """One utterance's [FRAMES x 244] float32 rows: consistent static / delta / acc means of smooth trajectories."""
    t = np.arange(FRAMES)[:, None] / 200.0
    stat_cols = [-3.0 + 0.5 * np.sin(2 * np.pi * (0.7 + rng.rand(1, 60)) * t + rng.rand(1, 60)),
                 0.4 * np.sin(2 * np.pi * rng.rand(1, 10) * t), 0.4 * np.cos(2 * np.pi * rng.rand(1, 10) * t),
                 np.log(150.0) + 0.1 * np.sin(2 * np.pi * 0.5 * t)]
    voiced = ((np.arange(FRAMES) // 100) % 3 != 2).astype(np.float64)[:, None]
    return stat_cols, voiced


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "r21_mlpg_probe.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(HERE))
    import torch

    from magphase_amd import hostmath as hm
    from magphase_amd import magphase as mp
    from magphase_amd.engine import get_engine

    e = get_engine()
    rng = np.random.RandomState(21)
    w = hm.mlpg_windows(mp.MLPG_WINDOWS)
    K = 3
    res = {"device": torch.cuda.get_device_name(e.device), "utterances": N_UTTS, "frames": FRAMES, "warmup": a.warmup,
           "repeats": a.repeats, "solve_us": {}}
    total = N_UTTS * FRAMES
    offs = e.to_device(np.arange(N_UTTS + 1, dtype=np.int32) * FRAMES, np.int32)
    for D in (60, 10, 1):
        mean = torch.randn((total, K * D), device=e.device)
        var = torch.rand(K * D, dtype=torch.float64, device=e.device) + 0.5
        out = torch.empty((total, D), dtype=torch.float64, device=e.device)
        work = torch.empty(int(e.lib.mpx_mlpg_work_doubles(total, D)), dtype=torch.float64, device=e.device)
        res["solve_us"]["D%d" % D] = timed(torch, lambda: e.mlpg_solve(mean, var, offs, D, w, out=out, work=work),
                                           a.warmup, a.repeats)
    # the whole chain on one batch
    stat_cols, voiced = cmp_rows(mp, rng)
    dyn = [mp.dynamic_features(s) for s in stat_cols]
    row = np.concatenate(dyn + [voiced], axis=1).astype(np.float32)
    cmps = [torch.from_numpy(row).to(e.device) for _ in range(N_UTTS)]
    var = np.full(row.shape[1], 0.1)
    res["streams_us"] = timed(torch, lambda: mp.mlpg_streams_batch(cmps, var, return_device=True), a.warmup, a.repeats)
    utts = mp.mlpg_streams_batch(cmps, var, return_device=True)
    kw = dict(b_const_rate=True, noise_mode="device", return_device=True)
    res["synthesis_forward_us"] = timed(torch, lambda: mp.synthesis_from_compressed_batch(utts, FS, **kw), a.warmup,
                                        a.repeats)
    res["solve_D60_over_synthesis_forward"] = res["solve_us"]["D60"]["median"] / res["synthesis_forward_us"]["median"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
