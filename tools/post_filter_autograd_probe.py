#!/usr/bin/env python
"""
What the backward passes of the two post-filters cost beside their forwards (64 utterances x 1000 rows, D = 60, 48 kHz):
one JSON under profiles/.

    python tools/post_filter_autograd_probe.py

  magphase   Engine.post_filter (k_post_filter) and Engine.post_filter_backward (k_post_filter_bwd) on the packed
             float32 [64000 x 60] rows
  merlin     Engine.post_filter_merlin (k_rows_gemm, k_merlin_r0, k_merlin_b, k_rows_gemm) and
             Engine.post_filter_merlin_backward (k_rows_gemm twice, k_merlin_r0_bwd, k_rows_gemm)
  one bin    the two Merlin C entries with ONE bin of G: the k_rows_gemm launches and the fixed parts -- what is left of the
             full figures is the chunk loop of k_merlin_r0 / k_merlin_r0_bwd
  batch      mp.post_filter_batch(..., return_device=True) on the 64 device matrices under grad, and backward() of a sum
             over its outputs (packing, autograd bookkeeping and the per-utterance gradient views included)

Every figure is the median of --repeats runs after --warmup (microseconds between two HIP events), with its spread.  The
backward of the Merlin filter does the forward's [F x D] . [D x 2049] product once more plus a transposed product of the
same size: at least twice the arithmetic of k_merlin_r0; `backward_over_forward` is the measured ratio of the two entries.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
N_UTTS, FRAMES, DIM, FS = 64, 1000, 60, 48000


def stat(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def timed(torch, fn, warmup, repeats, before=None):
    out = []
    for i in range(warmup + repeats):
        arg = before() if before else None
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn(arg) if before else fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append(1e3 * a.elapsed_time(b))
    return stat(out)


def rows(rng, n):
    """Log mel magnitudes with three formants per row (the generator of the post-filter tests)."""
    k = np.arange(DIM)[None, :]
    f1, f2, f3 = rng.uniform(4, 12, (n, 1)), rng.uniform(15, 28, (n, 1)), rng.uniform(32, 50, (n, 1))
    env = -0.04 * k + 2.2 * np.exp(-0.5 * ((k - f1) / 2.0) ** 2) + 1.6 * np.exp(-0.5 * ((k - f2) / 2.5) ** 2) \
        + 1.0 * np.exp(-0.5 * ((k - f3) / 3.0) ** 2)
    return (env + rng.uniform(-6, -2, (n, 1))).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "r24_post_filter_autograd_probe.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(HERE))
    import torch

    from magphase_amd import hostmath as hm
    from magphase_amd import libaudio as la
    from magphase_amd import magphase as mp
    from magphase_amd.engine import get_engine

    e = get_engine()
    rng = np.random.RandomState(24)
    total = N_UTTS * FRAMES
    x = torch.from_numpy(rows(rng, total)).to(e.device)
    g = torch.randn((total, DIM), device=e.device)
    res = {"device": torch.cuda.get_device_name(e.device), "utterances": N_UTTS, "frames": FRAMES, "dim": DIM, "fs": FS,
           "warmup": a.warmup, "repeats": a.repeats}
    entries = {"magphase": (lambda: e.post_filter(x, FS), lambda: e.post_filter_backward(g, FS)),
               "merlin": (lambda: e.post_filter_merlin(x, FS), lambda: e.post_filter_merlin_backward(x, g, FS))}
    for name, (fwd, bwd) in entries.items():
        r = {"forward_us": timed(torch, fwd, a.warmup, a.repeats), "backward_us": timed(torch, bwd, a.warmup, a.repeats)}
        r["backward_over_forward"] = r["backward_us"]["median"] / r["forward_us"]["median"]
        res[name] = r
    # where the Merlin time goes: the same entries with ONE bin of G -- the k_rows_gemm launches (and k_merlin_b) plus the
    # fixed part of k_merlin_r0 / k_merlin_r0_bwd; the rest of the full figure is the 33 chunks of the energy kernels
    t = hm.merlin_tables(DIM, FS, 1.4)
    d = {k: e.to_device(v, np.float32) for k, v in dict(t, cf_t=t["cf"].T, c1_t=t["c1"].T).items() if k != "alpha"}
    w5 = [e.empty((total, DIM)) for _ in range(5)]
    r2 = [e.empty((total,)) for _ in range(2)]
    res["merlin"]["forward_one_bin_us"] = timed(torch, lambda: e.launch(
        "mpx_post_filter_merlin", x, total, DIM, d["c1"], d["lifter"], d["g"], d["wk"], 1, float(t["alpha"]), d["cf"],
        float(la.MAGIC), w5[0], w5[1], r2[0], r2[1], w5[2]), a.warmup, a.repeats)
    res["merlin"]["backward_one_bin_us"] = timed(torch, lambda: e.launch(
        "mpx_post_filter_merlin_backward", x, g, total, DIM, d["c1"], d["lifter"], d["g"], d["wk"], 1, d["cf_t"],
        d["c1_t"], *w5), a.warmup, a.repeats)
    mats = [x[u * FRAMES:(u + 1) * FRAMES].clone().requires_grad_(True) for u in range(N_UTTS)]
    for name in entries:
        def forward():
            return mp.post_filter_batch(mats, FS, pf_type=name, return_device=True)

        def loss():
            return torch.cat(forward()).sum()

        res[name]["batch_forward_us"] = timed(torch, forward, a.warmup, a.repeats)
        res[name]["batch_backward_us"] = timed(torch, lambda l: l.backward(), a.warmup, a.repeats, before=loss)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
