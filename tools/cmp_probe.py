#!/usr/bin/env python
"""
What the acoustic composition costs (64 utterances x 1000 frames, the default layout 60 / 10 / 10 / 1, two windows, a
voicing column, norm): one JSON under profiles/.

    python tools/cmp_probe.py

  kernels    each C entry of magphase_cmp.hip alone on the packed [64000 x 81] float32 statics, HIP events: microseconds
             and bytes per second over the bytes the entry reads and writes (counted from the shapes below, not measured)
  compose    the whole mp.acoustic_compose_batch(..., norm=..., return_device=True) call on device tensors
  pieces     the same rows assembled from what the project had before: four mp.dynamic_features_batch launches (float64)
             plus torch for the lf0 interpolation (searchsorted over the voiced frames), the voicing column, the
             concatenation, the normalisation and the cast to float32

compose and pieces are timed in ONE process, alternating, between two HIP events around each call.  Every figure is the
median of --repeats runs after --warmup, with its spread.  No figure is fixed in advance; without a GPU the script fails.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
N_UTTS, FRAMES = 64, 1000
DIMS = (60, 10, 10, 1)


def stat(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def once(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b)


def timed(torch, fns, warmup, repeats):
    """The functions in turn, alternating -> one stat per function."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    out = [[] for _ in fns]
    for _ in range(repeats):
        for k, fn in enumerate(fns):
            out[k].append(once(torch, fn))
    return [stat(o) for o in out]


def pieces(torch, mp, feats, mean, std):
    """Today's pieces: the rows of acoustic_compose_batch without its kernels."""
    lf0 = [f[3].double() for f in feats]
    carried = []
    for v in lf0:
        F = v.numel()
        t = torch.arange(F, device=v.device)
        vi = torch.nonzero(v > 0)[:, 0]
        if vi.numel() == 0:
            carried.append(torch.zeros_like(v)[:, None])
            continue
        hi = torch.searchsorted(vi, t).clamp(max=vi.numel() - 1)
        lo = (torch.searchsorted(vi, t, right=True) - 1).clamp(min=0)
        p, n = vi[lo], vi[hi]
        span = (n - p).clamp(min=1).double()
        val = (v[n] - v[p]) / span * (t - p).double() + v[p]
        val = torch.where(t < vi[0], v[vi[0]], torch.where(t > vi[-1], v[vi[-1]], val))
        carried.append(val[:, None])
    dyn = [mp.dynamic_features_batch([f[s] for f in feats], return_device=True) for s in range(3)]
    dyn.append(mp.dynamic_features_batch(carried, return_device=True))
    rows = []
    for u, v in enumerate(lf0):
        y = torch.cat([dyn[0][u], dyn[1][u], dyn[2][u], dyn[3][u], (v > 0).double()[:, None]], 1)
        rows.append(((y - mean) / std).float())
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "r30_cmp_probe.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(HERE))
    import torch

    from magphase_amd import hostmath as hm
    from magphase_amd import magphase as mp
    from magphase_amd.engine import get_engine

    e = get_engine()
    rng = np.random.RandomState(30)
    w = hm.mlpg_windows(mp.MLPG_WINDOWS)
    total, SD, W = N_UTTS * FRAMES, sum(DIMS), 3 * sum(DIMS) + 1
    feats = []
    for _ in range(N_UTTS):
        lf0 = (np.log(150.0) + 0.1 * rng.randn(FRAMES)).astype(np.float32)
        lf0[((np.arange(FRAMES) + rng.randint(100)) // 100) % 3 == 2] = -1e10
        feats.append(tuple(torch.from_numpy(rng.randn(FRAMES, d).astype(np.float32)).to(e.device) for d in DIMS[:3])
                     + (torch.from_numpy(lf0).to(e.device),))
    mean = torch.from_numpy(rng.randn(W)).to(e.device)
    std = torch.from_numpy(np.exp(rng.randn(W))).to(e.device)
    dims = list(DIMS)
    x, offs = e.cmp_pack([[f[0], f[1], f[2], f[3][:, None]] for f in feats], dims)
    offs_dev = e.to_device(offs.astype(np.int32), np.int32)
    nb = e.cmp_neighbours(x[:, 80], offs_dev)
    out = torch.empty((total, W), dtype=torch.float32, device=e.device)
    g = torch.randn((total, W), dtype=torch.float32, device=e.device)
    mom = torch.zeros(1 + 2 * W, dtype=torch.float64, device=e.device)
    n_tiles = (total + 127) // 128
    # bytes each entry reads and writes, from the shapes (every operand counted once; the tap re-reads of neighbouring
    # rows and the neighbour table's re-reads are served by the caches)
    nbytes = {
        "mpx_cmp_voiced_neighbours": 2 * total * 4 + 2 * total * 4,                  # the lf0 column twice, two int32 planes
        "mpx_cmp_compose": total * SD * 4 + 2 * total * 4 + total * W * 4 + 2 * W * 8,
        "mpx_cmp_compose_backward": total * W * 4 + 2 * total * 4 + total * SD * 8 + W * 8,
        "mpx_cmp_column_moments": 2 * total * W * 4 + 4 * n_tiles * W * 8 + (1 + 2 * W) * 8,
    }
    calls = {
        "mpx_cmp_voiced_neighbours": lambda: e.cmp_neighbours(x[:, 80], offs_dev, out=nb),
        "mpx_cmp_compose": lambda: e.cmp_compose(x, nb, offs_dev, dims, 3, True, w, norm=(mean, std), out=out),
        "mpx_cmp_compose_backward": lambda: e.cmp_compose_backward(g, nb, offs_dev, dims, 3, True, w, std=std),
        "mpx_cmp_column_moments": lambda: e.cmp_column_moments(out, out=mom),
    }
    res = {"device": torch.cuda.get_device_name(e.device), "utterances": N_UTTS, "frames": FRAMES, "dims": dims,
           "width": W, "warmup": a.warmup, "repeats": a.repeats, "kernels": {}}
    for name, fn in calls.items():
        st = timed(torch, [fn], a.warmup, a.repeats)[0]
        res["kernels"][name] = {"us": st, "bytes": nbytes[name], "GB_per_s": nbytes[name] / (st["median"] * 1e-6) / 1e9}
    kw = dict(norm=(mean, std), return_device=True)
    whole, old = timed(torch, [lambda: mp.acoustic_compose_batch(feats, **kw),
                               lambda: pieces(torch, mp, feats, mean, std)], a.warmup, a.repeats)
    res["acoustic_compose_batch_us"] = whole
    res["pieces_us"] = old
    res["pieces_over_compose"] = old["median"] / whole["median"]
    got = torch.cat(mp.acoustic_compose_batch(feats, **kw)).double()
    ref = torch.cat(pieces(torch, mp, feats, mean, std)).double()
    res["max_abs_difference_compose_vs_pieces"] = float((got - ref).abs().max())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
