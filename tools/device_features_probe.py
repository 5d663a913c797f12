#!/usr/bin/env python
"""
What device-resident features buy on the generation launch (128 utterances x 5 s at 48 kHz, constant frame rate,
60 / 45 / 45 coefficients): one JSON under profiles/.

    python tools/device_features_probe.py                       # pack kernel + call times, this tree
    python tools/device_features_probe.py --ab PATH_TO_PARENT   # + the host-input call, this tree against another tree

  pack      k_rows_pack (one mpx_rows_pack launch on a prebuilt table: column slices of 128 [F x 151] tensors) against a
            contiguous device-to-device copy_ of the same number of output bytes, HIP events, alternated
  call      synthesis_from_compressed_batch(..., noise_mode='device', return_device=True): device inputs (float32 and
            bfloat16 column slices) against contiguous float32 host arrays, alternated; host clock around the call ended
            by a synchronise, HIP events for the device side
  host_ab   the host-input call with pcm16_norm=0.98 (an interface both trees have), in fresh child processes, the two
            trees taking turns

Every figure is the median of --repeats runs after --warmup; the spread (min, max) is reported beside it.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
N_UTTS, DUR_S, FS, MAG, PH, POOL = 128, 5.0, 48000, 60, 45, 16


def stat(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def workload(mp, syn):
    """[F x 151] float32 host matrices of the launch's utterances (a pool of analysed synthetic utterances, repeated)."""
    utts = []
    for u in range(POOL):
        pcm, pm, voi = syn.make_utterance(9000 + u, dur_s=DUR_S, fs=FS)
        utts.append((pcm, FS, pm, voi))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = mp.analysis_compressed_batch(utts, mag_dim=MAG, phase_dim=PH, b_const_rate=True, as_float32=True)
    wide = [np.ascontiguousarray(np.concatenate([r[0], r[1], r[2], np.asarray(r[3], np.float32)[:, None]], axis=1))
            for r in res]
    return [wide[u % POOL] for u in range(N_UTTS)]


def slices(w):
    return w[:, :MAG], w[:, MAG:MAG + PH], w[:, MAG + PH:MAG + 2 * PH], w[:, MAG + 2 * PH]


def timed_call(torch, fn):
    """(host seconds around fn() ended by a synchronise, device seconds between two events around it)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, a.elapsed_time(b) * 1e-3


def alternate(torch, fns, warmup, repeats):
    """fns: {name: callable}; the callables take turns.  -> {name: {"call_ms": stat, "device_ms": stat}}"""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    acc = {k: ([], []) for k in fns}
    for _ in range(repeats):
        for k, f in fns.items():
            h, d = timed_call(torch, f)
            acc[k][0].append(1e3 * h)
            acc[k][1].append(1e3 * d)
    return {k: {"call_ms": stat(v[0]), "device_ms": stat(v[1])} for k, v in acc.items()}


def probe(tree, mode, warmup, repeats):
    sys.path.insert(0, tree)
    import torch

    from magphase_amd import hostmath as hm
    from magphase_amd import magphase as mp
    from magphase_amd import synthetic as syn
    from magphase_amd.engine import get_engine

    e = get_engine()
    wide = workload(mp, syn)
    host = [tuple(np.ascontiguousarray(x) for x in slices(w)) for w in wide]
    rows = int(sum(w.shape[0] for w in wide))
    out = {"tree": os.path.abspath(tree), "device": torch.cuda.get_device_name(e.device), "utterances": N_UTTS,
           "rows": rows, "coef_bytes": 4 * rows * (MAG + 2 * PH), "warmup": warmup, "repeats": repeats}
    kw = dict(b_const_rate=True, noise_mode="device")
    if mode == "host":   # the interface every tree has
        out["host_pcm16"] = alternate(torch, {"host": lambda: mp.synthesis_from_compressed_batch(host, FS, pcm16_norm=0.98, **kw)},
                                      warmup, repeats)["host"]
        return out
    dev32 = [torch.from_numpy(w).to(e.device) for w in wide]
    dev16 = [t.bfloat16() for t in dev32]
    d32 = [slices(t) for t in dev32]
    d16 = [slices(t)[:3] + (slices(s)[3],) for t, s in zip(dev16, dev32)]
    # --- the kernel alone, on a prebuilt table, against copy_ of the same output bytes
    n_m, n_p = rows * MAG, rows * PH
    coef = e.empty((n_m + 2 * n_p,))
    src = torch.randn(n_m + 2 * n_p, device=e.device)
    outs = [coef[:n_m].view(rows, MAG), coef[n_m:n_m + n_p].view(rows, PH), coef[n_m + n_p:].view(rows, PH)]
    pack = {}
    for name, utts in (("float32", d32), ("bfloat16", d16)):
        table, widths, nrows = hm.rows_pack_table([[u[k] for u in utts] for k in range(3)])
        d_table = e.to_device(table.view(np.uint8), np.uint8)
        args = []
        for o, w, n in zip(outs, widths, nrows):
            args += [o, w, w, n]

        def launch(d_table=d_table, table=table, args=args):
            e.launch("mpx_rows_pack", d_table, table.ctypes.data, N_UTTS, 3, *args)

        r = alternate(torch, {"pack": launch, "copy": lambda: coef.copy_(src)}, warmup, 4 * repeats)
        pack[name] = {"pack_us": {k: 1e3 * v for k, v in r["pack"]["device_ms"].items() if k != "n"},
                      "copy_us": {k: 1e3 * v for k, v in r["copy"]["device_ms"].items() if k != "n"},
                      "ratio": r["pack"]["device_ms"]["median"] / r["copy"]["device_ms"]["median"]}
    out["pack"] = pack
    # --- the whole call
    fns = {"device_float32": lambda: mp.synthesis_from_compressed_batch(d32, FS, return_device=True, **kw),
           "device_bfloat16": lambda: mp.synthesis_from_compressed_batch(d16, FS, return_device=True, **kw),
           "host_float32": lambda: mp.synthesis_from_compressed_batch(host, FS, return_device=True, **kw)}
    out["call"] = alternate(torch, fns, warmup, repeats)
    c = out["call"]
    out["call"]["host_minus_device_float32_ms"] = c["host_float32"]["call_ms"]["median"] - c["device_float32"]["call_ms"]["median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(HERE))
    ap.add_argument("--mode", default="all", choices=("all", "host"))
    ap.add_argument("--ab", default=None, help="another tree (the parent commit, built): host-input call in turns")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "r10_device_features_probe.json"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        print("PROBE_JSON " + json.dumps(probe(a.tree, a.mode, a.warmup, a.repeats)), flush=True)
        return
    res = probe(a.tree, a.mode, a.warmup, a.repeats)
    if a.ab:
        ab = {"this": [], "other": []}
        for _ in range(a.rounds):
            for key, tree in (("other", a.ab), ("this", a.tree)):   # fresh processes, the trees taking turns
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--mode", "host", "--tree", tree,
                       "--warmup", str(a.warmup), "--repeats", str(a.repeats)]
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
                if p.returncode != 0:
                    raise RuntimeError("child failed (%d): %s" % (p.returncode, p.stderr[-2000:]))
                line = [l for l in p.stdout.splitlines() if l.startswith("PROBE_JSON ")][-1]
                ab[key].append(json.loads(line[len("PROBE_JSON "):])["host_pcm16"]["call_ms"])
        res["host_ab"] = {"other_tree": os.path.abspath(a.ab),
                          "this_ms": stat([r["median"] for r in ab["this"]]), "other_ms": stat([r["median"] for r in ab["other"]]),
                          "this_runs": ab["this"], "other_runs": ab["other"]}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
