#!/usr/bin/env python
"""
How k_roundtrip_pair's slots finish, what their frames cost, and whether dealing the frames by that cost pays.

    python tools/roundtrip_deal_probe.py --prepare                 # HERE (needs hipcc): the probe build under tools/_ab/rtprobe
                                                                   # (python -m magphase_amd.build's -DMPX_PROBE_ENDTIME variant)
    python tools/roundtrip_deal_probe.py probe --out P.json        # on the GPU box: per-slot end times of one launch of the
                                                                   # bench batch (MAGPHASE_RT_DEAL=count for the shares by count)
    python tools/roundtrip_deal_probe.py fit P.json --out C.json   # anywhere: least squares per age class -> MPX_RT_COST_*
    python tools/roundtrip_deal_probe.py ab --out AB.txt           # on the GPU box, the DEFAULT build: count dealing against cost
                                                                   # dealing, interleaved in one process on shared buffers

probe: the probe build's waves store the 100 MHz clock at entry and exit of their frame loop (one tick = 10 ns).  A slot is
a wave pair; its busy time runs from the earlier start to the later end of its two waves.  Printed and stored: per slot
end, busy, frames, sum of gathered rows, sum of extra tiles, runs; the spread of the end times (max over mean) per age
class and per workgroup; the correlation of busy time with the row sum at a fixed age class.
fit: busy ~ a frames + b rows + c extra per age class (coefficients kept >= 0), rounded to integers of 10 ns.
ab: 17 rounds (the first 2 dropped), each round = both plans in turn, HIP events around rt.run (launch + fix-up).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
VARIANT = "rtprobe"
PAIRS_PER_GROUP = 6        # wave pairs of a 12-wave workgroup; pairs 0-1 / 2-3 / 4-5 hold the oldest / middle / youngest waves


def age_of(slot):
    return ((slot % PAIRS_PER_GROUP) * 2) // 4


def prepare():
    import ab_bench
    ab_bench.prepare(VARIANT, None, ["-DMPX_PROBE_ENDTIME"])


def _slot_tables(rt, hm, hostplan):
    """Per slot: frames, row sum, extra-tile sum, runs -- from the plan's run tables and the analysis plan's host tables."""
    tabs = rt.analysis._host_tabs
    terms = hm.roundtrip_frame_terms(tabs[1], tabs[2], rt.fft_len).astype(np.int64)
    cum = np.concatenate((np.zeros((1, 3), dtype=np.int64), np.cumsum(terms, axis=0)))
    runs = rt.synthesis.runs_host
    slot_off = rt.synthesis.slot_off.cpu().numpy().astype(np.int64)
    slot_runs = rt.synthesis.slot_runs.cpu().numpy().astype(np.int64)
    ns = slot_off.size - 1
    out = np.zeros((ns, 4), dtype=np.int64)
    for s in range(ns):
        for ci in slot_runs[slot_off[s]:slot_off[s + 1]]:
            fb, fe = int(runs[ci]["frame_begin"]), int(runs[ci]["frame_end"])
            out[s, :3] += cum[fe] - cum[fb]
            out[s, 3] += 1
    return out


def probe(args):
    import torch
    import ab_bench
    import bench
    em = ab_bench.load(VARIANT)
    pkg = sys.modules["mpa_" + VARIANT]
    hm, hostplan = pkg.hostmath, pkg.hostplan
    eng = em.Engine()
    utts = bench.make_batch(0)
    rt = em.LosslessRoundTripPlan(eng, utts)
    F, H = rt.total_frames, rt.fft_len // 2 + 1
    feats = tuple(eng.empty_feats(F, H) for _ in range(3))
    strips, pcm = eng.empty((max(rt.synthesis.strip_floats, 1),)), eng.empty((rt.total_out,))
    for _ in range(args.launches):     # (the first ~40 launches after idle run in the power transient: bench.py)
        rt.run(feats=feats, strips=strips, out=pcm)
    torch.cuda.synchronize()
    ns = int(rt.synthesis.n_slots)
    n_waves = 2 * ns
    buf = (ctypes.c_ulonglong * (4 * n_waves))()
    eng.lib.mpx_probe_rt_endtimes.argtypes = [ctypes.c_void_p, ctypes.c_int]
    assert eng.lib.mpx_probe_rt_endtimes(buf, 4 * n_waves) == 0
    a = np.frombuffer(buf, dtype=np.uint64).reshape(ns, 2, 4).astype(np.int64)
    tab = _slot_tables(rt, hm, hostplan)
    assert np.array_equal(a[:, :, 2].sum(axis=1), tab[:, 0]), "the waves' frame counts do not add up to the plan's"
    t0 = int(a[:, :, 0].min())
    start, end = a[:, :, 0].min(axis=1) - t0, a[:, :, 1].max(axis=1) - t0
    busy = end - start
    cyc = a[:, :, 3].max(axis=1)
    age = np.asarray([age_of(s) for s in range(ns)])
    rep = {"deal": rt.deal, "n_slots": ns, "frames": int(F), "launches": int(args.launches), "tick_ns": 10,
           "launch_ticks": int(end.max()), "end_max_over_mean": float(end.max() / end.mean()), "by_age": {}, "slots": {
               "end": end.tolist(), "busy": busy.tolist(), "frames": tab[:, 0].tolist(), "rows": tab[:, 1].tolist(),
               "extra": tab[:, 2].tolist(), "runs": tab[:, 3].tolist(), "shader_cycles": cyc.tolist()}}
    print("dealing: %s; %d slots, %d frames; launch (first start to last end) %.1f us; end max/mean %.4f"
          % (rt.deal, ns, F, end.max() / 100.0, rep["end_max_over_mean"]))
    for g in range(3):
        m = age == g
        r = float(np.corrcoef(busy[m], tab[m, 1])[0, 1]) if np.ptp(tab[m, 1]) > 0 else float("nan")
        rep["by_age"][str(g)] = {"slots": int(m.sum()), "end_mean": float(end[m].mean()), "end_max": int(end[m].max()),
                                 "end_max_over_mean": float(end[m].max() / end[m].mean()),
                                 "frames_min": int(tab[m, 0].min()), "frames_max": int(tab[m, 0].max()),
                                 "busy_per_frame_mean": float((busy[m] / np.maximum(tab[m, 0], 1)).mean()),
                                 "corr_busy_rows": r}
        print("  age %d: %4d slots, frames %d..%d, end mean %.1f us max %.1f us (max/mean %.4f), busy per frame %.2f us, "
              "corr(busy, rows) %.3f" % (g, m.sum(), tab[m, 0].min(), tab[m, 0].max(), end[m].mean() / 100.0,
                                         end[m].max() / 100.0, end[m].max() / end[m].mean(),
                                         (busy[m] / np.maximum(tab[m, 0], 1)).mean() / 100.0, r))
    wg_end = end[:ns // PAIRS_PER_GROUP * PAIRS_PER_GROUP].reshape(-1, PAIRS_PER_GROUP).max(axis=1)
    rep["workgroup_end_max_over_mean"] = float(wg_end.max() / wg_end.mean())
    rep["workgroup_end_mean_over_max"] = float(wg_end.mean() / wg_end.max())
    print("  workgroups: end mean %.1f us, max %.1f us (max/mean %.4f; the mean workgroup leaves its CU at %.3f of the launch)"
          % (wg_end.mean() / 100.0, wg_end.max() / 100.0, rep["workgroup_end_max_over_mean"], rep["workgroup_end_mean_over_max"]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rep, f)


def _nnls(X, y):
    """Least squares with the coefficients kept >= 0: the most negative one is dropped and the rest refitted."""
    keep = list(range(X.shape[1]))
    while True:
        c, *_ = np.linalg.lstsq(X[:, keep], y, rcond=None)
        if np.all(c >= 0) or len(keep) == 1:
            out = np.zeros(X.shape[1])
            out[keep] = np.maximum(c, 0)
            return out
        del keep[int(np.argmin(c))]


def fit(args):
    rep = json.load(open(args.probe))
    s = rep["slots"]
    busy = np.asarray(s["busy"], dtype=np.float64)
    X = np.stack([s["frames"], s["rows"], s["extra"]], axis=1).astype(np.float64)
    age = np.asarray([age_of(i) for i in range(busy.size)])
    out = {"source": {k: rep[k] for k in ("deal", "n_slots", "frames", "launches", "tick_ns", "launch_ticks",
                                          "end_max_over_mean", "workgroup_end_max_over_mean", "by_age")},
           "model": "slot busy time [10 ns] = a frames + b rows + c extra_tiles, per age class of the wave pair", "fit": {},
           "slots": s}
    for g in range(3):
        m = age == g
        c = _nnls(X[m], busy[m])
        res = busy[m] - X[m] @ c
        c_count = _nnls(X[m][:, :1], busy[m])
        res_count = busy[m] - X[m][:, :1] @ c_count
        ci = [int(round(v)) for v in c]
        share = [float((X[m][:, k] * c[k]).sum() / busy[m].sum()) for k in range(3)]
        out["fit"][str(g)] = {"a": ci[0], "b": ci[1], "c": ci[2], "float": c.tolist(), "rms_residual": float(np.sqrt((res ** 2).mean())),
                              "max_abs_residual": float(np.abs(res).max()), "rms_residual_frames_only": float(np.sqrt((res_count ** 2).mean())),
                              "a_frames_only": float(c_count[0]), "busy_mean": float(busy[m].mean()),
                              "share_of_busy_time": {"frames": share[0], "rows": share[1], "extra": share[2]}}
        print("age %d: a %d  b %d  c %d  (10 ns); rms residual %.0f (frames only: %.0f) of mean busy %.0f; rows %.1f %% and extra "
              "tiles %.1f %% of the busy time" % (g, ci[0], ci[1], ci[2], out["fit"][str(g)]["rms_residual"],
                                                out["fit"][str(g)]["rms_residual_frames_only"], busy[m].mean(),
                                                100 * share[1], 100 * share[2]))
    print("flags: " + " ".join("-DMPX_RT_COST_%s%d=%d" % (k.upper(), g, out["fit"][str(g)][k]) for g in range(3) for k in "abc"))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f)


def ab(args):
    import torch
    import bench
    from magphase_amd import engine as em
    eng = em.get_engine()
    utts = bench.make_batch(0)
    plans = {}
    for name in ("count", "cost"):      # (MAGPHASE_RT_COSTS, if set, gives the cost plan other coefficients than the library's)
        if name == "count":
            os.environ["MAGPHASE_RT_DEAL"] = "count"
        else:
            os.environ.pop("MAGPHASE_RT_DEAL", None)
        plans[name] = em.LosslessRoundTripPlan(eng, utts)
        assert plans[name].deal == name, (name, plans[name].deal)
    os.environ.pop("MAGPHASE_RT_DEAL", None)
    F, H = plans["cost"].total_frames, plans["cost"].fft_len // 2 + 1
    feats = tuple(eng.empty_feats(F, H) for _ in range(3))        # shared by both plans: same addresses, same channels
    strips = eng.empty((max(p.synthesis.strip_floats for p in plans.values()),))
    pcm = eng.empty((plans["cost"].total_out,))
    ref = {}
    for name, p in plans.items():
        p.run(feats=feats, strips=strips, out=pcm)
        torch.cuda.synchronize()
        ref[name] = ([t.clone() for t in feats], pcm.clone())
    same_rows = all(bool(torch.equal(x, y)) for x, y in zip(ref["count"][0], ref["cost"][0]))
    d_pcm = float((ref["count"][1] - ref["cost"][1]).abs().max() / ref["count"][1].abs().max())
    for _ in range(64):     # out of the post-idle power transient (bench.py)
        plans["count"].run(feats=feats, strips=strips, out=pcm)
    ms = {"count": [], "cost": []}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rnd in range(args.rounds):
        for name in (("count", "cost") if rnd % 2 == 0 else ("cost", "count")):
            p = plans[name]
            for _ in range(5):
                p.run(feats=feats, strips=strips, out=pcm)
            e0.record()
            for _ in range(args.steps):
                p.run(feats=feats, strips=strips, out=pcm)
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / args.steps)
    costs = os.environ.get("MAGPHASE_RT_COSTS") or "the library's (mpx_roundtrip_slot_costs)"
    lines = ["cost coefficients: %s" % costs, "interleaved A/B of LosslessRoundTripPlan.run (launch + fix-up) on the bench batch, shared feature / strip / output "
             "buffers, %d rounds of %d steps per plan (first %d rounds dropped), HIP events" % (args.rounds, args.steps, args.drop),
             "feature rows bit-identical: %s; waveforms differ by %.3g of the peak" % (same_rows, d_pcm)]
    kept = {k: v[args.drop:] for k, v in ms.items()}
    for name in ("count", "cost"):
        v = kept[name]
        lines.append("%-5s  runs %d  slots %d  median %.4f ms  min %.4f  max %.4f   rounds: %s"
                     % (name, plans[name].synthesis.n_runs, plans[name].synthesis.n_slots, statistics.median(v), min(v), max(v),
                        " ".join("%.4f" % x for x in v)))
    mc, mk = statistics.median(kept["count"]), statistics.median(kept["cost"])
    lines.append("cost / count (medians): %.4f  (%+.2f %% of the step); slowest cost round %.4f ms vs median count %.4f ms"
                 % (mk / mc, 100 * (mk - mc) / mc, max(kept["cost"]), mc))
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--prepare", action="store_true")
    sub = ap.add_subparsers(dest="cmd")
    p = sub.add_parser("probe")
    p.add_argument("--out")
    p.add_argument("--launches", type=int, default=80)
    p = sub.add_parser("fit")
    p.add_argument("probe")
    p.add_argument("--out")
    p = sub.add_parser("ab")
    p.add_argument("--out")
    p.add_argument("--rounds", type=int, default=17)
    p.add_argument("--drop", type=int, default=2)
    p.add_argument("--steps", type=int, default=40)
    args = ap.parse_args()
    if args.prepare:
        return prepare()
    if args.cmd is None:
        ap.error("nothing to do")
    {"probe": probe, "fit": fit, "ab": ab}[args.cmd](args)


if __name__ == "__main__":
    main()
