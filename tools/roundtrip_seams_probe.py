#!/usr/bin/env python
"""
Whether sizing the round-trip plan's run seams by what the frames add (the default) pays against the seams of dense
frames (MAGPHASE_RT_SEAMS=full), on the bench batch.

    python tools/roundtrip_seams_probe.py ab --out AB.txt      # on the GPU box

Both plans are built in one process and run in turn on shared feature / strip / output buffers, the scheme of
tools/roundtrip_deal_probe.py ab: 17 rounds (the first 2 dropped) of 40 steps per plan, HIP events around rt.run (launch +
fix-up), the order of the two alternating from round to round.  Printed: the fix-up's element totals of both run tables
(12 bytes per element: strip read, pcm_out read and written), whether the outputs are equal, the rounds, and the verdict
-- a gain only if every round of the new seams is faster than every round of the old and the medians differ by more than
three times the larger spread (max - min over the median) of the two.
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def seam_stats(runs):
    """Elements the fix-up moves, and the ranges as k_ola_fixup walks them (from fix_lo's 64-element block to fix_hi)."""
    n = (runs["fix_hi"] - runs["fix_lo"]).astype(np.int64)
    n = n[n > 0]
    head = runs["head_end"].astype(np.int64)
    return dict(runs=int(runs.size), seams=int(n.size), elements=int(n.sum()), mean=float(n.mean()) if n.size else 0.0,
                median=float(np.median(n)) if n.size else 0.0, max=int(n.max()) if n.size else 0,
                over_1024=int((n > 1024).sum()), strip_elements=int(head.sum()),
                flush_elements=int(runs["flush_end"].astype(np.int64).sum()))


def ab(args):
    import torch
    import bench
    from magphase_amd import engine as em
    eng = em.get_engine()
    utts = bench.make_batch(0)
    plans = {}
    for name in ("full", "extents"):
        if name == "full":
            os.environ["MAGPHASE_RT_SEAMS"] = "full"
        else:
            os.environ.pop("MAGPHASE_RT_SEAMS", None)
        plans[name] = em.LosslessRoundTripPlan(eng, utts)
        assert plans[name].full_seams == (name == "full")
    os.environ.pop("MAGPHASE_RT_SEAMS", None)
    pa, pb = plans["full"], plans["extents"]
    F, H = pb.total_frames, pb.fft_len // 2 + 1
    feats = tuple(eng.empty_feats(F, H) for _ in range(3))        # shared by both plans: same addresses, same channels
    strips = eng.empty((max(p.synthesis.strip_floats for p in plans.values()),))
    pcm = eng.empty((pb.total_out,))
    ref = {}
    for name, p in plans.items():
        strips.fill_(float("nan"))
        pcm.fill_(float("nan"))
        p.run(feats=feats, strips=strips, out=pcm)
        torch.cuda.synchronize()
        ref[name] = ([t.clone() for t in feats], pcm.clone())
    same_rows = all(bool(torch.equal(x.view(torch.int32), y.view(torch.int32))) for x, y in zip(ref["full"][0], ref["extents"][0]))
    same_pcm = bool(torch.equal(ref["full"][1] + 0.0, ref["extents"][1] + 0.0))
    nan = int(torch.isnan(ref["extents"][1]).sum())
    for _ in range(64):     # out of the post-idle power transient (bench.py)
        pa.run(feats=feats, strips=strips, out=pcm)
    ms = {"full": [], "extents": []}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rnd in range(args.rounds):
        for name in (("full", "extents") if rnd % 2 == 0 else ("extents", "full")):
            p = plans[name]
            for _ in range(5):
                p.run(feats=feats, strips=strips, out=pcm)
            e0.record()
            for _ in range(args.steps):
                p.run(feats=feats, strips=strips, out=pcm)
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / args.steps)
    lines = ["interleaved A/B of LosslessRoundTripPlan.run (launch + fix-up) on the bench batch (%d utterances, %d frames), "
             "shared feature / strip / output buffers, %d rounds of %d steps per plan (first %d rounds dropped), HIP events"
             % (len(utts), F, args.rounds, args.steps, args.drop),
             "dealing: %s / %s; same cuts: %s" % (pa.deal, pb.deal, bool(np.array_equal(
                 pa.runs_host["frame_begin"], pb.runs_host["frame_begin"]))),
             "outputs on NaN-filled pcm_out and strips: feature rows bit-identical: %s; pcm_out equal value for value: %s; "
             "NaN left in pcm_out: %d" % (same_rows, same_pcm, nan)]
    for name in ("full", "extents"):
        s = seam_stats(plans[name].runs_host)
        lines.append("%-7s run table: %d runs, %d seams, fix-up elements %d (%.1f MB at 12 B), per seam mean %.0f median %.0f "
                     "max %d, %d seams > 1024; head-strip elements %d; flushed elements %d; fix width %s"
                     % (name, s["runs"], s["seams"], s["elements"], 12e-6 * s["elements"], s["mean"], s["median"], s["max"],
                        s["over_1024"], s["strip_elements"], s["flush_elements"],
                        getattr(plans[name].seams, "fix_width", "(dense: N + 127)")))
    kept = {k: v[args.drop:] for k, v in ms.items()}
    spread = {}
    for name in ("full", "extents"):
        v = kept[name]
        spread[name] = (max(v) - min(v)) / statistics.median(v)
        lines.append("%-7s median %.4f ms  min %.4f  max %.4f  spread %.2f %%   rounds: %s"
                     % (name, statistics.median(v), min(v), max(v), 100 * spread[name], " ".join("%.4f" % x for x in v)))
    ma, mb = statistics.median(kept["full"]), statistics.median(kept["extents"])
    diff = (ma - mb) / ma
    every = max(kept["extents"]) < min(kept["full"])
    enough = diff > 3 * max(spread.values())
    lines.append("extents / full (medians): %.4f  (%+.2f %% of the step, %+.1f us)" % (mb / ma, -100 * diff, 1e3 * (mb - ma)))
    lines.append("every extents round faster than every full round: %s; difference %.2f %% against 3 x the larger spread "
                 "%.2f %%: %s  ->  %s" % (every, 100 * diff, 300 * max(spread.values()), enough,
                                           "a gain" if every and enough else "NOT a gain by the stated criterion"))
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd")
    p = sub.add_parser("ab")
    p.add_argument("--out")
    p.add_argument("--rounds", type=int, default=17)
    p.add_argument("--drop", type=int, default=2)
    p.add_argument("--steps", type=int, default=40)
    args = ap.parse_args()
    if args.cmd is None:
        ap.error("nothing to do")
    ab(args)


if __name__ == "__main__":
    main()
