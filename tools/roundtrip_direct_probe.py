#!/usr/bin/env python
"""
Whether overlap-adding the windowed frame directly pays in the round-trip launch (MAGPHASE_RT_INVERSE=direct | transform;
csrc/magphase_comp.hip, k_roundtrip_pair's DIRECT), on the bench batch.  On the GPU box:

    python tools/roundtrip_direct_probe.py ab     --out AB.txt      # interleaved timing of the two arms
    python tools/roundtrip_direct_probe.py energy --out ENERGY.txt  # joules per step above idle of the two arms

ab      both plans are built in one process and run in turn on shared feature / strip / output buffers (the scheme of
        tools/roundtrip_stores_probe.py ab): 17 rounds (the first 2 dropped) of 40 steps per plan, HIP events around rt.run
        (launch + fix-up), the order alternating from round to round.  direct is a gain only if every one of its rounds beats
        every round of transform and the medians differ by more than three times the larger spread (max - min over the
        median).  Before the timing: rows bit-identical between the arms, the largest waveform difference of the peak.
energy  each plan loops for ~2.5 s under the power sampler of tools/energy_probe.py: ms, W, J per step, J above idle.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from roundtrip_stores_probe import emit, power_files  # noqa: E402

ARMS = ("transform", "direct")


def build_plans(em, eng, utts):
    plans = {}
    for name in ARMS:
        os.environ["MAGPHASE_RT_INVERSE"] = name
        plans[name] = em.LosslessRoundTripPlan(eng, utts)
        assert plans[name].inverse == name
    os.environ.pop("MAGPHASE_RT_INVERSE", None)
    return plans


def shared_buffers(eng, plans):
    p = plans["transform"]
    F, H = p.total_frames, p.fft_len // 2 + 1
    feats = tuple(eng.empty_feats(F, H) for _ in range(3))
    strips = eng.empty((max(q.synthesis.strip_floats for q in plans.values()),))
    pcm = eng.empty((p.total_out,))
    return feats, strips, pcm


def ab(args):
    import torch
    import bench
    from magphase_amd import engine as em
    eng = em.get_engine()
    utts = bench.make_batch(0)
    plans = build_plans(em, eng, utts)
    feats, strips, pcm = shared_buffers(eng, plans)
    F = plans["transform"].total_frames
    ref = {}
    for name, p in plans.items():
        for t in feats:
            t.fill_(float("nan"))
        strips.fill_(float("nan"))
        pcm.fill_(float("nan"))
        p.run(feats=feats, strips=strips, out=pcm)
        torch.cuda.synchronize()
        ref[name] = ([t.clone() for t in feats], pcm.clone())
    lines = ["interleaved A/B of LosslessRoundTripPlan.run (launch + fix-up) on the bench batch (%d utterances, %d frames), "
             "stores %s, shared feature / strip / output buffers, %d rounds of %d steps per plan (first %d rounds dropped), HIP events"
             % (len(utts), F, plans["direct"].stores, args.rounds, args.steps, args.drop)]
    same_rows = all(bool(torch.equal(x.view(torch.int32), y.view(torch.int32)))
                    for x, y in zip(ref["transform"][0], ref["direct"][0]))
    yt, yd = ref["transform"][1].double(), ref["direct"][1].double()
    lines.append("direct on NaN-filled buffers: feature rows bit-identical to transform's: %s; max |pcm - pcm_transform| / peak: "
                 "%.3g; NaN left: %d" % (same_rows, float((yd - yt).abs().max() / yt.abs().max()),
                                         int(torch.isnan(ref["direct"][1]).sum())
                                         + sum(int(torch.isnan(t).sum()) for t in ref["direct"][0])))
    del ref
    for _ in range(64):     # out of the post-idle power transient (bench.py)
        plans["transform"].run(feats=feats, strips=strips, out=pcm)
    ms = {k: [] for k in ARMS}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rnd in range(args.rounds):
        for k in range(len(ARMS)):
            name = ARMS[(k + rnd) % len(ARMS)]
            p = plans[name]
            for _ in range(5):
                p.run(feats=feats, strips=strips, out=pcm)
            e0.record()
            for _ in range(args.steps):
                p.run(feats=feats, strips=strips, out=pcm)
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / args.steps)
    kept = {k: v[args.drop:] for k, v in ms.items()}
    spread = {}
    for name in ARMS:
        v = kept[name]
        spread[name] = (max(v) - min(v)) / statistics.median(v)
        lines.append("%-9s median %.4f ms  min %.4f  max %.4f  spread %.2f %%   rounds: %s"
                     % (name, statistics.median(v), min(v), max(v), 100 * spread[name], " ".join("%.4f" % x for x in v)))
    ma, mb = statistics.median(kept["transform"]), statistics.median(kept["direct"])
    diff = (ma - mb) / ma
    every = max(kept["direct"]) < min(kept["transform"])
    bar = 3 * max(spread.values())
    lines.append("direct / transform (medians): %.4f  (%+.2f %% of the step, %+.1f us); every direct round faster than every "
                 "transform round: %s; difference %.2f %% against 3 x the larger spread %.2f %%  ->  %s"
                 % (mb / ma, -100 * diff, 1e3 * (mb - ma), every, 100 * diff, 100 * bar,
                    "a gain" if every and diff > bar else
                    ("slower than transform by more than the spread" if -diff > max(spread.values())
                     else "NOT a gain by the stated criterion")))
    emit(lines, args.out)


def energy(args):
    import torch
    import bench
    import energy_probe
    from magphase_amd import engine as em
    eng = em.get_engine()
    files = power_files(torch)
    utts = bench.make_batch(0)
    plans = build_plans(em, eng, utts)
    feats, strips, pcm = shared_buffers(eng, plans)
    torch.cuda.synchronize()
    time.sleep(1.0)
    idle = [float(open(f).read()) for f in files]
    lines = ["energy per step of LosslessRoundTripPlan.run on the bench batch, %d rounds, each arm looping %.1f s under the "
             "power sampler; idle %.0f W, sclk %.0f MHz" % (args.rounds, args.seconds, idle[0] / 1e6, idle[1] / 1e6),
             "%-9s %5s %9s %8s %9s %9s %9s" % ("inverse", "round", "ms", "W", "sclk MHz", "J/step", "J - idle")]
    for _ in range(64):
        plans["transform"].run(feats=feats, strips=strips, out=pcm)
    res = {k: [] for k in ARMS}
    for rnd in range(args.rounds):
        for k in range(len(ARMS)):
            name = ARMS[(k + rnd) % len(ARMS)]
            p = plans[name]
            ms, (pw, fq) = energy_probe.measure(torch, files, lambda: p.run(feats=feats, strips=strips, out=pcm),
                                                seconds=args.seconds)
            rec = (ms, pw / 1e6, fq / 1e6, pw / 1e6 * ms / 1e3, (pw - idle[0]) / 1e6 * ms / 1e3)
            res[name].append(rec)
            lines.append("%-9s %5d %9.4f %8.0f %9.0f %9.4f %9.4f" % ((name, rnd) + rec))
    for name in ARMS:
        j = [r[4] for r in res[name]]
        lines.append("%-9s J above idle: median %.4f  min %.4f  max %.4f;  ms median %.4f;  W median %.0f"
                     % (name, statistics.median(j), min(j), max(j), statistics.median([r[0] for r in res[name]]),
                        statistics.median([r[1] for r in res[name]])))
    emit(lines, args.out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd")
    p = sub.add_parser("ab")
    p.add_argument("--out")
    p.add_argument("--rounds", type=int, default=17)
    p.add_argument("--drop", type=int, default=2)
    p.add_argument("--steps", type=int, default=40)
    p = sub.add_parser("energy")
    p.add_argument("--out")
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--seconds", type=float, default=2.5)
    args = ap.parse_args()
    if args.cmd is None:
        ap.error("nothing to do")
    {"ab": ab, "energy": energy}[args.cmd](args)


if __name__ == "__main__":
    main()
