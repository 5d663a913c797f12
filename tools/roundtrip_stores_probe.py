#!/usr/bin/env python
"""
Whether storing the round-trip kernel's feature rows by line pays (MAGPHASE_RT_STORES=rows | lines | lines_nt; csrc/
mpx_common.hpp, "Row stores by line"), on the bench batch, and what a written byte costs with and without the non-temporal
bit.  On the GPU box:

    python tools/roundtrip_stores_probe.py fill   --out FILL.txt    # 1 GiB fills, plain against non-temporal: GB/s, pJ/B
    python tools/roundtrip_stores_probe.py ab     --out AB.txt      # interleaved timing of the three forms
    python tools/roundtrip_stores_probe.py energy --out ENERGY.txt  # joules per step above idle of the three forms

fill    mpx_bw_probe's fill kernel (whole aligned 16-byte stores per lane, 8192 x 512 threads, 4 stores in flight) in its
        plain and its non-temporal shape, alternating, each looping for ~2 s while a thread samples this device's board power
        (tools/energy_probe.py); energy above the idle reading taken first.  The spread of a column over the rounds is the
        table's own run-to-run spread.  (mpx_bw_probe has no 4-byte-per-lane shape.)
ab      the three plans are built in one process and run in turn on shared feature / strip / output buffers (the scheme of
        tools/roundtrip_seams_probe.py): 17 rounds (the first 2 dropped) of 40 steps per plan, HIP events around rt.run
        (launch + fix-up), the order rotating from round to round.  A form is a gain only if every one of its rounds beats
        every round of rows and the medians differ by more than three times the larger spread (max - min over the median).
energy  each plan loops for ~2.5 s under the power sampler: ms, W, J per step, J above idle.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

FORMS = ("rows", "lines", "lines_nt")


def emit(lines, out):
    print("\n".join(lines), flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


def power_files(torch):
    import energy_probe
    d = energy_probe.my_hwmon(torch)
    if d is None:
        sys.exit("roundtrip_stores_probe: no hwmon directory for this device")
    return [os.path.join(d, "power1_input"), os.path.join(d, "freq1_input")]


def build_plans(em, eng, utts):
    plans = {}
    for name in FORMS:
        os.environ["MAGPHASE_RT_STORES"] = name
        plans[name] = em.LosslessRoundTripPlan(eng, utts)
        assert plans[name].stores == name
    os.environ.pop("MAGPHASE_RT_STORES", None)
    return plans


def shared_buffers(eng, plans):
    p = plans["rows"]
    F, H = p.total_frames, p.fft_len // 2 + 1
    feats = tuple(eng.empty_feats(F, H) for _ in range(3))   # shared by the plans: same addresses, same channels
    strips = eng.empty((max(q.synthesis.strip_floats for q in plans.values()),))
    pcm = eng.empty((p.total_out,))
    return feats, strips, pcm


def fill(args):
    import torch
    import energy_probe
    from magphase_amd import _lib, engine as em
    eng = em.get_engine()
    files = power_files(torch)
    n = 1 << 28
    a, one = eng.empty((n,)), eng.empty((4,))
    a.zero_()
    torch.cuda.synchronize()
    time.sleep(1.0)
    idle = [float(open(f).read()) for f in files]
    shapes = {"plain": 4, "non-temporal": 5}   # kShapes of csrc/magphase_probe.hip: {8192, 512, 4, 0} and {8192, 512, 4, 1}

    def launch(shape):
        return lambda: _lib.check(eng.lib.mpx_bw_probe(eng.stream_ptr(), 1 + 16 * shape, a.data_ptr(), one.data_ptr(), n),
                                  "mpx_bw_probe")

    for s in shapes.values():     # out of the post-idle power transient
        for _ in range(200):
            launch(s)()
    torch.cuda.synchronize()
    rows = {k: [] for k in shapes}
    lines = ["1 GiB fill, whole aligned 16-byte stores per lane (mpx_bw_probe fill, 8192 x 512 threads, 4 stores in flight), "
             "plain against non-temporal, alternating, %d rounds of %.1f s each; board power of this device sampled every 4 ms"
             % (args.rounds, args.seconds),
             "idle before the first round: %.0f W, sclk %.0f MHz" % (idle[0] / 1e6, idle[1] / 1e6),
             "%-13s %5s %9s %9s %8s %9s %12s %14s" % ("stores", "round", "ms", "GB/s", "W", "sclk MHz", "pJ/B (board)", "pJ/B above idle")]
    for rnd in range(args.rounds):
        for name in (tuple(shapes) if rnd % 2 == 0 else tuple(shapes)[::-1]):
            ms, (pw, fq) = energy_probe.measure(torch, files, launch(shapes[name]), seconds=args.seconds, batch=20)
            nbytes = 4.0 * n
            rec = (ms, nbytes / (ms * 1e-3) / 1e9, pw / 1e6, fq / 1e6, pw / 1e6 * ms * 1e-3 / nbytes * 1e12,
                   (pw - idle[0]) / 1e6 * ms * 1e-3 / nbytes * 1e12)
            rows[name].append(rec)
            lines.append("%-13s %5d %9.4f %9.1f %8.0f %9.0f %12.2f %14.2f" % ((name, rnd) + rec))
    med = {}
    for name, v in rows.items():
        col = [r[5] for r in v]
        bw = [r[1] for r in v]
        med[name] = statistics.median(col)
        lines.append("%-13s pJ/B above idle: median %.2f  min %.2f  max %.2f  spread %.2f %%;  GB/s: median %.1f  min %.1f  max %.1f"
                     % (name, med[name], min(col), max(col), 100 * (max(col) - min(col)) / med[name], statistics.median(bw),
                        min(bw), max(bw)))
    spread = max((max(r[5] for r in v) - min(r[5] for r in v)) / med[k] for k, v in rows.items())
    diff = (med["plain"] - med["non-temporal"]) / med["plain"]
    lines.append("non-temporal against plain, pJ/B above idle (medians): %+.2f %%; the table's larger spread: %.2f %%  ->  "
                 "the non-temporal fill is %s" % (-100 * diff, 100 * spread,
                                                  "cheaper per byte by more than the spread" if diff > spread
                                                  else "NOT cheaper per byte by more than the spread"))
    emit(lines, args.out)


def ab(args):
    import torch
    import bench
    from magphase_amd import engine as em
    eng = em.get_engine()
    utts = bench.make_batch(0)
    plans = build_plans(em, eng, utts)
    feats, strips, pcm = shared_buffers(eng, plans)
    F = plans["rows"].total_frames
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
             "shared feature / strip / output buffers, %d rounds of %d steps per plan (first %d rounds dropped), HIP events"
             % (len(utts), F, args.rounds, args.steps, args.drop),
             "phases of the three planes' first rows: %s" % " ".join(str((t.data_ptr() // 4) % 32) for t in feats)]
    for name in FORMS[1:]:
        same_rows = all(bool(torch.equal(x.view(torch.int32), y.view(torch.int32))) for x, y in zip(ref["rows"][0], ref[name][0]))
        same_pcm = bool(torch.equal(ref["rows"][1].view(torch.int32), ref[name][1].view(torch.int32)))
        lines.append("%-8s on NaN-filled buffers: feature rows bit-identical to rows': %s; pcm_out bit-identical: %s; NaN left: %d"
                     % (name, same_rows, same_pcm, int(torch.isnan(ref[name][1]).sum()) + sum(int(torch.isnan(t).sum()) for t in ref[name][0])))
    del ref
    for _ in range(64):     # out of the post-idle power transient (bench.py)
        plans["rows"].run(feats=feats, strips=strips, out=pcm)
    ms = {k: [] for k in FORMS}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rnd in range(args.rounds):
        for k in range(len(FORMS)):
            name = FORMS[(k + rnd) % len(FORMS)]
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
    for name in FORMS:
        v = kept[name]
        spread[name] = (max(v) - min(v)) / statistics.median(v)
        lines.append("%-8s median %.4f ms  min %.4f  max %.4f  spread %.2f %%   rounds: %s"
                     % (name, statistics.median(v), min(v), max(v), 100 * spread[name], " ".join("%.4f" % x for x in v)))
    ma = statistics.median(kept["rows"])
    for name in FORMS[1:]:
        mb = statistics.median(kept[name])
        diff = (ma - mb) / ma
        every = max(kept[name]) < min(kept["rows"])
        bar = 3 * max(spread["rows"], spread[name])
        lines.append("%s / rows (medians): %.4f  (%+.2f %% of the step, %+.1f us); every %s round faster than every rows round: "
                     "%s; difference %.2f %% against 3 x the larger spread %.2f %%  ->  %s"
                     % (name, mb / ma, -100 * diff, 1e3 * (mb - ma), name, every, 100 * diff, 100 * bar,
                        "a gain" if every and diff > bar else
                        ("slower than rows by more than the spread" if -diff > max(spread["rows"], spread[name])
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
    lines = ["energy per step of LosslessRoundTripPlan.run on the bench batch, %d rounds, each form looping %.1f s under the "
             "power sampler; idle %.0f W, sclk %.0f MHz" % (args.rounds, args.seconds, idle[0] / 1e6, idle[1] / 1e6),
             "%-8s %5s %9s %8s %9s %9s %9s" % ("stores", "round", "ms", "W", "sclk MHz", "J/step", "J - idle")]
    for _ in range(64):
        plans["rows"].run(feats=feats, strips=strips, out=pcm)
    res = {k: [] for k in FORMS}
    for rnd in range(args.rounds):
        for k in range(len(FORMS)):
            name = FORMS[(k + rnd) % len(FORMS)]
            p = plans[name]
            ms, (pw, fq) = energy_probe.measure(torch, files, lambda: p.run(feats=feats, strips=strips, out=pcm),
                                                seconds=args.seconds)
            rec = (ms, pw / 1e6, fq / 1e6, pw / 1e6 * ms / 1e3, (pw - idle[0]) / 1e6 * ms / 1e3)
            res[name].append(rec)
            lines.append("%-8s %5d %9.4f %8.0f %9.0f %9.4f %9.4f" % ((name, rnd) + rec))
    for name in FORMS:
        j = [r[4] for r in res[name]]
        lines.append("%-8s J above idle: median %.4f  min %.4f  max %.4f;  ms median %.4f"
                     % (name, statistics.median(j), min(j), max(j), statistics.median([r[0] for r in res[name]])))
    emit(lines, args.out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd")
    p = sub.add_parser("fill")
    p.add_argument("--out")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--seconds", type=float, default=2.0)
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
    {"fill": fill, "ab": ab, "energy": energy}[args.cmd](args)


if __name__ == "__main__":
    main()
