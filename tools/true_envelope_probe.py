"""
True envelope on the headline batch (64 synthetic 5 s utterances at 48 kHz: magphase_amd.synthetic ->
analysis_lossless_batch, ~57 k frames, fft_len 4096).  Prints one JSON line:
  te_<nc>_ms / te_<nc>_ticket_ms   median launch time (HIP events, warmed up, alternated in this process) of
                                   mpx_true_envelope ('abs', thres_db 0.1) with frames by grid stride / by ticket counter
  passes_<nc>_mean / _max          passes per frame (rows with a zero magnitude, nan_rows_<nc>, run none: left out)
  te_<nc>_us_per_frame_pass        launch time / (frames x mean passes) -- beside min_phase_us_per_frame, the time per
                                   frame of k_min_phase (the same two transforms, once) on the same frames
  speedup_<nc>                     the reference's CPU time per frame (tests/golden/g15_true_envelope.npz, one core) /
                                   the device's
    python tools/true_envelope_probe.py [--reps 10] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--utts", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from magphase_amd import magphase as mp
    from magphase_amd import synthetic as syn
    from magphase_amd.engine import get_engine

    fs, dur, N = 48000, 5.0, 4096
    H = N // 2 + 1
    utts = []
    for i in range(args.utts):
        pcm, pm, voi = syn.make_utterance(i, dur_s=dur, fs=fs)
        utts.append((pcm, fs, pm, voi))
    mags = [f[0] for f in mp.analysis_lossless_batch(utts)]
    e = get_engine()
    dev = [torch.from_numpy(m.astype(np.float32)).to(e.device) for m in mags]
    F = sum(m.shape[0] for m in mags)
    gold = np.load(os.path.join(ROOT, "tests", "golden", "g15_true_envelope.npz"))

    # k_min_phase on the same frames (rows at mpx_spec_ld)
    ld = int(e.lib.mpx_spec_ld(H))
    x = e.empty((F, ld))
    x[:, :H].copy_(torch.cat(dev))
    ident = torch.arange(F, dtype=torch.int32, device=e.device)
    zeros_t = torch.zeros(F, dtype=torch.float32, device=e.device)
    o = [e.empty((F, ld)) for _ in range(3)]
    tab = e.tables(N)

    def min_phase():
        e.lib.mpx_min_phase(e.stream_ptr(), N, tab.data_ptr(), x.data_ptr(), ident.data_ptr(), ident.data_ptr(),
                            zeros_t.data_ptr(), F, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), ld)

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn):
        ev[0].record()
        fn()
        ev[1].record()
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1])

    res = {"frames": F, "utts": len(mags), "fft_len": N}
    fns = {"min_phase": min_phase}
    for nc in (60, 600):
        for tk in (False, True):   # grid stride / ticket counter
            fns["te_%d%s" % (nc, "_ticket" if tk else "")] = (
                lambda nc=nc, tk=tk: e.true_envelope(dev, "abs", nc, 0.1, want_iters=True, ticket=tk))
    for fn in fns.values():
        for _ in range(2):
            timed(fn)
    t = {k: [] for k in fns}
    for _ in range(args.reps):
        for k, fn in fns.items():
            t[k].append(timed(fn))
    for k in fns:
        res[k + "_ms"] = float(np.median(t[k]))
        res[k + "_ms_min"] = float(np.min(t[k]))
    res["min_phase_us_per_frame"] = 1e3 * res["min_phase_ms"] / F
    for nc in (60, 600):
        out, _, it = e.true_envelope(dev, "abs", nc, 0.1, want_iters=True, ticket=False)
        out_t, _, it_t = e.true_envelope(dev, "abs", nc, 0.1, want_iters=True, ticket=True)
        res["ticket_bit_identical_%d" % nc] = bool(torch.equal(torch.nan_to_num(out[:, :H], nan=-7.0),
                                                              torch.nan_to_num(out_t[:, :H], nan=-7.0))
                                                   and torch.equal(it, it_t))
        nan_rows = torch.isnan(out[:, :H]).all(dim=1).cpu().numpy()   # a zero magnitude: no passes run
        res["nan_rows_%d" % nc] = int(nan_rows.sum())
        it = it.cpu().numpy()[~nan_rows]
        best = min(res["te_%d_ms" % nc], res["te_%d_ticket_ms" % nc])
        res["passes_%d_mean" % nc] = float(it.mean())
        res["passes_%d_max" % nc] = int(it.max())
        res["te_%d_us_per_frame_pass" % nc] = 1e3 * best / it.sum()
        res["te_%d_frame_pass_over_min_phase_frame" % nc] = res["te_%d_us_per_frame_pass" % nc] / res["min_phase_us_per_frame"]
        ref_ms = float(gold["ref_ms_per_frame_48k_%d" % nc])
        res["ref_cpu_ms_per_frame_%d" % nc] = ref_ms
        res["speedup_%d" % nc] = ref_ms * F / best
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
