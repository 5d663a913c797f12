#!/usr/bin/env python
"""
Type-2 copy synthesis on the MI355X path: analysis_compressed_type2 -> synthesis_from_compressed_type2.

True-envelope magnitudes (60 coefficients), 45 phase coefficients, at the variable (pitch-synchronous) rate and on a
5 ms grid, on the bundled 48 kHz recordings.  The reference gets its epochs from the REAPER binary; here they come from
<stem>.est next to the wav, else from the built-in tracker (--epochs builtin, the default of this demo; not REAPER:
parity unpinned) or from a REAPER binary (--epochs reaper).

    python demos/demo_copy_synthesis_type2.py [--wav FILE ...] [--out-dir DIR] [--epochs builtin|reaper]
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.realpath(__file__))
sys.path.append(os.path.realpath(os.path.join(HERE, "..", "src")))

import libaudio as la  # noqa: E402
import libutils as lu  # noqa: E402
import magphase as mp  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    nat = os.path.join(HERE, "data_48k", "wavs_nat")
    ap.add_argument("--wav", nargs="+", default=[os.path.join(nat, "hvd_593.wav"), os.path.join(nat, "hvd_577.wav")])
    ap.add_argument("--out-dir", default=os.path.join(HERE, "data_48k", "wavs_syn"))
    ap.add_argument("--mag-dim", type=int, default=60)
    ap.add_argument("--phase-dim", type=int, default=45)
    ap.add_argument("--epochs", default="builtin", choices=["builtin", "reaper"],
                    help="epoch source when there is no <stem>.est next to the wav")
    args = ap.parse_args()
    lu.mkdir(args.out_dir)
    if args.epochs == "builtin" and not all(os.path.isfile(os.path.splitext(w)[0] + ".est") for w in args.wav):
        print("epochs: built-in zero-frequency-filtering tracker (not REAPER)")
        mp.use_builtin_epoch_tracker()

    for wav in args.wav:
        for rate in (-1.0, 5.0):
            mag_mel_log, real_mel, imag_mel, lf0, _shift, fs, fft_len, _lgain = mp.analysis_compressed_type2(
                wav, mag_dim=args.mag_dim, phase_dim=args.phase_dim, const_rate_ms=rate)
            v_syn = mp.synthesis_from_compressed_type2(mag_mel_log, real_mel, imag_mel, lf0, fs, fft_len=fft_len,
                                                       const_rate_ms=rate)
            name = "%s_copy_syn_type2_mag_dim_%d_ph_dim_%d_%s.wav" % (
                lu.get_filename(wav), args.mag_dim, args.phase_dim, "var_rate" if rate <= 0 else "const_rate_%gms" % rate)
            la.write_audio_file(os.path.join(args.out_dir, name), v_syn, fs)
            print("wrote", os.path.join(args.out_dir, name))


if __name__ == "__main__":
    main()
