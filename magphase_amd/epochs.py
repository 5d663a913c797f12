"""
Epoch (glottal-closure instant) and voicing front end -- SURVEY.md section 8f rank 1.

The reference shells out to REAPER (libaudio.py:450-455, `reaper -s -x 400 -m 50 -a -u 0.005`), an external binary
that exists neither in the build container nor on the GPU box.  This module is NOT a port of REAPER and makes no parity
claim (**parity unpinned**; quality is checked against synthetic utterances whose epochs are known and on the
reference's bundled natural recordings, tests/test_epochs.py).  It is never substituted silently: magphase.py uses it
only after magphase.use_builtin_epoch_tracker() or with MAGPHASE_EPOCHS=builtin.  It produces what
read_reaper_est_file returns -- epoch times in seconds and a 0/1 voicing flag per epoch, with marks every 5 ms in
unvoiced regions (REAPER's `-u 0.005`) -- in two stages, both batched HIP kernels behind the C ABI
(csrc/magphase_epochs.hip; there is no CPU path -- tests/epochs_model.py is a numpy model of each kernel, for the tests
only):

  1. F0 / voicing track (mpx_epoch_f0_track): normalised cross-correlation on the signal box-decimated to ~4 kHz, 40 ms
     frames every 5 ms, lags for 60-400 Hz (REAPER's -m 50 -x 400 range); the host median-smooths the per-frame
     candidates and takes the voicing decision (a few thousand numbers per utterance).
  2. Epochs by zero-frequency filtering (Murty & Yegnanarayana 2008; mpx_epoch_zff): the differenced signal through two
     zero-frequency resonators (four cumulative sums, float64) with the local mean over ~1.5 average pitch periods
     removed after each resonator (keeps the numbers bounded for any length) and twice more at the end; the zero
     crossings of one direction are the glottal closure instants (which direction = the recording's polarity, decided
     by where the excitation energy sits).  Crossings in frames the first stage calls unvoiced, or with a weak slope,
     are dropped on the host.
"""
import numpy as np


ZFF_ADVANCE_SMPLS = 1.5   # four inclusive cumulative sums (-0.5 sample each) and one first difference (+0.5)


def _median5(v):
    """Median of 5 with replicated ends (per frame track)."""
    vp = np.concatenate((v[:1], v[:1], v, v[-1:], v[-1:]))
    return np.median(np.lib.stride_tricks.sliding_window_view(vp, 5), axis=1)


def _geometry(fs, hop_s=0.005, win_s=0.040, f_lo=60.0, f_hi=400.0):
    dec = max(1, int(round(fs / 4000.0)))
    fs_d = fs / float(dec)
    hop = max(1, int(round(hop_s * fs_d)))
    win = int(round(win_s * fs_d))
    l_min, l_max = max(2, int(fs_d / f_hi)), int(np.ceil(fs_d / f_lo))
    return dec, fs_d, hop, win, l_min, l_max


def _voicing_from_candidates(f0, peak, e_ref, fs, nccf_min=0.5, energy_db=-45.0):
    """Host half of stage 1 for one utterance: the per-frame candidates of mpx_epoch_f0_track (float64 arrays [T]) ->
    (f0 track [T], 0 in unvoiced frames; half_win of the zero-frequency filter's moving mean: ~1.5 median pitch periods,
    1 without a voiced frame)."""
    e_db = 10.0 * np.log10(e_ref / (e_ref.max() + 1e-30) + 1e-30)
    voiced = (peak > nccf_min) & (e_db > energy_db)
    voiced = _median5(voiced.astype(np.float64)) > 0.5           # isolated flips / octave slips
    f0 = np.where(voiced, _median5(f0), 0.0)
    half_win = 1
    if voiced.any():
        t0 = float(np.median(1.0 / f0[voiced]))
        half_win = (int(round(1.5 * t0 * fs)) | 1) // 2
    return f0, half_win


def _epochs_from_crossings(n, fs, f0_h, cnt, idx_h, slope_h, score_h, frac_h, cap, hop_s, win_s, unvoiced_step_s=0.005):
    """Host half of stage 2 for one utterance of n samples: the F0 track of _voicing_from_candidates and the two crossing
    lists of mpx_epoch_zff (cnt [2] as counted on the device, idx_h / slope_h / score_h / frac_h [2, cap], unordered) ->
    (v_pm_sec, v_voi)."""
    dur = n / float(fs)
    voiced_fr = f0_h > 0
    if not voiced_fr.any():
        t = np.arange(unvoiced_step_s, dur - 2.0 / fs, unvoiced_step_s)
        return np.round(t, 6), np.zeros(t.size)
    # polarity: at a closure instant the vocal-tract response is (re-)excited -- the signal energy in the millisecond
    # after it exceeds the energy in the millisecond before; half a period later it is just decaying
    best, cand = -1e30, (np.zeros(0, dtype=np.int64), np.zeros(0), np.zeros(0))
    for p in (0, 1):
        k = min(int(cnt[p]), cap)
        if k == 0:
            continue
        sc = float(score_h[p, :k].mean())
        if sc > best:
            order = np.argsort(idx_h[p, :k], kind="stable")
            best, cand = sc, (idx_h[p, :k][order].astype(np.int64), slope_h[p, :k][order], frac_h[p, :k][order])
    idx, slope, frac = cand
    # Epoch time = the sub-sample zero of the filtered signal, plus the filter chain's own advance: every inclusive
    # cumulative sum 1 / (1 - z^-1) leads the integrator it stands for by half a sample (four of them: two zero-frequency
    # resonators), the first difference lags by half a sample -- 1.5 samples early in all, at any rate; the moving-mean
    # removals are symmetric.  (Round 5: whole-sample crossings and no compensation gave -130 us at 16 kHz against
    # synthetic truth, two samples; the rest of that figure is the test generator's own vocal-tract resonators, whose
    # group delay at zero frequency is -1 sample each plus B / (2 pi f^2) seconds: tools/epoch_natural.py --bias-model.)
    t_ep = (idx - frac + ZFF_ADVANCE_SMPLS) / float(fs)
    # voicing of each crossing: the F0 frame whose centre is nearest
    fr_of = np.clip(np.round((t_ep - 0.5 * win_s) / hop_s).astype(int), 0, f0_h.size - 1)
    keep = voiced_fr[fr_of] if idx.size else np.zeros(0, dtype=bool)
    if keep.any():
        keep &= slope > 0.15 * np.median(slope[keep])
    # the period implied by neighbouring crossings must be plausible for the local F0 (drops spurious crossings)
    t_v = t_ep[keep]
    f_v = f0_h[fr_of[keep]] if idx.size else np.zeros(0)
    if t_v.size > 2:
        # A crossing much closer to its predecessor than the crossings around it are to theirs is spurious.  The
        # yardstick is the filter's OWN rhythm (median of the seven intervals around it), not the F0 track: where the
        # correlation stage locks onto the double period (an octave error: F0 frames of 73 Hz for a 146 Hz voice),
        # "closer than half the F0 period" dropped every second epoch of the stretch -- round 3's 8 % misses sat in the
        # MIDDLE of voiced runs, with the crossing present and kept, not at voicing boundaries.  (Growing the voiced
        # runs outwards by the filter's crossings was tried as well: no more identified cycles, twice the voicing error.)
        dt = np.diff(t_v)
        pad = np.r_[dt[:3][::-1], dt, dt[-3:][::-1]] if dt.size >= 3 else np.r_[dt, dt, dt, dt, dt, dt, dt][:dt.size + 6]
        local = np.median(np.lib.stride_tricks.sliding_window_view(pad, 7), axis=1)
        p_f0 = 1.0 / np.maximum(f_v[1:], 50.0)
        # (never longer than the F0 track's period; never shorter than half of it -- an octave error at worst -- so
        # that the noise crossings the correlation stage's 40 ms frames let through next to a voiced stretch, which
        # have no rhythm of their own, are still thinned out)
        local = np.maximum(np.minimum(local, p_f0), 0.5 * p_f0)
        good = np.ones(t_v.size, dtype=bool)
        good[1:][dt < 0.5 * local] = False
        t_v = t_v[good]
    # unvoiced marks every 5 ms outside voiced runs (REAPER -u 0.005); a voiced run ends when the next epoch is more
    # than 20 ms away (1 / 50 Hz)
    pm, voi = [], []
    t_prev, max_gap = 0.0, 1.0 / 50.0
    for k in range(t_v.size + 1):
        t_next = t_v[k] if k < t_v.size else dur
        if t_next - t_prev > max_gap:
            t = t_prev + unvoiced_step_s
            while t < t_next - 0.5 * unvoiced_step_s:
                pm.append(t)
                voi.append(0.0)
                t += unvoiced_step_s
        if k < t_v.size:
            pm.append(t_next)
            voi.append(1.0)
            t_prev = t_next
    pm, voi = np.asarray(pm), np.asarray(voi)
    ok = (pm > 0) & (pm * fs < n - 2)
    return np.round(pm[ok], 6), voi[ok]


def track_epochs_batch(sigs, fs, engine=None, unvoiced_step_s=0.005, nccf_min=0.5, energy_db=-45.0):
    """
    sigs: list of float arrays in [-1, 1] (or int16 PCM), all at sample rate fs -> list of (v_pm_sec float64 [F],
    v_voi float64 [F] in {0, 1}), the two columns the reference reads from REAPER's .est file.  One set of kernel
    launches for the whole list.
    """
    import torch

    from .engine import get_engine

    e = engine or get_engine()
    U = len(sigs)
    if U == 0:
        return []
    dec, fs_d, hop, win, l_min, l_max = _geometry(fs)
    n_lags = l_max - l_min + 1
    span = win + l_max
    lens = np.asarray([int(np.shape(s)[0]) for s in sigs], dtype=np.int64)
    off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    # the tracker's OWN host buffer: iobatch calls this from its reader thread while the compute thread fills and uploads
    # the engine's shared page-locked staging buffer (Engine.host_staging / upload_staged) -- sharing it corrupted both
    buf = np.empty(int(off[-1]), dtype=np.float32)
    for u, s in enumerate(sigs):
        s = np.asarray(s)
        if s.dtype.kind in "iu":
            np.multiply(s, np.float32(1.0 / 32768.0), out=buf[off[u]:off[u + 1]])
        else:
            buf[off[u]:off[u + 1]] = s
    sig = e.to_device(buf, np.float32)
    nd = np.maximum((lens + 2 * (dec // 2) - 2 * dec) // dec + 1, 0)                 # avg_pool1d(kernel 2 dec, stride dec, pad dec//2)
    T = (np.maximum(nd, span + hop) - span) // hop + 1
    doff = np.concatenate(([0], np.cumsum(nd))).astype(np.int64)
    foff = np.concatenate(([0], np.cumsum(T))).astype(np.int64)
    d = e.to_device_packed([("off", off, np.int64), ("doff", doff, np.int64), ("foff", foff, np.int64)])
    xd = torch.empty(max(int(doff[-1]), 1), dtype=torch.float64, device=e.device)
    means = torch.empty(2 * U, dtype=torch.float64, device=e.device)
    # zeros: the entries launch nothing for a batch without a decimated sample or without any sample, and the host reads these
    f0_d, pk_d, en_d = (torch.zeros(max(int(foff[-1]), 1), dtype=torch.float32, device=e.device) for _ in range(3))
    e.launch("mpx_epoch_f0_track", sig, d["off"], U, dec, d["doff"], int(nd.max()), xd, means, d["foff"], int(T.max()), hop,
             win, l_min, n_lags, float(fs_d), f0_d, pk_d, en_d)
    f0_all, pk_all, en_all = (t.cpu().numpy().astype(np.float64) for t in (f0_d, pk_d, en_d))
    hop_s, win_s = hop / fs_d, win / fs_d

    # ---- host: voicing decision and smoothing per utterance (a thousand frames each)
    f0_tracks, half_win = [], np.ones(U, dtype=np.int32)
    for u in range(U):
        a, b = int(foff[u]), int(foff[u + 1])
        f0, half_win[u] = _voicing_from_candidates(f0_all[a:b], pk_all[a:b], en_all[a:b], fs, nccf_min, energy_db)
        f0_tracks.append(f0)
    # ---- zero-frequency filtering for the utterances that have voiced frames
    n_max = int(lens.max())
    cap = n_max // 16 + 64
    w = max(2, int(round(0.001 * fs)))
    total = max(int(off[-1]), 1)
    bufs = [torch.empty(total, dtype=torch.float64, device=e.device) for _ in range(3)]
    counts = torch.zeros(2 * U, dtype=torch.int32, device=e.device)
    c_idx = torch.zeros(2 * U * cap, dtype=torch.int32, device=e.device)
    c_slope, c_score, c_frac = (torch.zeros(2 * U * cap, dtype=torch.float32, device=e.device) for _ in range(3))
    d_half = e.to_device(half_win, np.int32)
    e.launch("mpx_epoch_zff", sig, d["off"], U, n_max, d_half, w, bufs[0], bufs[1], bufs[2], cap, counts, c_idx, c_slope,
             c_score, c_frac)
    cnt = counts.cpu().numpy()
    idx_h = c_idx.cpu().numpy().reshape(2 * U, cap)
    slope_h = c_slope.cpu().numpy().reshape(2 * U, cap).astype(np.float64)
    score_h = c_score.cpu().numpy().reshape(2 * U, cap).astype(np.float64)
    frac_h = c_frac.cpu().numpy().reshape(2 * U, cap).astype(np.float64)

    out = []
    for u in range(U):
        r = slice(2 * u, 2 * u + 2)
        out.append(_epochs_from_crossings(int(lens[u]), fs, f0_tracks[u], cnt[r], idx_h[r], slope_h[r], score_h[r], frac_h[r],
                                          cap, hop_s, win_s, unvoiced_step_s))
    return out


def track_epochs(v_sig, fs, device=None, unvoiced_step_s=0.005):
    """One utterance: (v_pm_sec, v_voi).  device: a torch device of the engine to use (default: the current one)."""
    from .engine import get_engine

    return track_epochs_batch([v_sig], fs, engine=get_engine(device), unvoiced_step_s=unvoiced_step_s)[0]


def accuracy_against_truth(pm_true, voi_true, pm_est, voi_est, max_period_s=0.02):
    """
    The usual glottal-closure-instant scores (Naylor et al. 2007) of an estimated (v_pm_sec, v_voi) track against a
    known one, plus pitch and voicing errors -- what tests/test_epochs.py prints and bounds and tools/epoch_accuracy.py
    records (the front end is quality-judged, there is no REAPER here to be bit-judged against).

    A larynx cycle is the span around a true voiced epoch t_k bounded by the midpoints to its voiced neighbours (cycles
    next to a voicing boundary, where a neighbour is further than max_period_s away, are bounded by half that period).
      identification_rate   cycles with exactly ONE estimated voiced epoch
      miss_rate / false_alarm_rate   cycles with none / with more than one
      jitter_us, bias_us    standard deviation / median of (estimate - truth) over the identified cycles, microseconds
      gross_f0_error_rate   identified consecutive cycle pairs whose estimated period differs from the true one by > 20 %
      voicing_error_rate    disagreement of the voiced / unvoiced decision on a 5 ms grid
    """
    pm_true, voi_true = np.asarray(pm_true, dtype=np.float64), np.asarray(voi_true) > 0
    pm_est, voi_est = np.asarray(pm_est, dtype=np.float64), np.asarray(voi_est) > 0
    tv, ev = pm_true[voi_true], np.sort(pm_est[voi_est])
    out = {"true_voiced_epochs": int(tv.size), "estimated_voiced_epochs": int(ev.size)}
    if tv.size < 3:
        return out
    half = np.minimum(np.diff(tv), max_period_s) / 2.0
    lo = tv - np.r_[half[0], half]
    hi = tv + np.r_[half, half[-1]]
    n_in = np.searchsorted(ev, hi, side="left") - np.searchsorted(ev, lo, side="left")
    ident = n_in == 1
    first = np.searchsorted(ev, lo, side="left")
    err = ev[np.minimum(first[ident], max(ev.size - 1, 0))] - tv[ident] if ev.size else np.zeros(0)
    out.update(identification_rate=float(ident.mean()), miss_rate=float((n_in == 0).mean()),
               false_alarm_rate=float((n_in > 1).mean()),
               jitter_us=float(np.std(err) * 1e6) if err.size else float("nan"),
               bias_us=float(np.median(err) * 1e6) if err.size else float("nan"))
    both = ident[1:] & ident[:-1] & (np.diff(tv) < max_period_s)
    if both.any():
        e_of = np.full(tv.size, np.nan)
        e_of[ident] = tv[ident] + err
        p_true, p_est = np.diff(tv)[both], np.diff(e_of)[both]
        out["gross_f0_error_rate"] = float((np.abs(p_est / p_true - 1.0) > 0.2).mean())
        out["f0_fine_error_percent"] = float(np.mean(np.abs(p_est / p_true - 1.0)[np.abs(p_est / p_true - 1.0) <= 0.2]) * 100)
    dur = max(pm_true[-1], pm_est[-1] if pm_est.size else 0.0)
    grid = np.arange(0.0025, dur, 0.005)

    def voiced_on(pm, voi):
        k = np.clip(np.searchsorted(pm, grid), 0, pm.size - 1)
        return voi[k]

    if pm_est.size:
        out["voicing_error_rate"] = float((voiced_on(pm_true, voi_true) != voiced_on(pm_est, voi_est)).mean())
    return out


# ----------------------------------------------------------------------------------------------------------------------
# Natural speech: voicing truth from phone labels.  The reference bundles ten recordings WITH their HTS state-aligned labels
# (demos/data_48k/labs/*.lab, the input of its label re-timing script); the identity of a phone says whether it is voiced,
# independently of any epoch tracker -- the one natural-speech truth there is offline (no REAPER output exists here).
# ----------------------------------------------------------------------------------------------------------------------
# Unilex phone names of the bundled labels.  Sonorants are voiced throughout; voiceless obstruents and silence are not;
# voiced obstruents (b d g v D z dZ) and /h/ devoice or voice with their context and are not scored.
PHONES_VOICED = frozenset("@ @@ a A aI aU E eI i I I@ O OI Q u U @U V n m N r l lw l! w j".split())
PHONES_UNVOICED = frozenset("# pau sil s t k p f T tS S".split())


def label_voicing_spans(lab_file, margin_s=0.015, min_len_s=0.03):
    """HTS state-aligned label file -> (voiced spans, unvoiced spans), lists of (t0, t1) in seconds: consecutive states of one
    phone and consecutive phones of one class merged, `margin_s` cut off both ends (forced-alignment boundaries are good to ~10-20 ms, and voicing sets in /
    dies out inside the neighbouring phones), spans shorter than min_len_s after trimming dropped."""
    import re

    phones = []
    with open(lab_file) as fh:
        for line in fh:
            p = line.split()
            if len(p) < 3:
                continue
            m = re.match(r"[^-]*-([^+]+)\+", p[2])
            if not m:
                continue
            t0, t1, ph = int(p[0]) * 1e-7, int(p[1]) * 1e-7, m.group(1)
            if phones and phones[-1][2] == ph and abs(phones[-1][1] - t0) < 1e-9 and "[2]" not in p[2]:
                phones[-1][1] = t1          # the next state of the same phone
            else:
                phones.append([t0, t1, ph])
    # consecutive phones of one class form a run (a vowel between a nasal and a liquid is voiced throughout): the margins
    # are cut at the ends of runs, where the class changes
    runs = []
    for t0, t1, ph in phones:
        c = "v" if ph in PHONES_VOICED else ("u" if ph in PHONES_UNVOICED else "x")
        if runs and runs[-1][2] == c and abs(runs[-1][1] - t0) < 1e-9:
            runs[-1][1] = t1
        else:
            runs.append([t0, t1, c])
    voiced, unvoiced = [], []
    for t0, t1, c in runs:
        a, b = t0 + margin_s, t1 - margin_s
        if b - a < min_len_s or c == "x":
            continue
        (voiced if c == "v" else unvoiced).append((a, b))
    return voiced, unvoiced


def score_against_labels(pm_sec, voi, lab_file, step_s=0.005):
    """Agreement of a (v_pm_sec, v_voi) track with the voicing the phone labels imply, on a 5 ms grid inside the labelled
    spans (label_voicing_spans), plus the continuity of F0 inside the voiced spans:
      voiced_recall      grid points of voiced phones the track calls voiced
      unvoiced_recall    grid points of voiceless phones / silence the track calls unvoiced
      agreement          both classes pooled
      f0_median_hz, f0_jump_rate   consecutive voiced periods inside voiced spans: median 1 / period; share of neighbouring
                                   periods that differ by more than 20 % (octave slips, dropped or doubled epochs)"""
    pm_sec, voi = np.asarray(pm_sec, dtype=np.float64), np.asarray(voi) > 0
    v_spans, u_spans = label_voicing_spans(lab_file)

    def track_voiced(t):
        k = np.clip(np.searchsorted(pm_sec, t), 0, pm_sec.size - 1)
        return voi[k]

    def grid(spans):
        return np.concatenate([np.arange(a, b, step_s) for a, b in spans]) if spans else np.zeros(0)

    gv, gu = grid(v_spans), grid(u_spans)
    hit_v, hit_u = track_voiced(gv), ~track_voiced(gu)
    per, jumps = [], []
    for a, b in v_spans:
        sel = (pm_sec >= a) & (pm_sec <= b) & voi
        t = pm_sec[sel]
        if t.size >= 3:
            d = np.diff(t)
            per.append(d)
            jumps.append(np.abs(d[1:] / d[:-1] - 1.0) > 0.2)
    per = np.concatenate(per) if per else np.zeros(0)
    jumps = np.concatenate(jumps) if jumps else np.zeros(0, dtype=bool)
    return {"voiced_points": int(gv.size), "unvoiced_points": int(gu.size),
            "voiced_recall": float(hit_v.mean()) if gv.size else float("nan"),
            "unvoiced_recall": float(hit_u.mean()) if gu.size else float("nan"),
            "agreement": float((hit_v.sum() + hit_u.sum()) / max(1, gv.size + gu.size)),
            "f0_median_hz": float(1.0 / np.median(per)) if per.size else float("nan"),
            "f0_jump_rate": float(jumps.mean()) if jumps.size else float("nan")}
