"""GPU: k_griffin_lim_pair<P> (mpx_griffin_lim_ola, csrc/magphase_comp.hip) launched by itself -- one iteration, no
first synthesis by another kernel -- against the fp64 model of one iteration (tests/griffin_lim_iter_model.py, held to the
reference's model and golden by tests/test_griffin_lim_iter_host.py).

How the kernel is driven: GriffinLimPlan builds the frame, run and slot tables only; Engine.griffin_lim_ola and
Engine.ola_fixup(plan.iter) are called with this file's own buffers:

  sig_in      float32 white noise the test makes (the model gets exactly these values), between runs of NaN
  target      rows of pitch mpx_spec_ld(H), the pad columns NaN, rows of NaN before and after
  sig_out     inside a sentinel-filled buffer with guards: every sample of [0, total_out) must lose the sentinel, nothing else
  phase rows  the same, pitched: columns [H, ld) and the rows around keep the sentinel
  strips      NaN before the launch (an element read before it is written reaches the output), sentinel guards around

The batch of each fft_len (griffin_lim_iter_model.shifts: 6 utterances, ~80 frames) holds a first shift of N/2, right
lengths of N/2 - 1, shifts of 0 (the smallest accepted), 1, 2, 63, 64, 65, around 155 and 240, 512 and 513 where N allows,
a lone frame, a two-frame utterance and an utterance of digital silence between two loud ones; frames_per_run 1 (every
frame a run: a seam and a head strip per frame), 3 and the planner's default.  Targets are random in [0.5, 1.5] with exact
zeros (DC, Nyquist and the handover bin M/2 among them) and one-hot rows at bins 0, 1, N/4, N/2 - 1 and N/2.

What is held to what (no bin, frame or sample is left out of any comparison):

  GLK_ITER_BOUND        max |out - model| / bound <= 1: the derived per-sample bound of griffin_lim_iter_model.bound
  GLK_PHASE_BOUND       max circular |phi - model| / (e_k + 4 u pi) <= 1 per bin; |phi| <= float32(pi); DC and Nyquist exactly
                        0 or float32(pi); with phase_out = None the signal is bit-identical
  GLK_ZERO_BOUND        the silent utterance (T != 0): phase rows exactly 0, output within the bound of ola(ifft(T)) -- one
                        sample read from a neighbour, or the phasor (-1)^k dropped, breaks it; all-zero frames of the loud
                        utterances (the noise is sparse) likewise give phase 0
  GLK_SCALE_BOUND,      sig_in scaled by 2^-40, 2^-62, 2^-90: the model is scale-invariant, the same bounds hold; at 2^-62
  GLK_SCALE_PHASE_BOUND the spectrum's components lie on both sides of the kernel's 2^-60 threshold, at 2^-90 all below it
  discipline            no NaN in any output, the guards, sig_in and the target bitwise unchanged, a second launch into
                        fresh buffers bit-identical

Measured against the fp64 model on the MI355X (never against another device path); the two tolerances are stated at
<= 3 x the worst value (tests/_tol.py; profiles/r29_griffin_lim_kernel_tolerance_report.json):

  label                            1024        2048        4096
  GLK_ITER_BOUND         (frac)    0.0104      0.0019      0.0038      loud utterances, both launches (with / without rows)
  GLK_ZERO_BOUND         (frac)    0.0193      0.0076      0.0064      the silent utterance: e_k = 0, the bound is (L + 4) u
  GLK_PHASE_BOUND        (frac)    0.147       0.099       0.149
  GLK_SCALE_BOUND        (frac)    0.0096      0.0019      0.0038      the figures of the unscaled launch: the arithmetic
  GLK_SCALE_PHASE_BOUND  (frac)    0.147       0.099       0.149       is scale-invariant up to the kernel's branch
  GLK_ITER_TOL           (/peak)   2.13e-7     4.03e-7     3.84e-7     max |err| / the utterance's peak
  GLK_PHASE_TOL          (rad)     9.70e-8     9.52e-8     9.91e-8     |X|-weighted mean circular error of an utterance

What these tests found: as two template instances (with / without phase rows) the kernel's signal differed between the two
launches at fft_len 4096 in the last bit of 3 samples in 4 (worst 1.2e-7 absolute; both within 0.7 % of the bound): the
compiler contracted the same source differently in the two.  The phase rows are a run-time branch of one instance now
(csrc/magphase_comp.hip), and test_phase_rows asks for the equality bit for bit.
"""
import functools

import numpy as np
import pytest
import torch

import griffin_lim_iter_model as gi
from _tol import within
from magphase_amd.plans import GriffinLimPlan

pytestmark = pytest.mark.gpu

SENT = -77.25
GUARD = 64            # sentinel floats before and after sig_out and the strips
ROW_GUARD = 2         # rows before and after the target (NaN) and the phase rows (sentinel)
NAN_GUARD = 2112      # NaNs before and after sig_in
PI32 = np.float32(np.pi)

GLK_ITER_TOL = {1024: 6e-7, 2048: 1.2e-6, 4096: 1.1e-6}    # <= 3 x measured: see the table above
GLK_PHASE_TOL = {1024: 2.8e-7, 2048: 2.8e-7, 4096: 2.8e-7}

CASES = [(N, fpr) for N in gi.FFT_LENS for fpr in gi.FRAMES_PER_RUN]
CASE_IDS = ["%d-%s" % (N, fpr or "default") for N, fpr in CASES]


def _engine():
    from magphase_amd.engine import get_engine
    return get_engine()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _plan(N, fpr):
    return GriffinLimPlan(_engine(), gi.shifts(N), N, frames_per_run=fpr)


@functools.lru_cache(maxsize=None)
def _inputs(N, exp):
    """The batch's inputs on the device, fenced: -> (sig_in view, its whole host image, target view [F x H] of pitch ld,
    its whole host image, ld)."""
    e, b = _engine(), gi.batch(N)
    H = N // 2 + 1
    ld = int(e.lib.mpx_spec_ld(H))
    assert ld > H
    sig = np.concatenate(b["sig"]) * np.float32(2.0 ** exp)
    assert sig.dtype == np.float32 and np.array_equal(np.float64(sig), np.float64(np.concatenate(b["sig"])) * 2.0 ** exp)
    assert np.all((sig == 0) | (np.abs(sig) >= 2.0 ** -125))          # no denormal
    h_sig = np.full(sig.size + 2 * NAN_GUARD, np.nan, dtype=np.float32)
    h_sig[NAN_GUARD:NAN_GUARD + sig.size] = sig
    t = np.concatenate(b["target"])
    F = t.shape[0]
    h_t = np.full((F + 2 * ROW_GUARD, ld), np.nan, dtype=np.float32)
    h_t[ROW_GUARD:ROW_GUARD + F, :H] = t
    d_sig = torch.from_numpy(h_sig).to(e.device)
    d_t = torch.from_numpy(h_t).to(e.device)
    return d_sig, h_sig, d_t, h_t, ld


def _launch(N, fpr, exp, phase=True):
    """One launch of the iteration and its fix-up into fresh buffers -> dict of host copies (after a synchronise)."""
    e, plan = _engine(), _plan(N, fpr)
    H = N // 2 + 1
    d_sig, h_sig, d_t, h_t, ld = _inputs(N, exp)
    F, total = plan.total_frames, plan.total_out
    assert F == h_t.shape[0] - 2 * ROW_GUARD and total == h_sig.size - 2 * NAN_GUARD
    assert plan.out_len == [x.size for x in gi.batch(N)["sig"]]
    out = torch.full((total + 2 * GUARD,), SENT, dtype=torch.float32, device=e.device)
    n_strip = max(int(plan.iter.strip_floats), 1)
    strips = torch.full((n_strip + 2 * GUARD,), SENT, dtype=torch.float32, device=e.device)
    strips[GUARD:GUARD + n_strip] = float("nan")
    ph = torch.full((F + 2 * ROW_GUARD, ld), SENT, dtype=torch.float32, device=e.device) if phase else None
    sig_in = d_sig[NAN_GUARD:NAN_GUARD + total]
    target = d_t[ROW_GUARD:ROW_GUARD + F, :H]
    assert int(target.stride(0)) == ld
    s_out, s_strips = out[GUARD:GUARD + total], strips[GUARD:GUARD + n_strip]
    e.griffin_lim_ola(N, plan, target, sig_in, s_out, s_strips,
                      phase_out=ph[ROW_GUARD:ROW_GUARD + F, :H] if phase else None)
    e.ola_fixup(N, plan.iter, s_strips, s_out)
    torch.cuda.synchronize()
    return dict(out=out.cpu().numpy(), strips=strips.cpu().numpy(), phase=ph.cpu().numpy() if phase else None,
                sig_after=d_sig.cpu().numpy(), target_after=d_t.cpu().numpy(), total=total, F=F, ld=ld, n_strip=n_strip)


@functools.lru_cache(maxsize=None)
def _case(N, fpr, exp=0):
    return _launch(N, fpr, exp)


@functools.lru_cache(maxsize=None)
def _case_plain(N, fpr, exp=0):
    return _launch(N, fpr, exp, phase=False)


def _per_utt(N, r):
    """-> [(u, device signal float64, device phase rows [F_u x H] float32 or None)] of a launch's host copies."""
    b = gi.batch(N)
    H = N // 2 + 1
    sig = r["out"][GUARD:GUARD + r["total"]]
    rows = r["phase"][ROW_GUARD:ROW_GUARD + r["F"], :H] if r["phase"] is not None else None
    o_off = np.concatenate(([0], np.cumsum([x.size for x in b["sig"]])))
    f_off = np.concatenate(([0], np.cumsum([v.size for v in b["shifts"]])))
    return [(u, np.float64(sig[o_off[u]:o_off[u + 1]]), None if rows is None else rows[f_off[u]:f_off[u + 1]])
            for u in range(len(b["sig"]))]


def _figures(N, r, what, silent=False):
    """Every sample and every bin of a launch's loud utterances (silent: of the silent one) against the model -> (worst
    |err| / bound, worst |err| / peak, worst phase error / bound, worst |X|-weighted mean phase error); each printed."""
    b = gi.batch(N)
    f_sig = f_peak = f_ph = f_wph = 0.0
    for u, sig, rows in _per_utt(N, r):
        if (u == gi.SILENT) != silent:
            continue
        ref, ref_ph, X, S = b["model"][u]
        sig_bound, ph_bound = b["bound"][u]
        assert not np.isnan(sig).any(), "%s: NaN in utterance %d" % (what, u)
        err = np.abs(sig - ref)
        f_sig = max(f_sig, float(np.max(err / sig_bound)))
        f_peak = max(f_peak, float(np.max(err) / np.max(np.abs(ref))))
        if rows is None:
            continue
        assert not np.isnan(rows).any(), "%s: NaN in the phase rows of utterance %d" % (what, u)
        d = gi.circular(rows, ref_ph)
        f_ph = max(f_ph, float(np.max(d / ph_bound)))
        wgt = np.abs(X)
        if np.any(wgt):
            f_wph = max(f_wph, float(np.sum(wgt * d) / np.sum(wgt)))
    print("%s: |err|/bound %.4g  |err|/peak %.4g  phase/bound %.4g  weighted phase %.4g" % (what, f_sig, f_peak, f_ph, f_wph))
    return f_sig, f_peak, f_ph, f_wph


@pytest.mark.parametrize("N,fpr", CASES, ids=CASE_IDS)
def test_signal_against_model(N, fpr):
    """Both launches: with phase rows (the last iteration of a call) and without (every other one)."""
    for r, name in ((_case(N, fpr), "phase"), (_case_plain(N, fpr), "plain")):
        f_sig, f_peak, _, _ = _figures(N, r, "iter %d/%s %s" % (N, fpr, name))
        within(f_sig, 1.0, "GLK_ITER_BOUND:%d" % N)
        within(f_peak, GLK_ITER_TOL[N], "GLK_ITER_TOL:%d" % N)


@pytest.mark.parametrize("N,fpr", CASES, ids=CASE_IDS)
def test_phase_rows(N, fpr):
    r = _case(N, fpr)
    H = N // 2 + 1
    _, _, f_ph, f_wph = _figures(N, r, "phase %d/%s" % (N, fpr))
    within(f_ph, 1.0, "GLK_PHASE_BOUND:%d" % N)
    within(f_wph, GLK_PHASE_TOL[N], "GLK_PHASE_TOL:%d" % N)
    rows = r["phase"][ROW_GUARD:ROW_GUARD + r["F"], :H]
    assert np.all(np.abs(rows) <= PI32)
    for k in (0, H - 1):                                    # a real bin: 0 or pi, nothing in between
        a = np.abs(rows[:, k])
        assert np.all((a == 0) | (a == PI32)), "bin %d: %r" % (k, a[(a != 0) & (a != PI32)][:4])
    # and pi where the model's bin is negative, wherever the bound tells the two apart
    ref = np.concatenate([m[1] for m in gi.batch(N)["model"]])
    bnd = np.concatenate([bd[1] for bd in gi.batch(N)["bound"]])
    for k in (0, H - 1):
        sure = bnd[:, k] < 1.0
        assert np.any(np.abs(ref[sure, k]) > 3) and np.any(ref[sure, k] == 0)
        np.testing.assert_array_equal(np.abs(rows[sure, k]) == PI32, np.abs(ref[sure, k]) > 3)
    # stores: nothing outside the H columns of the F rows
    assert np.all(r["phase"][:ROW_GUARD] == SENT) and np.all(r["phase"][ROW_GUARD + r["F"]:] == SENT)
    assert np.all(r["phase"][:, H:] == SENT)
    assert not np.any(rows == SENT)
    # without phase rows (every iteration but the last) the signal is the same, bit for bit
    plain = _case_plain(N, fpr)["out"]
    diff = np.flatnonzero(_bits(plain) != _bits(r["out"]))
    if diff.size:
        print("plain != phase %d/%s: %d samples of %d, first %d last %d, worst |d| %.4g" % (
            N, fpr, diff.size, r["total"], diff[0] - GUARD, diff[-1] - GUARD, np.max(np.abs(plain[diff] - r["out"][diff]))))
    assert diff.size == 0


@pytest.mark.parametrize("N,fpr", CASES, ids=CASE_IDS)
def test_exact_zero_frames(N, fpr):
    b = gi.batch(N)
    r = _case(N, fpr)
    per = _per_utt(N, r)
    u, sig, rows = per[gi.SILENT]
    assert np.all(rows == 0.0), "silence: phase rows not exactly 0"
    assert np.max(np.abs(b["model"][u][0])) > 0.5            # T != 0: a response, not silence
    for rr, name in ((r, "phase"), (_case_plain(N, fpr), "plain")):
        frac = _figures(N, rr, "zero %d/%s %s" % (N, fpr, name), silent=True)[0]
        within(frac, 1.0, "GLK_ZERO_BOUND:%d" % N)
    # all-zero frames inside the loud utterances
    n_zero = 0
    for u, sig, rows in per:
        if u != gi.SILENT:
            dead = b["model"][u][3] == 0
            n_zero += int(dead.sum())
            assert np.all(rows[dead] == 0.0)
    assert n_zero > 0


@pytest.mark.parametrize("exp", gi.SCALE_EXPS)
@pytest.mark.parametrize("N", gi.FFT_LENS)
def test_rescaling_branch(N, exp):
    r = _case(N, None, exp)
    f_sig, f_peak, f_ph, f_wph = _figures(N, r, "scale %d/2^%d" % (N, exp))
    within(f_sig, 1.0, "GLK_SCALE_BOUND:%d" % N)
    within(f_ph, 1.0, "GLK_SCALE_PHASE_BOUND:%d" % N)
    within(f_peak, GLK_ITER_TOL[N], "GLK_ITER_TOL:%d" % N)
    within(f_wph, GLK_PHASE_TOL[N], "GLK_PHASE_TOL:%d" % N)
    _discipline(N, r, exp)
    plain = _case_plain(N, None, exp)                         # the launch without phase rows
    f_sig, f_peak, _, _ = _figures(N, plain, "scale %d/2^%d plain" % (N, exp))
    within(f_sig, 1.0, "GLK_SCALE_BOUND:%d" % N)
    within(f_peak, GLK_ITER_TOL[N], "GLK_ITER_TOL:%d" % N)
    _discipline(N, plain, exp)


def _discipline(N, r, exp):
    d_sig, h_sig, d_t, h_t, ld = _inputs(N, exp)
    H = N // 2 + 1
    total, F = r["total"], r["F"]
    out = r["out"]
    assert np.all(out[:GUARD] == SENT), "written before sig_out"
    assert np.all(out[GUARD + total:] == SENT), "written past total_out"
    body = out[GUARD:GUARD + total]
    assert not np.isnan(body).any(), "NaN in sig_out: a read outside the signal, of a pad column or of an unwritten strip"
    assert not np.any(body == SENT), "samples of [0, total_out) not written"
    assert np.all(np.isfinite(body))
    if r["phase"] is not None:
        rows = r["phase"][ROW_GUARD:ROW_GUARD + F, :H]
        assert not np.isnan(rows).any() and not np.any(rows == SENT)
    assert np.all(r["strips"][:GUARD] == SENT) and np.all(r["strips"][GUARD + r["n_strip"]:] == SENT), "strips' guards"
    assert np.array_equal(r["sig_after"].view(np.uint32), h_sig.view(np.uint32)), "sig_in written"
    assert np.array_equal(r["target_after"].view(np.uint32), h_t.view(np.uint32)), "target written"


@pytest.mark.parametrize("N,fpr", CASES, ids=CASE_IDS)
def test_memory_discipline(N, fpr):
    r = _case(N, fpr)
    _discipline(N, r, 0)
    _discipline(N, _case_plain(N, fpr), 0)
    again = _launch(N, fpr, 0)                               # fresh sentinel and NaN buffers
    assert np.array_equal(_bits(again["out"]), _bits(r["out"])), "a second launch differs"
    assert np.array_equal(_bits(again["phase"]), _bits(r["phase"])), "a second launch's phase rows differ"
