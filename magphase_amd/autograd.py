"""
Autograd for the batch API: every path is a torch.autograd.Function around the UNCHANGED forward launches, with the
backward pass in hand-written kernels.  Imported lazily by magphase.py and libaudio.py, and only under hostmath.wants_grad's
rule (return_device, grad mode on, a device tensor that requires grad).  Every gradient comes back in its input's own dtype
and shape; host arrays and inputs that need no gradient get None.

entry function                forward -> backward                                 differentiable | not             DESIGN.md
synthesize                    Lossless[ConstRate]SynthesisPlan.run                m_mag, m_real, m_imag            3.3h
                                -> .run_backward                                    | v_f0, fs
analyze                       LosslessAnalysisPlan.run -> .run_backward           v_sig | v_pm_sec, v_voi, fs      3.3i
analyze_const_rate            LosslessConstRateAnalysisPlan.run -> .run_backward  v_sig | v_pm_sec, v_voi, fs,     3.3i
                                                                                    const_rate_ms
analyze_compressed            CompressedAnalysisPlan.run -> .run_backward         v_sig | v_pm_sec, v_voi, fs      3.3j
synthesize_compressed         CompressedSynthesisPlan.run, Engine.output_hpf      m_mag_mel_log, m_real_mel,       3.3k
                                -> .adjoint_hpf, .run_backward                      m_imag_mel | v_lf0, fs, noise
synthesize_compressed_type2   Type2SynthesisPlan.run, output_hpf('ellip60')       the same three | v_lf0, fs,      3.3l
                                -> .adjoint_hpf('ellip60'), .run_backward           hf_slope_coeff, noise, its gain
true_envelope                 Engine.true_envelope                                the matrices | thres_db, the     3.3m
                                -> Engine.true_envelope_backward                    stop test (pass counts held)
analyze_type2                 Type2AnalysisPlan.run -> .run_backward              v_sig | v_pm_sec, v_voi, fs,     3.3m
analyze_compressed_type2      Type2CompressedAnalysisPlan.run -> .run_backward      the per-frame gain             3.3m
mlpg                          Engine.mlpg_streams -> .mlpg_streams_backward       the means, with var_grad the     3.3n
                                (var_grad: .mlpg_streams_var_backward)              variances | windows
mlpg_trajectory_nll           Engine.mlpg_solve, .mlpg_trajectory_nll             the means, device variances      3.3n
                                -> .mlpg_trajectory_nll_backward                    | targets, windows
synthesize_from_mag           MagnitudeSynthesisPlan.run, Engine.output_hpf       m_mag_mel_log | v_lf0, fs,       3.3o
                                -> .adjoint_hpf, .run_backward                      noise and its gains
min_phase                     Engine.min_phase_rows -> .min_phase_backward        the magnitudes (not where m<=0)  3.3o
post_filter                   Engine.post_filter[_merlin]                         the log-mel magnitudes | fs,     3.3p
                                -> Engine.post_filter[_merlin]_backward             pf_coef, av_* / boost_*
acoustic_compose              Engine.cmp_pack, .cmp_neighbours, .cmp_compose      every stream's statics (unvoiced 3.3q
                                -> Engine.cmp_compose_backward                      lf0: 0) | voicing, norm,
                                                                                    windows, unv_fill

No double backward.  synthesis_from_compressed_batch with per_phase_type 'min_phase' / 'linear' (synthesis_from_mag_batch
is the differentiable form) and any synthesis with a post-filter, with pcm16_norm or with prepared= have no backward
pass.
"""
from collections import namedtuple
from itertools import accumulate

import torch
from torch.autograd.function import once_differentiable


# ------------------------------------------------------------------------------------------------------------------
# the scaffold: what every Function below does with its inputs' descriptions and with the gradients (any device)
# ------------------------------------------------------------------------------------------------------------------
def _like(inputs):
    """Per input what its gradient has to look like: (dtype, shape) of a tensor, None for a host array."""
    return [(m.dtype, tuple(m.shape)) if torch.is_tensor(m) else None for m in inputs]


def _coerce(g, dtype=torch.float32, unit_cols=False):
    """An incoming gradient as the kernels read it: of dtype and contiguous (unit_cols: a unit column stride is enough) --
    the tensor itself where it already is, a converted contiguous copy otherwise.  None (nobody differentiated that
    output) stays None."""
    if g is None:
        return None
    ok = g.stride(1) == 1 if unit_cols else g.is_contiguous()
    return g if g.dtype == dtype and ok else g.to(dtype).contiguous()


def _offsets(rows):
    """Row offsets [0, r0, r0 + r1, ...] of consecutive blocks of rows[i] rows."""
    return [0] + list(accumulate(int(n) for n in rows))


def _scatter(g, offs, like, need_in):
    """A batch gradient cut back into per-input gradients.  g: ONE tensor whose rows offs[i]:offs[i + 1] belong to input i,
    or a tuple of k stream tensors (None where no input of that stream needs one) for inputs that come utterance-major,
    k per utterance (input i = stream i % k of utterance i // k, rows offs[i // k]:offs[i // k + 1]).  like: _like() of the
    inputs; need_in: their needs_input_grad.  -> per input its rows in the input's dtype and shape, or None for a host
    array and for an input that needs no gradient."""
    streams = g if isinstance(g, (tuple, list)) else (g,)
    k = len(streams)
    out = []
    for i, (lk, need) in enumerate(zip(like, need_in)):
        if lk is None or not need:
            out.append(None)
        else:
            out.append(streams[i % k][offs[i // k]:offs[i // k + 1]].to(lk[0]).reshape(lk[1]))
    return tuple(out)


# ------------------------------------------------------------------------------------------------------------------
# lossless synthesis: packs its inputs itself and keeps them
# ------------------------------------------------------------------------------------------------------------------
class _LosslessSynthesis(torch.autograd.Function):
    """forward(plan, cat_fn, n_utts, *mats): mats = the batch's matrices, utterance-major (m_mag_0, m_real_0, m_imag_0,
    m_mag_1, ...: tensors or host arrays); cat_fn(feats) -> the three packed float32 device matrices (magphase.py's
    _feats_cat_device: Engine.pack_rows); plan.run(...) is the forward launch, plan.run_backward(...) the backward one.
    Output: the ONE float32 [total_out] waveform buffer; the per-utterance signals are views of it."""

    @staticmethod
    def forward(ctx, plan, cat_fn, n_utts, *mats):
        feats = [tuple(mats[3 * u:3 * u + 3]) for u in range(n_utts)]
        cat = cat_fn(feats)
        pcm = plan.run(cat[0], cat[1], cat[2])
        ctx.plan = plan
        ctx.offs = _offsets(f[0].shape[0] for f in feats)
        ctx.like = _like(mats)
        ctx.save_for_backward(*cat)
        return pcm

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        mag, real, imag = ctx.saved_tensors
        n_head = 3   # plan, cat_fn, n_utts
        need_in = ctx.needs_input_grad[n_head:]
        need = tuple(any(need_in[k::3]) for k in range(3))
        grad_out = _coerce(grad_out)
        with torch.cuda.device(grad_out.device):
            g = ctx.plan.run_backward(grad_out, mag, real, imag, need=need)
        return (None,) * n_head + _scatter(g, ctx.offs, ctx.like, need_in)


def synthesize(plan, cat_fn, feats):
    """plan.run on the packed matrices of feats = [(m_mag, m_real, m_imag, ...)], differentiable with respect to the
    matrices that are tensors requiring grad.  Returns the float32 [total_out] waveform buffer (with grad_fn)."""
    plan.check_differentiable()
    mats = [x for f in feats for x in f[:3]]
    return _LosslessSynthesis.apply(plan, cat_fn, len(feats), *mats)


# ------------------------------------------------------------------------------------------------------------------
# signal -> rows: the four analyses
# ------------------------------------------------------------------------------------------------------------------
# What is particular to one analysis.  run(plan) -> its outputs as ONE flat tuple, the three differentiable float32
# matrices first (anything after them is marked non-differentiable); keep: the indices of the outputs kept for the backward
# pass; backward(plan, kept, grads) -> the float32 [total_smpls] sample gradient, grads = the three matrices' gradients
# (contiguous float32, or None for an output nobody differentiated: not read by the kernels); n_smpls(plan): the utterances'
# sample counts.
_AnalysisPath = namedtuple("_AnalysisPath", "run keep backward n_smpls")


def _run_type2_compressed(plan):
    (mag, real, imag), gain, iters = plan.run(want_iters=True)
    return mag, real, imag, gain, iters


# the three [total_frames x H] matrices; all three are kept (X = mag (real + j imag): nothing else is)
_LOSSLESS = _AnalysisPath(run=lambda p: p.run(), keep=(0, 1, 2),
                          backward=lambda p, kept, grads: p.run_backward(kept[0], kept[1], kept[2], grads),
                          n_smpls=lambda p: p.n_smpls)
# the three [total_out_frames x H] constant-rate matrices; nothing is kept (the variable-rate rows are recomputed)
_CONST_RATE = _AnalysisPath(run=lambda p: p.run(), keep=(),
                            backward=lambda p, kept, grads: p.run_backward(grads),
                            n_smpls=lambda p: p.lossless.n_smpls)
# [total_out_frames x mag_dim], [.. x phase_dim] twice: only these three small matrices are kept
_COMPRESSED = _AnalysisPath(run=lambda p: p.run(), keep=(0, 1, 2),
                            backward=lambda p, kept, grads: p.run_backward(kept, grads),
                            n_smpls=lambda p: p.lossless.n_smpls)
# (env, real, imag [total_frames x H]; the float64 per-frame gain, the int32 passes per envelope row): the pass counts only
# are kept -- both sets of rows are recomputed
_TYPE2 = _AnalysisPath(run=lambda p: p.run(want_iters=True), keep=(4,),
                       backward=lambda p, kept, grads: p.run_backward(grads, kept[0]),
                       n_smpls=lambda p: p.lossless.n_smpls)
# (mag, real, imag as _COMPRESSED; gain, passes): the three small matrices and the pass counts are kept
_TYPE2_COMPRESSED = _AnalysisPath(run=_run_type2_compressed, keep=(0, 1, 2, 4),
                                  backward=lambda p, kept, grads: p.run_backward(kept[:3], grads, kept[3]),
                                  n_smpls=lambda p: p.t2.lossless.n_smpls)


class _Analysis(torch.autograd.Function):
    """forward(path, plan, *sigs): plan = an analysis plan built from the utterances whose v_sig are sigs (tensors or host
    arrays; the plan holds the samples as one float32 device buffer already), path = its _AnalysisPath.  Outputs: path.run's;
    the per-utterance results are row views of them."""

    @staticmethod
    def forward(ctx, path, plan, *sigs):
        outs = tuple(path.run(plan))
        ctx.path, ctx.plan = path, plan
        ctx.like = _like(sigs)
        ctx.set_materialize_grads(False)     # an output nobody differentiated arrives as None: not read by the kernels
        if outs[3:]:
            ctx.mark_non_differentiable(*outs[3:])
        ctx.save_for_backward(*(outs[k] for k in path.keep))
        return outs

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        kept = ctx.saved_tensors
        path, plan = ctx.path, ctx.plan
        grads = tuple(_coerce(g) for g in grads[:3])
        # (a path that keeps nothing: the device of the first gradient given -- backward() is not called without one)
        dev = kept[0].device if kept else next(g for g in grads if g is not None).device
        with torch.cuda.device(dev):
            gsig = path.backward(plan, kept, grads)
        return (None, None) + _scatter(gsig, _offsets(path.n_smpls(plan)), ctx.like, ctx.needs_input_grad[2:])


def _analyze(path, plan, sigs):
    plan.check_differentiable()      # what has no backward pass says so before the forward is launched
    return _Analysis.apply(path, plan, *sigs)


def analyze(plan, sigs):
    """plan.run(), differentiable with respect to the v_sig in sigs that are tensors requiring grad.  Returns the three
    float32 [total_frames x H] matrices (with grad_fn)."""
    return _analyze(_LOSSLESS, plan, sigs)


def analyze_const_rate(plan, sigs):
    """plan.run() of a LosslessConstRateAnalysisPlan, differentiable with respect to the v_sig in sigs that are tensors
    requiring grad.  Returns the three float32 [total_out_frames x H] matrices (with grad_fn)."""
    return _analyze(_CONST_RATE, plan, sigs)


def analyze_compressed(plan, sigs):
    """plan.run() of a CompressedAnalysisPlan, differentiable with respect to the v_sig in sigs that are tensors requiring
    grad.  Returns the three float32 device matrices (with grad_fn)."""
    return _analyze(_COMPRESSED, plan, sigs)


def analyze_type2(plan, sigs):
    """plan.run(want_iters=True) of a Type2AnalysisPlan, differentiable with respect to the v_sig in sigs that are tensors
    requiring grad.  Returns (env, real, imag, gain, iters) as plan.run does, the three matrices with grad_fn."""
    return _analyze(_TYPE2, plan, sigs)


def analyze_compressed_type2(plan, sigs):
    """plan.run(want_iters=True) of a Type2CompressedAnalysisPlan, differentiable with respect to the v_sig in sigs that are
    tensors requiring grad.  Returns ((mag, real, imag) with grad_fn, gain)."""
    mag, real, imag, gain, _iters = _analyze(_TYPE2_COMPRESSED, plan, sigs)
    return (mag, real, imag), gain


# ------------------------------------------------------------------------------------------------------------------
# coefficients -> waveform: the compressed, the type-2 and the magnitude-only synthesis
# ------------------------------------------------------------------------------------------------------------------
class _Synthesis(torch.autograd.Function):
    """forward(plan, k, hpf, pass_need, *mats): plan = a CompressedSynthesisPlan (or one of its subclasses) built from the
    utterances whose coefficient matrices are mats, utterance-major, k per utterance (tensors or host arrays; the plan holds
    them packed as float32 device rows already); hpf = the output high-pass' design or None.  plan.run() and Engine.output_hpf
    are the forward, plan.adjoint_hpf and plan.run_backward (given need= per stream with pass_need) the backward.  Output:
    the ONE [total_out] waveform buffer (float64 after the high-pass, float32 without it); the per-utterance signals are
    views of it.  Nothing is saved: the backward pass reads the plan's work buffers."""

    @staticmethod
    def forward(ctx, plan, k, hpf, pass_need, *mats):
        pcm = plan.run()
        if hpf:
            pcm = plan.engine.output_hpf(pcm, plan.out_off_host, plan.fs, design=hpf)
        ctx.plan, ctx.k, ctx.hpf, ctx.pass_need = plan, k, hpf, pass_need
        ctx.offs = _offsets(m.shape[0] for m in mats[::k])
        ctx.like = _like(mats)
        return pcm

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        plan, k = ctx.plan, ctx.k
        n_head = 4   # plan, k, hpf, pass_need
        need_in = ctx.needs_input_grad[n_head:]
        kw = dict(need=tuple(any(need_in[s::k]) for s in range(k))) if ctx.pass_need else {}
        with torch.cuda.device(grad_out.device):
            g = plan.adjoint_hpf(grad_out, design=ctx.hpf) if ctx.hpf else grad_out
            g = plan.run_backward(_coerce(g), **kw)
        return (None,) * n_head + _scatter(g, ctx.offs, ctx.like, need_in)


def _synthesize(plan, k, hpf, pass_need, mats):
    plan.check_differentiable()      # what has no backward pass says so before the forward is launched
    return _Synthesis.apply(plan, k, hpf, pass_need, *mats)


def synthesize_compressed(plan, b_out_hpf, utts):
    """plan.run() of a CompressedSynthesisPlan (and the output high-pass), differentiable with respect to the coefficient
    matrices in utts = [(m_mag_mel_log, m_real_mel, m_imag_mel, v_lf0)] that are tensors requiring grad.  Returns the
    [total_out] waveform buffer (with grad_fn)."""
    return _synthesize(plan, 3, "butter40" if b_out_hpf else None, True, [x for u in utts for x in u[:3]])


def synthesize_compressed_type2(plan, utts):
    """plan.run() of a Type2SynthesisPlan and the elliptic output high-pass, differentiable with respect to the coefficient
    matrices in utts = [(m_mag_mel_log, m_real_mel, m_imag_mel, v_lf0)] that are tensors requiring grad.  Returns the
    float64 [total_out] waveform buffer (with grad_fn)."""
    return _synthesize(plan, 3, "ellip60", True, [x for u in utts for x in u[:3]])


def synthesize_from_mag(plan, b_out_hpf, utts):
    """plan.run() of a MagnitudeSynthesisPlan (and the output high-pass), differentiable with respect to the
    m_mag_mel_log in utts = [(m_mag_mel_log, v_lf0)] that are tensors requiring grad.  Returns the [total_out] waveform
    buffer (with grad_fn)."""
    return _synthesize(plan, 1, "butter40" if b_out_hpf else None, False, [u[0] for u in utts])


# ------------------------------------------------------------------------------------------------------------------
# the rest: engine calls with a forward / backward of their own
# ------------------------------------------------------------------------------------------------------------------
class _TrueEnvelope(torch.autograd.Function):
    """forward(engine, in_type, ncoeffs, thres_db, *mats): mats = the [F_i x H] matrices of la.true_envelope_batch (tensors
    or host arrays); Engine.true_envelope is the forward launch, Engine.true_envelope_backward the backward one.  Outputs:
    the ONE float32 [sum F_i x ld] buffer of envelope rows (the per-matrix results are views of it) and the int32 passes
    per row (not differentiable).  Kept for the backward pass: the packed float32 input rows and the pass counts."""

    @staticmethod
    def forward(ctx, engine, in_type, ncoeffs, thres_db, *mats):
        out, offs, iters, x = engine.true_envelope(list(mats), in_type, ncoeffs, thres_db, want_iters=True,
                                                   return_input=True)
        ctx.engine, ctx.in_type, ctx.ncoeffs = engine, in_type, ncoeffs
        ctx.offs, ctx.n_bins = [int(o) for o in offs], int(mats[0].shape[1])
        ctx.like = _like(mats)
        ctx.mark_non_differentiable(iters)
        ctx.save_for_backward(x, iters)
        return out, iters

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out, _grad_iters):
        x, iters = ctx.saved_tensors
        n_head = 4   # engine, in_type, ncoeffs, thres_db
        grad_out = _coerce(grad_out, unit_cols=True)
        with torch.cuda.device(x.device):
            g = ctx.engine.true_envelope_backward(x, iters, grad_out, ctx.n_bins, ctx.in_type, ctx.ncoeffs)
        return (None,) * n_head + _scatter(g[:, :ctx.n_bins], ctx.offs, ctx.like, ctx.needs_input_grad[n_head:])


def true_envelope(engine, mats, in_type, ncoeffs, thres_db):
    """Engine.true_envelope on mats, differentiable with respect to the matrices that are tensors requiring grad.  Returns
    (the float32 [sum F_i x ld] envelope buffer with grad_fn, the row offsets, the int32 passes per row)."""
    import numpy as np

    out, iters = _TrueEnvelope.apply(engine, in_type, int(ncoeffs), float(thres_db), *mats)
    offs = np.concatenate(([0], np.cumsum([int(m.shape[0]) for m in mats]))).astype(np.int64)
    return out, offs, iters


class _MLPG(torch.autograd.Function):
    """forward(engine, var, streams, windows, width, *means): means = the [F_i x width] mean matrices of mp.mlpg_batch /
    mp.mlpg_streams_batch (tensors or host arrays), var = the device variances ([width] or [sum F_i x width]), streams =
    [(first column, D), ...].  Engine.mlpg_streams is the forward launch (one mpx_mlpg_solve per stream).  Output: the ONE
    float64 [sum F_i x sum D] buffer of trajectories.  The backward pass keeps no factor: per stream it solves A z = g
    again from the variances (mpx_mlpg_solve with the right-hand side given) and applies P_k W_k (mpx_mlpg_apply).  Kept:
    the variances and the frame offsets -- MLPG is linear in the means, so the means themselves are not.
    The variance path (n_means < len(mats): mats = the means, then the caller's variance tensors -- ONE [width] global row
    or one [F_i x width] matrix per utterance, of which var is the packed, detached device form): the packed means and the
    output are kept as well, and Engine.mlpg_streams_var_backward adds mpx_mlpg_var_backward to the two launches above."""

    @staticmethod
    def forward(ctx, engine, var, streams, windows, width, n_means, *mats):
        import numpy as np

        means, var_in = mats[:n_means], mats[n_means:]
        buf, offs = engine.mlpg_pack(list(means), width)
        offs_dev = engine.to_device(offs.astype(np.int32), np.int32)
        out = engine.mlpg_streams(buf, var, offs_dev, streams, windows)
        ctx.engine, ctx.streams, ctx.windows, ctx.width, ctx.n_means = engine, streams, windows, width, n_means
        ctx.offs = [int(o) for o in offs]
        ctx.like = _like(mats)
        if var_in:
            ctx.save_for_backward(var, offs_dev, buf, out)
        else:
            ctx.save_for_backward(var, offs_dev)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        n_head = 6   # engine, var, streams, windows, width, n_means
        n = ctx.n_means
        need_in = ctx.needs_input_grad[n_head:]
        grad_out = _coerce(grad_out, dtype=torch.float64)
        if len(ctx.like) == n:
            var, offs_dev = ctx.saved_tensors
            with torch.cuda.device(var.device):
                g = ctx.engine.mlpg_streams_backward(grad_out, var, offs_dev, ctx.streams, ctx.windows, ctx.width)
            return (None,) * n_head + _scatter(g, ctx.offs, ctx.like, need_in)
        var, offs_dev, buf, out = ctx.saved_tensors
        with torch.cuda.device(var.device):
            g, gv = ctx.engine.mlpg_streams_var_backward(grad_out, buf, out, var, offs_dev, ctx.streams, ctx.windows,
                                                         ctx.width, need_mean=any(need_in[:n]))
        g_means = _scatter(g, ctx.offs, ctx.like[:n], need_in[:n]) if g is not None else (None,) * n
        return (None,) * n_head + g_means + _var_grads(gv, ctx.offs, ctx.like[n:], need_in[n:])


def _var_grads(gv, offs, like, need_in):
    """The variances' gradient cut back to the caller's tensors: a [width] vector for the ONE global row, else the rows of
    a [sum F_i x width] matrix per utterance."""
    if gv.dim() == 1:
        return (gv.to(like[0][0]).reshape(like[0][1]) if like[0] is not None and need_in[0] else None,)
    return _scatter(gv, offs, like, need_in)


def mlpg(engine, means, var, streams, windows, width, var_inputs=()):
    """Engine.mlpg_streams on the packed means, differentiable with respect to the mean matrices that are tensors
    requiring grad and to var_inputs (the caller's variance tensors behind the device form var: the one global row, or
    one matrix per utterance; empty: the variances get no gradient).  The windows get none.  -> the float64
    [sum F_i x sum D] buffer with grad_fn."""
    return _MLPG.apply(engine, var, streams, windows, int(width), len(means), *means, *var_inputs)


class _MLPGTrajectoryNLL(torch.autograd.Function):
    """forward(engine, var, x, windows, D, n_means, *mats): mats = the [F_i x K D] mean matrices of
    mp.mlpg_trajectory_nll_batch, then the caller's variance tensors (as in _MLPG; none: no gradient for them); var = the
    device variances, x = the packed static targets [sum F_i x D] (no gradient).  Forward: mpx_mlpg_solve, then
    mpx_mlpg_trajectory_nll.  Output: float64 [n_utts x D].  Kept: the packed means, the variances, the trajectory, the
    targets and the frame offsets; the backward pass is ONE mpx_mlpg_trajectory_nll_backward launch (and the column pass
    for a global variance row)."""

    @staticmethod
    def forward(ctx, engine, var, x, windows, D, n_means, *mats):
        import numpy as np

        means = mats[:n_means]
        K = int(windows.shape[0]) + 1
        buf, offs = engine.mlpg_pack(list(means), K * D)
        offs_dev = engine.to_device(offs.astype(np.int32), np.int32)
        c = engine.mlpg_solve(buf, var, offs_dev, D, windows)
        nll = engine.mlpg_trajectory_nll(c, x, var, offs_dev, D, windows)
        ctx.engine, ctx.windows, ctx.D, ctx.n_means = engine, windows, D, n_means
        ctx.offs = [int(o) for o in offs]
        ctx.like = _like(mats)
        ctx.save_for_backward(var, offs_dev, buf, c, x)
        return nll

    @staticmethod
    @once_differentiable
    def backward(ctx, go):
        var, offs_dev, buf, c, x = ctx.saved_tensors
        n_head = 6   # engine, var, x, windows, D, n_means
        n = ctx.n_means
        need_in = ctx.needs_input_grad[n_head:]
        go = _coerce(go, dtype=torch.float64)
        with torch.cuda.device(var.device):
            g, gv = ctx.engine.mlpg_trajectory_nll_backward(buf, var, c, x, go, offs_dev, ctx.D, ctx.windows,
                                                            need_mean=any(need_in[:n]), need_var=any(need_in[n:]))
        g_means = _scatter(g, ctx.offs, ctx.like[:n], need_in[:n]) if g is not None else (None,) * n
        g_vars = _var_grads(gv, ctx.offs, ctx.like[n:], need_in[n:]) if gv is not None else (None,) * (len(ctx.like) - n)
        return (None,) * n_head + g_means + g_vars


def mlpg_trajectory_nll(engine, means, var, x, windows, D, var_inputs=()):
    """The trajectory likelihood of the packed targets x under MLPG of the means, differentiable with respect to the mean
    matrices that are tensors requiring grad and to var_inputs (as in mlpg()).  -> float64 [n_utts x D] with grad_fn."""
    return _MLPGTrajectoryNLL.apply(engine, var, x, windows, int(D), len(means), *means, *var_inputs)


class _MinPhase(torch.autograd.Function):
    """forward(engine, *mats): mats = the [F_i x H] magnitude matrices of la.build_min_phase_from_mag_spec_batch (tensors or
    host arrays); Engine.min_phase_rows (ONE mpx_min_phase launch over all rows) is the forward, mpx_min_phase_backward the
    backward.  Outputs: the unit phasor rows (cos phi, sin phi) of all matrices, float32 [sum F_i x H] views at the spectra's
    row pitch; the product with the magnitudes is the caller's (plain torch).  Kept for the backward pass: the three rows
    the forward wrote.  The incoming gradients go to the kernel as they arrive."""

    @staticmethod
    def forward(ctx, engine, *mats):
        o_m, o_r, o_i = engine.min_phase_rows(list(mats))
        ctx.engine = engine
        ctx.offs = _offsets(m.shape[0] for m in mats)
        ctx.like = _like(mats)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(o_m, o_r, o_i)
        return o_r, o_i

    @staticmethod
    @once_differentiable
    def backward(ctx, g_r, g_i):
        o_m, o_r, o_i = ctx.saved_tensors
        with torch.cuda.device(o_m.device):
            g = ctx.engine.min_phase_backward(o_m, o_r, o_i, None, g_r, g_i)
        return (None,) + _scatter(g, ctx.offs, ctx.like, ctx.needs_input_grad[1:])


def min_phase(engine, mats):
    """Engine.min_phase_rows on mats, differentiable with respect to the matrices that are tensors requiring grad.
    Returns the float32 (cos phi, sin phi) row matrices of the whole batch (with grad_fn)."""
    return _MinPhase.apply(engine, *mats)


class _PostFilter(torch.autograd.Function):
    """forward(engine, pf_type, fs, opts, *mats): mats = the [F_i x D] log-mel magnitude matrices of mp.post_filter_batch
    (tensors or host arrays), opts = the filter's options as sorted (name, value) pairs; Engine.post_filter_pack (ONE
    mpx_rows_pack launch) and Engine.post_filter / Engine.post_filter_merlin are the forward, Engine.post_filter_backward /
    Engine.post_filter_merlin_backward the backward.  Output: the ONE float32 [sum F_i x D] buffer of filtered rows (the
    per-utterance results are row views of it).  Kept for the backward pass: the packed input rows ('merlin' only)."""

    @staticmethod
    def forward(ctx, engine, pf_type, fs, opts, *mats):
        x, offs = engine.post_filter_pack(list(mats))
        kw = dict(opts)
        out = engine.post_filter_merlin(x, fs, **kw) if pf_type == "merlin" else engine.post_filter(x, fs, **kw)
        ctx.engine, ctx.pf_type, ctx.fs, ctx.kw = engine, pf_type, fs, kw
        ctx.offs = [int(o) for o in offs]
        ctx.like = _like(mats)
        if pf_type == "merlin":
            ctx.save_for_backward(x)
        else:
            ctx.save_for_backward()
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        n_head = 4   # engine, pf_type, fs, opts
        with torch.cuda.device(grad_out.device):
            if ctx.pf_type == "merlin":
                (x,) = ctx.saved_tensors
                g = ctx.engine.post_filter_merlin_backward(x, grad_out, ctx.fs, **ctx.kw)
            else:
                ctx.saved_tensors   # (none kept; raises as torch does when the graph was freed)
                g = ctx.engine.post_filter_backward(grad_out, ctx.fs, **ctx.kw)
        return (None,) * n_head + _scatter(g, ctx.offs, ctx.like, ctx.needs_input_grad[n_head:])


class _AcousticCompose(torch.autograd.Function):
    """forward(engine, dims, interp, vuv, windows, norm, unv_fill, *mats): mats = the streams of mp.acoustic_compose_batch,
    utterance-major, len(dims) per utterance ([F_i x dims[s]] tensors or host arrays).  Engine.cmp_pack,
    Engine.cmp_neighbours and Engine.cmp_compose are the forward, Engine.cmp_compose_backward (ONE
    mpx_cmp_compose_backward launch) the backward.  Output: the ONE float32 [sum F_i x W] buffer of composed rows (the
    per-utterance results are row views of it).  Kept: the neighbour table, the frame offsets and std -- the composition
    is linear in the voiced statics, so the statics themselves are not."""

    @staticmethod
    def forward(ctx, engine, dims, interp, vuv, windows, norm, unv_fill, *mats):
        import numpy as np

        k = len(dims)
        utts = [list(mats[i:i + k]) for i in range(0, len(mats), k)]
        x, offs = engine.cmp_pack(utts, dims)
        offs_dev = engine.to_device(offs.astype(np.int32), np.int32)
        nb = engine.cmp_neighbours(x[:, int(sum(dims[:interp]))], offs_dev) if interp >= 0 else None
        mean, std = engine._cmp_norm(norm, (int(windows.shape[0]) + 1) * int(sum(dims)) + int(vuv))
        out = engine.cmp_compose(x, nb, offs_dev, dims, interp, vuv, windows, norm=norm and (mean, std), unv_fill=unv_fill)
        ctx.engine, ctx.dims, ctx.interp, ctx.vuv, ctx.windows = engine, dims, interp, vuv, windows
        ctx.offs = [int(o) for o in offs]
        ctx.like = _like(mats)
        ctx.has_nb, ctx.has_std = nb is not None, std is not None
        ctx.save_for_backward(offs_dev, *([nb] if nb is not None else []), *([std] if std is not None else []))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        saved = list(ctx.saved_tensors)
        offs_dev = saved.pop(0)
        nb = saved.pop(0) if ctx.has_nb else None
        std = saved.pop(0) if ctx.has_std else None
        n_head = 7   # engine, dims, interp, vuv, windows, norm, unv_fill
        grad_out = _coerce(grad_out, unit_cols=True)
        with torch.cuda.device(grad_out.device):
            gx = ctx.engine.cmp_compose_backward(grad_out, nb, offs_dev, ctx.dims, ctx.interp, ctx.vuv, ctx.windows, std=std)
        cols = _offsets(ctx.dims)
        g = tuple(gx[:, a:b] for a, b in zip(cols[:-1], cols[1:]))
        return (None,) * n_head + _scatter(g, ctx.offs, ctx.like, ctx.needs_input_grad[n_head:])


def acoustic_compose(engine, utts, dims, interp, vuv, windows, norm, unv_fill):
    """The composed rows of utts (per utterance the list of its streams' [F_i x dims[s]] operands), differentiable with
    respect to the streams that are tensors requiring grad.  -> (the float32 [sum F_i x W] buffer with grad_fn, the row
    offsets)."""
    import numpy as np

    out = _AcousticCompose.apply(engine, list(dims), int(interp), bool(vuv), windows, norm, float(unv_fill),
                                 *[m for u in utts for m in u])
    offs = np.concatenate(([0], np.cumsum([int(u[0].shape[0]) for u in utts]))).astype(np.int64)
    return out, offs


def post_filter(engine, mats, pf_type, fs, opts):
    """Engine.post_filter / Engine.post_filter_merlin on the packed rows of mats, differentiable with respect to the matrices
    that are tensors requiring grad.  Returns (the float32 [sum F_i x D] buffer with grad_fn, the row offsets)."""
    import numpy as np

    out = _PostFilter.apply(engine, pf_type, fs, tuple(sorted(opts.items())), *mats)
    offs = np.concatenate(([0], np.cumsum([int(m.shape[0]) for m in mats]))).astype(np.int64)
    return out, offs
