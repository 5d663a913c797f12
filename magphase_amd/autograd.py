"""
Autograd for the lossless features, both directions, for the compressed features, both directions, for the type-2 features,
both directions, and for the true envelope.  Imported lazily by
magphase.py, and only when a device tensor that requires grad goes in with return_device=True and grad mode on.

Synthesis: a torch.autograd.Function around the unchanged forward launch of
synthesis_from_lossless_batch / synthesis_from_lossless_const_rate_batch, with the gradients with respect to
m_mag / m_real / m_imag computed by k_synth_lossless_bwd (and k_rows_lerp_adjoint for constant-rate rows).
Not differentiable: v_f0 (the pitch marks are integers) and fs.

Analysis (section 3.3i): a second Function around the unchanged forward launch of analysis_lossless_batch, with the
gradient with respect to the samples v_sig computed by k_analysis_lossless_bwd and k_analysis_bwd_gather from the
forward's own output rows (X = mag (real + j imag): nothing else is kept).  Not differentiable: v_pm_sec, v_voi and fs
(the epochs are rounded to samples); v_f0 and v_shift come from the host and carry no grad_fn.  Where mag^2 < 1e-37 --
the clamp region of the forward's 1 / |X|, which holds X == 0 -- the gradient with respect to X is defined as zero: a
silent frame gives zeros, never Inf or NaN.

Compressed analysis (section 3.3j): a third Function around the unchanged forward launch of analysis_compressed_batch
(CompressedAnalysisPlan.run(), whichever of its paths it takes), at the variable and the constant rate, with the gradient
with respect to the samples v_sig computed by CompressedAnalysisPlan.run_backward: the lossless rows are recomputed (only
the three small output matrices are kept), k_phase_grad_mask and k_mel_warp_bwd take the gradients back through the two
mel warps -- the phase streams' voicing mask and clip are read from the forward's own outputs, and the gradient at a
clipped element (exactly +-1.0f) is defined as zero --, k_rows_lerp_adjoint through the constant-rate interpolation, and
the lossless analysis' backward kernels do the rest.  Not differentiable: v_pm_sec, v_voi and fs; v_lf0_smth and v_shift
come from the host and carry no grad_fn.

Compressed synthesis (section 3.3k): a fourth Function around the unchanged forward of synthesis_from_compressed_batch
(the plan's packing of the coefficient rows, CompressedSynthesisPlan.run() and the output high-pass), type 1 with
per_phase_type='magphase' and no post-filter, at the variable and the constant rate, with the gradients with respect to
m_mag_mel_log / m_real_mel / m_imag_mel computed by CompressedSynthesisPlan.run_backward: the high-pass' adjoint (the same
filter run backwards in time, per utterance), k_synth_comp_bwd (per frame: the noise spectrum recomputed, the gradient
window through the anti-ringing window and one FFT, the epilogue against the forward's own unwarped rows),
k_rows_lerp_adjoint through the constant-rate interpolation and k_mel_unwarp_bwd through the two mel unwarps.  Not
differentiable: v_lf0 (it only produces integer pitch marks and the voicing flag), fs, and the noise with its two gains
(they do not depend on the features).  Bins 0 and N/2 keep |S|: where S == 0 there the gradient is defined as zero; where
a phase bin is a == b == 0 its gradient is m P gS (k_synth_lossless_bwd's convention).  A plan that stores its noise
spectra (MAGPHASE_NOISE_SPECTRA=store) is differentiated the same way: the backward pass recomputes them.

Type-2 synthesis (section 3.3l): a fifth Function around the unchanged forward of synthesis_from_compressed_type2_batch
(Type2SynthesisPlan.run() and the elliptic output high-pass), at the variable rate and at any const_rate_ms, with the
gradients computed by the same run_backward: the elliptic filter run backwards in time, k_synth_comp_bwd's type-2 arm
(bins 0 and N/2 keep Re S, a linear map: the real end-bin gradient passes straight through), the type-2 phase unwarp
matrix and curves as the plan holds them.  The one noise gain per utterance does not depend on the features: it is held
constant and the backward pass is exact.  Not differentiable: v_lf0, fs, hf_slope_coeff, the noise and its gain.

True envelope (section 3.3m): a sixth Function around the unchanged launch of la.true_envelope_batch(return_device=True)
(Engine.true_envelope), for the three in_types and any ncoeffs, with the gradient with respect to the input matrices
computed by k_true_envelope_bwd (Engine.true_envelope_backward): the exact adjoint of the passes as the device ran them --
the forward's pass counts and its packed input rows are kept, the decisions of the max updates are recomputed on chip.  The
stop test is not differentiated (the pass count is a constant of the backward pass), so the gradient is that of the
envelope with K passes; it jumps where a decision or the pass count flips.  A row with a non-finite dB value (all NaN
in the forward) gets a zero gradient.  Not differentiable: thres_db.

Type-2 analysis (section 3.3m): a seventh and an eighth Function around the unchanged forward launches of
analysis_lossless_type2_batch (Type2AnalysisPlan.run) and analysis_compressed_type2_batch
(Type2CompressedAnalysisPlan.run), with the gradient with respect to the samples v_sig computed by the plans' run_backward:
both sets of rows are recomputed (only the envelope's pass counts and, for the compressed form, the three small matrices
are kept), k_true_envelope_bwd takes the envelope's gradient to the two-period magnitudes, the lossless analysis' backward
kernels run over the two-period and the one-period frame table and the two sample gradients are added; the compressed form
first runs the tail of the type-1 compressed backward on the type-2 row tables.  Not differentiable: v_pm_sec, v_voi, fs,
the per-frame gain.

Magnitude-only synthesis (section 3.3o): a Function around the unchanged forward of synthesis_from_mag_batch
(MagnitudeSynthesisPlan.run() -- the compressed plan with per_phase_type 'min_phase' / 'linear' -- and the output
high-pass), with the gradient with respect to m_mag_mel_log computed by MagnitudeSynthesisPlan.run_backward:
k_synth_comp_bwd against the rows the pair kernel read, k_min_phase_bwd (the adjoint of the minimum-phase stage, in
place on the magnitude gradient rows; 'min_phase' only), k_rows_lerp_adjoint and k_mel_unwarp_bwd's magnitude job.  And a
Function around la.build_min_phase_from_mag_spec_batch's one mpx_min_phase launch, magnitude rows -> unit phasor rows,
with mpx_min_phase_backward as its backward.  Where m <= 0 the phase gets no gradient (the protected logarithm is a
constant there).  Not differentiable: v_lf0, fs, the noise and its gains.

Post-filters (section 3.3p): a Function around the unchanged forward launches of Engine.post_filter (k_post_filter) and
Engine.post_filter_merlin (mpx_post_filter_merlin's four launches) on the packed float32 rows of mp.post_filter_batch, with
the gradient with respect to the log-mel magnitudes computed by k_post_filter_bwd (the MagPhase filter is linear per frame:
g_x = g_y M as a gather over the inverse of the forward's own tables; nothing is kept) and by mpx_post_filter_merlin_backward (k_rows_gemm
and k_merlin_r0_bwd: the cepstra and both frame energies are recomputed from the packed input rows, the only thing kept).
A Merlin row for which the forward wrote la.MAGIC gets a zero gradient.  Not differentiable: fs, pf_coef and the four
av_* / boost_* options.  The stage composes in front of the syntheses with b_post_filter=False.

No double backward.  synthesis_from_compressed_batch with per_phase_type 'min_phase' / 'linear' (synthesis_from_mag_batch
is the differentiable form), any synthesis with a post-filter, with pcm16_norm or with prepared=, and the constant-rate
lossless analysis, have no backward pass.
"""
import torch
from torch.autograd.function import once_differentiable


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
        ctx.rows = [int(f[0].shape[0]) for f in feats]
        ctx.like = [(m.dtype, tuple(m.shape)) if torch.is_tensor(m) else None for m in mats]
        ctx.save_for_backward(*cat)
        return pcm

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        mag, real, imag = ctx.saved_tensors
        n_head = 3   # plan, cat_fn, n_utts
        need_in = ctx.needs_input_grad[n_head:]
        need = tuple(any(need_in[k::3]) for k in range(3))
        if grad_out.dtype != torch.float32 or not grad_out.is_contiguous():
            grad_out = grad_out.to(torch.float32).contiguous()
        with torch.cuda.device(grad_out.device):
            g = ctx.plan.run_backward(grad_out, mag, real, imag, need=need)
        out, a = [], 0
        for u, n in enumerate(ctx.rows):
            for k in range(3):
                like = ctx.like[3 * u + k]
                if like is None or not need_in[3 * u + k]:
                    out.append(None)
                else:
                    out.append(g[k][a:a + n].to(like[0]).reshape(like[1]))
            a += n
        return (None,) * n_head + tuple(out)


def synthesize(plan, cat_fn, feats):
    """plan.run on the packed matrices of feats = [(m_mag, m_real, m_imag, ...)], differentiable with respect to the
    matrices that are tensors requiring grad.  Returns the float32 [total_out] waveform buffer (with grad_fn)."""
    mats = [x for f in feats for x in f[:3]]
    return _LosslessSynthesis.apply(plan, cat_fn, len(feats), *mats)


class _LosslessAnalysis(torch.autograd.Function):
    """forward(plan, *sigs): plan = a LosslessAnalysisPlan built from the utterances whose v_sig are sigs (tensors or
    host arrays; the plan holds the samples as one float32 device buffer already); plan.run() is the forward launch,
    plan.run_backward(...) the backward ones.  Outputs: the three float32 [total_frames x H] matrices of the batch; the
    per-utterance results are row views of them."""

    @staticmethod
    def forward(ctx, plan, *sigs):
        mag, real, imag = plan.run()
        ctx.plan = plan
        ctx.like = [(s.dtype, tuple(s.shape)) if torch.is_tensor(s) else None for s in sigs]
        ctx.set_materialize_grads(False)     # an output nobody differentiated arrives as None: not read by the kernel
        ctx.save_for_backward(mag, real, imag)
        return mag, real, imag

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        mag, real, imag = ctx.saved_tensors
        need_in = ctx.needs_input_grad[1:]
        grads = tuple(g if g is None or (g.dtype == torch.float32 and g.is_contiguous())
                      else g.to(torch.float32).contiguous() for g in grads)
        with torch.cuda.device(mag.device):
            gsig = ctx.plan.run_backward(mag, real, imag, grads)
        out, a = [], 0
        for like, need, n in zip(ctx.like, need_in, ctx.plan.n_smpls):
            out.append(gsig[a:a + n].to(like[0]).reshape(like[1]) if like is not None and need else None)
            a += n
        return (None,) + tuple(out)


def analyze(plan, sigs):
    """plan.run(), differentiable with respect to the v_sig in sigs that are tensors requiring grad.  Returns the three
    float32 [total_frames x H] matrices (with grad_fn)."""
    return _LosslessAnalysis.apply(plan, *sigs)


class _CompressedAnalysis(torch.autograd.Function):
    """forward(plan, *sigs): plan = a CompressedAnalysisPlan built from the utterances whose v_sig are sigs (tensors or
    host arrays); plan.run() is the forward launch, plan.run_backward(...) the backward ones.  Outputs: the three float32
    matrices of the batch ([total_out_frames x mag_dim], [.. x phase_dim] twice); the per-utterance results are row views of
    them.  Only these three are kept for the backward pass."""

    @staticmethod
    def forward(ctx, plan, *sigs):
        mag, real, imag = plan.run()
        ctx.plan = plan
        ctx.like = [(s.dtype, tuple(s.shape)) if torch.is_tensor(s) else None for s in sigs]
        ctx.set_materialize_grads(False)     # an output nobody differentiated arrives as None: not read by the kernels
        ctx.save_for_backward(mag, real, imag)
        return mag, real, imag

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        outs = ctx.saved_tensors
        need_in = ctx.needs_input_grad[1:]
        grads = tuple(g if g is None or (g.dtype == torch.float32 and g.is_contiguous())
                      else g.to(torch.float32).contiguous() for g in grads)
        with torch.cuda.device(outs[0].device):
            gsig = ctx.plan.run_backward(outs, grads)
        out, a = [], 0
        for like, need, n in zip(ctx.like, need_in, ctx.plan.lossless.n_smpls):
            out.append(gsig[a:a + n].to(like[0]).reshape(like[1]) if like is not None and need else None)
            a += n
        return (None,) + tuple(out)


def analyze_compressed(plan, sigs):
    """plan.run() of a CompressedAnalysisPlan, differentiable with respect to the v_sig in sigs that are tensors requiring
    grad.  Returns the three float32 device matrices (with grad_fn)."""
    return _CompressedAnalysis.apply(plan, *sigs)


class _CompressedSynthesis(torch.autograd.Function):
    """forward(plan, b_out_hpf, n_utts, *mats): plan = a CompressedSynthesisPlan built from the utterances whose
    coefficient matrices are mats, utterance-major (m_mag_mel_log_0, m_real_mel_0, m_imag_mel_0, m_mag_mel_log_1, ...:
    tensors or host arrays; the plan holds them packed as float32 device rows already); plan.run() and Engine.output_hpf
    are the forward, plan.adjoint_hpf and plan.run_backward the backward.  Output: the ONE [total_out] waveform buffer
    (float64 after the high-pass, float32 without it); the per-utterance signals are views of it."""

    @staticmethod
    def forward(ctx, plan, b_out_hpf, n_utts, *mats):
        pcm = plan.run()
        if b_out_hpf:
            pcm = plan.engine.output_hpf(pcm, plan.out_off_host, plan.fs)
        ctx.plan, ctx.hpf = plan, bool(b_out_hpf)
        ctx.rows = [int(mats[3 * u].shape[0]) for u in range(n_utts)]
        ctx.like = [(m.dtype, tuple(m.shape)) if torch.is_tensor(m) else None for m in mats]
        return pcm

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        plan = ctx.plan
        n_head = 3   # plan, b_out_hpf, n_utts
        need_in = ctx.needs_input_grad[n_head:]
        need = tuple(any(need_in[k::3]) for k in range(3))
        with torch.cuda.device(grad_out.device):
            if ctx.hpf:
                g = plan.adjoint_hpf(grad_out)
            else:
                g = grad_out.to(torch.float32)
            g = plan.run_backward(g.contiguous(), need=need)
        out, a = [], 0
        for u, n in enumerate(ctx.rows):
            for k in range(3):
                like = ctx.like[3 * u + k]
                if like is None or not need_in[3 * u + k]:
                    out.append(None)
                else:
                    out.append(g[k][a:a + n].to(like[0]).reshape(like[1]))
            a += n
        return (None,) * n_head + tuple(out)


def synthesize_compressed(plan, b_out_hpf, utts):
    """plan.run() of a CompressedSynthesisPlan (and the output high-pass), differentiable with respect to the coefficient
    matrices in utts = [(m_mag_mel_log, m_real_mel, m_imag_mel, v_lf0)] that are tensors requiring grad.  Returns the
    [total_out] waveform buffer (with grad_fn)."""
    mats = [x for u in utts for x in u[:3]]
    return _CompressedSynthesis.apply(plan, bool(b_out_hpf), len(utts), *mats)


class _Type2Synthesis(torch.autograd.Function):
    """forward(plan, n_utts, *mats): plan = a Type2SynthesisPlan built from the utterances whose coefficient matrices are
    mats, utterance-major as for _CompressedSynthesis; plan.run() and Engine.output_hpf(design='ellip60') are the forward,
    plan.adjoint_hpf(design='ellip60') and plan.run_backward the backward.  Output: the ONE float64 [total_out] waveform
    buffer; the per-utterance signals are views of it."""

    @staticmethod
    def forward(ctx, plan, n_utts, *mats):
        pcm = plan.engine.output_hpf(plan.run(), plan.out_off_host, plan.fs, design="ellip60")
        ctx.plan = plan
        ctx.rows = [int(mats[3 * u].shape[0]) for u in range(n_utts)]
        ctx.like = [(m.dtype, tuple(m.shape)) if torch.is_tensor(m) else None for m in mats]
        return pcm

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        plan = ctx.plan
        n_head = 2   # plan, n_utts
        need_in = ctx.needs_input_grad[n_head:]
        need = tuple(any(need_in[k::3]) for k in range(3))
        with torch.cuda.device(grad_out.device):
            g = plan.run_backward(plan.adjoint_hpf(grad_out, design="ellip60").contiguous(), need=need)
        out, a = [], 0
        for u, n in enumerate(ctx.rows):
            for k in range(3):
                like = ctx.like[3 * u + k]
                if like is None or not need_in[3 * u + k]:
                    out.append(None)
                else:
                    out.append(g[k][a:a + n].to(like[0]).reshape(like[1]))
            a += n
        return (None,) * n_head + tuple(out)


def synthesize_compressed_type2(plan, utts):
    """plan.run() of a Type2SynthesisPlan and the elliptic output high-pass, differentiable with respect to the coefficient
    matrices in utts = [(m_mag_mel_log, m_real_mel, m_imag_mel, v_lf0)] that are tensors requiring grad.  Returns the
    float64 [total_out] waveform buffer (with grad_fn)."""
    plan._check_differentiable()     # what has no backward pass says so before the forward is launched
    mats = [x for u in utts for x in u[:3]]
    return _Type2Synthesis.apply(plan, len(utts), *mats)


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
        ctx.like = [(m.dtype, tuple(m.shape)) if torch.is_tensor(m) else None for m in mats]
        ctx.mark_non_differentiable(iters)
        ctx.save_for_backward(x, iters)
        return out, iters

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out, _grad_iters):
        x, iters = ctx.saved_tensors
        n_head = 4   # engine, in_type, ncoeffs, thres_db
        need_in = ctx.needs_input_grad[n_head:]
        if grad_out.dtype != torch.float32 or grad_out.stride(1) != 1:
            grad_out = grad_out.to(torch.float32).contiguous()
        with torch.cuda.device(x.device):
            g = ctx.engine.true_envelope_backward(x, iters, grad_out, ctx.n_bins, ctx.in_type, ctx.ncoeffs)
        out = []
        for like, need, a, b in zip(ctx.like, need_in, ctx.offs[:-1], ctx.offs[1:]):
            out.append(g[a:b, :ctx.n_bins].to(like[0]).reshape(like[1]) if like is not None and need else None)
        return (None,) * n_head + tuple(out)


def true_envelope(engine, mats, in_type, ncoeffs, thres_db):
    """Engine.true_envelope on mats, differentiable with respect to the matrices that are tensors requiring grad.  Returns
    (the float32 [sum F_i x ld] envelope buffer with grad_fn, the row offsets, the int32 passes per row)."""
    import numpy as np

    out, iters = _TrueEnvelope.apply(engine, in_type, int(ncoeffs), float(thres_db), *mats)
    offs = np.concatenate(([0], np.cumsum([int(m.shape[0]) for m in mats]))).astype(np.int64)
    return out, offs, iters


class _Type2Analysis(torch.autograd.Function):
    """forward(plan, *sigs): plan = a Type2AnalysisPlan built from the utterances whose v_sig are sigs (tensors or host
    arrays); plan.run(want_iters=True) is the forward launch sequence, plan.run_backward the backward one.  Outputs: the
    three float32 [total_frames x H] matrices of the batch (envelope, real, imag; the per-utterance results are row views
    that leave out row 0), the float64 per-frame gain and the int32 passes per envelope row (neither differentiable).
    Kept for the backward pass: the pass counts only -- both sets of rows are recomputed."""

    @staticmethod
    def forward(ctx, plan, *sigs):
        env, real, imag, gain, iters = plan.run(want_iters=True)
        ctx.plan = plan
        ctx.like = [(s.dtype, tuple(s.shape)) if torch.is_tensor(s) else None for s in sigs]
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(gain, iters)
        ctx.save_for_backward(iters)
        return env, real, imag, gain, iters

    @staticmethod
    @once_differentiable
    def backward(ctx, g_env, g_real, g_imag, _g_gain, _g_iters):
        (iters,) = ctx.saved_tensors
        need_in = ctx.needs_input_grad[1:]
        grads = tuple(g if g is None or (g.dtype == torch.float32 and g.is_contiguous())
                      else g.to(torch.float32).contiguous() for g in (g_env, g_real, g_imag))
        with torch.cuda.device(iters.device):
            gsig = ctx.plan.run_backward(grads, iters)
        out, a = [], 0
        for like, need, n in zip(ctx.like, need_in, ctx.plan.lossless.n_smpls):
            out.append(gsig[a:a + n].to(like[0]).reshape(like[1]) if like is not None and need else None)
            a += n
        return (None,) + tuple(out)


def analyze_type2(plan, sigs):
    """plan.run(want_iters=True) of a Type2AnalysisPlan, differentiable with respect to the v_sig in sigs that are tensors
    requiring grad.  Returns (env, real, imag, gain, iters) as plan.run does, the three matrices with grad_fn."""
    return _Type2Analysis.apply(plan, *sigs)


class _Type2CompressedAnalysis(torch.autograd.Function):
    """forward(plan, *sigs): plan = a Type2CompressedAnalysisPlan built from the utterances whose v_sig are sigs;
    plan.run(want_iters=True) is the forward, plan.run_backward the backward.  Outputs: the three float32 matrices of the
    batch ([total_out_frames x mag_dim], [.. x phase_dim] twice), the float64 per-frame gain and the int32 passes per
    envelope row (neither differentiable).  Kept for the backward pass: the three small matrices and the pass counts."""

    @staticmethod
    def forward(ctx, plan, *sigs):
        (mag, real, imag), gain, iters = plan.run(want_iters=True)
        ctx.plan = plan
        ctx.like = [(s.dtype, tuple(s.shape)) if torch.is_tensor(s) else None for s in sigs]
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(gain, iters)
        ctx.save_for_backward(mag, real, imag, iters)
        return mag, real, imag, gain, iters

    @staticmethod
    @once_differentiable
    def backward(ctx, g_mag, g_real, g_imag, _g_gain, _g_iters):
        mag, real, imag, iters = ctx.saved_tensors
        need_in = ctx.needs_input_grad[1:]
        grads = tuple(g if g is None or (g.dtype == torch.float32 and g.is_contiguous())
                      else g.to(torch.float32).contiguous() for g in (g_mag, g_real, g_imag))
        with torch.cuda.device(mag.device):
            gsig = ctx.plan.run_backward((mag, real, imag), grads, iters)
        out, a = [], 0
        for like, need, n in zip(ctx.like, need_in, ctx.plan.t2.lossless.n_smpls):
            out.append(gsig[a:a + n].to(like[0]).reshape(like[1]) if like is not None and need else None)
            a += n
        return (None,) + tuple(out)


def analyze_compressed_type2(plan, sigs):
    """plan.run(want_iters=True) of a Type2CompressedAnalysisPlan, differentiable with respect to the v_sig in sigs that are
    tensors requiring grad.  Returns ((mag, real, imag) with grad_fn, gain)."""
    plan.check_grad_dims()           # what has no backward pass says so before the forward is launched
    mag, real, imag, gain, _iters = _Type2CompressedAnalysis.apply(plan, *sigs)
    return (mag, real, imag), gain


class _MLPG(torch.autograd.Function):
    """forward(engine, var, streams, windows, width, *means): means = the [F_i x width] mean matrices of mp.mlpg_batch /
    mp.mlpg_streams_batch (tensors or host arrays), var = the device variances ([width] or [sum F_i x width]), streams =
    [(first column, D), ...].  Engine.mlpg_streams is the forward launch (one mpx_mlpg_solve per stream).  Output: the ONE
    float64 [sum F_i x sum D] buffer of trajectories.  The backward pass keeps no factor: per stream it solves A z = g
    again from the variances (mpx_mlpg_solve with the right-hand side given) and applies P_k W_k (mpx_mlpg_apply).  Kept:
    the variances and the frame offsets -- MLPG is linear in the means, so the means themselves are not."""

    @staticmethod
    def forward(ctx, engine, var, streams, windows, width, *means):
        import numpy as np

        buf, offs = engine.mlpg_pack(list(means), width)
        offs_dev = engine.to_device(offs.astype(np.int32), np.int32)
        out = engine.mlpg_streams(buf, var, offs_dev, streams, windows)
        ctx.engine, ctx.streams, ctx.windows, ctx.width = engine, streams, windows, width
        ctx.offs = [int(o) for o in offs]
        ctx.like = [(m.dtype, tuple(m.shape)) if torch.is_tensor(m) else None for m in means]
        ctx.save_for_backward(var, offs_dev)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        var, offs_dev = ctx.saved_tensors
        n_head = 5   # engine, var, streams, windows, width
        need_in = ctx.needs_input_grad[n_head:]
        if grad_out.dtype != torch.float64 or grad_out.stride(1) != 1 or not grad_out.is_contiguous():
            grad_out = grad_out.to(torch.float64).contiguous()
        with torch.cuda.device(var.device):
            g = ctx.engine.mlpg_streams_backward(grad_out, var, offs_dev, ctx.streams, ctx.windows, ctx.width)
        out = []
        for like, need, a, b in zip(ctx.like, need_in, ctx.offs[:-1], ctx.offs[1:]):
            out.append(g[a:b].to(like[0]).reshape(like[1]) if like is not None and need else None)
        return (None,) * n_head + tuple(out)


def mlpg(engine, means, var, streams, windows, width):
    """Engine.mlpg_streams on the packed means, differentiable with respect to the mean matrices that are tensors
    requiring grad (the variances and the windows get no gradient).  -> the float64 [sum F_i x sum D] buffer with grad_fn."""
    return _MLPG.apply(engine, var, streams, windows, int(width), *means)


class _MagnitudeSynthesis(torch.autograd.Function):
    """forward(plan, b_out_hpf, n_utts, *mats): plan = a MagnitudeSynthesisPlan built from the utterances whose
    m_mag_mel_log are mats (tensors or host arrays; the plan holds them packed as float32 device rows already); plan.run()
    and Engine.output_hpf are the forward, plan.adjoint_hpf and plan.run_backward (k_synth_comp_bwd, k_min_phase_bwd,
    k_rows_lerp_adjoint, k_mel_unwarp_bwd: DESIGN.md section 3.3o) the backward.  Output: the ONE [total_out] waveform
    buffer (float64 after the high-pass, float32 without it); the per-utterance signals are views of it."""

    @staticmethod
    def forward(ctx, plan, b_out_hpf, n_utts, *mats):
        pcm = plan.run()
        if b_out_hpf:
            pcm = plan.engine.output_hpf(pcm, plan.out_off_host, plan.fs)
        ctx.plan, ctx.hpf = plan, bool(b_out_hpf)
        ctx.rows = [int(m.shape[0]) for m in mats]
        ctx.like = [(m.dtype, tuple(m.shape)) if torch.is_tensor(m) else None for m in mats]
        return pcm

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        plan = ctx.plan
        n_head = 3   # plan, b_out_hpf, n_utts
        need_in = ctx.needs_input_grad[n_head:]
        with torch.cuda.device(grad_out.device):
            g = plan.adjoint_hpf(grad_out) if ctx.hpf else grad_out.to(torch.float32)
            g = plan.run_backward(g.contiguous())
        out, a = [], 0
        for like, need, n in zip(ctx.like, need_in, ctx.rows):
            out.append(g[a:a + n].to(like[0]).reshape(like[1]) if like is not None and need else None)
            a += n
        return (None,) * n_head + tuple(out)


def synthesize_from_mag(plan, b_out_hpf, utts):
    """plan.run() of a MagnitudeSynthesisPlan (and the output high-pass), differentiable with respect to the
    m_mag_mel_log in utts = [(m_mag_mel_log, v_lf0)] that are tensors requiring grad.  Returns the [total_out] waveform
    buffer (with grad_fn)."""
    plan.check_differentiable()      # what has no backward pass says so before the forward is launched
    return _MagnitudeSynthesis.apply(plan, bool(b_out_hpf), len(utts), *[u[0] for u in utts])


class _MinPhase(torch.autograd.Function):
    """forward(engine, *mats): mats = the [F_i x H] magnitude matrices of la.build_min_phase_from_mag_spec_batch (tensors or
    host arrays); Engine.min_phase_rows (ONE mpx_min_phase launch over all rows) is the forward, mpx_min_phase_backward the
    backward.  Outputs: the unit phasor rows (cos phi, sin phi) of all matrices, float32 [sum F_i x H] views at the spectra's
    row pitch; the product with the magnitudes is the caller's (plain torch).  Kept for the backward pass: the three rows
    the forward wrote."""

    @staticmethod
    def forward(ctx, engine, *mats):
        o_m, o_r, o_i = engine.min_phase_rows(list(mats))
        ctx.engine = engine
        ctx.rows = [int(m.shape[0]) for m in mats]
        ctx.like = [(m.dtype, tuple(m.shape)) if torch.is_tensor(m) else None for m in mats]
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(o_m, o_r, o_i)
        return o_r, o_i

    @staticmethod
    @once_differentiable
    def backward(ctx, g_r, g_i):
        o_m, o_r, o_i = ctx.saved_tensors
        need_in = ctx.needs_input_grad[1:]
        with torch.cuda.device(o_m.device):
            g = ctx.engine.min_phase_backward(o_m, o_r, o_i, None, g_r, g_i)
        out, a = [], 0
        for like, need, n in zip(ctx.like, need_in, ctx.rows):
            out.append(g[a:a + n].to(like[0]).reshape(like[1]) if like is not None and need else None)
            a += n
        return (None,) + tuple(out)


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
        ctx.like = [(m.dtype, tuple(m.shape)) if torch.is_tensor(m) else None for m in mats]
        if pf_type == "merlin":
            ctx.save_for_backward(x)
        else:
            ctx.save_for_backward()
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        n_head = 4   # engine, pf_type, fs, opts
        need_in = ctx.needs_input_grad[n_head:]
        with torch.cuda.device(grad_out.device):
            if ctx.pf_type == "merlin":
                (x,) = ctx.saved_tensors
                g = ctx.engine.post_filter_merlin_backward(x, grad_out, ctx.fs, **ctx.kw)
            else:
                ctx.saved_tensors   # (none kept; raises as torch does when the graph was freed)
                g = ctx.engine.post_filter_backward(grad_out, ctx.fs, **ctx.kw)
        out = []
        for like, need, a, b in zip(ctx.like, need_in, ctx.offs[:-1], ctx.offs[1:]):
            out.append(g[a:b].to(like[0]).reshape(like[1]) if like is not None and need else None)
        return (None,) * n_head + tuple(out)


def post_filter(engine, mats, pf_type, fs, opts):
    """Engine.post_filter / Engine.post_filter_merlin on the packed rows of mats, differentiable with respect to the matrices
    that are tensors requiring grad.  Returns (the float32 [sum F_i x D] buffer with grad_fn, the row offsets)."""
    import numpy as np

    out = _PostFilter.apply(engine, pf_type, fs, tuple(sorted(opts.items())), *mats)
    offs = np.concatenate(([0], np.cumsum([int(m.shape[0]) for m in mats]))).astype(np.int64)
    return out, offs
