"""
Autograd for the lossless synthesis: a torch.autograd.Function around the unchanged forward
launch of synthesis_from_lossless_batch / synthesis_from_lossless_const_rate_batch, with the gradients with respect to
m_mag / m_real / m_imag computed by k_synth_lossless_bwd (and k_rows_lerp_adjoint for constant-rate rows).  Imported
lazily by magphase.py, and only when a device tensor that requires grad goes in with return_device=True and grad mode on.

Not differentiable: v_f0 (the pitch marks are integers) and fs.  No double backward.  The compressed and type-2
synthesis and the analysis direction have no backward pass.
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
