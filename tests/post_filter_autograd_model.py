"""
References of the post-filter backward tests (tests/test_post_filter_autograd_host.py on the CPU,
tests/test_gpu_post_filter_autograd.py on the device).  numpy / torch float64: no GPU.

  pf_matrix            the MagPhase post-filter as the matrix M it is per frame (y = x M^T), restated from
                       hostmath.post_filter_tables' output: M = diag(tilt) (I - A) + A, A the clamped moving average, the
                       two end rows identity rows.  Its backward is g M
  pf_forward_torch     mp.post_filter restated as a float64 torch graph (autograd is the authority for g M)
  merlin_forward_torch mpx_post_filter_merlin launch by launch (output_stage_model.merlin_stages without the float32
                       pipe boundaries) as a float64 torch graph
  merlin_closed_form   the closed form of its gradient that mpx_post_filter_merlin_backward computes:
                       g_pf = g Cf^T, g_d = g_pf[0], Q(v) = S(v) / R(v),
                       g_c = lifter * (g_pf - g_d Q(cw)) + g_d Q(c), g_x = g_c C1^T
"""
import warnings

import numpy as np


def pf_tables(dim, fs, **opts):
    """hostmath.post_filter_tables without its warnings -> (nx0, nx1, half int64[], tilt float64[dim])."""
    from magphase_amd import hostmath as hm
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return hm.post_filter_tables(dim, fs, **opts)


def pf_matrix(dim, nx0, nx1, half, tilt):
    """M [dim x dim] float64, row = output bin, column = input bin."""
    m = np.zeros((dim, dim))
    for b in range(dim):
        if b == 0 or b == dim - 1:
            m[b, b] = 1.0
            continue
        c = min(max(b, nx0), nx1)
        h = int(half[c - nx0])
        assert h >= 0 and c - h >= 0 and c + h < dim
        a = np.zeros(dim)
        a[c - h:c + h + 1] = 1.0 / (2 * h + 1)
        e = np.zeros(dim)
        e[b] = 1.0
        m[b] = tilt[b] * (e - a) + a
    return m


def pf_fan_in(m):
    """Non-zero entries per column of M."""
    return (m != 0).sum(axis=0)


def pf_forward_torch(x, nx0, nx1, half, tilt):
    """mp.post_filter's operations on a float64 torch [F x D] matrix, from the tables."""
    import torch
    dim = x.shape[1]
    cols = []
    for j in range(nx0, nx1 + 1):
        h = int(half[j - nx0])
        cols.append(x[:, j - h:j + h + 1].mean(dim=1))
    ave = [cols[min(max(b, nx0), nx1) - nx0] for b in range(dim)]
    ave = torch.stack(ave, dim=1)
    enh = (x - ave) * torch.as_tensor(tilt, dtype=torch.float64)[None, :] + ave
    return torch.cat((x[:, :1], enh[:, 1:-1], x[:, -1:]), dim=1)


def _tab(tables):
    return tuple(np.asarray(tables[k], dtype=np.float64) for k in ("c1", "lifter", "g", "wk", "cf"))


def merlin_forward_torch(x, tables):
    """x: float64 torch [F x D] -> out [F x D], the device's launch sequence in float64 (NaN -> MAGIC left out: the
    reference rows are finite)."""
    import torch
    c1, lifter, g, wk, cf = (torch.as_tensor(a) for a in _tab(tables))
    alpha = float(tables["alpha"])
    c = x @ c1
    cw = c * lifter
    r0 = torch.exp(2.0 * (c @ g)) @ wk
    p = torch.exp(2.0 * (cw @ g)) @ wk
    dim = x.shape[1]
    b = [None] * dim
    b[dim - 1] = cw[:, dim - 1]
    for m in range(dim - 2, -1, -1):
        b[m] = cw[:, m] - alpha * b[m + 1]
    b[0] = b[0] + 0.5 * torch.log(r0 / p)
    pf = [b[m] + alpha * b[m + 1] for m in range(dim - 1)] + [b[dim - 1]]
    return torch.stack(pf, dim=1) @ cf


def merlin_energy(x, tables):
    """(r0, p_r0) float64 of the rows x."""
    c1, lifter, g, wk, _cf = _tab(tables)
    c = np.asarray(x, dtype=np.float64) @ c1
    with np.errstate(all="ignore"):
        return np.exp(2.0 * (c @ g)) @ wk, np.exp(2.0 * ((c * lifter) @ g)) @ wk


def merlin_closed_form(x, g_out, tables):
    """The gradient with respect to x of sum(out * g_out), float64 [F x D]."""
    c1, lifter, g, wk, cf = _tab(tables)
    x, g_out = np.asarray(x, dtype=np.float64), np.asarray(g_out, dtype=np.float64)
    c = x @ c1
    cw = c * lifter
    g_pf = g_out @ cf.T
    g_d = g_pf[:, :1]

    def q(v):
        e = np.exp(2.0 * (v @ g)) * wk        # [F x bins]
        return (e @ g.T) / e.sum(axis=1, keepdims=True)

    g_cw = g_pf - g_d * q(cw)
    g_c = lifter * g_cw + g_d * q(c)
    return g_c @ c1.T
