"""The scaffold every autograd path shares (magphase_amd/autograd.py: _like, _coerce, _scatter) and the one rule that sends
a call into a torch.autograd.Function (hostmath.wants_grad), on CPU tensors: no device."""
import numpy as np
import pytest
import torch

from magphase_amd import autograd as ag
from magphase_amd import hostmath as hm

OFFS = [0, 2, 2, 5]      # three inputs of 2, 0 and 3 rows
WIDTH = 4


def _inputs():
    return [torch.zeros(2, WIDTH, dtype=torch.float64, requires_grad=True), np.zeros((0, WIDTH)),
            torch.zeros(3, WIDTH, dtype=torch.float16)]


def _batch(seed=0):
    return torch.from_numpy(np.random.RandomState(seed).randn(5, WIDTH).astype(np.float32))


def _same(t, dtype, ref):
    return torch.is_tensor(t) and t.dtype == dtype and t.shape == ref.shape and torch.equal(t, ref.to(dtype))


def test_like_describes_tensors_and_leaves_host_arrays_out():
    assert ag._like(_inputs()) == [(torch.float64, (2, WIDTH)), None, (torch.float16, (3, WIDTH))]
    assert ag._like([]) == []


def test_offsets():
    assert ag._offsets([2, 0, 3]) == OFFS and ag._offsets([]) == [0]


def test_scatter_one_batch_gradient():
    like, g = ag._like(_inputs()), _batch()
    out = ag._scatter(g, OFFS, like, (True, True, False))     # (a host array "needing" a gradient still gets None)
    assert isinstance(out, tuple) and len(out) == 3
    assert _same(out[0], torch.float64, g[0:2]) and out[1] is None and out[2] is None
    out = ag._scatter(g, OFFS, like, (True, False, True))
    assert _same(out[0], torch.float64, g[0:2]) and out[1] is None and _same(out[2], torch.float16, g[2:5])
    assert ag._scatter(g, OFFS, like, (False, False, False)) == (None, None, None)


@pytest.mark.parametrize("need", [(True, False, False), (False, True, True)])
def test_scatter_three_streams_per_utterance(need):
    """Utterance-major inputs (mag_0, real_0, imag_0, mag_1, ...); a stream nobody needs arrives as None and is not read."""
    mats = []
    for n in (2, 0, 3):                           # utterance u: rows OFFS[u]:OFFS[u + 1] of every stream's gradient
        mats += [torch.zeros(n, WIDTH, dtype=torch.float64), np.zeros((n, WIDTH)), torch.zeros(n, WIDTH, dtype=torch.float16)]
    like = ag._like(mats)
    g = tuple(_batch(seed=k) if need[k] else None for k in range(3))
    need_in = tuple(need[i % 3] for i in range(9))
    out = ag._scatter(g, OFFS, like, need_in)
    assert len(out) == 9
    for i, o in enumerate(out):
        u, k = divmod(i, 3)
        if k == 1 or not need[k]:                  # the host array, or a stream that needs no gradient
            assert o is None
        else:
            assert _same(o, torch.float64 if k == 0 else torch.float16, g[k][OFFS[u]:OFFS[u + 1]])
    # one utterance alone needing a gradient: every other input gets None
    only = tuple(i == 6 and need[0] for i in range(9))
    out = ag._scatter(g, OFFS, like, only)
    assert [o is not None for o in out] == list(only)


def test_scatter_gives_a_vector_input_its_own_shape():
    """The analyses pass 1-D v_sig: the [total_smpls] gradient comes back per utterance, 1-D, in the input's dtype."""
    sigs = [torch.zeros(2, dtype=torch.float64), np.zeros(0), torch.zeros(3, dtype=torch.bfloat16)]
    g = torch.arange(5, dtype=torch.float32)
    out = ag._scatter(g, OFFS, ag._like(sigs), (True, True, True))
    assert _same(out[0], torch.float64, g[0:2]) and out[0].shape == (2,)
    assert out[1] is None
    assert _same(out[2], torch.bfloat16, g[2:5]) and out[2].shape == (3,)
    # a [rows x 1] input gets [rows x 1] back from a [total] gradient
    out = ag._scatter(g, [0, 5], ag._like([torch.zeros(5, 1)]), (True,))
    assert out[0].shape == (5, 1) and torch.equal(out[0][:, 0], g)


def test_coerce():
    g = _batch()
    assert ag._coerce(None) is None and ag._coerce(None, unit_cols=True) is None
    assert ag._coerce(g) is g and ag._coerce(g, unit_cols=True) is g
    for unit_cols in (False, True):
        c = ag._coerce(g.double(), unit_cols=unit_cols)
        assert c.dtype == torch.float32 and c.is_contiguous() and torch.equal(c, g)
    view = torch.cat((g, g), dim=1)[:, 1:1 + WIDTH]            # a column slice: unit column stride, not contiguous
    assert view.stride(1) == 1 and not view.is_contiguous()
    assert ag._coerce(view, unit_cols=True) is view
    c = ag._coerce(view)
    assert c is not view and c.is_contiguous() and c.dtype == torch.float32 and torch.equal(c, view)
    t = g.t()                                                    # neither
    for unit_cols in (False, True):
        c = ag._coerce(t, unit_cols=unit_cols)
        assert c is not t and c.is_contiguous() and torch.equal(c, t)
    d = g.double()                                               # another dtype asked for (MLPG's float64)
    assert ag._coerce(d, dtype=torch.float64) is d
    assert ag._coerce(g, dtype=torch.float64).dtype == torch.float64
    v = torch.arange(5, dtype=torch.float32)                     # 1-D (a waveform gradient): the contiguous rule
    assert ag._coerce(v) is v and ag._coerce(v[::2]).is_contiguous()


def test_the_gate():
    dev = torch.zeros(2, 3, device="meta", requires_grad=True)        # stands for a device tensor
    dev_plain = torch.zeros(2, 3, device="meta")
    cpu = torch.zeros(2, 3, requires_grad=True)
    host = np.zeros((2, 3))
    assert hm.wants_grad(True, [host, dev_plain, dev]) is True
    assert hm.wants_grad(1, [dev]) is True
    assert hm.wants_grad(False, [host, dev]) is False
    with torch.no_grad():
        assert hm.wants_grad(True, [dev]) is False
    assert hm.wants_grad(True, [dev]) is True
    assert hm.wants_grad(True, [cpu]) is False                        # a CPU tensor is a host array to every path
    assert hm.wants_grad(True, [dev_plain]) is False
    assert hm.wants_grad(True, [host, host]) is False
    assert hm.wants_grad(True, []) is False
    # la.true_envelope_batch alone lets a CPU tensor that requires grad in; nothing else changes with that
    assert hm.wants_grad(True, [cpu], cpu_too=True) is True
    assert hm.wants_grad(False, [cpu], cpu_too=True) is False
    assert hm.wants_grad(True, [cpu.detach(), host], cpu_too=True) is False
    with torch.no_grad():
        assert hm.wants_grad(True, [cpu], cpu_too=True) is False
