"""
float64 numpy model of la.true_envelope (libaudio.py:295-340) and la.spectral_smoothing_rceps (:203-238), vectorised
over frames, in the formulation of the device kernel: one cepstral weight per index (hostmath.true_envelope_lifter),
the mean-abs stop rule, the max update.  forced (optional, int per frame): run exactly that many passes, no stop test.
"""
import numpy as np

from magphase_amd import hostmath as hm

_TO_DB = {"abs": lambda x: 20.0 * np.log10(x), "db": lambda x: x, "log": lambda x: (20.0 / np.log(10.0)) * x}
_FROM_DB = {"abs": lambda v: 10.0 ** (v / 20.0), "db": lambda v: v, "log": lambda v: (np.log(10.0) / 20.0) * v}


def smooth(m_sp_log, w):
    """la.spectral_smoothing_rceps of [F x H] rows with the weight table w [N]."""
    m = np.asarray(m_sp_log, dtype=np.float64)
    N = 2 * (m.shape[1] - 1)
    c = np.fft.ifft(np.hstack((m, m[:, -2:0:-1]))).real
    return np.fft.fft(c * w, n=N).real[:, :m.shape[1]]


def true_envelope(m_sp, in_type="abs", ncoeffs=60, thres_db=0.1, forced=None, max_iters=hm.TRUE_ENV_MAX_ITERS):
    """-> (envelope [F x H] float64, passes per frame int32)."""
    m_sp = np.atleast_2d(np.asarray(m_sp, dtype=np.float64))
    F, H = m_sp.shape
    w = hm.true_envelope_lifter(2 * (H - 1), ncoeffs, 0.7)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = _TO_DB[in_type](m_sp).copy()
        sm = np.zeros_like(v)
        iters = np.zeros(F, dtype=np.int32)
        idx = np.arange(F)
        for i in range(max_iters):
            if idx.size == 0:
                break
            s = smooth(v[idx], w)
            sm[idx] = s
            iters[idx] = i + 1
            if forced is not None:
                stop = np.asarray(forced)[idx] <= i + 1
            else:
                stop = np.mean(np.abs(v[idx] - s), axis=1) < thres_db
            go = idx[~stop]
            v[go] = np.maximum(v[go], s[~stop])
            idx = go
        return _FROM_DB[in_type](sm), iters
