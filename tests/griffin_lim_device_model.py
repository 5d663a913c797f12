"""
fp64 model of the device fold of Griffin-Lim's first synthesis (k_gl_fold, mpx_griffin_lim_fold)
and of griffin_lim_from_mag_batch, composed from numpy and oracle.magphase_oracle primitives: the yardstick of
tests/test_griffin_lim_device_host.py and tests/test_gpu_griffin_lim_device.py.
"""
import numpy as np

import griffin_lim_model as glm
from oracle import magphase_oracle as orc

HALF, FULL, WORDS = 0, 1, 2   # MPX_GL_FOLD_HALF / _FULL / _WORDS


def words_to_rand(words):
    """numpy's random_sample from raw MT19937 words, two per sample (randomkit's rk_double): uint32 [..., 2 n] ->
    float64 [..., n].  Every step is exact in float64."""
    w = np.asarray(words, dtype=np.uint32)
    a = (w[..., 0::2] >> np.uint32(5)).astype(np.float64)
    b = (w[..., 1::2] >> np.uint32(6)).astype(np.float64)
    return (a * 67108864.0 + b) / 9007199254740992.0


def words_to_phase(words, F, N):
    """The 'random' initial phase 2 pi (rand(F, N) - 0.5) (magphase.py:3335) from the words of that draw."""
    return 2 * np.pi * (words_to_rand(np.asarray(words).reshape(F, 2 * N)) - 0.5)


def fold(m_mag, phase, form):
    """(mag', phasor real, phasor imag, phi_k for k < H, |c|) in float64 for target rows m_mag [F x H] and the phase in one
    of the kernel's three forms: HALF [F x H] (columns 0 and H - 1 count as 0), FULL [F x N], WORDS uint32 [F * 2 N].
    The inputs are taken as they are (the tests round them to float32 first: the kernel widens float32 exactly)."""
    m = np.asarray(m_mag, dtype=np.float64)
    F, H = m.shape
    N = 2 * (H - 1)
    sgn = np.where(np.arange(H) % 2 == 0, 1.0, -1.0)
    if form == HALF:
        ph = np.array(phase, dtype=np.float64)
        ph[:, 0] = 0.0
        ph[:, -1] = 0.0
        return m.copy(), np.cos(ph) * sgn, np.sin(ph) * sgn, ph, np.ones_like(m)
    ph = words_to_phase(phase, F, N) if form == WORDS else np.asarray(phase, dtype=np.float64)
    assert ph.shape == (F, N)
    mir = ph[:, (N - np.arange(H)) % N]
    cr = 0.5 * (np.cos(ph[:, :H]) + np.cos(mir))
    ci = 0.5 * (np.sin(ph[:, :H]) - np.sin(mir))
    a = np.hypot(cr, ci)
    nz = a > 0
    inv = np.where(nz, 1.0 / np.where(nz, a, 1.0), 0.0)
    return m * a, cr * inv * sgn, ci * inv * sgn, ph[:, :H].copy(), a


def ulp32(x):
    """One float32 unit in the last place at float32(x) (the spacing towards larger magnitudes)."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


def from_mag(m_mag_mel_log, v_lf0, fs, fft_len, phase_init, niters, b_const_rate=False, b_fbank_mel=False):
    """griffin_lim_from_mag in float64: exp of the oracle's mel unwarp, the oracle's shifts and constant -> variable rate
    row interpolation (synthesis_from_compressed, magphase.py:846-870, :879), then the Griffin-Lim model.
    Returns (v_sig, m_mag [frames x H], v_shift int)."""
    alpha = orc.define_alpha(fs)
    half = fft_len // 2 + 1
    v_shift = orc.f0_to_shift(np.exp(np.asarray(v_lf0, dtype=np.float64)), fs)
    x = np.asarray(m_mag_mel_log, dtype=np.float64)
    if b_fbank_mel:
        m_mag = np.exp(orc.sp_mel_unwarp_fbank(x, half, alpha=alpha))
    else:
        m_mag = np.exp(orc.sp_mel_unwarp(x, half, alpha=alpha, in_type="log"))
    if b_const_rate:
        v_shift, v_locs = orc.get_shifts_and_frm_locs_from_const_shifts(v_shift, 5.0, fs)
        m_mag = orc.interp_from_const_to_variable_rate(m_mag, v_locs, 5.0, fs)
    v_shift = v_shift.astype(int)
    v_sig, _ = glm.griffin_lim(m_mag, v_shift, phase_init, niters)
    return v_sig, m_mag, v_shift
