"""
fp64 model of griffin_lim (reference magphase.py:3320-3372) composed from oracle.magphase_oracle primitives: the yardstick
of the Griffin-Lim tests (pinned to the reference by tests/golden/g13_griffin_lim.npz).
"""
import numpy as np

from oracle import magphase_oracle as orc


def initial_phase(m_mag, phase_init):
    """magphase.py:3334-3352 (Hermitian extension included): the [F x N] phase of the first synthesis.  An ndarray init
    has its columns 0 and H - 1 zeroed in place, as la.add_hermitian_half does."""
    F, H = m_mag.shape
    N = 2 * (H - 1)
    if isinstance(phase_init, str):
        if phase_init == "random":
            return 2 * np.pi * (np.random.rand(F, N) - 0.5)
        if phase_init == "linear":
            z = np.zeros((F, N))
            z[:, N // 2] = 1.0
            return np.angle(np.fft.fft(z))
        assert phase_init == "min_phase"
        ph = np.angle(orc.build_min_phase_from_mag_spec(m_mag))
    else:
        ph = phase_init
    ph[:, 0] = 0
    ph[:, -1] = 0
    return np.hstack((ph, -ph[:, -2:0:-1]))


def griffin_lim(m_mag, v_shift, phase_init="random", niters=30):
    m_mag = np.asarray(m_mag, dtype=np.float64)
    v_shift = orc.round_to_int(v_shift)
    F, H = m_mag.shape
    N = 2 * (H - 1)
    m_phase = initial_phase(m_mag, phase_init)
    m_full = orc.add_hermitian_half_real(m_mag)
    v_pm = np.cumsum(v_shift)
    for i in range(niters):
        v_sig = orc.ola(np.fft.ifft(m_full * np.exp(1j * m_phase)).real, v_pm)
        if i == niters - 1:
            break
        frames = orc.windowing(v_sig, v_pm)[0]
        m_phase = np.angle(np.fft.fft(orc.frm_list_to_matrix(frames, v_shift, N)))
    return v_sig, m_phase[:, :H]


def spectral_convergence(v_sig, m_mag, v_shift):
    """||M - |STFT(v_sig)||| / ||M|| with the analysis of the iterations (windowing + frm_list_to_matrix + FFT)."""
    m_mag = np.asarray(m_mag, dtype=np.float64)
    H = m_mag.shape[1]
    N = 2 * (H - 1)
    v_shift = orc.round_to_int(v_shift)
    frames = orc.windowing(v_sig, np.cumsum(v_shift))[0]
    X = np.abs(np.fft.fft(orc.frm_list_to_matrix(frames, v_shift, N))[:, :H])
    return np.linalg.norm(m_mag - X) / np.linalg.norm(m_mag)
