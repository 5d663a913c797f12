"""
Float64 numpy restatement of synthesis_from_compressed_type2 (magphase.py:1452-1606) for the CPU and GPU tests, in this
project's own words.  It takes the noise vector as an argument (None: drawn from numpy's global generator exactly where
the reference draws it) and returns the signal together with what the tests compare: the frame tables, rms_noise computed
from the noise spectra AND by the transform-free identity, the per-bin curves and the pre-filter signal.

The generic pieces (pitch-synchronous windows, frame placement, cosine-matrix unwarp, constant -> variable rate scan and
interpolation, centred anti-ringing window, overlap-add) are the numpy oracle's; what is specific to type 2 is spelled
out here: the phase coefficients' extension to mag_dim columns, one rms gain over all frames and bins, the plain Hann
crossfade, the hf_slope line, signed real DC / Nyquist bins, the elliptic high-pass.
"""
import os

import numpy as np
from scipy import signal

from oracle import magphase_oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RATE_CASE = {-1.0: 0, 5.0: 2, 4.0: 4}   # const_rate_ms -> g16's compressed case without b_norm_mag


def golden():
    """(g17: the reference's type-2 synthesis outputs, g16: the type-2 analysis golden its inputs are rows of)."""
    return np.load(os.path.join(GOLDEN, "g17_type2_synthesis.npz")), np.load(os.path.join(GOLDEN, "g16_type2.npz"))


def case_inputs(g17, g16, i):
    """(name, (mag, real, imag, lf0), fs, keyword arguments, seed) of golden case i."""
    name, utt, rate = str(g17["names"][i]), str(g17["utts"][i]), float(g17["rates"][i])
    key = "%s_c%d" % (utt, RATE_CASE[rate])
    feats = tuple(np.asarray(g16[key + "_" + n], dtype=np.float64) for n in ("mag", "real", "imag", "lf0"))
    n = int(g17[name + "_fft_len"])
    kw = dict(hf_slope_coeff=float(g17[name + "_hf_slope"]), b_voi_ap_win=bool(g17[name + "_voi_ap_win"]),
              const_rate_ms=rate, fft_len=n if n else None)
    return name, feats, int(g16[utt + "_fs"]), kw, int(g17["seeds"][i])


def n_cases(g17):
    return len(g17["names"])


def crossfade_windows(half, fs):
    """la.spectral_crossfade's two long windows (libaudio.py:165-179): (falling / low-pass, rising / high-pass)."""
    cf, bw = orc.define_crossfade_params(fs)
    nfft = (half - 1) * 2
    bin_l = int(orc.round_to_int((cf - bw / 2.0) * nfft / float(fs)))
    bin_r = int(orc.round_to_int((cf + bw / 2.0) * nfft / float(fs)))
    n = bin_r - bin_l
    w = np.hanning(2 * n + 1)
    win_l = np.hstack((np.ones(bin_l), w[n:], np.zeros(half - bin_r - 1)))
    win_r = np.hstack((np.zeros(bin_l), w[:n + 1], np.ones(half - bin_r - 1)))
    return win_l, win_r


def bin_curves(fs, fft_len, hf_slope_coeff=1.0):
    """(per_v, ap_v, ap_u): what multiplies the periodic / aperiodic magnitudes of voiced frames and the aperiodic
    magnitude of unvoiced frames (magphase.py:1544-1553)."""
    half = fft_len // 2 + 1
    win_l, win_r = crossfade_windows(half, fs)
    return win_l, win_r, np.linspace(1, hf_slope_coeff, num=half)


def extend_phase_coeffs(m, mag_dim):
    """interp1d(arange(n), m, kind='nearest', fill_value='extrapolate')(arange(mag_dim)) (magphase.py:1494-1498):
    column j for j < n, the last column beyond."""
    return m[:, np.minimum(np.arange(mag_dim), m.shape[1] - 1)]


def phase_unwarp(m_real_mel, m_imag_mel, mag_dim, half, alpha):
    return (orc.sp_mel_unwarp(extend_phase_coeffs(m_real_mel, mag_dim), half, alpha=alpha, in_type="log"),
            orc.sp_mel_unwarp(extend_phase_coeffs(m_imag_mel, mag_dim), half, alpha=alpha, in_type="log"))


def phase_unwarp_matrix(phase_dim, mag_dim, half, alpha):
    """The extension followed by the unwarp as one [phase_dim x half] matrix: unit coefficient vectors pushed through."""
    eye = np.eye(phase_dim)
    return orc.sp_mel_unwarp(extend_phase_coeffs(eye, mag_dim), half, alpha=alpha, in_type="log")


def frame_tables(v_lf0, fs, const_rate_ms):
    """(v_shift int, v_pm, v_voi, rows (lo, hi, t) or None, ns_len): magphase.py:1504-1519, :1524."""
    v_f0 = np.exp(np.asarray(v_lf0, dtype=np.float64))
    v_shift = orc.f0_to_shift(v_f0, fs)
    v_locs = None
    if const_rate_ms > 0.0:
        v_shift, v_locs = orc.get_shifts_and_frm_locs_from_const_shifts(v_shift, const_rate_ms, fs)
        v_voi = orc.interp_from_const_to_variable_rate(v_f0 > 0.0, v_locs, const_rate_ms, fs) > 0.5
        v_f0 = v_voi * fs / v_shift.astype("float64")
    v_shift = v_shift.astype(int)
    v_pm = np.cumsum(v_shift)
    ns_len = int(v_pm[-1] + (v_pm[-1] - v_pm[-2]))
    return v_shift, v_pm, v_f0 > 1, v_locs, ns_len


def noise_frames(v_noise, v_pm, v_voi, b_voi_ap_win):
    wins = [orc.voi_noise_window if (b_voi_ap_win and v) else np.hanning for v in v_voi]
    return orc.windowing(v_noise, v_pm, win_func=wins)[0]


def rms_from_frames(frames, fft_len):
    """rms_noise without a transform: for a real frame x padded to N, sum_{k=0}^{N/2} |X_k|^2 =
    (N sum x^2 + (sum x)^2 + (sum (-1)^n x[n])^2) / 2; the frame's position only changes the alternating sum's sign."""
    tot = 0.0
    for x in frames:
        x = np.asarray(x, dtype=np.float64)[:fft_len]
        alt = np.sum(x[0::2]) - np.sum(x[1::2])
        tot += 0.5 * (fft_len * np.sum(x * x) + np.sum(x) ** 2 + alt ** 2)
    return float(np.sqrt(tot / (len(frames) * (fft_len // 2 + 1))))


def output_filter(v_sig, fs):
    """magphase.py:1599-1604."""
    b, a = signal.ellip(4, 0.5, 80, 60 / (fs / 2.0), btype="highpass")
    return signal.lfilter(b, a, v_sig)


def synthesis(m_mag_mel_log, m_real_mel, m_imag_mel, v_lf0, fs, fft_len=None, hf_slope_coeff=1.0, b_voi_ap_win=True,
              const_rate_ms=-1.0, v_noise=None):
    """Returns (signal, debug dict)."""
    alpha = orc.define_alpha(fs)
    if fft_len is None:
        fft_len = orc.define_fft_len(fs)
    half = fft_len // 2 + 1
    m_mag_mel_log = np.asarray(m_mag_mel_log, dtype=np.float64)
    m_real_mel = np.asarray(m_real_mel, dtype=np.float64)
    m_imag_mel = np.asarray(m_imag_mel, dtype=np.float64)
    mag_dim = m_mag_mel_log.shape[1]

    m_mag = np.exp(orc.sp_mel_unwarp(m_mag_mel_log, half, alpha=alpha, in_type="log"))
    m_real, m_imag = phase_unwarp(m_real_mel, m_imag_mel, mag_dim, half, alpha)

    v_shift, v_pm, v_voi, v_locs, ns_len = frame_tables(v_lf0, fs, const_rate_ms)
    if v_locs is not None:
        m_mag = orc.interp_from_const_to_variable_rate(m_mag, v_locs, const_rate_ms, fs)
        m_real = orc.interp_from_const_to_variable_rate(m_real, v_locs, const_rate_ms, fs)
        m_imag = orc.interp_from_const_to_variable_rate(m_imag, v_locs, const_rate_ms, fs)
    nfrms = v_shift.size

    if v_noise is None:
        v_noise = np.random.uniform(-1, 1, ns_len)
    v_noise = np.asarray(v_noise, dtype=np.float64)
    assert v_noise.size == ns_len
    frames = noise_frames(v_noise, v_pm, v_voi, b_voi_ap_win)
    m_ns = orc.frm_list_to_matrix(frames, v_shift, fft_len)
    m_ns_spec = np.fft.fft(np.fft.fftshift(m_ns, axes=1))[:, :half]
    rms_spec = float(np.sqrt(np.mean(np.absolute(m_ns_spec) ** 2)))
    rms_ident = rms_from_frames(frames, fft_len)

    per_v, ap_v, ap_u = bin_curves(fs, fft_len, hf_slope_coeff)
    m_ap_mag = m_mag / rms_spec
    m_ap_mag[v_voi] = m_ap_mag[v_voi] * ap_v
    m_ap_mag[~v_voi] = m_ap_mag[~v_voi] * ap_u
    m_per_mag = np.zeros(m_mag.shape)
    m_per_mag[v_voi] = m_mag[v_voi] * per_v

    ph = m_real + 1j * m_imag
    ph_abs = np.absolute(ph)
    ph_abs[ph_abs == 0.0] = 1.0
    m_syn = m_ap_mag * m_ns_spec + m_per_mag * ph / ph_abs
    # la.add_hermitian_half(.., 'complex'): DC and Nyquist keep the signed real part, their imaginary part is dropped
    m_frms = np.fft.fftshift(np.fft.ifft(orc.hermitian_full_spectrum(m_syn)).real, axes=1)

    se = np.r_[v_shift[0], v_shift, v_shift[-1], v_shift[-1]]
    for n in range(nfrms):
        m_frms[n] *= orc.centred_window(se[n] + se[n + 1], se[n + 2] + se[n + 3], fft_len, orc.raised_hanning, True)
    v_pre = orc.ola(m_frms, v_pm)
    dbg = dict(v_shift=v_shift, v_pm=v_pm, v_voi=v_voi, v_locs=v_locs, ns_len=ns_len, rms_spec=rms_spec,
               rms_ident=rms_ident, v_pre_hpf=v_pre, nfrms=nfrms)
    return output_filter(v_pre, fs), dbg
