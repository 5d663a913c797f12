"""
Drop-in counterpart of the reference's vocoder API (src/magphase.py) for the analysis/synthesis hot path.

Same function names, positional order, defaults and return arity as the reference
(SURVEY.md section 8b); numpy float64 arrays in and out, float32 feature files on disk.  The per-frame
arithmetic runs in hand-written gfx950 kernels (libmagphase_hip.so via ctypes); the float64
epoch/index arithmetic stays on the host (hostmath.py).  There is no CPU fallback.

Epochs: the reference shells out to the REAPER binary (magphase.py:2875-2876).  REAPER is outside the hot path
(SURVEY.md section 8f #1); epochs come, in this order, from a provider set with ``set_epoch_provider``,
from ``<wav stem>.est`` next to the wav (REAPER text format), from the built-in tracker if MAGPHASE_EPOCHS=builtin
is set (explicit opt-in: it is not REAPER), or from a REAPER binary if one is installed; otherwise RuntimeError.
"""
import os
import warnings

import numpy as np

from . import hostmath as hm
from . import libaudio as la
from . import libutils as lu
from .engine import get_engine
from .hostmath import check_const_rate_ms
from .hostplan import plan_const_rate_synthesis
from .plans import (CompressedAnalysisPlan, CompressedSynthesisPlan, GriffinLimPlan, LosslessAnalysisPlan,
                    LosslessConstRateAnalysisPlan, LosslessConstRateSynthesisPlan, LosslessRoundTripPlan,
                    LosslessSynthesisPlan, MagnitudeSynthesisPlan, Type2AnalysisPlan, Type2CompressedAnalysisPlan, Type2SynthesisPlan,
                    check_type2_grad_dims)

_epoch_provider = None

_WARN_LONG = ("fft_len (%d) is shorter than the current detected frame length (%d). "
              "This issue is not very critical, but if it occurs often "
              "(e.g., more than 3 times per utterance), please increase de FFT length.")

_SYN_NAMES = ("m_mag_mel_log", "m_real_mel", "m_imag_mel", "v_lf0")
_LOSSLESS_NAMES = ("m_mag", "m_real", "m_imag")


def _tensor_inputs(utts, names, lf0_at=None):
    """
    torch tensors among the feature arguments of a batch (names: the tuple positions that may hold one).  Checked without
    a device: float32 / float16 / bfloat16 / float64 only, 2-D (the lf0 vector at position lf0_at: 1-D, not float16) --
    ValueError naming the argument otherwise.  CPU tensors become host arrays (float16 / bfloat16 widened to float32:
    exact) and take the host path.  Returns (utts, True when a tensor of another device remains): a batch without
    tensors comes back as it is.
    """
    import sys

    torch = sys.modules.get("torch")
    if torch is None or not any(issubclass(t, torch.Tensor) for t in {type(x) for u in utts for x in u}):
        return utts, False
    out, on_dev = [], False
    for i, u in enumerate(utts):
        u = list(u)
        for k, name in enumerate(names[:len(u)]):
            x = u[k]
            if not torch.is_tensor(x):
                continue
            hm.check_feature_tensor(x, "utts[%d]: %s" % (i, name), lf0=(k == lf0_at))
            if x.device.type == "cpu":
                x = x.detach()
                u[k] = (x.float() if x.element_size() == 2 else x).numpy()
            else:
                on_dev = True
        out.append(tuple(u))
    return out, on_dev


def set_epoch_provider(fn):
    """fn(wav_file) -> (v_pm_sec, v_voi) or None.  Replaces the REAPER call of magphase.py:2875-2876."""
    global _epoch_provider
    _epoch_provider = fn


def use_builtin_epoch_tracker(device=None):
    """Installs magphase_amd.epochs.track_epochs as the epoch provider (instead of <wav>.est files / REAPER).
    The device is resolved HERE, in the caller's thread: torch's "current device" is thread-local and iobatch calls the
    provider from its reader thread, where it is device 0 on every rank."""
    from . import epochs

    dev = device if device is not None else get_engine().device

    def provider(wav_file):
        v_sig, fs = la.read_audio_file(wav_file)
        return epochs.track_epochs(v_sig, fs, device=dev)

    set_epoch_provider(provider)


def _epochs_for(wav_file, device=None):
    """device: the engine's device for the built-in tracker (MAGPHASE_EPOCHS=builtin); callers that run this in a worker
    thread pass it (see use_builtin_epoch_tracker), None = this thread's current device."""
    if _epoch_provider is not None:
        r = _epoch_provider(wav_file)
        if r is not None:
            return np.asarray(r[0], dtype=np.float64), np.asarray(r[1], dtype=np.float64)
    est = os.path.splitext(wav_file)[0] + ".est"
    if os.path.isfile(est):
        return la.read_est_fast(est)      # == np.loadtxt(est, skiprows=7, usecols=[0, 1]) columns, 5x faster
    if os.environ.get("MAGPHASE_EPOCHS", "") == "builtin":
        # explicit opt-in (or use_builtin_epoch_tracker()): the built-in zero-frequency-filtering tracker
        # (magphase_amd/epochs.py).  Not REAPER: the epochs differ, hence so do the pitch-synchronous features --
        # parity unpinned for this front end, so it is never substituted silently.
        from . import epochs
        v_sig, fs = la.read_audio_file(wav_file)
        return epochs.track_epochs(v_sig, fs, device=device if device is not None else get_engine().device)
    if la.find_reaper() is None:
        raise RuntimeError(
            "no epochs for %s: neither an epoch provider (set_epoch_provider), nor %s, nor a REAPER binary.  Features "
            "are pitch-synchronous, so the epoch source is part of the result: opt into the built-in tracker "
            "explicitly with MAGPHASE_EPOCHS=builtin or magphase.use_builtin_epoch_tracker() (not REAPER: parity "
            "unpinned)." % (wav_file, est))
    est_tmp = lu.ins_pid("temp.est")
    la.reaper(wav_file, est_tmp)
    try:
        m = np.atleast_2d(np.loadtxt(est_tmp, skiprows=7, usecols=[0, 1]))
    finally:
        if os.path.exists(est_tmp):
            os.remove(est_tmp)
    return m[:, 0], m[:, 1]


def _epochs_for_batch(wav_files, device=None):
    """_epochs_for over a list: [(v_pm_sec, v_voi) | Exception].  Without an epoch provider the .est files next to the
    wavs are parsed in one native call (la.read_est_batch); a wav without one takes _epochs_for's remaining routes
    (device: see _epochs_for -- iobatch's reader thread passes its engine's device)."""
    if _epoch_provider is None:
        res = la.read_est_batch([os.path.splitext(f)[0] + ".est" for f in wav_files])
    else:
        res = [FileNotFoundError()] * len(wav_files)
    out = []
    for f, r in zip(wav_files, res):
        if isinstance(r, FileNotFoundError):
            try:
                r = _epochs_for(f, device=device)
            except (KeyboardInterrupt, SystemExit):
                raise
            except Exception as e:
                r = e
        out.append(r)
    return out


# ======================================================================================================
# helper names of the reference's module that Merlin-side callers import (array in, float64 array out)
# ======================================================================================================
def windowing(v_sig, v_pm, win_func=np.hanning):
    """
    magphase.py:74-119: pitch-synchronous frames sig[pm_{f-1} .. pm_{f+1}] times the non-symmetric window of their two
    half lengths.  win_func: a window function, a list of them (one per frame, Q11) or None (no window).
    Returns (l_frames, v_lens, v_pm_plus, v_shift, v_rights) -- float64 frames on the host, like the reference (the
    batched device form of the same step is the front end of mpx_analysis_frames).
    """
    v_sig = np.asarray(v_sig)
    pm, left, right = hm.frame_bounds(v_pm, np.size(v_sig))
    v_pm_plus = np.hstack((0, pm, np.size(v_sig) - 1))
    l_frames = []
    for f in range(pm.size):
        v_frm = v_sig[v_pm_plus[f]:v_pm_plus[f + 2] + 1]
        fn = win_func[f] if isinstance(win_func, list) else win_func
        if fn is not None:
            v_frm = v_frm * la.gen_non_symmetric_win(left[f], right[f], fn)
        l_frames.append(v_frm)
    v_lens = np.array([len(x) for x in l_frames], dtype=int)
    return l_frames, v_lens, v_pm_plus, left.astype(int), right.astype(int)


def ola(m_frm, v_pm, win_func=None, device=None):
    """
    magphase.py:34-62 (PSOLA): frame i added at pm[i] - pm[0], head and tail trimmed so that frame centres land on the
    epochs.  Frames of 1024 / 2048 / 4096 samples without a window go through the device gather (mpx_ola_gather: the
    reference's ascending summation order, float32); anything else is summed on the host in float64.  With win_func the
    frames are multiplied by the centred anti-ringing window first -- IN PLACE, like the reference (magphase.py:48).
    device=False (or MAGPHASE_OLA_HOST=1) keeps every call on the float64 host sum, the reference's own arithmetic.
    """
    if device is None:
        device = os.environ.get("MAGPHASE_OLA_HOST", "0") != "1"
    v_pm = np.asarray(v_pm).astype(int)
    nfrms, frmlen = np.shape(m_frm)
    rel, start, out_len = hm.ola_plan(v_pm, frmlen)
    if win_func is not None:
        v_shift = np.append(la.pm_to_shift(v_pm), v_pm[-1] - v_pm[-2] if nfrms > 1 else v_pm[-1])
        for i in range(nfrms):
            m_frm[i, :] *= la.gen_centr_win(v_shift[i], v_shift[i + 1], frmlen, win_func=win_func)
    if device and win_func is None and frmlen in (1024, 2048, 4096) and nfrms > 0 and out_len > 0:
        e = get_engine()
        frames = e.to_device(np.ascontiguousarray(m_frm, dtype=np.float32), np.float32)
        t = e.to_device_packed([("fo", np.array([0, nfrms]), np.int32), ("rel", rel, np.int32),
                                ("st", np.array([start]), np.int32), ("oo", np.array([0, out_len]), np.int64)])
        out = e.ola_gather(frmlen, frames, t["fo"], t["rel"], t["st"], t["oo"], out_len, out_len)
        return e.to_host_f64(out)
    v_sig = np.zeros(int(v_pm[-1]) + frmlen)
    for i in range(nfrms):
        v_sig[rel[i]:rel[i] + frmlen] += m_frm[i, :]
    return v_sig[start:start + out_len]


def get_shifts_and_frm_locs_from_const_shifts(v_shift_c_rate, frm_rate_ms, fs, interp_type='linear'):
    """magphase.py:1426-1449 (Q16): the serial backward scan from the last constant-rate centre, in the library's host
    function (scipy interp1d's float64 operation sequence, bit-identical: golden G7)."""
    from .hostplan import _const_to_variable_scan

    if interp_type != 'linear':
        return hm._const_to_variable_scan_scipy(v_shift_c_rate, frm_rate_ms, fs)
    return _const_to_variable_scan(v_shift_c_rate, frm_rate_ms, fs)


def interp_from_variable_to_const_frm_rate(m_data, v_pm_smpls, const_rate_ms, fs, interp_type='linear'):
    """magphase.py:2219-2239 (Q15): rows at the epochs -> rows on the constant-rate grid, float64 on the host (scipy's
    interp1d like the reference; the batched device form is the operand load of mpx_mel_warp)."""
    from scipy import interpolate

    m_data = np.asarray(m_data, dtype=np.float64)
    squeeze = m_data.ndim == 1
    m2 = m_data[:, None] if squeeze else m_data
    v_pm_smpls = np.asarray(v_pm_smpls)
    grid = np.arange(fs * const_rate_ms / 1000, v_pm_smpls[-1], fs * const_rate_ms / 1000)
    if v_pm_smpls[0] > 0:   # the first row is held back to sample 0
        f = interpolate.interp1d(np.r_[0, v_pm_smpls], np.vstack((m2[0, :], m2)), axis=0, kind=interp_type)
    else:
        f = interpolate.interp1d(v_pm_smpls, m2, axis=0, kind=interp_type)
    out = f(grid)
    return out[:, 0] if squeeze else out


def interp_from_const_to_variable_rate(m_data, v_frm_locs_smpls, frm_rate_ms, fs, interp_type='linear'):
    """magphase.py:2242-2252: rows on the constant-rate grid -> rows at the frame locations (host float64)."""
    from scipy import interpolate

    m_data = np.asarray(m_data, dtype=np.float64)
    centres = (fs * frm_rate_ms / 1000) * np.arange(1, np.size(m_data, 0) + 1)
    return interpolate.interp1d(centres, m_data, axis=0, kind=interp_type)(v_frm_locs_smpls)


# constants (magphase.py:3279-3317)
define_alpha = hm.define_alpha
define_fft_len = hm.define_fft_len
define_crossfade_params = hm.define_crossfade_params
shift_to_f0_raw = hm.shift_to_f0
f0_to_shift = hm.f0_to_shift


def write_featfile(m_data, out_dir, filename):
    """magphase.py:2787-2791."""
    lu.write_binfile(m_data, os.path.join(out_dir, filename))


# ======================================================================================================
# lossless analysis
# ======================================================================================================
def analysis_lossless_batch(utts, fft_len=None, engine=None, return_device=False, copy=True):
    """
    Batched magphase.py:2869-2906 for utterances that already have epochs.
    utts: list of (v_sig, fs, v_pm_sec, v_voi).  Returns a list of
    (m_mag, m_real, m_imag, v_f0, fs, v_shift) in float64 numpy (or device tensors if return_device).
    copy=True (default): every utterance owns its arrays, like the reference's (independent, freeing one frees its
    memory).  copy=False: the utterances' matrices are ROW VIEWS of three arrays that hold the whole batch -- no second
    pass over the data (0.7 GB for 16 utterances), but keeping one utterance alive keeps the batch alive and in-place
    edits are made in the shared arrays; bench.py and iobatch use it.
    v_sig may be a 1-D torch tensor on the engine's device (float32 / float16 / bfloat16 / float64, any element stride):
    the samples stay on the device -- one float32 contiguous utterance is read where it lies, otherwise the batch is
    converted and concatenated there; host arrays in the same batch are uploaded one by one (the slow mixed case) -- and
    the rows equal those of the host-array call on the same float32 samples bit for bit.  v_pm_sec and v_voi stay host
    arrays.  A CPU tensor is treated as a host array; a tensor on another device raises ValueError.  Launches go to
    torch's current stream of the engine's device.
    Autograd: with return_device, grad mode on and a device v_sig that requires grad, m_mag / m_real / m_imag carry a
    grad_fn and tensor.backward() reaches v_sig (magphase_amd/autograd.py; the forward launch and its rows are the
    same).  Not differentiable: v_pm_sec, v_voi and fs; v_f0 and v_shift carry no grad_fn; no double backward.
    """
    engine = engine or get_engine()
    plan = LosslessAnalysisPlan(engine, utts, fft_len=fft_len)
    for lens in plan.long_frame_lens:
        for n in lens:  # Q19: truncation warns, it does not raise (magphase.py:311-315)
            warnings.warn(_WARN_LONG % (plan.fft_len, n))
    mag, real, imag = _run_lossless_analysis(plan, utts, return_device)
    if not return_device:   # one pinned, chunked D2H per stream for the whole batch (engine.to_host_f64)
        h_feats = tuple(engine.to_host_f64_many([mag, real, imag]))
    out = []
    for u in range(len(utts)):
        a, b = int(plan.frame_off[u]), int(plan.frame_off[u + 1])
        if return_device:
            feats = (mag[a:b], real[a:b], imag[a:b])
        else:
            # the utterance's rows of the batch's arrays (disjoint views: no second pass over the 0.7 GB a 16-utterance
            # batch returns; a one-utterance batch is its own array)
            feats = h_feats if len(utts) == 1 else tuple((h[a:b].copy() if copy else h[a:b]) for h in h_feats)
        out.append(feats + (plan.v_f0[u], plan.fs[u], plan.v_shift[u].astype(int)))
    return out


def _run_lossless_analysis(plan, utts, return_device):
    """plan.run() -> the batch's three float32 device matrices.  Through autograd.analyze -- the same launch inside a
    torch.autograd.Function -- under hostmath.wants_grad's rule for the v_sig (a CPU tensor is a host array to the plan)."""
    if hm.wants_grad(return_device, [u[0] for u in utts]):
        from .autograd import analyze

        return analyze(plan, [u[0] for u in utts])
    return plan.run()


def analysis_lossless_from_epochs(v_sig, fs, v_pm_sec, v_voi, fft_len=None):
    """magphase.py:2869-2906 from the point where the epochs have been read (array interface)."""
    return analysis_lossless_batch([(v_sig, fs, v_pm_sec, v_voi)], fft_len=fft_len)[0]


def analysis_lossless(wav_file, fft_len=None, out_dir=None):
    """magphase.py:2869-2906."""
    v_sig, fs = la.read_audio_file(wav_file)
    v_pm_sec, v_voi = _epochs_for(wav_file)
    m_mag, m_real, m_imag, v_f0, fs, v_shift = analysis_lossless_from_epochs(v_sig, fs, v_pm_sec, v_voi, fft_len)
    if type(out_dir) is str:
        file_id = os.path.basename(wav_file).split(".")[0]
        write_featfile(m_mag, out_dir, file_id + ".mag")
        write_featfile(m_real, out_dir, file_id + ".real")
        write_featfile(m_imag, out_dir, file_id + ".imag")
        write_featfile(v_f0, out_dir, file_id + ".f0")
        write_featfile(v_shift, out_dir, file_id + ".shift")
        return
    return m_mag, m_real, m_imag, v_f0, fs, v_shift


# ======================================================================================================
# lossless synthesis
# ======================================================================================================
def synthesis_from_lossless_batch(feats, engine=None, return_device=False):
    """
    Batched magphase.py:1759-1776.  feats: list of (m_mag, m_real, m_imag, v_f0, fs), all with the same
    number of bins.  Returns a list of float64 numpy signals (device float32 with return_device: views of one buffer).
    m_mag / m_real / m_imag may be torch tensors on the engine's device (float32 / float16 / bfloat16 / float64, any
    row stride): they are gathered on the device (Engine.pack_rows); one float32 utterance is taken without a copy.  CPU
    tensors are treated as host arrays.  Launches go to torch's current stream of the engine's device.
    Autograd: with return_device, grad mode on and a device matrix that requires grad, the returned signals carry a
    grad_fn and tensor.backward() reaches m_mag / m_real / m_imag (magphase_amd/autograd.py; the forward launch and its
    samples are the same).  Not differentiable: v_f0 and fs; no double backward.
    """
    feats, _on_dev = _tensor_inputs(feats, _LOSSLESS_NAMES)
    engine = engine or get_engine()
    H = int(np.shape(feats[0][0])[1])
    fft_len = 2 * (H - 1)
    plan = LosslessSynthesisPlan(engine, [f[3] for f in feats], [f[4] for f in feats], fft_len)
    pcm = _run_lossless_synthesis(engine, plan, feats, H, return_device)
    if return_device:
        return [pcm[int(plan.out_off_host[u]):int(plan.out_off_host[u + 1])] for u in range(len(feats))]
    pcm = engine.to_host_f64(pcm)
    return [pcm[plan.out_off_host[u]:plan.out_off_host[u + 1]] for u in range(len(feats))]


def _run_lossless_synthesis(engine, plan, feats, H, return_device):
    """plan.run on the packed matrices of feats (_feats_cat_device) -> the float32 [total_out] device buffer.  Through
    autograd.synthesize -- the same two calls inside a torch.autograd.Function -- under hostmath.wants_grad's rule for the
    matrices (CPU tensors are host arrays by now)."""
    if hm.wants_grad(return_device, [x for f in feats for x in f[:3]]):
        from .autograd import synthesize

        return synthesize(plan, lambda fs_: _feats_cat_device(engine, fs_, H), feats)
    cat = _feats_cat_device(engine, feats, H)
    return plan.run(cat[0], cat[1], cat[2])


def _feats_cat_device(engine, feats, H):
    """The mag / real / imag matrices of a batch, each stream as ONE device float32 matrix (engine.empty_feats pitch):
    a one-utterance float32 device tensor is taken as it is, host arrays go through pinned staging in one DMA, device
    tensors (float32 / float16 / bfloat16 / float64, any row stride) are gathered by ONE mpx_rows_pack launch for all
    the streams that hold any (Engine.pack_rows; host arrays among them are uploaded one by one: the slow mixed case)."""
    torch = __import__("torch")
    rows = np.concatenate(([0], np.cumsum([int(np.shape(f[0])[0]) for f in feats])))
    for u, f in enumerate(feats):
        for k in range(3):
            if torch.is_tensor(f[k]) and f[k].device != engine.device:
                raise ValueError("feats[%d]: %s is on %s, the engine runs on %s"
                                 % (u, _LOSSLESS_NAMES[k], f[k].device, engine.device))
    cat, packed = [None] * 3, []
    for k in range(3):   # one device matrix per stream (engine.empty_feats)
        if len(feats) == 1 and torch.is_tensor(feats[0][k]) and feats[0][k].dtype == torch.float32:
            cat[k] = feats[0][k]
            continue
        if not any(torch.is_tensor(f[k]) for f in feats):   # host arrays: narrowed into pinned staging, one DMA
            cat[k] = engine.feats_cat_to_device([f[k] for f in feats], H)
            if cat[k] is not None:
                continue
        cat[k] = engine.empty_feats(int(rows[-1]), H)
        packed.append(k)
    if packed:
        engine.pack_rows([[f[k] for f in feats] for k in packed], [cat[k] for k in packed])
    return cat


def synthesis_from_lossless(m_mag, m_real, m_imag, v_f0, fs):
    """magphase.py:1759-1776."""
    return synthesis_from_lossless_batch([(m_mag, m_real, m_imag, v_f0, fs)])[0]


# ======================================================================================================
# lossless features on a constant frame rate (analysis: magphase.py:2967-2980 without the mel warp; synthesis: the
# constant -> variable rate steps of :848, :861-870 followed by :1759-1776)
# ======================================================================================================
def analysis_lossless_const_rate_batch(utts, fft_len=None, const_rate_ms=5.0, engine=None, return_device=False, copy=True):
    """
    analysis_lossless_batch with the rows on a constant frame rate: per utterance the reference's
    interp_from_variable_to_const_frm_rate of mag / real / imag (grid arange(step, pm[-1], step), the first row held back
    to t = 0) and f0 interpolated through the voiced points times the interpolated voicing > 0.5 (magphase.py:2967-2980,
    const_rate_ms as a parameter).  utts: list of (v_sig, fs, v_pm_sec, v_voi), one fft_len per batch.  Returns a list of
    (m_mag, m_real, m_imag, v_f0, fs): float64 numpy, or float32 device rows with return_device (v_f0 is float64 numpy
    either way).  An utterance shorter than one step gives (0, H) matrices and an empty f0; one without a voiced frame
    raises (IndexError, as analysis_compressed_batch(b_const_rate=True) does).  copy: as analysis_lossless_batch.
    v_sig may be a 1-D torch tensor on the engine's device (float32 / float16 / bfloat16 / float64, any element stride),
    under analysis_lossless_batch's rules: the samples stay on the device, the rows equal those of the host-array call on
    the same float32 samples bit for bit, a CPU tensor is a host array, a tensor on another device raises ValueError.
    Autograd: with return_device, grad mode on and a device v_sig that requires grad, m_mag / m_real / m_imag carry a
    grad_fn and tensor.backward() reaches v_sig (magphase_amd/autograd.py: analyze_const_rate; the forward launches and
    their rows are the same, nothing is kept between the passes).  Not differentiable: v_pm_sec, v_voi, fs and
    const_rate_ms; v_f0 stays a float64 host vector without grad_fn; no double backward.
    """
    const_rate_ms = check_const_rate_ms(const_rate_ms)
    utts = list(utts)
    if not utts:
        return []
    engine = engine or get_engine()
    plan = LosslessConstRateAnalysisPlan(engine, utts, fft_len=fft_len, const_rate_ms=const_rate_ms)
    for lens in plan.long_frame_lens:
        for n in lens:  # Q19: truncation warns, it does not raise (magphase.py:311-315)
            warnings.warn(_WARN_LONG % (plan.fft_len, n))
    if hm.wants_grad(return_device, [u[0] for u in utts]):
        from .autograd import analyze_const_rate

        mag, real, imag = analyze_const_rate(plan, [u[0] for u in utts])
    else:
        mag, real, imag = plan.run()
    if not return_device:
        h_feats = tuple(engine.to_host_f64_many([mag, real, imag]))
    out = []
    for u in range(len(utts)):
        a, b = int(plan.out_off[u]), int(plan.out_off[u + 1])
        if return_device:
            feats = (mag[a:b], real[a:b], imag[a:b])
        else:
            feats = h_feats if len(utts) == 1 else tuple((h[a:b].copy() if copy else h[a:b]) for h in h_feats)
        out.append(feats + (plan.v_f0[u], plan.fs[u]))
    return out


def analysis_lossless_const_rate(wav_file, fft_len=None, out_dir=None, const_rate_ms=5.0):
    """analysis_lossless (magphase.py:2869-2906) with the rows on a constant frame rate (see
    analysis_lossless_const_rate_batch).  With out_dir: writes <name>.mag / .real / .imag / .f0 (float32 binfiles)."""
    const_rate_ms = check_const_rate_ms(const_rate_ms)
    v_sig, fs = la.read_audio_file(wav_file)
    v_pm_sec, v_voi = _epochs_for(wav_file)
    m_mag, m_real, m_imag, v_f0, fs = analysis_lossless_const_rate_batch([(v_sig, fs, v_pm_sec, v_voi)], fft_len=fft_len,
                                                                         const_rate_ms=const_rate_ms)[0]
    if type(out_dir) is str:
        file_id = os.path.basename(wav_file).split(".")[0]
        write_featfile(m_mag, out_dir, file_id + ".mag")
        write_featfile(m_real, out_dir, file_id + ".real")
        write_featfile(m_imag, out_dir, file_id + ".imag")
        write_featfile(v_f0, out_dir, file_id + ".f0")
        return
    return m_mag, m_real, m_imag, v_f0, fs


def _const_rate_synthesis_check(feats):
    """Argument checks of synthesis_from_lossless_const_rate_batch, on the host: one bin count, row counts that agree.
    Returns H."""
    H = None
    for i, f in enumerate(feats):
        if len(f) != 5:
            raise ValueError("feats[%d]: expected (m_mag, m_real, m_imag, v_f0, fs)" % i)
        shapes = [tuple(np.shape(x)) for x in f[:3]]
        if any(len(sh) != 2 for sh in shapes) or len(set(shapes)) != 1:
            raise ValueError("feats[%d]: m_mag, m_real and m_imag must be 2-D of one shape, got %s" % (i, shapes))
        n, h = shapes[0]
        if np.ndim(f[3]) != 1 or np.size(f[3]) != n:
            raise ValueError("feats[%d]: v_f0 has %d values for %d rows" % (i, np.size(f[3]), n))
        if H is not None and h != H:
            raise ValueError("synthesis_from_lossless_const_rate_batch: all utterances of a call must share the bin count "
                             "(%d and %d)" % (H, h))
        H = h
    if H is None or 2 * (H - 1) not in (1024, 2048, 4096):
        raise ValueError("synthesis_from_lossless_const_rate_batch: %s bins (fft_len 1024, 2048 or 4096)" % (H,))
    return H


def synthesis_from_lossless_const_rate_batch(feats, const_rate_ms=5.0, engine=None, return_device=False):
    """
    synthesis_from_lossless (magphase.py:1759-1776) from lossless features on a constant frame rate: feats is a list of
    (m_mag, m_real, m_imag, v_f0, fs) with one row per const_rate_ms (numpy or device tensors, as
    synthesis_from_lossless_batch takes them; one bin count per call).  Per utterance, the reference's composition
    f0_to_shift -> get_shifts_and_frm_locs_from_const_shifts -> interp_from_const_to_variable_rate of mag / real / imag
    and of the voicing (> 0.5) -> shift_to_f0(b_smooth=False) -> synthesis_from_lossless, except that the scan runs to
    the start of the grid (the reference's stops after 2n slots).  Time-stretch: synthesise with
    another const_rate_ms than the analysis used; pitch-shift: scale v_f0.  The rows are interpolated as the synthesis
    kernel loads them.  Returns a list of float64 signals (device float32 with return_device).
    Autograd as synthesis_from_lossless_batch: with return_device, grad mode on and a device matrix that requires grad, the
    signals carry a grad_fn and backward() reaches the constant-rate rows of m_mag / m_real / m_imag (not v_f0, not fs).
    """
    const_rate_ms = check_const_rate_ms(const_rate_ms)
    feats = list(feats)
    if not feats:
        return []
    feats, _on_dev = _tensor_inputs(feats, _LOSSLESS_NAMES)
    H = _const_rate_synthesis_check(feats)
    f0_list = [np.asarray(f[3].cpu() if hasattr(f[3], "cpu") else f[3], dtype=np.float64) for f in feats]
    fs_list = [f[4] for f in feats]
    host = plan_const_rate_synthesis(f0_list, fs_list, const_rate_ms)   # (raises before any device call)
    engine = engine or get_engine()
    plan = LosslessConstRateSynthesisPlan(engine, f0_list, fs_list, 2 * (H - 1), const_rate_ms=const_rate_ms,
                                          host=host)
    pcm = _run_lossless_synthesis(engine, plan, feats, H, return_device)
    o = plan.out_off_host
    if return_device:
        return [pcm[int(o[u]):int(o[u + 1])] for u in range(len(feats))]
    h = engine.to_host_f64(pcm)
    return [h[int(o[u]):int(o[u + 1])] for u in range(len(feats))]


def synthesis_from_lossless_const_rate(m_mag, m_real, m_imag, v_f0, fs, const_rate_ms=5.0):
    """synthesis_from_lossless from constant-rate lossless features (see synthesis_from_lossless_const_rate_batch)."""
    return synthesis_from_lossless_const_rate_batch([(m_mag, m_real, m_imag, v_f0, fs)], const_rate_ms=const_rate_ms)[0]


def copy_synthesis_lossless_batch(utts, fft_len=None, engine=None, return_device=False, with_feats=True):
    """
    analysis_lossless followed by synthesis_from_lossless on the same frames (magphase.py:2869-2906, :1759-1776: what
    demos/demo_copy_synthesis_lossless.py:44-50 does per file) for a batch, as ONE device launch
    (mpx_roundtrip_lossless_ola): the feature rows are written and the waveform is built from them without reading them
    back.  utts: list of (v_sig, fs, v_pm_sec, v_voi), one fft_len per batch.  Returns a list of
    ((m_mag, m_real, m_imag, v_f0, fs, v_shift), v_syn_sig): analysis_lossless' tuple and synthesis_from_lossless' signal,
    float64 numpy (device tensors with return_device); with_feats=False skips the download of the three matrices
    (None in their place) when only the waveform is wanted.
    """
    engine = engine or get_engine()
    if not utts:
        return []
    plan = LosslessRoundTripPlan(engine, utts, fft_len=fft_len)
    a = plan.analysis
    for lens in a.long_frame_lens:
        for n in lens:  # Q19: truncation warns, it does not raise (magphase.py:311-315)
            warnings.warn(_WARN_LONG % (plan.fft_len, n))
    (mag, real, imag), pcm = plan.run()
    if not return_device:
        h_feats = tuple(engine.to_host_f64_many([mag, real, imag])) if with_feats else None
        h_pcm = engine.to_host_f64(pcm)
    out = []
    for u in range(len(utts)):
        fa, fb = int(a.frame_off[u]), int(a.frame_off[u + 1])
        oa, ob = int(plan.out_off_host[u]), int(plan.out_off_host[u + 1])
        if return_device:
            feats, sig = (mag[fa:fb], real[fa:fb], imag[fa:fb]), pcm[oa:ob]
        else:
            feats = tuple(h[fa:fb].copy() for h in h_feats) if with_feats else (None, None, None)
            sig = h_pcm[oa:ob]
        out.append((feats + (a.v_f0[u], a.fs[u], a.v_shift[u].astype(int)), sig))
    return out


_GL_INITS = ("random", "linear", "min_phase")


def _griffin_lim_check(utts, win_func, phase_init, niters):
    """All of griffin_lim_batch's argument checks, on the host, before any draw or device call.  Returns
    (shifts, inits, N)."""
    if win_func is not np.hanning:
        raise ValueError("griffin_lim: only win_func=np.hanning is supported")
    if isinstance(niters, bool) or not isinstance(niters, (int, np.integer)) or niters < 1:
        raise ValueError("griffin_lim: niters must be an integer >= 1")
    if isinstance(phase_init, (list, tuple)):
        if len(phase_init) != len(utts):
            raise ValueError("griffin_lim_batch: one phase_init per utterance")
        inits = list(phase_init)
    else:
        inits = [phase_init] * len(utts)
    shifts, N = [], None
    for (m_mag, v_shift), init in zip(utts, inits):
        v, n = hm.griffin_lim_shifts(m_mag, v_shift)
        if N is not None and n != N:
            raise ValueError("griffin_lim_batch: all utterances of a call must share fft_len (bucket by bins)")
        N = n
        if isinstance(init, str):
            if init not in _GL_INITS:
                raise ValueError("griffin_lim: unknown phase_init %r (%s or an ndarray)" % (init, ", ".join(_GL_INITS)))
        elif isinstance(init, np.ndarray):
            if init.shape != np.shape(m_mag):
                raise ValueError("griffin_lim: phase_init array of shape %s for m_mag of shape %s"
                                 % (init.shape, np.shape(m_mag)))
        else:
            raise ValueError("griffin_lim: phase_init must be 'random', 'linear', 'min_phase' or an ndarray")
        shifts.append(v)
    return shifts, inits, N


def _griffin_lim_tensor_args(utts, phase_init):
    """torch tensors among griffin_lim_batch's m_mag and phase_init, checked without a device: float32 / float16 /
    bfloat16 / float64 and 2-D (ValueError naming the utterance otherwise); CPU tensors become host arrays (float16 /
    bfloat16 widened to float32: exact).  Returns (utts, phase_init, the tensors that are not on the CPU)."""
    import sys

    torch = sys.modules.get("torch")
    per_utt = isinstance(phase_init, (list, tuple))
    inits = list(phase_init) if per_utt else [phase_init]
    if torch is None or not any(torch.is_tensor(x) for x in [u[0] for u in utts] + inits):
        return utts, phase_init, []
    on_dev = []

    def host_or_device(x, name):
        if not torch.is_tensor(x):
            return x
        hm.check_feature_tensor(x, name)
        if x.device.type == "cpu":
            x = x.detach()
            return (x.float() if x.element_size() == 2 else x).numpy()
        on_dev.append((name, x))
        return x.detach()

    utts = [(host_or_device(u[0], "utts[%d]: m_mag" % i),) + tuple(u[1:]) for i, u in enumerate(utts)]
    inits = [host_or_device(x, "phase_init[%d]" % i if per_utt else "phase_init") for i, x in enumerate(inits)]
    return utts, (inits if per_utt else inits[0]), on_dev


def _shape_only(x):
    """A device tensor's stand-in for the host checks (shape only; no memory, no device access)."""
    return x if isinstance(x, np.ndarray) or not hasattr(x, "data_ptr") else np.broadcast_to(np.float32(0), tuple(x.shape))


def _griffin_lim_min_phase(engine, N, tgt, mp_rows, i_re, i_im, want_phase):
    """la.build_min_phase_from_mag_spec's phasors of rows mp_rows of tgt, bins 0 and N/2 at phase 0, (-1)^k folded in,
    written to those rows of i_re / i_im; returns their phases when want_phase."""
    torch = __import__("torch")
    H = N // 2 + 1
    ld = int(engine.lib.mpx_spec_ld(H))
    idx = np.concatenate(mp_rows)
    rows = torch.from_numpy(idx.astype(np.int32)).to(engine.device)
    n = int(idx.size)
    o_m, o_r, o_i = (engine.empty((n, ld)) for _ in range(3))
    engine.launch("mpx_min_phase", N, engine.tables(N), tgt, rows, rows,
                  torch.zeros(n, dtype=torch.float32, device=engine.device), n, o_m, o_r, o_i, ld)
    re, im = o_r[:, :H].clone(), o_i[:, :H].clone()
    re[:, 0], im[:, 0], re[:, -1], im[:, -1] = 1.0, 0.0, 1.0, 0.0
    mp_phase = torch.atan2(im, re) if want_phase else None
    sgn = torch.ones(H, dtype=torch.float32, device=engine.device)
    sgn[1::2] = -1.0
    ridx = rows.long()
    i_re[ridx] = re * sgn
    i_im[ridx] = im * sgn
    return mp_phase


def _griffin_lim_device_fold(engine, utts, shifts, inits, N, niters, return_device):
    """griffin_lim_batch with the initial phase and the fold on the device (fold='device'): the target rows are gathered
    by Engine.pack_rows when one of them is a device tensor, else uploaded as with the host fold; the rest is
    _griffin_lim_device_rows."""
    torch = __import__("torch")
    H = N // 2 + 1
    sizes = [int(m.shape[0]) for m, _ in utts]
    F = int(sum(sizes))
    tgt = engine.empty((max(F, 1), int(engine.lib.mpx_spec_ld(H))))[:F, :H]
    for init in inits:   # the reference zeroes columns 0 and H - 1 of an ndarray init in place; a device tensor is not written
        print('Starting Griffin-Lim. It could take a while...')
        if isinstance(init, np.ndarray):
            init[:, 0] = 0
            init[:, -1] = 0
    if any(torch.is_tensor(m) for m, _ in utts):
        engine.pack_rows([[m for m, _ in utts]], [tgt])
    else:
        tgt.copy_(torch.from_numpy(np.concatenate([np.asarray(m, dtype=np.float32) for m, _ in utts])))
    return _griffin_lim_device_rows(engine, tgt, sizes, shifts, inits, N, niters, return_device)


def _griffin_lim_device_rows(engine, tgt, sizes, shifts, inits, N, niters, return_device, init_rows=None):
    """Griffin-Lim from device target rows tgt ([sum(sizes) x H] at pitch mpx_spec_ld), initial phase and fold on the
    device: array inits -- host or device -- are gathered into one float32 [rows x H] matrix and folded as
    MPX_GL_FOLD_HALF, 'random' utterances are folded from numpy's raw words (Engine.numpy_global_words, in groups of at
    most Engine.GL_WORDS_GROUP_SAMPLES samples), 'linear' is (M, 1, 0), 'min_phase' takes mpx_min_phase's phasors.
    init_rows: three matrices of tgt's shape and pitch to fold into (allocated here when None).  Returns a list of
    (signal, phase rows) per utterance: float64 host arrays, or float32 device views with return_device."""
    torch = __import__("torch")
    H = N // 2 + 1
    U = len(sizes)
    f_off = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    F = int(f_off[-1])
    ld = int(engine.lib.mpx_spec_ld(H))
    dev = lambda: engine.empty((max(F, 1), ld))[:F, :H]   # noqa: E731
    i_mag, i_re, i_im = init_rows if init_rows is not None else (dev(), dev(), dev())
    del init_rows
    ph_dev = dev() if niters == 1 else None
    outs = (i_mag, i_re, i_im)
    # array inits: one gather, then one fold per utterance
    arr = [u for u in range(U) if not isinstance(inits[u], str)]
    if arr:
        half = engine.empty((sum(sizes[u] for u in arr), H))
        engine.pack_rows([[inits[u] for u in arr]], [half])
        o = 0
        for u in arr:
            engine.griffin_lim_fold(N, "half", tgt, half[o:o + sizes[u]], int(f_off[u]), sizes[u], outs, ph_dev)
            o += sizes[u]
        del half
    # 'linear': angle(fft(delta_{N/2})) is 0 or pi, the fold is (M, 1, 0) exactly
    lin = [u for u in range(U) if isinstance(inits[u], str) and inits[u] == "linear"]
    if lin:
        row = None
        if ph_dev is not None:
            ph, _full = hm.griffin_lim_initial_phase("linear", np.empty((1, H)))
            row = torch.from_numpy(np.ascontiguousarray(ph[0, :H], dtype=np.float32)).to(engine.device)
        for u in lin:
            a, b = int(f_off[u]), int(f_off[u + 1])
            i_mag[a:b] = tgt[a:b]
            i_re[a:b] = 1.0
            i_im[a:b] = 0.0
            if row is not None:
                ph_dev[a:b] = row
    # 'min_phase': mpx_min_phase's phasors, as with the host fold
    mp_u = [u for u in range(U) if isinstance(inits[u], str) and inits[u] == "min_phase"]
    if mp_u:
        mp_rows = [np.arange(int(f_off[u]), int(f_off[u + 1])) for u in mp_u]
        for u in mp_u:
            a, b = int(f_off[u]), int(f_off[u + 1])
            i_mag[a:b] = tgt[a:b]
        mp_phase = _griffin_lim_min_phase(engine, N, tgt, mp_rows, i_re, i_im, ph_dev is not None)
        if mp_phase is not None:
            ph_dev[torch.from_numpy(np.concatenate(mp_rows)).to(engine.device)] = mp_phase
    # 'random': consecutive utterances are one contiguous draw of numpy's stream; generated and folded in groups
    rnd = [u for u in range(U) if isinstance(inits[u], str) and inits[u] == "random"]
    k = 0
    while k < len(rnd):
        group, n = [rnd[k]], sizes[rnd[k]] * N
        k += 1
        while k < len(rnd) and n + sizes[rnd[k]] * N <= engine.GL_WORDS_GROUP_SAMPLES:
            group.append(rnd[k])
            n += sizes[rnd[k]] * N
            k += 1
        words = engine.numpy_global_words(n, defer=True)
        o = j = 0
        while j < len(group):   # utterances that follow one another in the batch: one launch
            j1 = j + 1
            while j1 < len(group) and group[j1] == group[j1 - 1] + 1:
                j1 += 1
            a, b = int(f_off[group[j]]), int(f_off[group[j1 - 1] + 1])
            engine.griffin_lim_fold(N, "words", tgt, words, a, b - a, outs, ph_dev, phase_offset=o)
            o += (b - a) * N
            j = j1
        del words
    if rnd:
        engine.mt_sync()
    plan = GriffinLimPlan(engine, shifts, N)
    init = [i_mag, i_re, i_im]
    del i_mag, i_re, i_im, outs   # plan.run releases the init rows after the first synthesis
    sig, ph_last = plan.run(tgt, init, niters, phase_rows=True)
    if niters > 1:
        ph_dev = ph_last
    cut = lambda x, off: [x[int(off[u]):int(off[u + 1])] for u in range(U)]   # noqa: E731
    if return_device:
        return list(zip(cut(sig, plan.out_off_host), cut(ph_dev, f_off)))
    h_sig, h_ph = engine.to_host_f64(sig), engine.to_host_f64(ph_dev)
    return [(s.copy(), p.copy()) for s, p in zip(cut(h_sig, plan.out_off_host), cut(h_ph, f_off))]


def griffin_lim_batch(utts, win_func=np.hanning, phase_init='random', niters=30, engine=None, return_device=False,
                      fold=None):
    """
    griffin_lim (magphase.py:3320-3372) for a batch: utts = [(m_mag, v_shift), ...] with one fft_len per call;
    phase_init: one of 'random' / 'linear' / 'min_phase' / an ndarray for all, or a list with one per utterance.  Equal to
    sequential griffin_lim calls, numpy's global random draws included (one rand(F, N) per 'random' utterance, in batch
    order; an ndarray init has its columns 0 and H - 1 zeroed in place, as the reference's la.add_hermitian_half does).
    The first synthesis is the lossless synthesis kernel on folded inputs (hostmath.griffin_lim_fold); every further one
    is one mpx_griffin_lim_ola launch.  Returns a list of (v_sig, m_phase) float64 (device float32 with return_device).
    Deviation: shifts outside the reference's domain raise ValueError for every niters (the reference only fails once
    it analyses, niters >= 2).
    Device tensors: m_mag and an array phase_init may be 2-D torch tensors on the engine's device (float32 / float16 /
    bfloat16 / float64, any row stride: gathered by Engine.pack_rows; never written).  CPU tensors are host arrays;
    tensors of another device and integer / bool / complex tensors raise ValueError before any draw or launch.  v_shift
    stays a host vector.
    fold: where the initial phase is built and folded into the first synthesis' inputs.  'host': numpy, as described
    above.  'device': mpx_griffin_lim_fold (k_gl_fold) -- 'random' continues numpy's global
    MT19937 stream on the device (Engine.numpy_global_words: the state is left where the host draws would leave it, no
    [F x N] phase matrix exists) and the phases returned for niters = 1 are the kernel's float32 rows.  None: 'device' if
    an input is a device tensor, else 'host'; 'host' with a device tensor raises ValueError.
    """
    utts = list(utts)
    if not utts:
        return []
    if fold not in (None, 'host', 'device'):
        raise ValueError("griffin_lim_batch: fold must be None, 'host' or 'device', not %r" % (fold,))
    utts, phase_init, on_dev = _griffin_lim_tensor_args(utts, phase_init)
    if on_dev and fold == 'host':
        raise ValueError("griffin_lim_batch: fold='host' with a device tensor (%s)" % on_dev[0][0])
    if on_dev or fold == 'device':
        real = list(phase_init) if isinstance(phase_init, (list, tuple)) else [phase_init] * len(utts)
        shifts, _stand_ins, N = _griffin_lim_check(
            [(_shape_only(m),) + tuple(r) for m, *r in utts], win_func,
            [_shape_only(x) for x in phase_init] if isinstance(phase_init, (list, tuple)) else _shape_only(phase_init),
            niters)
        engine = engine or get_engine()
        for name, x in on_dev:
            if x.device != getattr(engine, "device", None):
                raise ValueError("griffin_lim_batch: %s is on %s, the engine runs on %s"
                                 % (name, x.device, getattr(engine, "device", None)))
        utts = [(m if hasattr(m, "data_ptr") else np.asarray(m), v) for m, v in utts]
        return _griffin_lim_device_fold(engine, utts, shifts, real, N, niters, return_device)
    shifts, inits, N = _griffin_lim_check(utts, win_func, phase_init, niters)
    H = N // 2 + 1
    sizes = [np.shape(m)[0] for m, _ in utts]
    f_off = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    F = int(f_off[-1])
    h_mag, h_re, h_im = (np.empty((F, H), dtype=np.float32) for _ in range(3))
    phase0, mp_rows = [None] * len(utts), []
    for u, ((m_mag, _), init) in enumerate(zip(utts, inits)):
        print('Starting Griffin-Lim. It could take a while...')
        a, b = int(f_off[u]), int(f_off[u + 1])
        ph, full = hm.griffin_lim_initial_phase(init, m_mag)
        if ph is None:   # 'min_phase': phasors from mpx_min_phase below
            h_mag[a:b] = m_mag
            mp_rows.append(np.arange(a, b))
            continue
        if niters == 1:
            phase0[u] = np.array(ph[:, :H], dtype=np.float64)
        h_mag[a:b], h_re[a:b], h_im[a:b] = hm.griffin_lim_fold(m_mag, ph, full)
    engine = engine or get_engine()
    torch = __import__("torch")
    ld = int(engine.lib.mpx_spec_ld(H))
    dev = lambda: engine.empty((max(F, 1), ld))[:F, :H]   # noqa: E731
    tgt, i_mag, i_re, i_im = dev(), dev(), dev(), dev()
    tgt.copy_(torch.from_numpy(np.concatenate([np.asarray(m, dtype=np.float32) for m, _ in utts])))
    for d, h in ((i_mag, h_mag), (i_re, h_re), (i_im, h_im)):
        d.copy_(torch.from_numpy(h))
    del h_mag, h_re, h_im   # (the copies above are synchronous: the host rows are no longer needed)
    mp_phase = None
    if mp_rows:
        mp_phase = _griffin_lim_min_phase(engine, N, tgt, mp_rows, i_re, i_im, niters == 1)
    plan = GriffinLimPlan(engine, shifts, N)
    init = [i_mag, i_re, i_im]
    del i_mag, i_re, i_im   # plan.run releases the init rows after the first synthesis
    sig, ph_dev = plan.run(tgt, init, niters, phase_rows=True)
    if niters == 1:
        if mp_phase is not None:
            ph_dev = dev()
            ph_dev[torch.from_numpy(np.concatenate(mp_rows)).to(engine.device)] = mp_phase
        if return_device and ph_dev is None:
            ph_dev = dev()
        if ph_dev is not None:
            for u, p in enumerate(phase0):
                if p is not None:
                    ph_dev[int(f_off[u]):int(f_off[u + 1])] = torch.from_numpy(p.astype(np.float32)).to(engine.device)
    if return_device:
        return [(sig[int(plan.out_off_host[u]):int(plan.out_off_host[u + 1])], ph_dev[int(f_off[u]):int(f_off[u + 1])])
                for u in range(len(utts))]
    h_sig = engine.to_host_f64(sig)
    h_ph = engine.to_host_f64(ph_dev) if ph_dev is not None else None
    out = []
    for u in range(len(utts)):
        a, b = int(f_off[u]), int(f_off[u + 1])
        p = phase0[u] if (niters == 1 and phase0[u] is not None) else h_ph[a:b].copy()
        out.append((h_sig[int(plan.out_off_host[u]):int(plan.out_off_host[u + 1])].copy(), p))
    return out


def griffin_lim(m_mag, v_shift, win_func=np.hanning, phase_init='random', niters=30):
    """magphase.py:3320-3372 (pitch-synchronous Griffin-Lim): (v_sig, m_phase) float64.  See griffin_lim_batch."""
    return griffin_lim_batch([(m_mag, v_shift)], win_func=win_func,
                             phase_init=[phase_init] if isinstance(phase_init, np.ndarray) else phase_init,
                             niters=niters)[0]


def _griffin_lim_from_mag_tables(lf0s, fs, N, b_const_rate):
    """The frame tables of synthesis_from_compressed (magphase.py:846-870, :879: integer shifts, constant -> variable rate
    rows) for a batch of host lf0 vectors, checked against Griffin-Lim's domain; ValueError naming the utterance."""
    from . import hostplan

    try:
        try:
            r = hostplan.plan_synthesis([np.exp(l) for l in lf0s], fs, N, b_const_rate, True)
        except hostplan.PlanFallback:
            r = hostplan.plan_synthesis_numpy(lf0s, fs, N, b_const_rate, True)
    except ValueError:   # which utterance: one at a time, in numpy (the reference's arithmetic, spelled out)
        for i, l in enumerate(lf0s):
            try:
                hostplan.plan_synthesis_numpy([l], fs, N, b_const_rate, True)
            except ValueError as err:
                raise ValueError("utts[%d]: v_lf0 gives shifts outside Griffin-Lim's domain at fft_len %d (v_shift[0] <= "
                                 "%d, the others <= %d): %s" % (i, N, N // 2, N // 2 - 1, err)) from None
        raise
    fo = np.asarray(r["frame_off"], dtype=np.int64)
    shifts = []
    for i in range(len(lf0s)):
        v = np.asarray(r["v_shift"][int(fo[i]):int(fo[i + 1])], dtype=np.int64)
        if v.size == 0:
            raise ValueError("utts[%d]: no synthesis frames" % i)
        right = np.append(v[1:], v[-1])
        if np.any(v < 0) or v[0] > N // 2 or np.any(right > N // 2 - 1):
            raise ValueError("utts[%d]: v_lf0 gives shifts outside Griffin-Lim's domain at fft_len %d (v_shift[0] <= %d, "
                             "the others <= %d)" % (i, N, N // 2, N // 2 - 1))
        shifts.append(v)
    return r, shifts


def griffin_lim_from_mag_batch(utts, fs, fft_len=None, phase_init='min_phase', niters=30, b_const_rate=False,
                               b_fbank_mel=False, engine=None, return_device=False):
    """Pitch-synchronous Griffin-Lim from the mel-log magnitudes and lf0 alone -- the third phase option of a
    magnitude-only acoustic model, beside synthesis_from_mag_batch's 'min_phase' and 'zero'.  utts: list of
    (m_mag_mel_log [rows x mag_dim], v_lf0 [rows]), host arrays or device tensors as synthesis_from_mag_batch takes them.
    The target magnitudes are exp of the mel unwarp on the device, one row per synthesis frame (mpx_mel_unwarp; at the
    constant rate mpx_mel_unwarp_rows with the constant -> variable rate row tables); the shifts are the integer v_shift of
    synthesis_from_compressed (magphase.py:846-870, :879), so the signal has the length and the epochs of
    synthesis_from_mag_batch on the same input; the rest is griffin_lim_batch(fold='device') on those device rows with
    phase_init 'min_phase', 'random' (numpy's global generator, continued on the device) or 'linear' for the whole batch.
    No noise is drawn and no noise table is built: nothing is taken from numpy's generator except the 'random' init.
    Returns the signals: float64 host arrays, or float32 device views with return_device.
    ValueError, naming the utterance, where a shift leaves Griffin-Lim's domain (v_shift[0] <= fft_len / 2, the others
    <= fft_len / 2 - 1) or the utterances differ in mag_dim; ValueError for an fft_len without Griffin-Lim kernels and an
    unknown phase_init.  No post-filter argument: post_filter_batch composes in front of this.  No autograd: the
    iterations are not differentiated, a tensor that requires grad is read as a constant."""
    utts = [tuple(u) for u in utts]
    if any(len(u) != 2 for u in utts):
        raise ValueError("utts: a list of (m_mag_mel_log, v_lf0)")
    if not isinstance(phase_init, str) or phase_init not in _GL_INITS:
        raise ValueError("griffin_lim_from_mag: unknown phase_init %r (%s)" % (phase_init, ", ".join(_GL_INITS)))
    if isinstance(niters, bool) or not isinstance(niters, (int, np.integer)) or niters < 1:
        raise ValueError("griffin_lim_from_mag: niters must be an integer >= 1")
    if not utts:
        return []
    N = int(fft_len) if fft_len else hm.define_fft_len(fs)
    if N not in hm.GL_FFT_LENS:
        raise ValueError("griffin_lim_from_mag: fft_len %d; supported: %s" % (N, hm.GL_FFT_LENS))
    alpha = hm.define_alpha(fs)
    utts, _on_dev = _tensor_inputs(utts, _MAG_NAMES, lf0_at=1)
    is_t = lambda x: hasattr(x, "data_ptr")   # noqa: E731  (what _tensor_inputs left: tensors that are not on the CPU)
    mags = [m if is_t(m) else np.atleast_2d(np.asarray(m)) for m, _ in utts]
    lf0s = [l if is_t(l) else np.atleast_1d(np.asarray(l, dtype=np.float64)) for _, l in utts]
    mag_dim = int(mags[0].shape[1]) if len(mags[0].shape) == 2 else -1
    for i, (m, l) in enumerate(zip(mags, lf0s)):
        if len(m.shape) != 2 or int(m.shape[1]) != mag_dim:
            raise ValueError("utts[%d]: m_mag_mel_log must be [rows x %d] like utts[0]'s, got shape %s"
                             % (i, mag_dim, tuple(m.shape)))
        if int(m.shape[0]) != int(l.shape[0]) or int(m.shape[0]) == 0:
            raise ValueError("utts[%d]: m_mag_mel_log has %d rows, v_lf0 %d" % (i, int(m.shape[0]), int(l.shape[0])))
    if not any(is_t(l) for l in lf0s):   # host lf0: every check before the first device call
        r, shifts = _griffin_lim_from_mag_tables(lf0s, fs, N, b_const_rate)
    engine = engine or get_engine()
    for i, m in enumerate(mags):
        if is_t(m) and m.device != getattr(engine, "device", None):
            raise ValueError("utts[%d]: m_mag_mel_log is on %s, the engine runs on %s"
                             % (i, m.device, getattr(engine, "device", None)))
    if any(is_t(l) for l in lf0s):
        r, shifts = _griffin_lim_from_mag_tables(engine.lf0_to_host(lf0s), fs, N, b_const_rate)
    torch = __import__("torch")
    H = N // 2 + 1
    n_rows = int(sum(int(m.shape[0]) for m in mags))
    sizes = [int(v.size) for v in shifts]
    F = int(sum(sizes))
    a_mag = engine.empty((n_rows, mag_dim))
    if any(is_t(m) for m in mags):
        engine.pack_rows([mags], [a_mag])
    else:
        a_mag.copy_(torch.from_numpy(np.concatenate([np.asarray(m, dtype=np.float32) for m in mags])))
    if b_fbank_mel:
        u_mag = engine.constant(("u_mag_fbank", mag_dim, H, float(alpha)), lambda: hm.unwarp_fbank_matrix(mag_dim, H, alpha))
    else:
        u_mag = engine.constant(("u_mag", mag_dim, H, float(alpha)), lambda: hm.unwarp_matrix(mag_dim, H, alpha))
    # the unwarp's two phase jobs run on one zero column each; their outputs are the rows the fold overwrites afterwards
    u_zero = engine.constant(("u_zero", 1, H), lambda: np.zeros((1, H)))
    zcol = torch.zeros((n_rows, 1), dtype=torch.float32, device=engine.device)
    ld = int(engine.lib.mpx_spec_ld(H))
    dev = lambda: engine.empty((max(F, 1), ld))[:F, :H]   # noqa: E731
    tgt, i_mag, i_re, i_im = dev(), dev(), dev(), dev()
    if b_const_rate:
        row0 = np.asarray(r["row0"])
        CompressedSynthesisPlan._check_rows_for_tiles(row0, np.asarray(r["row1"]))
        t = engine.to_device_packed([
            ("row0", row0, np.int32), ("row1", r["row1"], np.int32), ("rowt", r["rowt"], np.float32),
            ("tile_first", np.searchsorted(row0, 31 * np.arange((n_rows + 30) // 31 + 1), side="left"), np.int32)])
        engine.launch("mpx_mel_unwarp_rows", F, H, a_mag, mag_dim, u_mag, tgt, zcol, zcol, 1, u_zero, i_re, i_im, ld,
                      t["row0"], t["row1"], t["rowt"], n_rows, t["tile_first"], None, 0)
    else:
        if F != n_rows:
            raise RuntimeError("griffin_lim_from_mag: %d frames for %d variable-rate rows" % (F, n_rows))
        engine.launch("mpx_mel_unwarp", n_rows, H, a_mag, mag_dim, u_mag, tgt, zcol, zcol, 1, u_zero, i_re, i_im, ld)
    for _ in utts:
        print('Starting Griffin-Lim. It could take a while...')
    out = _griffin_lim_device_rows(engine, tgt, sizes, shifts, [phase_init] * len(utts), N, niters, return_device,
                                   init_rows=(i_mag, i_re, i_im))
    return [sig for sig, _phase in out]


def griffin_lim_from_mag(m_mag_mel_log, v_lf0, fs, fft_len=None, phase_init='min_phase', niters=30, b_const_rate=False,
                         b_fbank_mel=False):
    """One utterance of griffin_lim_from_mag_batch: the float64 signal."""
    return griffin_lim_from_mag_batch([(m_mag_mel_log, v_lf0)], fs, fft_len=fft_len, phase_init=phase_init,
                                      niters=niters, b_const_rate=b_const_rate, b_fbank_mel=b_fbank_mel)[0]


def copy_synthesis_lossless(wav_file, fft_len=None):
    """analysis_lossless(wav_file) + synthesis_from_lossless of its result in one launch: returns
    ((m_mag, m_real, m_imag, v_f0, fs, v_shift), v_syn_sig)."""
    v_sig, fs = la.read_audio_file(wav_file)
    v_pm_sec, v_voi = _epochs_for(wav_file)
    return copy_synthesis_lossless_batch([(v_sig, fs, v_pm_sec, v_voi)], fft_len=fft_len)[0]


# ======================================================================================================
# compressed-feature synthesis
# ======================================================================================================
def post_filter(m_mag_mel_log, fs, av_len_at_zero=None, av_len_at_nyq=None, boost_at_zero=None, boost_at_nyq=None):
    """
    magphase.py:2300-2378 (Q20).  [F x 60] float64 on the host, vectorised over frames: 0.5 KB per frame, not worth
    a kernel launch.  Same defaults, warnings and ValueError as the reference.
    """
    m_mag_mel_log = np.asarray(m_mag_mel_log, dtype=np.float64)
    nfrms, mag_dim = m_mag_mel_log.shape
    if mag_dim != 60:
        warnings.warn('Post-filter: It has been only tested with 60 dimensional mag data. '
                      'If you use another dimension, the result may be suboptimal.')
    opts = [av_len_at_zero, av_len_at_nyq, boost_at_zero, boost_at_nyq]
    if fs == 48000:
        defaults = [hm.round_to_int(11.0 * (mag_dim / 60.0)), hm.round_to_int(3.0 * (mag_dim / 60.0)), 1.8, 2.0]
    elif fs == 16000:
        if any(o is None for o in opts):
            warnings.warn('Post-filter: The default parameters for 16kHz sample rate have not being tunned.')
        defaults = [hm.round_to_int(9.0 * (mag_dim / 60.0)), hm.round_to_int(12.0 * (mag_dim / 60.0)), 2.0, 1.6]
    else:
        if any(o is None for o in opts):
            raise ValueError('Post-filter: It has only been tested with 16kHz and 48kHz sample rates.'
                             '\nProvide your own values for the options: av_len_at_zero, av_len_at_nyq, '
                             'boost_at_zero,\nboost_at_nyq if you use another sample rate')
        defaults = opts
    av0, avn, b0, bn = [d if o is None else o for o, d in zip(opts, defaults)]
    v_nx = np.arange(np.floor(av0 / 2), mag_dim - np.floor(avn / 2)).astype(int)
    v_lens = (2 * np.ceil(np.linspace(av0, avn, v_nx.size) / 2) - 1).astype(int)
    half = v_lens // 2
    m_ave = np.zeros((nfrms, mag_dim))
    for j, nxb in enumerate(v_nx):
        m_ave[:, nxb] = np.mean(m_mag_mel_log[:, nxb - half[j]:nxb + half[j] + 1], axis=1)
    m_ave[:, :v_nx[0]] = m_ave[:, [v_nx[0]]]
    m_ave[:, v_nx[-1]:] = m_ave[:, [v_nx[-1]]]
    m_enh = (m_mag_mel_log - m_ave) * np.linspace(b0, bn, mag_dim)[None, :] + m_ave
    m_enh[:, 0] = m_mag_mel_log[:, 0]
    m_enh[:, -1] = m_mag_mel_log[:, -1]
    return m_enh


def post_filter_merlin(m_mag_mel_log, fs, pf_coef=1.4):
    """
    magphase.py:3375-3465: Merlin / HTS style formant enhancement of the log mel magnitudes.  The reference pipes the
    frames through nine SPTK-3.9 binaries; the same arithmetic is restated here on the host in float64 with a float32
    rounding at every pipe boundary (SPTK's stream format) -- **parity unpinned**: neither SPTK nor any reference
    output of this branch exists in the build container, the checks in tests/test_post_filter_merlin.py are
    known-answer properties (pf_coef = 1 is the identity of the cepstral round trip; the frame energy r0 is kept).
      mcep   = rceps(mag, 'log', 'compact')                           -> temp.mcep (float32)
      r0     = c2acr_0(freqt_{alpha->0, 2047}(mcep)),  p_r0 = the same of mcep * lifter, lifter = (1, 1, pf, pf, ...)
      b      = mc2b(mcep * lifter, alpha);  b0 += ln(r0 / p_r0) / 2;  mcep_pf = b2mc(b, alpha)
      out    = cosine-matrix log spectrum of mcep_pf on mag_dim points (alpha = 0), NaN -> la.MAGIC
    Host-side on purpose: [F x 60] per utterance, a few matrix products.
    """
    fft_len = 4096
    minph_ord = fft_len // 2 - 1
    alpha = define_alpha(fs)
    ncoeffs = np.shape(m_mag_mel_log)[1]
    m_mcep = hm._f32(hm.rceps_compact(m_mag_mel_log))
    v_lifter = hm._f32(np.concatenate(([1.0, 1.0], np.full(ncoeffs - 2, float("%1.2f" % pf_coef)))))
    m_mcep_w = hm._f32(m_mcep * v_lifter)                                    # vopr -m
    v_r0 = hm._f32(hm.sptk_c2acr_r0(hm._f32(hm.sptk_freqt(m_mcep, minph_ord, alpha)), fft_len))
    v_p_r0 = hm._f32(hm.sptk_c2acr_r0(hm._f32(hm.sptk_freqt(m_mcep_w, minph_ord, alpha)), fft_len))
    m_b = hm._f32(hm.sptk_mc2b(m_mcep_w, alpha))
    with np.errstate(divide="ignore", invalid="ignore"):
        v_p_b0 = hm._f32(hm._f32(np.log(hm._f32(v_r0 / v_p_r0)) / 2.0) + m_b[:, 0])   # vopr -d | sopr -LN -d 2 | vopr -a
    m_b[:, 0] = v_p_b0                                                       # bcp 1..order | merge
    m_mcep_pf = hm._f32(hm.sptk_b2mc(m_b, alpha))
    m_out = hm.cos_matrix_log_spectrum(m_mcep_pf, ncoeffs)
    m_out[np.isnan(m_out)] = la.MAGIC
    return m_out


def post_filter_merlin_device(m_mag_mel_log, fs, pf_coef=1.4, engine=None):
    """post_filter_merlin on the device (mpx_post_filter_merlin): the same chain in float32 for all frames at once --
    what iobatch.generate_waveforms_corpus(pf_type='merlin') and synthesis_from_compressed_batch(b_post_filter='merlin')
    run.  Host array in, float64 array out; differs from the host form by float32 rounding (tests: -m gpu)."""
    engine = engine or get_engine()
    x = engine.to_device(np.atleast_2d(np.asarray(m_mag_mel_log)), np.float32)
    return engine.to_host_f64(engine.post_filter_merlin(x, fs, pf_coef=pf_coef))


def post_filter_batch(mats, fs, pf_type='magphase', pf_coef=1.4, av_len_at_zero=None, av_len_at_nyq=None,
                      boost_at_zero=None, boost_at_nyq=None, engine=None, return_device=False):
    """
    The post-filter as a stage of its own on the device, for a whole batch: pf_type 'magphase' = post_filter
    (k_post_filter), 'merlin' = post_filter_merlin (mpx_post_filter_merlin), one forward launch sequence over all frames.
    mats: list of [F_i x D] log-mel magnitude matrices, each a host array or a tensor on the engine's device (float16 /
    bfloat16 / float32 / float64, any row stride -- column slices of a wider tensor are read where they lie: one
    mpx_rows_pack launch gathers them into float32 rows).  F_i = 0 and an empty list are legal.
    Returns a list of [F_i x D] float64 arrays (return_device: float32 device tensors, row views of one buffer); the
    values are Engine.post_filter's / Engine.post_filter_merlin's on the packed float32 rows, bit for bit -- what
    synthesis_from_compressed_batch(b_post_filter=True / 'merlin') filters its magnitudes with.
    ValueError: a pf_type other than 'magphase' / 'merlin'; av_len_at_zero / av_len_at_nyq / boost_at_zero / boost_at_nyq
    given with 'merlin' or a pf_coef other than 1.4 with 'magphase' (each option belongs to one filter); D outside 3..64
    ('merlin') or 3..256 ('magphase'); matrices that are not 2-D or differ in D -- all before any launch.  The sample-rate
    defaults, the warnings and the ValueError of 'magphase' are hostmath.post_filter_tables'.
    Autograd: with return_device, grad mode on and a device matrix that requires grad, the results carry a grad_fn
    (autograd._PostFilter) and backward() gives each matrix a gradient in its own dtype and shape, computed by
    k_post_filter_bwd / mpx_post_filter_merlin_backward; the forward values are the same bits
    either way.  A 'merlin' row whose output is la.MAGIC gets a zero gradient.  Not differentiable: fs, pf_coef and the
    four av_* / boost_* options; no double backward.  Under grad the 'magphase' tables must hold no negative half length
    (D = 3 with the 48 kHz defaults does: ValueError).
    Composition: mlpg_streams_batch -> post_filter_batch -> synthesis_from_compressed_batch / synthesis_from_mag_batch with
    b_post_filter=False carries a waveform loss through the filter to the acoustic model's means.
    """
    if pf_type not in ('magphase', 'merlin'):
        raise ValueError("post_filter_batch: pf_type must be 'magphase' or 'merlin', not %r" % (pf_type,))
    if isinstance(mats, np.ndarray) or not isinstance(mats, (list, tuple)):
        raise ValueError("post_filter_batch: mats must be a list of [frames x D] matrices")
    opts = dict(av_len_at_zero=av_len_at_zero, av_len_at_nyq=av_len_at_nyq, boost_at_zero=boost_at_zero,
                boost_at_nyq=boost_at_nyq)
    opts = {k: v for k, v in opts.items() if v is not None}
    if pf_type == 'merlin':
        if opts:
            raise ValueError("post_filter_batch: %s belong to pf_type='magphase'" % ", ".join(sorted(opts)))
        opts = dict(pf_coef=float(pf_coef))
    elif float(pf_coef) != 1.4:
        raise ValueError("post_filter_batch: pf_coef belongs to pf_type='merlin'")
    mats = list(mats)
    if not mats:
        return []
    for i, m in enumerate(mats):
        if not hasattr(m, "shape"):
            mats[i] = m = np.asarray(m)
        if len(m.shape) != 2:
            raise ValueError("post_filter_batch: mats[%d] must be a 2-D [frames x D] matrix" % i)
    D = int(mats[0].shape[1])
    if any(int(m.shape[1]) != D for m in mats):
        raise ValueError("post_filter_batch: every matrix must have the same number of columns")
    d_max = 64 if pf_type == 'merlin' else 256
    if not 3 <= D <= d_max:
        raise ValueError("post_filter_batch: pf_type=%r needs 3 <= D <= %d, not %d" % (pf_type, d_max, D))
    if pf_type == 'magphase':
        hm.post_filter_tables(D, fs, **opts)   # the reference's warnings and its ValueError, before any launch
    engine = engine or get_engine()
    import torch

    wants_grad = hm.wants_grad(return_device, mats)
    total = int(sum(int(m.shape[0]) for m in mats))
    if total == 0:
        out = torch.zeros((0, D), dtype=torch.float32, device=engine.device)
        offs = np.zeros(len(mats) + 1, dtype=np.int64)
    else:
        with warnings.catch_warnings():   # (the tables' warnings were given above)
            warnings.simplefilter("ignore")
            if wants_grad:
                from . import autograd

                out, offs = autograd.post_filter(engine, mats, pf_type, fs, opts)
            else:
                x, offs = engine.post_filter_pack(mats)
                out = engine.post_filter_merlin(x, fs, **opts) if pf_type == 'merlin' else engine.post_filter(x, fs, **opts)
    if not return_device:
        out = engine.to_host_f64(out) if total else np.zeros((0, D))
    return [out[int(a):int(b)] for a, b in zip(offs[:-1], offs[1:])]


def post_filter_device(m_mag_mel_log, fs, **kw):
    """post_filter_batch for one matrix ([F x D] in, [F x D] out; kw as post_filter_batch's)."""
    return post_filter_batch([m_mag_mel_log], fs, **kw)[0]


def _output_hpf(v_syn_sig, fs):
    """magphase.py:981-995: 4th-order Butterworth high-pass at 40 Hz, float64 on the host (poles at |z|~0.997)."""
    from scipy import signal

    v_b, v_a = signal.butter(4, 40 / (fs / 2.0), btype='highpass')
    return signal.lfilter(v_b, v_a, v_syn_sig)


def synthesis_from_compressed_batch(utts, fs, fft_len=None, b_voi_ap_win=True, b_const_rate=False, alpha_phase=None,
                                    b_out_hpf=True, noise=None, engine=None, per_phase_type='magphase',
                                    b_post_filter=False, b_fbank_mel=False, noise_mode='reference', noise_seeds=None,
                                    pcm16_norm=False, async_out=False, defer_rng=False, prepared=None,
                                    return_device=False):
    """Batched synthesis_from_compressed; utts: list of (m_mag_mel_log, m_real_mel, m_imag_mel, v_lf0).
    Device features: the three matrices may be torch tensors on the engine's device (an acoustic model's output) --
    float32 / float16 / bfloat16 / float64, any row stride (column slices of one [F x 151] tensor are read where they
    lie, a non-unit column stride is made contiguous first); they are gathered on the device (Engine.pack_rows,
    mpx_rows_pack), not staged through the host.  v_lf0 may be a device tensor too (not float16): the lf0 vectors of the
    batch come down in one copy, the frame tables are host arithmetic.  CPU tensors are treated as host arrays; tensors
    of another device, integer / bool / complex tensors and `prepared` together with tensors raise ValueError.  Host
    arrays mixed into a device batch are uploaded one by one (slow).
    return_device: the signals stay on the device -- a list of per-utterance views of the PCM buffer: float64 after the
    output high-pass, float32 without it, int16 with pcm16_norm.  Not with async_out.
    Streams: every launch goes to torch's CURRENT stream of the engine's device; inputs produced on that stream and
    outputs consumed on it need no further synchronisation.
    defer_rng: reference noise only -- numpy's advanced generator state stays on the device between calls; the caller owes
    engine.mt_sync() before numpy's global generator is used again (iobatch does this for a corpus run).
    async_out (with pcm16_norm): returns (signals, ticket) -- the int16 signals are views of a page-locked buffer the
    device is still copying into; ticket.wait() before reading them, ticket.release() when done (engine.HostTicket).
    b_post_filter: apply a post-filter to the log-mel magnitudes on the device first: True / 'magphase' = the MagPhase
    post-filter (pf_type='magphase'), 'merlin' = the Merlin-style one (pf_type='merlin', mpx_post_filter_merlin).
    noise_mode: 'reference' (default) draws the aperiodic source from numpy's global RNG like magphase.py:883;
    'device' generates it on the GPU (Philox, one uint64 seed per utterance in noise_seeds, default 0, 1, ...): same
    distribution, not the reference's sample values, independent of batching and sharding.
    pcm16_norm: False (default) returns float64 signals; a number (la.write_audio_file's norm, 0.98) or None returns
    the int16 samples la.write_audio_file(..., norm=pcm16_norm) would store, converted on the device (mpx_pcm16).
    prepared: the host side of THIS batch built ahead of time (engine.prepare_async("synthesis", utts, fs, fft_len=...,
    b_voi_ap_win=..., b_const_rate=...).result(): the planner thread prepares launch i + 1 while this thread enqueues
    launch i; None: prepared here).
    Autograd: with return_device, grad mode on and a device m_mag_mel_log / m_real_mel / m_imag_mel that requires grad,
    the signals carry a grad_fn and tensor.backward() reaches the three coefficient matrices, in each one's own dtype and
    shape (magphase_amd/autograd.py; the forward launches and their samples are the same).  At
    both frame rates, with and without b_out_hpf / b_voi_ap_win / b_fbank_mel, for either noise_mode or an explicit noise.
    Not differentiable: v_lf0 (integer pitch marks and the voicing flag), fs, the noise and its two gains.
    NotImplementedError, naming the argument, for per_phase_type 'min_phase' / 'linear', a truthy b_post_filter,
    pcm16_norm other than False and prepared=.  MAGPHASE_NOISE_SPECTRA=store is ignored by the backward pass (it
    recomputes the noise spectra).  No double backward."""
    if return_device and async_out:
        raise ValueError("return_device and async_out exclude each other (async_out is a download)")
    want_grad = hm.wants_grad(return_device, [x for u in utts for x in u[:3]])   # (CPU tensors take the host path)
    if want_grad:   # what has no backward pass says so before anything is built
        if per_phase_type in ('min_phase', 'linear'):
            raise NotImplementedError("per_phase_type=%r has no backward pass: only 'magphase' is differentiable"
                                      % (per_phase_type,))
        if b_post_filter and b_post_filter != 'no':
            raise NotImplementedError("b_post_filter=%r has no backward pass" % (b_post_filter,))
        if pcm16_norm is not False:
            raise NotImplementedError("pcm16_norm=%r (int16 output) has no backward pass" % (pcm16_norm,))
        if prepared is not None:
            raise NotImplementedError("prepared= (built from host arrays) has no backward pass")
    checked, _on_dev = _tensor_inputs(utts, _SYN_NAMES, lf0_at=3)
    if checked is not utts and prepared is not None:
        raise ValueError("prepared= was built from host arrays: it cannot be combined with tensor inputs")
    utts = checked
    engine = engine or get_engine()
    plan = CompressedSynthesisPlan(engine, utts, fs, fft_len=fft_len, b_voi_ap_win=b_voi_ap_win,
                                   b_const_rate=b_const_rate, alpha_phase=alpha_phase, noise=noise,
                                   per_phase_type=per_phase_type, post_filter=b_post_filter, b_fbank_mel=b_fbank_mel,
                                   noise_mode=noise_mode, noise_seeds=noise_seeds, defer_rng=defer_rng, prepared=prepared)
    if want_grad:   # the same launches inside a torch.autograd.Function (magphase_amd/autograd.py)
        from .autograd import synthesize_compressed

        pcm_dev = synthesize_compressed(plan, b_out_hpf, utts)
        return [pcm_dev[int(plan.out_off_host[u]):int(plan.out_off_host[u + 1])] for u in range(len(utts))]
    pcm_dev = plan.run()
    if b_out_hpf:   # magphase.py:981-995, float64 on the device (engine.output_hpf); _output_hpf is the host form
        pcm_dev = engine.output_hpf(pcm_dev, plan.out_off_host, fs)
    if return_device:
        if pcm16_norm is not False:
            pcm_dev = engine.output_pcm16(pcm_dev, plan.out_off_host, norm=pcm16_norm, return_device=True)
        return [pcm_dev[int(plan.out_off_host[u]):int(plan.out_off_host[u + 1])] for u in range(len(utts))]
    if pcm16_norm is not False and async_out:
        pcm, ticket = engine.output_pcm16(pcm_dev, plan.out_off_host, norm=pcm16_norm, async_out=True)
        return [pcm[plan.out_off_host[u]:plan.out_off_host[u + 1]] for u in range(len(utts))], ticket
    if async_out:
        raise ValueError("async_out needs pcm16_norm")
    if pcm16_norm is not False:
        pcm = engine.output_pcm16(pcm_dev, plan.out_off_host, norm=pcm16_norm)
    elif b_out_hpf:
        pcm = pcm_dev.cpu().numpy()
    else:
        pcm = engine.to_host_f64(pcm_dev)
    return [pcm[plan.out_off_host[u]:plan.out_off_host[u + 1]] for u in range(len(utts))]


def synthesis_from_compressed(m_mag_mel_log, m_real_mel, m_imag_mel, v_lf0, fs, fft_len=None, b_voi_ap_win=True,
                              b_fbank_mel=False, b_const_rate=False, per_phase_type='magphase', alpha_phase=None,
                              b_out_hpf=True):
    """magphase.py:825-997, per_phase_type in {'magphase', 'min_phase', 'linear'}; b_fbank_mel: magnitudes unwarped by
    the filter-bank interpolation (la.sp_mel_unwarp_fbank) instead of the cepstral cosine matrix."""
    return synthesis_from_compressed_batch([(m_mag_mel_log, m_real_mel, m_imag_mel, v_lf0)], fs, fft_len=fft_len,
                                           b_voi_ap_win=b_voi_ap_win, b_const_rate=b_const_rate,
                                           alpha_phase=alpha_phase, b_out_hpf=b_out_hpf,
                                           per_phase_type=per_phase_type, b_fbank_mel=b_fbank_mel)[0]


_MAG_NAMES = ("m_mag_mel_log", "v_lf0")


def synthesis_from_mag_batch(utts, fs, fft_len=None, phase='min_phase', b_voi_ap_win=True, b_const_rate=False,
                             b_out_hpf=True, noise=None, engine=None, b_post_filter=False, b_fbank_mel=False,
                             noise_mode='reference', noise_seeds=None, pcm16_norm=False, return_device=False):
    """Batched synthesis from the magnitudes alone; utts: list of (m_mag_mel_log, v_lf0).  phase: 'min_phase' -- the
    periodic component takes the complex-cepstrum minimum phase of the unwarped magnitude (per_phase_type='min_phase',
    magphase.py:937-938) -- or 'zero' (per_phase_type='linear', magphase.py:933-936); ValueError otherwise.  The samples
    are those of synthesis_from_compressed_batch with that per_phase_type, whatever phase matrices it is given, bit for
    bit.  Every other argument as synthesis_from_compressed_batch takes it: host arrays or device tensors (float32 /
    float16 / bfloat16 / float64, any row stride; column slices are read where they lie), return_device, pcm16_norm,
    noise / noise_mode / noise_seeds, b_post_filter, b_fbank_mel.
    Autograd: with return_device, grad mode on and a device m_mag_mel_log that requires grad, the signals carry a grad_fn
    and tensor.backward() reaches m_mag_mel_log, in its own dtype and shape (magphase_amd/autograd.py, DESIGN.md section
    3.3o: k_synth_comp_bwd, k_min_phase_bwd, k_rows_lerp_adjoint, k_mel_unwarp_bwd; through the output high-pass'
    adjoint with b_out_hpf).  The forward launches and their samples are the same.  Not differentiable: v_lf0, fs, the
    noise and its gains.  NotImplementedError, naming the argument, for a truthy b_post_filter or pcm16_norm under grad
    and for mag_dim > 64.  No double backward."""
    if phase not in ('min_phase', 'zero'):
        raise ValueError("phase must be 'min_phase' or 'zero', not %r" % (phase,))
    utts = [tuple(u) for u in utts]
    if any(len(u) != 2 for u in utts):
        raise ValueError("utts: a list of (m_mag_mel_log, v_lf0)")
    want_grad = hm.wants_grad(return_device, [u[0] for u in utts])
    if want_grad:   # what has no backward pass says so before anything is built
        if b_post_filter and b_post_filter != 'no':
            raise NotImplementedError("b_post_filter=%r has no backward pass" % (b_post_filter,))
        if pcm16_norm is not False:
            raise NotImplementedError("pcm16_norm=%r (int16 output) has no backward pass" % (pcm16_norm,))
        for i, u in enumerate(utts):
            if len(np.shape(u[0])) == 2 and int(np.shape(u[0])[1]) > 64:
                raise NotImplementedError("utts[%d]: m_mag_mel_log (mag_dim) has %d columns: the backward pass takes at "
                                          "most 64" % (i, int(np.shape(u[0])[1])))
    utts, _on_dev = _tensor_inputs(utts, _MAG_NAMES, lf0_at=1)
    engine = engine or get_engine()
    plan = MagnitudeSynthesisPlan(engine, utts, fs, fft_len=fft_len, phase=phase, b_voi_ap_win=b_voi_ap_win,
                                  b_const_rate=b_const_rate, noise=noise, post_filter=b_post_filter,
                                  b_fbank_mel=b_fbank_mel, noise_mode=noise_mode, noise_seeds=noise_seeds)
    cut = lambda x: [x[int(plan.out_off_host[u]):int(plan.out_off_host[u + 1])] for u in range(len(utts))]
    if want_grad:   # the same launches inside a torch.autograd.Function (magphase_amd/autograd.py)
        from .autograd import synthesize_from_mag

        return cut(synthesize_from_mag(plan, b_out_hpf, utts))
    pcm_dev = plan.run()
    if b_out_hpf:
        pcm_dev = engine.output_hpf(pcm_dev, plan.out_off_host, fs)
    if return_device:
        if pcm16_norm is not False:
            pcm_dev = engine.output_pcm16(pcm_dev, plan.out_off_host, norm=pcm16_norm, return_device=True)
        return cut(pcm_dev)
    if pcm16_norm is not False:
        pcm = engine.output_pcm16(pcm_dev, plan.out_off_host, norm=pcm16_norm)
    elif b_out_hpf:
        pcm = pcm_dev.cpu().numpy()
    else:
        pcm = engine.to_host_f64(pcm_dev)
    return cut(pcm)


def synthesis_from_mag(m_mag_mel_log, v_lf0, fs, fft_len=None, phase='min_phase', b_voi_ap_win=True, b_fbank_mel=False,
                       b_const_rate=False, b_out_hpf=True):
    """synthesis_from_compressed without transmitted phase: one utterance of synthesis_from_mag_batch."""
    return synthesis_from_mag_batch([(m_mag_mel_log, v_lf0)], fs, fft_len=fft_len, phase=phase,
                                    b_voi_ap_win=b_voi_ap_win, b_const_rate=b_const_rate, b_out_hpf=b_out_hpf,
                                    b_fbank_mel=b_fbank_mel)[0]


def synthesis_from_acoustic_modelling(in_feats_dir, filename_token, out_syn_dir, mag_dim, phase_dim, fs,
                                      fft_len=None, pf_type='no', b_const_rate=False):
    """magphase.py:3229-3275."""
    print("\nSynthesising file: " + filename_token + '.wav............................')
    m_mag_mel_log = lu.read_binfile(in_feats_dir + '/' + filename_token + '.mag', dim=mag_dim)
    m_real_mel = lu.read_binfile(in_feats_dir + '/' + filename_token + '.real', dim=phase_dim)
    m_imag_mel = lu.read_binfile(in_feats_dir + '/' + filename_token + '.imag', dim=phase_dim)
    v_lf0 = lu.read_binfile(in_feats_dir + '/' + filename_token + '.lf0', dim=1)
    if pf_type == 'magphase':
        print('Using MagPhase postfilter...')
        m_mag_mel_log = post_filter(m_mag_mel_log, fs)
    elif pf_type == 'merlin':
        # the device form, as iobatch.generate_waveforms_corpus(pf_type='merlin') runs it: one pf_type, one result whichever
        # entry point writes the wav (post_filter_merlin, the float64 host chain, stays the array API)
        print('Using Merlin postfilter...')
        m_mag_mel_log = post_filter_merlin_device(m_mag_mel_log, fs)
    elif pf_type == 'no':
        print('No postfilter...')
    v_syn_sig = synthesis_from_compressed(m_mag_mel_log, m_real_mel, m_imag_mel, v_lf0, fs, fft_len=fft_len,
                                          b_const_rate=b_const_rate)
    la.write_audio_file(out_syn_dir + '/' + filename_token + '.wav', v_syn_sig, fs)
    return


# ======================================================================================================
# compressed-feature analysis
# ======================================================================================================
def analysis_compressed_batch(utts, fft_len=None, mag_dim=60, phase_dim=10, b_const_rate=False, alpha_phase=None,
                              engine=None, as_float32=False, async_out=False, prepared=None, return_device=False):
    """
    Batched magphase.py:2947-2988 for utterances with epochs: utts = list of (v_sig, fs, v_pm_sec, v_voi), one
    sample rate per call.  Lossless analysis (k_analysis) stays on the device; the mel warp runs on it directly.
    Returns a list of (m_mag_mel_log, m_real_mel, m_imag_mel, v_lf0_smth, v_shift, fs, fft_len).
    async_out (with as_float32): returns (list, ticket) -- the three matrices are views of a page-locked buffer the device
    is still copying into; ticket.wait() before reading them, ticket.release() when done (engine.HostTicket).
    prepared: the host side of THIS batch built ahead of time (engine.prepare_async("analysis", utts, fft_len).result():
    the planner thread prepares launch i + 1 while this thread enqueues launch i; None: prepared here).
    return_device: the three matrices stay on the device -- float32 row views of the plan's output (the values
    as_float32 downloads), for a training loop that extracts features on the fly; v_lf0_smth, v_shift, fs and fft_len are
    host values as always.  Not with async_out.  The launches go to torch's CURRENT stream of the engine's device: work
    that consumes the matrices on that stream needs no further synchronisation.
    v_sig may be a 1-D torch tensor on the engine's device (float32 / float16 / bfloat16 / float64, any element stride), as
    for analysis_lossless_batch: the samples stay on the device, and the rows equal those of the host-array call on the
    same float32 samples bit for bit.  Not with prepared= (built from host arrays).
    Autograd: with return_device, grad mode on and a device v_sig that requires grad, m_mag_mel_log / m_real_mel /
    m_imag_mel carry a grad_fn and tensor.backward() reaches v_sig, at both frame rates (magphase_amd/autograd.py,
    DESIGN.md section 3.3j; the forward launch and its values are the same).  The gradient of a phase coefficient that
    sits on the clip at +-1 is defined as zero.  Not differentiable: v_pm_sec, v_voi and fs; v_lf0_smth and v_shift carry
    no grad_fn; no double backward.
    """
    if return_device and async_out:
        raise ValueError("return_device and async_out exclude each other (async_out is a download)")
    engine = engine or get_engine()
    if len(utts) == 0:   # nothing to do (the per-utterance loop of the reference would run zero times)
        from .engine import HostTicket

        return ([], HostTicket(None, None, None, None)) if async_out else []
    plan = CompressedAnalysisPlan(engine, utts, fft_len=fft_len, mag_dim=mag_dim, phase_dim=phase_dim,
                                  b_const_rate=b_const_rate, alpha_phase=alpha_phase, prepared=prepared)
    for lens in plan.lossless.long_frame_lens:
        for n in lens:
            warnings.warn(_WARN_LONG % (plan.fft_len, n))
    # as_float32: the device's float32 values as they are (what the feature files store), no widening to float64
    ticket = None
    if async_out:
        if not as_float32:
            raise ValueError("async_out needs as_float32")
        (h_mag, h_real, h_imag), ticket = engine.to_host_f32_async(list(plan.run()))
    elif return_device:
        h_mag, h_real, h_imag = _run_compressed_analysis(plan, utts)
    else:
        h_mag, h_real, h_imag = ((engine.to_host_f32 if as_float32 else engine.to_host_f64)(t_) for t_ in plan.run())
    res = []
    try:
        # signal.medfilt of every utterance's f0 in one pass (hostmath.medfilt3_batch: bit-identical, also for 0 or 1
        # vectors; 30 us per scipy call)
        med_flat = None if b_const_rate else getattr(plan.lossless, "f0_med_flat", None)
        if med_flat is not None:   # the native planner already holds f0 and its median-3 for the whole batch
            f0_flat = plan.f0_out.flat
            lf0_cat = la.f0_to_lf0((f0_flat > 0).astype('float') * med_flat)   # magphase.py:2499-2501
            off = np.asarray(plan.out_off).tolist()
        else:
            f0_med = hm.medfilt3_batch(plan.f0_out)
            # lf0 of the whole batch in one pass (la.f0_to_lf0 per utterance: the same element-wise operations)
            sizes = [int(np.size(f)) for f in plan.f0_out]
            lf0_cat = la.f0_to_lf0((np.concatenate(plan.f0_out) > 0).astype('float') * np.concatenate(f0_med)) if sizes else np.zeros(0)  # magphase.py:2499-2501
            off = np.concatenate(([0], np.cumsum(sizes))).tolist()
        o_off = np.asarray(plan.out_off).tolist()
        shifts = plan.lossless.v_shift
        for u in range(len(utts)):
            a, b = o_off[u], o_off[u + 1]
            v_lf0 = lf0_cat[off[u]:off[u + 1]].copy()
            res.append((h_mag[a:b], h_real[a:b], h_imag[a:b], v_lf0, shifts[u].astype(int), plan.fs, plan.fft_len))
    except BaseException:
        if ticket is not None:   # the page-locked slot goes back to the ring when the host part fails
            ticket.release()
        raise
    return (res, ticket) if async_out else res


def _run_compressed_analysis(plan, utts):
    """plan.run() -> the batch's three float32 device matrices, for return_device.  Through autograd.analyze_compressed --
    the same launch inside a torch.autograd.Function -- under hostmath.wants_grad's rule for the v_sig (a CPU tensor is a
    host array to the plan; a prepared= batch was built from host arrays)."""
    if hm.wants_grad(True, [u[0] for u in utts]):
        from .autograd import analyze_compressed

        return analyze_compressed(plan, [u[0] for u in utts])
    return plan.run()


def format_for_modelling(m_mag, m_real, m_imag, v_f0, fs, mag_dim=60, phase_dim=45, b_mag_fbank_mel=False,
                         alpha_phase=None):
    """
    magphase.py:2490-2544 for lossless features that are already in host arrays: f0 smoothing / lf0 on the host (fp64),
    the two mel warps on the device (mpx_mel_warp).  Returns (m_mag_mel_log, m_real_mel, m_imag_mel, v_lf0_smth).
    b_mag_fbank_mel=True: the magnitudes go through the mel filter bank (la.sp_mel_warp_fbank, magphase.py:2504-2505;
    mpx_mel_warp_fbank) instead of the cepstral warp.  In the reference this branch is reachable only through this
    function (analysis_compressed never forwards the flag, Q7).
    """
    from scipy import signal
    engine = get_engine()
    v_f0 = np.asarray(v_f0, dtype=np.float64)
    v_voi = (v_f0 > 0).astype('float')                                       # magphase.py:2497
    v_lf0_smth = la.f0_to_lf0(v_voi * signal.medfilt(v_f0))                  # :2499-2501
    mag, real, imag = (engine.feats_to_device(x) for x in (m_mag, m_real, m_imag))
    out = engine.mel_warp_feats(mag, real, imag, v_voi, fs, mag_dim, phase_dim, alpha_phase=alpha_phase,
                                b_mag_fbank_mel=bool(b_mag_fbank_mel))
    return tuple(engine.to_host_f64(t) for t in out) + (v_lf0_smth,)


shift_to_f0 = hm.shift_to_f0
get_num_full_mel_coeffs_from_num_phase_coeffs = hm.get_num_full_mel_coeffs_from_num_phase_coeffs


def analysis_compressed(wav_file, fft_len=None, mag_dim=60, phase_dim=10, b_const_rate=False, b_mag_fbank_mel=False,
                        alpha_phase=None):
    """magphase.py:2947-2988 (b_mag_fbank_mel is accepted and, as in the reference, never forwarded)."""
    v_sig, fs = la.read_audio_file(wav_file)
    v_pm_sec, v_voi = _epochs_for(wav_file)
    return analysis_compressed_batch([(v_sig, fs, v_pm_sec, v_voi)], fft_len=fft_len, mag_dim=mag_dim,
                                     phase_dim=phase_dim, b_const_rate=b_const_rate, alpha_phase=alpha_phase)[0]


def analysis_for_acoustic_modelling(wav_file, out_dir, fft_len=None, mag_dim=60, phase_dim=10, b_const_rate=False,
                                    b_mag_fbank_mel=False, alpha_phase=None):
    """magphase.py:2992-3022, including Q7: alpha_phase=b_mag_fbank_mel is what the reference forwards (:3010)."""
    m_mag_mel_log, m_real_mel, m_imag_mel, v_lf0_smth, v_shift, fs, fft_len = analysis_compressed(
        wav_file, fft_len=fft_len, mag_dim=mag_dim, phase_dim=phase_dim, b_const_rate=b_const_rate,
        b_mag_fbank_mel=b_mag_fbank_mel, alpha_phase=b_mag_fbank_mel)
    file_id = os.path.basename(wav_file).split(".")[0]
    write_featfile(m_mag_mel_log, out_dir, file_id + '.mag')
    write_featfile(m_real_mel, out_dir, file_id + '.real')
    write_featfile(m_imag_mel, out_dir, file_id + '.imag')
    write_featfile(v_lf0_smth, out_dir, file_id + '.lf0')
    if not b_const_rate:
        write_featfile(v_shift, out_dir, file_id + '.shift')
    return


# ======================================================================================================
# type-2 analysis (magphase.py:2793-2866, :3123-3196): true-envelope magnitude of two-period frames, a per-frame gain
# ======================================================================================================
def _type2_rate(const_rate_ms):
    """const_rate_ms of the type-2 functions: any finite number; <= 0 means the variable (pitch-synchronous) rate."""
    if isinstance(const_rate_ms, (bool, np.bool_)) or not isinstance(const_rate_ms, (int, float, np.integer, np.floating)):
        raise ValueError("const_rate_ms must be a finite number, got %r" % (const_rate_ms,))
    v = float(const_rate_ms)
    if not np.isfinite(v):
        raise ValueError("const_rate_ms must be a finite number, got %r" % (const_rate_ms,))
    return v


def _is_device_tensor(x):
    import sys

    torch = sys.modules.get("torch")
    return torch is not None and torch.is_tensor(x) and x.device.type != "cpu"


def _type2_check(utts, fft_len):
    """Host argument checks of the type-2 analysis: (v_sig, fs, v_pm_sec, v_voi) tuples, one fft_len the device path
    takes (1024, 2048 or 4096) for the whole call, epochs and voicing of one length."""
    N = None
    for i, u in enumerate(utts):
        if len(u) != 4:
            raise ValueError("utts[%d]: expected (v_sig, fs, v_pm_sec, v_voi)" % i)
        v_sig, fs, v_pm_sec, v_voi = u
        if (v_sig.dim() if _is_device_tensor(v_sig) else np.ndim(v_sig)) != 1:   # (a device tensor is not staged for this)
            raise ValueError("utts[%d]: v_sig must be 1-D" % i)
        if np.ndim(v_pm_sec) != 1 or np.shape(v_pm_sec) != np.shape(v_voi) or np.size(v_pm_sec) == 0:
            raise ValueError("utts[%d]: v_pm_sec and v_voi must be non-empty 1-D vectors of one length" % i)
        n = int(fft_len) if fft_len is not None else hm.define_fft_len(fs)
        if n not in (1024, 2048, 4096):
            raise ValueError("fft_len %r not supported by the HIP path (1024, 2048 or 4096)" % (n,))
        if N is not None and n != N:
            raise ValueError("all utterances of a call must share fft_len (bucket by sample rate)")
        N = n
    if N is not None:
        hm.true_envelope_check(N // 2 + 1, "abs", 600)
    return N


def analysis_lossless_type2_batch(utts, fft_len=None, engine=None, return_device=False, return_iters=False):
    """
    Batched analysis_lossless_type2 (magphase.py:2793-2866) for utterances that already have epochs: utts = list of
    (v_sig, fs, v_pm_sec, v_voi), one fft_len per call.  Returns a list of (m_mag_env, m_real, m_imag, v_f0, fs, v_shift,
    v_gain): the true envelope (600 coefficients, thres_db 0.1) of the two-period magnitudes, the one-period phase, f0,
    the float shifts of the unrounded epochs and the per-frame gain, all without the reference's row 0; float64 numpy
    (return_device: float32 device rows for the three matrices and a float64 device gain; v_f0 / v_shift stay numpy).
    Both transforms are float64 (k_analysis_f64), as analysis_compressed's.  A magnitude row with a zero bin gives an
    all-NaN envelope row, as in the reference.  return_iters: each tuple gets the envelope's passes per frame (int32)
    appended.  Engine: Type2AnalysisPlan.
    v_sig may be a 1-D torch tensor on the engine's device (float32 / float16 / bfloat16 / float64, any element stride),
    under the rules of analysis_lossless_batch: no sample is staged through the host, and the rows equal those of the
    host-array call on the same float32 samples bit for bit.
    Autograd: with return_device, grad mode on and a device v_sig that requires grad, m_mag_env / m_real / m_imag carry a
    grad_fn and tensor.backward() reaches v_sig (magphase_amd/autograd.py, Type2AnalysisPlan.run_backward: the envelope's
    backward kernel k_true_envelope_bwd, then the lossless analysis' backward kernels over the two frame tables; the
    forward launches and their rows are the same).  The envelope's gradient is that of the passes as the device ran them:
    the stop test is not differentiated.  Not differentiable: v_pm_sec, v_voi and fs; v_f0, v_shift and the per-frame
    gain (float64, detached) carry no grad_fn; no double backward.
    """
    utts = list(utts)
    if not utts:
        return []
    _type2_check(utts, fft_len)
    engine = engine or get_engine()
    plan = Type2AnalysisPlan(engine, utts, fft_len=fft_len)
    for lens in plan.long_frame_lens:
        for n in lens:  # Q19: truncation warns, it does not raise (magphase.py:311-315)
            warnings.warn(_WARN_LONG % (plan.fft_len, n))
    if hm.wants_grad(return_device, [u[0] for u in utts]):
        from .autograd import analyze_type2

        env, real, imag, gain, iters = analyze_type2(plan, [u[0] for u in utts])
    else:
        env, real, imag, gain, iters = plan.run(want_iters=return_iters)
    if not return_device:
        h = engine.to_host_f64_many([env, real, imag]) if plan.total_frames else [np.zeros((0, env.shape[1]))] * 3
        h_gain = gain.cpu().numpy()
    h_iters = iters.cpu().numpy() if return_iters else None   # (under autograd iters exists either way: no copy unasked)
    out = []
    for u in range(len(utts)):
        a, b = plan.out_rows(u)
        if return_device:
            feats = (env[a:b], real[a:b], imag[a:b])
            g = gain[a:b]
        else:
            feats = tuple(x[a:b].copy() for x in h)
            g = h_gain[a:b].copy()
        r = feats + (plan.v_f0[u], plan.fs[u], plan.v_shift[u], g)
        out.append(r + (h_iters[a:b].copy(),) if return_iters else r)
    return out


def analysis_lossless_type2(wav_file, fft_len=None, out_dir=None):
    """magphase.py:2793-2866: (m_mag_env, m_real, m_imag, v_f0, fs, v_shift, v_gain); with out_dir: writes
    <name>.mag (the envelope) / .real / .imag / .f0 / .shift as float32 and returns None (no gain file, as the reference)."""
    v_sig, fs = la.read_audio_file(wav_file)
    v_pm_sec, v_voi = _epochs_for(wav_file)
    m_mag, m_real, m_imag, v_f0, fs, v_shift, v_gain = analysis_lossless_type2_batch([(v_sig, fs, v_pm_sec, v_voi)],
                                                                                     fft_len=fft_len)[0]
    if type(out_dir) is str:
        file_id = os.path.basename(wav_file).split(".")[0]
        write_featfile(m_mag, out_dir, file_id + ".mag")
        write_featfile(m_real, out_dir, file_id + ".real")
        write_featfile(m_imag, out_dir, file_id + ".imag")
        write_featfile(v_f0, out_dir, file_id + ".f0")
        write_featfile(v_shift, out_dir, file_id + ".shift")
        return
    return m_mag, m_real, m_imag, v_f0, fs, v_shift, v_gain


def analysis_compressed_type2_batch(utts, fft_len=None, mag_dim=60, phase_dim=45, b_norm_mag=False,
                                    const_rate_ms=-1.0, engine=None, return_device=False):
    """
    Batched analysis_compressed_type2 (magphase.py:3123-3196): utts = list of (v_sig, fs, v_pm_sec, v_voi), one sample
    rate per call.  Returns a list of (m_mag_mel_log, m_real_mel, m_imag_mel, v_lf0_smth, v_shift, fs, fft_len, v_lgain).
    const_rate_ms > 0 (any value): rows, f0 / voicing and gain on the grid of that period (v_shift stays at the variable
    rate); <= 0: the variable rate.  v_lgain = la.log(v_gain); b_norm_mag: the mean of columns 1.. of each log-mel row is
    subtracted, stored in column 0 and returned as v_lgain (magphase.py:3178-3182).  The three matrices are float64 numpy
    (return_device: float32 device rows); v_lf0_smth, v_shift and v_lgain are float64 numpy.
    v_sig may be a 1-D torch tensor on the engine's device, under the rules of analysis_lossless_batch (no host staging,
    rows bit-identical to the host-array call).
    Autograd: with return_device, grad mode on and a device v_sig that requires grad, the three matrices carry a grad_fn
    and tensor.backward() reaches v_sig, at the variable rate and at any const_rate_ms > 0, for mag_dim and phase_dim up
    to 64 (more: NotImplementedError naming the argument); b_norm_mag is then applied with out-of-place torch operations,
    so it is differentiated too (Type2CompressedAnalysisPlan.run_backward).  An unvoiced frame
    contributes no phase gradient and a phase coefficient on the clip (exactly +-1) has a zero gradient, as in
    analysis_compressed_batch.  Not differentiable: v_pm_sec, v_voi, fs; v_lf0_smth, v_shift and v_lgain (the gain stays
    float64 and detached) carry no grad_fn; no double backward.
    """
    const_rate_ms = _type2_rate(const_rate_ms)
    utts = list(utts)
    if not utts:
        return []
    _type2_check(utts, fft_len)
    fs0 = utts[0][1]
    if any(u[1] != fs0 for u in utts):
        raise ValueError("one sample rate per batch")
    hm.define_alpha(fs0)   # (ValueError for a sample rate the warp has no alpha for)
    engine = engine or get_engine()
    plan = Type2CompressedAnalysisPlan(engine, utts, fft_len=fft_len, mag_dim=mag_dim, phase_dim=phase_dim,
                                       const_rate_ms=const_rate_ms)
    for lens in plan.t2.long_frame_lens:
        for n in lens:
            warnings.warn(_WARN_LONG % (plan.fft_len, n))
    with_grad = hm.wants_grad(return_device, [u[0] for u in utts])
    if with_grad:
        from .autograd import analyze_compressed_type2

        (mag, real, imag), gain = analyze_compressed_type2(plan, [u[0] for u in utts])
    else:
        (mag, real, imag), gain = plan.run()
    h_gain = gain.cpu().numpy()
    v_mean = None
    if b_norm_mag and with_grad:   # the same arithmetic out of place, so that autograd sees it
        import torch

        md = mag.double()
        v_mean = md[:, 1:].mean(dim=1)
        mag = torch.cat((v_mean[:, None], md[:, 1:] - v_mean[:, None]), dim=1).to(torch.float32)
        v_mean = v_mean.detach().cpu().numpy()
    elif b_norm_mag:   # magphase.py:3178-3182, float64
        md = mag.double()
        v_mean = md[:, 1:].mean(dim=1)
        md -= v_mean[:, None]
        md[:, 0] = v_mean
        mag.copy_(md)
        v_mean = v_mean.cpu().numpy()
    if not return_device:
        h = (engine.to_host_f64_many([mag, real, imag]) if plan.total_out_frames else
             [np.zeros((0, int(t.shape[1]))) for t in (mag, real, imag)])
    lf0 = la.f0_to_lf0(np.concatenate([(f > 0).astype("float") * m for f, m in
                                       zip(plan.f0_out, hm.medfilt3_batch(plan.f0_out))]))   # magphase.py:2497-2501
    res = []
    for u in range(len(utts)):
        a, b = int(plan.out_off[u]), int(plan.out_off[u + 1])
        fa, fb = plan.t2.out_rows(u)
        v_gain = h_gain[fa:fb]
        if plan.const:   # magphase.py:3135 (float64 on the host)
            v_gain = interp_from_variable_to_const_frm_rate(v_gain, plan.grid[u], const_rate_ms, plan.fs)
        v_lgain = v_mean[a:b].copy() if b_norm_mag else la.log(v_gain)
        feats = (mag[a:b], real[a:b], imag[a:b]) if return_device else tuple(x[a:b].copy() for x in h)
        res.append(feats + (lf0[a:b].copy(), plan.t2.v_shift[u], plan.fs, plan.fft_len, v_lgain))
    return res


def analysis_compressed_type2(wav_file, fft_len=None, out_dir=None, mag_dim=60, phase_dim=45, b_norm_mag=False,
                              const_rate_ms=-1.0):
    """magphase.py:3123-3196: (m_mag_mel_log, m_real_mel, m_imag_mel, v_lf0_smth, v_shift, fs, fft_len, v_lgain); with
    out_dir: writes <name>.mag / .real / .imag / .lf0 (and .shift at the variable rate) and returns None."""
    const_rate_ms = _type2_rate(const_rate_ms)
    v_sig, fs = la.read_audio_file(wav_file)
    v_pm_sec, v_voi = _epochs_for(wav_file)
    r = analysis_compressed_type2_batch([(v_sig, fs, v_pm_sec, v_voi)], fft_len=fft_len, mag_dim=mag_dim,
                                        phase_dim=phase_dim, b_norm_mag=b_norm_mag, const_rate_ms=const_rate_ms)[0]
    if type(out_dir) is str:
        file_id = os.path.basename(wav_file).split(".")[0]
        write_featfile(r[0], out_dir, file_id + ".mag")
        write_featfile(r[1], out_dir, file_id + ".real")
        write_featfile(r[2], out_dir, file_id + ".imag")
        write_featfile(r[3], out_dir, file_id + ".lf0")
        if const_rate_ms <= 0.0:
            write_featfile(r[4], out_dir, file_id + ".shift")
        return
    return r


# ======================================================================================================
# type-2 synthesis from compressed features (magphase.py:1452-1606)
# ======================================================================================================
def _type2_synthesis_check(utts, fs, fft_len, hf_slope_coeff):
    """Host argument checks of the type-2 synthesis, before any device work; returns fft_len."""
    n = int(fft_len) if fft_len is not None else hm.define_fft_len(fs)
    if n not in (1024, 2048, 4096):
        raise ValueError("fft_len %r not supported by the HIP path (1024, 2048 or 4096)" % (n,))
    hm.define_alpha(fs)   # (ValueError for a sample rate the warp has no alpha for)
    if isinstance(hf_slope_coeff, (bool, np.bool_)) or not np.isscalar(hf_slope_coeff) or not np.isfinite(hf_slope_coeff):
        raise ValueError("hf_slope_coeff must be a finite number, got %r" % (hf_slope_coeff,))
    for i, u in enumerate(utts):
        if len(u) != 4:
            raise ValueError("utts[%d]: expected (m_mag_mel_log, m_real_mel, m_imag_mel, v_lf0)" % i)
        mag, real, imag, lf0 = u
        if np.ndim(mag) != 2 or np.ndim(real) != 2 or np.ndim(imag) != 2 or np.ndim(lf0) != 1:
            raise ValueError("utts[%d]: m_mag_mel_log / m_real_mel / m_imag_mel must be 2-D and v_lf0 1-D" % i)
        rows = [int(np.shape(x)[0]) for x in (mag, real, imag, lf0)]
        if len(set(rows)) != 1:
            raise ValueError("utts[%d]: mag / real / imag / lf0 have %d / %d / %d / %d rows" % ((i,) + tuple(rows)))
        if np.shape(real)[1] != np.shape(imag)[1]:
            raise ValueError("utts[%d]: m_real_mel and m_imag_mel have different widths (%d, %d)"
                             % (i, np.shape(real)[1], np.shape(imag)[1]))
        if np.shape(mag)[1] < 1 or np.shape(real)[1] < 1:
            raise ValueError("utts[%d]: empty coefficient rows" % i)
        if rows[0] < 2:   # the reference indexes v_pm[-2] (magphase.py:1519)
            raise ValueError("utts[%d]: fewer than two synthesis frames (%d rows)" % (i, rows[0]))
        if not np.all(np.isfinite(np.asarray(lf0, dtype=np.float64))):
            raise ValueError("utts[%d]: v_lf0 has non-finite values (unvoiced frames carry a finite log, e.g. -1e10)" % i)
    return n


def synthesis_from_compressed_type2_batch(utts, fs, fft_len=None, hf_slope_coeff=1.0, b_voi_ap_win=True,
                                          const_rate_ms=-1.0, noise=None, noise_mode='reference', noise_seeds=None,
                                          engine=None, pcm16_norm=False, defer_rng=False, return_device=False):
    """
    Batched synthesis_from_compressed_type2 (magphase.py:1452-1606); utts: list of (m_mag_mel_log, m_real_mel,
    m_imag_mel, v_lf0) as analysis_compressed_type2 returns them, one sample rate per call.  const_rate_ms > 0: the rows
    lie on a grid of that period (any value); <= 0: the variable rate.  hf_slope_coeff: the aperiodic spectrum of
    unvoiced frames is multiplied by np.linspace(1, hf_slope_coeff, fft_len/2 + 1).  The output always passes the
    reference's elliptic high-pass (order 4, 60 Hz).  noise, noise_mode, noise_seeds, pcm16_norm and defer_rng as in
    synthesis_from_compressed_batch.  Returns a list of float64 signals (int16 with pcm16_norm).  Engine:
    Type2SynthesisPlan.
    Device features and return_device as in synthesis_from_compressed_batch: the matrices (and v_lf0) may be tensors on
    the engine's device; with return_device the signals are float64 (int16 with pcm16_norm) views of the device PCM
    buffer.  Device lf0 vectors come to the host first (one copy), so every argument check, the finite-lf0 check
    included, still runs before the first kernel.  Launches go to torch's current stream of the engine's device.
    Autograd: with return_device, grad mode on and a device m_mag_mel_log / m_real_mel / m_imag_mel that requires grad,
    the float64 signals carry a grad_fn and tensor.backward() reaches the three coefficient matrices, in each one's own
    dtype and shape (magphase_amd/autograd.py; the forward launches and their samples are the
    same).  At the variable rate and at any const_rate_ms, for any hf_slope_coeff, either b_voi_ap_win, either noise_mode
    or an explicit noise.  phase_dim > mag_dim: the gradient columns from mag_dim on are zeros (the forward does not read
    them).  Not differentiable: v_lf0, fs, hf_slope_coeff, the noise and its gain (one per utterance, the rms of the noise
    spectra alone: the backward pass is exact with it held constant).  NotImplementedError, naming the argument, for
    pcm16_norm other than False and for more than 64 columns in a matrix.  No double backward.
    """
    const_rate_ms = _type2_rate(const_rate_ms)
    utts = list(utts)
    if not utts:
        return []
    want_grad = hm.wants_grad(return_device, [x for u in utts for x in u[:3]])   # (CPU tensors take the host path)
    if want_grad and pcm16_norm is not False:   # what has no backward pass says so before anything is built
        raise NotImplementedError("pcm16_norm=%r (int16 output) has no backward pass" % (pcm16_norm,))
    utts, on_dev = _tensor_inputs(utts, _SYN_NAMES, lf0_at=3)
    if on_dev:
        engine = engine or get_engine()
        if all(len(u) == 4 for u in utts):   # (device lf0 comes down for the checks below; a malformed tuple raises there)
            utts = [tuple(u[:3]) + (l,) for u, l in zip(utts, engine.lf0_to_host([u[3] for u in utts]))]
    _type2_synthesis_check(utts, fs, fft_len, hf_slope_coeff)
    if want_grad:
        check_type2_grad_dims(np.shape(utts[0][0])[1], np.shape(utts[0][1])[1])
    engine = engine or get_engine()
    plan = Type2SynthesisPlan(engine, utts, fs, fft_len=fft_len, hf_slope_coeff=hf_slope_coeff,
                              b_voi_ap_win=b_voi_ap_win, const_rate_ms=const_rate_ms, noise=noise,
                              noise_mode=noise_mode, noise_seeds=noise_seeds, defer_rng=defer_rng)
    if want_grad:   # the same launches inside a torch.autograd.Function (magphase_amd/autograd.py)
        from .autograd import synthesize_compressed_type2

        pcm_dev = synthesize_compressed_type2(plan, utts)
        return [pcm_dev[int(plan.out_off_host[u]):int(plan.out_off_host[u + 1])] for u in range(len(utts))]
    pcm_dev = engine.output_hpf(plan.run(), plan.out_off_host, fs, design="ellip60")   # magphase.py:1599-1604
    if return_device:
        if pcm16_norm is not False:
            pcm_dev = engine.output_pcm16(pcm_dev, plan.out_off_host, norm=pcm16_norm, return_device=True)
        return [pcm_dev[int(plan.out_off_host[u]):int(plan.out_off_host[u + 1])] for u in range(len(utts))]
    if pcm16_norm is not False:
        pcm = engine.output_pcm16(pcm_dev, plan.out_off_host, norm=pcm16_norm)
    else:
        pcm = pcm_dev.cpu().numpy()
    return [pcm[plan.out_off_host[u]:plan.out_off_host[u + 1]] for u in range(len(utts))]


def synthesis_from_compressed_type2(m_mag_mel_log, m_real_mel, m_imag_mel, v_lf0, fs, fft_len=None, hf_slope_coeff=1.0,
                                    b_voi_ap_win=True, b_norm_mag=False, v_lgain=None, const_rate_ms=-1.0):
    """magphase.py:1452-1606.  b_norm_mag and v_lgain are accepted and ignored, as in the reference (it overwrites
    b_norm_mag with False at :1467 and its gain block, :1578-1594, is commented out): features written with
    b_norm_mag=True synthesise as they do there, wrongly scaled."""
    return synthesis_from_compressed_type2_batch([(m_mag_mel_log, m_real_mel, m_imag_mel, v_lf0)], fs, fft_len=fft_len,
                                                 hf_slope_coeff=hf_slope_coeff, b_voi_ap_win=b_voi_ap_win,
                                                 const_rate_ms=const_rate_ms)[0]


# ======================================================================================================
# label re-timing for constant-frame-rate trainers
# ======================================================================================================
def get_num_of_frms_per_state(v_shift, lab_state_align_file, fs, b_prevent_zeros=False, n_states_x_phone=5,
                              nfrms_tolerance=6):
    """
    magphase.py:2111-2150: number of pitch-synchronous frames (epochs) that fall inside every line of an HTS
    state-aligned label file ([start, end) in units of 100 ns).  Frames left over after the last line (at most
    `nfrms_tolerance`: label files often end early) go to the last state; a total mismatch or a phone without any
    frame raises ValueError like the reference.  Returns float64[n_states].
    """
    m_lab = np.loadtxt(lab_state_align_file, usecols=(0, 1), ndmin=2)
    m_lab_ms = m_lab / 10000.0
    v_ep_ms = np.cumsum(v_shift) * 1000.0 / fs
    # epochs e with start <= e < end == (#epochs < end) - (#epochs < start); the epoch times are non-decreasing
    v_ep_sorted = np.sort(v_ep_ms)
    v_n = (np.searchsorted(v_ep_sorted, m_lab_ms[:, 1], side="left")
           - np.searchsorted(v_ep_sorted, m_lab_ms[:, 0], side="left")).astype(np.float64)
    v_n = np.maximum(v_n, 0.0)
    n_left = np.size(v_shift) - np.sum(v_n)
    if 0 < n_left <= nfrms_tolerance:
        v_n[-1] += n_left
    if np.sum(v_n) != np.size(v_shift):
        raise ValueError("Total number of frames is different to the number of frames of the shifts.")
    v_n_ph = v_n.reshape((v_n.size // n_states_x_phone, n_states_x_phone)).sum(axis=1)
    if np.any(v_n_ph == 0.0):
        raise ValueError("There is some phoneme(s) that do(es) not contain any frame.")
    if b_prevent_zeros:
        v_n[v_n == 0] = 1
    return v_n


# ---------------------------------------------------------------------------------------------
# Maximum-likelihood parameter generation.  Stated here, not taken from Merlin / bandmat:
# parity with Merlin's mlpg is UNPINNED.
# ---------------------------------------------------------------------------------------------
MLPG_WINDOWS = ((-0.5, 0.0, 0.5), (1.0, -2.0, 1.0))   # delta and acceleration, taps (w[-1], w[0], w[+1])


def _mlpg_device_var(engine, var, per_frame, width):
    return engine.mlpg_pack(var, width)[0] if per_frame else \
        (var if not isinstance(var, np.ndarray) else engine.to_device(var, var.dtype))


def _mlpg_run(engine, means, var, per_frame, w, streams, width, return_device, var_inputs=()):
    """The launches of mlpg_batch / mlpg_streams_batch -> (float64 device buffer [sum F_i x sum D] (None when the batch has
    no frames), packed means or None, row offsets).  var_inputs: the variance tensors of var_grad=True."""
    offs = np.concatenate(([0], np.cumsum([int(m.shape[0]) for m in means]))).astype(np.int64)
    if int(offs[-1]) == 0:
        return None, None, offs
    var_dev = _mlpg_device_var(engine, var, per_frame, width)
    if not hm.wants_grad(return_device, var_inputs):
        var_inputs = ()
    if var_inputs or hm.wants_grad(return_device, means):   # (hm.mlpg_check made host arrays of CPU tensors)
        from . import autograd

        buf = None
        out = autograd.mlpg(engine, means, var_dev, streams, w, width, var_inputs)
    else:
        buf, _ = engine.mlpg_pack(means, width)
        out = engine.mlpg_streams(buf, var_dev, engine.to_device(offs.astype(np.int32), np.int32), streams, w)
    return out, buf, offs


def mlpg_batch(means, var, windows=MLPG_WINDOWS, engine=None, return_device=False, var_grad=False):
    """
    Maximum-likelihood parameter generation on the device (k_mlpg_solve): the trajectory c = A^-1 b with
    A = sum_k W_k^T P_k W_k and b = sum_k W_k^T P_k mu_k over the K = 1 + len(windows) streams (static, then one per
    three-tap window (w[-1], w[0], w[+1])); window taps that fall outside an utterance are dropped.
    means: list of [F_i x K D] matrices, columns [static D | delta D | acc D], each a numpy array or a device tensor
    (float32 / float64, any row stride); one D per call.  var: ONE [K D] vector (the global variance), or a list of
    [F_i x K D] matrices (per-frame variances; also the way to another boundary convention).  Variances in host arrays must
    be finite and > 0 (ValueError, before any device call); variances in DEVICE tensors are not inspected.
    Returns a list of [F_i x D] float64 arrays (return_device: float64 device tensors, views of one buffer); an utterance
    without frames gives a (0, D) result.
    Autograd: with return_device, grad mode on and a device mean matrix that requires grad, the results carry a grad_fn
    and backward() gives each mean matrix a gradient in its own dtype and shape (dL/dmu_k = P_k W_k A^-1 dL/dc); the
    forward values are the same bits either way.  Variances and windows get no gradient; no double backward.
    var_grad=True (with return_device, and the variances in device tensors: ValueError otherwise): a variance tensor that
    requires grad gets one too, in its own dtype and shape -- dL/dvar_k[t] = -(W_k z)[t] (mu_k[t] - (W_k c)[t]) / var_k[t]^2
    with z = A^-1 dL/dc (k_mlpg_var_bwd), a global row the sum over all frames of the batch -- whether or not a mean
    requires grad; the forward values are the same bits.
    Not Merlin's code: the mathematics is restated, parity with Merlin / bandmat is unpinned.
    """
    var_given = var
    means, var, w, D, per_frame = hm.mlpg_check(means, var, windows, "mlpg_batch")
    if not means:
        return []
    var_inputs = hm.mlpg_var_grad_check(var_grad, return_device, var_given, var, per_frame, "mlpg_batch")
    engine = engine or get_engine()
    K = w.shape[0] + 1
    out, _buf, offs = _mlpg_run(engine, means, var, per_frame, w, [(0, D)], K * D, return_device, var_inputs)
    if out is None:
        if return_device:
            import torch

            return [torch.zeros((0, D), dtype=torch.float64, device=engine.device) for _ in means]
        return [np.zeros((0, D)) for _ in means]
    rows = [out[int(a):int(b)] for a, b in zip(offs[:-1], offs[1:])]
    if return_device:
        return rows
    host = out.cpu().numpy()
    return [host[int(a):int(b)] for a, b in zip(offs[:-1], offs[1:])]


def mlpg_trajectory_nll_batch(means, var, targets, windows=MLPG_WINDOWS, engine=None, return_device=False):
    """
    The trajectory negative log-likelihood -log N(x; c, A^-1) of natural static features under the MLPG system
    (k_mlpg_solve, then k_mlpg_nll): c = A^-1 b is the MLPG trajectory of the means, A = sum_k W_k^T P_k W_k, and per
    utterance and dimension
        NLL = 1/2 sum_k sum_t p_k[t] (W_k (x - c))[t]^2 - 1/2 sum_i log d_i + F/2 log 2 pi,
    d_i the pivots of the LDL^T factor of A.  means, var: as mlpg_batch takes them; targets: list of
    [F_i x D] static matrices (host arrays or device tensors, float32 / float64, any row stride).  Returns [n_utts x D]
    float64 (a numpy array; return_device: a device tensor); an utterance without frames gives zeros.
    Autograd: with return_device, grad mode on and a device mean or variance tensor that requires grad, the result
    carries a grad_fn and backward() gives the means and the device variance tensors gradients in their own dtype and
    shape (k_mlpg_nll_bwd; a global variance row: the sum over all frames of the batch).  The targets get none.
    One stream per call: pass column slices per stream; voicing-dependent lf0 likelihoods are the caller's.
    """
    what = "mlpg_trajectory_nll_batch"
    var_given = var
    means, var, w, D, per_frame = hm.mlpg_check(means, var, windows, what)
    targets = hm.mlpg_targets_check(targets, means, D if means else None, what)
    if not means:
        return np.zeros((0, 0))
    var_inputs = hm.mlpg_var_inputs(var_given, var, per_frame) or []
    engine = engine or get_engine()
    import torch

    K = w.shape[0] + 1
    offs = np.concatenate(([0], np.cumsum([int(m.shape[0]) for m in means]))).astype(np.int64)
    if int(offs[-1]) == 0:
        z = torch.zeros((len(means), D), dtype=torch.float64, device=engine.device)
        return z if return_device else z.cpu().numpy()
    var_dev = _mlpg_device_var(engine, var, per_frame, K * D)
    x, _ = engine.mlpg_pack(targets, D)
    if not hm.wants_grad(return_device, var_inputs):
        var_inputs = []
    if var_inputs or hm.wants_grad(return_device, means):
        from . import autograd

        nll = autograd.mlpg_trajectory_nll(engine, means, var_dev, x, w, D, var_inputs)
    else:
        buf, _ = engine.mlpg_pack(means, K * D)
        offs_dev = engine.to_device(offs.astype(np.int32), np.int32)
        nll = engine.mlpg_trajectory_nll(engine.mlpg_solve(buf, var_dev, offs_dev, D, w), x, var_dev, offs_dev, D, w)
    return nll if return_device else nll.detach().cpu().numpy()


def mlpg_trajectory_nll(m_mean, var, m_target, windows=MLPG_WINDOWS):
    """mlpg_trajectory_nll_batch for one utterance: [F x K D] means, [K D] or [F x K D] variances, [F x D] static
    targets -> [D] float64."""
    per_frame = getattr(var, "ndim", None) == 2 or (hasattr(var, "dim") and var.dim() == 2)
    return mlpg_trajectory_nll_batch([m_mean], [var] if per_frame else var, [m_target], windows=windows)[0]


def mlpg(m_mean, var, windows=MLPG_WINDOWS):
    """mlpg_batch for one utterance: [F x K D] means, [K D] or [F x K D] variances -> [F x D] float64."""
    per_frame = getattr(var, "ndim", None) == 2 or (hasattr(var, "dim") and var.dim() == 2)
    return mlpg_batch([m_mean], [var] if per_frame else var, windows=windows)[0]


def dynamic_features_batch(mats, windows=MLPG_WINDOWS, engine=None, return_device=False):
    """
    The static / delta / acceleration features of MLPG's own windows (k_mlpg_apply, no precision factor): every [F_i x D]
    matrix (numpy or device tensor, float32 / float64) -> [F_i x K D] float64, columns [static | delta | acc], window taps
    outside the utterance dropped -- what mlpg_batch inverts: mlpg_batch(dynamic_features_batch(x), any variances) == x.
    """
    w = hm.mlpg_windows(windows)
    if isinstance(mats, np.ndarray) or not isinstance(mats, (list, tuple)):
        raise ValueError("dynamic_features_batch: mats must be a list of [frames x D] matrices")
    mats = [hm._mlpg_matrix(m, "dynamic_features_batch: mats[%d]" % i) for i, m in enumerate(mats)]
    if not mats:
        return []
    D, K = int(mats[0].shape[1]), w.shape[0] + 1
    if D < 1 or any(int(m.shape[1]) != D for m in mats):
        raise ValueError("dynamic_features_batch: every matrix must have the same number (>= 1) of columns")
    engine = engine or get_engine()
    import torch

    x, offs = engine.mlpg_pack(mats, D)
    total = int(offs[-1])
    if total == 0:
        out = torch.zeros((0, K * D), dtype=torch.float64, device=engine.device)
    else:
        out = engine.mlpg_apply(x, None, engine.to_device(offs.astype(np.int32), np.int32), D, w)
    if not return_device:
        out = out.cpu().numpy()
    return [out[int(a):int(b)] for a, b in zip(offs[:-1], offs[1:])]


def dynamic_features(m, windows=MLPG_WINDOWS):
    """dynamic_features_batch for one matrix."""
    return dynamic_features_batch([m], windows=windows)[0]


MLPG_LAYOUT = (("mag", 60), ("real", 10), ("imag", 10), ("lf0", 1))


def mlpg_streams_batch(cmps, var, layout=MLPG_LAYOUT, vuv=True, vuv_thres=0.5, windows=MLPG_WINDOWS, engine=None,
                       return_device=False, var_grad=False):
    """
    MLPG of an acoustic model's whole output rows.  cmps: list of [F_i x W] matrices (numpy or device tensors, as
    mlpg_batch takes them); stream s of layout = ((name, dim), ...) occupies K dim_s columns [static | delta | acc], the
    streams in layout order, then ONE static voicing column when vuv is set.  var: one [W] vector or a list of [F_i x W]
    matrices (the voicing column's entries are not used and not checked).  One mpx_mlpg_solve launch per stream, on column
    slices of the same packed matrix.
    Returns per utterance the tuple of trajectories in layout order -- with the default layout (m_mag_mel_log, m_real_mel,
    m_imag_mel, v_lf0), exactly what synthesis_from_compressed_batch takes: [F_i x dim] float64 matrices, a stream named
    'lf0' as a vector, set to the unvoiced value of la.f0_to_lf0 (-1e10) where the voicing column is <= vuv_thres.
    return_device: device tensors (column slices of one float64 buffer; v_lf0 a float64 device vector), which the synthesis
    reads where they lie.  Autograd as in mlpg_batch (the voicing decision is not differentiated; unvoiced frames send no
    gradient to lf0).  var_grad as in mlpg_batch; the voicing column of the variances gets zeros.
    """
    import torch

    K = hm.mlpg_windows(windows).shape[0] + 1
    layout, streams, need = hm.mlpg_layout(layout, vuv, K)
    if isinstance(vuv_thres, bool) or not isinstance(vuv_thres, (int, float)) or not np.isfinite(vuv_thres):
        raise ValueError("mlpg_streams_batch: vuv_thres must be a finite number")

    def width_of(width, _k):
        if width != need:
            raise ValueError("mlpg_streams_batch: the layout asks for %d columns, the matrices have %d" % (need, width))
        return 0

    var_given = var
    means, var, w, _D, per_frame = hm.mlpg_check(cmps, var, windows, "mlpg_streams_batch", width_of=width_of,
                                                 var_cols=slice(0, need - (1 if vuv else 0)))
    if not means:
        return []
    var_inputs = hm.mlpg_var_grad_check(var_grad, return_device, var_given, var, per_frame, "mlpg_streams_batch")
    width = int(means[0].shape[1])
    engine = engine or get_engine()
    out, buf, offs = _mlpg_run(engine, means, var, per_frame, w, streams, width, return_device, var_inputs)
    if out is None:
        z = [np.zeros(0) if n == "lf0" else np.zeros((0, d)) for n, d in layout]
        if return_device:
            z = [torch.from_numpy(a).to(engine.device) for a in z]
        return [tuple(z) for _ in means]
    cols, o = [], 0
    for n, d in layout:
        c = out[:, o:o + d]
        if n == "lf0" and d == 1:
            c = c[:, 0]
            if vuv:
                if buf is None:
                    buf, _ = engine.mlpg_pack(means, width)
                voiced = buf[:, width - 1].detach() > float(vuv_thres)
                c = torch.where(voiced, c, torch.full((), la.MAGIC, dtype=torch.float64, device=engine.device))
        cols.append(c)
        o += d
    if not return_device:
        cols = [c.cpu().numpy() for c in cols]
    return [tuple(c[int(a):int(b)] for c in cols) for a, b in zip(offs[:-1], offs[1:])]


# ---------------------------------------------------------------------------------------------
# Acoustic composition: the rows an acoustic model is trained on -- the inverse of
# mlpg_streams_batch.  Not the reference's code but for the interpolation of lf0, which is la.interp_unv_regions'.
# ---------------------------------------------------------------------------------------------
def _cmp_run(engine, utts, dims, interp, vuv, w, norm, unv_fill):
    """The launches of acoustic_compose_batch -> (float32 device rows [sum F_i x W], row offsets)."""
    x, offs = engine.cmp_pack(utts, dims)
    offs_dev = engine.to_device(offs.astype(np.int32), np.int32)
    nb = engine.cmp_neighbours(x[:, int(sum(dims[:interp]))], offs_dev) if interp >= 0 else None
    return engine.cmp_compose(x, nb, offs_dev, dims, interp, vuv, w, norm=norm, unv_fill=unv_fill), offs


def acoustic_compose_batch(feats, layout=MLPG_LAYOUT, vuv=True, windows=MLPG_WINDOWS, norm=None, unv_fill=0.0, engine=None,
                           return_device=False):
    """
    The rows a Merlin-style acoustic model is trained on, composed on the device (k_cmp_neighbours, k_cmp_compose): what
    mlpg_streams_batch takes apart again.  feats: list of per-utterance tuples in layout order -- with the default layout
    (m_mag_mel_log, m_real_mel, m_imag_mel, v_lf0), what analysis_compressed_batch and mlpg_streams_batch return; each a
    host array or a tensor on the engine's device, any float dtype (a float16 lf0 is refused: it cannot hold -1e10) and
    any row stride; a stream of dimension 1 may be a vector.
    Returns per utterance [F_i x W], W = K sum(dims) + (1 if vuv), K = 1 + len(windows): stream s as [static | delta | acc]
    in its K dim_s columns, the streams in layout order, then the voicing column (hostmath.mlpg_layout's map) -- float64
    host arrays, or with return_device float32 device tensors, row views of one buffer.
    A stream named 'lf0' of dimension 1 is carried through unvoiced frames before its deltas are taken: voiced means
    v_lf0 > 0 (NaN is unvoiced); between two voiced frames the value is linear in the frame index; before the first and
    after the last voiced frame the nearest voiced value is held; an utterance without a voiced frame gets unv_fill.  An
    utterance with exactly ONE voiced frame holds that value everywhere -- the one departure from the reference's
    la.interp_unv_regions, which gives NaN at that frame (a 0 / 0 in scipy's interp1d).  The value stored in an unvoiced
    entry (-1e10, NaN, anything) is never read.  The voicing column is 1.0 in voiced frames, else 0.0.
    Deltas: the windows, taps and edge rule of dynamic_features_batch (taps outside the utterance are dropped), so
    mlpg_streams_batch(acoustic_compose_batch(feats), var) returns the statics.
    norm=(mean, std): two [W] vectors (host or device; AcousticStats.finalize()): the result is (y - mean) / std in every
    column, the voicing column included (pass 0 and 1 there to keep it raw); std must be finite and > 0 (ValueError).
    All arithmetic is float64, rounded once to float32 on the store.
    ValueError / TypeError before any launch: a stream of the wrong width, streams of one utterance with different frame
    counts, a dtype that is not a float dtype, bad windows, a bad layout.
    Autograd: with return_device, grad mode on and a device input that requires grad the rows carry a grad_fn
    (k_cmp_compose_bwd) and every stream's statics get a gradient in their own dtype and shape; unvoiced lf0 entries get
    exactly 0.  Voicing, norm, windows and unv_fill are not differentiated; no double backward.
    """
    what = "acoustic_compose_batch"
    layout, _streams, W, w, utts, interp = hm.cmp_check(feats, layout, vuv, windows, unv_fill, what)
    norm = hm.cmp_norm(norm, W, what)
    if not utts:
        return []
    dims = [d for _, d in layout]
    engine = engine or get_engine()
    import torch

    for u in utts:
        for m in u:
            if torch.is_tensor(m) and m.device != engine.device:
                raise ValueError("%s: tensor on %s, the engine runs on %s" % (what, m.device, engine.device))
    flat = [m for u in utts for m in u]
    if hm.wants_grad(return_device, flat):
        from . import autograd

        out, offs = autograd.acoustic_compose(engine, utts, dims, interp, bool(vuv), w, norm, float(unv_fill))
    else:
        out, offs = _cmp_run(engine, utts, dims, interp, bool(vuv), w, norm, float(unv_fill))
    if not return_device:
        out = engine.to_host_f64(out) if int(offs[-1]) else np.zeros((0, W))
    return [out[int(a):int(b)] for a, b in zip(offs[:-1], offs[1:])]


def acoustic_compose(m_mag_mel_log, m_real_mel, m_imag_mel, v_lf0, **kw):
    """acoustic_compose_batch for one utterance with the default layout -> [F x W]."""
    return acoustic_compose_batch([(m_mag_mel_log, m_real_mel, m_imag_mel, v_lf0)], **kw)[0]


class AcousticStats:
    """Corpus mean and standard deviation of composed rows for acoustic_compose_batch(norm=).  update(cmps) takes a list of
    [F_i x width] matrices (host arrays or device tensors, float32 / float64): count, column sums and centred sums of
    squares are computed on the device in one fixed order (k_cmp_moment_tiles / k_cmp_moment_final: the same input gives
    the same bits on every run) and merged into the running totals on the host in float64 with Chan's formula.
    finalize() -> (mean, std) float64 [width]: the population standard deviation; a zero-variance column gets std = 1.0
    and so normalises to 0."""

    def __init__(self, width):
        if isinstance(width, bool) or not isinstance(width, (int, np.integer)) or width < 1:
            raise ValueError("AcousticStats: width must be an integer >= 1")
        self.width = int(width)
        self.n = 0.0
        self.sums = np.zeros(self.width)
        self.m2 = np.zeros(self.width)

    def update(self, cmps, engine=None):
        if isinstance(cmps, np.ndarray) or not isinstance(cmps, (list, tuple)):
            raise ValueError("AcousticStats.update: a list of [frames x %d] matrices expected" % self.width)
        mats = [hm._mlpg_matrix(m, "AcousticStats.update: cmps[%d]" % i, self.width) for i, m in enumerate(cmps)]
        if not mats or sum(int(m.shape[0]) for m in mats) == 0:
            return self
        engine = engine or get_engine()
        x, _ = engine.mlpg_pack(mats, self.width)
        res = engine.cmp_column_moments(x).cpu().numpy()
        nb, sb, mb = float(res[0]), res[1:1 + self.width], res[1 + self.width:]
        if self.n == 0:
            self.n, self.sums, self.m2 = nb, sb.copy(), mb.copy()
        else:
            na = self.n
            n = na + nb
            delta = sb / nb - self.sums / na
            self.m2 = self.m2 + mb + delta * delta * (na * nb / n)
            self.sums = self.sums + sb
            self.n = n
        return self

    def finalize(self):
        if self.n == 0:
            raise ValueError("AcousticStats.finalize: no frames seen")
        std = np.sqrt(self.m2 / self.n)
        return self.sums / self.n, np.where(std > 0, std, 1.0)
