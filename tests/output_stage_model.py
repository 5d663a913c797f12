"""
References and operands of the output-stage kernel tests (tests/test_output_stage_host.py on the CPU,
tests/test_gpu_output_stage.py on the device).  numpy only: no torch, no GPU.

  hpf_cascade      the two direct-form-II-transposed sections of the output high-pass in np.longdouble, from the float64
                   sos of hostmath.hpf_tables: the authority the kernels of mpx_output_hpf are compared with
  hpf_blocked      mpx_output_hpf's ALGORITHM in float64 (per-block zero state, 2x2 carry as the 64-lane scan, G[n] . z_start,
                   section 0's free response folded into section 1's input).  It tests no kernel: its distance from
                   hpf_cascade is the error the blocked scan owns, the figure a device result is judged against
  pcm16            la.write_audio_file's host operations, NaN -> 0 explicit;  pcm16_to_f32: p * 2^-15
  merlin_stages    the four launches of mpx_post_filter_merlin in float64 from hostmath.merlin_tables, with the float32
                   rounding where the device stores float32 (the SPTK chain's pipe boundaries): names the launch that is
                   wrong when the output misses the oracle
"""
import warnings

import numpy as np

LD = np.longdouble
SENTINEL = -7.25            # what every output buffer is pre-filled with (exact in float32, float64)
SENTINEL_I16 = 0x5A5A       # ... the int16 ones

HPF_BLOCK = 256             # mpx_hpf_block(); the GPU tests assert it
HPF_LENS = (0, 1, 255, 256, 257, 16383, 16384, 16385, 32769, 49153)
HPF_CASES = (("butter40", 48000), ("butter40", 44100), ("butter40", 22050), ("butter40", 16000), ("butter40", 8000),
             ("ellip60", 48000), ("ellip60", 8000))
HPF_CORNER = {"butter40": 40.0, "ellip60": 60.0}
HPF_INPUTS = ("noise", "dc", "impulse0", "impulse255", "alternating", "corner_sine", "dc_noise")
HPF_HOST_FS = (48000, 44100, 22050, 16000, 8000)


# ---------------------------------------------------------------------------------------------------------------------
# high-pass
# ---------------------------------------------------------------------------------------------------------------------
def _section_coefs(sos_row, dtype):
    q = np.asarray(sos_row, dtype=np.float64)
    # the divisions as mpx_output_hpf does them, in float64 (a0 = 1 from scipy: exact)
    return [dtype(v) for v in (q[0] / q[3], q[1] / q[3], q[2] / q[3], q[4] / q[3], q[5] / q[3])]


def _biquad_loop(c, x):
    """y = b0 x + z0 ; z0 = b1 x + z1 - a1 y ; z1 = b2 x - a2 y  -- the kernel's operation order, in x's dtype."""
    b0, b1, b2, a1, a2 = c
    y = np.empty_like(x)
    z0 = z1 = x.dtype.type(0)
    for n in range(x.size):
        xv = x[n]
        yv = b0 * xv + z0
        z0 = b1 * xv + z1 - a1 * yv
        z1 = b2 * xv - a2 * yv
        y[n] = yv
    return y


def _biquad_ld(c, x):
    """One section in longdouble: scipy's lfilter (direct form II transposed as well) where it keeps longdouble, the
    plain loop otherwise."""
    if x.size == 0:
        return x.copy()
    try:
        from scipy import signal
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            y = signal.lfilter(np.array(c[:3], dtype=LD), np.array([LD(1), c[3], c[4]], dtype=LD), x)
        if y.dtype == np.dtype(LD) and y.shape == x.shape:
            return y
    except Exception:
        pass
    return _biquad_loop(c, x)


def hpf_cascade(sos, x, loop=False):
    """The output high-pass of one utterance from a zero state, longdouble [len(x)]."""
    y = np.asarray(x).astype(LD)
    for sec in range(2):
        c = _section_coefs(sos[sec], LD)
        y = _biquad_loop(c, y) if loop else _biquad_ld(c, y)
    return y


def _zero_state_blocks(c, x, block):
    """Every block of x (zero-padded to whole blocks) through one section from z = 0 -> (y [len(x)], zend [nb x 2])."""
    b0, b1, b2, a1, a2 = c
    nb = (x.size + block - 1) // block
    xp = np.zeros(nb * block)
    xp[:x.size] = x
    xp = xp.reshape(nb, block)
    y = np.empty_like(xp)
    z0, z1 = np.zeros(nb), np.zeros(nb)
    for n in range(block):
        xv = xp[:, n]
        yv = b0 * xv + z0
        z0 = b1 * xv + z1 - a1 * yv
        z1 = b2 * xv - a2 * yv
        y[:, n] = yv
    return y.reshape(-1)[:x.size], np.stack((z0, z1), axis=1)


def _carry_scan(pm, zend):
    """k_hpf_carry: z_{j+1} = P z_j + e_j, 64 blocks per step as a scan across the lanes -> zstart [nb x 2]."""
    nb = zend.shape[0]
    pw = [np.asarray(pm, dtype=np.float64).reshape(2, 2)]
    for _ in range(6):
        pw.append(pw[-1] @ pw[-1])
    t = np.arange(64)
    q = np.tile(np.eye(2), (64, 1, 1))
    for k in range(6):
        on = ((t >> k) & 1) == 1
        q[on] = q[on] @ pw[k]
    zstart = np.zeros((nb, 2))
    zt = np.zeros(2)
    for g in range(0, nb, 64):
        cnt = min(64, nb - g)
        e = np.zeros((64, 2))
        e[:cnt] = zend[g:g + cnt]
        c = e.copy()
        for k in range(6):
            s = 1 << k
            o = np.zeros((64, 2))
            o[s:] = c[:-s]
            c[s:] = c[s:] + o[s:] @ pw[k].T
        m = np.zeros((64, 2))
        m[1:] = c[:-1]
        zs = q @ zt + m
        zstart[g:g + cnt] = zs[:cnt]
        nxt = zs @ pw[0].T + e
        zt = nxt[cnt - 1]
    return zstart


def hpf_blocked(sos, pmat, gtab, x, block=HPF_BLOCK):
    """mpx_output_hpf's algorithm in float64 on one utterance (x float32 or float64) -> float64 [len(x)]."""
    x = np.asarray(x).astype(np.float64)
    if x.size == 0:
        return x
    gtab = np.asarray(gtab, dtype=np.float64)
    r = np.arange(x.size) % block
    j = np.arange(x.size) // block
    # section 0: zero-state pass and carry; its free response is NOT applied to y_tmp ...
    y_tmp, zend = _zero_state_blocks(_section_coefs(sos[0], np.float64), x, block)
    zs0 = _carry_scan(pmat[0], zend)
    # ... but added while section 1 loads: x1[n] = y_tmp[n] + G0[n mod block] . zstart0[block of n]
    x1 = y_tmp + (gtab[0, r, 0] * zs0[j, 0] + gtab[0, r, 1] * zs0[j, 1])
    y, zend = _zero_state_blocks(_section_coefs(sos[1], np.float64), x1, block)
    zs1 = _carry_scan(pmat[1], zend)
    return y + (gtab[1, r, 0] * zs1[j, 0] + gtab[1, r, 1] * zs1[j, 1])


def hpf_input(name, design, fs, lens=HPF_LENS):
    """The float32 utterances of one batch (peak 1, 1.001 for dc_noise)."""
    out = []
    for i, n in enumerate(lens):
        k = np.arange(n)
        if name == "noise":
            x = np.random.RandomState(1000 + i).uniform(-1, 1, n)
        elif name == "dc":
            x = np.ones(n)
        elif name in ("impulse0", "impulse255"):
            x = np.zeros(n)
            at = 0 if name == "impulse0" else 255
            if n > at:
                x[at] = 1.0
        elif name == "alternating":
            x = 1.0 - 2.0 * (k % 2)
        elif name == "corner_sine":
            x = np.sin(2.0 * np.pi * HPF_CORNER[design] * k / fs)
        elif name == "dc_noise":   # the cancellation case: large zero-state responses per block that the carries must cancel
            x = 1.0 + 1e-3 * np.random.RandomState(2000 + i).uniform(-1, 1, n)
        else:
            raise ValueError(name)
        out.append(x.astype(np.float32))
    return out


_HPF_REF = {}


def hpf_reference(design, fs, name):
    """(utterances float32, hpf_cascade of each) of one batch; computed once per session, never modified."""
    key = (design, int(fs), name)
    if key not in _HPF_REF:
        from magphase_amd import hostmath as hm
        sos = hm.hpf_tables(fs, HPF_BLOCK, design)[0]
        sigs = hpf_input(name, design, fs)
        refs = [hpf_cascade(sos, x) for x in sigs]
        for a in sigs + refs:
            a.setflags(write=False)
        _HPF_REF[key] = (sigs, refs)
    return _HPF_REF[key]


def block_offsets(lens, block=HPF_BLOCK):
    lens = np.asarray(lens, dtype=np.int64)
    return np.concatenate(([0], np.cumsum((lens + block - 1) // block))).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------------
# 16-bit PCM
# ---------------------------------------------------------------------------------------------------------------------
def pcm16(y, norm):
    """la.write_audio_file's samples, operation for operation: norm * y / max|y| (norm None: as they are), * 32767.0,
    np.rint (half to even), NaN -> 0 (a silent utterance: 0 / 0), clip to int16."""
    v = np.asarray(y).astype(np.float64)
    if norm is not None:
        with np.errstate(invalid="ignore", divide="ignore"):
            v = norm * v / (np.max(np.abs(v)) if v.size else 1.0)
    p = np.rint(v * 32767.0)
    p[np.isnan(p)] = 0.0
    return np.clip(p, -32768.0, 32767.0).astype(np.int16)


def pcm16_to_f32(p):
    """int16 -> float32 in [-1, 1): p * 2^-15, exact."""
    return (np.asarray(p, dtype=np.int16).astype(np.float64) * 2.0 ** -15).astype(np.float32)


def pcm16_ties():
    """y[k] = (k + 0.5) / 32767 for the 65 535 k in -32768 .. 32766: y * 32767.0 == k + 0.5 exactly in float64."""
    k = np.arange(-32768, 32767, dtype=np.float64)
    return k, (k + 0.5) / 32767.0


# ---------------------------------------------------------------------------------------------------------------------
# Merlin post-filter
# ---------------------------------------------------------------------------------------------------------------------
MAGIC = -1.0E+10   # la.MAGIC (asserted by the tests)
MERLIN_DIMS = (3, 24, 60, 64)
MERLIN_FS = (48000, 16000)
MERLIN_FRAMES = (1, 63, 64, 65, 257)
MERLIN_ROWS = 257   # the F = 257 input; a launch of F frames takes its first F rows
MERLIN_UNIQUE = 33  # row f is row f mod MERLIN_UNIQUE: the oracle runs frame by frame (0.01 s each), 33 frames per reference
MERLIN_SILENT = 4   # ... the last MERLIN_SILENT of which are constant -23


def _f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def log_mel_mags(n_frames, dim, seed):
    """Log mel magnitudes with three formants per frame (the generator of tests/test_post_filter_merlin.py, any dim)."""
    rng = np.random.RandomState(seed)
    k = np.arange(dim)
    out = []
    for _ in range(n_frames):
        f1, f2, f3 = rng.uniform(4, 12), rng.uniform(15, 28), rng.uniform(32, 50)
        env = -0.04 * k + 2.2 * np.exp(-0.5 * ((k - f1) / 2.0) ** 2) + 1.6 * np.exp(-0.5 * ((k - f2) / 2.5) ** 2) \
            + 1.0 * np.exp(-0.5 * ((k - f3) / 3.0) ** 2)
        out.append(env + rng.uniform(-6, -2))
    return np.array(out).reshape(n_frames, dim)


def merlin_input(dim):
    """[MERLIN_ROWS x dim] float32 values as float64: formant rows and constant -23 rows (silence), row f = row f mod 33."""
    x = log_mel_mags(MERLIN_UNIQUE, dim, seed=100 + dim)
    x[MERLIN_UNIQUE - MERLIN_SILENT:] = -23.0
    return _f32(x[np.arange(MERLIN_ROWS) % MERLIN_UNIQUE])


def merlin_stages(x, tables, pipe=True):
    """mpx_post_filter_merlin launch by launch in float64 from hostmath.merlin_tables(...):
      k_rows_gemm  mcep = x c1, mcep_w = mcep * lifter      k_merlin_r0  r0, p_r0 = sum_k wk exp(2 (c g)[k])
      k_merlin_b   mcep_pf = b2mc(mc2b(mcep_w) with b[0] += ln(r0 / p_r0) / 2)      k_rows_gemm  out = mcep_pf cf, NaN -> MAGIC
    pipe: round to float32 where the device stores float32 (and the SPTK chain pipes float32)."""
    p = _f32 if pipe else (lambda a: np.asarray(a, dtype=np.float64))
    x = np.asarray(x, dtype=np.float64)
    c1, lifter, g, wk, cf = (np.asarray(tables[k], dtype=np.float64) for k in ("c1", "lifter", "g", "wk", "cf"))
    alpha = float(tables["alpha"])
    with np.errstate(all="ignore"):
        mcep = p(x @ c1)
        mcep_w = p(mcep * p(lifter))
        r0 = p(np.exp(2.0 * (mcep @ g)) @ wk)
        p_r0 = p(np.exp(2.0 * (mcep_w @ g)) @ wk)
        b = np.array(mcep_w)
        for m in range(b.shape[1] - 2, -1, -1):
            b[:, m] -= alpha * b[:, m + 1]
        b = p(b)
        b[:, 0] = p(p(np.log(p(r0 / p_r0)) / 2.0) + b[:, 0])
        mcep_pf = np.array(b)
        mcep_pf[:, :-1] += alpha * b[:, 1:]
        mcep_pf = p(mcep_pf)
        out = mcep_pf @ cf
    out[np.isnan(out)] = MAGIC
    return dict(mcep=mcep, mcep_w=mcep_w, r0=r0, p_r0=p_r0, mcep_pf=mcep_pf, out=out)


_MERLIN_REF = {}


def merlin_reference(dim, fs, pf_coef=1.4):
    """(input [MERLIN_ROWS x dim], oracle output) -- the oracle works frame by frame, so a launch of F frames is compared
    with the first F rows.  Computed once per session, never modified."""
    key = (int(dim), int(fs), float(pf_coef))
    if key not in _MERLIN_REF:
        from oracle import magphase_oracle as orc
        x = merlin_input(dim)
        want = orc.post_filter_merlin(x[:MERLIN_UNIQUE], fs, pf_coef=pf_coef)[np.arange(MERLIN_ROWS) % MERLIN_UNIQUE]
        x.setflags(write=False)
        want.setflags(write=False)
        _MERLIN_REF[key] = (x, want)
    return _MERLIN_REF[key]
