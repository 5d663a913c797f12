/*
 * magphase_hip.h -- C ABI of libmagphase_hip.so: the MI355X (gfx950) implementation of the MagPhase
 * per-frame analysis / synthesis hot path.
 *
 * The reference (CSTR-Edinburgh/magphase) has no FFI: its boundary is the Python module API of
 * src/magphase.py.  These entry points are what magphase_amd/magphase.py binds through ctypes in
 * place of the numpy loops cited on each function; INTEGRATION.md shows the reference-side stub.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host; the caller owns all buffers
 *     (PyTorch-ROCm tensors are only the allocator); nothing is allocated or freed here;
 *   - `stream` is a hipStream_t (passed as void*); all work is enqueued on it, nothing synchronises;
 *   - fft_len N is 4096, 2048 or 1024; H = N/2+1; feature matrices are row-major float32 [F x H];
 *   - return 0 on success, <0 on error (text via mpx_last_error()); re-entrant per stream.
 */
#ifndef MAGPHASE_HIP_H
#define MAGPHASE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPX_ABI_VERSION 2

#define MPX_OK 0
#define MPX_ERR_ARG (-1)     /* bad argument (unsupported fft_len, null pointer, negative count) */
#define MPX_ERR_HIP (-2)     /* a HIP runtime call failed */
#define MPX_ERR_HOST (-3)    /* a host-side helper ran out of memory (or threw) in one of its worker threads */

int mpx_version(void);
const char* mpx_last_error(void);

/* Number of bytes of the per-fft_len twiddle table, and its initialisation (a small kernel enqueued on `stream`
 * evaluates it in float64 and rounds to float32: no host copy, no synchronisation).  The table is read-only
 * afterwards and may be shared by every stream of the device. */
size_t mpx_tables_bytes(int fft_len);
int mpx_tables_init(void* stream, int fft_len, void* tables);

/*
 * Analysis of pitch-synchronous frames.  Replaces, for all frames of a batch at once:
 *   magphase.py:74-119   windowing()               (Hann half windows, frame = sig[pm-left .. pm+right])
 *   magphase.py:309-323  zero-pad/truncate to N, circular rotation (epoch -> index 0)
 *   magphase.py:325      np.fft.fft, first H bins
 *   magphase.py:457-476  compute_lossless_feats(): mag=|X|, real=Re X/|X|, imag=Im X/|X| (0 where |X|==0)
 * sig        : float32 PCM of all utterances of the batch, concatenated
 * frame_pos  : int64[n_frames]  absolute index in `sig` of each frame's epoch (utterance offset + pm)
 * frame_left : int32[n_frames]  left length  (pm - previous epoch; == v_shift of the reference)
 * frame_right: int32[n_frames]  right length (next epoch - pm)
 * out_*      : float32 [n_frames x H], row pitch `ld` floats (ld >= H; dense ld == H is the fastest, see mpx_feat_ld)
 * The host keeps the fp64 epoch/index math (np.round, int casts) -- it is never recomputed on the device.
 */
int mpx_analysis_frames(void* stream, int fft_len, const void* tables, const float* sig,
                        const int64_t* frame_pos, const int32_t* frame_left, const int32_t* frame_right,
                        int64_t n_frames, float* out_mag, float* out_real, float* out_imag, int64_t ld);

/*
 * The same analysis with the window, the transform and the epilogue in float64 (features still float32: correctly
 * rounded values of the reference's float64 features instead of values carrying the fp32 FFT's ~1e-6-of-peak noise).
 * For callers whose next step amplifies that noise on weak bins -- the compressed analysis takes ln(mag^2 + 1e-8)
 * and uses Re X/|X| of bins 60-80 dB below the frame peak (magphase.py:2508-2521, libaudio.py:575-601).  About twice
 * the time of mpx_analysis_frames (float64 vector rate, 8 waves per CU).  tables_f64: mpx_tables_f64_bytes() bytes
 * initialised by mpx_tables_f64_init() (float64 twiddles; same life cycle as mpx_tables_init's table).
 * rows_in_use [n_frames] (DEVICE) or NULL: frames with a 0 get their magnitude row only -- out_real / out_imag keep what
 * they held (the compressed analysis never reads the phase features of rows no voiced frame interpolates from:
 * mpx_mel_warp_rows' rows_in_use).
 */
size_t mpx_tables_f64_bytes(int fft_len);
int mpx_tables_f64_init(void* stream, int fft_len, void* tables);
int mpx_analysis_frames_f64(void* stream, int fft_len, const void* tables_f64, const float* sig,
                            const int64_t* frame_pos, const int32_t* frame_left, const int32_t* frame_right,
                            int64_t n_frames, float* out_mag, float* out_real, float* out_imag, int64_t ld,
                            const float* rows_in_use);

/*
 * mpx_analysis_frames_f64 with the WINDOW WEIGHTS READ FROM A HOST-BUILT TABLE instead of evaluated on the device:
 * win_tab (DEVICE, float64) holds, for every half length h <= win_cap, the rising half np.hanning(2 h + 1)[0 .. h] at
 * offset h (h + 1) / 2 -- (win_cap + 1)(win_cap + 2) / 2 doubles, built by the host's numpy (hostmath.hann_half_table), i.e.
 * by the very function the reference windows with (libaudio.py:70-84).  The products sample x weight are then the
 * reference's own float64 values, and a bin that cancels exactly carries the reference's own residue (0.0 or a few 2^-53,
 * with its sign) instead of being flushed to zero.  Frames with a half longer than win_cap use the analytic window.
 * win_tab == NULL: exactly mpx_analysis_frames_f64.
 */
int mpx_analysis_frames_f64w(void* stream, int fft_len, const void* tables_f64, const float* sig,
                             const int64_t* frame_pos, const int32_t* frame_left, const int32_t* frame_right,
                             int64_t n_frames, float* out_mag, float* out_real, float* out_imag, int64_t ld,
                             const float* rows_in_use, const double* win_tab, int32_t win_cap);

/*
 * FUSED compressed analysis at the variable frame rate (magphase.py:2947-2988 with b_const_rate=False: analysis_lossless ->
 * format_for_modelling; SURVEY.md section 8d, configuration C4 "fused; lossless features never hit HBM"): float64 analysis
 * of every frame (as mpx_analysis_frames_f64w) -> log power / unit phasor of every bin -> both mel warps on the matrix
 * cores -> voicing mask and clip, in ONE kernel; the [n_frames x H] lossless features are never written.
 *   wpack, whalf : the two warp matrices in MFMA fragment order (hostmath.pack_warp_fused of the [mag_dim x H] and
 *                  [phase_dim x H] matrices mpx_mel_warp takes, in the layout mpx_analysis_compressed_fused_layout()
 *                  names; DEVICE, float32)
 *   voiced       : float32[n_frames] (DEVICE): 0 = unvoiced frame, phase outputs +0 (magphase.py:2527-2529)
 *   mag_fbank    : 0 = cepstral mel warp of ln(mag^2 + 1e-8) (la.sp_mel_warp), 1 = mel filter bank (la.sp_mel_warp_fbank)
 *   out_mag [n_frames x mag_dim], out_real / out_imag [n_frames x phase_dim], dense float32
 * mag_dim <= 64, phase_dim <= 48, fft_len 2048 or 4096.  Equals mpx_analysis_frames_f64w followed by mpx_mel_warp up to the
 * float32 summation order of the warp.
 */
int mpx_analysis_compressed_fused(void* stream, int fft_len, const void* tables_f64, const float* sig,
                                  const int64_t* frame_pos, const int32_t* frame_left, const int32_t* frame_right,
                                  int64_t n_frames, const double* win_tab, int32_t win_cap, const float* wpack,
                                  const float* whalf, int32_t mag_dim, int32_t phase_dim, const float* voiced,
                                  int32_t mag_fbank, float* out_mag, float* out_real, float* out_imag);
/*
 * The same at the CONSTANT frame rate (analysis_compressed_type1(..., const_rate_ms=5.0), magphase.py:2967-2983: the
 * lossless features are interpolated to the 5 ms grid by interp_from_variable_to_const_frm_rate, :2219-2239, BEFORE
 * format_for_modelling, :2490-2544).  Constant-rate frame c lies between the frames row0[c] and row1[c] (== row0[c] + 1, or
 * == row0[c] for the duplicated first row; row1 ascending over the batch) with weight row_t[c]:
 *   out_mag [n_const x mag_dim]            ln((|X_row0| + t (|X_row1| - |X_row0|))^2 + 1e-8) . W_mag -- the operand rows of
 *                                          the matrix product are built per constant-rate frame inside the kernel;
 *   tmp_real / tmp_imag [n_frames x phase_dim]   the phase streams' warp of the VARIABLE-rate frames with rows_in_use != 0
 *                                          (no mask, no clip), to be finished by mpx_warp_phase_rows -- the split
 *                                          mpx_mel_warp_rows makes.
 * wpack / whalf as for mpx_analysis_compressed_fused (layout 1, eight waves; mel-warp magnitudes only).  work: DEVICE
 * scratch of mpx_analysis_compressed_fused_cr_work_bytes(fft_len, n_frames) bytes (an index of row1 and 8 KB per
 * workgroup for the frame a round hands to the next).  The lossless features never reach HBM.
 */
int mpx_analysis_compressed_fused_cr(void* stream, int fft_len, const void* tables_f64, const float* sig,
                                     const int64_t* frame_pos, const int32_t* frame_left, const int32_t* frame_right,
                                     int64_t n_frames, const double* win_tab, int32_t win_cap, const float* wpack,
                                     const float* whalf, int32_t mag_dim, int32_t phase_dim, const float* rows_in_use,
                                     const int32_t* row0, const int32_t* row1, const float* row_t, int64_t n_const,
                                     float* out_mag, float* tmp_real, float* tmp_imag, void* work);
int64_t mpx_analysis_compressed_fused_cr_work_bytes(int fft_len, int64_t n_frames);
/* column tiles of 16 the fused kernel runs for the magnitude / phase job (what pack_warp_fused must produce) */
int mpx_analysis_compressed_fused_tiles(int32_t mag_dim, int32_t phase_dim, int32_t* ntm, int32_t* ntp);
/* waves per workgroup = frames per round = K slices the packed weights are cut into (pack_warp_fused's n_waves) */
int mpx_analysis_compressed_fused_waves(void);
/* fragment layout of `wpack` this build's mpx_analysis_compressed_fused expects (pack_warp_fused's `layout`): 0 = one
 * v_mfma_f32_16x16x4_f32 fragment per column tile; 1 = the magnitude product on v_mfma_f32_4x4x1_16b_f32 (eight
 * fragments [bin group][half of the 64 coefficients] per wave and chunk), then the phase tiles' fragments */
int mpx_analysis_compressed_fused_layout(void);
/* resident workgroups per CU of the fused kernel (the runtime's occupancy query), < 0 on error: diagnostics */
int mpx_analysis_compressed_fused_blocks_per_cu(int fft_len, int32_t phase_dim);

/*
 * Row pitch (in floats) the lossless feature matrices should be allocated with.  Any ld >= H is CORRECT for every
 * entry point that takes `ld` (so the matrices may live inside wider buffers); mpx_feat_ld() returns the pitch
 * measured fastest on MI355X, which is the reference's dense [F x H] layout, ld == H: padding the rows to a
 * multiple of 32 or 64 floats leaves one partially written 128-byte line per row (the lone Nyquist bin) and costs
 * 7 % of the analysis kernel.  Returns 0 for an unsupported fft_len.
 */
int64_t mpx_feat_ld(int fft_len);

/*
 * Lossless synthesis, per-frame part.  Replaces magphase.py:1761-1770 (synthesis_from_lossless):
 *   X = mag * (real + j imag)/|real + j imag|  (|.|==0 -> 1), Hermitian extension with Im X[0]=Im X[N/2]=0
 *   (libaudio.py:369-388), np.fft.ifft(.).real, np.fft.fftshift  (epoch at index N/2).
 * mag/real/imag : float32 [n_frames x H], row pitch `ld` floats
 * frames_out : float32 [n_frames x N]
 */
int mpx_synthesis_lossless_frames(void* stream, int fft_len, const void* tables, const float* mag,
                                  const float* real, const float* imag, int64_t n_frames, float* frames_out,
                                  int64_t ld);

/*
 * PSOLA overlap-add, gather form, deterministic (ascending frame order).  Replaces magphase.py:34-62 ola():
 * for utterance u, out[t] = sum_i frames[i][t + out_start[u] - pm_rel[i]] over its frames i with
 * 0 <= t + out_start[u] - pm_rel[i] < N, for t in [0, out_off[u+1]-out_off[u]).
 * utt_frame_off : int32[n_utts+1]  frame range of each utterance
 * pm_rel        : int32[n_frames]  pm_i - pm_0 within the utterance (non-decreasing)
 * out_start     : int32[n_utts]    first kept sample of the OLA buffer (python slice start N/2 - pm_0, resolved on host)
 * out_off       : int64[n_utts+1]  sample offsets of each utterance in pcm_out
 * max_out_len   : max over utterances of the output length (grid sizing)
 */
int mpx_ola_gather(void* stream, int fft_len, const float* frames, int32_t n_utts, const int32_t* utt_frame_off,
                   const int32_t* pm_rel, const int32_t* out_start, const int64_t* out_off, int64_t max_out_len,
                   float* pcm_out);

/*
 * Fused lossless synthesis + PSOLA (the production path; the two calls above stay as the reference form).
 * Replaces magphase.py:1759-1776 (synthesis_from_lossless) + :34-62 (ola) for a batch.
 * The frames of every utterance are cut into RUNS of consecutive frames (host: hostmath.ola_runs).  A run is
 * overlap-added, in ascending frame order, in an on-chip ring buffer by one wavefront pair; finished samples go
 * straight to pcm_out, except the first head_end elements of a run that has a predecessor in its utterance -- those
 * positions also receive the predecessor's last frames -- which go to the run's head strip and are added to pcm_out by
 * mpx_ola_fixup afterwards (predecessor's sum + head strip: a fixed order, so the result is deterministic; it differs
 * from the reference's single ascending sum only by fp32 re-association).  Runs of one utterance must be long
 * enough that only ADJACENT runs overlap: pm_rel[frame_end] - pm_rel[frame_begin - 1] >= N for every run that has
 * both neighbours (hostmath.ola_runs guarantees it).
 * Element coordinates e of a run are OLA-buffer positions (magphase.py:38) minus x0.
 */
typedef struct mpx_ola_run {
    int32_t frame_begin, frame_end; /* global frame indices: rows of mag/real/imag, entries of pm_rel */
    int32_t x0;                     /* OLA-buffer position of element 0; chosen so that out_base is a multiple of 64 */
    int32_t head_end;               /* elements e < head_end go to the head strip (0: first run of its utterance) */
    int32_t out_lo, out_hi;         /* elements out_lo <= e < out_hi are written to pcm_out[out_base + e] */
    int32_t flush_end;              /* the ring is streamed out and cleared up to this element when the run ends */
    int32_t fix_lo, fix_hi;         /* mpx_ola_fixup: pcm_out[out_base + e] += strip[e] for fix_lo <= e < fix_hi */
    int32_t pad;
    int64_t out_base;               /* pcm_out index of element 0 (may be negative) */
    int64_t strip_off;              /* float offset of the head strip in `strips`; head_end <= mpx_ola_strip_floats() */
} mpx_ola_run;

/* slot_off : int32[n_slots+1], slot_runs : int32[n_runs] -- work list: pair slot s processes the runs
 *            slot_runs[slot_off[s] .. slot_off[s+1]) in that order (the host balances the lists for
 *            mpx_synth_ola_slots() slots; with runs of equal length every slot gets one)
 * pm_rel   : int32[n_frames]  pm_i - pm_0 within the utterance (as mpx_ola_gather)
 * strips   : float32 [n_runs x mpx_ola_strip_floats(fft_len)]
 * pcm_out  : float32, the utterances' outputs concatenated (every kept sample is written exactly once by
 *            mpx_synthesis_lossless_ola; mpx_ola_fixup then adds the head strips) */
int mpx_synth_ola_slots(void); /* pair slots the current device runs concurrently (CUs x pairs per workgroup) */
/* Relative speed of the slots (HOST float32[n_slots], n_slots = mpx_synth_ola_slots()): a SIMD serves its resident waves
 * by age, so the wave groups of a workgroup run at different, fixed rates; the planner (hostmath.ola_runs) deals the frames
 * of a batch in proportion to these weights so that all slots finish together. */
int mpx_synth_ola_slot_weights(float* weights_host, int32_t n_slots);
int64_t mpx_ola_strip_floats(int fft_len); /* floats per head strip: fft_len + 64 */
int mpx_synthesis_lossless_ola(void* stream, int fft_len, const void* tables, const float* mag, const float* real,
                               const float* imag, const mpx_ola_run* runs, int32_t n_runs, const int32_t* slot_off,
                               const int32_t* slot_runs, int32_t n_slots, const int32_t* pm_rel, float* strips,
                               float* pcm_out, int64_t ld /* row pitch of mag/real/imag */);
int mpx_ola_fixup(void* stream, int fft_len, const mpx_ola_run* runs, int32_t n_runs, const float* strips,
                  float* pcm_out);
/* The same with the launch sized by the run table's widest fix range: max_width = the largest fix_hi - (fix_lo & ~63) of
 * the runs (0 <= max_width <= fft_len + 127; 0: nothing to fix, no launch).  Ranges wider than max_width are not completed. */
int mpx_ola_fixup_width(void* stream, int fft_len, const mpx_ola_run* runs, int32_t n_runs, const float* strips,
                        float* pcm_out, int32_t max_width);
/*
 * mpx_synthesis_lossless_ola with row tables (constant-rate lossless synthesis, magphase.py:2242-2252 + :1759-1776):
 * frame f is synthesised from the row (1 - row_t[f]) x[row0[f]] + row_t[f] x[row1[f]] of each of mag / real / imag
 * (int32 / float32 [frames]; 0 <= row0, row1 < rows of the matrices -- the caller's promise), interpolated in registers as
 * the kernel loads the two rows.  Everything else as mpx_synthesis_lossless_ola (same slots, weights, strips;
 * mpx_ola_fixup afterwards).
 */
int mpx_synthesis_lossless_ola_lerp(void* stream, int fft_len, const void* tables, const float* mag, const float* real,
                                    const float* imag, const int32_t* row0, const int32_t* row1, const float* row_t,
                                    const mpx_ola_run* runs, int32_t n_runs, const int32_t* slot_off,
                                    const int32_t* slot_runs, int32_t n_slots, const int32_t* pm_rel, float* strips,
                                    float* pcm_out, int64_t ld);

/*
 * Row interpolation of the three lossless feature streams: dst_X[c] = (1 - row_t[c]) src_X[row0[c]] + row_t[c] src_X[row1[c]]
 * for c < n_out, bins 0..n_bins-1 (X = mag / real / imag; row pitches ld_src / ld_dst in floats, >= n_bins; row indices
 * within the source -- the caller's promise).  Variable -> constant rate (magphase.py:2219-2239, the constant-rate lossless
 * analysis) and constant -> variable rate (:2242-2252, the staged form of mpx_synthesis_lossless_ola_lerp).
 */
int mpx_rows_lerp(void* stream, int32_t n_bins, const float* src_mag, const float* src_real, const float* src_imag,
                  int64_t ld_src, const int32_t* row0, const int32_t* row1, const float* row_t, int64_t n_out,
                  float* dst_mag, float* dst_real, float* dst_imag, int64_t ld_dst);

/*
 * Backward pass of mpx_synthesis_lossless_ola / mpx_synthesis_lossless_ola_lerp (magphase.py:1759-1776, ola :34-62): from
 * grad_out = dL/d pcm_out (float32 [total_out], the utterances where the forward wrote them) the gradients with respect to
 * the rows of mag / real / imag.  irfft and the overlap-add are linear, so frame f needs only the fft_len gradient samples
 * that lie under it: sample n of its window is grad_out[grad_pos[f] + n], read for grad_lo[f] <= n < grad_hi[f] and zero
 * elsewhere (the part of the frame inside its own utterance's kept output; hostmath.lossless_backward_table builds the
 * three tables from the plan: grad_pos = out_off[u] + pm_rel[f] - out_start[u]).  Reads are also clamped to
 * [0, total_out) on the device, whatever the tables say.  Per frame: one forward FFT of the window rotated by fft_len/2,
 * gX_k = (c_k / fft_len) G_k (c_k = 2, 1 at bins 0 and fft_len/2, whose imaginary parts are dropped), and with
 * u = (real + j imag) / den, den = |real + j imag| (1 where that is 0), d = Re(conj(u) gX):
 *     grad_mag = d,   grad_real = (mag / den) (Re gX - Re u d),   grad_imag = (mag / den) (Im gX - Im u d).
 * mag / real / imag (row pitch ld) are the forward's inputs.  row0 / row1 / row_t: all null (frame f reads row f) or the
 * forward's row tables (frame f reads fma(x[row1[f]] - x[row0[f]], row_t[f], x[row0[f]]), the forward's own arithmetic);
 * either way the gradient rows are per FRAME: grad_X + f * ld_grad, [n_frames x fft_len/2 + 1] -- with row tables
 * mpx_rows_lerp_adjoint folds them back onto the constant-rate rows.  A null grad_X is not computed; all three null
 * launches nothing.  Every element of a non-null grad_X is written exactly once: no atomics, deterministic.
 */
int mpx_synthesis_lossless_backward(void* stream, int fft_len, const void* tables, const float* grad_out,
                                    int64_t total_out, const int64_t* grad_pos, const int32_t* grad_lo,
                                    const int32_t* grad_hi, int64_t n_frames, const float* mag, const float* real,
                                    const float* imag, int64_t ld, const int32_t* row0, const int32_t* row1,
                                    const float* row_t, float* grad_mag, float* grad_real, float* grad_imag,
                                    int64_t ld_grad);

/*
 * Backward pass of mpx_synthesis_compressed_ola (synthesis_from_compressed, magphase.py:825-997; per_phase_type
 * 'magphase', no post-filter): from grad_out = dL/d pcm_out BEFORE the output high-pass (float32 [total_out]) the gradients
 * with respect to the frames' unwarped rows mag / real / imag (row pitch ld, one row per FRAME: what mpx_mel_unwarp_rows
 * wrote).  grad_pos / grad_lo / grad_hi: as for mpx_synthesis_lossless_backward (hostmath.lossless_backward_table; reads are
 * also clamped to [0, total_out) on the device).  noise .. noise_wtype, voiced, inv_gain, win_left / win_right, per_v / ap_v /
 * ap_u and n_per are the forward's own arguments.  Per frame f and bin k, with N = fft_len:
 *     Ns  = FFT_N of the frame's windowed, rotated noise (recomputed; not bit-identical to the forward's compact form),
 *     u   = (real + j imag) / den, den = |real + j imag| (u = 0 where that is 0),
 *     T   = P u + A inv_gain[f] Ns,  P = per_v (voiced, k < n_per) / 0,  A = ap_v (voiced) / ap_u,
 *     gS  = (c_k / N) FFT_N(ifftshift(w_f g))_k, w_f the anti-ringing window (win_left, win_right), g the gradient samples
 *           under the frame, c_k = 2 and 1 at bins 0 and N/2, where gS <- Re(gS) S / |S| with S = mag T (0 where S == 0),
 *     grad_mag = Re(conj(T) gS),   grad_real + j grad_imag = (mag P / den) (gS - u Re(conj(u) gS))   (den == 0: mag P gS).
 * grad_mag is written over all fft_len/2 + 1 bins of row f (pitch ld_grad); grad_real / grad_imag over the first
 * min(64 ceil(n_per / 64), fft_len/2 + 1) bins -- zeros in unvoiced frames and from n_per on -- and nowhere else.  The phase
 * rows of unvoiced frames and the bins from n_per on are not read (the forward does not produce them).  A null grad_X is not
 * computed; all three null launches nothing.  Every element named above of a non-null grad_X is written exactly once: no
 * atomics, deterministic.  Arguments are checked before the device is touched.
 */
int mpx_synthesis_compressed_backward(void* stream, int fft_len, const void* tables, const float* grad_out,
                                      int64_t total_out, const int64_t* grad_pos, const int32_t* grad_lo,
                                      const int32_t* grad_hi, int64_t n_frames, const float* mag, const float* real,
                                      const float* imag, int64_t ld, const float* noise, const int64_t* noise_pos,
                                      const int32_t* noise_left, const int32_t* noise_right, const int32_t* noise_wtype,
                                      const int32_t* voiced, const float* inv_gain, const int32_t* win_left,
                                      const int32_t* win_right, const float* per_v, const float* ap_v, const float* ap_u,
                                      int32_t n_per, float* grad_mag, float* grad_real, float* grad_imag,
                                      int64_t ld_grad);

/*
 * Backward pass of mpx_synthesis_compressed_type2_ola (synthesis_from_compressed_type2, magphase.py:1452-1597): the
 * arguments, the argument checks and the results of mpx_synthesis_compressed_backward, with the type-2 assembly at bins 0
 * and N/2: the forward keeps Re S there (not |S|), so gS <- (Re gS, 0) at those two bins and no projection on S / |S|.
 * per_v / ap_v / ap_u are the type-2 curves, inv_gain[f] is 1 / rms_noise of the frame's utterance (mpx_noise_rms), n_per
 * the first bin from which per_v is zero.  grad_imag at bins 0 and N/2 is -(mag P / den) u_i u_r Re gS: in general not zero.
 */
int mpx_synthesis_compressed_type2_backward(void* stream, int fft_len, const void* tables, const float* grad_out,
                                            int64_t total_out, const int64_t* grad_pos, const int32_t* grad_lo,
                                            const int32_t* grad_hi, int64_t n_frames, const float* mag, const float* real,
                                            const float* imag, int64_t ld, const float* noise, const int64_t* noise_pos,
                                            const int32_t* noise_left, const int32_t* noise_right,
                                            const int32_t* noise_wtype, const int32_t* voiced, const float* inv_gain,
                                            const int32_t* win_left, const int32_t* win_right, const float* per_v,
                                            const float* ap_v, const float* ap_u, int32_t n_per, float* grad_mag,
                                            float* grad_real, float* grad_imag, int64_t ld_grad);

/*
 * Adjoint of the row interpolation out[f] = fma(x[row1[f]] - x[row0[f]], row_t[f], x[row0[f]]):
 *     dst_X[r] = sum over f with row0[f] == r of (1 - row_t[f]) src_X[f] + sum over f with row1[f] == r of row_t[f] src_X[f]
 * for r < n_rows (a frame with row0 == row1 == r weighs exactly 1).  ranges: int32 [n_rows x 4] = (a0, a1, b0, b1) per
 * row, the frames with row0 == r are [a0, a1), those with row1 == r are [b0, b1) (hostmath.lerp_adjoint_table; the row
 * tables are non-decreasing, so both sets are contiguous); row_t [frames].  One wavefront per row sums in ascending frame
 * order: deterministic, no atomics; a row no frame reads gets zeros.  A null dst_X (with any src_X) is skipped.
 */
int mpx_rows_lerp_adjoint(void* stream, int32_t n_bins, const float* src_mag, const float* src_real,
                          const float* src_imag, int64_t ld_src, const int32_t* ranges, const float* row_t,
                          int64_t n_rows, float* dst_mag, float* dst_real, float* dst_imag, int64_t ld_dst);

/*
 * Backward pass of mpx_analysis_frames (magphase.py:74-119, :266-334, :457-476): from grad_mag / grad_real / grad_imag =
 * dL/d(out_mag, out_real, out_imag) (rows f * ld_grad, [n_frames x fft_len/2 + 1]) and the forward's own output rows
 * mag / real / imag (row pitch ld) the gradient with respect to the samples, grad_sig float32 [total_smpls].  Per frame,
 * with N = fft_len, L / R = frame_left / frame_right, len = min(L + R + 1, N), rot = L if L < N else 0:
 *     d = real grad_real + imag grad_imag,
 *     gX = grad_mag (real + j imag) + ((grad_real + j grad_imag) - (real + j imag) d) / mag,
 *          and gX = 0 where mag^2 < 1e-37 (the forward's clamp region, which holds X == 0: silent frames give zeros),
 *     b = N irfft_N(Y), Y_k = gX_k / 2 for 0 < k < N/2, Y_0 = Re gX_0, Y_{N/2} = Re gX_{N/2},
 *     gfrm[k] = b[(k - rot) mod N] w(k) for 0 <= k < len (w: the forward's window),
 *     grad_sig[frame_pos - L + k] += gfrm[k].
 * Two launches: the frames' len samples go to `scratch` at scratch_off[f] (int64 [n_frames + 1], scratch_off[f + 1] -
 * scratch_off[f] = len: hostmath.analysis_backward_table; scratch_floats >= scratch_off[n_frames]), then one thread per
 * sample adds the frames that cover it in ascending frame order -- frame starts and ends must be non-decreasing, as they
 * are for the batches the plans build.  Every element of grad_sig is written exactly once (0 where no frame covers it):
 * no atomics, deterministic.  Whatever the tables say, nothing is written outside scratch and grad_sig.  A null grad_X
 * is not read and contributes zero; all three null, or n_frames == 0, launches nothing and leaves grad_sig untouched.
 */
int mpx_analysis_lossless_backward(void* stream, int fft_len, const void* tables, const float* mag, const float* real,
                                   const float* imag, int64_t ld, const float* grad_mag, const float* grad_real,
                                   const float* grad_imag, int64_t ld_grad, const int64_t* frame_pos,
                                   const int32_t* frame_left, const int32_t* frame_right, const int64_t* scratch_off,
                                   int64_t n_frames, float* scratch, int64_t scratch_floats, float* grad_sig,
                                   int64_t total_smpls);

/*
 * mpx_analysis_lossless_backward for rows that mpx_rows_lerp took to a constant frame rate afterwards (the constant-rate
 * lossless analysis): grad_mag / grad_real / grad_imag are the gradients of the CONSTANT-rate rows out[c] =
 * fma(x[row1[c]] - x[row0[c]], row_t[c], x[row0[c]]), [n_const_rows x fft_len/2 + 1] at row pitch ld_grad; mag / real /
 * imag are the variable-rate rows x of the n_frames frames, as above.  ranges: int32 [n_frames x 4] = (a0, a1, b0, b1)
 * per FRAME f -- the constant-rate rows with row0 == f are [a0, a1), those with row1 == f are [b0, b1)
 * (hostmath.lerp_adjoint_table(row0, row1, row_t, n_frames)); row_t float32 [n_const_rows].  The frame kernel forms
 * frame f's gradient row in registers as it loads it: c ascending over the union of the two ranges, weight 1 in both,
 * 1 - row_t[c] in the first only, row_t[c] in the second only, acc = fmaf(w, grad_X[c][k], acc) from 0 -- the operation
 * sequence of mpx_rows_lerp_adjoint, so grad_sig equals mpx_rows_lerp_adjoint followed by mpx_analysis_lossless_backward
 * bit for bit, without the [n_frames x fft_len/2 + 1] gradient rows in between and with one launch fewer.  Ranges are
 * clamped to [0, n_const_rows) whatever the table holds; a frame no row reads contributes zeros.  Everything else is as
 * for mpx_analysis_lossless_backward: two launches, no atomics, one writer per element, deterministic; a null grad_X is
 * never read; all three null, or n_frames == 0, launches nothing and leaves grad_sig untouched.  n_const_rows == 0 with
 * frames and a gradient pointer zeroes grad_sig (ranges and row_t may then be null).
 */
int mpx_analysis_lossless_const_rate_backward(void* stream, int fft_len, const void* tables, const float* mag,
                                              const float* real, const float* imag, int64_t ld, const float* grad_mag,
                                              const float* grad_real, const float* grad_imag, int64_t ld_grad,
                                              int64_t n_const_rows, const int32_t* ranges, const float* row_t,
                                              const int64_t* frame_pos, const int32_t* frame_left,
                                              const int32_t* frame_right, const int64_t* scratch_off, int64_t n_frames,
                                              float* scratch, int64_t scratch_floats, float* grad_sig,
                                              int64_t total_smpls);

/*
 * Copy synthesis in one launch: analysis_lossless (magphase.py:2869-2906: windowing :74-119, analysis_with_del_comp_from_pm
 * :266-334, compute_lossless_feats :457-476) followed by synthesis_from_lossless (:1759-1776, ola :34-62) on the same
 * frames, as demos/demo_copy_synthesis_lossless.py:44-50 calls them back to back.  Frame f is cut out of `sig` exactly as
 * by mpx_analysis_frames (frame_pos / frame_left / frame_right), its three feature rows are written to out_mag / out_real /
 * out_imag (row pitch ld) -- analysis_lossless' return values -- and the frame is rebuilt from those float32 values and
 * overlap-added exactly as by mpx_synthesis_lossless_ola (runs / slot_off / slot_runs / pm_rel / strips / pcm_out: the
 * tables of a synthesis plan built from the analysis' v_f0; mpx_ola_fixup afterwards).  pcm_out equals what
 * mpx_synthesis_lossless_ola gives on the rows written here, and the rows equal mpx_analysis_frames', to the last bits
 * of float32 (the same arithmetic, contracted differently by the compiler / another order of the same transform).  The
 * feature rows are not read back from memory.
 * Every frame of [0, n_frames) must belong to exactly one run (slots: mpx_synth_comp_slots(), weights:
 * mpx_roundtrip_slot_weights).
 */
int mpx_roundtrip_slot_weights(float* weights_host, int32_t n_slots); /* as mpx_synth_comp_slot_weights, for this kernel */
/*
 * What the planner deals this kernel's frames by (mpx_host_deal_cuts).  mpx_roundtrip_frame_terms: per frame the terms
 * (1, active_rows, extra_tiles) of its cost -- the 128-sample register rows the analysis gathers, summed over the frame's
 * sample tiles, and the tiles after the first -- from the frame's host tables; terms_host: int32 [n_frames][3].
 * mpx_roundtrip_slot_costs: per slot the integer coefficients (a, b, c) of those terms, by the age class of the slot's
 * wave pair (10 ns of wall clock; fitted on the MI355X); coef_host: int32 [n_slots][3].  Frame f costs
 * slot s  a_s + b_s rows_f + c_s extra_f.  Host functions: no stream, no device.
 */
int mpx_roundtrip_frame_terms(int fft_len, const int32_t* frame_left, const int32_t* frame_right, int64_t n_frames,
                              int32_t* terms_host);
int mpx_roundtrip_slot_costs(int32_t* coef_host, int32_t n_slots);
int mpx_roundtrip_lossless_ola(void* stream, int fft_len, const void* tables, const float* sig, const int64_t* frame_pos,
                               const int32_t* frame_left, const int32_t* frame_right, int64_t n_frames,
                               const mpx_ola_run* runs, int32_t n_runs, const int32_t* slot_off, const int32_t* slot_runs,
                               int32_t n_slots, const int32_t* pm_rel, float* out_mag, float* out_real, float* out_imag,
                               float* strips, float* pcm_out, int64_t ld);
/*
 * The same launch with flags.  The frame that is rebuilt is the windowed frame that was analysed, so at fft_len 4096 a
 * frame with frame_left <= 512 and frame_right <= 511 (support class 4 of mpx_roundtrip_support_classes; every other frame
 * and every other fft_len: the full class fft_len / 256) is zero outside 8 of its 32 register rows of 128 samples, and by
 * default the kernel neither transforms nor overlap-adds the other rows: the feature rows are unchanged, the waveform
 * loses the float32 rounding residue the full transform adds outside the frame.  MPX_RT_FULL_SUPPORT: every frame takes
 * the full class.  mpx_roundtrip_lossless_ola is this call with flags 0.  mpx_roundtrip_support_classes: the class of each
 * frame from its host tables (host function: no stream, no device); class_host: int32 [n_frames].
 */
#define MPX_RT_FULL_SUPPORT 1u
/*
 * How the feature rows are stored (fft_len 4096 without MPX_RT_FULL_SUPPORT; every other instance ignores both bits and
 * stores as under MPX_RT_STORE_ROWS).  Default: by line -- every interior store of a row covers two whole, aligned 128-byte
 * lines of memory whatever the row's offset in its line (the phase, taken from each row pointer: any ld, any base).
 * MPX_RT_STORE_ROWS: 256-byte blocks aligned to the row's first float.  MPX_RT_STORE_NT: by line, the interior stores
 * non-temporal (not together with MPX_RT_STORE_ROWS).  The values written are the same under all three.
 * mpx_roundtrip_store_map: the by-line shape for a row of phase 0 ... 31, out: int32 [34][64] -- per store of a plane in
 * issue order the row float each lane writes, -1 where the lane is masked -- from the functions the kernel takes its
 * addresses and predicates from; phase 0 is the MPX_RT_STORE_ROWS shape.  fft_len must be 4096.  Host function.
 */
#define MPX_RT_STORE_ROWS 4u
#define MPX_RT_STORE_NT 8u
/*
 * How the waveform is rebuilt at fft_len 4096.  The spectrum the synthesis half is given is the one the analysis half has
 * just computed, so the frame it rebuilds, fftshift(IFFT(hermitian(FFT(y)))) of the windowed, rotated, zero-padded frame y,
 * is fftshift(y) up to the two transforms' float32 error.  Default: direct -- the kernel overlap-adds the windowed frame
 * itself, right after it has gathered it, and runs neither the Hermitian merge nor the inverse transform.
 * MPX_RT_INVERSE_TRANSFORM: it runs them (the earlier behaviour; the A/B switch).  The feature rows are the same bit for
 * bit; the waveforms differ by that float32 error (about 3e-7 of the peak).  fft_len 2048 and 1024 keep the transform
 * and ignore the bit: their inverse leaves the samples in kappa(lane) order, the gather in lane order, so the ring
 * address of the direct add would differ.  mpx_roundtrip_frame_extents accepts and ignores the bit.
 */
#define MPX_RT_INVERSE_TRANSFORM 32u
int mpx_roundtrip_store_map(int fft_len, int phase, int32_t* out);
int mpx_roundtrip_lossless_ola_flags(void* stream, int fft_len, const void* tables, const float* sig,
                                     const int64_t* frame_pos, const int32_t* frame_left, const int32_t* frame_right,
                                     int64_t n_frames, const mpx_ola_run* runs, int32_t n_runs, const int32_t* slot_off,
                                     const int32_t* slot_runs, int32_t n_slots, const int32_t* pm_rel, float* out_mag,
                                     float* out_real, float* out_imag, float* strips, float* pcm_out, int64_t ld,
                                     uint32_t flags);
int mpx_roundtrip_support_classes(int fft_len, const int32_t* frame_left, const int32_t* frame_right, int64_t n_frames,
                                  int32_t* class_host);
/*
 * What the kernel that mpx_roundtrip_lossless_ola_flags launches for (fft_len, flags) can add to its overlap-add ring, per
 * frame: extents_host: int32 [n_frames][2], the half-open range (ext_lo, ext_hi) of frame samples.  (1536, 2560) for a frame
 * of support class 4 at fft_len 4096 where the launched instance has the pruned passes; (0, fft_len) for every other frame,
 * and for every frame under MPX_RT_FULL_SUPPORT or in a build without those passes.  The planner sizes the seams between
 * runs by these (mpx_host_ola_runs_extents).  Host function: no stream, no device.
 */
int mpx_roundtrip_frame_extents(int fft_len, const int32_t* frame_left, const int32_t* frame_right, int64_t n_frames,
                                uint32_t flags, int32_t* extents_host);

/*
 * One iteration of the pitch-synchronous Griffin-Lim algorithm (magphase.py:3320-3372, the loop body after the first
 * synthesis): frame f is cut out of sig_in and analysed as by mpx_roundtrip_lossless_ola (frame_pos / frame_left /
 * frame_right: windowing :74-119 of the previous iteration's signal, with the bounds [0, pm..., len - 1]), the
 * magnitude of every bin is replaced by target_mag's row f (float32, row pitch ld; bins 0..fft_len/2), keeping the phase
 * (X == 0: the reference's angle(0) = 0), and the frame is rebuilt (ifft, no fftshift in the reference's centring) and
 * overlap-added into sig_out by the runs of a synthesis plan over the same epochs (runs / slot_off / slot_runs / pm_rel /
 * strips: slots mpx_synth_comp_slots(), weights mpx_roundtrip_slot_weights; mpx_ola_fixup afterwards).  The output index
 * of epoch pm_f is pm_f, so the next iteration reads sig_out with the same frame tables.  sig_in and sig_out must be
 * different buffers.  phase_out: null, or rows (pitch ld) that receive the phase that was synthesised, angle of the
 * reference's spectrum (epoch at fft_len/2), bins 0..fft_len/2.  No feature rows are written.
 */
int mpx_griffin_lim_ola(void* stream, int fft_len, const void* tables, const float* sig_in, const int64_t* frame_pos,
                        const int32_t* frame_left, const int32_t* frame_right, int64_t n_frames, const float* target_mag,
                        const mpx_ola_run* runs, int32_t n_runs, const int32_t* slot_off, const int32_t* slot_runs,
                        int32_t n_slots, const int32_t* pm_rel, float* phase_out, float* strips, float* sig_out,
                        int64_t ld);

/*
 * The inputs of Griffin-Lim's FIRST synthesis from the target magnitudes and an initial phase (magphase.py:3334-3356:
 * frames = ifft(M e^{j phi}).real with phi not necessarily Hermitian), as the rows mpx_synthesis_lossless_ola reads
 * (k_gl_fold, one thread per frame and bin, float64 arithmetic rounded once to float32).
 * Frames frame0 .. frame0 + n_frames - 1 of mag and of the outputs (row pitch ld, H = fft_len / 2 + 1 columns) are
 * folded; `phase` points at the phase of frame frame0 (the caller folds a batch in groups of utterances):
 *   MPX_GL_FOLD_HALF   float32 [n_frames x H] at pitch ld_phase, a Hermitian extension; columns 0 and H - 1 count as 0
 *                      whatever they hold.  Outputs (M, cos phi (-1)^k, sin phi (-1)^k).
 *   MPX_GL_FOLD_FULL   float32 [n_frames x fft_len] at pitch ld_phase.  c_k = (e^{j phi_k} + e^{-j phi_{N-k}}) / 2 (the
 *                      real cos phi_0 and cos phi_{N/2} at the ends); outputs mag' = M |c| and the phasor c (-1)^k / |c|,
 *                      (0, 0, 0) where |c| = 0.
 *   MPX_GL_FOLD_WORDS  numpy's raw MT19937 words (uint32, 8-byte aligned, the `raw` buffer of mpx_noise_numpy_mt19937),
 *                      two per sample, row-major over [n_frames x fft_len]: r = ((w0 >> 5) 2^26 + (w1 >> 6)) / 2^53 (what
 *                      np.random.rand returns), phi = 2 pi (r - 0.5), then the FULL fold.  ld_phase is not read.
 * out_phase: null, or rows (pitch ld) that receive float32 phi_k, k < H (HALF: with the zeroed ends).  Every element of
 * columns 0 .. H - 1 of the output rows is written exactly once, nothing else is written.  n_frames == 0 returns MPX_OK
 * without a launch; MPX_ERR_ARG (detected on the host, without a device) for another fft_len, an unknown form, a
 * negative size, ld < H, ld_phase smaller than the phase rows, or a null pointer with frames to fold.
 */
#define MPX_GL_FOLD_HALF 0
#define MPX_GL_FOLD_FULL 1
#define MPX_GL_FOLD_WORDS 2
int mpx_griffin_lim_fold(void* stream, int fft_len, int32_t form, const float* mag, const void* phase, int64_t ld_phase,
                         int64_t frame0, int64_t n_frames, float* out_mag, float* out_real, float* out_imag,
                         float* out_phase, int64_t ld);

/* ------------------------------------------------------------------------------------------------------------------
 * Compressed-feature synthesis (magphase.py:825-997 synthesis_from_compressed, b_fbank_mel=False, per_phase_type='magphase')
 * ------------------------------------------------------------------------------------------------------------------ */

/*
 * Mel unwarp of the three feature streams as the linear maps they are:
 *   out_mag  = exp(a_mag  [F x k_mag]   @ u_mag   [k_mag   x n_bins])   la.sp_mel_unwarp + np.exp   (magphase.py:854)
 *   out_real =     a_real [F x k_phase] @ u_phase [k_phase x n_bins]    phase_uncompress_type1_mcep (magphase.py:1219-1235,
 *   out_imag =     a_imag [F x k_phase] @ u_phase                        nearest-neighbour extension folded into u_phase)
 * The matrices are computed on the host in float64 (magphase_amd/hostmath.py: unwarp_matrix, phase_unwarp_matrix).
 */
int mpx_mel_unwarp(void* stream, int64_t n_frames, int32_t n_bins, const float* a_mag, int32_t k_mag,
                   const float* u_mag, float* out_mag, const float* a_real, const float* a_imag, int32_t k_phase,
                   const float* u_phase, float* out_real, float* out_imag,
                   int64_t ld /* row pitch of the three outputs in floats, >= n_bins; see mpx_spec_ld */);

/*
 * mpx_mel_unwarp with the constant -> variable frame-rate interpolation of synthesis_from_compressed folded in
 * (magphase.py:861-868, interp_from_const_to_variable_rate :2242-2252): output row f (n_frames = VARIABLE-rate frames) is
 * the linear interpolation, weight row_t[f], between the unwarped rows row0[f] and row1[f] of the constant-rate
 * coefficient matrices -- out_mag = lerp(exp(U a[row0]), exp(U a[row1])), out_real / out_imag = U lerp(a[row0], a[row1])
 * (the phase unwarp is linear).  The [rows x n_bins] spectra are written once, at the variable rate, and the synthesis
 * kernel reads one row per frame.  row0, row1: DEVICE int32[n_frames]; row_t: DEVICE float32[n_frames].
 * tile_first (optional, with n_rows = number of constant-rate rows): DEVICE int32[ceil(n_rows / 31) + 1], tile_first[T] =
 * the first frame whose row0 >= 31 T (row0 ascending, row1 - row0 in {0, 1}: what the constant -> variable scan yields);
 * the magnitudes are then unwarped once per constant-rate ROW and interpolated out of an LDS tile (same values, 44 % fewer
 * products).  NULL: two products per frame.
 * voiced (optional): DEVICE int32[n_frames]; the PHASE rows of a 32-frame tile without a voiced frame are not computed (out_real /
 * out_imag keep their previous content there): mpx_synthesis_compressed_ola never reads the phase rows of unvoiced frames.
 * n_phase_bins: only the first n_phase_bins bins (rounded up to a multiple of 64) of out_real / out_imag are produced (0: all):
 * above the periodic / aperiodic crossfade (magphase.py:873-876; 6 kHz at 48 kHz = bin 512 of 2049) the periodic curve is
 * exactly zero and the synthesis (n_per_bins below) does not read them.
 */
int mpx_mel_unwarp_rows(void* stream, int64_t n_frames, int32_t n_bins, const float* a_mag, int32_t k_mag,
                        const float* u_mag, float* out_mag, const float* a_real, const float* a_imag, int32_t k_phase,
                        const float* u_phase, float* out_real, float* out_imag, int64_t ld, const int32_t* row0,
                        const int32_t* row1, const float* row_t, int64_t n_rows, const int32_t* tile_first,
                        const int32_t* voiced, int32_t n_phase_bins);

/*
 * Row pitch the unwarped spectra (outputs of mpx_mel_unwarp / mpx_min_phase, inputs of mpx_synthesis_compressed_ola)
 * should be allocated with: n_bins rounded up to a multiple of 32 floats.  mpx_mel_unwarp runs on the matrix cores
 * (v_mfma_f32_32x32x2_f32) and a wave stores 32-float row segments; with 128-byte aligned rows every segment is one
 * full line (measured: 0.80 -> 0.55 ms for the three matrices of 57 k frames), with the dense pitch every segment
 * leaves two partially written lines behind.  Any ld >= n_bins is correct.
 */
int64_t mpx_spec_ld(int32_t n_bins);

/*
 * Device noise source -- OPT-IN replacement of np.random.uniform(-1, 1, n) (magphase.py:883; the reference draws the
 * aperiodic excitation from numpy's global Mersenne twister on the host).  out[offsets[u] + i] = sample i of utterance
 * u = word (i & 3) of Philox4x32-10(counter = i >> 2, key = seeds[u]) mapped to (w >> 8) * 2^-23 - 1 in [-1, 1).
 * A sample depends on (seed, i) only: the result is independent of batching and sharding (bit-identical files from 1 or
 * 8 GPUs).  Same distribution as the reference's source, NOT its sample values; the default mode of the Python layer
 * keeps drawing on the host so that a seeded run reproduces the reference sample for sample.
 * seeds: uint64[n_utts]; offsets: int64[n_utts+1]; max_len: longest utterance (grid sizing).
 */
int mpx_noise_uniform(void* stream, int32_t n_utts, const uint64_t* seeds, const int64_t* offsets, int64_t max_len,
                      float* out);

/*
 * The reference's noise source, np.random.uniform(-1, 1, n) drawn from numpy's GLOBAL generator (magphase.py:883), produced
 * on the device from numpy's own state: key [624] (DEVICE uint32) and pos are np.random.get_state()[1:3]; out [n_samples]
 * gets float32(-1 + 2 d), d = the 53-bit doubles random_sample() would return (two MT19937 words each) -- bit-identical to
 * the host draw --, key_out [624] / pos_out [1] (DEVICE) the state numpy is left in after those draws (the caller puts it
 * back with np.random.set_state).  raw: DEVICE scratch of 2 * n_samples uint32.  work: DEVICE scratch of
 * mpx_noise_numpy_mt19937_work_words() uint32, or NULL.  With work and more than one segment of 319 488 words to draw,
 * the stream is produced by one workgroup per segment: the 624-word window each segment starts from is a jump-ahead of
 * the first one (X[n + J] = xor of X[n + i] over the set bits of x^J mod the generator's characteristic polynomial;
 * log2(segments) rounds of k_mt_seq + k_mt_xor, polynomials from mpx_host_mt19937_jump_polys).  Without work, or for short draws,
 * one workgroup runs the recurrence from the key (454 words per barrier).  A second kernel converts.  Bit-identical
 * either way.  The many-workgroup form waits for the stream once (the polynomials are uploaded from pageable memory);
 * its caller reads key_out / pos_out back right afterwards anyway.
 */
int mpx_noise_numpy_mt19937(void* stream, const uint32_t* key, int32_t pos, int64_t n_samples, uint32_t* raw,
                            float* out, uint32_t* key_out, int32_t* pos_out, uint32_t* work);
int64_t mpx_noise_numpy_mt19937_work_words(void);

/*
 * Host helper (no device): out [n_levels x 624] uint32 (HOST), level l = the bits of x^(jump_words * 2^l) mod phi, phi the
 * characteristic polynomial (degree 19937) of MT19937's word recurrence; bit i of a level = bit (i & 31) of word i >> 5.
 * For the words X[n] the recurrence produces (n >= 624 counted from a key), X[n + jump] = xor_{i : bit i} X[n + i].
 * phi is found once per process (Berlekamp-Massey), ladders are cached per jump_words.
 */
int32_t mpx_host_mt19937_jump_poly(int64_t jump_words, int32_t n_levels, uint32_t* out);
/* The same for n arbitrary jumps, independent of each other (no cache), on up to n_threads host threads: out [n x 624].
 * mpx_noise_numpy_mt19937's ladder takes the multiples p * J * R^l (p < R; R = 2: the doubling ladder) of its segment
 * length from here. */
int32_t mpx_host_mt19937_jump_polys(const int64_t* jumps, int32_t n, uint32_t* out, int32_t n_threads);

/*
 * Noise-gain statistics (magphase.py:886-903, Q10/Q11): for every frame, the windowed noise frame
 * (frame_wtype 0: Hann halves, 1: np.bartlett**2.5 halves; epoch at index 0) is transformed and
 * out_sum[f] = sum_{k=1}^{N/2-1} (ln|Ns[k]|)^2.  The host turns the per-class means into the two gains per utterance.
 * noise / frame_pos / frame_left / frame_right as sig / frame_* of mpx_analysis_frames.
 */
int mpx_noise_stats(void* stream, int fft_len, const void* tables, const float* noise, const int64_t* frame_pos,
                    const int32_t* frame_left, const int32_t* frame_right, const int32_t* frame_wtype,
                    int64_t n_frames, float* out_sum);
/*
 * "Noise spectra once" form of the pair mpx_noise_stats -> mpx_synthesis_compressed_ola (fft_len 4096 only; the same
 * reference lines, magphase.py:886-903 and :908-976): mpx_noise_stats_spectra also stores every frame's noise spectrum
 * (mpx_noise_spectra_floats(fft_len, n_frames) floats, in the kernels' own register layout), and
 * mpx_synthesis_compressed_ola_spectra (one row per frame: row0 / row1 / row_t NULL) loads it instead of transforming
 * the noise frame a second time.  Trades the second FFT for 17.4 KB of HBM traffic per frame each way; opt-in
 * (MAGPHASE_NOISE_SPECTRA=store), measured in docs/LAB_NOTES.md (round 5).
 */
int64_t mpx_noise_spectra_floats(int fft_len, int64_t n_frames);
int mpx_noise_stats_spectra(void* stream, int fft_len, const void* tables, const float* noise, const int64_t* frame_pos,
                            const int32_t* frame_left, const int32_t* frame_right, const int32_t* frame_wtype,
                            int64_t n_frames, float* out_sum, float* spectra);

/*
 * Spectrum assembly + inverse FFT + anti-ringing window + PSOLA for compressed-feature synthesis
 * (magphase.py:908-976; run / slot / strip tables and pcm_out exactly as mpx_synthesis_lossless_ola, followed by mpx_ola_fixup).
 * Per frame f (all arrays int32/float32[n_frames] unless noted):
 *   noise_pos(int64)/noise_left/noise_right/noise_wtype : this frame's noise frame (recomputed here)
 *   voiced, inv_gain                                    : class flag and 1/gain of its class
 *   row0,row1,row_t : the frame's mag/real/imag row = (1-row_t)*row[row0] + row_t*row[row1] of the [rows x H] matrices
 *                     (constant -> variable frame rate, magphase.py:2242-2252; row0 == row1 for variable-rate input);
 *                     all three NULL: one row per frame, row index = frame index (variable-rate input, or rows already
 *                     interpolated by mpx_mel_unwarp_rows -- half the feature loads)
 *   win_left, win_right : anti-ringing window half lengths (Q14);  pm_rel : as mpx_ola_gather
 * per_v, ap_v, ap_u : float32[H] per-bin constants (hostmath.synthesis_bin_curves: tilt x sqrt(mask) etc., Q12/Q13)
 * n_per_bins : per_v[k] == 0 for k >= n_per_bins (the caller's promise; 0 or > H: no promise, n_per_bins counts as H): those
 *              bins have no periodic component.  One row per frame form: real / imag (and per_v) are read in whole groups of
 *              64 bins, of VOICED frames only (the real / imag rows of unvoiced frames are not read at all).  With
 *              Q = fft_len / 4 the groups are
 *                [64 q, 64 q + 63]                 for every 64 q < min(n_per_bins, Q)        (the lanes' own bins),
 *                [Q, Q + 63]                       when n_per_bins > Q                        (bin Q; the other 63 are loaded, not used),
 *                [Q + 1 + 64 j, Q + 64 + 64 j]     for every j >= 0 with Q + 1 + 64 j < n_per_bins  (the mirror bins),
 *              that is the leading hostmath.synth_comp_phase_columns(fft_len, n_per_bins) columns: n_per_bins rounded up to 64
 *              while n_per_bins <= Q + 1 (every supported sample rate), Q + 1 + (n_per_bins - Q - 1 rounded up to 64) beyond,
 *              at most H.  Every element of a group that is read must be finite -- a NaN or an infinity there reaches the
 *              output even where per_v is 0 --; no other element of real / imag is read.
 *              Row-table form: n_per_bins is not looked at; every bin of the rows row0[f] and row1[f] of mag, real and imag is
 *              read for every frame, voiced or not, and must be finite.
 */
int mpx_synth_comp_slots(void); /* wave slots of mpx_synthesis_compressed_ola on the current device */
/* Relative speed of the compressed synthesis kernel's slots (see mpx_synth_ola_slot_weights). */
int mpx_synth_comp_slot_weights(float* weights_host, int32_t n_slots);
int mpx_synthesis_compressed_ola(void* stream, int fft_len, const void* tables, const float* mag, const float* real,
                                 const float* imag, const float* noise, const int64_t* noise_pos,
                                 const int32_t* noise_left, const int32_t* noise_right, const int32_t* noise_wtype,
                                 const int32_t* voiced, const float* inv_gain, const int32_t* row0,
                                 const int32_t* row1, const float* row_t, const int32_t* win_left,
                                 const int32_t* win_right, const int32_t* pm_rel, const float* per_v,
                                 const float* ap_v, const float* ap_u, const mpx_ola_run* runs, int32_t n_runs,
                                 const int32_t* slot_off, const int32_t* slot_runs, int32_t n_slots,
                                 float* strips, float* pcm_out,
                                 int64_t ld /* row pitch of mag/real/imag in floats, >= fft_len/2 + 1 */,
                                 int32_t n_per_bins);
int mpx_synthesis_compressed_ola_spectra(void* stream, int fft_len, const void* tables, const float* mag, const float* real,
                                 const float* imag, const float* noise, const int64_t* noise_pos,
                                 const int32_t* noise_left, const int32_t* noise_right, const int32_t* noise_wtype,
                                 const int32_t* voiced, const float* inv_gain, const int32_t* row0,
                                 const int32_t* row1, const float* row_t, const int32_t* win_left,
                                 const int32_t* win_right, const int32_t* pm_rel, const float* per_v,
                                 const float* ap_v, const float* ap_u, const mpx_ola_run* runs, int32_t n_runs,
                                 const int32_t* slot_off, const int32_t* slot_runs, int32_t n_slots,
                                 float* strips, float* pcm_out, int64_t ld, int32_t n_per_bins,
                                 const float* spectra /* as stored by mpx_noise_stats_spectra */);
/*
 * The same launch for synthesis_from_compressed_type2 (magphase.py:1556-1597): the DC and Nyquist bins keep their signed
 * real part with a zero imaginary part (la.add_hermitian_half(.., 'complex'), :1567) instead of the modulus.  What else
 * differs from type 1 arrives as data: inv_gain = 1 / rms of the utterance's noise spectra for every frame
 * (mpx_noise_power + mpx_noise_rms), per_v / ap_v / ap_u = hostmath.type2_synthesis_bin_curves (plain crossfade, the
 * hf_slope line).  Arguments, tables and dispatch as mpx_synthesis_compressed_ola; no stored-spectra form.
 */
int mpx_synthesis_compressed_type2_ola(void* stream, int fft_len, const void* tables, const float* mag, const float* real,
                                 const float* imag, const float* noise, const int64_t* noise_pos,
                                 const int32_t* noise_left, const int32_t* noise_right, const int32_t* noise_wtype,
                                 const int32_t* voiced, const float* inv_gain, const int32_t* row0,
                                 const int32_t* row1, const float* row_t, const int32_t* win_left,
                                 const int32_t* win_right, const int32_t* pm_rel, const float* per_v,
                                 const float* ap_v, const float* ap_u, const mpx_ola_run* runs, int32_t n_runs,
                                 const int32_t* slot_off, const int32_t* slot_runs, int32_t n_slots,
                                 float* strips, float* pcm_out, int64_t ld, int32_t n_per_bins);

/*
 * HOST function (no device work, no stream): the serial constant -> variable frame-rate scan of
 * magphase.py:1426-1449 (get_shifts_and_frm_locs_from_const_shifts, Q16) in the reference's float64 operation
 * sequence (scipy interp1d's linear formula, no FMA): bit-identical shifts / frame locations, ~100x faster than one
 * scipy call per step.  centres, shift_c: HOST float64[n] (centres ascending); shifts_out, locs_out: HOST float64[2n].
 * Returns the index `start` of the first valid element (results are out[start .. 2n)), or -1 on bad arguments.
 */
int64_t mpx_host_const_to_var_scan(const double* centres, const double* shift_c, int64_t n, double* shifts_out,
                                   double* locs_out);
/*
 * The same scan with an explicit capacity: shifts_out / locs_out hold `cap` elements, the scan runs until the position
 * leaves the grid (the reference's 2n slots can run out first: more than two frames per constant-rate frame on average).
 * Where 2n slots suffice the results equal mpx_host_const_to_var_scan's.  n == 1: one frame at the single centre.  A cap of
 * floor((centres[n-1] - centres[0]) / min(shift_c)) + 2 is always enough for positive shifts.  Returns `start` (results
 * are out[start .. cap)), -1 on bad arguments, -2 when cap was too small.
 */
int64_t mpx_host_const_to_var_scan_cap(const double* centres, const double* shift_c, int64_t n, double* shifts_out,
                                       double* locs_out, int64_t cap);

/* ------------------------------------------------------------------------------------------------------------------
 * Compressed-feature analysis (magphase.py:2490-2544 format_for_modelling, :2947-2988 analysis_compressed)
 * ------------------------------------------------------------------------------------------------------------------ */

/*
 * Mel warp of the lossless features (la.sp_mel_warp, libaudio.py:643-661 = SPTK-3.9 ``mcep -j 0`` + alpha=0 cosine matrix;
 * the SPTK part is a restatement, PARITY UNPINNED) as linear maps of the log-periodogram, plus the epilogues of
 * format_for_modelling:
 *   out_mag  [F x mag_dim]   = W_mag   . ln(mag^2 + 1e-8)                                  (== la.log(sp_mel_warp(mag)))
 *   out_real [F x phase_dim] = clip(voiced * (W_phase . ln(exp(real)^2 + 1e-8)), -1, 1)    (same for imag)
 * W_mag [mag_dim x n_bins], W_phase [phase_dim x n_bins] float32 from hostmath.warp_matrix (float64 on the host).
 * row0/row1/row_t (all null, or int32/int32/float32 [F]): output frame f reads the interpolated input row
 * (1-row_t)*x[row0] + row_t*x[row1] (variable -> constant frame rate, magphase.py:2219-2239); null = row f.
 */
int mpx_mel_warp(void* stream, int64_t n_frames, int32_t n_bins, const float* mag, const float* real, const float* imag,
                 const int32_t* row0, const int32_t* row1, const float* row_t, const float* w_mag, int32_t mag_dim,
                 const float* w_phase, int32_t phase_dim, const float* voiced, float* out_mag, float* out_real,
                 float* out_imag, int64_t ld /* row pitch of mag/real/imag in floats, >= n_bins */);

/*
 * mpx_mel_warp with the magnitudes compressed by the mel FILTER BANK instead of the cepstral warp
 * (format_for_modelling(b_mag_fbank_mel=True), magphase.py:2504-2510; la.sp_mel_warp_fbank / apply_fbank 'average',
 * libaudio.py:721-769): out_mag = la.log(exp(W_fbank . la.log(mag))), la.log's floor (-1e10 for mag == 0, and where the
 * exp underflows) included.  w_fbank: [mag_dim x n_bins] (hostmath.warp_fbank_matrix).  The phase streams are unchanged.
 */
int mpx_mel_warp_fbank(void* stream, int64_t n_frames, int32_t n_bins, const float* mag, const float* real,
                       const float* imag, const int32_t* row0, const int32_t* row1, const float* row_t,
                       const float* w_fbank, int32_t mag_dim, const float* w_phase, int32_t phase_dim, const float* voiced,
                       float* out_mag, float* out_real, float* out_imag, int64_t ld);

/*
 * mpx_mel_warp / mpx_mel_warp_fbank (mag_fbank != 0) with the row tables given, and the phase streams warped on the
 * VARIABLE-rate rows: the phase prologue ln(e^{2x} + 1e-8) = 2x + 1e-8 e^{-2x} is linear up to its floor term, so the
 * product is formed once per variable-rate row (n_var_rows rows of real / imag, no row interpolation in the operand
 * load: half the loads of the phase jobs, 11 % fewer rows at a 5 ms rate) into tmp_real / tmp_imag [n_var_rows x phase_dim]
 * (DEVICE scratch) and the phase_dim outputs are interpolated to the constant rate, masked and clipped afterwards
 * (magphase.py:2219-2239 then :2520-2532 in the other order; difference < 1e-8 per bin).  rows_in_use [n_var_rows]: != 0
 * for the rows a voiced constant-rate frame interpolates from -- 64-row tiles without one are not computed.  With
 * tmp_real == NULL: exactly mpx_mel_warp / mpx_mel_warp_fbank.
 */
int mpx_mel_warp_rows(void* stream, int64_t n_frames, int32_t n_bins, const float* mag, const float* real,
                      const float* imag, const int32_t* row0, const int32_t* row1, const float* row_t, const float* w_mag,
                      int32_t mag_dim, const float* w_phase, int32_t phase_dim, const float* voiced, float* out_mag,
                      float* out_real, float* out_imag, int64_t ld, int32_t mag_fbank, int64_t n_var_rows,
                      const float* rows_in_use, float* tmp_real, float* tmp_imag);

/*
 * The second half of mpx_mel_warp_rows' phase streams on its own: out[f] = clip(voiced[f] * ((1 - t) tmp[row0[f]] +
 * t tmp[row1[f]])) for the phase_dim columns of both streams, 0 where voiced[f] == 0 (magphase.py:2219-2239, :2527-2532).
 */
int mpx_warp_phase_rows(void* stream, int64_t n_frames, int32_t phase_dim, const float* tmp_real, const float* tmp_imag,
                        const int32_t* row0, const int32_t* row1, const float* row_t, const float* voiced, float* out_real,
                        float* out_imag);

/*
 * Backward pass of the mel warp (mpx_mel_warp / mpx_mel_warp_rows, cepstral magnitudes): up to three jobs in ONE launch,
 *     grad_x[r][k] = d(x~[r][k]) * sum_{i < n_out} g[r][i] W[i][k],   k < n_bins,
 * the product [rows x n_out] . [n_out x n_bins] on the f32 matrix instructions; g rows are dense ([rows x n_out]), the
 * operand rows mag / real / imag have the row pitch ld, the output rows the pitch ld_grad (both >= n_bins; nothing is
 * written between the rows).
 *   magnitude job: g_mag [n_mag_rows x mag_dim], w_mag [mag_dim x n_bins], grad_mag [n_mag_rows x n_bins];
 *                  x~[r] = mag[r], or with row0 / row1 / row_t (all null or all given, n_mag_rows entries)
 *                  fma(mag[row1[r]] - mag[row0[r]], row_t[r], mag[row0[r]]), the forward's interpolated operand (the result
 *                  is then per OUTPUT frame: mpx_rows_lerp_adjoint folds it onto the rows of mag);
 *                  d = 2 x~ / (x~^2 + 1e-8), the derivative of ln(x~^2 + 1e-8): 0 at x~ == 0.
 *   phase jobs:    h_real / h_imag [n_phase_rows x phase_dim], w_phase [phase_dim x n_bins], operands real / imag (plain
 *                  rows), grad_real / grad_imag [n_phase_rows x n_bins]; d = 2 - 2e-8 e^{-2x}, the derivative of
 *                  2x + 1e-8 e^{-2x}.  h is taken ALREADY MASKED by the forward's voicing mask and clip
 *                  (mpx_phase_grad_mask; at the constant rate folded onto the variable-rate rows by
 *                  mpx_rows_lerp_adjoint at n_bins = phase_dim in between).  live [n_phase_rows] or null: a row with
 *                  live == 0 is one whose h is zero by construction (an unvoiced frame; a row no voiced frame reads) --
 *                  it is written as zeros whatever its operand row holds, and a 64-row tile without a live row is
 *                  written as zeros without reading its operands.
 * A job whose grad_X is null is skipped (its other pointers are not looked at, nothing of it is written); a job with
 * zero rows launches nothing; with nothing to do the call returns 0 without a launch.  n_out (mag_dim / phase_dim of a
 * job that runs) must be in 1..64.  Every element of a non-null grad_X is written exactly once with plain stores: no
 * atomics, deterministic.  Arguments are checked before the device is touched.
 */
int mpx_mel_warp_backward(void* stream, int32_t n_bins, const float* g_mag, const float* w_mag, int32_t mag_dim,
                          const float* mag, int64_t n_mag_rows, const int32_t* row0, const int32_t* row1,
                          const float* row_t, float* grad_mag, const float* h_real, const float* h_imag,
                          const float* w_phase, int32_t phase_dim, const float* real, const float* imag,
                          int64_t n_phase_rows, const float* live, float* grad_real, float* grad_imag, int64_t ld,
                          int64_t ld_grad);

/*
 * Backward of mpx_mel_unwarp / mpx_mel_unwarp_rows (la.sp_mel_unwarp, libaudio.py:663-690; the compressed synthesis): the
 * gradients with respect to the coefficient rows, up to three products [rows x K] . [K x n_out] in one launch (float32
 * matrix instructions, float32 accumulation).
 *   magnitude job: grad_a_mag[r][c] = sum_{k < n_bins} u_mag[c][k] e_mag[r][k] g_mag[r][k] -- e_mag = exp(a_mag . u_mag),
 *                  the forward's unwarped magnitudes at the ROWS' rate (row pitch ld_e), g_mag the gradient with respect
 *                  to them (pitch ld_g), u_mag [mag_dim x n_bins] the forward's matrix; grad_a_mag [n_mag_rows x mag_dim].
 *   phase jobs:    grad_a_real[r][c] = sum_{k < n_phase_bins} u_phase[c][k] g_real[r][k] (imag alike): g_real / g_imag
 *                  [n_phase_rows x n_phase_bins] at pitch ld_phase, u_phase [phase_dim x n_bins]; outputs
 *                  [n_phase_rows x phase_dim].
 * Nothing beyond the named columns of an operand row is read.  A job whose output is null is skipped (its other pointers are
 * not looked at); a job with zero rows launches nothing.  n_out (mag_dim / phase_dim of a job that runs) must be in 1..64.
 * Every element of a non-null output is written exactly once: no atomics, deterministic.  Arguments are checked before the
 * device is touched.
 */
int mpx_mel_unwarp_backward(void* stream, int32_t n_bins, const float* e_mag, int64_t ld_e, const float* g_mag,
                            int64_t ld_g, const float* u_mag, int32_t mag_dim, int64_t n_mag_rows, float* grad_a_mag,
                            const float* g_real, const float* g_imag, int64_t ld_phase, int32_t n_phase_bins,
                            const float* u_phase, int32_t phase_dim, int64_t n_phase_rows, float* grad_a_real,
                            float* grad_a_imag);

/*
 * The upstream gradients of the two phase streams through the voicing mask and clip of mpx_mel_warp's epilogue
 * (magphase.py:2527-2532): h[f][j] = g[f][j] where voiced[f] != 0 and |out[f][j]| < 1, else 0 -- out_real / out_imag are
 * the forward's own outputs, a clipped value is exactly +-1.0f, and the gradient there is defined as zero.  All matrices
 * dense [n_frames x phase_dim].  A null h_X skips that stream.
 */
int mpx_phase_grad_mask(void* stream, int64_t n_frames, int32_t phase_dim, const float* voiced, const float* out_real,
                        const float* out_imag, const float* g_real, const float* g_imag, float* h_real, float* h_imag);

/*
 * Minimum-phase spectrum of a magnitude spectrum by the complex cepstrum (la.build_min_phase_from_mag_spec,
 * libaudio.py:920-934; synthesis_from_compressed(per_phase_type='min_phase'), magphase.py:937-938).
 * For output frame f: m = (1-row_t)*mag[row0] + row_t*mag[row1] ([rows x H]); out_mag[f] = m and
 * (out_real, out_imag)[f] = (cos phi, sin phi), phi = Im FFT(causal fold(IFFT(ln m))) -- the unit phasor the
 * synthesis kernel expects in place of the unwarped phase features ([n_frames x H] each).
 */
int mpx_min_phase(void* stream, int fft_len, const void* tables, const float* mag, const int32_t* row0,
                  const int32_t* row1, const float* row_t, int64_t n_frames, float* out_mag, float* out_real,
                  float* out_imag, int64_t ld /* row pitch of mag and of the three outputs, floats */);

/*
 * Backward pass of mpx_min_phase with respect to the magnitude row it was computed from (the row interpolation is not
 * part of it: mpx_rows_lerp_adjoint), one wavefront per frame.  mag / real / imag: mpx_min_phase's own outputs
 * (m, cos phi, sin phi), [n_frames x H] at row pitch ld, H = fft_len / 2 + 1.  grad_m / grad_a / grad_b: the gradients with
 * respect to those three rows, at row pitch ld_grad; columns of grad_a / grad_b at or beyond n_phase (0 <= n_phase <= H)
 * are not read and count as zero (mpx_synthesis_compressed_backward writes min(n_per rounded up to 64, H) columns).
 * A null grad_a or grad_b is zero -- both null: grad_mag = grad_m, no transform -- and so is a null grad_m.
 * grad_mag[f][k] = grad_m[f][k] + (T^t g_phi)[k] / m[k] where m[k] > 0, grad_m[f][k] elsewhere, with
 * g_phi = grad_b cos phi - grad_a sin phi (0 at bins 0 and fft_len / 2) and T the linear map ln m -> phi
 * (DESIGN.md section 3.3o).  [n_frames x H] at row pitch ld_out; every element is written exactly once, no atomics,
 * nothing outside columns 0 .. H - 1.  grad_mag may be grad_m itself (same pointer and ld_out == ld_grad), no other overlap.
 * Returns 0 without a launch when n_frames is 0.
 */
int mpx_min_phase_backward(void* stream, int fft_len, const void* tables, const float* mag, const float* real,
                           const float* imag, int64_t ld, const float* grad_m, const float* grad_a, const float* grad_b,
                           int64_t ld_grad, int32_t n_phase, int64_t n_frames, float* grad_mag, int64_t ld_out);

/*
 * True envelope (la.true_envelope, libaudio.py:295-340), one wavefront per frame.  For each row of in ([n_frames x H],
 * H = fft_len / 2 + 1, row pitch ld_in): v = the row in dB (in_type 0: 20 log10 x, 1: x, 2: (20 / ln 10) x); then up
 * to max_iters passes of sm = Re FFT(weights . IFFT(even extension of v))[0..H-1] (la.spectral_smoothing_rceps),
 * stopping when sum |v - sm| < thres_db * H, else v = max(v, sm); out = the last sm, converted back (in_type 0: 10^(sm/20),
 * 2: (ln 10 / 20) sm).  weights: float32 [fft_len], the cepstral weight of every index (hostmath.true_envelope_lifter).
 * A row with a non-finite dB value (a zero or negative magnitude for in_type 0) is written as NaN.  iters (optional):
 * int32 [n_frames], the passes made.  forced_iters (optional): exactly clamp(forced_iters[f], 1, max_iters) passes, no
 * stop test.  ticket (optional): a device int32 the launch zeroes and then hands out frames from (else grid stride).
 */
int mpx_true_envelope(void* stream, int fft_len, const void* tables, const float* weights, const float* in,
                      int64_t ld_in, int64_t n_frames, int32_t in_type, double thres_db, int32_t max_iters, float* out,
                      int64_t ld_out, int32_t* iters, const int32_t* forced_iters, int32_t* ticket);

/*
 * Backward pass of the true envelope, one wavefront per frame: the exact adjoint of the forward pass as the device decides
 * it.  in / in_type / weights as the forward call took them; iters (required): int32 [n_frames], the passes the forward
 * made.  Per row the K = clamp(iters[f], 1, max_iters) passes are recomputed, the decisions of the max updates
 * (m_k[b] = sm_k[b] > v_k[b], k < K; a tie keeps v) are kept on chip, and the K passes are run in reverse on grad_out
 * ([n_frames x H], the gradient with respect to out): with S one smoothing pass, S^T g = D^-1 S (D g), D = diag(2, 1, ...,
 * 1, 2).  grad_in ([n_frames x H]): the gradient with respect to in; every element is written exactly once, no atomics.
 * The stop test is not differentiated.  A row the forward wrote as NaN gets an all-zero gradient row.  max_iters <= 100
 * (the capacity of the on-chip decision history).  Optional outputs, for tests: decisions, int32 [n_frames x max_iters x
 * ceil(H / 32)]: bit b % 32 of word b / 32 of pass k's words (k = 1 .. max_iters, pass-major) is m_k[b]; the words of the
 * passes that decide nothing (k >= K) are 0.  env_out ([n_frames x H], row pitch ld_env_out): the recomputed out rows.
 * ticket as in mpx_true_envelope.
 */
int mpx_true_envelope_backward(void* stream, int fft_len, const void* tables, const float* weights, const float* in,
                               int64_t ld_in, int64_t n_frames, int32_t in_type, int32_t max_iters, const int32_t* iters,
                               const float* grad_out, int64_t ld_grad_out, float* grad_in, int64_t ld_grad_in,
                               int32_t* decisions, float* env_out, int64_t ld_env_out, int32_t* ticket);

/*
 * Per-frame gain of the type-2 analysis (analysis_with_del_comp_from_pm_type2, magphase.py:236-242), one wavefront per
 * frame, float64.  Frames as mpx_analysis_frames takes them (frame_pos / frame_left / frame_right into sig).  voi: float32
 * [n_frames], the epoch's voicing.  gain[f] = (voi[f] == 1) ? max |x| over the first fft_len/2 + 1 samples of the
 * rotated, zero-padded or truncated FFT input : np.std of the whole Hann-windowed frame (all left + right + 1 samples).
 * blocks_per_cu: workgroups of 8 waves per CU at most (<= 0: the default, 3; at most 8).
 */
int mpx_frame_gain(void* stream, int fft_len, const float* sig, const int64_t* frame_pos, const int32_t* frame_left,
                   const int32_t* frame_right, const float* voi, int64_t n_frames, double* gain,
                   int32_t blocks_per_cu);

/*
 * Noise gains on the device (magphase.py:902-906, Q10): per utterance u and class c (0 voiced, 1 unvoiced)
 * g = sqrt(exp( sum of out_sum over the class's frames / (n_frames_of_class * bins_per_frame) )), float64;
 * inv_gain[f] = 1/g(class of f) (float32, input of mpx_synthesis_compressed_ola); gains (optional, may be null):
 * float64 [n_utts x 2].  bins_per_frame = N/2 - 1.
 */
int mpx_noise_gains(void* stream, const float* sums, const int32_t* voiced, const int32_t* utt_frame_off,
                    int32_t n_utts, int32_t bins_per_frame, float* inv_gain, double* gains);

/*
 * Noise statistic of the type-2 synthesis (synthesis_from_compressed_type2, magphase.py:1530-1541), without a transform.
 * mpx_noise_power: one wavefront per frame; noise / frame_pos / frame_left / frame_right / frame_wtype as mpx_noise_stats
 * takes them; power[f] (float64) = sum over the fft_len/2 + 1 bins of |Ns[k]|^2 of the windowed noise frame
 * = (fft_len sum x^2 + (sum x)^2 + (sum (-1)^n x[n])^2) / 2, the three sums in float64 over the frame's samples.
 * mpx_noise_rms: per utterance u, rms[u] = sqrt(sum of power over its frames / (frames * (fft_len/2 + 1))) (float64,
 * optional, may be null; NaN for an utterance without frames), inv_gain[f] = 1 / rms[u] (float32, input of
 * mpx_synthesis_compressed_type2_ola).  The frames are added in a fixed order: an utterance's rms does not depend on
 * the batch it is in.
 */
int mpx_noise_power(void* stream, int fft_len, const float* noise, const int64_t* frame_pos, const int32_t* frame_left,
                    const int32_t* frame_right, const int32_t* frame_wtype, int64_t n_frames, double* power);
int mpx_noise_rms(void* stream, int fft_len, const double* power, const int32_t* utt_frame_off, int32_t n_utts,
                  float* inv_gain, double* rms);

/*
 * Maximum-likelihood parameter generation (MLPG): the smooth trajectory of an acoustic model's static / delta /
 * acceleration means and variances.  NOT taken from Merlin or bandmat (neither is at hand): the mathematics is stated in
 * DESIGN.md section 3.3n, parity with Merlin is unpinned.  Per utterance u (rows utt_frame_off[u] .. utt_frame_off[u + 1]
 * - 1 of every operand; utt_frame_off: device int32 [n_utts + 1]) and dimension d < D, with K = 1 + n_win streams
 * (stream 0 static, window (0, 1, 0); windows: HOST pointer to n_win x 3 float64 taps (w[-1], w[0], w[+1]); n_win 1 or 2):
 * W_k[t, t + j] = w_k[j], taps outside the utterance dropped; P_k = diag(1 / var[., k D + d]); A = sum_k W_k^T P_k W_k;
 * b = sum_k W_k^T P_k mean[., k D + d]; out[., d] = A^-1 b.
 * mpx_mlpg_solve: one lane per system (u, d), LDL^T of bandwidth 2 in float64.  mean: float32 (mean_f64 == 0) or float64
 * [total_frames x K D] at row pitch ld_mean (a column slice of a wider matrix: pass its first element and the matrix's
 * pitch); var likewise (var_f64, ld_var), ld_var == 0: ONE row for all frames (the global variance); every variance must
 * be finite and > 0 (not checked on the device).  out: float64 [total_frames x D] at ld_out.  work: float64
 * [mpx_mlpg_work_doubles(total_frames, D)], the factor rows as two [total_frames x D] planes.  rhs_direct != 0: mean is
 * the right-hand side itself, [total_frames x D] at ld_mean, and out = A^-1 mean (the backward pass: z = A^-1 g).
 * No atomics; a system's result does not depend on the batch it is in; nothing outside an utterance's rows is read.
 * mpx_mlpg_apply: y[t, k D + d] = [1 / var[t, k D + d]] (W_k x)[t, d], one thread per element; x: float32 / float64
 * [total_frames x D] at ld_x; var as above, or null: no precision factor (the dynamic features of x); y: float64
 * [total_frames x K D] at ld_y.  With var it is the tail of the backward pass: d L / d mean_k = P_k W_k z.
 * Both return 0 without a launch when total_frames or n_utts is 0.
 */
int64_t mpx_mlpg_work_doubles(int64_t total_frames, int32_t D);
int mpx_mlpg_solve(void* stream, const void* mean, int32_t mean_f64, int64_t ld_mean, const void* var, int32_t var_f64,
                   int64_t ld_var, const int32_t* utt_frame_off, int32_t n_utts, int64_t total_frames, int32_t D,
                   int32_t n_win, const double* windows, int32_t rhs_direct, double* out, int64_t ld_out, double* work);
int mpx_mlpg_apply(void* stream, const void* x, int32_t x_f64, int64_t ld_x, const void* var, int32_t var_f64,
                   int64_t ld_var, const int32_t* utt_frame_off, int32_t n_utts, int64_t total_frames, int32_t D,
                   int32_t n_win, const double* windows, double* y, int64_t ld_y);

/*
 * Variance gradients of MLPG and the trajectory likelihood ("variances").  Operands are typed and
 * pitched as in mpx_mlpg_solve (float32 / float64, any row pitch, ld_var == 0: the global row); all arithmetic and every
 * output is float64; no atomics, deterministic; an element's or a system's result does not depend on the batch it is in;
 * nothing outside an utterance's rows is read.  Every entry returns 0 without a launch when total_frames or n_utts is 0.
 * mpx_mlpg_var_backward: g[t, k D + d] = -p^2 (W_k z)[t, d] (mean[t, k D + d] - (W_k c)[t, d]), p = 1 / var[t, k D + d]: the
 * gradient of a loss on the trajectory with respect to the variances, for z = A^-1 dL/dc (mpx_mlpg_solve, rhs_direct) and
 * the trajectory c, both float64 [total_frames x D].  g: float64 [total_frames x K D] at ld_g.  With ld_var == 0 it also
 * writes gsum [K D], the column sums of g over all rows (the gradient of the global row), through work
 * [mpx_mlpg_colsum_work_doubles(total_frames, K D)]; gsum and work may be null otherwise.
 * mpx_mlpg_column_sums: sums[col] = sum over the rows of x [total_frames x width] (float64 at ld_x): per column one
 * partial sum per tile of 128 rows, rows in ascending order, then the tiles in ascending order -- the same bits every run.
 * mpx_mlpg_trajectory_nll: nll[u D + d] = -log N(x[., d]; c[., d], A^-1) of utterance u, one lane per system, for the
 * trajectory c of a preceding mpx_mlpg_solve launch and the static target x [total_frames x D]:
 * 1/2 sum_k sum_t p_k[t] (W_k (x - c))[t]^2 - 1/2 sum_i log d_i + F/2 log 2 pi, d_i the pivots of the LDL^T factor; 0 for
 * an utterance without frames.  nll: float64 [n_utts x D].
 * mpx_mlpg_trajectory_nll_backward: the gradients of sum go[u D + d] nll[u D + d], one lane per system:
 * g_mean[t, k D + d] = -go p (W_k (x - c))[t] and g_var[t, k D + d] = -go p^2 ((W_k e)^2 / 2 - (W_k e)(mean - W_k c) - s_k / 2)
 * with s_k[t] = (W_k A^-1 W_k^T)[t, t] from the band of A^-1, e = x - c; both float64 [total_frames x K D]; either may be
 * null (not computed).  work: float64 [mpx_mlpg_nll_work_doubles(total_frames, D)] (the factor as three planes), needed
 * with g_var.  With ld_var == 0 the gradient of the global row is mpx_mlpg_column_sums of g_var.
 */
int64_t mpx_mlpg_colsum_work_doubles(int64_t total_frames, int64_t width);
int mpx_mlpg_column_sums(void* stream, const double* x, int64_t ld_x, int64_t total_frames, int64_t width, double* sums,
                         double* work);
int mpx_mlpg_var_backward(void* stream, const double* z, int64_t ld_z, const double* c, int64_t ld_c, const void* mean,
                          int32_t mean_f64, int64_t ld_mean, const void* var, int32_t var_f64, int64_t ld_var,
                          const int32_t* utt_frame_off, int32_t n_utts, int64_t total_frames, int32_t D, int32_t n_win,
                          const double* windows, double* g, int64_t ld_g, double* gsum, double* work);
int mpx_mlpg_trajectory_nll(void* stream, const double* c, int64_t ld_c, const void* x, int32_t x_f64, int64_t ld_x,
                            const void* var, int32_t var_f64, int64_t ld_var, const int32_t* utt_frame_off, int32_t n_utts,
                            int64_t total_frames, int32_t D, int32_t n_win, const double* windows, double* nll);
int64_t mpx_mlpg_nll_work_doubles(int64_t total_frames, int32_t D);
int mpx_mlpg_trajectory_nll_backward(void* stream, const void* mean, int32_t mean_f64, int64_t ld_mean, const void* var,
                                     int32_t var_f64, int64_t ld_var, const double* c, int64_t ld_c, const void* x,
                                     int32_t x_f64, int64_t ld_x, const double* go, const int32_t* utt_frame_off,
                                     int32_t n_utts, int64_t total_frames, int32_t D, int32_t n_win, const double* windows,
                                     double* g_mean, int64_t ld_gm, double* g_var, int64_t ld_gv, double* work);

/* ------------------------------------------------------------------------------------------------------------------
 * Acoustic composition (magphase_cmp.hip): the inverse of MLPG's stream split.  No counterpart in
 * the reference but la.interp_unv_regions (libaudio.py:273-291), the interpolation of the carried stream.
 *
 * The layout: n_streams <= 16 streams of dims[s] >= 1 columns (dims: HOST int32).  The static matrix x [total_frames x SD],
 * SD = sum dims, holds their statics side by side; a composed row has W = K SD + vuv columns, K = n_win + 1 (n_win 0, 1 or
 * 2; windows: HOST float64 [n_win x 3] taps (w[-1], w[0], w[+1])): stream s as [static | delta | acc] from column
 * K (dims[0] + ... + dims[s - 1]), then one voicing column.  utt_frame_off: device int32 [n_utts + 1].  interp_stream: the
 * stream carried through unvoiced frames (every column of it), or -1.  Every entry returns 0 without a launch for
 * total_frames == 0 or n_utts == 0, and MPX_ERR_ARG for null or inconsistent arguments.
 *
 * mpx_cmp_voiced_neighbours: frame t of an utterance is voiced where v[(row0 + t) ld_v] > 0 (float32 / float64; NaN:
 * unvoiced).  nb: device int32 [2 x total_frames]: nb[r] = the last voiced frame <= t, nb[total_frames + r] = the first
 * voiced frame >= t, utterance-relative, -1 without one.
 *
 * mpx_cmp_compose: out[r, c] = ((sum_j w_k[j] x~[t + j, .]) - mean[c]) / std[c], taps outside the utterance dropped; x~ = x
 * but in the carried stream, where an unvoiced frame holds the line through the voiced frames on either side, the nearest
 * voiced value before the first / after the last, unv_fill without any (interp_zeros: 0 in every unvoiced frame); the
 * voicing column is 1 in voiced frames, else 0.  The value stored in an unvoiced entry of the carried stream is never
 * loaded.  mean, std: device float64 [W], or both null.  Float64 arithmetic without fused multiply-adds, one rounding on
 * the store; out: float32 (out_f64: float64) [total_frames x W] at row pitch ld_out.
 *
 * mpx_cmp_compose_backward: gx [total_frames x SD] (float64) = the gradient of sum g . out with respect to x; g: float32
 * [total_frames x W].  Unvoiced entries of the carried stream get exactly 0.  One writer per element, no atomics.
 *
 * mpx_cmp_column_moments: out[0] = total_frames, out[1 .. 1 + width) = the column sums, out[1 + width .. 1 + 2 width) = the
 * sums of (x - sum / total_frames)^2, each summed over tiles of 128 rows in ascending order, then over the tiles in
 * ascending order (mpx_mlpg_column_sums' order).  work: float64 [mpx_cmp_moments_work_doubles(total_frames, width)].
 * ------------------------------------------------------------------------------------------------------------------ */
int mpx_cmp_voiced_neighbours(void* stream, const void* v, int32_t v_f64, int64_t ld_v, const int32_t* utt_frame_off,
                              int32_t n_utts, int64_t total_frames, int32_t* nb);
int mpx_cmp_compose(void* stream, const void* x, int32_t x_f64, int64_t ld_x, const int32_t* dims, int32_t n_streams,
                    int32_t interp_stream, int32_t interp_zeros, double unv_fill, int32_t vuv, const int32_t* nb,
                    const int32_t* utt_frame_off, int32_t n_utts, int64_t total_frames, int32_t n_win,
                    const double* windows, const double* mean, const double* std_dev, void* out, int32_t out_f64,
                    int64_t ld_out);
int mpx_cmp_compose_backward(void* stream, const float* g, int64_t ld_g, const int32_t* dims, int32_t n_streams,
                             int32_t interp_stream, int32_t vuv, const int32_t* nb, const int32_t* utt_frame_off,
                             int32_t n_utts, int64_t total_frames, int32_t n_win, const double* windows,
                             const double* std_dev, double* gx, int64_t ld_gx);
int64_t mpx_cmp_moments_work_doubles(int64_t total_frames, int64_t width);
int mpx_cmp_column_moments(void* stream, const void* x, int32_t x_f64, int64_t ld_x, int64_t total_frames, int64_t width,
                           double* out, double* work);

/*
 * MagPhase post-filter (magphase.py:2300-2378, Q20) on [n_frames x dim] log-mel magnitudes.  half_len: int32
 * [nx_last - nx_first + 1] half lengths of the centred moving average of bins nx_first..nx_last (host table,
 * magphase.py:2342-2344); tilt: float32[dim] enhancement factors (np.linspace(boost_at_zero, boost_at_nyq, dim)).
 */
int mpx_post_filter(void* stream, const float* mag_mel_log, int64_t n_frames, int32_t dim, const int32_t* half_len,
                    int32_t nx_first, int32_t nx_last, const float* tilt, float* out);

/*
 * Backward of mpx_post_filter (k_post_filter_bwd).  The forward is linear per frame, y = x M^T; grad_in = grad_out M, as a
 * gather: per input bin i the cover_cnt[i] output bins cover_idx[t * dim + i] whose window holds bin i (its own among them)
 * and their weights cover_w[t * dim + i] = M[idx][i], t < fan -- hostmath.post_filter_backward_tables, built from the
 * forward's half_len / tilt tables.  grad_out, grad_in: float32 [n_frames x dim] (3 <= dim <= 256, 1 <= fan <= dim).
 * Deterministic (no atomics, every element written once); table entries outside the row are clamped into it.
 */
int mpx_post_filter_backward(void* stream, const float* grad_out, int64_t n_frames, int32_t dim, const int32_t* cover_cnt,
                             const int32_t* cover_idx, const float* cover_w, int32_t fan, float* grad_in);

/*
 * Output high-pass filter (magphase.py:981-995: scipy.signal.butter(4, 40 Hz) + lfilter) in float64 on the device,
 * as a cascade of the two second-order sections of the same Butterworth design (scipy output='sos'), each run as
 * a blocked scan: zero-state recurrence per block of mpx_hpf_block() samples, block end states chained per
 * utterance through A^B, free responses added from G[n] = C A^n.  (The 4th-order direct form cannot be chained in
 * float64: clustered poles at |z| ~ 0.997.  The cascade agrees with lfilter to ~1e-7 of peak = lfilter's own noise.)
 * sos_host: HOST pointer to 2 x 6 float64 (b0 b1 b2 a0 a1 a2 per section); pmat: float64 [2 x 4] (A^B row-major per
 * section); gtab: float64 [2 x B x 2]; blk_off: int32[n_utts+1] cumulative block counts; zend/zstart: float64
 * scratch [total_blocks x 2]; y_tmp, y: float64 [total samples] (y = output).  Tables: hostmath.hpf_tables.
 */
int mpx_hpf_block(void);
int mpx_output_hpf(void* stream, const float* pcm, const int64_t* out_off, const int32_t* blk_off, int32_t n_utts,
                   int64_t max_len, const double* sos_host, const double* pmat, const double* gtab, double* zend,
                   double* zstart, double* y_tmp, double* y);

/* ------------------------------------------------------------------------------------------------------------------
 * Built-in epoch / voicing front end.  NOT REAPER (libaudio.py:450-455 shells out to it): parity
 * unpinned, opt-in (magphase_amd/epochs.py documents the algorithm and its quality checks).  Batched over utterances.
 * ------------------------------------------------------------------------------------------------------------------ */

/*
 * F0 / voicing candidates: box-decimation by `dec` (to ~4 kHz), then per 5 ms frame the normalised cross-correlation
 * for n_lags lags starting at l_min; the shortest lag within 0.06 of the best is refined by a parabola.
 * sig: float32 PCM, utterances at off[0..n_utts]; dec_off / frame_off: int64[n_utts+1] offsets of the decimated
 * signals (scratch xd, float64) and of the frames in the outputs; means: float64[2 n_utts] scratch.
 * Outputs per frame: f0 (fs_d / lag), peak (NCCF at the chosen lag), energy (sum of squares of the frame's window).
 */
int mpx_epoch_f0_track(void* stream, const float* sig, const int64_t* off, int32_t n_utts, int32_t dec,
                       const int64_t* dec_off, int64_t max_dec_len, double* xd, double* means, const int64_t* frame_off,
                       int64_t max_frames, int32_t hop, int32_t win, int32_t l_min, int32_t n_lags, double fs_d,
                       float* f0, float* peak, float* energy);

/*
 * Epoch candidates by zero-frequency filtering: x differenced, through two zero-frequency resonators (cumulative
 * sums, float64) with the local mean over 2 half_win[u] + 1 samples removed after the first and three times after the
 * second; then the zero crossings of both directions of the result.  List p of utterance u (p = 0: negative-going,
 * 1: positive-going) holds counts[2u + p] entries at [(2u + p) * cap ...): sample index, |slope|, and the excitation
 * energy of the w_score samples after the crossing minus the w_score before it (which direction carries the epochs
 * depends on the recording's polarity: the host keeps the one with the larger mean score).  Entries are unordered.
 * cross_frac (may be null): the zero of the line through the two samples of the sign change, as the fraction of a sample
 * BEFORE sample index cross_idx (0 .. 1): sub-sample crossing position = cross_idx - cross_frac.
 * buf_a/b/c: float64 scratch of the total sample count each.
 */
int mpx_epoch_zff(void* stream, const float* sig, const int64_t* off, int32_t n_utts, int64_t max_len,
                  const int32_t* half_win, int32_t w_score, double* buf_a, double* buf_b, double* buf_c, int32_t cap,
                  int32_t* counts, int32_t* cross_idx, float* cross_slope, float* cross_score, float* cross_frac);

/*
 * 16-bit PCM of the synthesised utterances for the wav writer (libaudio.py:352-365 write_audio_file, Q17): per
 * utterance v = norm * y / max|y| in float64 (skipped when norm <= 0), then lrint(v * 0x7FFF) as libsndfile converts
 * floats to PCM_16 -- the host form's IEEE operations in the same order, so the samples are bit-identical to
 * la.write_audio_file's.  y: float64 (y_is_f64 != 0; the output of mpx_output_hpf) or float32 samples, utterances
 * concatenated at out_off (int64[n_utts+1]); peaks: float64[n_utts] scratch (receives max|y|); out: int16, same layout.
 */
int mpx_pcm16(void* stream, const void* y, int32_t y_is_f64, const int64_t* out_off, int32_t n_utts, int64_t max_len,
              double norm, double* peaks, int16_t* out);

/*
 * int16 PCM -> float32 samples in [-1, 1) (x / 32768, exact): the conversion la.read_audio_file's caller needs
 * (libaudio.py:369-377 returns float64 in [-1, 1); the analysis reads float32, magphase.py:2869-2879), done on the
 * device so that 16-bit wavs cross PCIe as int16.  pcm: DEVICE int16[n], 8-byte aligned; out: DEVICE float32[n],
 * 16-byte aligned.
 */
int mpx_pcm16_to_f32(void* stream, const int16_t* pcm, int64_t n, float* out);

/*
 * Merlin / HTS style post-filter of the log mel magnitudes (magphase.py:3375-3465: the reference pipes each utterance
 * through nine SPTK-3.9 binaries -- x2x | freqt | c2acr, vopr, mc2b | bcp | merge | b2mc -- SPTK restated from its published
 * algorithms, PARITY UNPINNED) for all frames of a batch (csrc/magphase_merlin.hip):
 *   mcep = x . c1 (la.rceps 'log' / 'compact' as a matrix);  mcep_w = mcep * lifter (1, 1, pf, pf, ...);
 *   r0, p_r0 = sum_k wk[k] exp(2 (mcep | mcep_w) . g)[k]   (frame energy: freqt to the linear axis + c2acr -M 0 -l 4096);
 *   b = mc2b(mcep_w, alpha); b[0] += ln(r0 / p_r0) / 2; mcep_pf = b2mc(b, alpha);  out = mcep_pf . cf, NaN -> magic.
 * mag_mel_log, out: float32 [n_frames x dim] (3 <= dim <= 64); c1, cf: [dim x dim]; lifter: [dim]; g: [dim x n_bins];
 * wk: [n_bins] (hostmath.merlin_tables builds them in float64); mcep, mcep_w: scratch [n_frames x dim]; r0, p_r0: scratch
 * [n_frames].  Deterministic (no atomics).
 */
int mpx_post_filter_merlin(void* stream, const float* mag_mel_log, int64_t n_frames, int32_t dim, const float* c1,
                           const float* lifter, const float* g, const float* wk, int32_t n_bins, double alpha,
                           const float* cf, double magic, float* mcep, float* mcep_w, float* r0, float* p_r0, float* out);

/*
 * Backward of mpx_post_filter_merlin: grad_in = the gradient with respect to mag_mel_log, given grad_out, the gradient
 * with respect to the forward's output (the chain mc2b | b[0] += delta | b2mc taken as mcep_pf = mcep_w + delta e0, which
 * it is in exact arithmetic):
 *   mcep, mcep_w recomputed from mag_mel_log (k_rows_gemm);  grad_pf = grad_out . cf_t (k_rows_gemm);
 *   grad_mcep = lifter * (grad_pf - g_d Q(mcep_w)) + g_d Q(mcep), g_d = grad_pf[0], Q(v) = S(v) / R(v),
 *     R(v) = sum_k wk[k] exp(2 (v . g)[k]), S(v)[n] = sum_k wk[k] exp(2 (v . g)[k]) g[n][k]   (k_merlin_r0_bwd);
 *   grad_in = grad_mcep . c1_t (k_rows_gemm).
 * cf_t, c1_t: the forward's cf and c1 transposed, [dim x dim]; the other tables as the forward's.  mcep, mcep_w, grad_pf,
 * grad_mcep: scratch [n_frames x dim] -- nothing of n_frames x n_bins is stored.  A frame whose R is not a positive finite
 * number for either coefficient set (the forward wrote magic, or an infinity, there) gets an all-zero grad_in row.
 * Deterministic (no atomics).
 */
int mpx_post_filter_merlin_backward(void* stream, const float* mag_mel_log, const float* grad_out, int64_t n_frames,
                                    int32_t dim, const float* c1, const float* lifter, const float* g, const float* wk,
                                    int32_t n_bins, const float* cf_t, const float* c1_t, float* mcep, float* mcep_w,
                                    float* grad_pf, float* grad_mcep, float* grad_in);

/*
 * Memory-rate probe (csrc/magphase_probe.hip; measurement only, not on the MagPhase path): one streaming float4 kernel
 * over n_floats (a multiple of 4) elements.  mode = kind + 16 * shape: kind 0 reads `a` (b: one float of scratch), kind 1
 * fills `a`, kind 2 copies a -> b; shape < mpx_bw_probe_shapes() selects the launch shape (grid x block, independent
 * 16-byte accesses in flight per lane, non-temporal bit; shape 0 = 2048 x 256 with one access in flight).  bench.py times
 * every shape with HIP events and quotes the best per kind as the device's own streaming read / write / copy ceilings
 * beside the 8 TB/s spec peak in its roofline object.  The reference has no counterpart.
 */
int mpx_bw_probe_shapes(void);
int mpx_bw_probe(void* stream, int32_t mode, float* a, float* b, int64_t n_floats);

/*
 * Feature rows that already live in device memory, gathered into a plan's dense float32 buffers (csrc/magphase_pack.hip,
 * k_rows_pack): what Engine.stage_rows + upload_staged do for host arrays, for rows an acoustic model left on the GPU.
 * One launch serves n_utts utterances and n_streams <= 3 streams (mag | real | imag) of different widths.
 *
 * Descriptor table: n_streams * n_utts entries of mpx_pack_desc, 32 bytes each, entry [s * n_utts + u] = utterance u of
 * stream s:
 *   base        DEVICE pointer to element [0, 0] of the utterance's rows (any element alignment)
 *   row_stride  elements between the starts of two rows (>= 0; the column stride is 1)
 *   dtype       element type code: MPX_PACK_F32 0, MPX_PACK_F16 1, MPX_PACK_BF16 2, MPX_PACK_F64 3
 *   n_rows      rows of this utterance (0: nothing is read, base may be NULL)
 *   out_row0    its first row in the stream's output; within a stream the entries follow one another:
 *               out_row0[0] = 0, out_row0[u + 1] = out_row0[u] + n_rows[u], and the last one ends at rows_s
 * table: the DEVICE copy the kernel reads; table_host: the same bytes in HOST memory, checked in full before the launch
 * (type codes, sizes, the tiling above), so that every store lands inside [0, rows_s) x [0, width_s) of its stream.
 *
 * Stream s: out_s DEVICE float32, row r at out_s + r * ld_s (ld_s >= width_s: width_s for the dense `coef` layout of the
 * compressed synthesis plan, Engine.empty_feats' pitch for lossless features), rows_s rows of width_s columns.  Arguments
 * of streams >= n_streams are ignored.
 * Conversion: f16 and bf16 widen exactly; f64 narrows round-to-nearest-even (numpy's astype(float32)); f32 is copied bit
 * for bit (NaN payloads, -0).  n_utts == 0 and utterances without rows launch nothing.
 * Returns MPX_ERR_ARG for a null table with n_utts > 0, an unknown type code, negative sizes or a table that does not
 * tile the outputs -- all detected on the host, without a device.
 */
#define MPX_PACK_F32 0
#define MPX_PACK_F16 1
#define MPX_PACK_BF16 2
#define MPX_PACK_F64 3
typedef struct {
    const void* base;
    int64_t row_stride;
    int32_t dtype;
    int32_t n_rows;
    int64_t out_row0;
} mpx_pack_desc;
int mpx_rows_pack(void* stream, const mpx_pack_desc* table, const mpx_pack_desc* table_host, int32_t n_utts,
                  int32_t n_streams, float* out0, int32_t width0, int64_t ld0, int64_t rows0, float* out1, int32_t width1,
                  int64_t ld1, int64_t rows1, float* out2, int32_t width2, int64_t ld2, int64_t rows2);

/* ------------------------------------------------------------------------------------------------------------------
 * Host-side file helpers of the batch scripts (csrc/magphase_host.cpp; no device work, no stream).  Called from the
 * reader / writer threads of iobatch.py: the FFI call drops the interpreter lock, so reading, computing and writing overlap.
 * ------------------------------------------------------------------------------------------------------------------ */

/*
 * Batch planners (csrc/magphase_plan.cpp): the reference's float64 / integer index arithmetic for all utterances of a
 * batch in one call, the same IEEE-754 operation sequence as the numpy forms in magphase_amd/hostmath.py / engine.py
 * (np.round = half to even, astype(int) = truncation, sequential cumsum).  All pointers are HOST memory.  A negative
 * return value -(u + 2) names utterance u as the one the numpy form would raise on; -1 = bad arguments.
 *
 * mpx_host_plan_analysis: libaudio.py:435-447 (epoch clean-up), magphase.py:77-98 (frame bounds), :2198-2207 (f0).
 *   pm_sec, voi [ep_off[n_utts]]: epochs (seconds) and voicing flags, utterance u at [ep_off[u], ep_off[u+1]);
 *   n_smpls, fs [n_utts]; sig_off [n_utts]: offset of the utterance's samples in the batch's sample buffer.
 *   Outputs (capacity = number of epochs): pos = rounded epoch + sig_off, pm = rounded epoch, left / right = distances to
 *   the neighbouring epochs (0 and n_smpls - 1 at the ends), f0 = voi * fs / left; frame_off [n_utts + 1].
 *   Returns the total number of frames.
 */
int64_t mpx_host_plan_analysis(int32_t n_utts, const double* pm_sec, const double* voi, const int64_t* ep_off,
                               const int64_t* n_smpls, const double* fs, const int64_t* sig_off, int64_t* pos,
                               int64_t* pm_out, int64_t* left, int64_t* right, double* f0, int64_t* frame_off);

/*
 * mpx_host_plan_analysis_batch: the WHOLE host side of a lossless / compressed analysis launch in one call, the utterances
 * given by pointer (nothing is concatenated by the caller), on n_threads threads -- what the reference does once per
 * utterance in its Pool worker (libutils.py:32-63; scripts/batch_feature_extraction_for_tts.py:40-57):
 *   - the samples of all utterances copied into `stage`, the page-locked buffer the H2D DMA reads (stage_kind 0: every
 *     utterance is int16, staged as int16 and widened on the device by mpx_pcm16_to_f32; 1: float32, int16 * 2^-15 /
 *     float64 rounded to nearest even; pcm_kind[u] 0 int16, 1 float32, 2 float64; stage may be null: no copy);
 *   - mpx_host_plan_analysis' arithmetic per utterance (libaudio.py:435-447, magphase.py:77-98, :2198-2207) with the device
 *     tables written in their final types: pos int64, left32 / right32 int32, voi32 float32 (f0 > 0; may be null);
 *   - host results: pm, left64 (the reference's v_shift), f0, f0_med = scipy.signal.medfilt(f0) per utterance (kernel 3,
 *     zero-padded; magphase.py:2499-2500; may be null), frame_off [n_utts + 1];
 *   - frames longer than fft_len (the reference warns once per such frame, magphase.py:311-315): their global frame index
 *     and length in long_frame / long_len (capacity long_cap), their number in *n_long_out (fft_len <= 0: not looked for).
 * Every per-frame output has capacity sum(n_epochs).  Returns the number of frames, -(u + 2) for the first utterance the
 * numpy form raises on (no epochs), -1 for bad arguments.
 */
int64_t mpx_host_plan_analysis_batch(int32_t n_utts, const void* const* pcm, const int32_t* pcm_kind,
                                     const int64_t* n_smpls, const double* fs, const double* const* pm_sec,
                                     const double* const* voi, const int64_t* n_epochs, void* stage, int32_t stage_kind,
                                     int64_t* pos, int32_t* left32, int32_t* right32, float* voi32, int64_t* pm_out,
                                     int64_t* left64, double* f0, double* f0_med, int64_t* frame_off, int32_t fft_len,
                                     int64_t* long_frame, int64_t* long_len, int64_t long_cap, int64_t* n_long_out,
                                     int32_t n_threads);

/*
 * mpx_host_plan_synthesis: the per-utterance part of synthesis_from_compressed before any spectrum (magphase.py:846-848
 * f0 -> voicing / shifts, :861-868 constant -> variable rate via mpx_host_const_to_var_scan, :879-882 epochs and noise
 * length, :77-98 noise frame bounds, :969-973 anti-ringing window lengths, :34-62 OLA offsets).  f0 = exp(lf0) of the
 * rows [row_off[u], row_off[u+1]) (the caller evaluates the exp).  Per-frame outputs have capacity `cap` (2 x rows is
 * always enough); row0 / row1 index the batch's coefficient rows; npos is relative to the batch's noise buffer.
 * Returns the total number of (variable-rate) frames.
 */
int64_t mpx_host_plan_synthesis(int32_t n_utts, const double* f0, const int64_t* row_off, double fs, int32_t fft_len,
                                int32_t b_const_rate, int32_t b_voi_ap_win, int64_t cap, int64_t* v_shift, int64_t* v_pm,
                                int64_t* npos, int32_t* nleft, int32_t* nright, int32_t* wtype, int32_t* voiced,
                                int32_t* row0, int32_t* row1, double* rowt, int32_t* win_l, int32_t* win_r,
                                int64_t* pm_rel, int64_t* frame_off, int64_t* ns_len_out, int64_t* out_start,
                                int64_t* out_len);

/*
 * mpx_host_plan_lossless_synthesis: synthesis_from_lossless's epochs and OLA offsets (magphase.py:1771-1772: v_pm =
 * cumsum(f0_to_shift(f0, fs)).astype(int) -- float cumsum, then truncation (Q3); :34-62) for the utterances
 * [frame_off[u], frame_off[u+1]) of f0.  Outputs v_pm, pm_rel [frames], out_start, out_len [n_utts].
 */
int64_t mpx_host_plan_lossless_synthesis(int32_t n_utts, const double* f0, const int64_t* frame_off, const double* fs,
                                         int32_t fft_len, int64_t* v_pm, int64_t* pm_rel, int64_t* out_start,
                                         int64_t* out_len);

/*
 * mpx_host_ola_runs: the run planner of mpx_synthesis_lossless_ola / mpx_synthesis_compressed_ola (see mpx_ola_run) in
 * its default mode: the batch's frames are cut at `gcuts` (equal shares of the frame sequence, one per wave-pair slot)
 * and at utterance boundaries; cuts that would let non-adjacent runs overlap are dropped.  pm_rel / frame_off: frame
 * positions relative to each utterance's first frame; starts / out_lens: ola's kept part per utterance; out_offs:
 * utterance offsets in pcm_out.  Returns the number of runs written (capacity n_utts + n_gcuts is always enough).
 */
int64_t mpx_host_ola_runs(int32_t n_utts, const int64_t* pm_rel, const int64_t* frame_off, const int64_t* starts,
                          const int64_t* out_lens, const int64_t* out_offs, int32_t fft_len, const int64_t* gcuts,
                          int64_t n_gcuts, mpx_ola_run* runs, int64_t cap_runs);
/*
 * The same with per-frame extents (int32 [frames][2], global frame index: the half-open range of a frame's samples that
 * can be non-zero, 0 <= ext_lo <= ext_hi <= fft_len; mpx_roundtrip_frame_extents).  A run then ends where its frames'
 * extents end (never before its predecessor's end), its successor's head strip ends there, and a fix range begins no
 * earlier than the successor's first extent: the seams move no zeros.  Everything outside the extents must be an exact
 * zero the kernel never adds.  extents == NULL: mpx_host_ola_runs' result.  Bit-identical to hostmath.ola_runs(extents=).
 */
int64_t mpx_host_ola_runs_extents(int32_t n_utts, const int64_t* pm_rel, const int64_t* frame_off, const int64_t* starts,
                                  const int64_t* out_lens, const int64_t* out_offs, int32_t fft_len, const int64_t* gcuts,
                                  int64_t n_gcuts, const int32_t* extents, mpx_ola_run* runs, int64_t cap_runs);

/*
 * mpx_host_deal_cuts: cuts for mpx_host_ola_runs that deal the frames by COST instead of by count.  Frame f costs slot s
 * sum_k coef[s][k] * terms[f][k] (terms: int32 [n_frames][n_terms], coef: int32 [n_slots][n_terms], none negative; the
 * sums are int64).  Finds the smallest integer T for which the greedy fill -- slots 0, 1, ... each take the longest run of
 * consecutive frames whose summed cost is <= T -- consumes every frame, and writes that fill's cuts: cuts[0] == 0,
 * ascending, cuts[n_slots] == n_frames (trailing slots may be empty); *t_out = T (may be null).  Integer arithmetic only:
 * bit-identical to hostmath.deal_cuts.  Returns 0, or -1 on bad arguments.
 */
int64_t mpx_host_deal_cuts(const int32_t* terms, int64_t n_frames, int32_t n_terms, const int32_t* coef, int32_t n_slots,
                           int64_t* cuts, int64_t* t_out);

/*
 * mpx_host_plan_synthesis_batch: the whole host side of a compressed-feature synthesis launch (what the reference does per
 * utterance in scripts/batch_waveform_generation.py:28-58 -> magphase.py:3229-3275 -> :836-897, :969-976), utterances by
 * pointer, on n_threads threads:
 *   - the coefficient matrices (kind[u] 1 float32 / 2 float64, C-contiguous [n_rows[u] x mag_dim | phase_dim]) copied /
 *     narrowed into `stage` (page-locked, float32) as [R x mag_dim | R x phase_dim | R x phase_dim], R = sum n_rows; null:
 *     no copy;
 *   - mpx_host_plan_synthesis' arithmetic per utterance on f0 = exp(lf0) (concatenated, evaluated by the caller with
 *     numpy's exp), mpx_host_ola_runs over n_slots slots (wcum / wsum: np.concatenate(([0.], np.cumsum(w))) and w.sum() of
 *     the slots' float64 weights, null = equal shares), the slots' work lists and, with want_tiles, the frames of every
 *     31-row tile of the coefficient matrix (mpx_mel_unwarp_rows);
 *   - every device table written in its final type into `desc` (page-locked; one H2D copy), table k at byte offset
 *     desc_off[k], 256-byte aligned, in this order: utt_frame_off i32[U+1], npos i64[F], nleft, nright, wtype, voiced i32[F],
 *     tile_first i32[tiles+1], row0, row1 i32[F], rowt f32[F], win_l, win_r, pm_rel i32[F], out_start i32[U], out_off
 *     i64[U+1], runs (mpx_ola_run[n_runs]), slot_off i32[slots+1], slot_runs i32[n_runs]      (desc_off: int64[18]);
 *   - host results: v_shift, v_pm (int64), voiced_host (int32) with capacity 2 R + 2 U; frame_off [U+1]; ns_len, out_start,
 *     out_len [U]; runs_host (capacity runs_cap >= U + n_slots + 1);
 *     counts[8] = {frames, runs, slots in use, bytes of desc in use, noise samples, output samples, tiles + 1, R}.
 * Returns the number of frames; -(u + 2): the numpy form raises on utterance u; -4000000: weighted shares and fewer frames
 * than slots (counts[0] = frames: call again with n_slots = frames and the first `frames` weights' cumsum / sum); other
 * values <= -1000000: a capacity / table-order case left to the numpy form; -1: bad arguments.
 */
int64_t mpx_host_plan_synthesis_batch(int32_t n_utts, const void* const* mag, const void* const* real,
                                      const void* const* imag, const int32_t* kind, const int64_t* n_rows,
                                      int32_t mag_dim, int32_t phase_dim, float* stage, const double* f0, double fs,
                                      int32_t fft_len, int32_t b_const_rate, int32_t b_voi_ap_win, int32_t n_slots,
                                      const double* wcum, double wsum, int32_t want_tiles, uint8_t* desc,
                                      int64_t desc_cap, int64_t* desc_off, int64_t* v_shift, int64_t* v_pm,
                                      int32_t* voiced_host, int64_t* frame_off, int64_t* ns_len, int64_t* out_start,
                                      int64_t* out_len, mpx_ola_run* runs_host, int64_t runs_cap, int64_t* counts,
                                      int32_t n_threads);

/* dst[i] = (double)src[i], i < n, on a few threads: the float32 -> float64 widening of the array API's outputs (the
 * reference's arrays are float64, magphase.py:457-476; numpy's astype is one thread at ~1.5 GB/s). */
int32_t mpx_host_widen_f32(const float* src, double* dst, int64_t n, int32_t n_threads);

/* n byte ranges src[i][0 .. nbytes[i]) copied to dst + dst_off[i] on n_threads threads (HOST pointers): the samples of a
 * batch's utterances into the page-locked staging buffer of the analysis plan.  Returns 0, or MPX_ERR_ARG. */
int32_t mpx_host_copy_many(int32_t n, const void* const* src, const int64_t* nbytes, const int64_t* dst_off, void* dst,
                           int32_t n_threads);

/* dst[i] = (float)src[i] (round to nearest even, numpy's astype), i < n, on a few threads: the array API's float64 inputs
 * on their way to the device. */
int32_t mpx_host_narrow_f64(const double* src, float* dst, int64_t n, int32_t n_threads);

/* sizes[i] = size of paths[i] in bytes, or -errno. */
int32_t mpx_host_file_sizes(int32_t n, const char* const* paths, int64_t* sizes);

/*
 * np.loadtxt(est_file, skiprows=skiprows, usecols=[0, 1]) for n files at once (libaudio.py:421-447 read_reaper_est_file's
 * read): the first two whitespace-separated columns of every non-blank line after `skiprows` lines, as float64 (correctly
 * rounded decimal -> binary, the values strtod gives).  File i writes its rows to col0 / col1 [row_off[i], row_off[i+1])
 * (HOST float64); counts[i] = rows, or -errno (-EINVAL: a row with one column, -ENOSPC: more rows than its slice holds;
 * a file has at most size / 4 + 1 rows).  n_threads <= 1: in the calling thread.
 */
int32_t mpx_host_read_est_batch(int32_t n, const char* const* paths, int32_t skiprows, const int64_t* row_off,
                                double* col0, double* col1, int64_t* counts, int32_t n_threads);

/*
 * n files written at once: headers[i] (header_bytes[i] bytes; headers may be NULL) followed by bodies[i]
 * (body_bytes[i] bytes) -- lu.write_binfile (libutils.py:193-199) for the feature files, the RIFF header + samples of
 * la.write_audio_file (libaudio.py:352-365) for wavs.  status[i] = 0 or errno.
 */
int32_t mpx_host_write_files(int32_t n, const char* const* paths, const void* const* headers, const int64_t* header_bytes,
                             const void* const* bodies, const int64_t* body_bytes, int32_t* status, int32_t n_threads);

/* n files read at once into bufs[i] (at most cap[i] bytes): got[i] = bytes read or -errno (lu.read_binfile's np.fromfile). */
int32_t mpx_host_read_files(int32_t n, const char* const* paths, void* const* bufs, const int64_t* cap, int64_t* got,
                            int32_t n_threads);


#ifdef __cplusplus
}
#endif
#endif /* MAGPHASE_HIP_H */
