// magphase_output.hip -- the output stage of the synthesis paths and the 16-bit conversions.
//
//   k_post_filter                          log-mel post-filter (Q20)
//   k_hpf_*, k_peak_abs, k_pcm16(_to_f32)  high-pass filter of the output, peak normalisation, int16 conversion
#include "mpx_common.hpp"

namespace mpx {

// ---------------------------------------------------------------------------------------------
// post-filter (magphase.py:2300-2378, Q20) on the log-mel magnitude [F x D]: per bin a centred moving average of odd
// length lens[b] (host table, linearly shrinking/growing with frequency), enhancement
// y = (x - ave) * tilt[b] + ave, the two end bins copied.  One thread per (frame, bin); D <= 256.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_post_filter(const float* __restrict__ x, long long F, int D,
                                                     const int* __restrict__ half_len, int nx0, int nx1,
                                                     const float* __restrict__ tilt, float* __restrict__ y) {
    extern __shared__ float row[];   // rows_per_block x D
    const int rows_per_block = blockDim.x / D;
    const int rl = threadIdx.x / D, b = threadIdx.x - rl * D;
    const long long f = (long long)blockIdx.x * rows_per_block + rl;
    const bool live = (rl < rows_per_block) && (f < F);
    if (live) row[rl * D + b] = x[f * D + b];
    __syncthreads();
    if (!live) return;
    const float* r = row + rl * D;
    // averages exist for bins nx0..nx1 (inclusive); outside they repeat the boundary value (magphase.py:2357-2358:
    // v_ave[:v_nx[0]] = v_ave[v_nx[0]] ; v_ave[v_nx[-1]:] = v_ave[v_nx[-1]])
    const int bc = min(max(b, nx0), nx1);
    const int h = half_len[bc - nx0];
    float acc = 0.0f;
    for (int k = bc - h; k <= bc + h; ++k) acc += r[k];
    const float ave = acc / (float)(2 * h + 1);
    float out = (r[b] - ave) * tilt[b] + ave;
    if (b == 0 || b == D - 1) out = r[b];
    y[f * D + b] = out;
}

// ---------------------------------------------------------------------------------------------
// Backward of k_post_filter.  The forward is linear per frame, y = x M^T with
// M = diag(tilt) (I - A) + A, A the clamped moving average and the two end rows of M identity rows; the backward is
// g_x = g_y M as a GATHER over column i of M: one thread per (frame, input bin i) sums w[t][i] * g_y[idx[t][i]] over the
// cnt[i] output bins whose window covers bin i (the diagonal among them), in the table's order.  idx / w / cnt are
// hostmath.post_filter_backward_tables' inverse of the forward's half_len / tilt tables, [fan x D] with the entry t of
// bin i at t * D + i.  No atomics, every output written once.  Table entries are clamped into the row: a wrong table
// gives wrong numbers, never a read outside the frame.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_post_filter_bwd(const float* __restrict__ gy, long long F, int D,
                                                         const int* __restrict__ cnt, const int* __restrict__ idx,
                                                         const float* __restrict__ w, int fan, float* __restrict__ gx) {
    extern __shared__ float row[];   // rows_per_block x D
    const int rows_per_block = blockDim.x / D;
    const int rl = threadIdx.x / D, i = threadIdx.x - rl * D;
    const long long f = (long long)blockIdx.x * rows_per_block + rl;
    const bool live = (rl < rows_per_block) && (f < F);
    if (live) row[rl * D + i] = gy[f * D + i];
    __syncthreads();
    if (!live) return;
    const float* r = row + rl * D;
    const int n = min(max(cnt[i], 0), fan);
    float acc = 0.0f;
    for (int t = 0; t < n; ++t) acc = fmaf(w[t * D + i], r[min(max(idx[t * D + i], 0), D - 1)], acc);
    gx[f * D + i] = acc;
}

// ---------------------------------------------------------------------------------------------
// output high-pass (magphase.py:981-995: butter(4, 40 Hz) + lfilter), float64, blocked scan over a CASCADE of two
// second-order sections.  Each section's direct-form-II-transposed recurrence
//   y = b0 x + z0 ; z0 = b1 x + z1 - a1 y ; z1 = b2 x - a2 y
// is linear in (z, x): k_hpf_zero_state runs it per block of kHpfBlock samples from z = 0 (parallel over blocks),
// k_hpf_carry chains the block end states z_{j+1} = A^B z_j + zs_j per utterance (2x2, serial, tiny), k_hpf_apply adds
// each block's free response G[n] . z_start (G[n] = C A^n, host table).  Why a cascade: chaining the states of the
// 4th-order direct form is hopeless in float64 (four poles at |z| ~ 0.997 within 0.005 of each other: A^1024 has
// entries of 3e8 and the block hand-over loses everything -- measured), while the biquads' tables stay below 120.
// The cascade differs from scipy's direct-form lfilter by ~1e-7 of peak, which is lfilter's own round-off noise.
// ---------------------------------------------------------------------------------------------
// Round 5: on the corpus generation path (32 utterances per launch) the two section passes took 0.57 ms of the launch's
// 2.8 ms of device time -- one THREAD per 1024-sample block, every lane of a wave reading its own cache line.  Now a
// block is 256 samples and a WAVE takes 64 consecutive blocks of an utterance: 64 x 64 tiles go through LDS (row stride
// 65 doubles: the wave-wide loads / stores are 64 consecutive samples, a lane's serial pass reads its own row without bank
// conflicts), and the carry kernel is one wave per utterance with the block states staged through LDS the same way.
constexpr int kHpfBlock = 256;
constexpr int kHpfTile = 64;                    // samples of a block per LDS pass (and blocks per wave)
constexpr int kHpfTileStride = kHpfTile + 1;    // doubles per LDS row

struct BiquadCoef {
    double b0, b1, b2, a1, a2;
};

// cg / cz (second section only): the PREVIOUS section's free response is added while loading -- x[n] + G[n mod 256] . z_start
// of the block -- instead of by a k_hpf_apply pass over the whole signal in between (0.49 GB of traffic per 128 utterances).
template <typename TIn>
__global__ __launch_bounds__(64) void k_hpf_zero_state(const TIn* __restrict__ x, const long long* __restrict__ off,
                                                       const int* __restrict__ blk_off, BiquadCoef c,
                                                       double* __restrict__ y, double* __restrict__ zend,
                                                       const double* __restrict__ cg, const double* __restrict__ cz) {
    // one wave per 64 consecutive blocks of an utterance, lane t = block 64 blockIdx.x + t; blk_off[u] = first global
    // block index of utterance u
    __shared__ double tile[kHpfTile * kHpfTileStride];
    const int u = blockIdx.y;
    const int nb = blk_off[u + 1] - blk_off[u];
    const int j0 = blockIdx.x * 64;
    if (j0 >= nb) return;
    const int t = threadIdx.x;
    const long long base = off[u] + (long long)j0 * kHpfBlock;   // first sample of the wave's blocks
    const long long end = off[u + 1];
    __shared__ double czs[2 * kHpfTile];
    if (cg) {   // start states of the wave's 64 blocks in the previous section
        const int jb = min(j0 + t, nb - 1);
        czs[2 * t] = cz[2 * (long long)(blk_off[u] + jb)];
        czs[2 * t + 1] = cz[2 * (long long)(blk_off[u] + jb) + 1];
        __syncthreads();
    }
    double z0 = 0, z1 = 0;
    for (int ch = 0; ch < kHpfBlock / kHpfTile; ++ch) {
        // row r = block j0 + r, its samples [ch * 64, ch * 64 + 64): lane t loads column t of every row (coalesced)
        {   // all 64 row loads in flight before the first LDS write (eight at a time left the pass waiting on memory
            // latency: 266 us per 128 utterances; see the round-5 notes)
            TIn xv[kHpfTile];
#pragma unroll
            for (int r = 0; r < kHpfTile; ++r) {
                const long long n = base + (long long)r * kHpfBlock + ch * kHpfTile + t;
                xv[r] = x[min(n, end - 1)];
            }
            double g0 = 0.0, g1 = 0.0;
            if (cg) {
                g0 = cg[2 * (ch * kHpfTile + t)];
                g1 = cg[2 * (ch * kHpfTile + t) + 1];
            }
#pragma unroll
            for (int r = 0; r < kHpfTile; ++r) {
                const long long n = base + (long long)r * kHpfBlock + ch * kHpfTile + t;
                double xd = (double)xv[r];
                if (cg) xd += g0 * czs[2 * r] + g1 * czs[2 * r + 1];   // the same operations as k_hpf_apply's
                tile[r * kHpfTileStride + t] = (n < end) ? xd : 0.0;
            }
        }
        __syncthreads();
        {   // the lane's row into registers first: 64 independent LDS reads in flight, then the recurrence alone is the chain
            double v[kHpfTile];
#pragma unroll
            for (int i = 0; i < kHpfTile; ++i) v[i] = tile[t * kHpfTileStride + i];
#pragma unroll
            for (int i = 0; i < kHpfTile; ++i) {
                const double xv = v[i];
                const double yv = c.b0 * xv + z0;
                z0 = c.b1 * xv + z1 - c.a1 * yv;
                z1 = c.b2 * xv - c.a2 * yv;
                v[i] = yv;
            }
#pragma unroll
            for (int i = 0; i < kHpfTile; ++i) tile[t * kHpfTileStride + i] = v[i];
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < kHpfTile; ++r) {
            const long long n = base + (long long)r * kHpfBlock + ch * kHpfTile + t;
            if (n < end) y[n] = tile[r * kHpfTileStride + t];
        }
        __syncthreads();
    }
    // (a block that ends before its 256th sample ran on zero padding: its end state is never used -- it is the
    // utterance's last block)
    if (j0 + t < nb) {
        double* ze = zend + 2 * (long long)(blk_off[u] + j0 + t);
        ze[0] = z0;
        ze[1] = z1;
    }
}

__global__ __launch_bounds__(64) void k_hpf_carry(const int* __restrict__ blk_off, int n_utts,
                                                  const double* __restrict__ pmat /* A^B, row-major 2x2 */,
                                                  const double* __restrict__ zend, double* __restrict__ zstart) {
    // z_{j+1} = P z_j + e_j over an utterance's blocks (e_j = the zero-state end state of block j), one wave per utterance,
    // 64 blocks per step as a SCAN across the lanes: after log-step k lane t holds sum_{t - 2^{k+1} < i <= t} P^{t-i} e_i
    // (c_t += P^{2^k} c_{t - 2^k}), so block t starts from P^t z_tile + c_{t-1} -- 6 exchange steps per 64 blocks instead
    // of 64 dependent LDS round trips (the serial form: 59 us per 32 utterances of 938 blocks).
    const int u = blockIdx.x;
    if (u >= n_utts) return;
    const int g0 = blk_off[u], g1 = blk_off[u + 1], t = threadIdx.x;
    double pw[7][4];   // P^(2^k)
    pw[0][0] = pmat[0], pw[0][1] = pmat[1], pw[0][2] = pmat[2], pw[0][3] = pmat[3];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const double a = pw[k][0], b = pw[k][1], c = pw[k][2], d = pw[k][3];
        pw[k + 1][0] = a * a + b * c;
        pw[k + 1][1] = a * b + b * d;
        pw[k + 1][2] = c * a + d * c;
        pw[k + 1][3] = c * b + d * d;
    }
    double q0 = 1.0, q1 = 0.0, q2 = 0.0, q3 = 1.0;   // P^t of this lane (binary expansion of t)
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        if ((t >> k) & 1) {
            const double a = q0 * pw[k][0] + q1 * pw[k][2], b = q0 * pw[k][1] + q1 * pw[k][3];
            const double c = q2 * pw[k][0] + q3 * pw[k][2], d = q2 * pw[k][1] + q3 * pw[k][3];
            q0 = a, q1 = b, q2 = c, q3 = d;
        }
    }
    double zt0 = 0.0, zt1 = 0.0;   // state at the start of the tile
    for (int g = g0; g < g1; g += 64) {
        const int cnt = min(64, g1 - g);
        const double e0 = (t < cnt) ? zend[2 * (long long)(g + t)] : 0.0;
        const double e1 = (t < cnt) ? zend[2 * (long long)(g + t) + 1] : 0.0;
        double c0 = e0, c1 = e1;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const double o0 = __shfl_up(c0, 1 << k), o1 = __shfl_up(c1, 1 << k);
            if (t >= (1 << k)) {
                c0 += pw[k][0] * o0 + pw[k][1] * o1;
                c1 += pw[k][2] * o0 + pw[k][3] * o1;
            }
        }
        double m0 = __shfl_up(c0, 1), m1 = __shfl_up(c1, 1);   // c_{t-1}
        if (t == 0) m0 = m1 = 0.0;
        const double zs0 = q0 * zt0 + q1 * zt1 + m0, zs1 = q2 * zt0 + q3 * zt1 + m1;
        if (t < cnt) {
            zstart[2 * (long long)(g + t)] = zs0;
            zstart[2 * (long long)(g + t) + 1] = zs1;
        }
        // the state after block t = one more step of the recurrence; the next tile starts from lane cnt - 1's
        const double n0 = pw[0][0] * zs0 + pw[0][1] * zs1 + e0, n1 = pw[0][2] * zs0 + pw[0][3] * zs1 + e1;
        zt0 = __shfl(n0, cnt - 1);
        zt1 = __shfl(n1, cnt - 1);
    }
}

__global__ __launch_bounds__(256) void k_hpf_apply(const long long* __restrict__ off, const int* __restrict__ blk_off,
                                                   const double* __restrict__ gtab /* [kHpfBlock x 2] */,
                                                   const double* __restrict__ zstart, double* __restrict__ y) {
    const int u = blockIdx.y;
    const long long len = off[u + 1] - off[u];
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= len) return;
    const int j = (int)(t / kHpfBlock), r = (int)(t - (long long)j * kHpfBlock);
    const double* z = zstart + 2 * (long long)(blk_off[u] + j);
    y[off[u] + t] += gtab[2 * r] * z[0] + gtab[2 * r + 1] * z[1];
}

// ---------------------------------------------------------------------------------------------
// 16-bit PCM for the wav writer (libaudio.py:352-365, Q17, as soundfile / libsndfile writes it): per utterance
// v = norm * y / max|y| in float64, then lrint(v * 0x7FFF) (round half to even; no clipping of in-range input).  Same
// IEEE operations in the same order as the host form (la.write_audio_file) -- __dmul_rn / __ddiv_rn keep the compiler
// from fusing them -- so the samples are bit-identical; the device hands the writer thread ready int16 samples and the
// D2H copy is a quarter of the float64 one.  k_peak_abs: one block per utterance; k_pcm16: one thread per sample.
// ---------------------------------------------------------------------------------------------
constexpr int kPeakPerThread = 16;   // elements per thread of k_peak_abs
template <typename T>
__global__ __launch_bounds__(256) void k_peak_abs(const T* __restrict__ y, const long long* __restrict__ off,
                                                  double* __restrict__ peak) {
    // peak[u] = max |y| over utterance u; peak[] zeroed by the caller.  blockIdx.y = utterance, 4096 elements per block
    // (one block per utterance ran 240 us per 32 x 5 s: a single wave front of loads in flight per CU).  The maximum is
    // order-independent, so the result is the serial one bit for bit; non-negative doubles order like their bit patterns.
    __shared__ double s_max[256];
    const int u = blockIdx.y;
    const long long b0 = off[u] + (long long)blockIdx.x * (256 * kPeakPerThread), b1 = off[u + 1];
    if (b0 >= b1) return;
    double m = 0.0;
#pragma unroll
    for (int k = 0; k < kPeakPerThread; ++k) {
        const long long i = b0 + k * 256 + threadIdx.x;
        if (i < b1) m = fmax(m, fabs((double)y[i]));
    }
    s_max[threadIdx.x] = m;
    __syncthreads();
    for (int k = 128; k >= 1; k >>= 1) {
        if (threadIdx.x < k) s_max[threadIdx.x] = fmax(s_max[threadIdx.x], s_max[threadIdx.x + k]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        // (fmax drops NaNs, as the serial chain did: s_max[0] is a non-negative number)
        atomicMax(reinterpret_cast<unsigned long long*>(peak + u), (unsigned long long)__double_as_longlong(s_max[0]));
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_pcm16(const T* __restrict__ y, const long long* __restrict__ off,
                                               const double* __restrict__ peak, double norm, short* __restrict__ out) {
    const int u = blockIdx.y;
    const long long i = off[u] + (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= off[u + 1]) return;
    double v = (double)y[i];
    if (norm > 0.0) v = __ddiv_rn(__dmul_rn(norm, v), peak[u]);
    const double r = rint(__dmul_rn(v, 32767.0));
    // NaN (a silent utterance: 0 / 0) is written as 0, as the host form stores it -- fmax / fmin alone would pick the
    // bound, -32768: a full-scale DC file instead of silence
    out[i] = (r != r) ? (short)0 : (short)fmin(fmax(r, -32768.0), 32767.0);
}

// int16 PCM -> float32 in [-1, 1): x * 2^-15, exact (what the host did with np.multiply before uploading float32 --
// the int16 samples cross PCIe at half the bytes and the host pass is gone).  4 samples per thread.
__global__ __launch_bounds__(256) void k_pcm16_to_f32(const short* __restrict__ in, long long n, float* __restrict__ out) {
    const long long i = 4 * ((long long)blockIdx.x * 256 + threadIdx.x);
    if (i + 3 < n) {
        const short4 v = *reinterpret_cast<const short4*>(in + i);
        *reinterpret_cast<float4*>(out + i) = make_float4((float)v.x * (1.0f / 32768.0f), (float)v.y * (1.0f / 32768.0f),
                                                          (float)v.z * (1.0f / 32768.0f), (float)v.w * (1.0f / 32768.0f));
    } else {
        for (long long k = i; k < n; ++k) out[k] = (float)in[k] * (1.0f / 32768.0f);
    }
}

}  // namespace mpx

using namespace mpx;

extern "C" {

int mpx_post_filter(void* stream, const float* mag_mel_log, int64_t n_frames, int32_t dim, const int32_t* half_len,
                    int32_t nx_first, int32_t nx_last, const float* tilt, float* out) {
    if (n_frames < 0 || dim < 3 || dim > 256) return fail(MPX_ERR_ARG, "mpx_post_filter: dim must be in 3..256%s");
    if (nx_first < 0 || nx_last >= dim || nx_first > nx_last) return fail(MPX_ERR_ARG, "mpx_post_filter: bad bin range%s");
    if (n_frames == 0) return MPX_OK;
    if (!mag_mel_log || !half_len || !tilt || !out) return fail(MPX_ERR_ARG, "mpx_post_filter: null pointer%s");
    const int rows = 256 / dim;
    const dim3 grid((unsigned)((n_frames + rows - 1) / rows)), block(256);
    hipLaunchKernelGGL(k_post_filter, grid, block, sizeof(float) * (size_t)rows * dim, (hipStream_t)stream,
                       mag_mel_log, (long long)n_frames, (int)dim, half_len, (int)nx_first, (int)nx_last, tilt, out);
    MPX_HIP_CHECK(hipGetLastError());
    return MPX_OK;
}

int mpx_post_filter_backward(void* stream, const float* grad_out, int64_t n_frames, int32_t dim, const int32_t* cover_cnt,
                             const int32_t* cover_idx, const float* cover_w, int32_t fan, float* grad_in) {
    if (n_frames < 0 || dim < 3 || dim > 256) return fail(MPX_ERR_ARG, "mpx_post_filter_backward: dim must be in 3..256%s");
    if (fan < 1 || fan > dim) return fail(MPX_ERR_ARG, "mpx_post_filter_backward: fan must be in 1..dim%s");
    if (n_frames == 0) return MPX_OK;
    if (!grad_out || !cover_cnt || !cover_idx || !cover_w || !grad_in)
        return fail(MPX_ERR_ARG, "mpx_post_filter_backward: null pointer%s");
    const int rows = 256 / dim;
    const dim3 grid((unsigned)((n_frames + rows - 1) / rows)), block(256);
    hipLaunchKernelGGL(k_post_filter_bwd, grid, block, sizeof(float) * (size_t)rows * dim, (hipStream_t)stream, grad_out,
                       (long long)n_frames, (int)dim, cover_cnt, cover_idx, cover_w, (int)fan, grad_in);
    MPX_HIP_CHECK(hipGetLastError());
    return MPX_OK;
}

int mpx_pcm16(void* stream, const void* y, int32_t y_is_f64, const int64_t* out_off, int32_t n_utts, int64_t max_len,
              double norm, double* peaks, int16_t* out) {
    if (n_utts < 0 || max_len < 0) return fail(MPX_ERR_ARG, "mpx_pcm16: negative size%s");
    if (n_utts == 0 || max_len == 0) return MPX_OK;
    if (!y || !out_off || !peaks || !out) return fail(MPX_ERR_ARG, "mpx_pcm16: null pointer%s");
    if (n_utts > 65535) return fail(MPX_ERR_ARG, "mpx_pcm16: at most 65535 utterances per call%s");
    hipStream_t s = (hipStream_t)stream;
    const dim3 g2((unsigned)((max_len + 255) / 256), (unsigned)n_utts);
    const dim3 gp((unsigned)((max_len + 256 * kPeakPerThread - 1) / (256 * kPeakPerThread)), (unsigned)n_utts);
    MPX_HIP_CHECK(hipMemsetAsync(peaks, 0, sizeof(double) * (size_t)n_utts, s));
    if (y_is_f64) {
        hipLaunchKernelGGL(k_peak_abs<double>, gp, dim3(256), 0, s, (const double*)y, (const long long*)out_off, peaks);
        hipLaunchKernelGGL(k_pcm16<double>, g2, dim3(256), 0, s, (const double*)y, (const long long*)out_off, peaks, norm, (short*)out);
    } else {
        hipLaunchKernelGGL(k_peak_abs<float>, gp, dim3(256), 0, s, (const float*)y, (const long long*)out_off, peaks);
        hipLaunchKernelGGL(k_pcm16<float>, g2, dim3(256), 0, s, (const float*)y, (const long long*)out_off, peaks, norm, (short*)out);
    }
    MPX_HIP_CHECK(hipGetLastError());
    return MPX_OK;
}

int mpx_pcm16_to_f32(void* stream, const int16_t* pcm, int64_t n, float* out) {
    if (n < 0) return fail(MPX_ERR_ARG, "mpx_pcm16_to_f32: negative size%s");
    if (n == 0) return MPX_OK;
    if (!pcm || !out) return fail(MPX_ERR_ARG, "mpx_pcm16_to_f32: null pointer%s");
    if (((uintptr_t)pcm & 7) || ((uintptr_t)out & 15)) return fail(MPX_ERR_ARG, "mpx_pcm16_to_f32: pcm must be 8-byte, out 16-byte aligned%s");
    const long long blocks = (n + 1023) / 1024;
    hipLaunchKernelGGL(k_pcm16_to_f32, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const short*)pcm,
                       (long long)n, out);
    MPX_HIP_CHECK(hipGetLastError());
    return MPX_OK;
}

int mpx_hpf_block(void) { return kHpfBlock; }

int mpx_output_hpf(void* stream, const float* pcm, const int64_t* out_off, const int32_t* blk_off, int32_t n_utts,
                   int64_t max_len, const double* sos_host, const double* pmat, const double* gtab, double* zend,
                   double* zstart, double* y_tmp, double* y) {
    if (n_utts < 0 || max_len < 0) return fail(MPX_ERR_ARG, "mpx_output_hpf: negative size%s");
    if (n_utts == 0 || max_len == 0) return MPX_OK;
    if (!pcm || !out_off || !blk_off || !sos_host || !pmat || !gtab || !zend || !zstart || !y_tmp || !y)
        return fail(MPX_ERR_ARG, "mpx_output_hpf: null pointer%s");
    if (n_utts > 65535) return fail(MPX_ERR_ARG, "mpx_output_hpf: at most 65535 utterances per call%s");
    hipStream_t s = (hipStream_t)stream;
    const unsigned max_blocks = (unsigned)((max_len + kHpfBlock - 1) / kHpfBlock);
    const dim3 gz((max_blocks + 63) / 64, (unsigned)n_utts), gc((unsigned)n_utts),
        ga((unsigned)((max_len + 255) / 256), (unsigned)n_utts);
    for (int sec = 0; sec < 2; ++sec) {
        const double* q = sos_host + 6 * sec;   // scipy sos row: b0 b1 b2 a0 a1 a2
        const BiquadCoef c{q[0] / q[3], q[1] / q[3], q[2] / q[3], q[4] / q[3], q[5] / q[3]};
        double* out = (sec == 0) ? y_tmp : y;
        // section 0's free response is folded into section 1's loads: no k_hpf_apply pass over y_tmp in between
        if (sec == 0)
            hipLaunchKernelGGL(k_hpf_zero_state<float>, gz, dim3(64), 0, s, pcm, (const long long*)out_off, blk_off, c,
                               out, zend, (const double*)nullptr, (const double*)nullptr);
        else
            hipLaunchKernelGGL(k_hpf_zero_state<double>, gz, dim3(64), 0, s, (const double*)y_tmp,
                               (const long long*)out_off, blk_off, c, out, zend, gtab, (const double*)zstart);
        // (section 1's zero-state pass has consumed zstart: the carry may overwrite it -- same stream, in order)
        hipLaunchKernelGGL(k_hpf_carry, gc, dim3(64), 0, s, blk_off, (int)n_utts, pmat + 4 * sec, zend, zstart);
        if (sec == 1)
            hipLaunchKernelGGL(k_hpf_apply, ga, dim3(256), 0, s, (const long long*)out_off, blk_off,
                               gtab + 2 * (size_t)kHpfBlock * sec, zstart, out);
    }
    MPX_HIP_CHECK(hipGetLastError());
    return MPX_OK;
}

}  // extern "C"
