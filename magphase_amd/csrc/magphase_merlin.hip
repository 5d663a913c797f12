// magphase_merlin.hip -- Merlin / HTS style post-filter of the log mel magnitudes (magphase.py:3375-3465, SURVEY.md 8f
// rank 3) as batched device work.  The reference pipes every utterance through nine SPTK-3.9 binaries (x2x, freqt, c2acr,
// vopr, mc2b, bcp, sopr, merge, b2mc); SPTK is not available here, the arithmetic is restated from its published
// algorithms -- PARITY UNPINNED, held by the known-answer tests of tests/test_post_filter_merlin.py and, for this device
// form, by a -m gpu comparison with the host form (magphase_amd.magphase.post_filter_merlin, float64 with a float32
// rounding at every pipe boundary).  All frames of a batch at once:
//   k_rows_gemm     mcep   = x . C1            la.rceps('log', 'compact') as the [D x D] matrix it is
//                   mcep_w = mcep * lifter     (1, 1, pf, pf, ...)                                   (vopr -m)
//   k_merlin_r0     r0, p_r0 = mean over the 4096 bins of exp(2 Re FFT(freqt(mcep | mcep_w, 2047, alpha -> 0)))   (freqt | c2acr)
//                   = sum_k w_k exp(2 (c . G)[k]) with G [D x 2049] = freqt matrix x cosine matrix, built on the host:
//                   a [64 frames x D] . [D x 2049] product whose exp'd outputs are reduced on the fly -- nothing of the
//                   [F x 2049] spectra is written
//   k_merlin_b      b = mc2b(mcep_w); b[0] += ln(r0 / p_r0) / 2; mcep_pf = b2mc(b)                    (mc2b | bcp | merge | b2mc)
//   k_rows_gemm     out = mcep_pf . Cf         cosine matrix, alpha = 0 (la.mcep_to_sp_cosmat 'log'); NaN -> la.MAGIC
// float32 throughout: the pipe boundaries of the SPTK chain are float32 as well.
// The backward pass (mpx_post_filter_merlin_backward) reuses k_rows_gemm with host-transposed
// matrices around one new kernel, k_merlin_r0_bwd.
#include "mpx_common.hpp"

namespace mpx {

// out[f][i] = (sum_k a[f][k] * mat[k][i]) * (scale ? scale[i] : 1), K, n <= 64.  Optionally out2 = the unscaled product.
// 256 threads = 4 frames x 64 outputs; the matrix lives in LDS.
__global__ __launch_bounds__(256) void k_rows_gemm(const float* __restrict__ a, long long F, int K, int n,
                                                   const float* __restrict__ mat, const float* __restrict__ scale,
                                                   float* __restrict__ out_plain, float* __restrict__ out_scaled,
                                                   float nan_value, int replace_nan) {
    __shared__ float ms[64 * 65];
    __shared__ float as[4][64];
    for (int i = threadIdx.x; i < K * n; i += 256) ms[(i / n) * 65 + (i % n)] = mat[i];
    const int i = threadIdx.x & 63, r = threadIdx.x >> 6;
    for (long long f0 = (long long)blockIdx.x * 4; f0 < F; f0 += (long long)gridDim.x * 4) {
        __syncthreads();
        const long long f = f0 + r;
        if (f < F && i < K) as[r][i] = a[f * K + i];
        __syncthreads();
        if (f < F && i < n) {
            float acc = 0.0f;
            for (int k = 0; k < K; ++k) acc = fmaf(as[r][k], ms[k * 65 + i], acc);
            if (replace_nan && acc != acc) acc = nan_value;
            if (out_plain) out_plain[f * n + i] = acc;
            if (out_scaled) out_scaled[f * n + i] = acc * (scale ? scale[i] : 1.0f);
        }
    }
}

// r0[f] = sum_k w[k] exp(2 sum_n c[f][n] G[n][k]) for TWO coefficient sets (c1 -> r1, c2 -> r2) against the same G.
// One workgroup = 64 frames; thread t: frame t & 63, bins 16 (t >> 6) .. + 15 of every 64-bin chunk.  G chunk and both
// coefficient tiles in LDS; a wave's 64 lanes share their G values (broadcast reads), every lane its own frame's
// coefficients (row stride D + 1: conflict-free).  Deterministic: fixed summation order, no atomics.
__global__ __launch_bounds__(256) void k_merlin_r0(const float* __restrict__ c1, const float* __restrict__ c2,
                                                   long long F, int D, const float* __restrict__ G,
                                                   const float* __restrict__ wk, int nb, float* __restrict__ r1,
                                                   float* __restrict__ r2) {
    __shared__ float gs[64][64 + 4];    // [n][bin of the chunk]
    __shared__ float a1[64][65], a2[64][65];
    __shared__ float part[2][4][64];
    const int fl = threadIdx.x & 63, q = rfl((int)(threadIdx.x >> 6));
    const long long f0 = (long long)blockIdx.x * 64;
    for (int i = threadIdx.x; i < 64 * D; i += 256) {
        const int r = i / D, n = i % D;
        const long long f = min(f0 + r, F - 1);
        a1[r][n] = c1[f * D + n];
        a2[r][n] = c2[f * D + n];
    }
    float s1 = 0.0f, s2 = 0.0f;
    for (int k0 = 0; k0 < nb; k0 += 64) {
        __syncthreads();
        for (int i = threadIdx.x; i < D * 64; i += 256) {
            const int n = i >> 6, kb = i & 63;
            gs[n][kb] = (k0 + kb < nb) ? G[(long long)n * nb + k0 + kb] : 0.0f;
        }
        __syncthreads();
        float acc1[16], acc2[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) acc1[e] = acc2[e] = 0.0f;
        for (int n = 0; n < D; ++n) {
            const float x1 = a1[fl][n], x2 = a2[fl][n];
            const float4* g4 = reinterpret_cast<const float4*>(&gs[n][16 * q]);
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const float4 g = g4[v];
                acc1[4 * v + 0] = fmaf(x1, g.x, acc1[4 * v + 0]);
                acc1[4 * v + 1] = fmaf(x1, g.y, acc1[4 * v + 1]);
                acc1[4 * v + 2] = fmaf(x1, g.z, acc1[4 * v + 2]);
                acc1[4 * v + 3] = fmaf(x1, g.w, acc1[4 * v + 3]);
                acc2[4 * v + 0] = fmaf(x2, g.x, acc2[4 * v + 0]);
                acc2[4 * v + 1] = fmaf(x2, g.y, acc2[4 * v + 1]);
                acc2[4 * v + 2] = fmaf(x2, g.z, acc2[4 * v + 2]);
                acc2[4 * v + 3] = fmaf(x2, g.w, acc2[4 * v + 3]);
            }
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int k = k0 + 16 * q + e;
            const float w = (k < nb) ? wk[k] : 0.0f;
            s1 = fmaf(w, expf(2.0f * acc1[e]), s1);
            s2 = fmaf(w, expf(2.0f * acc2[e]), s2);
        }
    }
    part[0][q][fl] = s1;
    part[1][q][fl] = s2;
    __syncthreads();
    if (threadIdx.x < 64 && f0 + threadIdx.x < F) {
        const int t = threadIdx.x;
        r1[f0 + t] = (part[0][0][t] + part[0][1][t]) + (part[0][2][t] + part[0][3][t]);
        r2[f0 + t] = (part[1][0][t] + part[1][1][t]) + (part[1][2][t] + part[1][3][t]);
    }
}

// Per frame: b = mc2b(mcep_w) (b[m] = mc[m] - alpha b[m + 1], from the top down); b[0] += ln(r0 / p_r0) / 2;
// mcep_pf = b2mc(b) (mc[m] = b[m] + alpha b[m + 1]).  One thread per frame, the D coefficients in registers' stead in a
// small per-thread loop over global memory (D floats per frame: 13 MB for 57 k frames).
__global__ __launch_bounds__(256) void k_merlin_b(const float* __restrict__ mcw, long long F, int D, float alpha,
                                                  const float* __restrict__ r0, const float* __restrict__ p_r0,
                                                  float* __restrict__ out) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const float* x = mcw + f * D;
    float* y = out + f * D;
    float b_next = x[D - 1];            // b[D-1] = mc[D-1]
    y[D - 1] = b_next;                  // mcep_pf[D-1] = b[D-1]
    for (int m = D - 2; m >= 0; --m) {
        float b = x[m] - alpha * b_next;                        // mc2b
        if (m == 0) b += 0.5f * logf(r0[f] / p_r0[f]);        // vopr -d | sopr -LN -d 2 | vopr -a, merged into b[0]
        y[m] = b + alpha * b_next;                              // b2mc (b[m+1] of the unmodified tail: only b[0] changes)
        b_next = b;
    }
}

// ---------------------------------------------------------------------------------------------
// Backward of k_merlin_r0 and of the b[0] correction of k_merlin_b in one kernel.  In exact
// arithmetic mc2b | b[0] += delta | b2mc is mcep_pf = mcep_w + delta e0 with delta = (ln R(mcep) - ln R(mcep_w)) / 2 and
// R(v) = sum_k w_k exp(2 (v . G)_k), so with g_pf the gradient with respect to mcep_pf and g_d = g_pf[0]
//   g_c = lifter * (g_pf - g_d Q(mcep_w)) + g_d Q(mcep),   Q(v)[n] = S(v)[n] / R(v),  S(v)[n] = sum_k w_k exp(2 (v . G)_k) G[n][k]
// is the gradient with respect to mcep.  One workgroup = 64 frames; per 64-bin chunk of G, for both coefficient sets:
//   1. k_merlin_r0's product and exponentials, same roles and same summation order (R equals the forward's r0 / p_r0 bit for
//      bit): thread t = frame t & 63, bins 16 (t >> 6) .. + 15; the weighted exponentials E = w exp(.) go to LDS as [frame][bin];
//   2. S += E[64 frames x 64 bins] . G^T[64 bins x D] on v_mfma_f32_16x16x4_f32 in the shape of k_mel_unwarp_bwd: wave w owns
//      frames 16 w .. 16 w + 15 and every 16-wide tile of n, lane group g takes bins 16 g + 4 q + {0..3} of step q, a fresh
//      accumulator per chunk, the chunk sums added up in chunk order.
// Nothing of the [F x n_bins] spectra leaves the chip.  Bins past n_bins are staged as G = 0, w = 0 (E = 0); rows n >= D of
// the G tile are zero.  A frame whose R is not a positive finite number for either set (the forward's ln(r0 / p_r0) is NaN
// or infinite there: it wrote MAGIC, or +-Inf) gets g_c = 0; the select keeps its NaN / Inf inside the kernel, and a
// frame's sums never touch another frame's.  Deterministic: fixed summation order, no atomics, every output written once.
// ---------------------------------------------------------------------------------------------
using f32x4 = __attribute__((ext_vector_type(4))) float;
constexpr int kMerlinStride = 64 + 4;   // floats per LDS row of the G and E tiles (k_merlin_r0's padding; float4 reads)

template <int NT>
__device__ __forceinline__ void merlin_r0_bwd_block(const float* __restrict__ c1, const float* __restrict__ c2,
                                                    const float* __restrict__ gpf, const float* __restrict__ lifter,
                                                    long long F, int D, const float* __restrict__ G,
                                                    const float* __restrict__ wk, int nb, float* __restrict__ gc,
                                                    float (*gs)[kMerlinStride], float (*e1)[kMerlinStride],
                                                    float (*e2)[kMerlinStride], float (*a1)[65], float (*a2)[65],
                                                    float (*part)[4][64]) {
    const int fl = threadIdx.x & 63, q = rfl((int)(threadIdx.x >> 6));   // roles of step 1 (k_merlin_r0's)
    const int li = fl & 15, lg = fl >> 4;                                 // fragment roles of step 2; q is the wave
    const long long f0 = (long long)blockIdx.x * 64;
    for (int i = threadIdx.x; i < 64 * D; i += 256) {
        const int r = i / D, n = i % D;
        const long long f = min(f0 + r, F - 1);
        a1[r][n] = c1[f * D + n];
        a2[r][n] = c2[f * D + n];
    }
    for (int i = threadIdx.x; i < (64 - D) * kMerlinStride; i += 256) gs[D][i] = 0.0f;   // rows D..63: never staged
    float s1 = 0.0f, s2 = 0.0f;
    f32x4 tot1[NT], tot2[NT];
#pragma unroll
    for (int jt = 0; jt < NT; ++jt) tot1[jt] = tot2[jt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int k0 = 0; k0 < nb; k0 += 64) {
        __syncthreads();   // the previous chunk's fragment reads are done
        for (int i = threadIdx.x; i < D * 64; i += 256) {
            const int n = i >> 6, kb = i & 63;
            gs[n][kb] = (k0 + kb < nb) ? G[(long long)n * nb + k0 + kb] : 0.0f;
        }
        __syncthreads();
        float acc1[16], acc2[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) acc1[e] = acc2[e] = 0.0f;
        for (int n = 0; n < D; ++n) {
            const float x1 = a1[fl][n], x2 = a2[fl][n];
            const float4* g4 = reinterpret_cast<const float4*>(&gs[n][16 * q]);
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const float4 g = g4[v];
                acc1[4 * v + 0] = fmaf(x1, g.x, acc1[4 * v + 0]);
                acc1[4 * v + 1] = fmaf(x1, g.y, acc1[4 * v + 1]);
                acc1[4 * v + 2] = fmaf(x1, g.z, acc1[4 * v + 2]);
                acc1[4 * v + 3] = fmaf(x1, g.w, acc1[4 * v + 3]);
                acc2[4 * v + 0] = fmaf(x2, g.x, acc2[4 * v + 0]);
                acc2[4 * v + 1] = fmaf(x2, g.y, acc2[4 * v + 1]);
                acc2[4 * v + 2] = fmaf(x2, g.z, acc2[4 * v + 2]);
                acc2[4 * v + 3] = fmaf(x2, g.w, acc2[4 * v + 3]);
            }
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int k = k0 + 16 * q + e;
            const float w = (k < nb) ? wk[k] : 0.0f;
            const float x1 = expf(2.0f * acc1[e]), x2 = expf(2.0f * acc2[e]);
            s1 = fmaf(w, x1, s1);
            s2 = fmaf(w, x2, s2);
            acc1[e] = w * x1;
            acc2[e] = w * x2;
        }
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            *reinterpret_cast<float4*>(&e1[fl][16 * q + 4 * v]) =
                float4{acc1[4 * v + 0], acc1[4 * v + 1], acc1[4 * v + 2], acc1[4 * v + 3]};
            *reinterpret_cast<float4*>(&e2[fl][16 * q + 4 * v]) =
                float4{acc2[4 * v + 0], acc2[4 * v + 1], acc2[4 * v + 2], acc2[4 * v + 3]};
        }
        __syncthreads();
        f32x4 p1[NT], p2[NT];
#pragma unroll
        for (int jt = 0; jt < NT; ++jt) p1[jt] = p2[jt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int col = 16 * lg + 4 * s;
            const float4 u1 = *reinterpret_cast<const float4*>(&e1[16 * q + li][col]);
            const float4 u2 = *reinterpret_cast<const float4*>(&e2[16 * q + li][col]);
            float4 bq[NT];
#pragma unroll
            for (int jt = 0; jt < NT; ++jt) bq[jt] = *reinterpret_cast<const float4*>(&gs[16 * jt + li][col]);
#pragma unroll
            for (int jt = 0; jt < NT; ++jt) {
                p1[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(u1.x, bq[jt].x, p1[jt], 0, 0, 0);
                p2[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(u2.x, bq[jt].x, p2[jt], 0, 0, 0);
            }
#pragma unroll
            for (int jt = 0; jt < NT; ++jt) {
                p1[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(u1.y, bq[jt].y, p1[jt], 0, 0, 0);
                p2[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(u2.y, bq[jt].y, p2[jt], 0, 0, 0);
            }
#pragma unroll
            for (int jt = 0; jt < NT; ++jt) {
                p1[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(u1.z, bq[jt].z, p1[jt], 0, 0, 0);
                p2[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(u2.z, bq[jt].z, p2[jt], 0, 0, 0);
            }
#pragma unroll
            for (int jt = 0; jt < NT; ++jt) {
                p1[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(u1.w, bq[jt].w, p1[jt], 0, 0, 0);
                p2[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(u2.w, bq[jt].w, p2[jt], 0, 0, 0);
            }
        }
#pragma unroll
        for (int jt = 0; jt < NT; ++jt) {
            tot1[jt] += p1[jt];
            tot2[jt] += p2[jt];
        }
    }
    part[0][q][fl] = s1;
    part[1][q][fl] = s2;
    __syncthreads();
    // C: column li of tile jt (n = 16 jt + li), row 4 lg + r of this wave's 16 frames
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int t = 16 * q + 4 * lg + r;
        const long long f = f0 + t;
        if (f >= F) continue;
        const float R1 = (part[0][0][t] + part[0][1][t]) + (part[0][2][t] + part[0][3][t]);   // k_merlin_r0's r1, r2
        const float R2 = (part[1][0][t] + part[1][1][t]) + (part[1][2][t] + part[1][3][t]);
        const bool ok = R1 > 0.0f && R1 < INFINITY && R2 > 0.0f && R2 < INFINITY;
        const float gd = gpf[f * D];
#pragma unroll
        for (int jt = 0; jt < NT; ++jt) {
            const int n = 16 * jt + li;
            if (n >= D) continue;
            const float v = lifter[n] * (gpf[f * D + n] - gd * (tot2[jt][r] / R2)) + gd * (tot1[jt][r] / R1);
            gc[f * D + n] = ok ? v : 0.0f;
        }
    }
}

__global__ __launch_bounds__(256) void k_merlin_r0_bwd(const float* __restrict__ c1, const float* __restrict__ c2,
                                                       const float* __restrict__ gpf, const float* __restrict__ lifter,
                                                       long long F, int D, const float* __restrict__ G,
                                                       const float* __restrict__ wk, int nb, float* __restrict__ gc) {
    __shared__ __attribute__((aligned(16))) float gs[64][kMerlinStride];   // [n][bin of the chunk]
    __shared__ __attribute__((aligned(16))) float e1[64][kMerlinStride];   // [frame][bin of the chunk]
    __shared__ __attribute__((aligned(16))) float e2[64][kMerlinStride];
    __shared__ float a1[64][65], a2[64][65];
    __shared__ float part[2][4][64];
    const int nt = (D + 15) >> 4;   // wave-uniform (a kernel argument)
    if (nt == 1) merlin_r0_bwd_block<1>(c1, c2, gpf, lifter, F, D, G, wk, nb, gc, gs, e1, e2, a1, a2, part);
    else if (nt == 2) merlin_r0_bwd_block<2>(c1, c2, gpf, lifter, F, D, G, wk, nb, gc, gs, e1, e2, a1, a2, part);
    else if (nt == 3) merlin_r0_bwd_block<3>(c1, c2, gpf, lifter, F, D, G, wk, nb, gc, gs, e1, e2, a1, a2, part);
    else merlin_r0_bwd_block<4>(c1, c2, gpf, lifter, F, D, G, wk, nb, gc, gs, e1, e2, a1, a2, part);
}

}  // namespace mpx

using namespace mpx;

extern "C" int mpx_post_filter_merlin_backward(void* stream, const float* mag_mel_log, const float* grad_out,
                                               int64_t n_frames, int32_t dim, const float* c1, const float* lifter,
                                               const float* g, const float* wk, int32_t n_bins, const float* cf_t,
                                               const float* c1_t, float* mcep, float* mcep_w, float* grad_pf,
                                               float* grad_mcep, float* grad_in) {
    if (n_frames < 0 || dim < 3 || dim > 64 || n_bins < 1)
        return fail(MPX_ERR_ARG, "mpx_post_filter_merlin_backward: need 3 <= dim <= 64, n_frames >= 0, n_bins >= 1%s");
    if (n_frames == 0) return MPX_OK;
    if (!mag_mel_log || !grad_out || !c1 || !lifter || !g || !wk || !cf_t || !c1_t || !mcep || !mcep_w || !grad_pf ||
        !grad_mcep || !grad_in)
        return fail(MPX_ERR_ARG, "mpx_post_filter_merlin_backward: null pointer%s");
    hipStream_t s = (hipStream_t)stream;
    const long long F = n_frames;
    const unsigned gb = (unsigned)std::min<long long>((F + 3) / 4, 4096);
    // the forward's first launch again: mcep and mcep_w as the forward had them (it overwrote its mcep buffer)
    hipLaunchKernelGGL(k_rows_gemm, dim3(gb), dim3(256), 0, s, mag_mel_log, F, (int)dim, (int)dim, c1, lifter, mcep, mcep_w,
                       0.0f, 0);
    hipLaunchKernelGGL(k_rows_gemm, dim3(gb), dim3(256), 0, s, grad_out, F, (int)dim, (int)dim, cf_t, (const float*)nullptr,
                       grad_pf, (float*)nullptr, 0.0f, 0);
    hipLaunchKernelGGL(k_merlin_r0_bwd, dim3((unsigned)((F + 63) / 64)), dim3(256), 0, s, (const float*)mcep,
                       (const float*)mcep_w, (const float*)grad_pf, lifter, F, (int)dim, g, wk, (int)n_bins, grad_mcep);
    hipLaunchKernelGGL(k_rows_gemm, dim3(gb), dim3(256), 0, s, (const float*)grad_mcep, F, (int)dim, (int)dim, c1_t,
                       (const float*)nullptr, grad_in, (float*)nullptr, 0.0f, 0);
    MPX_HIP_CHECK(hipGetLastError());
    return MPX_OK;
}

extern "C" int mpx_post_filter_merlin(void* stream, const float* mag_mel_log, int64_t n_frames, int32_t dim,
                                      const float* c1, const float* lifter, const float* g, const float* wk,
                                      int32_t n_bins, double alpha, const float* cf, double magic, float* mcep,
                                      float* mcep_w, float* r0, float* p_r0, float* out) {
    if (n_frames < 0 || dim < 3 || dim > 64 || n_bins < 1)
        return fail(MPX_ERR_ARG, "mpx_post_filter_merlin: need 3 <= dim <= 64, n_frames >= 0, n_bins >= 1%s");
    if (n_frames == 0) return MPX_OK;
    if (!mag_mel_log || !c1 || !lifter || !g || !wk || !cf || !mcep || !mcep_w || !r0 || !p_r0 || !out)
        return fail(MPX_ERR_ARG, "mpx_post_filter_merlin: null pointer%s");
    hipStream_t s = (hipStream_t)stream;
    const long long F = n_frames;
    const unsigned gb = (unsigned)std::min<long long>((F + 3) / 4, 4096);
    hipLaunchKernelGGL(k_rows_gemm, dim3(gb), dim3(256), 0, s, mag_mel_log, F, (int)dim, (int)dim, c1, lifter, mcep, mcep_w,
                       0.0f, 0);
    hipLaunchKernelGGL(k_merlin_r0, dim3((unsigned)((F + 63) / 64)), dim3(256), 0, s, (const float*)mcep,
                       (const float*)mcep_w, F, (int)dim, g, wk, (int)n_bins, r0, p_r0);
    // mcep is free now: it receives the post-filtered mel cepstrum
    hipLaunchKernelGGL(k_merlin_b, dim3((unsigned)((F + 255) / 256)), dim3(256), 0, s, (const float*)mcep_w, F, (int)dim,
                       (float)alpha, (const float*)r0, (const float*)p_r0, mcep);
    hipLaunchKernelGGL(k_rows_gemm, dim3(gb), dim3(256), 0, s, (const float*)mcep, F, (int)dim, (int)dim, cf,
                       (const float*)nullptr, out, (float*)nullptr, (float)magic, 1);
    MPX_HIP_CHECK(hipGetLastError());
    return MPX_OK;
}
