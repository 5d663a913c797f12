// magphase_grad.hip -- backward pass of the lossless synthesis.
//
//   k_synth_lossless_bwd<P, L>  one wavefront per frame, persistent waves (grid-stride over frames), the shape of
//                               k_analysis: the N samples of the incoming waveform gradient around the frame's pitch mark
//                               -> LDS (two tiles of N/2) -> rotated by N/2 into FFT order -> 64*P-point complex FFT ->
//                               real-FFT split -> pointwise epilogue against the frame's feature rows -> 3 x H coalesced
//                               stores.  L = LERP: the feature row is the interpolation of two constant-rate rows, formed as
//                               the forward's k_synth_ola_pair<P, true> forms it (fma(x1 - x0, t, x0)); the stores then
//                               go to variable-rate scratch rows that k_rows_lerp_adjoint folds back.
//   k_rows_lerp_adjoint         one wavefront per constant-rate row: the weighted sum of the variable-rate gradient rows
//                               that read it, in ascending frame order (two contiguous frame ranges per row, built on the
//                               host: hostmath.lerp_adjoint_table).  No atomics: one writer per output element.
//
// The forward is y = overlap-add of fftshift(irfft(X)), X = mag (R + jI) / |R + jI| (divisor 1 where |R + jI| == 0, the
// imaginary parts of bins 0 and N/2 dropped).  irfft and the overlap-add are linear, so the gradient with respect to X is
// their transpose: gX_k = (c_k / N) FFT_N(ifftshift(g))_k with g the gradient samples under the frame, c_k = 2 for
// 0 < k < N/2 and 1 at the two ends (a bin and its mirror both carry X_k), Im gX_0 = Im gX_{N/2} = 0.  No overlap-add,
// no run seams: every frame GATHERS, and writes rows nobody else writes.
#include "mpx_common.hpp"

namespace mpx {

// The frame's window into the gradient buffer: sample n (0 <= n < N) is base[n], to be read for lo <= n < hi only --
// the part of the frame that lies inside its own utterance's output AND inside the buffer.  Everything else is zero (the
// forward dropped those samples of the frame).
struct GradGeom {
    const float* base;
    int lo, hi;
};

__device__ __forceinline__ GradGeom grad_geom(const float* __restrict__ gy, long long total, long long pos, int lo, int hi,
                                              int N) {
    GradGeom g;
    // whatever the tables say, no address outside [gy, gy + total) is formed for a read
    const long long lo_b = (pos < 0) ? -pos : 0, hi_b = total - pos;
    g.lo = (int)max((long long)max(lo, 0), min(lo_b, (long long)N));
    g.hi = (int)min((long long)min(hi, N), max(hi_b, 0ll));
    g.hi = max(g.hi, g.lo);
    g.base = gy + pos;
    return g;
}

// Asynchronous HBM -> LDS copy of the gradient samples [tile0, tile0 + 64 P) in sample order, as stage_samples_async
// copies signal samples (mpx_common.hpp: one global_load_lds_dword per 64 samples, waited for with staged_wait).  Reads are
// clamped into [lo, hi); 64-sample rows wholly outside it are not copied (their LDS words keep old contents: the
// gather masks by sample index, it never multiplies).
template <int P>
__device__ __forceinline__ void stage_grad_async(const GradGeom& g, int tile0, unsigned lds_byte, int lane) {
    for (int c = 0; c < P; ++c) {
        const int n0 = tile0 + 64 * c;
        if (n0 + 64 <= g.lo || n0 >= g.hi) continue;   // wave-uniform
        const float* src = g.base + min(max(n0 + lane, g.lo), g.hi - 1);
        const unsigned m0v = __builtin_amdgcn_readfirstlane(lds_byte + 256u * (unsigned)c);
        asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dword %0, off" ::"v"(src), "s"(m0v) : "m0", "memory");
    }
}

// One bin of the epilogue.  (m, a, b) the bin's features, (gr, gi) = gX.  u = (a, b) / den, d = Re(conj(u) gX):
//   dL/dmag = d,  dL/d(a, b) = (mag / den) (gX - u d);   den == 0 counts as 1: u = 0, d = 0, dL/d(a, b) = mag gX.
// rsq(max(s, tiny)) is the forward's own divisor (feat_convert): finite, and it multiplies a == b == 0 when s == 0.
__device__ __forceinline__ void bwd_bin(float m, float a, float b, float gr, float gi, float& om, float& orr, float& oi) {
    const float s = a * a + b * b;
    const float r = __builtin_amdgcn_rsqf(fmaxf(s, 1.0e-37f));
    const float ur = a * r, ui = b * r;
    const float d = ur * gr + ui * gi;
    const float mr = (s > 0.0f) ? m * r : m;
    om = d;
    orr = mr * (gr - ur * d);
    oi = mr * (gi - ui * d);
}

// The feature rows of one frame: three base pointers, or with LERP two rows each and the interpolation weight.
template <bool LERP>
struct BwdRows {
    const float *m0, *r0, *i0, *m1, *r1, *i1;
    float t;
    __device__ __forceinline__ void load(int k, float& m, float& a, float& b) const {
        if constexpr (LERP) {   // the forward's arithmetic (feat_lerp_paired_part): (1 - t) x0 + t x1 = fma(x1 - x0, t, x0)
            const float xm0 = m0[k], xa0 = r0[k], xb0 = i0[k];
            const float xm1 = m1[k], xa1 = r1[k], xb1 = i1[k];
            m = fmaf(xm1 - xm0, t, xm0);
            a = fmaf(xa1 - xa0, t, xa0);
            b = fmaf(xb1 - xb0, t, xb0);
        } else {
            m = m0[k];
            a = r0[k];
            b = i0[k];
        }
    }
};

template <int P, bool LERP>
__global__ __launch_bounds__(kAnaThreads) void k_synth_lossless_bwd(
    const float* __restrict__ gy, long long total_out, const long long* __restrict__ gpos, const int* __restrict__ glo,
    const int* __restrict__ ghi, long long nframes, const float* __restrict__ tw_g, const float* __restrict__ mag,
    const float* __restrict__ real, const float* __restrict__ imag, long long ld, const int* __restrict__ row0,
    const int* __restrict__ row1, const float* __restrict__ rowt, float* __restrict__ omag, float* __restrict__ oreal,
    float* __restrict__ oimag, long long ldg) {
    constexpr int M = 64 * P, N = 2 * M, LB = ilog2(P), HP = P / 2;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* tw = smem;
    const int lane_id = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    float* xbuf = smem + tw_floats<P>() + wave * (P * kXStride);
    // byte address of xbuf in LDS (the dynamic segment starts at 0: the kernel has no static __shared__)
    const unsigned xbuf_byte = 4u * (unsigned)(tw_floats<P>() + rfl(wave) * (P * kXStride));
    for (int i = threadIdx.x; i < tw_floats<P>(); i += kAnaThreads) tw[i] = tw_g[i];
    __syncthreads();

    // lane part of the split twiddle W_N^kappa = e^{-2 pi i kappa / N}
    float wl_s0, wl_c0;
    sincospif(-2.0f * (float)kappa<P>(lane_id) / (float)N, &wl_s0, &wl_c0);

    const long long fstep = (long long)gridDim.x * kAnaWaves;
    long long f = (long long)blockIdx.x * kAnaWaves + rfl(wave);
    if (f >= nframes) return;

    // Software pipeline as in k_analysis: the first tile of the wave's next frame is copied HBM -> LDS (into the transpose
    // buffer, idle after the FFT's exchange) while this frame's second FFT pass and epilogue run.  The buffer holds half a
    // frame, and a gradient window is always the whole frame: the second tile is copied once the first has been gathered.
    GradGeom g = grad_geom(gy, total_out, gpos[f], glo[f], ghi[f], N);
    stage_grad_async<P>(g, 0, xbuf_byte, lane_id);
    staged_wait<0>();

    while (true) {
        // Launder the per-lane invariants once per frame (see k_analysis: LICM would hoist every lane x register product)
        int lane = lane_id;
        float wl_s = wl_s0, wl_c = wl_c0;
        asm volatile("" : "+v"(lane), "+v"(wl_s), "+v"(wl_c));
        const int kap = kappa<P>(lane);
        const int src_lane = kappa<P>((64 - kap) & 63);
        const bool lane0 = (kap == 0);

        // ---- gather in FFT order with the fixed rotation N/2 (ifftshift): buffer index m = 128 j + 2 lane (+ 1) holds
        // sample k = (m + N/2) mod N.  Samples [0, N/2) (tile 0) are the registers j >= P/2, samples [N/2, N) (tile 1) the
        // registers j < P/2; within its tile a register pair is one aligned 8-byte LDS read.
        float re[P], im[P];
#pragma unroll
        for (int j = HP; j < P; ++j) {
            const int k0 = 128 * (j - HP) + 2 * lane;
            const float2 v = *reinterpret_cast<const float2*>(xbuf + k0);
            re[j] = (k0 >= g.lo && k0 < g.hi) ? v.x : 0.0f;
            im[j] = (k0 + 1 >= g.lo && k0 + 1 < g.hi) ? v.y : 0.0f;
        }
        wave_sync();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // tile 0 has been read before the copy overwrites it
        stage_grad_async<P>(g, M, xbuf_byte, lane);
        staged_wait<0>();
#pragma unroll
        for (int j = 0; j < HP; ++j) {
            const int k0 = 128 * j + 2 * lane;
            const float2 v = *reinterpret_cast<const float2*>(xbuf + k0);
            re[j] = (M + k0 >= g.lo && M + k0 < g.hi) ? v.x : 0.0f;
            im[j] = (M + k0 + 1 >= g.lo && M + k0 + 1 < g.hi) ? v.y : 0.0f;
        }
        wave_sync();

        wave_fft_front<P, -1>(re, im, tw, xbuf, lane);

        // ---- the exchange buffer is idle from here on: start the copy of the next frame's first tile into it
        const long long fn = f + fstep;
        GradGeom gn = g;
        if (fn < nframes) {
            gn = grad_geom(gy, total_out, gpos[fn], glo[fn], ghi[fn], N);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the exchange's own LDS reads have returned
            stage_grad_async<P>(gn, 0, xbuf_byte, lane);
        }

        fft_inreg<P, -1>(re, im);

        // ---- real-FFT split as in k_analysis (one (k, M-k) bin pair per step q; lane kappa owns k = kappa + 64 q), then
        // per bin: gX = (c_k / N) G_k, the three gradients from the bin's features.  Loads and stores share k_analysis'
        // lane <-> bin layout: the ascending stream at kappa + 64 q, the mirrors regrouped into blocks that start a multiple
        // of 64 floats from the row start (block S_{q-1} stored during step q with lane 0's own output of step q).
        BwdRows<LERP> fr;
        if constexpr (LERP) {
            const long long a = row0[f], b = row1[f];
            fr.m0 = mag + a * ld, fr.r0 = real + a * ld, fr.i0 = imag + a * ld;
            fr.m1 = mag + b * ld, fr.r1 = real + b * ld, fr.i1 = imag + b * ld;
            fr.t = rowt[f];
        } else {
            fr.m0 = fr.m1 = mag + f * ld, fr.r0 = fr.r1 = real + f * ld, fr.i0 = fr.i1 = imag + f * ld;
            fr.t = 0.0f;
        }
        float* row_m = omag + f * ldg;     // a stream that needs no gradient is a null pointer: never dereferenced
        float* row_r = oreal + f * ldg;
        float* row_i = oimag + f * ldg;
        const int hoff = lane0 ? M - 64 : M - kap;   // X[M-k] blocks: descending lanes, -64 q (lane 0: one block lower)
        constexpr float kS2 = 2.0f / (float)N, kS1 = 1.0f / (float)N;
        float zpr[HP], zpi[HP];   // all partner bins first: P lane exchanges in flight together
#pragma unroll
        for (int q = 0; q < HP; ++q) {
            const int i = brev(q, LB);
            zpr[q] = __shfl(re[P - 1 - i], src_lane);
            zpi[q] = __shfl(im[P - 1 - i], src_lane);
        }
        float hm = 0.0f, hr = 0.0f, hi_ = 0.0f;   // mirror outputs of the previous step
#pragma unroll
        for (int q = 0; q < HP; ++q) {
            const int i = brev(q, LB);            // even register
            const int i0 = brev((P - q) % P, LB);
            const float pr = lane0 ? re[i0] : zpr[q];
            const float pi = lane0 ? im[i0] : zpi[q];
            const float er = 0.5f * (re[i] + pr), ei = 0.5f * (im[i] - pi);
            const float orr = 0.5f * (im[i] + pi), oi = -0.5f * (re[i] - pr);
            const float cq = cos2p<P>(q), sq = -sin2p<P>(q);   // W_N^k = W_N^kappa * e^{-2 pi i q/(2P)}
            const float wr = wl_c * cq - wl_s * sq, wi = wl_c * sq + wl_s * cq;
            const float tr = wr * orr - wi * oi, ti = wr * oi + wi * orr;
            // bins 0 and M (lane 0 of step 0): c_k = 1 and the imaginary part dropped
            const bool edge = (q == 0) && lane0;
            const float sc = edge ? kS1 : kS2, sci = edge ? 0.0f : kS2;
            float fm, fa, fb, fmq, faq, fbq;
            fr.load(kap + 64 * q, fm, fa, fb);          // bin k
            fr.load(M - kap - 64 * q, fmq, faq, fbq);   // bin M - k (lane 0 of step 0: bin M)
            {
                float cm, cr, ci;
                bwd_bin(fm, fa, fb, (er + tr) * sc, (ei + ti) * sci, cm, cr, ci);
                if (omag) row_m[kap + 64 * q] = cm;
                if (oreal) row_r[kap + 64 * q] = cr;
                if (oimag) row_i[kap + 64 * q] = ci;
            }
            {
                float cm, cr, ci;
                bwd_bin(fmq, faq, fbq, (er - tr) * sc, (ti - ei) * sci, cm, cr, ci);
                if (q == 0) {
                    if (lane0) {                      // bin M
                        if (omag) row_m[M] = cm;
                        if (oreal) row_r[M] = cr;
                        if (oimag) row_i[M] = ci;
                    }
                } else {                              // block S_{q-1}
                    if (omag) row_m[hoff - 64 * (q - 1)] = lane0 ? cm : hm;
                    if (oreal) row_r[hoff - 64 * (q - 1)] = lane0 ? cr : hr;
                    if (oimag) row_i[hoff - 64 * (q - 1)] = lane0 ? ci : hi_;
                }
                hm = cm;
                hr = cr;
                hi_ = ci;
            }
        }
        {   // block S_{P/2-1} = [M/2, M/2+63]: lane 0 supplies bin M/2 (register 1 holds q = P/2): G = conj Z.  Every lane
            // loads "its" bin M/2 + lane (in range; a lane-0-only load would be a scalar load and an immediate wait)
            float fm, fa, fb, cm, cr, ci;
            fr.load(M / 2 + lane, fm, fa, fb);
            bwd_bin(fm, fa, fb, re[1] * kS2, -im[1] * kS2, cm, cr, ci);
            if (omag) row_m[hoff - 64 * (HP - 1)] = lane0 ? cm : hm;
            if (oreal) row_r[hoff - 64 * (HP - 1)] = lane0 ? cr : hr;
            if (oimag) row_i[hoff - 64 * (HP - 1)] = lane0 ? ci : hi_;
        }
        g = gn;
        if (fn >= nframes) break;
        // At least one stream is stored (the host refuses a launch without one): P + 1 or more stores were issued after the
        // copy's loads, so "at most P + 1 operations outstanding" implies the copy has landed (one in-order counter).
        staged_wait<P + 1>();
        f = fn;
    }
}

// ---------------------------------------------------------------------------------------------
// Adjoint of the constant -> variable rate row interpolation row_f = fma(rows[row1_f] - rows[row0_f], t_f, rows[row0_f]):
//   d rows[r] = sum_{f: row0_f = r} (1 - t_f) gv_f + sum_{f: row1_f = r} t_f gv_f
// rng[4 r .. 4 r + 3] = (a0, a1, b0, b1): the frames with row0 == r are [a0, a1), those with row1 == r are [b0, b1) (both
// tables are non-decreasing within an utterance, and rows are global).  One wavefront per row r walks the union of the two
// ranges in ascending frame order; a frame in both (row0 == row1: the forward returns the row itself) weighs exactly 1.
// A row no frame reads gets zeros.  Four columns per lane in flight; a null stream is skipped.
// ---------------------------------------------------------------------------------------------
constexpr int kAdjWaves = 4;

__global__ __launch_bounds__(kAdjWaves * 64) void k_rows_lerp_adjoint(int H, const float* __restrict__ sm,
                                                                      const float* __restrict__ sr,
                                                                      const float* __restrict__ si, long long lds,
                                                                      const int* __restrict__ rng,
                                                                      const float* __restrict__ rowt, long long n_rows,
                                                                      float* __restrict__ dm, float* __restrict__ dr,
                                                                      float* __restrict__ di, long long ldd) {
    const long long r = (long long)blockIdx.x * kAdjWaves + rfl((int)(threadIdx.x >> 6));
    if (r >= n_rows) return;
    const int lane = threadIdx.x & 63;
    const int a0 = rng[4 * r + 0], a1 = rng[4 * r + 1], b0 = rng[4 * r + 2], b1 = rng[4 * r + 3];
    const bool has_a = a1 > a0, has_b = b1 > b0;
    const int f_lo = has_a ? (has_b ? min(a0, b0) : a0) : b0;
    const int f_hi = has_a ? (has_b ? max(a1, b1) : a1) : (has_b ? b1 : b0);
    const float* src[3] = {sm, sr, si};
    float* dst[3] = {dm, dr, di};
    for (int c0 = lane; c0 < H; c0 += 256) {
        float acc[3][4];
#pragma unroll
        for (int s = 0; s < 3; ++s)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[s][e] = 0.0f;
        for (int f = f_lo; f < f_hi; ++f) {
            const bool in_a = (f >= a0 && f < a1), in_b = (f >= b0 && f < b1);
            if (!in_a && !in_b) continue;   // wave-uniform
            const float t = rowt[f];
            const float w = (in_a && in_b) ? 1.0f : (in_a ? 1.0f - t : t);
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                if (!dst[s]) continue;
                const float* row = src[s] + (long long)f * lds;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int c = c0 + 64 * e;
                    if (c < H) acc[s][e] = fmaf(w, row[c], acc[s][e]);
                }
            }
        }
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            if (!dst[s]) continue;
            float* row = dst[s] + r * ldd;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int c = c0 + 64 * e;
                if (c < H) row[c] = acc[s][e];
            }
        }
    }
}

}  // namespace mpx

using namespace mpx;

extern "C" {

int mpx_synthesis_lossless_backward(void* stream, int fft_len, const void* tables, const float* grad_out,
                                    int64_t total_out, const int64_t* grad_pos, const int32_t* grad_lo,
                                    const int32_t* grad_hi, int64_t n_frames, const float* mag, const float* real,
                                    const float* imag, int64_t ld, const int32_t* row0, const int32_t* row1,
                                    const float* row_t, float* grad_mag, float* grad_real, float* grad_imag,
                                    int64_t ld_grad) {
    const int P = p_of(fft_len);
    if (!P) return fail(MPX_ERR_ARG, "mpx_synthesis_lossless_backward: fft_len must be 1024, 2048 or 4096%s");
    if (n_frames < 0 || total_out < 0) return fail(MPX_ERR_ARG, "mpx_synthesis_lossless_backward: negative count%s");
    if (ld < fft_len / 2 + 1 || ld_grad < fft_len / 2 + 1)
        return fail(MPX_ERR_ARG, "mpx_synthesis_lossless_backward: ld < fft_len/2 + 1%s");
    const bool lerp = row0 || row1 || row_t;
    if (lerp && !(row0 && row1 && row_t))
        return fail(MPX_ERR_ARG, "mpx_synthesis_lossless_backward: row0, row1 and row_t come together or not at all%s");
    if (n_frames == 0) return MPX_OK;
    if (!grad_mag && !grad_real && !grad_imag) return MPX_OK;   // nothing asked for
    if (!tables || !grad_pos || !grad_lo || !grad_hi || !mag || !real || !imag || (total_out > 0 && !grad_out))
        return fail(MPX_ERR_ARG, "mpx_synthesis_lossless_backward: null pointer%s");
    const dim3 grid(grid_for(n_frames, kAnaWaves)), block(kAnaThreads);
    hipStream_t s = (hipStream_t)stream;
#define MPX_LAUNCH_BWD(PP, LL)                                                                                        \
    do {                                                                                                              \
        if (int rc = set_lds((k_synth_lossless_bwd<PP, LL>), lds_bytes_ana<PP>())) return rc;                         \
        hipLaunchKernelGGL((k_synth_lossless_bwd<PP, LL>), grid, block, lds_bytes_ana<PP>(), s, grad_out,             \
                           (long long)total_out, (const long long*)grad_pos, grad_lo, grad_hi, (long long)n_frames,  \
                           (const float*)tables, mag, real, imag, (long long)ld, row0, row1, row_t, grad_mag,        \
                           grad_real, grad_imag, (long long)ld_grad);                                                \
    } while (0)
    if (lerp) {
        if (P == 32) MPX_LAUNCH_BWD(32, true);
        else if (P == 16) MPX_LAUNCH_BWD(16, true);
        else MPX_LAUNCH_BWD(8, true);
    } else {
        if (P == 32) MPX_LAUNCH_BWD(32, false);
        else if (P == 16) MPX_LAUNCH_BWD(16, false);
        else MPX_LAUNCH_BWD(8, false);
    }
#undef MPX_LAUNCH_BWD
    MPX_HIP_CHECK(hipGetLastError());
    return MPX_OK;
}

int mpx_rows_lerp_adjoint(void* stream, int32_t n_bins, const float* src_mag, const float* src_real,
                          const float* src_imag, int64_t ld_src, const int32_t* ranges, const float* row_t,
                          int64_t n_rows, float* dst_mag, float* dst_real, float* dst_imag, int64_t ld_dst) {
    if (n_bins < 1 || n_rows < 0) return fail(MPX_ERR_ARG, "mpx_rows_lerp_adjoint: n_bins < 1 or negative n_rows%s");
    if (ld_src < n_bins || ld_dst < n_bins) return fail(MPX_ERR_ARG, "mpx_rows_lerp_adjoint: row pitch < n_bins%s");
    if (n_rows == 0) return MPX_OK;
    if (!dst_mag && !dst_real && !dst_imag) return MPX_OK;   // nothing asked for
    if (!ranges || !row_t || (dst_mag && !src_mag) || (dst_real && !src_real) || (dst_imag && !src_imag))
        return fail(MPX_ERR_ARG, "mpx_rows_lerp_adjoint: null pointer%s");
    if ((n_rows + kAdjWaves - 1) / kAdjWaves > 2147483647LL)
        return fail(MPX_ERR_ARG, "mpx_rows_lerp_adjoint: too many rows%s");
    const dim3 block(kAdjWaves * 64), grid((unsigned)((n_rows + kAdjWaves - 1) / kAdjWaves));
    hipLaunchKernelGGL(k_rows_lerp_adjoint, grid, block, 0, (hipStream_t)stream, (int)n_bins, src_mag, src_real, src_imag,
                       (long long)ld_src, ranges, row_t, (long long)n_rows, dst_mag, dst_real, dst_imag,
                       (long long)ld_dst);
    MPX_HIP_CHECK(hipGetLastError());
    return MPX_OK;
}

}  // extern "C"
