// magphase_grad.hip -- backward passes of the lossless synthesis (first part of this file) and of
// the lossless analysis (section 3.3i: k_analysis_lossless_bwd<P, CR>, k_analysis_bwd_gather, further down; CR: the
// gradients come on the constant-rate rows of the constant-rate analysis and are gathered per frame in registers).
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
    if (g.hi <= g.lo) return;   // nothing kept of the frame: no address is formed at all
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

// ---------------------------------------------------------------------------------------------
// Backward pass of the lossless analysis.
//
// The forward (k_analysis) is X = rfft_N(buf), buf = the windowed frame rotated by rot, and (mag, real, imag) =
// (|X|, X / |X|) (all 0 where X == 0).  Given (gm, gr, gi) = dL/d(mag, real, imag) and the forward's own outputs:
//   d = real gr + imag gi,   gX = gm (real + j imag) + ((gr + j gi) - (real + j imag) d) / mag     (0 where mag^2 < 1e-37)
//   b = N irfft_N(Y), Y_k = gX_k / 2 for 0 < k < N/2, Y_0 = Re gX_0, Y_{N/2} = Re gX_{N/2}   (the transpose of rfft_N)
//   gfrm[k] = b[(k - rot) mod N] w(k) for 0 <= k < len,   gsig[pos - L + k] += gfrm[k]
//
//   k_analysis_lossless_bwd<P, CR>  (CR = false here; the CR arm is described at the kernel)
//                               one wavefront per frame, persistent waves (grid-stride), the shape of k_synth_lossless:
//                               the six rows of a frame in the paired layout of feat_load_paired (ascending bins
//                               lane + 64 j and their mirrors M - k: every load one contiguous 256-byte block) -> gX ->
//                               merge_pair_step / merge_handover -> wave_fft<P, +1> -> rotation, hann_half -> the frame's
//                               len samples into a COMPACT scratch (scratch_off[f]: prefix sums built on the host).
//   k_analysis_bwd_gather       one thread per signal sample: the sum over the frames that cover it, in ascending frame
//                               order (a contiguous frame range: hostmath.analysis_backward_table).  One writer per
//                               element, no atomics; a sample no frame covers gets 0.
// ---------------------------------------------------------------------------------------------
// One bin of the pointwise step: (m, a, b) the forward's mag / real / imag, (gm, gr, gi) their gradients -> sc gX.
// mag^2 < 1e-37 is the forward's clamp region (rsq(max(|X|^2, 1e-37)): X == 0 lies in it, and the outputs there are not
// (|X|, X / |X|)): the gradient is defined as 0 there -- silent frames give zeros, never Inf or NaN.
__device__ __forceinline__ void ana_bwd_bin(float m, float a, float b, float gm, float gr, float gi, float sc, float& x_r,
                                            float& x_i) {
    const bool live = m * m >= 1.0e-37f;
    const float inv = live ? sc * __builtin_amdgcn_rcpf(m) : 0.0f;
    const float gs = live ? sc * gm : 0.0f;
    const float d = a * gr + b * gi;
    x_r = gs * a + (gr - a * d) * inv;
    x_i = gs * b + (gi - b * d) * inv;
}

// merge_pair_step (mpx_common.hpp) in two parts, for the CR arm of k_analysis_lossless_bwd: the step's twiddle
// conj(W_N^k) = (wl_c + j wl_s) e^{2 pi i q / 2P}, and the step given it.  merge_pair_step writes the twiddle as
// wr = wl_c cq - wl_s sq, wi = wl_c sq + wl_s cq and leaves it to the compiler which product of each sum is folded into
// the fused multiply-add and which is rounded on its own.  The four products of step q are shared with step P/2 - q
// (cos and sin change places), so that choice depends on the order in which the instruction selector meets the steps --
// it is made per basic block, and the CR = false arm and this one do not have the same blocks: built from the same
// expressions, the two arms' twiddles differed in the last bit at P = 16 / 32, and the fused backward pass with them
// from the staged one.  So the CR arm spells out what the CR = false instantiations do (read from their gfx950 code with
// a symbolic trace of the twiddle registers, and held bit for bit by tests/test_gpu_const_rate_analysis_autograd.py): of
// the two products of a sum one is fused and the other rounded first -- at P = 16 / 32 the one with the larger constant
// is fused, at P = 8 the one with the smaller constant; at cq == sq the product of wl_s is fused.
template <int P>
__device__ __forceinline__ void merge_twiddle(int q, float wl_c, float wl_s, float& wr, float& wi) {
#pragma clang fp contract(off)
    const float cq = cos2p<P>(q), sq = sin2p<P>(q);
    // fuse_c: the products with cq are the fused ones (wl_c cq in wr, wl_s cq in wi); else those with sq
    const bool tie = (cq == sq), fuse_c = (P == 8) ? (cq < sq) : (cq > sq);
    wr = fuse_c ? __builtin_fmaf(wl_c, cq, -(wl_s * sq)) : __builtin_fmaf(-wl_s, sq, wl_c * cq);
    wi = (fuse_c || tie) ? __builtin_fmaf(wl_s, cq, wl_c * sq) : __builtin_fmaf(wl_c, sq, wl_s * cq);
}
__device__ __forceinline__ void merge_pair_step_w(float x_r, float x_i, float p_r, float p_i, float wr, float wi,
                                                  float& out_r, float& out_i, float& z_r, float& z_i) {
    const float er = x_r + p_r, ei = x_i - p_i, tr = x_r - p_r, ti = x_i + p_i;
    const float orr = wr * tr - wi * ti, oi = wr * ti + wi * tr;
    out_r = er - oi;
    out_i = ei + orr;
    z_r = er + oi;
    z_i = orr - ei;
}

// Waves per workgroup: k_analysis' 12 (three per SIMD, <= 168 VGPRs) for P = 8 / 16; P = 32 holds 64 spectrum registers
// beside the row loads and needs more than 168 (it spilled 51 at any load group size): 8 waves, two per SIMD, as
// k_synth_lossless.
template <int P>
constexpr int ana_bwd_waves() { return P == 32 ? kWavesPerBlock : kAnaWaves; }
template <int P>
constexpr size_t lds_bytes_ana_bwd() { return sizeof(float) * (size_t)(tw_floats<P>() + ana_bwd_waves<P>() * P * kXStride); }

//
// CR = true (the constant-rate analysis, mpx_analysis_lossless_const_rate_backward): gmag / greal / gimag are the gradients
// of the CONSTANT-rate rows out[c] = fma(rows[row1_c] - rows[row0_c], t_c, rows[row0_c]), [n_crows x H] at pitch ldg, and
// the wave forms frame f's own gradient row in registers while it loads a group of bin pairs: rng[4 f .. 4 f + 3] =
// (a0, a1, b0, b1) (hostmath.lerp_adjoint_table over the variable frames: the constant-rate rows with row0 == f are
// [a0, a1), those with row1 == f are [b0, b1), clamped to [0, n_crows) whatever the table holds), c ascending over their
// union, w = 1 in both, 1 - t_c in the first only, t_c in the second only, acc = fmaf(w, g[c][k], acc) from 0 -- per
// element k_rows_lerp_adjoint's operation sequence, so the result equals the staged form (that kernel, then CR = false)
// bit for bit, and nothing [nframes x H]-sized is written or read for the gradients.  A frame no row reads has a zero
// gradient row and still writes its zeros to the scratch.  The accumulators are the load group's own g / gq registers;
// the gather runs BEFORE the group's six forward loads, so that a row's 6 CH loads in flight stand where those would.
template <int P, bool CR = false>
__global__ __launch_bounds__(64 * ana_bwd_waves<P>()) void k_analysis_lossless_bwd(
    const float* __restrict__ mag, const float* __restrict__ real, const float* __restrict__ imag, long long ld,
    const float* __restrict__ gmag, const float* __restrict__ greal, const float* __restrict__ gimag, long long ldg,
    const int* __restrict__ fleft, const int* __restrict__ fright, const long long* __restrict__ soff, long long nframes,
    const float* __restrict__ tw_g, float* __restrict__ scratch, long long scratch_floats, const int* __restrict__ rng,
    const float* __restrict__ rowt, int n_crows) {
    constexpr int M = 64 * P, N = 2 * M, LB = ilog2(P), HP = P / 2;
    constexpr int CH = 4;   // bin pairs per load group: 12 CH row values in flight beside the 2 P of the growing spectrum
    constexpr int kWaves = ana_bwd_waves<P>(), kThr = 64 * kWaves;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* tw = smem;
    const int lane_id = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    float* xbuf = smem + tw_floats<P>() + wave * (P * kXStride);
    for (int i = threadIdx.x; i < tw_floats<P>(); i += kThr) tw[i] = tw_g[i];
    __syncthreads();

    // input layout is natural (k = lane + 64 j): lane twiddle conj(W_N^lane) = e^{+2 pi i lane/N}, as k_synth_lossless
    float wl_s0, wl_c0;
    sincospif(2.0f * (float)lane_id / (float)N, &wl_s0, &wl_c0);

    const long long fstep = (long long)gridDim.x * kWaves;
    for (long long f = (long long)blockIdx.x * kWaves + rfl(wave); f < nframes; f += fstep) {
        int lane = lane_id;  // laundered per frame (see k_analysis)
        float wl_s = wl_s0, wl_c = wl_c0;
        asm volatile("" : "+v"(lane), "+v"(wl_s), "+v"(wl_c));
        const int kap = kappa<P>(lane);
        const bool lane0 = (lane == 0);

        // ---- the six rows in the paired layout, CH bin pairs at a time; a null gradient stream is never loaded
        const float* row[3] = {mag + f * ld, real + f * ld, imag + f * ld};
        const float* grow[3] = {gmag ? gmag + f * ldg : nullptr, greal ? greal + f * ldg : nullptr,
                                gimag ? gimag + f * ldg : nullptr};
        // CR: the constant-rate streams from their row 0, frame f's two row ranges (wave-uniform) and the gathered
        // gradient of bin M/2 + lane (formed with the last group)
        const float* gsrc[3] = {gmag, greal, gimag};
        int a0 = 0, a1 = 0, b0 = 0, b1 = 0, c_lo = 0, c_hi = 0;
        float gh[3] = {0.0f, 0.0f, 0.0f};
        if constexpr (CR) {
            a0 = min(max(rng[4 * f + 0], 0), n_crows);
            a1 = min(max(rng[4 * f + 1], 0), n_crows);
            b0 = min(max(rng[4 * f + 2], 0), n_crows);
            b1 = min(max(rng[4 * f + 3], 0), n_crows);
            const bool has_a = a1 > a0, has_b = b1 > b0;
            c_lo = has_a ? (has_b ? min(a0, b0) : a0) : b0;
            c_hi = has_a ? (has_b ? max(a1, b1) : a1) : (has_b ? b1 : b0);
        }
        float xr[P], xi[P], zr[HP], zi[HP];
        float twr[HP], twi[HP];   // CR: the steps' twiddles (see merge_twiddle)
        if constexpr (CR) {
#pragma unroll
            for (int j = 0; j < HP; ++j) merge_twiddle<P>(j, wl_c, wl_s, twr[j], twi[j]);
        }
#pragma unroll
        for (int c = 0; c < HP; c += CH) {
            float v[3][CH], vq[3][CH], g[3][CH], gq[3][CH];
            float ga[3][CH], gqa[3][CH];   // CR: the group's gathered gradients, formed before its forward rows are loaded
            if constexpr (CR) {
#pragma unroll
                for (int s = 0; s < 3; ++s)
#pragma unroll
                    for (int e = 0; e < CH; ++e) ga[s][e] = gqa[s][e] = 0.0f;
                for (int r = c_lo; r < c_hi; ++r) {
                    const bool in_a = (r >= a0 && r < a1), in_b = (r >= b0 && r < b1);
                    if (!in_a && !in_b) continue;   // wave-uniform
                    const float t = rowt[r];
                    const float w = (in_a && in_b) ? 1.0f : (in_a ? 1.0f - t : t);
#pragma unroll
                    for (int s = 0; s < 3; ++s) {
                        if (!gsrc[s]) continue;   // wave-uniform: a null stream is never loaded
                        const float* lo = gsrc[s] + (long long)r * ldg + lane;
                        const float* hi = gsrc[s] + (long long)r * ldg + (M - lane);
#pragma unroll
                        for (int e = 0; e < CH; ++e) {
                            ga[s][e] = fmaf(w, lo[64 * (c + e)], ga[s][e]);
                            gqa[s][e] = fmaf(w, hi[-64 * (c + e)], gqa[s][e]);
                        }
                        if (c + CH >= HP) gh[s] = fmaf(w, lo[M / 2], gh[s]);
                    }
                }
            }
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                const float* lo = row[s] + lane;
                const float* hi = row[s] + (M - lane);
#pragma unroll
                for (int e = 0; e < CH; ++e) {
                    v[s][e] = lo[64 * (c + e)];
                    vq[s][e] = hi[-64 * (c + e)];
                    g[s][e] = gq[s][e] = 0.0f;
                }
            }
            if constexpr (!CR) {
#pragma unroll
                for (int s = 0; s < 3; ++s) {
                    if (!grow[s]) continue;   // wave-uniform
                    const float* lo = grow[s] + lane;
                    const float* hi = grow[s] + (M - lane);
#pragma unroll
                    for (int e = 0; e < CH; ++e) {
                        g[s][e] = lo[64 * (c + e)];
                        gq[s][e] = hi[-64 * (c + e)];
                    }
                }
            } else {
#pragma unroll
                for (int s = 0; s < 3; ++s)
#pragma unroll
                    for (int e = 0; e < CH; ++e) {
                        g[s][e] = ga[s][e];
                        gq[s][e] = gqa[s][e];
                    }
            }
#pragma unroll
            for (int e = 0; e < CH; ++e) {
                const int j = c + e;
                // bins 0 and M (lane 0 of step 0): Y = Re gX; every other bin: Y = gX / 2
                const bool edge = (j == 0) && lane0;
                const float sc = edge ? 1.0f : 0.5f;
                float x_r, x_i, p_r, p_i;
                ana_bwd_bin(v[0][e], v[1][e], v[2][e], g[0][e], g[1][e], g[2][e], sc, x_r, x_i);
                ana_bwd_bin(vq[0][e], vq[1][e], vq[2][e], gq[0][e], gq[1][e], gq[2][e], sc, p_r, p_i);
                x_i = edge ? 0.0f : x_i;
                p_i = edge ? 0.0f : p_i;
                if constexpr (!CR) merge_pair_step<P>(j, x_r, x_i, p_r, p_i, wl_c, wl_s, xr[j], xi[j], zr[j], zi[j]);
                else merge_pair_step_w(x_r, x_i, p_r, p_i, twr[j], twi[j], xr[j], xi[j], zr[j], zi[j]);
            }
        }
        {   // bin M/2 is its own mirror (lane 0): Z = 2 conj(Y).  Every lane loads "its" bin M/2 + lane (feat_load_paired)
            float v[3], g[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int s = 0; s < 3; ++s) v[s] = row[s][M / 2 + lane];
            if constexpr (!CR) {
#pragma unroll
                for (int s = 0; s < 3; ++s)
                    if (grow[s]) g[s] = grow[s][M / 2 + lane];
            } else {
#pragma unroll
                for (int s = 0; s < 3; ++s) g[s] = gh[s];
            }
            float h_r, h_i;
            ana_bwd_bin(v[0], v[1], v[2], g[0], g[1], g[2], 0.5f, h_r, h_i);
            merge_handover<P>(zr, zi, 2.0f * h_r, -2.0f * h_i, xr, xi, lane);
        }

        wave_fft<P, +1>(xr, xi, tw, xbuf, lane);

        // ---- register i holds b[2 n], b[2 n + 1], n = kappa + 64 brev(i): buffer index m is sample k = (m + rot) mod N of
        // the frame, kept for k < len.  Whatever the tables say, nothing is written outside the frame's own part of the
        // scratch, [soff[f], soff[f + 1]) within [0, scratch_floats).
        const FrameGeom fg = frame_geom(scratch, 0, fleft[f], fright[f], N);   // (base is not used: the samples go to dst)
        const long long so = soff[f], cap = soff[f + 1] - so;
        const bool fits = so >= 0 && cap >= 0 && so + cap <= scratch_floats;
        const int nvalid = fits ? max((int)min((long long)fg.len, cap), 0) : 0;
        float* dst = scratch + so;
#pragma unroll
        for (int i = 0; i < P; ++i) {
            const int m0 = 2 * (kap + 64 * brev(i, LB));
            int k0 = m0 + fg.rot;
            k0 = (k0 >= N) ? k0 - N : k0;
            int k1 = m0 + 1 + fg.rot;
            k1 = (k1 >= N) ? k1 - N : k1;
            if ((unsigned)k0 < (unsigned)nvalid) dst[k0] = xr[i] * hann_half(k0, fg.L, fg.LR, fg.kadd, fg.invL, fg.invR);
            if ((unsigned)k1 < (unsigned)nvalid) dst[k1] = xi[i] * hann_half(k1, fg.L, fg.LR, fg.kadd, fg.invL, fg.invR);
        }
    }
}

__global__ __launch_bounds__(256) void k_analysis_bwd_gather(const float* __restrict__ scratch, long long scratch_floats,
                                                             const long long* __restrict__ fpos,
                                                             const int* __restrict__ fleft,
                                                             const long long* __restrict__ soff, long long nframes,
                                                             float* __restrict__ gsig, long long total) {
    // the first frame that ends after the workgroup's first sample: one binary search per workgroup (wave-uniform: scalar
    // loads) over the frames' ends, which are non-decreasing; every thread then walks on from there
    const long long t0 = (long long)blockIdx.x * 256;
    long long lo = 0, hi = nframes;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        const long long end = fpos[mid] - fleft[mid] + (soff[mid + 1] - soff[mid]);   // one past the frame's last sample
        if (end > t0) hi = mid; else lo = mid + 1;
    }
    const long long t = t0 + threadIdx.x;
    if (t >= total) return;
    float acc = 0.0f;
    for (long long f = lo; f < nframes; ++f) {
        const long long start = fpos[f] - fleft[f];
        if (start > t) break;   // starts are non-decreasing: no later frame covers t
        const long long o = soff[f], n = soff[f + 1] - o, k = t - start;
        if (k < n && o >= 0 && o + n <= scratch_floats) acc += scratch[o + k];
    }
    gsig[t] = acc;
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

int mpx_analysis_lossless_backward(void* stream, int fft_len, const void* tables, const float* mag, const float* real,
                                   const float* imag, int64_t ld, const float* grad_mag, const float* grad_real,
                                   const float* grad_imag, int64_t ld_grad, const int64_t* frame_pos,
                                   const int32_t* frame_left, const int32_t* frame_right, const int64_t* scratch_off,
                                   int64_t n_frames, float* scratch, int64_t scratch_floats, float* grad_sig,
                                   int64_t total_smpls) {
    const int P = p_of(fft_len);
    if (!P) return fail(MPX_ERR_ARG, "mpx_analysis_lossless_backward: fft_len must be 1024, 2048 or 4096%s");
    if (n_frames < 0 || total_smpls < 0 || scratch_floats < 0)
        return fail(MPX_ERR_ARG, "mpx_analysis_lossless_backward: negative count%s");
    if (ld < fft_len / 2 + 1 || ld_grad < fft_len / 2 + 1)
        return fail(MPX_ERR_ARG, "mpx_analysis_lossless_backward: ld < fft_len/2 + 1%s");
    if (n_frames == 0) return MPX_OK;
    if (!grad_mag && !grad_real && !grad_imag) return MPX_OK;   // nothing to propagate: grad_sig is not written
    if (!tables || !mag || !real || !imag || !frame_pos || !frame_left || !frame_right || !scratch_off ||
        (scratch_floats > 0 && !scratch) || (total_smpls > 0 && !grad_sig))
        return fail(MPX_ERR_ARG, "mpx_analysis_lossless_backward: null pointer%s");
    if ((total_smpls + 255) / 256 > 2147483647LL)
        return fail(MPX_ERR_ARG, "mpx_analysis_lossless_backward: too many samples%s");
    hipStream_t s = (hipStream_t)stream;
#define MPX_LAUNCH_ABWD(PP)                                                                                           \
    do {                                                                                                              \
        const dim3 grid(grid_for(n_frames, ana_bwd_waves<PP>())), block(64 * ana_bwd_waves<PP>());                    \
        if (int rc = set_lds((k_analysis_lossless_bwd<PP>), lds_bytes_ana_bwd<PP>())) return rc;                      \
        hipLaunchKernelGGL((k_analysis_lossless_bwd<PP>), grid, block, lds_bytes_ana_bwd<PP>(), s, mag, real, imag,   \
                           (long long)ld, grad_mag, grad_real, grad_imag, (long long)ld_grad, frame_left, frame_right, \
                           (const long long*)scratch_off, (long long)n_frames, (const float*)tables, scratch,         \
                           (long long)scratch_floats, (const int*)nullptr, (const float*)nullptr, 0);                \
    } while (0)
    if (P == 32) MPX_LAUNCH_ABWD(32);
    else if (P == 16) MPX_LAUNCH_ABWD(16);
    else MPX_LAUNCH_ABWD(8);
#undef MPX_LAUNCH_ABWD
    MPX_HIP_CHECK(hipGetLastError());
    if (total_smpls > 0) {
        hipLaunchKernelGGL(k_analysis_bwd_gather, dim3((unsigned)((total_smpls + 255) / 256)), dim3(256), 0, s, scratch,
                           (long long)scratch_floats, (const long long*)frame_pos, frame_left,
                           (const long long*)scratch_off, (long long)n_frames, grad_sig, (long long)total_smpls);
        MPX_HIP_CHECK(hipGetLastError());
    }
    return MPX_OK;
}

int mpx_analysis_lossless_const_rate_backward(void* stream, int fft_len, const void* tables, const float* mag,
                                              const float* real, const float* imag, int64_t ld, const float* grad_mag,
                                              const float* grad_real, const float* grad_imag, int64_t ld_grad,
                                              int64_t n_const_rows, const int32_t* ranges, const float* row_t,
                                              const int64_t* frame_pos, const int32_t* frame_left,
                                              const int32_t* frame_right, const int64_t* scratch_off, int64_t n_frames,
                                              float* scratch, int64_t scratch_floats, float* grad_sig,
                                              int64_t total_smpls) {
    const int P = p_of(fft_len);
    if (!P) return fail(MPX_ERR_ARG, "mpx_analysis_lossless_const_rate_backward: fft_len must be 1024, 2048 or 4096%s");
    if (n_frames < 0 || total_smpls < 0 || scratch_floats < 0 || n_const_rows < 0)
        return fail(MPX_ERR_ARG, "mpx_analysis_lossless_const_rate_backward: negative count%s");
    if (ld < fft_len / 2 + 1 || ld_grad < fft_len / 2 + 1)
        return fail(MPX_ERR_ARG, "mpx_analysis_lossless_const_rate_backward: ld < fft_len/2 + 1%s");
    if (n_const_rows > 2147483647LL)
        return fail(MPX_ERR_ARG, "mpx_analysis_lossless_const_rate_backward: too many constant-rate rows%s");
    if (n_frames == 0) return MPX_OK;
    if (!grad_mag && !grad_real && !grad_imag) return MPX_OK;   // nothing to propagate: grad_sig is not written
    if (!tables || !mag || !real || !imag || !frame_pos || !frame_left || !frame_right || !scratch_off ||
        (scratch_floats > 0 && !scratch) || (total_smpls > 0 && !grad_sig) || (n_const_rows > 0 && (!ranges || !row_t)))
        return fail(MPX_ERR_ARG, "mpx_analysis_lossless_const_rate_backward: null pointer%s");
    if ((total_smpls + 255) / 256 > 2147483647LL)
        return fail(MPX_ERR_ARG, "mpx_analysis_lossless_const_rate_backward: too many samples%s");
    hipStream_t s = (hipStream_t)stream;
    if (n_const_rows == 0) {   // no row reads any frame: the gradient is zero (and the tables may be null)
        if (total_smpls > 0) MPX_HIP_CHECK(hipMemsetAsync(grad_sig, 0, sizeof(float) * (size_t)total_smpls, s));
        return MPX_OK;
    }
#define MPX_LAUNCH_ABWD_CR(PP)                                                                                        \
    do {                                                                                                              \
        const dim3 grid(grid_for(n_frames, ana_bwd_waves<PP>())), block(64 * ana_bwd_waves<PP>());                    \
        if (int rc = set_lds((k_analysis_lossless_bwd<PP, true>), lds_bytes_ana_bwd<PP>())) return rc;                \
        hipLaunchKernelGGL((k_analysis_lossless_bwd<PP, true>), grid, block, lds_bytes_ana_bwd<PP>(), s, mag, real,   \
                           imag, (long long)ld, grad_mag, grad_real, grad_imag, (long long)ld_grad, frame_left,       \
                           frame_right, (const long long*)scratch_off, (long long)n_frames, (const float*)tables,     \
                           scratch, (long long)scratch_floats, ranges, row_t, (int)n_const_rows);                    \
    } while (0)
    if (P == 32) MPX_LAUNCH_ABWD_CR(32);
    else if (P == 16) MPX_LAUNCH_ABWD_CR(16);
    else MPX_LAUNCH_ABWD_CR(8);
#undef MPX_LAUNCH_ABWD_CR
    MPX_HIP_CHECK(hipGetLastError());
    if (total_smpls > 0) {
        hipLaunchKernelGGL(k_analysis_bwd_gather, dim3((unsigned)((total_smpls + 255) / 256)), dim3(256), 0, s, scratch,
                           (long long)scratch_floats, (const long long*)frame_pos, frame_left,
                           (const long long*)scratch_off, (long long)n_frames, grad_sig, (long long)total_smpls);
        MPX_HIP_CHECK(hipGetLastError());
    }
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
