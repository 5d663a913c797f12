// magphase_grad_comp.hip -- backward pass of the compressed synthesis' frame kernel.
//
//   k_synth_comp_bwd<P, T2>  (T2: the type-2 synthesis, section 3.3l -- below)
//                        one wavefront per frame, persistent waves (grid-stride over frames), the shape of
//                        k_synth_lossless_bwd (magphase_grad.hip).  Per frame, two real transforms of N points, each as one
//                        64*P-point complex wave FFT plus the real split:
//                          1. Ns, the spectrum of the frame's windowed, rotated noise -- the forward's own inputs (noise,
//                             npos / nleft / nright / wtype) and the forward's arithmetic in its plain form (whole-height
//                             exchange buffer, tiles of N/2 samples); kept in registers in the paired layout (own bins
//                             kappa + 64 q, mirrors M - k, bin M/2);
//                          2. gS, the gradient with respect to the frame's spectrum: the N gradient samples under the
//                             frame -> LDS -> times the anti-ringing window (the forward's win_add arithmetic) -> rotated by
//                             N/2 -> FFT -> split, consumed bin pair by bin pair as it appears.
//                        A second real transform and not one N-point complex transform of (gradient, noise): that one needs
//                        a 128*P-point wave FFT, twice the spectrum registers of the largest instance there is.
//                        Epilogue per bin against the frame's unwarped rows (m, a, b), the per-bin curves and the frame's
//                        noise gain, then coalesced stores: grad m over all H bins, grad a / grad b over the first n_phase
//                        bins (zeros in unvoiced frames).  Every element of a non-null output is written exactly once.
//
// Forward (k_synth_comp_pair, magphase_comp.hip), frame f, bin k:
//   u = (a + j b) / |a + j b| (0 where that is 0),  T = P u + A ig Ns,  S = m T,  S_0 <- |S_0|, S_M <- |S_M|,
//   y = overlap-add of w_f fftshift(irfft(S))
// with P = per_v (voiced) / 0, A = ap_v / ap_u, ig = inv_gain[f], w_f the anti-ringing window.  irfft, the window and the
// overlap-add are linear: gS_k = (c_k / N) FFT_N(ifftshift(w_f g))_k, c_k = 2 inside and 1 at the two ends; at the ends the
// real gradient Re gS goes along S / |S| (0 where S == 0).  Then
//   grad m = Re(conj(T) gS),   grad (a, b) = (m P / den) (gS - u Re(conj(u) gS))      (den == 0: u = 0, m P gS: bwd_bin)
// T2 (the T2 arm of k_synth_comp_pair; mpx_synthesis_compressed_type2_backward): S_0 <- Re S_0, S_M <- Re S_M, a linear
// map: the real end-bin gradient goes straight through, gS_end = (Re gS, 0), no projection on S / |S|; everything after it
// is the same (at the ends grad b = -(m P / den) u_i u_r Re gS, in general not zero).
#include "mpx_common.hpp"

namespace mpx {

// The frame's window into the gradient buffer, and its asynchronous copy into LDS: as in magphase_grad.hip (which see).
struct CompGradGeom {
    const float* base;
    int lo, hi;
};

__device__ __forceinline__ CompGradGeom comp_grad_geom(const float* __restrict__ gy, long long total, long long pos, int lo,
                                                       int hi, int N) {
    CompGradGeom g;
    // whatever the tables say, no address outside [gy, gy + total) is formed for a read
    const long long lo_b = (pos < 0) ? -pos : 0, hi_b = total - pos;
    g.lo = (int)max((long long)max(lo, 0), min(lo_b, (long long)N));
    g.hi = (int)min((long long)min(hi, N), max(hi_b, 0ll));
    g.hi = max(g.hi, g.lo);
    g.base = gy + pos;
    return g;
}

// Gradient samples [tile0, tile0 + 64 P) -> LDS in sample order; reads clamped into [lo, hi), 64-sample rows wholly outside
// it are not copied (the gather masks by sample index, it never multiplies what it does not keep).
template <int P>
__device__ __forceinline__ void comp_stage_grad_async(const CompGradGeom& g, int tile0, unsigned lds_byte, int lane) {
    if (g.hi <= g.lo) return;   // nothing kept of the frame: no address is formed at all
    for (int c = 0; c < P; ++c) {
        const int n0 = tile0 + 64 * c;
        if (n0 + 64 <= g.lo || n0 >= g.hi) continue;   // wave-uniform
        const float* src = g.base + min(max(n0 + lane, g.lo), g.hi - 1);
        const unsigned m0v = __builtin_amdgcn_readfirstlane(lds_byte + 256u * (unsigned)c);
        asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dword %0, off" ::"v"(src), "s"(m0v) : "m0", "memory");
    }
}

// The exchange buffer is about to be overwritten by a copy: every LDS read of it has returned.
__device__ __forceinline__ void comp_xbuf_idle() {
    wave_sync();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// Windowed noise frame -> N-point real FFT as a 64*P-point complex one (register i <-> Z[kappa + 64 brev(i)]): the plain
// form of noise_fft (magphase_comp.hip) -- tiles of 64 P samples, window in LDS, gather y[n] = x[(n + rot) mod N].
template <int P>
__device__ __forceinline__ void comp_bwd_noise_fft(const FrameGeom& g, int wtype, const float* tw, float* xbuf,
                                                   unsigned xbuf_byte, int lane, float (&re)[P], float (&im)[P]) {
    constexpr int M = 64 * P, N = 2 * M, kTile = noise_tile_len(P, false);
#pragma unroll
    for (int j = 0; j < P; ++j) re[j] = im[j] = 0.0f;
    const int ntiles = MPX_NOISE_TILES(g.len, kTile);
    for (int t = 0; t < ntiles; ++t) {
        const int tile0 = t * kTile;
        comp_xbuf_idle();
        stage_samples_async(g, tile0, kTile, xbuf_byte, lane);
        staged_wait<0>();
        const int hi = min(g.len, tile0 + kTile);
        if (wtype == 0) {
            for (int k = tile0 + lane; k < hi; k += 64)
                xbuf[k - tile0] *= half_window(k, g.L, g.LR, g.kadd, g.invL, g.invR, 0);
        } else {
            for (int k = tile0 + lane; k < hi; k += 64)
                xbuf[k - tile0] *= half_window(k, g.L, g.LR, g.kadd, g.invL, g.invR, 1);
        }
        wave_sync();
        {
            int n_lo = g.len - g.rot, n_hi = N - g.rot;
            asm volatile("" : "+s"(n_lo), "+s"(n_hi));
            const unsigned span = (unsigned)(hi - tile0);
            const unsigned b0 = (unsigned)(2 * lane + g.rot) - (unsigned)tile0;
#pragma unroll
            for (int j = 0; j < P; ++j) {
                const int m0 = 128 * j;
                if (MPX_NOISE_ROW_ACTIVE(m0, n_lo, n_hi)) {
                    const unsigned d0 = (b0 + (unsigned)m0) & (unsigned)(N - 1), d1 = (d0 + 1u) & (unsigned)(N - 1);
                    const float v0 = xbuf[min(d0, (unsigned)(kTile - 1))], v1 = xbuf[min(d1, (unsigned)(kTile - 1))];
                    re[j] = (d0 < span) ? v0 : re[j];
                    im[j] = (d1 < span) ? v1 : im[j];
                }
            }
        }
        wave_sync();
    }
    wave_fft<P, -1>(re, im, tw, xbuf, lane);
}

// One bin of the epilogue.  (m, a, b): the frame's unwarped features, cpv = P_k (0 in unvoiced frames and from n_per on),
// cap = A_k ig, (nr, ni) = Ns_k, (gr, gi) = gS_k; ends: bins 0 and N/2, where the forward keeps |S| and gi comes in as 0.
// rsq(max(s, tiny)) multiplies a == b == 0 when s == 0: u = 0, and the phase gradient is m P gS (bwd_bin's convention).
// T2: the forward keeps Re S at the ends -- (gr, 0) is the gradient with respect to S as it comes in.
template <bool T2 = false>
__device__ __forceinline__ void comp_bwd_bin(float m, float a, float b, float cpv, float cap, float nr, float ni, float gr,
                                             float gi, bool ends, float& om, float& oa, float& ob) {
    const float s = a * a + b * b;
    const float r = __builtin_amdgcn_rsqf(fmaxf(s, 1.0e-37f));
    const float ur = a * r, ui = b * r;
    const float tr = fmaf(nr, cap, cpv * ur), ti = fmaf(ni, cap, cpv * ui);
    if constexpr (!T2) {
        if (ends) {   // S = m T -> |S|: the (real) gradient goes along S / |S| = sign(m) T / |T|, 0 where S == 0
            const float t2 = tr * tr + ti * ti;
            const float sg = (m > 0.0f) ? 1.0f : ((m < 0.0f) ? -1.0f : 0.0f);
            const float inv = (t2 >= 1.0e-37f) ? sg * __builtin_amdgcn_rsqf(t2) : 0.0f;
            gi = gr * ti * inv;
            gr = gr * tr * inv;
        }
    }
    om = tr * gr + ti * gi;
    const float d = ur * gr + ui * gi;
    const float mr = m * cpv * ((s > 0.0f) ? r : 1.0f);
    oa = mr * (gr - ur * d);
    ob = mr * (gi - ui * d);
}

struct CompBwdArgs {
    const float* gy;          // dL/d(waveform before the output high-pass), [total_out]
    long long total_out;
    const long long* gpos;    // hostmath.lossless_backward_table: where the frame finds its gradient samples
    const int* glo;
    const int* ghi;
    long long nframes;
    const float* tw;
    const float* mag;         // the forward's unwarped rows, one per frame, pitch ld
    const float* real;
    const float* imag;
    long long ld;
    const float* noise;
    const long long* npos;
    const int* nleft;
    const int* nright;
    const int* wtype;
    const int* voiced;
    const float* inv_gain;
    const int* win_l;
    const int* win_r;
    const float* per_v;
    const float* ap_v;
    const float* ap_u;
    int n_per;                // bins from n_per on have no periodic component: their phase rows are not read
    int n_phase;              // columns of grad a / grad b that are written: min(n_per rounded up to 64, H)
    float* omag;              // [nframes x ldg], null: not computed
    float* oreal;
    float* oimag;
    long long ldg;
};

// Waves per workgroup: two per SIMD for P = 8 / 16.  P = 32 holds the noise spectrum (66 registers) beside the 64 of the
// gradient transform and its partner bins: more than the 256 registers of a wave at two per SIMD (29 spilled), so one
// per SIMD there.
template <int P>
constexpr int comp_bwd_waves() { return P == 32 ? 4 : kWavesPerBlock; }
template <int P>
constexpr size_t lds_bytes_comp_bwd() { return sizeof(float) * (size_t)(tw_floats<P>() + comp_bwd_waves<P>() * P * kXStride); }

template <int P, bool T2 = false>
__global__ __launch_bounds__(64 * comp_bwd_waves<P>()) void k_synth_comp_bwd(CompBwdArgs A) {
    constexpr int M = 64 * P, N = 2 * M, LB = ilog2(P), HP = P / 2;
    constexpr int kWaves = comp_bwd_waves<P>(), kThr = 64 * kWaves;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* tw = smem;
    const int lane_id = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    float* xbuf = smem + tw_floats<P>() + wave * (P * kXStride);
    // byte address of xbuf in LDS (the dynamic segment starts at 0: the kernel has no static __shared__)
    const unsigned xbuf_byte = 4u * (unsigned)(tw_floats<P>() + rfl(wave) * (P * kXStride));
    for (int i = threadIdx.x; i < tw_floats<P>(); i += kThr) tw[i] = A.tw[i];
    __syncthreads();

    // lane part of the split twiddle W_N^kappa = e^{-2 pi i kappa / N}
    float wl_s0, wl_c0;
    sincospif(-2.0f * (float)kappa<P>(lane_id) / (float)N, &wl_s0, &wl_c0);

    const long long fstep = (long long)gridDim.x * kWaves;
    for (long long f = (long long)blockIdx.x * kWaves + rfl(wave); f < A.nframes; f += fstep) {
        // Launder the per-lane invariants once per frame (see k_analysis: LICM would hoist every lane x register product)
        int lane = lane_id;
        float wl_s = wl_s0, wl_c = wl_c0;
        asm volatile("" : "+v"(lane), "+v"(wl_s), "+v"(wl_c));
        const int kap = kappa<P>(lane);
        const int src_lane = kappa<P>((64 - kap) & 63);
        const bool lane0 = (kap == 0);

        // ---- 1. Ns in the paired layout: own bins kap + 64 q (no_*), mirrors M - k (nm_*; lane 0 of q == 0: bin M, real),
        // bin M/2 on lane 0 (nh_*)
        float no_r[HP], no_i[HP], nm_r[HP], nm_i[HP], nh_r, nh_i;
        {
            const FrameGeom ng = frame_geom(A.noise, A.npos[f], A.nleft[f], A.nright[f], N);
            float re[P], im[P];
            comp_bwd_noise_fft<P>(ng, A.wtype[f], tw, xbuf, xbuf_byte, lane, re, im);
            constexpr int SB = (HP < 8) ? HP : 8;   // partner bins SB at a time (noise_spectrum_paired)
#pragma unroll
            for (int qb = 0; qb < HP; qb += SB) {
                float zpr[SB], zpi[SB];
#pragma unroll
                for (int u = 0; u < SB; ++u) {
                    const int i = brev(qb + u, LB);
                    zpr[u] = __shfl(re[P - 1 - i], src_lane);
                    zpi[u] = __shfl(im[P - 1 - i], src_lane);
                }
#pragma unroll
                for (int u = 0; u < SB; ++u) {
                    const int q = qb + u;
                    const int i = brev(q, LB);
                    const int i0 = brev((P - q) % P, LB);
                    const float pr = lane0 ? re[i0] : zpr[u];
                    const float pi = lane0 ? im[i0] : zpi[u];
                    const float er = 0.5f * (re[i] + pr), ei = 0.5f * (im[i] - pi);
                    const float orr = 0.5f * (im[i] + pi), oi = -0.5f * (re[i] - pr);
                    const float cq = cos2p<P>(q), sq = -sin2p<P>(q);   // W_N^k = W_N^kappa * e^{-2 pi i q/(2P)}
                    const float wr = wl_c * cq - wl_s * sq, wi = wl_c * sq + wl_s * cq;
                    const float tr = wr * orr - wi * oi, ti = wr * oi + wi * orr;
                    no_r[q] = er + tr;
                    no_i[q] = ei + ti;
                    nm_r[q] = er - tr;
                    nm_i[q] = ti - ei;
                }
            }
            nh_r = re[1];    // bin M/2 = register brev(P/2) = 1 of the kappa == 0 lane: X = conj Z
            nh_i = -im[1];
        }

        // ---- 2. the gradient window: N samples through LDS, two tiles of N/2; times the anti-ringing window (centred at
        // N/2, support [N/2 - wl, N/2 + wr]: the forward's win_add); gathered in FFT order with the fixed rotation N/2
        // (ifftshift): buffer index m = 128 j + 2 lane (+ 1) holds sample (m + N/2) mod N -- tile 0 is the registers
        // j >= P/2, tile 1 the registers j < P/2
        const CompGradGeom g = comp_grad_geom(A.gy, A.total_out, A.gpos[f], A.glo[f], A.ghi[f], N);
        const int wl = A.win_l[f], wr_ = A.win_r[f];
        const float inv_wl = (wl > 0) ? 1.0f / (float)wl : 1.0f;
        const float inv_wr = (wr_ > 0) ? 1.0f / (float)wr_ : 0.0f;
        const int kadd = (wl == 0) ? 1 : 0;
        const int w_lo = M - wl, w_hi = M + wr_;
        auto win = [&](int n) {
            const int ks = n - w_lo;
            return (ks >= 0 && n <= w_hi) ? half_window(ks, wl, wl + wr_, kadd, inv_wl, inv_wr, 0) : 0.0f;
        };
        float re[P], im[P];
        comp_xbuf_idle();
        comp_stage_grad_async<P>(g, 0, xbuf_byte, lane);
        staged_wait<0>();
#pragma unroll
        for (int j = HP; j < P; ++j) {
            const int k0 = 128 * (j - HP) + 2 * lane;
            const float2 v = *reinterpret_cast<const float2*>(xbuf + k0);
            re[j] = (k0 >= g.lo && k0 < g.hi) ? v.x * win(k0) : 0.0f;
            im[j] = (k0 + 1 >= g.lo && k0 + 1 < g.hi) ? v.y * win(k0 + 1) : 0.0f;
        }
        comp_xbuf_idle();   // tile 0 has been read before the copy overwrites it
        comp_stage_grad_async<P>(g, M, xbuf_byte, lane);
        staged_wait<0>();
#pragma unroll
        for (int j = 0; j < HP; ++j) {
            const int k0 = 128 * j + 2 * lane;
            const float2 v = *reinterpret_cast<const float2*>(xbuf + k0);
            re[j] = (M + k0 >= g.lo && M + k0 < g.hi) ? v.x * win(M + k0) : 0.0f;
            im[j] = (M + k0 + 1 >= g.lo && M + k0 + 1 < g.hi) ? v.y * win(M + k0 + 1) : 0.0f;
        }
        wave_sync();
        wave_fft<P, -1>(re, im, tw, xbuf, lane);

        // ---- 3. split (one (k, M - k) bin pair per step q) and epilogue.  Stores share k_synth_lossless_bwd's layout: the
        // ascending stream at kap + 64 q, the mirrors regrouped into 64-bin blocks [M - 64 q, M - 64 q + 63] (block of
        // step q - 1 stored during step q with lane 0's own output of step q).
        const int voiced = A.voiced[f];
        const float ig = A.inv_gain[f];
        const float* apc = voiced ? A.ap_v : A.ap_u;
        const int n_per = voiced ? A.n_per : 0;    // unvoiced frames: no phase row is read, P = 0
        const float* mrow = A.mag + f * A.ld;
        const float* arow = A.real + f * A.ld;
        const float* brow = A.imag + f * A.ld;
        float* row_m = A.omag + f * A.ldg;     // a stream that needs no gradient is a null pointer: never dereferenced
        float* row_r = A.oreal + f * A.ldg;
        float* row_i = A.oimag + f * A.ldg;
        const int n_phase = A.n_phase;
        const int hoff = lane0 ? M - 64 : M - kap;
        constexpr float kS2 = 2.0f / (float)N, kS1 = 1.0f / (float)N;
        // the features of bin k: the phase rows and the periodic curve only below n_per (per lane; what lies above was
        // never produced by the forward)
        auto feat = [&](int k, float& m, float& a, float& b, float& cpv, float& cap) {
            m = mrow[k];
            cap = apc[k] * ig;
            const bool ph = k < n_per;
            a = ph ? arow[k] : 0.0f;
            b = ph ? brow[k] : 0.0f;
            cpv = ph ? A.per_v[k] : 0.0f;
        };
        float hm = 0.0f, hr = 0.0f, hi_ = 0.0f;   // mirror outputs of the previous step
        constexpr int SB = (HP < 8) ? HP : 8;
#pragma unroll
        for (int qb = 0; qb < HP; qb += SB) {
            float zpr[SB], zpi[SB];
#pragma unroll
            for (int u = 0; u < SB; ++u) {
                const int i = brev(qb + u, LB);
                zpr[u] = __shfl(re[P - 1 - i], src_lane);
                zpi[u] = __shfl(im[P - 1 - i], src_lane);
            }
            // keep the batch's feature loads here (the compiler moves loads of read-only memory across plain barriers;
            // hoisted above the transforms they spill): the lane's bin offset is laundered with a fake dependency on the
            // batch's partner bins
            int kapb = kap;
            asm volatile("" : "+v"(kapb) : "v"(zpr[0]), "v"(zpi[0]), "v"(zpr[SB - 1]), "v"(zpi[SB - 1]));
#pragma unroll
            for (int u = 0; u < SB; ++u) {
                const int q = qb + u;
                const int i = brev(q, LB);
                const int i0 = brev((P - q) % P, LB);
                const float pr = lane0 ? re[i0] : zpr[u];
                const float pi = lane0 ? im[i0] : zpi[u];
                const float er = 0.5f * (re[i] + pr), ei = 0.5f * (im[i] - pi);
                const float orr = 0.5f * (im[i] + pi), oi = -0.5f * (re[i] - pr);
                const float cq = cos2p<P>(q), sq = -sin2p<P>(q);
                const float wr = wl_c * cq - wl_s * sq, wi = wl_c * sq + wl_s * cq;
                const float tr = wr * orr - wi * oi, ti = wr * oi + wi * orr;
                // bins 0 and M (lane 0 of step 0): c_k = 1 and the imaginary part dropped
                const bool edge = (q == 0) && lane0;
                const float sc = edge ? kS1 : kS2, sci = edge ? 0.0f : kS2;
                const int k_own = kapb + 64 * q, k_mir = M - kapb - 64 * q;   // (lane 0 of step 0: bin M)
                float fm, fa, fb, fp, fc, fmq, faq, fbq, fpq, fcq;
                feat(k_own, fm, fa, fb, fp, fc);
                feat(k_mir, fmq, faq, fbq, fpq, fcq);
                {
                    float cm, cr, ci;
                    comp_bwd_bin<T2>(fm, fa, fb, fp, fc, no_r[q], no_i[q], (er + tr) * sc, (ei + ti) * sci, edge, cm, cr, ci);
                    if (A.omag) row_m[k_own] = cm;
                    if (64 * q < n_phase) {   // wave-uniform: the whole 64-bin block lies below n_phase
                        if (A.oreal) row_r[k_own] = cr;
                        if (A.oimag) row_i[k_own] = ci;
                    }
                }
                {
                    float cm, cr, ci;
                    comp_bwd_bin<T2>(fmq, faq, fbq, fpq, fcq, nm_r[q], nm_i[q], (er - tr) * sc, (ti - ei) * sci, edge, cm, cr, ci);
                    if (q == 0) {
                        if (lane0) {                      // bin M
                            if (A.omag) row_m[M] = cm;
                            if (M < n_phase) {
                                if (A.oreal) row_r[M] = cr;
                                if (A.oimag) row_i[M] = ci;
                            }
                        }
                    } else {                              // block [M - 64 q, M - 64 q + 63]
                        if (A.omag) row_m[hoff - 64 * (q - 1)] = lane0 ? cm : hm;
                        if (M - 64 * q < n_phase) {
                            if (A.oreal) row_r[hoff - 64 * (q - 1)] = lane0 ? cr : hr;
                            if (A.oimag) row_i[hoff - 64 * (q - 1)] = lane0 ? ci : hi_;
                        }
                    }
                    hm = cm;
                    hr = cr;
                    hi_ = ci;
                }
            }
        }
        {   // block [M/2, M/2 + 63]: lane 0 supplies bin M/2 (register 1 holds q = P/2): G = conj Z.  Every lane loads "its"
            // bin M/2 + kappa (in range; only lane 0's result is stored)
            float fm, fa, fb, fp, fc, cm, cr, ci;
            feat(M / 2 + kap, fm, fa, fb, fp, fc);
            comp_bwd_bin<T2>(fm, fa, fb, fp, fc, nh_r, nh_i, re[1] * kS2, -im[1] * kS2, false, cm, cr, ci);
            if (A.omag) row_m[hoff - 64 * (HP - 1)] = lane0 ? cm : hm;
            if (M / 2 < n_phase) {
                if (A.oreal) row_r[hoff - 64 * (HP - 1)] = lane0 ? cr : hr;
                if (A.oimag) row_i[hoff - 64 * (HP - 1)] = lane0 ? ci : hi_;
            }
        }
    }
}

}  // namespace mpx

using namespace mpx;

// T2: the type-2 arm of k_synth_comp_bwd (mpx_synthesis_compressed_type2_backward); who: the entry's name for the messages
template <bool T2>
static int synthesis_compressed_backward_impl(const char* who, void* stream, int fft_len, const void* tables,
                                              const float* grad_out, int64_t total_out, const int64_t* grad_pos,
                                              const int32_t* grad_lo, const int32_t* grad_hi, int64_t n_frames,
                                              const float* mag, const float* real, const float* imag, int64_t ld,
                                              const float* noise, const int64_t* noise_pos, const int32_t* noise_left,
                                              const int32_t* noise_right, const int32_t* noise_wtype, const int32_t* voiced,
                                              const float* inv_gain, const int32_t* win_left, const int32_t* win_right,
                                              const float* per_v, const float* ap_v, const float* ap_u, int32_t n_per,
                                              float* grad_mag, float* grad_real, float* grad_imag, int64_t ld_grad) {
    const int P = p_of(fft_len);
    if (!P) return fail(MPX_ERR_ARG, "%s: fft_len must be 1024, 2048 or 4096", who);
    const int H = fft_len / 2 + 1;
    if (n_frames < 0 || total_out < 0) return fail(MPX_ERR_ARG, "%s: negative count", who);
    if (ld < H || ld_grad < H) return fail(MPX_ERR_ARG, "%s: ld < fft_len/2 + 1", who);
    if (n_per < 0 || n_per > H) return fail(MPX_ERR_ARG, "%s: n_per outside [0, fft_len/2 + 1]", who);
    if (n_frames == 0) return MPX_OK;
    if (!grad_mag && !grad_real && !grad_imag) return MPX_OK;   // nothing asked for
    if (!tables || !grad_pos || !grad_lo || !grad_hi || !mag || !real || !imag || !noise || !noise_pos || !noise_left ||
        !noise_right || !noise_wtype || !voiced || !inv_gain || !win_left || !win_right || !per_v || !ap_v || !ap_u ||
        (total_out > 0 && !grad_out))
        return fail(MPX_ERR_ARG, "%s: null pointer", who);
    CompBwdArgs a;
    a.gy = grad_out, a.total_out = (long long)total_out, a.gpos = (const long long*)grad_pos, a.glo = grad_lo, a.ghi = grad_hi;
    a.nframes = (long long)n_frames, a.tw = (const float*)tables, a.mag = mag, a.real = real, a.imag = imag;
    a.ld = (long long)ld, a.noise = noise, a.npos = (const long long*)noise_pos, a.nleft = noise_left, a.nright = noise_right;
    a.wtype = noise_wtype, a.voiced = voiced, a.inv_gain = inv_gain, a.win_l = win_left, a.win_r = win_right;
    a.per_v = per_v, a.ap_v = ap_v, a.ap_u = ap_u, a.n_per = n_per;
    a.n_phase = min((n_per + 63) / 64 * 64, H);
    a.omag = grad_mag, a.oreal = grad_real, a.oimag = grad_imag, a.ldg = (long long)ld_grad;
    hipStream_t s = (hipStream_t)stream;
#define MPX_LAUNCH_CBWD(PP)                                                                              \
    do {                                                                                                 \
        const dim3 grid(grid_for(n_frames, comp_bwd_waves<PP>())), block(64 * comp_bwd_waves<PP>());     \
        if (int rc = set_lds((k_synth_comp_bwd<PP, T2>), lds_bytes_comp_bwd<PP>())) return rc;           \
        hipLaunchKernelGGL((k_synth_comp_bwd<PP, T2>), grid, block, lds_bytes_comp_bwd<PP>(), s, a);     \
    } while (0)
    if (P == 32) MPX_LAUNCH_CBWD(32);
    else if (P == 16) MPX_LAUNCH_CBWD(16);
    else MPX_LAUNCH_CBWD(8);
#undef MPX_LAUNCH_CBWD
    MPX_HIP_CHECK(hipGetLastError());
    return MPX_OK;
}

extern "C" {

int mpx_synthesis_compressed_backward(void* stream, int fft_len, const void* tables, const float* grad_out,
                                      int64_t total_out, const int64_t* grad_pos, const int32_t* grad_lo,
                                      const int32_t* grad_hi, int64_t n_frames, const float* mag, const float* real,
                                      const float* imag, int64_t ld, const float* noise, const int64_t* noise_pos,
                                      const int32_t* noise_left, const int32_t* noise_right, const int32_t* noise_wtype,
                                      const int32_t* voiced, const float* inv_gain, const int32_t* win_left,
                                      const int32_t* win_right, const float* per_v, const float* ap_v, const float* ap_u,
                                      int32_t n_per, float* grad_mag, float* grad_real, float* grad_imag,
                                      int64_t ld_grad) {
    return synthesis_compressed_backward_impl<false>(
        "mpx_synthesis_compressed_backward", stream, fft_len, tables, grad_out, total_out, grad_pos, grad_lo, grad_hi,
        n_frames, mag, real, imag, ld, noise, noise_pos, noise_left, noise_right, noise_wtype, voiced, inv_gain, win_left,
        win_right, per_v, ap_v, ap_u, n_per, grad_mag, grad_real, grad_imag, ld_grad);
}

int mpx_synthesis_compressed_type2_backward(void* stream, int fft_len, const void* tables, const float* grad_out,
                                            int64_t total_out, const int64_t* grad_pos, const int32_t* grad_lo,
                                            const int32_t* grad_hi, int64_t n_frames, const float* mag, const float* real,
                                            const float* imag, int64_t ld, const float* noise, const int64_t* noise_pos,
                                            const int32_t* noise_left, const int32_t* noise_right,
                                            const int32_t* noise_wtype, const int32_t* voiced, const float* inv_gain,
                                            const int32_t* win_left, const int32_t* win_right, const float* per_v,
                                            const float* ap_v, const float* ap_u, int32_t n_per, float* grad_mag,
                                            float* grad_real, float* grad_imag, int64_t ld_grad) {
    return synthesis_compressed_backward_impl<true>(
        "mpx_synthesis_compressed_type2_backward", stream, fft_len, tables, grad_out, total_out, grad_pos, grad_lo, grad_hi,
        n_frames, mag, real, imag, ld, noise, noise_pos, noise_left, noise_right, noise_wtype, voiced, inv_gain, win_left,
        win_right, per_v, ap_v, ap_u, n_per, grad_mag, grad_real, grad_imag, ld_grad);
}

}  // extern "C"
