// magphase_comp.hip -- the noise transform and the kernels that overlap-add frames through a wave pair's LDS ring: the
// compressed-feature synthesis (synthesis_from_compressed, magphase.py:825-997) and, on the lossless path, the one-launch
// round trip and the Griffin-Lim iteration.
//
//   k_noise_stats<P>, k_noise_gains        per frame: windowed noise frame -> FFT -> sum_k (ln|Ns[k]|)^2 (Q10 gain statistics)
//   k_min_phase                            minimum-phase spectrum from a magnitude spectrum
//   the three pair kernels, built from one set of frame stages (pair_wave_setup .. pair_ordered_ola below):
//   k_synth_comp_pair<P>                   noise FFT (recomputed or stored) + periodic/aperiodic spectrum assembly (Appendix
//                                          A2 steps 9-12) + inverse FFT + anti-ringing window + overlap-add
//   k_roundtrip_pair<P>                    lossless analysis and synthesis of the same frames in one launch (copy synthesis)
//   k_griffin_lim_pair<P>                  one pitch-synchronous Griffin-Lim iteration
#include <type_traits>

#include "mpx_common.hpp"

// waves per workgroup of k_synth_comp_pair (8 = two per SIMD, 12 = three: compact transform front, <= 168 VGPRs)
#ifndef MPX_COMP_PAIR_WAVES
#define MPX_COMP_PAIR_WAVES 12
#endif
#ifndef MPX_COMP_DIT
#define MPX_COMP_DIT 0   // 1: both transforms of the compact form in the DIT form (wave_fft.hpp; parity-green): -1 % on the
                         // synthesis side of configs[2], but 10 registers spill again at 12 waves per CU: off
#endif
#ifndef MPX_COMP_CH
#define MPX_COMP_CH 16   // ring values in registers at a time in the pair kernels' overlap-add (ring_add_plane)
#endif

namespace mpx {

// ---------------------------------------------------------------------------------------------
// noise frame -> half spectrum in registers
// ---------------------------------------------------------------------------------------------
// noise_fft's zero fill, window and gather (the loop in its body, which see) for the rows of support class W alone (P/2:
// all rows); the registers of the other rows are not touched.  A copy of that loop and not its replacement: called from
// there, the same statements come out of the compiler as other (equivalent) code in every kernel that transforms a frame.
template <int P, bool PRESTAGED, bool COMPACT, int W>
__device__ __forceinline__ void noise_window_gather(const FrameGeom& g, int wtype, float* xbuf, unsigned xbuf_byte, int lane,
                                                    float (&re)[P], float (&im)[P]) {
    constexpr int M = 64 * P, N = 2 * M, kTile = noise_tile_len(P, COMPACT);
    MPX_MARK("zero_init");
#pragma unroll
    for (int j = 0; j < P; ++j)
        if (j < W || j >= P - W) re[(COMPACT && MPX_COMP_DIT) ? brev(j, ilog2(P)) : j] = im[(COMPACT && MPX_COMP_DIT) ? brev(j, ilog2(P)) : j] = 0.0f;
    const int ntiles = MPX_NOISE_TILES(g.len, kTile);   // (mpx_common.hpp: the planner's cost terms count the same tiles and rows)
    for (int t = 0; t < ntiles; ++t) {
        MPX_MARK("window");
        const int tile0 = t * kTile;
        if (!PRESTAGED || t > 0) {
            stage_samples_async(g, tile0, kTile, xbuf_byte, lane);
            staged_wait<0>();
        }
        const int hi = min(g.len, tile0 + kTile);
        // the window type is per frame (wave-uniform): one loop per type, not a select per sample
        if (wtype == 0) {
            for (int k = tile0 + lane; k < hi; k += 64)
                xbuf[k - tile0] *= half_window(k, g.L, g.LR, g.kadd, g.invL, g.invR, 0);
        } else {
            for (int k = tile0 + lane; k < hi; k += 64)
                xbuf[k - tile0] *= half_window(k, g.L, g.LR, g.kadd, g.invL, g.invR, 1);
        }
        wave_sync();
        MPX_MARK("gather");
        // (the gather of noise_fft, rows of the class only)
        {
            int n_lo = g.len - g.rot, n_hi = N - g.rot;
            asm volatile("" : "+s"(n_lo), "+s"(n_hi));   // evaluated here, per tile: not hoisted as 32 lane masks
            const unsigned span = (unsigned)(hi - tile0);
            const unsigned b0 = (unsigned)(2 * lane + g.rot) - (unsigned)tile0;
#pragma unroll
            for (int j = 0; j < P; ++j) {
                constexpr int LBJ = ilog2(P);
                const int m0 = 128 * j;
                if ((j < W || j >= P - W) && MPX_NOISE_ROW_ACTIVE(m0, n_lo, n_hi)) {
                    const int rj = (COMPACT && MPX_COMP_DIT) ? brev(j, LBJ) : j;   // the DIT form wants register brev(j) <- z[l + 64 j]
                    // sample index relative to the tile, modulo N (tile0 is a multiple of the tile length, which divides N)
                    const unsigned d0 = (b0 + (unsigned)m0) & (unsigned)(N - 1), d1 = (d0 + 1u) & (unsigned)(N - 1);
                    const float v0 = xbuf[min(d0, (unsigned)(kTile - 1))], v1 = xbuf[min(d1, (unsigned)(kTile - 1))];
                    re[rj] = (d0 < span) ? v0 : re[rj];
                    im[rj] = (d1 < span) ? v1 : im[rj];
                }
            }
        }
        wave_sync();
    }
}

// What a caller may place inside noise_fft (k_roundtrip_pair's direct arm): gathered(re, im, narrow_c) runs right after the
// gather, on the windowed, rotated frame in its registers (row j <-> samples 128 j + 2 lane, + 1; narrow_c: a
// std::bool_constant, whether this is the class arm, whose other rows are not defined yet); exchanged() runs once the forward
// transform has made its last use of the exchange buffer.  The default does nothing: every other caller's code is unchanged.
struct NoiseFftNoHook {
    template <int P, typename B>
    __device__ __forceinline__ void gathered(float (&)[P], float (&)[P], B) const {}
    __device__ __forceinline__ void exchanged() const {}
};
template <typename GFn, typename XFn>
struct NoiseFftHook {
    GFn on_gathered;
    XFn on_exchanged;
    template <int P, typename B>
    __device__ __forceinline__ void gathered(float (&re)[P], float (&im)[P], B narrow_c) const { on_gathered(re, im, narrow_c); }
    __device__ __forceinline__ void exchanged() const { on_exchanged(); }
};
template <typename GFn, typename XFn>
__device__ __forceinline__ NoiseFftHook<GFn, XFn> noise_fft_hook(GFn g, XFn x) { return NoiseFftHook<GFn, XFn>{g, x}; }

// Windowed noise frame (magphase.py:886-897: windowing() with per-frame window list, epoch moved to index 0 by
// frm_list_to_matrix + fftshift) -> N-point real FFT -> Ns[k] for the bins kappa(lane) + 64 j, j = 0..P-1
// (natural j), plus the Nyquist bin (real) on the lane with kappa == 0.  Synchronous staging (no prefetch).
// COMPACT (P == 32): half-height exchange buffer (tiles of 32 P samples) and half twiddle table (wave_fft_front_compact;
// (lc, ls) = W_128^lane) -- k_synth_comp_pair at 12 waves per CU.
// NW > 0 (compact DIF form only): where `narrow` (wave-uniform) holds, the frame is of support class NW
// (frame_support_class, mpx_common.hpp; the caller's promise) -- only the rows j < NW and j >= P - NW are gathered, the
// others are constants 0, and the stages of the first in-register pass that meet those zeros are pruned for them.  Two
// straight-line instances of the gather with those stages, one wave-uniform branch around them; everything else is shared.
template <int P, bool PRESTAGED = false, bool COMPACT = false, int NW = 0, typename Hook = NoiseFftNoHook>   // PRESTAGED: the caller already copied tile 0 into xbuf and waited for it
__device__ __forceinline__ void noise_fft(const FrameGeom& g, int wtype, const float* tw, float* xbuf,
                                          unsigned xbuf_byte, int lane, float (&re)[P], float (&im)[P], float lc = 1.0f,
                                          float ls = 0.0f, bool narrow = false, Hook hook = Hook()) {
    static_assert(NW == 0 || (COMPACT && !MPX_COMP_DIT), "support classes: the compact DIF form only");
    if constexpr (NW > 0) {
        // one wave-uniform choice per frame between two straight-line instances of the gather and of the stages of the
        // first in-register pass that meet the class's zeros (stride > S0); the rows outside the class are never written
        // before the pruned stages define them
        constexpr unsigned kZin = support_zero_rows<P>(NW);
        constexpr int S0 = zin_clear_stride<P>(kZin);
        static_assert(S0 >= 1 && S0 < P / 2, "a class prunes some, not all, stages of the first pass");
        if (narrow) {
            noise_window_gather<P, PRESTAGED, COMPACT, NW>(g, wtype, xbuf, xbuf_byte, lane, re, im);
            mpx_pin_live<~kZin>(re), mpx_pin_live<~kZin>(im);
            hook.gathered(re, im, std::true_type());
            MPX_MARK("fft_forward");
            fft_inreg_pruned_stage<P, -1, P / 2, kZin, kAllRegs, 2 * S0>(re, im);
            MPX_ARM_END_CLASS();
        } else {
            noise_window_gather<P, PRESTAGED, COMPACT, P / 2>(g, wtype, xbuf, xbuf_byte, lane, re, im);
            mpx_pin(re), mpx_pin(im);
            hook.gathered(re, im, std::false_type());
            MPX_MARK("fft_forward");
            fft_inreg_stages<P, -1, P / 2, 2 * S0>(re, im);
            MPX_ARM_END_FULL();
        }
        const float4 pk = tw_half_pad<P>(tw, lane);
        fft_inreg_stages<P, -1, S0>(re, im);
        wave_fft_front_compact_rest<P, -1>(re, im, tw, xbuf, lane, pk.z, pk.w);
        hook.exchanged();
        fft_inreg<P, -1>(re, im);
        (void)lc;
        (void)ls;
        return;
    }
    constexpr int M = 64 * P, N = 2 * M, kTile = noise_tile_len(P, COMPACT);
    MPX_MARK("zero_init");
#pragma unroll
    for (int j = 0; j < P; ++j) re[j] = im[j] = 0.0f;
    const int ntiles = MPX_NOISE_TILES(g.len, kTile);   // (mpx_common.hpp: the planner's cost terms count the same tiles and rows)
    for (int t = 0; t < ntiles; ++t) {
        MPX_MARK("window");
        const int tile0 = t * kTile;
        if (!PRESTAGED || t > 0) {
            stage_samples_async(g, tile0, kTile, xbuf_byte, lane);
            staged_wait<0>();
        }
        const int hi = min(g.len, tile0 + kTile);
        // the window type is per frame (wave-uniform): one loop per type, not a select per sample
        if (wtype == 0) {
            for (int k = tile0 + lane; k < hi; k += 64)
                xbuf[k - tile0] *= half_window(k, g.L, g.LR, g.kadd, g.invL, g.invR, 0);
        } else {
            for (int k = tile0 + lane; k < hi; k += 64)
                xbuf[k - tile0] *= half_window(k, g.L, g.LR, g.kadd, g.invL, g.invR, 1);
        }
        wave_sync();
        MPX_MARK("gather");
        // Gather y[n] = x[(n + rot) mod N]: lane l, row j <-> n = 128 j + 2 l (real part), + 1 (imaginary part).  Rows that
        // hold no sample of the frame are skipped (wave-uniform: n < len - rot is the frame's right half, n >= N - rot its
        // left half); inside an active row every lane reads -- clamped address, no exec-masked branch, so all reads of the
        // row batch are in flight together instead of one LDS round trip per element -- and keeps the value only where its
        // sample index falls into the tile.  (Round 6: the branchy form was ~5 SALU + a serialised s_waitcnt per element, and
        // its 32 hoisted row masks were 64 SGPRs of the pair kernels' spills.)
        {
            int n_lo = g.len - g.rot, n_hi = N - g.rot;
            asm volatile("" : "+s"(n_lo), "+s"(n_hi));   // evaluated here, per tile: not hoisted as 32 lane masks
            const unsigned span = (unsigned)(hi - tile0);
            const unsigned b0 = (unsigned)(2 * lane + g.rot) - (unsigned)tile0;
#pragma unroll
            for (int j = 0; j < P; ++j) {
                constexpr int LBJ = ilog2(P);
                const int m0 = 128 * j;
                if (MPX_NOISE_ROW_ACTIVE(m0, n_lo, n_hi)) {
                    const int rj = (COMPACT && MPX_COMP_DIT) ? brev(j, LBJ) : j;   // the DIT form wants register brev(j) <- z[l + 64 j]
                    // sample index relative to the tile, modulo N (tile0 is a multiple of the tile length, which divides N)
                    const unsigned d0 = (b0 + (unsigned)m0) & (unsigned)(N - 1), d1 = (d0 + 1u) & (unsigned)(N - 1);
                    const float v0 = xbuf[min(d0, (unsigned)(kTile - 1))], v1 = xbuf[min(d1, (unsigned)(kTile - 1))];
                    re[rj] = (d0 < span) ? v0 : re[rj];
                    im[rj] = (d1 < span) ? v1 : im[rj];
                }
            }
        }
        wave_sync();
    }
    mpx_pin(re), mpx_pin(im);
    hook.gathered(re, im, std::false_type());
    MPX_MARK("fft_forward");
    if constexpr (COMPACT) {   // (lc, ls) = W_128^lane from the pad of the lane's table row (k_synth_comp_pair keeps them there)
        const float4 pk = tw_half_pad<P>(tw, lane);
#if MPX_COMP_DIT
        wave_fft_dit_compact<P, -1>(re, im, tw, xbuf, lane, pk.z, pk.w);   // output: register i <-> Z[lane + 64 i]
        hook.exchanged();
#else
        wave_fft_front_compact<P, -1>(re, im, tw, xbuf, lane, pk.z, pk.w);
        hook.exchanged();
        fft_inreg<P, -1>(re, im);
#endif
        (void)lc;
        (void)ls;
    } else {
        wave_fft_front<P, -1>(re, im, tw, xbuf, lane);
        hook.exchanged();
        fft_inreg<P, -1>(re, im);
    }
}

// Spectrum of the windowed noise frame in PAIRED layout: lane l (kappa = kappa(l)) gets, for q < P/2, its own bin
// k = kappa + 64 q (no_*) and the mirrored bin M - k (nm_*) from ONE evaluation of the real-FFT split's E / T terms
// (X[k] = E + T, X[M-k] = conj(E - T)): P lane exchanges and P/2 split evaluations per lane instead of 2P and P of the
// per-bin form.  The kappa == 0 lane's q == 0 pair is (DC, Nyquist); bin M/2 is its own mirror and comes out separately
// (nh_*, meaningful on the kappa == 0 lane).
template <int P, bool PRESTAGED = false, bool COMPACT = false, int NW = 0, typename Hook = NoiseFftNoHook>   // NW, narrow: support class; hook: see noise_fft
__device__ __forceinline__ void noise_spectrum_paired(const FrameGeom& g, int wtype, const float* tw, float* xbuf,
                                                      unsigned xbuf_byte, int lane, float wl_c, float wl_s,
                                                      float (&no_r)[P / 2], float (&no_i)[P / 2], float (&nm_r)[P / 2],
                                                      float (&nm_i)[P / 2], float& nh_r, float& nh_i, float lc = 1.0f,
                                                      float ls = 0.0f, bool narrow = false, Hook hook = Hook()) {
    constexpr int LB = ilog2(P);
    float re[P], im[P];
    noise_fft<P, PRESTAGED, COMPACT, NW>(g, wtype, tw, xbuf, xbuf_byte, lane, re, im, lc, ls, narrow, hook);
    mpx_pin(re), mpx_pin(im);
    MPX_MARK("split");
    if constexpr (COMPACT) {   // the split twiddle W_N^kappa from the table row's pad: not live across the transform
        const float4 pk = tw_half_pad<P>(tw, lane);
        wl_c = pk.x;
        wl_s = pk.y;
    }
    const int kap = kappa<P>(lane);
    const int src_lane = kappa<P>((64 - kap) & 63);
    const bool lane0 = (kap == 0);
    // partner bins SB at a time: 2 SB lane exchanges in flight together.  All P/2 at once (8 waves per CU) keeps 64 inputs +
    // 32 partners + the growing outputs live; in batches the own (even) and the source (odd) registers of a batch die as
    // its four outputs per bin pair appear -- what the 12-wave form (<= 168 VGPRs) needs.
#ifndef MPX_NOISE_SPLIT_BATCH
#define MPX_NOISE_SPLIT_BATCH (MPX_COMP_PAIR_WAVES > 8 ? 8 : 16)
#endif
    constexpr int SB = (P / 2 < MPX_NOISE_SPLIT_BATCH) ? P / 2 : MPX_NOISE_SPLIT_BATCH;
#pragma unroll
    for (int qb = 0; qb < P / 2; qb += SB) {
        float zpr[SB], zpi[SB];
        // register of row q: brev(q) after the DIF transform, q itself after the DIT one (compact form with MPX_COMP_DIT)
        constexpr bool NATR = COMPACT && MPX_COMP_DIT;
#pragma unroll
        for (int u = 0; u < SB; ++u) {
            const int i = NATR ? qb + u : brev(qb + u, LB);
            zpr[u] = __shfl(re[P - 1 - i], src_lane);
            zpi[u] = __shfl(im[P - 1 - i], src_lane);
        }
#pragma unroll
        for (int u = 0; u < SB; ++u) {
            const int q = qb + u;
            const int i = NATR ? q : brev(q, LB);
            const int i0 = NATR ? (P - q) % P : brev((P - q) % P, LB);
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
    constexpr int ih = (COMPACT && MPX_COMP_DIT) ? P / 2 : 1;   // bin M/2 = register brev(P/2) = 1 (DIF) / P/2 (DIT) of the kappa == 0 lane
    nh_r = re[ih];   // X = conj Z
    nh_i = -im[ih];
}

template <int P, bool PRESTAGED = false, bool COMPACT = false>   // PRESTAGED: the caller already copied tile 0 into xbuf and waited for it
__device__ __forceinline__ void noise_spectrum(const FrameGeom& g, int wtype, const float* tw, float* xbuf,
                                               unsigned xbuf_byte, int lane, float wl_c, float wl_s,
                                               float (&nr)[P], float (&ni)[P], float& nM, float lc = 1.0f, float ls = 0.0f) {
    constexpr int LB = ilog2(P);
    float re[P], im[P];
    noise_fft<P, PRESTAGED, COMPACT>(g, wtype, tw, xbuf, xbuf_byte, lane, re, im, lc, ls);
    if constexpr (COMPACT) {
        const float4 pk = tw_half_pad<P>(tw, lane);
        wl_c = pk.x;
        wl_s = pk.y;
    }
    // real-FFT split for every own bin (redundant form: each lane evaluates X[k] for all its bins)
    const int kap = kappa<P>(lane);
    const int src_lane = kappa<P>((64 - kap) & 63);
    const bool lane0 = (kap == 0);
    // partner fetches in batches of 8 bins: 16 lane exchanges in flight per LDS latency instead of one
#pragma unroll
    for (int ib = 0; ib < P; ib += 8) {
        float prb[8], pib[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            prb[u] = __shfl(re[P - 1 - (ib + u)], src_lane);
            pib[u] = __shfl(im[P - 1 - (ib + u)], src_lane);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = ib + u;
            constexpr bool NATR = COMPACT && MPX_COMP_DIT;   // register i holds row q = i (DIT) / brev(i) (DIF)
            const int q = NATR ? i : brev(i, LB);
            const int i0 = NATR ? (P - q) % P : brev((P - q) % P, LB);
            const float pr = lane0 ? re[i0] : prb[u];
            const float pi = lane0 ? im[i0] : pib[u];
            const float er = 0.5f * (re[i] + pr), ei = 0.5f * (im[i] - pi);
            const float orr = 0.5f * (im[i] + pi), oi = -0.5f * (re[i] - pr);
            const float cq = cos2p<P>(q), sq = -sin2p<P>(q);
            const float wr = wl_c * cq - wl_s * sq, wi = wl_c * sq + wl_s * cq;
            nr[q] = er + (wr * orr - wi * oi);
            ni[q] = ei + (wr * oi + wi * orr);
        }
    }
    nM = re[0] - im[0];   // Nyquist bin X[M] = Re Z[0] - Im Z[0] (meaningful on the kappa == 0 lane)
}

// floats per frame of the stored noise spectra (N = 4096): 17 slots x 64 lanes x float4
constexpr int kSpecFrameFloats = 17 * 64 * 4;
typedef float spec_f32x4 __attribute__((ext_vector_type(4)));

template <int P>
__global__ __launch_bounds__(kAnaThreads) void k_noise_stats(const float* __restrict__ noise,
                                                          const long long* __restrict__ npos,
                                                          const int* __restrict__ nleft,
                                                          const int* __restrict__ nright,
                                                          const int* __restrict__ wtype, long long nframes,
                                                          const float* __restrict__ tw_g,
                                                          float* __restrict__ out_sum,
                                                          float* __restrict__ spec_out) {
    constexpr int M = 64 * P, N = 2 * M;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* tw = smem;
    const int lane_id = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    float* xbuf = smem + tw_floats<P>() + wave * (P * kXStride);
    const unsigned xbuf_byte = 4u * (unsigned)(tw_floats<P>() + rfl(wave) * (P * kXStride));
    for (int i = threadIdx.x; i < tw_floats<P>(); i += kAnaThreads) tw[i] = tw_g[i];
    unsigned* queue = reinterpret_cast<unsigned*>(smem + tw_floats<P>() + kAnaWaves * (P * kXStride));
    if (threadIdx.x == 0) *queue = 0u;
    __syncthreads();
    float wl_s0, wl_c0;
    sincospif(-2.0f * (float)kappa<P>(lane_id) / (float)N, &wl_s0, &wl_c0);
    // compute-only kernel (one float out per frame): 12 waves per CU like k_analysis (3 per SIMD); the workgroup's frames
    // are pulled from its LDS queue (queue_pull, mpx_common.hpp: a SIMD serves its waves by age)
    long long fb, fe;
    block_frame_range(nframes, fb, fe);
    for (long long f = queue_pull(queue, fb); f < fe; f = queue_pull(queue, fb)) {
        int lane = lane_id;
        float wl_s = wl_s0, wl_c = wl_c0;
        asm volatile("" : "+v"(lane), "+v"(wl_s), "+v"(wl_c));
        const FrameGeom g = frame_geom(noise, npos[f], nleft[f], nright[f], N);
        float no_r[P / 2], no_i[P / 2], nm_r[P / 2], nm_i[P / 2], nh_r, nh_i;
        noise_spectrum_paired<P>(g, wtype[f], tw, xbuf, xbuf_byte, lane, wl_c, wl_s, no_r, no_i, nm_r, nm_i, nh_r, nh_i);
        if constexpr (P == 32) {
            // "noise spectra once" form (mpx_noise_stats_spectra): the frame's paired spectrum goes to HBM as the registers
            // hold it -- 17 slots of 64 lanes x float4 (no_r, no_i, nm_r, nm_i four rows at a time, then the bin-M/2 pair),
            // 1 KB per wave store -- and k_synth_comp_pair<.., SPEC> loads it back instead of transforming the frame again
            if (spec_out) {
                spec_f32x4* d = reinterpret_cast<spec_f32x4*>(spec_out + f * (long long)kSpecFrameFloats) + lane_id;
#pragma unroll
                for (int s_ = 0; s_ < 4; ++s_) {
                    __builtin_nontemporal_store(spec_f32x4{no_r[4 * s_], no_r[4 * s_ + 1], no_r[4 * s_ + 2], no_r[4 * s_ + 3]}, d + 64 * s_);
                    __builtin_nontemporal_store(spec_f32x4{no_i[4 * s_], no_i[4 * s_ + 1], no_i[4 * s_ + 2], no_i[4 * s_ + 3]}, d + 64 * (4 + s_));
                    __builtin_nontemporal_store(spec_f32x4{nm_r[4 * s_], nm_r[4 * s_ + 1], nm_r[4 * s_ + 2], nm_r[4 * s_ + 3]}, d + 64 * (8 + s_));
                    __builtin_nontemporal_store(spec_f32x4{nm_i[4 * s_], nm_i[4 * s_ + 1], nm_i[4 * s_ + 2], nm_i[4 * s_ + 3]}, d + 64 * (12 + s_));
                }
                __builtin_nontemporal_store(spec_f32x4{nh_r, nh_i, 0.0f, 0.0f}, d + 64 * 16);
            }
        }
        // sum over bins 1..M-1 of (ln|Ns|)^2 = (0.5 ln |Ns|^2)^2 ; |Ns| == 0 -> protected log MAGIC = -1e10 (libaudio.py:241-248)
        // paired layout: own bin + mirror per step; the kappa == 0 lane's first pair is (DC, Nyquist), both excluded, and
        // that lane adds bin M/2
        const bool lane0 = (kappa<P>(lane) == 0);
        // |Ns|^2 of every bin first; the logarithm is the hardware log2 as it is (3 instructions per bin) when no bin of the
        // frame is zero or a denormal -- always, in practice -- and __logf with its rescaling sequence otherwise (one
        // wave-uniform branch per frame instead of a select per bin)
        float so[P / 2], sm[P / 2];
        const float sh = nh_r * nh_r + nh_i * nh_i;
        float smin = lane0 ? sh : 1.0f;
#pragma unroll
        for (int q = 0; q < P / 2; ++q) {
            so[q] = no_r[q] * no_r[q] + no_i[q] * no_i[q];
            sm[q] = nm_r[q] * nm_r[q] + nm_i[q] * nm_i[q];
            smin = fminf(smin, fminf(so[q], sm[q]));
        }
        float acc;
        if (!__any(smin < 1.1754944e-38f)) {
            auto term = [](float s_) {
                const float lg = 0.34657359027997264f * __builtin_amdgcn_logf(s_);   // 0.5 ln 2 log2(s)
                return lg * lg;
            };
            acc = lane0 ? term(sh) : 0.0f;
#pragma unroll
            for (int q = 0; q < P / 2; ++q) {
                const float tq = term(so[q]) + term(sm[q]);
                acc += (q == 0 && lane0) ? 0.0f : tq;
            }
        } else {
            auto term = [](float s_) {
                const float lg = (s_ > 0.0f) ? 0.5f * __logf(s_) : -1.0e10f;
                return lg * lg;
            };
            acc = lane0 ? term(sh) : 0.0f;
#pragma unroll
            for (int q = 0; q < P / 2; ++q) {
                const float tq = term(so[q]) + term(sm[q]);
                acc += (q == 0 && lane0) ? 0.0f : tq;
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
        if (lane_id == 0) out_sum[f] = acc;
    }
}

// ---------------------------------------------------------------------------------------------
// noise gains (magphase.py:902-906, Q10): per utterance and class (voiced / unvoiced)
//   g = sqrt(exp(mean over the class's frames and bins 1..N/2-1 of (ln|Ns|)^2)),  inv_gain[f] = 1 / g(class of f)
// from the per-frame sums of k_noise_stats.  One block per utterance, float64 accumulation; an empty class gives
// NaN exactly like np.mean of an empty selection (it is never applied to a frame).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_noise_gains(const float* __restrict__ sums, const int* __restrict__ voiced,
                                                     const int* __restrict__ utt_frame_off, int bins_per_frame,
                                                     float* __restrict__ inv_gain, double* __restrict__ gains) {
    __shared__ double s_sum[2][256];
    __shared__ int s_cnt[2][256];
    const int u = blockIdx.x;
    const int f0 = utt_frame_off[u], f1 = utt_frame_off[u + 1];
    double acc[2] = {0.0, 0.0};
    int cnt[2] = {0, 0};
    for (int f = f0 + threadIdx.x; f < f1; f += 256) {
        const int c = voiced[f] ? 0 : 1;
        acc[c] += (double)sums[f];
        cnt[c] += 1;
    }
    for (int c = 0; c < 2; ++c) {
        s_sum[c][threadIdx.x] = acc[c];
        s_cnt[c][threadIdx.x] = cnt[c];
    }
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
        if (threadIdx.x < off) {
            for (int c = 0; c < 2; ++c) {
                s_sum[c][threadIdx.x] += s_sum[c][threadIdx.x + off];
                s_cnt[c][threadIdx.x] += s_cnt[c][threadIdx.x + off];
            }
        }
        __syncthreads();
    }
    double g[2];
    for (int c = 0; c < 2; ++c)
        g[c] = (s_cnt[c][0] > 0) ? sqrt(exp(s_sum[c][0] / ((double)s_cnt[c][0] * (double)bins_per_frame))) : nan("");
    if (threadIdx.x == 0 && gains) {
        gains[2 * u + 0] = g[0];
        gains[2 * u + 1] = g[1];
    }
    for (int f = f0 + threadIdx.x; f < f1; f += 256) inv_gain[f] = (float)(1.0 / g[voiced[f] ? 0 : 1]);
}

// ---------------------------------------------------------------------------------------------
// minimum-phase spectrum from a magnitude spectrum (complex cepstrum), la.build_min_phase_from_mag_spec
// (libaudio.py:920-934): ln|X| -> even extension -> real IFFT (cepstrum c) -> causal fold (c[1..N/2-1] *= 2,
// c[N/2+1..] = 0) -> FFT -> exp.  Since Re FFT(fold c) == ln|X|, only the phase phi = Im FFT(fold c) is new: the
// kernel writes the unit phasor (cos phi, sin phi) where the synthesis kernel expects the (real, imag) phase
// features, and the (row-interpolated) magnitude it was computed from.  One wavefront per frame, two FFTs.
// ---------------------------------------------------------------------------------------------
template <int P>
__global__ __launch_bounds__(kThreads) void k_min_phase(const float* __restrict__ mag, const int* __restrict__ row0,
                                                        const int* __restrict__ row1,
                                                        const float* __restrict__ rowt, long long nframes,
                                                        const float* __restrict__ tw_g, float* __restrict__ omag,
                                                        float* __restrict__ oreal, float* __restrict__ oimag,
                                                        long long ld) {
    constexpr int M = 64 * P, N = 2 * M, H = M + 1, LB = ilog2(P);
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* tw = smem;
    const int lane_id = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    float* xbuf = smem + tw_floats<P>() + wave * (P * kXStride);
    for (int i = threadIdx.x; i < tw_floats<P>(); i += kThreads) tw[i] = tw_g[i];
    __syncthreads();
    float wa_s0, wa_c0, ws_s0, ws_c0;
    sincospif(-2.0f * (float)kappa<P>(lane_id) / (float)N, &wa_s0, &wa_c0);
    sincospif(2.0f * (float)lane_id / (float)N, &ws_s0, &ws_c0);
    const int wave_u = rfl(wave);
    for (long long f = (long long)blockIdx.x * kWavesPerBlock + wave_u; f < nframes;
         f += (long long)gridDim.x * kWavesPerBlock) {
        int lane = lane_id;
        float wa_s = wa_s0, wa_c = wa_c0, ws_s = ws_s0, ws_c = ws_c0;
        asm volatile("" : "+v"(lane), "+v"(wa_s), "+v"(wa_c), "+v"(ws_s), "+v"(ws_c));
        const int r0 = row0[f], r1 = row1[f];
        const float rt = rowt[f];
        const float* m0p = mag + (long long)r0 * ld;
        const float* m1p = mag + (long long)r1 * ld;
        // ---- ln|X| (protected log, libaudio.py:241-248) on bins lane + 64 j, scaled for the inverse transform
        float xr[P], xi[P], mv[P];
        const float scale = 0.5f / (float)M;
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const float a = m0p[lane + 64 * j], b = m1p[lane + 64 * j];
            mv[j] = fmaf(b - a, rt, a);
        }
        float mM = 0.0f;
        if (lane == 0) {
            const float a = m0p[M], b = m1p[M];
            mM = fmaf(b - a, rt, a);
        }
#pragma unroll
        for (int j = 0; j < P; ++j) {
            xr[j] = ((mv[j] > 0.0f) ? logf(mv[j]) : -1.0e10f) * scale;
            xi[j] = 0.0f;
        }
        const float xm = ((mM > 0.0f) ? logf(mM) : -1.0e10f) * scale;
        hermitian_merge<P>(xr, xi, xm, lane, ws_c, ws_s);
        wave_fft<P, +1>(xr, xi, tw, xbuf, lane);
        // ---- cepstrum samples n = 2m, 2m+1 with m = kappa + 64 brev(i): causal fold
        const int kap = kappa<P>(lane);
#pragma unroll
        for (int i = 0; i < P; ++i) {
            const int n0 = 2 * (kap + 64 * brev(i, LB));
            const float w0 = (n0 == 0) ? 1.0f : ((n0 < M) ? 2.0f : ((n0 == M) ? 1.0f : 0.0f));
            const float w1 = (n0 + 1 < M) ? 2.0f : ((n0 + 1 == M) ? 1.0f : 0.0f);
            xr[i] *= w0;
            xi[i] *= w1;
        }
        // ---- forward real FFT of the folded cepstrum: input register j must hold z[lane + 64 j]
        float re[P], im[P];
#pragma unroll
        for (int i = 0; i < P; ++i) {
            re[brev(i, LB)] = xr[i];
            im[brev(i, LB)] = xi[i];
        }
        if (P != 32) {
            const int src = kappa<P>(lane);
#pragma unroll
            for (int j = 0; j < P; ++j) {
                re[j] = __shfl(re[j], src);
                im[j] = __shfl(im[j], src);
            }
        }
        wave_fft<P, -1>(re, im, tw, xbuf, lane);
        const int src_lane = kappa<P>((64 - kap) & 63);
        const bool lane0 = (kap == 0);
        float* mo = omag + f * ld;
        float* ro = oreal + f * ld;
        float* io = oimag + f * ld;
        // the magnitude row is stored from the lanes that loaded it (bins lane + 64 j)
#pragma unroll
        for (int j = 0; j < P; ++j) mo[lane + 64 * j] = mv[j];
        if (lane == 0) mo[M] = mM;
        // partner fetches in batches of 8 bins (16 lane exchanges in flight per LDS latency instead of one); phase ->
        // unit phasor with the hardware sin / cos (|error| ~ 5e-7, the phase itself carries ~1e-6 of fp32 FFT noise)
#pragma unroll
        for (int ib = 0; ib < P; ib += 8) {
            float prb[8], pib[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                prb[u] = __shfl(re[P - 1 - (ib + u)], src_lane);
                pib[u] = __shfl(im[P - 1 - (ib + u)], src_lane);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = ib + u;
                const int q = brev(i, LB);
                const int i0 = brev((P - q) % P, LB);
                const float pr = lane0 ? re[i0] : prb[u];
                const float pi = lane0 ? im[i0] : pib[u];
                const float ei = 0.5f * (im[i] - pi);
                const float orr = 0.5f * (im[i] + pi), oi = -0.5f * (re[i] - pr);
                const float cq = cos2p<P>(q), sq = -sin2p<P>(q);
                const float wr = wa_c * cq - wa_s * sq, wi = wa_c * sq + wa_s * cq;
                const float phi = ei + (wr * oi + wi * orr);   // Im S[k]
                float sn, cs;
                __sincosf(phi, &sn, &cs);
                const int k = kap + 64 * q;
                ro[k] = cs;
                io[k] = sn;
            }
        }
        if (lane0) {   // Nyquist bin of a real sequence: phase 0
            ro[M] = 1.0f;
            io[M] = 0.0f;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// compressed synthesis + PSOLA
// ---------------------------------------------------------------------------------------------
struct CompFrameTabs {
    const long long* npos;   // noise frame epoch (absolute index into the noise buffer)
    const int* nleft;
    const int* nright;
    const int* wtype;        // 0 hann / 1 bartlett^2.5
    const int* voiced;       // 0 / 1
    const float* inv_gain;   // 1 / noise gain of the frame's class (Q10)
    const int* row0;         // feature rows to interpolate between (constant -> variable rate), row0 == row1 if none
    const int* row1;
    const float* rowt;       // interpolation weight of row1
    const int* win_l;        // anti-ringing window half lengths (Q14)
    const int* win_r;
    const int* pm_rel;
    const float* nspec;      // SPEC form: the frames' noise spectra as k_noise_stats stored them (else unused)
};

// ---------------------------------------------------------------------------------------------
// Compressed-feature synthesis + PSOLA, pair form: two waves share one LDS ring and alternate over the frames of the
// pair's runs (tickets in LDS, exactly as k_synth_ola_pair).  Round 3: 12 waves per CU (three per SIMD, <= 168 VGPRs)
// instead of 8 -- the kernel is parked in s_waitcnt a third of its wave cycles and moves 1 TB/s, a third wave per SIMD
// fills those gaps: synthesis side of configs[2] 1.350 -> 1.25 ms (interleaved A/B), 0.727 -> 0.632 ms for the launch.
// What made it fit: the compact transform front (half-height exchange buffer, noise staged in tiles of 1024 samples:
// frames longer than that -- f0 below 94 Hz at 48 kHz -- take a second, synchronous tile; half twiddle table), the lane
// constants of the split / merge / compact twiddles kept in the PAD of the lane's table row and read where they are used
// (tw_half_pad: six registers that are not live across the frame loop), the feature loads in the form SGPR row pointer +
// one zero-extended 32-bit lane offset (the int-indexed form made a 64-bit address per load: 208 v_lshl_add_u64 and as
// many register pairs in the ISA), the overlap-add 16 ring values at a time (ring_add_plane), and -- what finally removed
// the spills -- the assembly's load batches sized by what a row can need (template parameter NPQ below): with room for 10
// values per bin pair on every row, batches of 1 / 2 / 4 pairs spilled 0 / 6-18 / 17 registers at 1.448 / 1.273 / 1.253
// ms (the loads in flight are what the kernel lives on), and the spilled registers' scratch lines, evicted from L2 by the
// feature stream, cost 176-340 MB of HBM traffic per launch.  The feature rows -- read once, by one wave -- are loaded
// non-temporally.  The single-wave form it replaced (git
// history) held both feature rows, the per-bin curves and the noise FFT at once (466 VGPRs, ONE wave per SIMD: at one
// instruction per ~5.4 cycles and wave its ~7.5 k instructions per frame were the whole 1.35 ms).  Here the noise spectrum is
// computed first and the features are folded into it in place, half a spectrum (16 register rows) at a time:
// 64 + 128 live registers instead of 64 + 262, so two waves fit a SIMD.
// ---------------------------------------------------------------------------------------------
constexpr int kCompPairWaves = MPX_COMP_PAIR_WAVES;
constexpr int kCompPairs = kCompPairWaves / 2;
// More than 8 waves per CU: P == 32 does not fit the LDS with full-height exchange buffers (6 rings + 12 buffers + the
// table = 223 KB) -- the compact transform front of wave_fft.hpp (half-height buffers, noise staged in tiles of 1024
// samples, half twiddle table): 162.9 KB, as k_synth_ola_pair.
template <int P>
constexpr bool comp_compact() { return P == 32 && kCompPairWaves > 8; }
template <int P>
constexpr int comp_tw_floats() { return comp_compact<P>() ? tw_half_floats<P>() : tw_floats<P>(); }
template <int P>
constexpr int comp_xbuf_floats() { return (comp_compact<P>() ? P / 2 : P) * kXStride; }
template <int P>
constexpr size_t lds_bytes_comp_pair() {
    return sizeof(float) * (size_t)(comp_tw_floats<P>() + kCompPairWaves * comp_xbuf_floats<P>() + kCompPairs * ring_len<P>() + 16);
}

// ---------------------------------------------------------------------------------------------
// Frame stages shared by the three pair kernels below (k_synth_comp_pair, k_roundtrip_pair, k_griffin_lim_pair).  Each
// kernel is: pair_wave_setup, then per frame pair_frame_lane, its own way to a spectrum Z in registers (the two that
// analyse a staged frame start from pair_analysis_spectrum), pair_inverse_fft_front, the start of the next frame's copy,
// pair_inverse_fft_back, pair_ordered_ola.
// ---------------------------------------------------------------------------------------------
// What a wave of a pair kernel knows before its first frame.  LDS: twiddle table | one exchange buffer per wave | one ring
// per pair | the pairs' tickets.
struct PairWave {
    float *tw, *xbuf, *ring;
    int* turn;                            // the pair's ticket: index of the frame whose overlap-add is due
    unsigned xbuf_byte, ring_byte;        // LDS byte addresses of xbuf and ring
    int lane_id, half, wi_end;            // half: which of the pair's two waves; wi_end: end of the pair's work list
    float wa_s0, wa_c0, ws_s0, ws_c0;     // analysis-side lane twiddle W_N^kappa and synthesis-side conj(W_N^lane)
    PairCursor cur;                       // at the wave's first frame
};

// Fills w; false when the wave has no slot or no frame.  Contains the prologue's __syncthreads(): every wave of the
// workgroup must reach this call before any returns.
template <int P>
__device__ __forceinline__ bool pair_wave_setup(PairWave& w, float* smem, const float* __restrict__ tw_g,
                                                const RunDesc* __restrict__ runs, const int* __restrict__ slot_off,
                                                const int* __restrict__ slot_runs, int nslots) {
    constexpr int N = 128 * P, R = ring_len<P>();
    const int wave = rfl((int)(threadIdx.x >> 6));
    const int pair = wave >> 1;
    constexpr int kRing0 = comp_tw_floats<P>() + kCompPairWaves * comp_xbuf_floats<P>();
    static_assert(kCompPairs <= 16, "the tickets fit the 16 floats behind the rings");
    w.tw = smem;
    w.lane_id = threadIdx.x & 63;
    w.half = wave & 1;
    w.xbuf = smem + comp_tw_floats<P>() + wave * comp_xbuf_floats<P>();
    w.xbuf_byte = 4u * (unsigned)(comp_tw_floats<P>() + wave * comp_xbuf_floats<P>());
    w.ring = smem + kRing0 + pair * R;
    w.ring_byte = 4u * (unsigned)(kRing0 + pair * R);
    w.turn = reinterpret_cast<int*>(smem + kRing0 + kCompPairs * R) + pair;
    pair_kernel_prologue<P, comp_compact<P>(), MPX_COMP_DIT != 0>(w.tw, tw_g, smem + kRing0, kCompPairs * R, w.turn - pair,
                                                                  kCompPairs, kCompPairWaves * 64);
    // (compact form: these constants live in the pad of the lane's table row and are read where they are used -- six
    // registers that are not live across the frame loop)
    sincospif(-2.0f * (float)kappa<P>(w.lane_id) / (float)N, &w.wa_s0, &w.wa_c0);
    sincospif(2.0f * (float)w.lane_id / (float)N, &w.ws_s0, &w.ws_c0);
    const int slot = blockIdx.x * kCompPairs + pair;
    if (slot >= nslots) return false;
    // cursor over this wave's frames: every second frame of every run of the pair's work list (see k_synth_ola_pair)
    w.wi_end = slot_off[slot + 1];
    w.cur.wi = slot_off[slot];
    w.cur.ticket_base = 0;
    pair_cursor_settle(w.cur, w.wi_end, w.half, runs, slot_runs);
    return w.cur.valid != 0;
}

// A frame's samples are copied HBM -> LDS (into the exchange buffer) while the previous frame's inverse FFT finishes and
// its overlap-add runs (same scheme as k_analysis): the first tile of frame g.
template <int P>
__device__ __forceinline__ void pair_stage_frame(const PairWave& w, const FrameGeom& g, int lane) {
    stage_samples_async(g, 0, comp_compact<P>() ? 32 * P : 64 * P, w.xbuf_byte, lane);
}
// ... of a later frame, once the wave's own reads of the exchange buffer have returned
template <int P>
__device__ __forceinline__ void pair_stage_next(const PairWave& w, const FrameGeom& g, int lane) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    pair_stage_frame<P>(w, g, lane);
}

// The lane index and the lane twiddles as this frame sees them, laundered once per frame: call it INSIDE the frame loop
// (hoisted out of it, what the compiler derives from them stays live across the loop).
template <int P>
__device__ __forceinline__ void pair_frame_lane(const PairWave& w, int& lane, float& wa_s, float& wa_c, float& ws_s,
                                                float& ws_c) {
    lane = w.lane_id;
    wa_s = 0.0f, wa_c = 1.0f, ws_s = 0.0f, ws_c = 1.0f;
    if constexpr (comp_compact<P>()) {
        asm volatile("" : "+v"(lane));
    } else {
        wa_s = w.wa_s0, wa_c = w.wa_c0, ws_s = w.ws_s0, ws_c = w.ws_c0;
        asm volatile("" : "+v"(lane), "+v"(wa_s), "+v"(wa_c), "+v"(ws_s), "+v"(ws_c));
    }
}

// Analysis of the staged frame g (Hann halves): X[k] of the own bins k = lane + 64 q (no_*) and of their mirrors M - k
// (nm_*), bin M/2 on lane 0 (nh_*).  NW, narrow: the frame's support class (noise_fft).
template <int P, int NW = 0, typename Hook = NoiseFftNoHook>
__device__ __forceinline__ void pair_analysis_spectrum(const PairWave& w, const FrameGeom& g, int lane, float wa_c,
                                                       float wa_s, float (&no_r)[P / 2], float (&no_i)[P / 2],
                                                       float (&nm_r)[P / 2], float (&nm_i)[P / 2], float& nh_r, float& nh_i,
                                                       bool narrow = false, Hook hook = Hook()) {
    constexpr bool kCompact = comp_compact<P>();
    MPX_MARK("frame_setup");
    staged_wait<0>();
    noise_spectrum_paired<P, true, kCompact, NW>(g, 0, w.tw, w.xbuf, w.xbuf_byte, lane, wa_c, wa_s, no_r, no_i, nm_r, nm_i,
                                                 nh_r, nh_i, 1.0f, 0.0f, narrow, hook);
    if (P != 32) {   // FFT output lanes hold bins kappa(lane) + 64 q; the rows and the merge want bins lane + 64 q
        const int src = kappa<P>(lane);
#pragma unroll
        for (int q = 0; q < P / 2; ++q) {
            no_r[q] = __shfl(no_r[q], src);
            no_i[q] = __shfl(no_i[q], src);
            nm_r[q] = __shfl(nm_r[q], src);
            nm_i[q] = __shfl(nm_i[q], src);
        }
        nh_r = __shfl(nh_r, src);
        nh_i = __shfl(nh_i, src);
    }
    mpx_pin(no_r), mpx_pin(no_i), mpx_pin(nm_r), mpx_pin(nm_i);
}

// Inverse transform of the merged spectrum, in place, in two halves.  The exchange buffer is idle once the front is
// through: between the halves the kernel starts the copy of the next frame's samples (pair_stage_next).
template <int P>
__device__ __forceinline__ void pair_inverse_fft_front(const PairWave& w, float (&xr)[P], float (&xi)[P], int lane) {
    constexpr bool kCompact = comp_compact<P>(), kDit = kCompact && MPX_COMP_DIT;
    mpx_pin(xr), mpx_pin(xi);
    MPX_MARK("fft_inverse");
    if constexpr (kDit) {
        // DIT form: its input wants register brev(j) <- bin lane + 64 j, its output is register i <-> samples 2 n, 2 n + 1
        // with n = lane + 64 i: static renamings on both sides
        constexpr int LBJ = ilog2(P);
        float yr[P], yi[P];
#pragma unroll
        for (int j = 0; j < P; ++j) {
            yr[brev(j, LBJ)] = xr[j];
            yi[brev(j, LBJ)] = xi[j];
        }
        const float4 pk = tw_half_pad<P>(w.tw, lane);
        wave_fft_dit_compact_front<P, +1>(yr, yi, w.tw, w.xbuf, lane, pk.z, pk.w);
#pragma unroll
        for (int j = 0; j < P; ++j) {
            xr[j] = yr[j];
            xi[j] = yi[j];
        }
    } else if constexpr (kCompact) {
        const float4 pk = tw_half_pad<P>(w.tw, lane);
        wave_fft_front_compact<P, +1>(xr, xi, w.tw, w.xbuf, lane, pk.z, pk.w);
    } else {
        wave_fft_front<P, +1>(xr, xi, w.tw, w.xbuf, lane);
    }
}
template <int P>
__device__ __forceinline__ void pair_inverse_fft_back(float (&xr)[P], float (&xi)[P]) {
    if constexpr (comp_compact<P>() && MPX_COMP_DIT) wave_fft_dit_back<P, +1>(xr, xi);
    else fft_inreg<P, +1>(xr, xi);
}
// The registers of the inverse transform's output (DIF form: register i <-> row brev(i)) that hold the rows
// P/2 - W <= q < P/2 + W of the fftshifted frame (ring_add_plane's ROT: frame row q = output row (q + P/2) mod P).
template <int P>
constexpr unsigned support_out_regs(int W) {
    unsigned o = 0u;
    for (int q = 0; q < P; ++q)
        if (support_row_live(q, W, P)) o |= 1u << brev((q + P / 2) % P, ilog2(P));
    return o;
}
// ... and the transform that forms only those where `narrow` (wave-uniform) holds (DIF form): the last stages, some of whose
// outputs the overlap-add of a class-NW frame does not read, in two instances; the registers it skips keep stale values.
template <int P, int NW>
__device__ __forceinline__ void pair_inverse_fft_back_class(float (&xr)[P], float (&xi)[P], bool narrow) {
    static_assert(!(comp_compact<P>() && MPX_COMP_DIT), "support classes: the DIF form only");
    constexpr unsigned kOut = support_out_regs<P>(NW);
    constexpr int S1 = out_prune_stride<P>(kOut);   // the stages of stride <= S1 have outputs nobody reads
    static_assert(S1 >= 1 && S1 < P / 2, "a class prunes some, not all, stages of the last pass");
    fft_inreg_stages<P, +1, P / 2, 2 * S1>(xr, xi);
    if (narrow) {
        fft_inreg_pruned_stage<P, +1, S1, 0u, kOut>(xr, xi);
        MPX_ARM_END_CLASS();
    } else {
        fft_inreg_stages<P, +1, S1>(xr, xi);
        MPX_ARM_END_FULL();
    }
}

// The ordered section of frame cur.fi: waits for the frame's ticket, streams out of the pair's ring what no later frame
// reaches, adds the frame (xr = samples 2n, xi = samples 2n + 1) at its strip position, and passes the ticket on; the
// last frame of a run streams out the rest and leaves the ring cleared.  combine(old, value, n) / live(q) as ring_add;
// ROT: the rows are taken half a transform apart (the fftshift, see ring_add_plane).
// NW > 0 (k_roundtrip_pair): where `narrow` (wave-uniform) holds, only the rows of support class NW are added -- a second
// straight-line instance of the ring add whose row set is a compile-time constant; xr / xi then hold only those rows.
// NATIN (k_roundtrip_pair's direct arm): xr / xi are not a transform's output but the gathered frame itself, register j <->
// samples 128 j + 2 lane (+ 1) -- natural register order whatever the transforms' form.
template <int P, bool ROT, int NW = 0, bool NATIN = false, typename CFn, typename LFn>
__device__ __forceinline__ void pair_ordered_ola(const PairWave& w, const PairCursor& cur, float* smem,
                                                 const RunDesc* __restrict__ runs, const int* __restrict__ pm_rel,
                                                 float* __restrict__ strips, float* __restrict__ pcm, float (&xr)[P],
                                                 float (&xi)[P], int lane, CFn combine, LFn live, bool narrow = false) {
    constexpr int R = ring_len<P>();
    constexpr bool kDit = comp_compact<P>() && MPX_COMP_DIT;
    constexpr bool kNat = kDit || NATIN;   // natural register order (ring_add_plane's NAT)
    static_assert(NW == 0 || (ROT && !kDit && (kCompPairWaves > 8)), "class row sets: the rotated DIF form only");
    static_assert(!NATIN || (ROT && P == 32), "the gathered frame's lanes are the ring's only where kappa(lane) == lane");
    if constexpr (NW == 0) mpx_pin(xr), mpx_pin(xi);
    MPX_MARK("ticket");
    const int fi = cur.fi;
    int* const turn = w.turn;
    const RunDesc rd = runs[cur.ci];
    float* strip = strips + rd.strip_off;
    float* pcm0 = pcm + rd.out_base;
    const int ticket = cur.ticket_base + (fi - cur.fb);
    const int x = pm_rel[fi] - cur.x0;   // strip position of the frame's first sample
    const int target = x & ~63;
    const int flushed = (fi == cur.fb) ? 0 : ((pm_rel[fi - 1] - cur.x0) & ~63);
    asm volatile("" ::"s"(x), "s"(flushed), "s"(rd.head_end), "s"(rd.out_lo), "s"(rd.out_hi), "s"(rd.flush_end));
    while (__hip_atomic_load(turn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != ticket)
        __builtin_amdgcn_s_sleep(1);
    asm volatile("" ::: "memory");
    MPX_MARK("flush");
    if (flushed < target) flush_ring<R>(w.ring, strip, pcm0, rd.head_end, rd.out_lo, rd.out_hi, flushed, target, lane);
    wave_sync();
    MPX_MARK("overlap_add");
    if constexpr (kCompPairWaves > 8 || ROT) {   // 16 ring values in registers at a time (<= 168 VGPRs)
        constexpr int CH = (P < MPX_COMP_CH) ? P : MPX_COMP_CH;
        const RingAddr ra = ring_addr<P>(w.ring_byte, x, lane);
        if constexpr (NW > 0) {
            if (narrow) {
                constexpr unsigned kOut = NATIN ? ~support_zero_rows<P>(NW) : support_out_regs<P>(NW);
                mpx_pin_live<kOut>(xr), mpx_pin_live<kOut>(xi);
                auto live_nw = [](int q) { return support_row_live(q, NW, P); };
                ring_add_plane<P, 0, CH, kNat, ROT>(smem, ra, xr, lane, combine, live_nw);
                ring_add_plane<P, 1, CH, kNat, ROT>(smem, ra, xi, lane, combine, live_nw);
                MPX_ARM_END_CLASS();
            } else {
                mpx_pin(xr), mpx_pin(xi);
                ring_add_plane<P, 0, CH, kNat, ROT>(smem, ra, xr, lane, combine, live);
                ring_add_plane<P, 1, CH, kNat, ROT>(smem, ra, xi, lane, combine, live);
                MPX_ARM_END_FULL();
            }
        } else {
            ring_add_plane<P, 0, CH, kNat, ROT>(smem, ra, xr, lane, combine, live);
            ring_add_plane<P, 1, CH, kNat, ROT>(smem, ra, xi, lane, combine, live);
        }
    } else {
        ring_add<P>(smem, w.ring_byte, x, xr, xi, lane, combine, live);
    }
    wave_sync();
    if (fi == cur.fe - 1) {   // last frame of the run: stream out the rest, leave the ring cleared
        flush_ring<R>(w.ring, strip, pcm0, rd.head_end, rd.out_lo, rd.out_hi, target, rd.flush_end, lane);
        wave_sync();
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __hip_atomic_store(turn, ticket + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    MPX_MARK("loop_end");
}

// LERP: every frame interpolates between two spectrum rows (row0 / row1 / rowt tables); false: one row per frame, row
// index = frame index (variable-rate input, or rows already interpolated by mpx_mel_unwarp_rows) -- half the feature loads.
// NPQ >= 0 (one-row-per-frame form): the caller's promise n_per <= 64 NPQ at compile time -- only the own bins of the
// register rows q < NPQ can have a periodic component, no mirror bin has (M - k > 64 NPQ).  The assembly then loads 7
// values per bin pair on those rows and 4 on the others instead of keeping room for 10 everywhere: batches of (4, 4, 8)
// pairs = 28 / 28 / 32 loads in flight for P == 32, NPQ == 8 (48 / 44.1 kHz: the crossfade ends at bin 512), against
// four batches of 40 -- the 17 registers the 40-wide batches spilled at 12 waves per CU are gone (166 VGPRs, no scratch),
// and the freed registers allow batches of (8, 8) = 56 / 32 loads: two exposed load latencies per frame instead of four.
// NPQ < 0: anything goes (run-time tests only).
// SPEC: the noise spectra come from HBM (tb.nspec, stored by k_noise_stats) instead of a second transform of the frame.
// T2: the assembly of synthesis_from_compressed_type2 (magphase.py:1556-1567) -- the DC and Nyquist bins keep their signed
// real part with a zero imaginary part (la.add_hermitian_half(.., 'complex')) instead of the modulus.  Everything else
// that differs in type 2 (one gain per utterance, other curves) arrives as data: tb.inv_gain, per_v, ap_v, ap_u.
template <int P, bool LERP, int NPQ = -1, bool SPEC = false, bool T2 = false>
__global__ __launch_bounds__(kCompPairWaves * 64) void k_synth_comp_pair(const float* __restrict__ mag,
                                                                        const float* __restrict__ real,
                                                                        const float* __restrict__ imag,
                                                                        const float* __restrict__ noise,
                                                                        CompFrameTabs tb,
                                                                        const float* __restrict__ per_v,
                                                                        const float* __restrict__ ap_v,
                                                                        const float* __restrict__ ap_u,
                                                                        const RunDesc* __restrict__ runs,
                                                                        const int* __restrict__ slot_off,
                                                                        const int* __restrict__ slot_runs,
                                                                        int nslots,
                                                                        const float* __restrict__ tw_g,
                                                                        float* __restrict__ strips,
                                                                        float* __restrict__ pcm, long long ld, int n_per) {
    static_assert(!SPEC || (P == 32 && !LERP), "stored noise spectra: N = 4096, one row per frame");
    static_assert(!(SPEC && T2), "type 2 has no stored-spectra form");
    constexpr int M = 64 * P, N = 2 * M;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr bool kCompact = comp_compact<P>();
    PairWave w;
    if (!pair_wave_setup<P>(w, smem, tw_g, runs, slot_off, slot_runs, nslots)) return;
    float* const tw = w.tw;
    float* const xbuf = w.xbuf;
    const unsigned xbuf_byte = w.xbuf_byte;
    PairCursor cur = w.cur;

    FrameGeom g = frame_geom(noise, tb.npos[cur.fi], tb.nleft[cur.fi], tb.nright[cur.fi], N);
    if constexpr (!SPEC) pair_stage_frame<P>(w, g, w.lane_id);

    while (cur.valid) {
        int lane;
        float wa_s, wa_c, ws_s, ws_c;
        pair_frame_lane<P>(w, lane, wa_s, wa_c, ws_s, ws_c);
        constexpr float lc = 1.0f, ls = 0.0f;
        PairCursor nxt = cur;
        pair_cursor_advance(nxt, w.wi_end, w.half, runs, slot_runs);
        const int fi = cur.fi;

        float xr[P], xi[P];
        const int voiced = tb.voiced[fi];
        const float ig = tb.inv_gain[fi];
        const float* apc = voiced ? ap_v : ap_u;    // aperiodic curve of the frame's class (uniform select)
        const float pvs = voiced ? 1.0f : 0.0f;     // periodic component only in voiced frames
        const float sgn_scale = ((lane & 1) ? -1.0f : 1.0f) * (0.5f / (float)M);
        if constexpr (!LERP) {
            // ---- aperiodic source in PAIRED layout: own bins k = lane + 64 q and their mirrors M - k, q < P/2 (one
            // evaluation of the split per pair), then the spectrum assembly (Appendix A2 steps 9-12) on the same pairs
            // with the features loaded ascending / descending, and the Hermitian merge without a second round of lane
            // exchanges (merge_paired_complex): against the per-bin form 2P fewer lane exchanges and half the split /
            // merge arithmetic per frame.
            constexpr int HP = P / 2;
            float no_r[HP], no_i[HP], nm_r[HP], nm_i[HP], nh_r, nh_i;
            if constexpr (SPEC) {
                const spec_f32x4* sp = reinterpret_cast<const spec_f32x4*>(tb.nspec + (long long)fi * kSpecFrameFloats) + lane;
                spec_f32x4 v[16];
#pragma unroll
                for (int s_ = 0; s_ < 16; ++s_) v[s_] = __builtin_nontemporal_load(sp + 64 * s_);
                const spec_f32x4 vh = __builtin_nontemporal_load(sp + 64 * 16);
#pragma unroll
                for (int s_ = 0; s_ < 4; ++s_) {
                    no_r[4 * s_] = v[s_].x, no_r[4 * s_ + 1] = v[s_].y, no_r[4 * s_ + 2] = v[s_].z, no_r[4 * s_ + 3] = v[s_].w;
                    no_i[4 * s_] = v[4 + s_].x, no_i[4 * s_ + 1] = v[4 + s_].y, no_i[4 * s_ + 2] = v[4 + s_].z, no_i[4 * s_ + 3] = v[4 + s_].w;
                    nm_r[4 * s_] = v[8 + s_].x, nm_r[4 * s_ + 1] = v[8 + s_].y, nm_r[4 * s_ + 2] = v[8 + s_].z, nm_r[4 * s_ + 3] = v[8 + s_].w;
                    nm_i[4 * s_] = v[12 + s_].x, nm_i[4 * s_ + 1] = v[12 + s_].y, nm_i[4 * s_ + 2] = v[12 + s_].z, nm_i[4 * s_ + 3] = v[12 + s_].w;
                }
                nh_r = vh.x, nh_i = vh.y;
            } else {
                staged_wait<0>();
                noise_spectrum_paired<P, true, kCompact>(g, tb.wtype[fi], tw, xbuf, xbuf_byte, lane, wa_c, wa_s, no_r, no_i,
                                                         nm_r, nm_i, nh_r, nh_i, lc, ls);
            }
            if (P != 32) {   // FFT output lanes hold bins kappa(lane) + 64 q; everything below wants bins lane + 64 q
                const int src = kappa<P>(lane);
#pragma unroll
                for (int q = 0; q < HP; ++q) {
                    no_r[q] = __shfl(no_r[q], src);
                    no_i[q] = __shfl(no_i[q], src);
                    nm_r[q] = __shfl(nm_r[q], src);
                    nm_i[q] = __shfl(nm_i[q], src);
                }
                nh_r = __shfl(nh_r, src);
                nh_i = __shfl(nh_i, src);
            }
            const float* mrow = mag + (long long)fi * ld;
            const float* arow = real + (long long)fi * ld;
            const float* brow = imag + (long long)fi * ld;
            // Unvoiced frames have no periodic component (its mask is zero, magphase.py:873-876): the phase features and
            // the periodic curve are neither loaded nor used -- one wave-uniform branch per frame, 4 instead of 10 loads and
            // a third of the arithmetic per bin pair for about a third of the frames.
            float xh_r, xh_i;
            auto assemble_all = [&](auto voiced_tag) {
                constexpr bool V = decltype(voiced_tag)::value;
                auto assemble = [&](float m, float a, float b, float cpv, float cap, float n_r, float n_i, bool real_only,
                                    float& o_r, float& o_i) {
                    const float apf = m * cap * ig;
                    float vr, vi;
                    if (V) {
                        const float s = a * a + b * b;
                        const float u = (s > 0.0f) ? m * cpv * __builtin_amdgcn_rsqf(s) : 0.0f;
                        vr = fmaf(n_r, apf, a * u);
                        vi = fmaf(n_i, apf, b * u);
                    } else {
                        vr = n_r * apf;
                        vi = n_i * apf;
                    }
                    if (real_only) {   // DC and Nyquist: X = |X| (magphase.py:958-961); type 2: Re X (:1567)
                        if constexpr (!T2) vr = __builtin_sqrtf(vr * vr + vi * vi);
                        vi = 0.0f;
                    }
                    o_r = vr * sgn_scale;
                    o_i = vi * sgn_scale;
                };
#ifndef MPX_COMP_QB
#define MPX_COMP_QB (MPX_COMP_PAIR_WAVES > 8 ? 4 : 8)
#endif
#ifndef MPX_COMP_SADDR
#define MPX_COMP_SADDR 1
#endif
#ifndef MPX_COMP_NT
#define MPX_COMP_NT 1   // feature rows are read once, by one wave: non-temporal loads keep them from evicting the other
#endif                  // waves' lines (and any scratch lines) out of L2
                constexpr int QB = (HP < MPX_COMP_QB) ? HP : MPX_COMP_QB;   // pairs per batch: 10 QB loads in flight
                // bin M/2 (lane 0) first: every lane loads "its" bin M/2 + lane (a lane-0-only load becomes a scalar load with
                // an immediate wait, see feat_load_paired); only lane 0's value is used by the merge.  First, because the
                // split's nh_* then die here instead of living through the whole assembly; at 12 waves per CU the result
                // waits in the (idle) exchange buffer, not in two registers.
                {
                    const bool ph = V && M / 2 < n_per;
                    const unsigned bl = 4u * (unsigned)lane;
                    auto gh = [&](const float* row) {
                        return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(row + M / 2) + (size_t)bl);
                    };
                    assemble(gh(mrow), ph ? gh(arow) : 0.0f, ph ? gh(brow) : 0.0f, ph ? gh(per_v) : 0.0f, gh(apc), nh_r, nh_i,
                             false, xh_r, xh_i);
                    if constexpr (kCompact) {
                        xbuf[lane] = xh_r;
                        xbuf[64 + lane] = xh_i;
                    }
                }
                // one batch = the bin pairs q0 .. q0 + QN - 1; OWN / MIR: their own / mirror bins may carry a periodic component
                auto batch = [&](auto q0_, auto qn_, auto own_, auto mir_) {
                    constexpr int Q0 = decltype(q0_)::value, QN = decltype(qn_)::value;
                    constexpr bool OWN = V && decltype(own_)::value, MIR = V && decltype(mir_)::value;
                    float m0[QN], d0[QN], m1[QN], d1[QN], a0[OWN ? QN : 1], b0[OWN ? QN : 1], c0[OWN ? QN : 1];
                    float a1[MIR ? QN : 1], b1[MIR ? QN : 1], c1[MIR ? QN : 1];
                    // keep each batch's loads where they are written (the compiler moves loads of read-only memory across
                    // plain barriers; hoisted above the noise spectrum they spill): the lane offset is laundered with a fake
                    // dependency on what has been produced so far
                    int lo = lane;
                    {
                        constexpr int c0_ = (Q0 == 0) ? 0 : ((Q0 >= 4) ? Q0 - 4 : 0), c1_ = (Q0 == 0) ? HP : Q0;
#pragma unroll
                        for (int c = c0_; c < c1_; c += 4)
                            asm volatile("" : "+v"(lo)
                                         : "v"(no_r[c]), "v"(no_r[c + 1]), "v"(no_r[c + 2]), "v"(no_r[c + 3]), "v"(no_i[c]),
                                           "v"(no_i[c + 1]), "v"(no_i[c + 2]), "v"(no_i[c + 3]), "v"(nm_r[c]), "v"(nm_r[c + 1]),
                                           "v"(nm_r[c + 2]), "v"(nm_r[c + 3]), "v"(nm_i[c]), "v"(nm_i[c + 1]), "v"(nm_i[c + 2]),
                                           "v"(nm_i[c + 3]));
                    }
                    // the row pointer (+ the constant part of the index) stays in SGPRs, the lane part is ONE zero-extended
                    // 32-bit byte offset (global_load_dword v, v, s[..] offset:imm); with int element indices every load got
                    // its own 64-bit address (v_lshl_add_u64 + a register pair: 208 of them in the kernel's ISA)
                    const unsigned blo = 4u * (unsigned)lo, bhi = 4u * (unsigned)(M - lo);
                    auto gl = [](const float* row, int kel, unsigned boff) {
#if MPX_COMP_SADDR && MPX_COMP_NT
                        return __builtin_nontemporal_load(
                            reinterpret_cast<const float*>(reinterpret_cast<const char*>(row + kel) + (size_t)boff));
#elif MPX_COMP_SADDR
                        return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(row + kel) + (size_t)boff);
#else
                        return row[kel + (int)(boff >> 2)];
#endif
                    };
#pragma unroll
                    for (int jj = 0; jj < QN; ++jj) {
                        const int k = 64 * (Q0 + jj);
                        m0[jj] = gl(mrow, k, blo);
                        d0[jj] = gl(apc, k, blo);
                        m1[jj] = gl(mrow, -k, bhi);
                        d1[jj] = gl(apc, -k, bhi);
                        // the periodic curve is zero from bin n_per on (above the crossfade): the phase rows and the curve
                        // are read only for the register rows that reach below it (wave-uniform conditions)
                        // (the offset is laundered inside the conditional block: instruction selection works block by block
                        // and only recognises base + zext(offset) when the zero-extension sits in the same block)
                        if constexpr (OWN) {
                            a0[jj] = b0[jj] = c0[jj] = 0.0f;
                            if (k < n_per) {               // own bins lane + k
                                unsigned bq = blo;
                                asm volatile("" : "+v"(bq));
                                a0[jj] = gl(arow, k, bq);
                                b0[jj] = gl(brow, k, bq);
                                c0[jj] = gl(per_v, k, bq);
                            }
                        }
                        if constexpr (MIR) {
                            a1[jj] = b1[jj] = c1[jj] = 0.0f;
                            if (M - k - 63 < n_per) {      // mirrors M - lane - k
                                unsigned bq = bhi;
                                asm volatile("" : "+v"(bq));
                                a1[jj] = gl(arow, -k, bq);
                                b1[jj] = gl(brow, -k, bq);
                                c1[jj] = gl(per_v, -k, bq);
                            }
                        }
                    }
#pragma unroll
                    for (int jj = 0; jj < QN; ++jj) {
                        const int q = Q0 + jj;
                        const bool ends = (q == 0) && (lane == 0);   // the (DC, Nyquist) pair
                        assemble(m0[jj], OWN ? a0[OWN ? jj : 0] : 0.0f, OWN ? b0[OWN ? jj : 0] : 0.0f,
                                 OWN ? c0[OWN ? jj : 0] : 0.0f, d0[jj], no_r[q], no_i[q], ends, no_r[q], no_i[q]);
                        assemble(m1[jj], MIR ? a1[MIR ? jj : 0] : 0.0f, MIR ? b1[MIR ? jj : 0] : 0.0f,
                                 MIR ? c1[MIR ? jj : 0] : 0.0f, d1[jj], nm_r[q], nm_i[q], ends, nm_r[q], nm_i[q]);
                    }
                };
                using std::integral_constant;
                constexpr auto yes = std::true_type{};
                constexpr auto no = std::false_type{};
#ifndef MPX_COMP_QA
#define MPX_COMP_QA 8   // pairs per batch on the rows with phase (7 loads per pair); (QA, QR) = (8, 8) / (4, 8) / (4, 4) /
                        // (2, 8): 1.182 / 1.191 / 1.193 / 1.201 ms for the synthesis side of configs[2], none spills
#endif
#ifndef MPX_COMP_QR
#define MPX_COMP_QR 8   // pairs per batch on the rows without (4 loads per pair)
#endif
                if constexpr (NPQ >= 0 && P == 32 && NPQ == 8) {   // (4, 4, 8): rows 0-7 with the own bins' phase, rows 8-15 without
                    constexpr int QA = MPX_COMP_QA, QR = MPX_COMP_QR;
                    static_assert(8 % QA == 0 && 8 % QR == 0, "MPX_COMP_QA / MPX_COMP_QR divide 8");
                    batch(integral_constant<int, 0>{}, integral_constant<int, QA>{}, yes, no);
                    if constexpr (QA < 8) batch(integral_constant<int, QA>{}, integral_constant<int, QA>{}, yes, no);
                    if constexpr (QA < 4) batch(integral_constant<int, 2 * QA>{}, integral_constant<int, QA>{}, yes, no);
                    if constexpr (QA < 4) batch(integral_constant<int, 3 * QA>{}, integral_constant<int, QA>{}, yes, no);
                    batch(integral_constant<int, 8>{}, integral_constant<int, QR>{}, no, no);
                    if constexpr (QR < 8) batch(integral_constant<int, 8 + QR>{}, integral_constant<int, QR>{}, no, no);
                    if constexpr (QR < 4) batch(integral_constant<int, 8 + 2 * QR>{}, integral_constant<int, QR>{}, no, no);
                    if constexpr (QR < 4) batch(integral_constant<int, 8 + 3 * QR>{}, integral_constant<int, QR>{}, no, no);
                } else {
                    static_assert(NPQ < 0 || (P == 32 && NPQ == 8), "k_synth_comp_pair: NPQ schedules exist for P == 32, NPQ == 8");
                    static_assert(QB == 1 || QB == 2 || QB == 4 || QB == 8 || QB == 16, "MPX_COMP_QB");
                    // uniform batches of QB pairs (unrolled by hand: the batch sizes are template arguments)
                    if constexpr (HP / QB >= 1) batch(integral_constant<int, 0 * QB>{}, integral_constant<int, QB>{}, yes, yes);
                    if constexpr (HP / QB >= 2) batch(integral_constant<int, 1 * QB>{}, integral_constant<int, QB>{}, yes, yes);
                    if constexpr (HP / QB >= 3) batch(integral_constant<int, 2 * QB>{}, integral_constant<int, QB>{}, yes, yes);
                    if constexpr (HP / QB >= 4) batch(integral_constant<int, 3 * QB>{}, integral_constant<int, QB>{}, yes, yes);
                    if constexpr (HP / QB >= 5) batch(integral_constant<int, 4 * QB>{}, integral_constant<int, QB>{}, yes, yes);
                    if constexpr (HP / QB >= 6) batch(integral_constant<int, 5 * QB>{}, integral_constant<int, QB>{}, yes, yes);
                    if constexpr (HP / QB >= 7) batch(integral_constant<int, 6 * QB>{}, integral_constant<int, QB>{}, yes, yes);
                    if constexpr (HP / QB >= 8) batch(integral_constant<int, 7 * QB>{}, integral_constant<int, QB>{}, yes, yes);
                    static_assert(HP / QB <= 8, "more batches than the hand-unrolled schedule covers");
                }
            };
            if (voiced) assemble_all(std::true_type{});
            else assemble_all(std::false_type{});
            if constexpr (kCompact) {   // kappa(lane) == lane: the synthesis-side twiddle is the conjugate of the split's
                const float4 pk = tw_half_pad<P>(tw, lane);
                ws_c = pk.x;
                ws_s = -pk.y;
                xh_r = xbuf[lane];
                xh_i = xbuf[64 + lane];
            }
            merge_paired_complex<P>(no_r, no_i, nm_r, nm_i, xh_r, xh_i, xr, xi, lane, ws_c, ws_s);
        } else {
            // ---- aperiodic source: spectrum of this frame's windowed noise, bins k = lane + 64 j
            float nM;
            {
                staged_wait<0>();
                noise_spectrum<P, true, kCompact>(g, tb.wtype[fi], tw, xbuf, xbuf_byte, lane, wa_c, wa_s, xr, xi, nM, lc, ls);
                if (P != 32) {   // FFT output lanes hold bins kappa(lane)+64j; everything below wants bins lane+64j
                    const int src = kappa<P>(lane);
    #pragma unroll
                    for (int j = 0; j < P; ++j) {
                        xr[j] = __shfl(xr[j], src);
                        xi[j] = __shfl(xi[j], src);
                    }
                    nM = __shfl(nM, src);
                }
            }

            // ---- spectrum assembly (Appendix A2 steps 9-12) in place, HB register rows at a time: all loads of a batch are
            // issued together and branch-free (one memory latency per batch)
            const int r0 = LERP ? tb.row0[fi] : fi, r1 = LERP ? tb.row1[fi] : fi;
            const float rt = LERP ? tb.rowt[fi] : 0.0f;   // 0 when r0 == r1: the lerp below is then exact
            const float* m0p = mag + (long long)r0 * ld;
            const float* a0p = real + (long long)r0 * ld;
            const float* b0p = imag + (long long)r0 * ld;
            const float* m1p = mag + (long long)r1 * ld;
            const float* a1p = real + (long long)r1 * ld;
            const float* b1p = imag + (long long)r1 * ld;
            float xm = 0.0f;
    #ifndef MPX_COMP_FEAT_ROWS
    #define MPX_COMP_FEAT_ROWS 16
    #endif
            // register rows per batch: 8 x HB loads in flight (P == 8 has fewer rows than a batch: one batch of P -- with
            // HB == 16 the loop below ran P / HB == 0 times and fft_len 1024 with row tables skipped the assembly)
            constexpr int HB = (P < MPX_COMP_FEAT_ROWS) ? P : MPX_COMP_FEAT_ROWS;
            static_assert(P % HB == 0 && HB % 8 == 0, "the batches cover the P register rows, 8 at a time");
    #pragma unroll
            for (int h = 0; h < P / HB; ++h) {
                float m0[HB], a0[HB], b0[HB], m1[HB], a1[HB], b1[HB], cpv[HB], cap[HB];
                // keep each half's loads where they are written: hoisted above the noise spectrum (or into the other
                // half) they cost 190 spilled registers
                // (the compiler moves loads of read-only memory across plain barriers: the lane offset is laundered with a
                // fake dependency on the last value produced before this half)
                int lo = lane;
                {
                    const int c0 = (h == 0) ? 0 : (h - 1) * HB, c1 = (h == 0) ? P : h * HB;   // everything produced so far
    #pragma unroll
                    for (int c = c0; c < c1; c += 8)
                        asm volatile("" : "+v"(lo)
                                     : "v"(xr[c]), "v"(xr[c + 1]), "v"(xr[c + 2]), "v"(xr[c + 3]), "v"(xr[c + 4]), "v"(xr[c + 5]),
                                       "v"(xr[c + 6]), "v"(xr[c + 7]), "v"(xi[c]), "v"(xi[c + 1]), "v"(xi[c + 2]), "v"(xi[c + 3]),
                                       "v"(xi[c + 4]), "v"(xi[c + 5]), "v"(xi[c + 6]), "v"(xi[c + 7]));
                }
    #pragma unroll
                for (int jj = 0; jj < HB; ++jj) {
                    const int k = 64 * (h * HB + jj);
                    m0[jj] = m0p[lo + k];
                    a0[jj] = a0p[lo + k];
                    b0[jj] = b0p[lo + k];
                    if (LERP) {
                        m1[jj] = m1p[lo + k];
                        a1[jj] = a1p[lo + k];
                        b1[jj] = b1p[lo + k];
                    }
                    cpv[jj] = per_v[lo + k];
                    cap[jj] = apc[lo + k];
                }
    #pragma unroll
                for (int jj = 0; jj < HB; ++jj) {
                    const int j = h * HB + jj;
                    // linear interpolation between constant-rate rows (magphase.py:2242-2252); rt == 0 for variable-rate input
                    const float m = LERP ? fmaf(m1[jj] - m0[jj], rt, m0[jj]) : m0[jj];
                    const float a = LERP ? fmaf(a1[jj] - a0[jj], rt, a0[jj]) : a0[jj];
                    const float b = LERP ? fmaf(b1[jj] - b0[jj], rt, b0[jj]) : b0[jj];
                    const float s = a * a + b * b;
                    const float u = (s > 0.0f) ? m * cpv[jj] * pvs * __builtin_amdgcn_rsqf(s) : 0.0f;
                    const float apf = m * cap[jj] * ig;
                    float vr = fmaf(xr[j], apf, a * u), vi = fmaf(xi[j], apf, b * u);
                    if (j == 0 && lane == 0) {   // DC: X = |X| (magphase.py:958-961); type 2: Re X (:1567)
                        if constexpr (!T2) vr = __builtin_sqrtf(vr * vr + vi * vi);
                        vi = 0.0f;
                    }
                    xr[j] = vr * sgn_scale;
                    xi[j] = vi * sgn_scale;
                }
            }
            if (lane == 0) {   // Nyquist bin: the noise spectrum is real there; X = |X| (type 2: Re X)
                const float m = LERP ? fmaf(m1p[M] - m0p[M], rt, m0p[M]) : m0p[M];
                const float a = LERP ? fmaf(a1p[M] - a0p[M], rt, a0p[M]) : a0p[M];
                const float b = LERP ? fmaf(b1p[M] - b0p[M], rt, b0p[M]) : b0p[M];
                const float s = a * a + b * b;
                const float u = (s > 0.0f) ? m * per_v[M] * pvs * __builtin_amdgcn_rsqf(s) : 0.0f;
                const float apf = m * apc[M] * ig;
                const float vr = fmaf(nM, apf, a * u), vi = b * u;
                xm = (T2 ? vr : __builtin_sqrtf(vr * vr + vi * vi)) * (0.5f / (float)M);   // (-1)^M = +1
            }

            if constexpr (kCompact) {
                const float4 pk = tw_half_pad<P>(tw, lane);
                ws_c = pk.x;
                ws_s = -pk.y;
            }
            hermitian_merge<P>(xr, xi, xm, lane, ws_c, ws_s);
        }
        pair_inverse_fft_front<P>(w, xr, xi, lane);
        if (!SPEC && nxt.valid) {
            g = frame_geom(noise, tb.npos[nxt.fi], tb.nleft[nxt.fi], tb.nright[nxt.fi], N);
            pair_stage_next<P>(w, g, lane);
        }
        pair_inverse_fft_back<P>(xr, xi);

        // ---- anti-ringing window (magphase.py:969-973, Q14): centred asymmetric Hann, zero outside
        const int wl = tb.win_l[fi], wr = tb.win_r[fi];
        const float inv_wl = (wl > 0) ? 1.0f / (float)wl : 1.0f;
        const float inv_wr = (wr > 0) ? 1.0f / (float)wr : 0.0f;
        const int kadd = (wl == 0) ? 1 : 0;
        const int n_lo = N / 2 - wl, n_hi = N / 2 + wr;   // support [n_lo, n_hi]
        auto win_add = [&](float o, float v, int n) {
            const int ks = n - n_lo;
            const float w_ = (ks >= 0 && n <= n_hi) ? half_window(ks, wl, wl + wr, kadd, inv_wl, inv_wr, 0) : 0.0f;
            return fmaf(v, w_, o);
        };
        // register rows whose samples all lie outside the window support add nothing: skipped (wave-uniform)
        auto row_live = [&](int q) { return !(128 * q + 127 < n_lo || 128 * q > n_hi); };
        pair_ordered_ola<P, false>(w, cur, smem, runs, tb.pm_rel, strips, pcm, xr, xi, lane, win_add, row_live);
        cur = nxt;
    }
}

// ---------------------------------------------------------------------------------------------
// Lossless analysis -> synthesis of the same frames in ONE launch (copy synthesis: analysis_lossless followed by
// synthesis_from_lossless, demos/demo_copy_synthesis_lossless.py:44-50; magphase.py:2869-2906, 1759-1776).  The wave that
// analysed frame f still holds X[k] for the bin pairs (k, M - k) the synthesis wants from it (PairFeat: lane l <-> bins
// l + 64 q and their mirrors): it writes the three feature rows -- the API's output -- and rebuilds the frame from the
// very float32 values it stored, so the 3 x 4 H bytes per frame that k_synth_ola_pair reads back from HBM (1.4 GB per
// 57 k frames: 0.14 J of the step's 0.7 J on a board that runs both kernels at its power limit) are not
// read at all.  Structure = k_synth_comp_pair without the spectrum assembly: frame geometry from the ANALYSIS tables
// (position / left / right of the epoch in the recording), samples staged by LDS-DMA into the exchange buffer while the
// previous frame overlap-adds, Hann halves, real FFT + split in the paired layout (noise_spectrum_paired), features
// (magphase.py:466-474) stored in k_analysis' line-friendly shape, unit-phase spectrum + Hermitian merge
// (feat_merge_paired: exactly what k_synth_ola_pair computes from the loaded values), inverse transform, overlap-add
// into the pair's LDS ring in frame order (runs / slots / tickets / head strips as k_synth_ola_pair; k_ola_fixup
// afterwards).  The output samples are what k_synth_ola_pair gives on the features this kernel wrote up to float32
// rounding (the same expressions; the compiler contracts their multiply-adds differently in the two kernels: measured
// 3.6e-7 of the signal peak; the DIRECT arm, see below, adds the windowed frame itself and is closer to the oracle); the features differ from k_analysis' in the last bits (DIT instead of DIF forward
// transform).  Both are held to the two-launch path's tolerances against the oracle.
// Every frame index of [0, n_frames) must belong to exactly one run: a frame outside the runs is not analysed.
// ---------------------------------------------------------------------------------------------
#ifdef MPX_PROBE_ENDTIME
// Probe build (tools/roundtrip_deal_probe.py), as k_synth_ola_pair's in magphase_hip.hip: every wave of k_roundtrip_pair
// stores the constant-rate clock (100 MHz) when it enters and when it leaves its frame loop, its frame count and its
// shader cycles -- per slot (= wave pair), the later of the two ends is when the slot's share was done.
__device__ unsigned long long g_rt_endprobe[4 * 8192];   // per wave: start, end (100 MHz clock), frames, shader cycles
#endif

// CLS: frames of a narrow support class (frame_support_class, mpx_common.hpp: the windowed frame is zero outside a few
// register rows, and so is the frame rebuilt from it) take instances of the gather, the first forward pass, the last
// inverse pass and the ring add whose row sets are compile-time constants -- one wave-uniform decision per frame, taken
// from the frame's own (L, R).  false: every frame takes the full class (MAGPHASE_RT_SUPPORT=full; every N but 4096).
#ifndef MPX_RT_FORCE_NARROW
#define MPX_RT_FORCE_NARROW 0   // 1 (timing experiments only, wrong results): every frame is treated as the narrow class
#endif
// Whether k_roundtrip_pair<P, CLS> has the pruned passes: the one condition the kernel and the host's view of what its
// frames add to the ring (mpx_roundtrip_frame_extents) both read.
template <int P>
constexpr bool roundtrip_prunes(bool cls) { return cls && P == 32 && comp_compact<P>() && !MPX_COMP_DIT; }
// ST: how the feature rows are stored.  kStoreRows: 256-byte blocks aligned to the row (k_analysis' shape).  kStoreLines
// (P = 32 with CLS only): blocks aligned to memory, two whole 128-byte lines each whatever the row's phase (mpx_common.hpp,
// "Row stores by line").  kStoreLinesNT: those with the non-temporal bit on the interior (whole-line) stores; the clipped
// edge blocks and the two parts of the middle block stay plain -- a sibling wave or the next store completes their lines,
// so they need L2's merging.
constexpr int kStoreRows = 0, kStoreLines = 1, kStoreLinesNT = 2;
// DIRECT (P = 32; the default of the launch, MPX_RT_INVERSE_TRANSFORM takes the other arm): the synthesis half is fed X
// exactly as the split leaves it, so what the merge and the inverse transform rebuild is fftshift(IFFT(hermitian(FFT(y))))
// of the windowed, rotated, zero-padded frame y that the gather has just put into registers -- whose exact value is
// fftshift(y) (X == 0 gives 0 on both paths; the .real of the inverse drops what is exactly 0 for a real y).  The direct
// arm overlap-adds y itself: row q of the shifted frame is gathered row (q + P/2) mod P on the same lane and plane, the
// ring add's combine is a plain sum, and the ordered section runs right after the gather (a hook of noise_fft), on the
// registers the forward transform then reads -- no copy of the frame is kept.  The next frame's staging moves behind the
// forward transform's last use of the exchange buffer.  Merge, handover and inverse transform are not instantiated; the
// feature rows are the other arm's bit for bit, the waveform loses the two transforms' float32 error (~3e-7 of the peak).
// N = 2048 / 1024 keep the transform: there the ring's lanes hold samples in kappa(lane) order, the gather's in lane order.
constexpr bool kRtDirectBuilt = !MPX_COMP_DIT;   // (the DIT form gathers into bit-reversed registers)
template <int P, bool CLS = false, int ST = kStoreRows, bool DIRECT = false>
__global__ __launch_bounds__(kCompPairWaves * 64) void k_roundtrip_pair(const float* __restrict__ sig,
                                                                       const long long* __restrict__ fpos,
                                                                       const int* __restrict__ fleft,
                                                                       const int* __restrict__ fright,
                                                                       const RunDesc* __restrict__ runs,
                                                                       const int* __restrict__ slot_off,
                                                                       const int* __restrict__ slot_runs, int nslots,
                                                                       const int* __restrict__ pm_rel,
                                                                       const float* __restrict__ tw_g,
                                                                       float* __restrict__ omag, float* __restrict__ oreal,
                                                                       float* __restrict__ oimag, float* __restrict__ strips,
                                                                       float* __restrict__ pcm, long long ld) {
    constexpr int M = 64 * P, N = 2 * M, HP = P / 2;
    static_assert(ST == kStoreRows || (P == 32 && CLS), "the line-aligned store forms exist for P = 32 with CLS only");
    static_assert(!DIRECT || (P == 32 && kRtDirectBuilt), "the direct arm: N = 4096, gather in natural register order");
    constexpr bool kCls = roundtrip_prunes<P>(CLS);   // the forms that have pruned passes
    constexpr int NW = kCls ? kSupportNarrow : 0;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    PairWave w;
    if (!pair_wave_setup<P>(w, smem, tw_g, runs, slot_off, slot_runs, nslots)) return;
    PairCursor cur = w.cur;

    FrameGeom g = frame_geom(sig, fpos[cur.fi], fleft[cur.fi], fright[cur.fi], N);
    pair_stage_frame<P>(w, g, w.lane_id);

#ifdef MPX_PROBE_ENDTIME
    const unsigned long long probe_t0 = wall_clock64();
    const unsigned long long probe_c0 = clock64();
    int probe_frames = 0;
#endif
    while (cur.valid) {
        int lane;
        float wa_s, wa_c, ws_s, ws_c;
        pair_frame_lane<P>(w, lane, wa_s, wa_c, ws_s, ws_c);
        PairCursor nxt = cur;
        pair_cursor_advance(nxt, w.wi_end, w.half, runs, slot_runs);
        const int fi = cur.fi;
        // the staged frame's support class (g is this frame's until the next one is staged below)
        bool narrow = false;
        if constexpr (kCls) narrow = MPX_RT_FORCE_NARROW || (frame_support_class(g.L, g.LR - g.L, N) == NW);

        float xr[P], xi[P];   // the merged spectrum, then the rebuilt frame (not under DIRECT)
        FrameGeom g_next = g;
        {
            float no_r[HP], no_i[HP], nm_r[HP], nm_i[HP], nh_r, nh_i;
            if constexpr (DIRECT) {
                // the ordered section on the gathered frame itself (ROT: rows half a transform apart, the fftshift; natural
                // register order), then the transform; the next frame is staged once the exchange buffer is idle
                auto on_gathered = [&](float (&re)[P], float (&im)[P], auto narrow_c) __attribute__((always_inline)) {
                    auto plain_sum = [](float o, float v, int) { return o + v; };
                    auto all_rows = [](int) { return true; };
                    pair_ordered_ola<P, true, NW, true>(w, cur, smem, runs, pm_rel, strips, pcm, re, im, lane, plain_sum,
                                                        all_rows, decltype(narrow_c)::value);
                };
                auto on_exchanged = [&]() __attribute__((always_inline)) {
                    if (nxt.valid) {
                        g_next = frame_geom(sig, fpos[nxt.fi], fleft[nxt.fi], fright[nxt.fi], N);
                        pair_stage_next<P>(w, g_next, lane);
                    }
                };
                pair_analysis_spectrum<P, NW>(w, g, lane, wa_c, wa_s, no_r, no_i, nm_r, nm_i, nh_r, nh_i, narrow,
                                              noise_fft_hook(on_gathered, on_exchanged));
            } else {
                pair_analysis_spectrum<P, NW>(w, g, lane, wa_c, wa_s, no_r, no_i, nm_r, nm_i, nh_r, nh_i, narrow);
            }
            // ---- per bin pair q: lossless features (magphase.py:466-474; as k_analysis: X == 0 -> all three 0), their
            // stores, and the pair's step of the Hermitian merge -- feat_merge_paired's arithmetic on the values just
            // stored (X = mag (R + jI) / |R + jI|, magphase.py:1761-1766), pair by pair so that a pair's four inputs die
            // as its four outputs appear (all 99 features at once, as k_synth_ola_pair holds them: 49 spilled registers)
            MPX_MARK("features_stores_merge");
            auto feat = [](float x_r, float x_i, float& m, float& a, float& b) {
                const float s2 = x_r * x_r + x_i * x_i;
                const float r = __builtin_amdgcn_rsqf(fmaxf(s2, 1.0e-37f));
                m = s2 * r;
                a = x_r * r;
                b = x_i * r;
            };
            if constexpr (comp_compact<P>()) {   // kappa(lane) == lane: the synthesis-side twiddle is the conjugate of the split's
                const float4 pk = tw_half_pad<P>(w.tw, lane);
                ws_c = pk.x;
                ws_s = -pk.y;
            }
            const bool lane0 = (lane == 0);
            // the three rows in k_analysis' store shape: ascending 256-byte blocks of the own bins in natural q order; the
            // mirrors of step q regrouped into aligned blocks [M - 64 q - 64, M - 64 q - 1] whose lowest float is lane 0's
            // mirror of step q + 1 (bin M/2 for the last block); bin M alone from lane 0
            float* row_m = omag + (long long)fi * ld;
            float* row_r = oreal + (long long)fi * ld;
            float* row_i = oimag + (long long)fi * ld;
            // ... or, by line (ST != kStoreRows), the same two streams in blocks aligned to memory: each plane's phase from
            // its own row pointer (wave-uniform; any ld, any base), the six predicates as lane masks formed once per frame
            int s_m = 0, s_r = 0, s_i = 0;
            if constexpr (ST != kStoreRows) {
                s_m = __builtin_amdgcn_readfirstlane(row_store_phase(row_m));
                s_r = __builtin_amdgcn_readfirstlane(row_store_phase(row_r));
                s_i = __builtin_amdgcn_readfirstlane(row_store_phase(row_i));
            }
            const bool pv_m = row_asc_prev(lane, s_m), pv_r = row_asc_prev(lane, s_r), pv_i = row_asc_prev(lane, s_i);
            const bool cu_m = row_mir_cur(lane, s_m), cu_r = row_mir_cur(lane, s_r), cu_i = row_mir_cur(lane, s_i);
            // (by line the per-lane offsets are formed per store from the lane and the store's predicate: offsets kept per plane
            // would be four more live registers, and the form then needs scratch)
            const int hoff = lane0 ? M - 64 : M - lane;
            float* mlo = row_m + (ST != kStoreRows ? 0 : lane);
            float* rlo = row_r + (ST != kStoreRows ? 0 : lane);
            float* ilo = row_i + (ST != kStoreRows ? 0 : lane);
            float* mhi = row_m + (ST != kStoreRows ? 0 : hoff);
            float* rhi = row_r + (ST != kStoreRows ? 0 : hoff);
            float* ihi = row_i + (ST != kStoreRows ? 0 : hoff);
            auto st_line = [](float* dst, float v) {   // an interior block: two whole lines
                if constexpr (ST == kStoreLinesNT) __builtin_nontemporal_store(v, dst);
                else *dst = v;
            };
            // A clipped block: the store under a lane mask, without a branch.  An `if` around a store is a basic block of its
            // own, and the compiler contracts products with sums block by block: the split's arithmetic, which it sinks past
            // the first step's stores, would be cut differently from the row-relative form's and the rows would differ from
            // that form's in their last bits.  So the by-line forms keep that form's control flow -- one conditional block in
            // the first step, where it stores bin M -- and mask their other clipped stores here.
            auto st_mask = [](float* dst, float v, unsigned long long mask) {
                unsigned long long saved;
                asm volatile("s_and_saveexec_b64 %0, %3\n\tglobal_store_dword %1, %2, off\n\ts_mov_b64 exec, %0"
                             : "=&s"(saved)
                             : "v"(dst), "v"(v), "s"(mask)
                             : "memory", "scc");
            };
            unsigned long long k_pv_m = 0, k_pv_r = 0, k_pv_i = 0, k_cu_m = 0, k_cu_r = 0, k_cu_i = 0;
            if constexpr (ST != kStoreRows) {
                k_pv_m = __builtin_amdgcn_ballot_w64(pv_m), k_cu_m = __builtin_amdgcn_ballot_w64(cu_m);
                k_pv_r = __builtin_amdgcn_ballot_w64(pv_r), k_cu_r = __builtin_amdgcn_ballot_w64(cu_r);
                k_pv_i = __builtin_amdgcn_ballot_w64(pv_i), k_cu_i = __builtin_amdgcn_ballot_w64(cu_i);
            }
            float zr[HP], zi[HP];   // Z[M - k]
            float hm = 0.0f, ha = 0.0f, hb = 0.0f;   // mirror features of the previous step
            float pm = 0.0f, pa = 0.0f, pb = 0.0f;   // own features of the previous step (by line only)
#pragma unroll
            for (int q = 0; q < HP; ++q) {
                float m, a, b, mq, aq, bq;
                feat(no_r[q], no_i[q], m, a, b);
                feat(nm_r[q], nm_i[q], mq, aq, bq);
                if constexpr (ST == kStoreRows) {
                    mlo[64 * q] = m;
                    rlo[64 * q] = a;
                    ilo[64 * q] = b;
                    if (q == 0) {
                        if (lane0) {
                            row_m[M] = mq;
                            row_r[M] = aq;
                            row_i[M] = bq;
                        }
                    } else {
                        mhi[-64 * (q - 1)] = lane0 ? mq : hm;
                        rhi[-64 * (q - 1)] = lane0 ? aq : ha;
                        ihi[-64 * (q - 1)] = lane0 ? bq : hb;
                    }
                } else if (q == 0) {   // the clipped blocks B_0 and B_P
                    st_mask(mlo + row_asc_base(lane, false) + row_asc_off(0), m, ~k_pv_m);
                    st_mask(rlo + row_asc_base(lane, false) + row_asc_off(0), a, ~k_pv_r);
                    st_mask(ilo + row_asc_base(lane, false) + row_asc_off(0), b, ~k_pv_i);
                    if (cu_m || cu_r || cu_i) {
                        st_mask(mhi + row_mir_base(lane, true, M) + row_mir_off(0), mq, k_cu_m);
                        st_mask(rhi + row_mir_base(lane, true, M) + row_mir_off(0), aq, k_cu_r);
                        st_mask(ihi + row_mir_base(lane, true, M) + row_mir_off(0), bq, k_cu_i);
                    }
                } else {               // B_q and B_{P - q}
                    st_line(mlo + row_asc_base(lane, pv_m) + row_asc_off(q), pv_m ? pm : m);
                    st_line(rlo + row_asc_base(lane, pv_r) + row_asc_off(q), pv_r ? pa : a);
                    st_line(ilo + row_asc_base(lane, pv_i) + row_asc_off(q), pv_i ? pb : b);
                    st_line(mhi + row_mir_base(lane, cu_m, M) + row_mir_off(q), cu_m ? mq : hm);
                    st_line(rhi + row_mir_base(lane, cu_r, M) + row_mir_off(q), cu_r ? aq : ha);
                    st_line(ihi + row_mir_base(lane, cu_i, M) + row_mir_off(q), cu_i ? bq : hb);
                }
                if constexpr (ST != kStoreRows) {
                    pm = m;
                    pa = a;
                    pb = b;
                }
                hm = mq;
                ha = aq;
                hb = bq;
                // feat_merge_paired, step j = q, on X itself: mag (R + jI) / |R + jI| of the three values just formed IS X up
                // to their float32 rounding (m = |X|^2 r, (a, b) = X r with r = rsq(|X|^2): the product differs from X by the
                // relative error of r, < 2.5e-7), so the magnitude, the second inverse square root and four products per bin
                // that feat_merge_paired spends on rebuilding it are not spent here.  The (-1)^k of the fftshift is a rotation
                // of the inverse transform's output by half its length -- a renaming of registers in the overlap-add below --
                // and the 0.5 / M of the inverse transform rides on the overlap-add's multiply-add: both exact.
                // (DIRECT: none of it -- the frame is in the ring already.  What stays is the merge's twiddle, formed and
                // thrown away: it is the conjugate of the split's W_N^k and shares that one's products, and which product of
                // a sum of two the compiler fuses into the multiply-add depends on how many uses each has -- without the
                // merge's uses the split's twiddles, and with them the rows, come out with other last bits than the other
                // arm's.  One multiply-add per bin pair.)
                if constexpr (DIRECT) {
                    const float cq = cos2p<P>(q), sq = sin2p<P>(q);
                    const float wr = ws_c * cq - ws_s * sq, wi = ws_c * sq + ws_s * cq;
                    asm volatile("" ::"v"(wr), "v"(wi));
                } else {
                    const float x_r = no_r[q], p_r = nm_r[q];
                    float x_i = no_i[q], p_i = nm_i[q];
                    if (q == 0) {   // DC and Nyquist: imaginary parts dropped (Q5)
                        x_i = lane0 ? 0.0f : x_i;
                        p_i = lane0 ? 0.0f : p_i;
                    }
                    merge_pair_step<P>(q, x_r, x_i, p_r, p_i, ws_c, ws_s, xr[q], xi[q], zr[q], zi[q]);
                }
            }
            float mH, aH, bH;
            feat(nh_r, nh_i, mH, aH, bH);
            if constexpr (ST == kStoreRows) {
                mhi[-64 * (HP - 1)] = lane0 ? mH : hm;
                rhi[-64 * (HP - 1)] = lane0 ? aH : ha;
                ihi[-64 * (HP - 1)] = lane0 ? bH : hb;
            } else {   // the middle block B_{P/2}: its low part from the ascending stream, its high part from the mirrors
                st_mask(mlo + row_asc_base(lane, true) + row_asc_off(HP), pm, k_pv_m);
                st_mask(rlo + row_asc_base(lane, true) + row_asc_off(HP), pa, k_pv_r);
                st_mask(ilo + row_asc_base(lane, true) + row_asc_off(HP), pb, k_pv_i);
                static_assert(row_mir_tail_live(0, true) && !row_mir_tail_live(1, true) && row_mir_tail_live(1, false),
                              "the mirror tail's lanes: lane 0 and those that do not store this step's mirror");
                st_mask(mhi + row_mir_base(lane, cu_m, M) + row_mir_off(HP), lane0 ? mH : hm, ~k_cu_m | 1ull);
                st_mask(rhi + row_mir_base(lane, cu_r, M) + row_mir_off(HP), lane0 ? aH : ha, ~k_cu_r | 1ull);
                st_mask(ihi + row_mir_base(lane, cu_i, M) + row_mir_off(HP), lane0 ? bH : hb, ~k_cu_i | 1ull);
            }
            // bin M/2 (lane 0): Z = 2 conj(X)
            if constexpr (!DIRECT) merge_handover<P>(zr, zi, 2.0f * nh_r, -2.0f * nh_i, xr, xi, lane);
        }
        if constexpr (DIRECT) {
            g = g_next;
        } else {
            pair_inverse_fft_front<P>(w, xr, xi, lane);
            if (nxt.valid) {
                g = frame_geom(sig, fpos[nxt.fi], fleft[nxt.fi], fright[nxt.fi], N);
                pair_stage_next<P>(w, g, lane);
            }
            if constexpr (kCls) pair_inverse_fft_back_class<P, NW>(xr, xi, narrow);
            else pair_inverse_fft_back<P>(xr, xi);
            constexpr float kScale = 0.5f / (float)M;   // the inverse transform's scale, on the overlap-add's multiply-add
            auto plain_add = [](float o, float v, int) { return fmaf(v, kScale, o); };
            auto all_rows = [](int) { return true; };
            // ROT: rows taken half a transform apart, the fftshift
            pair_ordered_ola<P, true, NW>(w, cur, smem, runs, pm_rel, strips, pcm, xr, xi, lane, plain_add, all_rows, narrow);
        }
        cur = nxt;
#ifdef MPX_PROBE_ENDTIME
        ++probe_frames;
#endif
    }
#ifdef MPX_PROBE_ENDTIME
    if (w.lane_id == 0) {
        const int pw = (blockIdx.x * kCompPairWaves + (int)(threadIdx.x >> 6)) % 8192;
        g_rt_endprobe[4 * pw + 0] = probe_t0;
        g_rt_endprobe[4 * pw + 1] = wall_clock64();
        g_rt_endprobe[4 * pw + 2] = (unsigned long long)probe_frames;
        g_rt_endprobe[4 * pw + 3] = clock64() - probe_c0;
    }
#endif
}

// ---------------------------------------------------------------------------------------------
// One pitch-synchronous Griffin-Lim iteration (magphase.py:3320-3372, the loop body after the first synthesis): the frames
// of sig_in are analysed as k_roundtrip_pair analyses them (Hann halves around the epoch, epoch rotated to index 0, real
// FFT in the paired layout), the magnitude of each bin is replaced by the target's, Y = |T| X / |X|, and the frame is
// rebuilt and overlap-added into sig_out exactly as k_roundtrip_pair does (Hermitian merge, inverse transform, fftshift by
// register renaming, LDS ring, runs / slots / tickets / head strips; k_ola_fixup afterwards).  Conventions: the reference
// centres its frames at N/2 and does not fftshift after the iFFT; here the epoch sits at index 0, so X = (-1)^k X_ref and
// the fftshift of the synthesis undoes the factor -- the magnitude is replaced in this kernel's own convention.  X == 0
// (the reference's angle(0) = 0) becomes the phasor (-1)^k, never NaN.  phase_out (null except on the last iteration)
// receives angle(X_ref) for bins 0..M with np.angle's range, rows `ld` floats apart like the target magnitudes.
// Whether the phase rows are written is a run-time branch around the arctangents (wave-uniform: a kernel argument), not a
// template parameter: as two instances the compiler contracted the same source differently (under -ffp-contract=fast a
// multiply fuses only with an add of its own basic block, and the arctangents' branches cut the blocks elsewhere; which
// product of a b - c d is fused depends on the order of the block's nodes), and at P = 32 the signal of the launch with
// phase rows differed from the other's in the last bit of 3 samples in 4.  One instance, one signal.
// No feature rows are written; target magnitudes are float32 rows of pitch ld.  sig_in and sig_out must not overlap.
// A kernel of its own, built from the same frame stages as k_roundtrip_pair, rather than a template arm of it: only the
// middle of the frame loop (what is done to the spectrum) is this kernel's.
// ---------------------------------------------------------------------------------------------
template <int P>
__global__ __launch_bounds__(kCompPairWaves * 64) void k_griffin_lim_pair(const float* __restrict__ sig,
                                                                         const long long* __restrict__ fpos,
                                                                         const int* __restrict__ fleft,
                                                                         const int* __restrict__ fright,
                                                                         const RunDesc* __restrict__ runs,
                                                                         const int* __restrict__ slot_off,
                                                                         const int* __restrict__ slot_runs, int nslots,
                                                                         const int* __restrict__ pm_rel,
                                                                         const float* __restrict__ tw_g,
                                                                         const float* __restrict__ tmag,
                                                                         float* __restrict__ phase_out,
                                                                         float* __restrict__ strips,
                                                                         float* __restrict__ pcm, long long ld) {
    constexpr int M = 64 * P, N = 2 * M, HP = P / 2;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    PairWave w;
    if (!pair_wave_setup<P>(w, smem, tw_g, runs, slot_off, slot_runs, nslots)) return;
    PairCursor cur = w.cur;

    FrameGeom g = frame_geom(sig, fpos[cur.fi], fleft[cur.fi], fright[cur.fi], N);
    pair_stage_frame<P>(w, g, w.lane_id);

    while (cur.valid) {
        int lane;
        float wa_s, wa_c, ws_s, ws_c;
        pair_frame_lane<P>(w, lane, wa_s, wa_c, ws_s, ws_c);
        PairCursor nxt = cur;
        pair_cursor_advance(nxt, w.wi_end, w.half, runs, slot_runs);
        const int fi = cur.fi;

        float xr[P], xi[P];
        {
            float no_r[HP], no_i[HP], nm_r[HP], nm_i[HP], nh_r, nh_i;
            pair_analysis_spectrum<P>(w, g, lane, wa_c, wa_s, no_r, no_i, nm_r, nm_i, nh_r, nh_i);
            MPX_MARK("magnitude_merge");
            // ---- per bin pair q: Y = T X / |X| (X == 0 -> T (-1)^k), then the pair's step of the Hermitian merge as in
            // k_roundtrip_pair.  Bin k = lane + 64 q and its mirror M - k share the parity of lane (M is even).
            const bool lane0 = (lane == 0);
            const float sgn = (lane & 1) ? -1.0f : 1.0f;
            const float* trow = tmag + (long long)fi * ld;
            if (phase_out != nullptr) {   // angle(X_ref), X_ref = (-1)^k X; X == 0 -> 0.  One bin pair at a time (the
                // barrier keeps the compiler from interleaving the arctangents, which spills at P = 32)
                auto ang = [](float x_r, float x_i, float s) {
                    return (x_r == 0.0f && x_i == 0.0f) ? 0.0f : atan2f(s * x_i, s * x_r);
                };
                float* prow = phase_out + (long long)fi * ld;
#pragma unroll
                for (int q = 0; q < HP; ++q) {
                    const int k = lane + 64 * q;
                    prow[k] = ang(no_r[q], no_i[q], sgn);
                    prow[M - k] = ang(nm_r[q], nm_i[q], sgn);
                    asm volatile("" ::: "memory");
                }
                if (lane0) prow[M / 2] = ang(nh_r, nh_i, 1.0f);
            }
            auto replace = [](float& x_r, float& x_i, float t, float s) {
                const bool z = (x_r == 0.0f) && (x_i == 0.0f);
                // largest component below 2^-60: scaled by 2^100 first, so that |u|^2 of any nonzero X (denormals
                // included: |u| >= 2^-49) is a normal float above the 1e-37 floor and |Y| is T, not less
                const float sc = (fmaxf(fabsf(x_r), fabsf(x_i)) < 0x1p-60f) ? 0x1p100f : 1.0f;
                const float u_r = x_r * sc, u_i = x_i * sc;
                const float r = __builtin_amdgcn_rsqf(fmaxf(u_r * u_r + u_i * u_i, 1.0e-37f));
                x_r = z ? t * s : t * (u_r * r);
                x_i = z ? 0.0f : t * (u_i * r);
            };
            if constexpr (comp_compact<P>()) {   // kappa(lane) == lane: the synthesis-side twiddle is the conjugate of the split's
                const float4 pk = tw_half_pad<P>(w.tw, lane);
                ws_c = pk.x;
                ws_s = -pk.y;
            }
            float zr[HP], zi[HP];   // Z[M - k]
#pragma unroll
            for (int q = 0; q < HP; ++q) {
                const int k = lane + 64 * q;
                float x_r = no_r[q], x_i = no_i[q], p_r = nm_r[q], p_i = nm_i[q];
                replace(x_r, x_i, trow[k], sgn);
                replace(p_r, p_i, trow[M - k], sgn);
                if (q == 0) {   // DC and Nyquist: imaginary parts dropped (Q5)
                    x_i = lane0 ? 0.0f : x_i;
                    p_i = lane0 ? 0.0f : p_i;
                }
                merge_pair_step<P>(q, x_r, x_i, p_r, p_i, ws_c, ws_s, xr[q], xi[q], zr[q], zi[q]);
            }
            // bin M/2 (lane 0; M/2 = 32 P is even): Y, then Z = 2 conj(Y)
            replace(nh_r, nh_i, trow[M / 2], 1.0f);
            merge_handover<P>(zr, zi, 2.0f * nh_r, -2.0f * nh_i, xr, xi, lane);
        }
        pair_inverse_fft_front<P>(w, xr, xi, lane);
        if (nxt.valid) {
            g = frame_geom(sig, fpos[nxt.fi], fleft[nxt.fi], fright[nxt.fi], N);
            pair_stage_next<P>(w, g, lane);
        }
        pair_inverse_fft_back<P>(xr, xi);
        constexpr float kScale = 0.5f / (float)M;   // the inverse transform's scale, on the overlap-add's multiply-add
        auto plain_add = [](float o, float v, int) { return fmaf(v, kScale, o); };
        auto all_rows = [](int) { return true; };
        pair_ordered_ola<P, true>(w, cur, smem, runs, pm_rel, strips, pcm, xr, xi, lane, plain_add, all_rows);
        cur = nxt;
    }
}

}  // namespace mpx

using namespace mpx;

extern "C" {

int64_t mpx_spec_ld(int32_t n_bins) { return n_bins <= 0 ? 0 : ((int64_t)n_bins + 31) / 32 * 32; }

static int noise_stats_impl(void* stream, int fft_len, const void* tables, const float* noise, const int64_t* frame_pos,
                            const int32_t* frame_left, const int32_t* frame_right, const int32_t* frame_wtype,
                            int64_t n_frames, float* out_sum, float* spectra) {
    const int P = p_of(fft_len);
    if (!P) return fail(MPX_ERR_ARG, "mpx_noise_stats: fft_len must be 1024, 2048 or 4096%s");
    if (n_frames < 0) return fail(MPX_ERR_ARG, "mpx_noise_stats: negative n_frames%s");
    if (n_frames == 0) return MPX_OK;
    if (!tables || !noise || !frame_pos || !frame_left || !frame_right || !frame_wtype || !out_sum)
        return fail(MPX_ERR_ARG, "mpx_noise_stats: null pointer%s");
    const dim3 grid(grid_for(n_frames, kAnaWaves)), block(kAnaThreads);
    hipStream_t s = (hipStream_t)stream;
    if (P == 32) {
        if (int rc = set_lds(k_noise_stats<32>, lds_bytes_ana<32>())) return rc;
        hipLaunchKernelGGL(k_noise_stats<32>, grid, block, lds_bytes_ana<32>(), s, noise, (const long long*)frame_pos,
                           frame_left, frame_right, frame_wtype, (long long)n_frames, (const float*)tables, out_sum, spectra);
    } else if (P == 16) {
        if (int rc = set_lds(k_noise_stats<16>, lds_bytes_ana<16>())) return rc;
        hipLaunchKernelGGL(k_noise_stats<16>, grid, block, lds_bytes_ana<16>(), s, noise, (const long long*)frame_pos,
                           frame_left, frame_right, frame_wtype, (long long)n_frames, (const float*)tables, out_sum, spectra);
    } else {
        if (int rc = set_lds(k_noise_stats<8>, lds_bytes_ana<8>())) return rc;
        hipLaunchKernelGGL(k_noise_stats<8>, grid, block, lds_bytes_ana<8>(), s, noise, (const long long*)frame_pos,
                           frame_left, frame_right, frame_wtype, (long long)n_frames, (const float*)tables, out_sum, spectra);
    }
    MPX_HIP_CHECK(hipGetLastError());
    return MPX_OK;
}

int mpx_noise_stats(void* stream, int fft_len, const void* tables, const float* noise, const int64_t* frame_pos,
                    const int32_t* frame_left, const int32_t* frame_right, const int32_t* frame_wtype,
                    int64_t n_frames, float* out_sum) {
    return noise_stats_impl(stream, fft_len, tables, noise, frame_pos, frame_left, frame_right, frame_wtype, n_frames,
                            out_sum, nullptr);
}

int64_t mpx_noise_spectra_floats(int fft_len, int64_t n_frames) {
    return (fft_len == 4096 && n_frames > 0) ? n_frames * (int64_t)kSpecFrameFloats : 0;
}

int mpx_noise_stats_spectra(void* stream, int fft_len, const void* tables, const float* noise, const int64_t* frame_pos,
                            const int32_t* frame_left, const int32_t* frame_right, const int32_t* frame_wtype,
                            int64_t n_frames, float* out_sum, float* spectra) {
    if (fft_len != 4096) return fail(MPX_ERR_ARG, "mpx_noise_stats_spectra: fft_len must be 4096%s");
    if (!spectra && n_frames > 0) return fail(MPX_ERR_ARG, "mpx_noise_stats_spectra: null pointer%s");
    return noise_stats_impl(stream, fft_len, tables, noise, frame_pos, frame_left, frame_right, frame_wtype, n_frames,
                            out_sum, spectra);
}

int mpx_synth_comp_slots(void) { return device_cus() * kCompPairs; }

// Relative speed of the slots' wave pairs (see mpx_synth_ola_slot_weights): the pairs (0, 1), (2, 3), (4, 5) of a workgroup
// hold the oldest / middle / youngest wave of every SIMD.  12 waves, interleaved A/B of the configs[2] synthesis side:
// equal shares 1.332 ms, 100:80:60 1.301, 100:75:55 1.314, 100:90:80 1.287, 100:85:70 .. 100:88:76 1.270-1.277 (flat).
// Re-tuned on the final kernel (no scratch, more of its time in the VALU: the age effect is stronger): 100:86:73 1.190,
// 100:90:80 1.194, 100:92:86 1.215, 100:82:66 1.167, 100:84:62 1.168, 100:80:62 1.178, 100:78:58 1.177, 100:76:62 1.179.
#ifndef MPX_COMP_W0
#define MPX_COMP_W0 100
#endif
#ifndef MPX_COMP_W1
#define MPX_COMP_W1 (MPX_COMP_PAIR_WAVES > 8 ? 82 : 80)
#endif
#ifndef MPX_COMP_W2
#define MPX_COMP_W2 66
#endif
int mpx_synth_comp_slot_weights(float* weights_host, int32_t n_slots) {
    if (!weights_host || n_slots < 0) return fail(MPX_ERR_ARG, "mpx_synth_comp_slot_weights: bad arguments%s");
    for (int s = 0; s < n_slots; ++s) {
        const int age = ((s % kCompPairs) * 2) / 4;   // age rank of the pair's waves on their SIMDs
        weights_host[s] = (age == 0) ? (float)MPX_COMP_W0 : ((age == 1) ? (float)MPX_COMP_W1 : (float)MPX_COMP_W2);
    }
    return MPX_OK;
}

// T2: the type-2 arm of k_synth_comp_pair (mpx_synthesis_compressed_type2_ola); who: the entry's name for the messages
extern "C++" {
template <bool T2>
static int synthesis_compressed_ola_impl(const char* who, void* stream, int fft_len, const void* tables, const float* mag, const float* real,
                                 const float* imag, const float* noise, const int64_t* noise_pos,
                                 const int32_t* noise_left, const int32_t* noise_right, const int32_t* noise_wtype,
                                 const int32_t* voiced, const float* inv_gain, const int32_t* row0,
                                 const int32_t* row1, const float* row_t, const int32_t* win_left,
                                 const int32_t* win_right, const int32_t* pm_rel, const float* per_v,
                                 const float* ap_v, const float* ap_u, const mpx_ola_run* runs, int32_t n_runs,
                                 const int32_t* slot_off, const int32_t* slot_runs, int32_t n_slots,
                                 float* strips, float* pcm_out, int64_t ld, int32_t n_per_bins,
                                 const float* spectra) {
    const int P = p_of(fft_len);
    if (!P) return fail(MPX_ERR_ARG, "%s: fft_len must be 1024, 2048 or 4096", who);
    const int n_per = (n_per_bins <= 0 || n_per_bins > fft_len / 2 + 1) ? fft_len / 2 + 1 : (int)n_per_bins;
    if (n_runs < 0 || n_slots < 0) return fail(MPX_ERR_ARG, "%s: negative count", who);
    if (n_runs == 0 || n_slots == 0) return MPX_OK;
    if (!tables || !mag || !real || !imag || !noise || !noise_pos || !noise_left || !noise_right || !noise_wtype ||
        !voiced || !inv_gain || !win_left || !win_right || !pm_rel || !per_v || !ap_v ||
        !ap_u || !runs || !slot_off || !slot_runs || !strips || !pcm_out)
        return fail(MPX_ERR_ARG, "%s: null pointer", who);
    const bool lerp = row0 || row1 || row_t;   // all three null: one spectrum row per frame, row index = frame index
    if (lerp && (!row0 || !row1 || !row_t))
        return fail(MPX_ERR_ARG, "%s: row0 / row1 / row_t must be given together", who);
    CompFrameTabs tb{(const long long*)noise_pos, noise_left, noise_right, noise_wtype, voiced, inv_gain,
                     row0, row1, row_t, win_left, win_right, pm_rel, spectra};
    hipStream_t s = (hipStream_t)stream;
    const dim3 pgrid((n_slots + kCompPairs - 1) / kCompPairs), pblock(kCompPairWaves * 64);
    if (spectra) {   // stored noise spectra (mpx_noise_stats_spectra): N = 4096, one row per frame; never given for type 2
        if (P != 32 || lerp)
            return fail(MPX_ERR_ARG, "mpx_synthesis_compressed_ola_spectra: fft_len 4096 and one row per frame only%s");
        if (n_per <= 512) {
            if (int rc = set_lds(k_synth_comp_pair<32, false, 8, true>, lds_bytes_comp_pair<32>())) return rc;
            hipLaunchKernelGGL((k_synth_comp_pair<32, false, 8, true>), pgrid, pblock, lds_bytes_comp_pair<32>(),
                               s, mag, real, imag, noise, tb, per_v, ap_v, ap_u, (const RunDesc*)runs, slot_off, slot_runs,
                               (int)n_slots, (const float*)tables, strips, pcm_out, (long long)ld, n_per);
        } else {
            if (int rc = set_lds(k_synth_comp_pair<32, false, -1, true>, lds_bytes_comp_pair<32>())) return rc;
            hipLaunchKernelGGL((k_synth_comp_pair<32, false, -1, true>), pgrid, pblock, lds_bytes_comp_pair<32>(),
                               s, mag, real, imag, noise, tb, per_v, ap_v, ap_u, (const RunDesc*)runs, slot_off, slot_runs,
                               (int)n_slots, (const float*)tables, strips, pcm_out, (long long)ld, n_per);
        }
        MPX_HIP_CHECK(hipGetLastError());
        return MPX_OK;
    }
#define MPX_LAUNCH_COMP(PP, LL)                                                                                        \
    do {                                                                                                             \
        if (int rc = set_lds(k_synth_comp_pair<PP, LL, -1, false, T2>, lds_bytes_comp_pair<PP>())) return rc;        \
        hipLaunchKernelGGL((k_synth_comp_pair<PP, LL, -1, false, T2>), pgrid, pblock, lds_bytes_comp_pair<PP>(), s,  \
                           mag, real, imag,                                                                          \
                           noise, tb, per_v, ap_v, ap_u, (const RunDesc*)runs, slot_off, slot_runs, (int)n_slots,    \
                           (const float*)tables, strips, pcm_out, (long long)ld, n_per);                 \
    } while (0)
    if (lerp) {
        if (P == 32) MPX_LAUNCH_COMP(32, true);
        else if (P == 16) MPX_LAUNCH_COMP(16, true);
        else MPX_LAUNCH_COMP(8, true);
    } else {
        if (P == 32 && n_per <= 512) {   // the crossfade ends at or below bin 512 (48 / 44.1 kHz): the NPQ == 8 schedule
            if (int rc = set_lds(k_synth_comp_pair<32, false, 8, false, T2>, lds_bytes_comp_pair<32>())) return rc;
            hipLaunchKernelGGL((k_synth_comp_pair<32, false, 8, false, T2>), pgrid, pblock, lds_bytes_comp_pair<32>(), s, mag, real, imag,
                               noise, tb, per_v, ap_v, ap_u, (const RunDesc*)runs, slot_off, slot_runs, (int)n_slots,
                               (const float*)tables, strips, pcm_out, (long long)ld, n_per);
        } else if (P == 32) MPX_LAUNCH_COMP(32, false);
        else if (P == 16) MPX_LAUNCH_COMP(16, false);
        else MPX_LAUNCH_COMP(8, false);
    }
#undef MPX_LAUNCH_COMP
    MPX_HIP_CHECK(hipGetLastError());
    return MPX_OK;
}
}  // extern "C++"

int mpx_synthesis_compressed_ola(void* stream, int fft_len, const void* tables, const float* mag, const float* real,
                                 const float* imag, const float* noise, const int64_t* noise_pos,
                                 const int32_t* noise_left, const int32_t* noise_right, const int32_t* noise_wtype,
                                 const int32_t* voiced, const float* inv_gain, const int32_t* row0,
                                 const int32_t* row1, const float* row_t, const int32_t* win_left,
                                 const int32_t* win_right, const int32_t* pm_rel, const float* per_v,
                                 const float* ap_v, const float* ap_u, const mpx_ola_run* runs, int32_t n_runs,
                                 const int32_t* slot_off, const int32_t* slot_runs, int32_t n_slots,
                                 float* strips, float* pcm_out, int64_t ld, int32_t n_per_bins) {
    return synthesis_compressed_ola_impl<false>("mpx_synthesis_compressed_ola", stream, fft_len, tables, mag, real, imag, noise,
                                                noise_pos, noise_left, noise_right, noise_wtype, voiced, inv_gain, row0, row1,
                                                row_t, win_left, win_right, pm_rel, per_v, ap_v, ap_u, runs, n_runs, slot_off,
                                                slot_runs, n_slots, strips, pcm_out, ld, n_per_bins, nullptr);
}

int mpx_synthesis_compressed_type2_ola(void* stream, int fft_len, const void* tables, const float* mag, const float* real,
                                       const float* imag, const float* noise, const int64_t* noise_pos,
                                       const int32_t* noise_left, const int32_t* noise_right, const int32_t* noise_wtype,
                                       const int32_t* voiced, const float* inv_gain, const int32_t* row0,
                                       const int32_t* row1, const float* row_t, const int32_t* win_left,
                                       const int32_t* win_right, const int32_t* pm_rel, const float* per_v,
                                       const float* ap_v, const float* ap_u, const mpx_ola_run* runs, int32_t n_runs,
                                       const int32_t* slot_off, const int32_t* slot_runs, int32_t n_slots,
                                       float* strips, float* pcm_out, int64_t ld, int32_t n_per_bins) {
    return synthesis_compressed_ola_impl<true>("mpx_synthesis_compressed_type2_ola", stream, fft_len, tables, mag, real, imag,
                                               noise, noise_pos, noise_left, noise_right, noise_wtype, voiced, inv_gain, row0,
                                               row1, row_t, win_left, win_right, pm_rel, per_v, ap_v, ap_u, runs, n_runs,
                                               slot_off, slot_runs, n_slots, strips, pcm_out, ld, n_per_bins, nullptr);
}

int mpx_synthesis_compressed_ola_spectra(void* stream, int fft_len, const void* tables, const float* mag, const float* real,
                                 const float* imag, const float* noise, const int64_t* noise_pos,
                                 const int32_t* noise_left, const int32_t* noise_right, const int32_t* noise_wtype,
                                 const int32_t* voiced, const float* inv_gain, const int32_t* row0,
                                 const int32_t* row1, const float* row_t, const int32_t* win_left,
                                 const int32_t* win_right, const int32_t* pm_rel, const float* per_v,
                                 const float* ap_v, const float* ap_u, const mpx_ola_run* runs, int32_t n_runs,
                                 const int32_t* slot_off, const int32_t* slot_runs, int32_t n_slots,
                                 float* strips, float* pcm_out, int64_t ld, int32_t n_per_bins, const float* spectra) {
    if (!spectra && n_runs > 0 && n_slots > 0)
        return fail(MPX_ERR_ARG, "mpx_synthesis_compressed_ola_spectra: null pointer%s");
    return synthesis_compressed_ola_impl<false>("mpx_synthesis_compressed_ola_spectra", stream, fft_len, tables, mag, real,
                                                imag, noise, noise_pos, noise_left, noise_right, noise_wtype, voiced, inv_gain,
                                                row0, row1, row_t, win_left, win_right, pm_rel, per_v, ap_v, ap_u, runs, n_runs,
                                                slot_off, slot_runs, n_slots, strips, pcm_out, ld, n_per_bins, spectra);
}

// Slot weights of k_roundtrip_pair (see mpx_synth_comp_slot_weights: pairs of the oldest / middle / youngest waves of the
// SIMDs).  Interleaved sweeps of the configs[1] step on two boxes: equal shares 0.592 ms, 100:90:80 0.574, 100:86:73 0.567,
// 100:82:66 0.555, 100:72:60 0.547, 100:75:55 0.539-0.545; a smallest share below ~25 frames per run (100:70:48, 100:78:50)
// fell off a cliff (0.80 ms) while the planner DROPPED cuts that would let non-adjacent runs overlap (runs shorter than
// fft_len output samples: one slot idle, its neighbour with twice the frames).  It now moves such a cut forward
// (hostmath._enforce_span); on that planner, another box: 100:77:58 0.522, 100:75:55 0.523, 100:72:52 0.512, 100:71:49 0.511,
// 100:68:46 0.516, 100:65:42 0.527, 100:60:38 0.548 -- the per-frame times by age (tools/roundtrip_phase_probe.py: 22.5 /
// 31.6 / 46.3 us) say 100:71:49.
#ifndef MPX_RT_W1
#define MPX_RT_W1 71
#endif
#ifndef MPX_RT_W2
#define MPX_RT_W2 50
#endif
int mpx_roundtrip_slot_weights(float* weights_host, int32_t n_slots) {
    if (!weights_host || n_slots < 0) return fail(MPX_ERR_ARG, "mpx_roundtrip_slot_weights: bad arguments%s");
    for (int s = 0; s < n_slots; ++s) {
        const int age = ((s % kCompPairs) * 2) / 4;
        weights_host[s] = (age == 0) ? 100.0f : ((age == 1) ? (float)MPX_RT_W1 : (float)MPX_RT_W2);
    }
    return MPX_OK;
}

// Cost model of k_roundtrip_pair's frames, for the planner that deals them to the slots (hostmath.deal_cuts /
// mpx_host_deal_cuts): frame f costs slot s  a_s + b_s rows_f + c_s extra_f  with (1, rows_f, extra_f) = frame_cost_terms --
// the rows noise_fft's gather visits and the tiles it stages synchronously, counted by the functions the kernel itself
// calls -- and (a, b, c) by the age class of the slot's wave pair (the rule of mpx_roundtrip_slot_weights).  Unit: 10 ns of
// wall clock per frame of the pair's share (its two waves alternate over the share).  Uncalibrated, a = 100 / 141 / 200 and
// b = c = 0 deal by frame count in the proportions of MPX_RT_W1 / MPX_RT_W2 = 71 / 50.
#ifndef MPX_RT_COST_A0
#define MPX_RT_COST_A0 793
#endif
#ifndef MPX_RT_COST_A1
#define MPX_RT_COST_A1 1039
#endif
#ifndef MPX_RT_COST_A2
#define MPX_RT_COST_A2 1514
#endif
#ifndef MPX_RT_COST_B0
#define MPX_RT_COST_B0 14
#endif
#ifndef MPX_RT_COST_B1
#define MPX_RT_COST_B1 16
#endif
#ifndef MPX_RT_COST_B2
#define MPX_RT_COST_B2 15
#endif
#ifndef MPX_RT_COST_C0
#define MPX_RT_COST_C0 0
#endif
#ifndef MPX_RT_COST_C1
#define MPX_RT_COST_C1 0
#endif
#ifndef MPX_RT_COST_C2
#define MPX_RT_COST_C2 0
#endif
int mpx_roundtrip_slot_costs(int32_t* coef_host, int32_t n_slots) {
    if (!coef_host || n_slots < 0) return fail(MPX_ERR_ARG, "mpx_roundtrip_slot_costs: bad arguments%s");
    static const int32_t kCost[3][3] = {{MPX_RT_COST_A0, MPX_RT_COST_B0, MPX_RT_COST_C0},
                                        {MPX_RT_COST_A1, MPX_RT_COST_B1, MPX_RT_COST_C1},
                                        {MPX_RT_COST_A2, MPX_RT_COST_B2, MPX_RT_COST_C2}};
    for (int s = 0; s < n_slots; ++s) {
        const int age = ((s % kCompPairs) * 2) / 4;
        for (int k = 0; k < 3; ++k) coef_host[3 * s + k] = kCost[age][k];
    }
    return MPX_OK;
}

int mpx_roundtrip_frame_terms(int fft_len, const int32_t* frame_left, const int32_t* frame_right, int64_t n_frames,
                              int32_t* terms_host) {
    const int P = p_of(fft_len);
    if (!P) return fail(MPX_ERR_ARG, "mpx_roundtrip_frame_terms: fft_len must be 1024, 2048 or 4096%s");
    if (n_frames < 0 || (n_frames > 0 && (!frame_left || !frame_right || !terms_host)))
        return fail(MPX_ERR_ARG, "mpx_roundtrip_frame_terms: bad arguments%s");
    const bool compact = (P == 32) && comp_compact<32>();   // the kernel's own choice of tile
    for (int64_t f = 0; f < n_frames; ++f) {
        int t[3];
        frame_cost_terms(frame_left[f], frame_right[f], fft_len, P, compact, t);
        terms_host[3 * f + 0] = t[0];
        terms_host[3 * f + 1] = t[1];
        terms_host[3 * f + 2] = t[2];
    }
    return MPX_OK;
}

#ifdef MPX_PROBE_ENDTIME
int mpx_probe_rt_endtimes(unsigned long long* host, int n_words) {   // probe builds only (not part of the ABI)
    if (!host || n_words < 0 || n_words > 4 * 8192) return fail(MPX_ERR_ARG, "mpx_probe_rt_endtimes: bad arguments%s");
    MPX_HIP_CHECK(hipDeviceSynchronize());
    MPX_HIP_CHECK(hipMemcpyFromSymbol(host, HIP_SYMBOL(g_rt_endprobe), sizeof(unsigned long long) * (size_t)n_words));
    return MPX_OK;
}
#endif

int mpx_roundtrip_support_classes(int fft_len, const int32_t* frame_left, const int32_t* frame_right, int64_t n_frames,
                                  int32_t* class_host) {
    if (!p_of(fft_len)) return fail(MPX_ERR_ARG, "mpx_roundtrip_support_classes: fft_len must be 1024, 2048 or 4096%s");
    if (n_frames < 0 || (n_frames > 0 && (!frame_left || !frame_right || !class_host)))
        return fail(MPX_ERR_ARG, "mpx_roundtrip_support_classes: bad arguments%s");
    for (int64_t f = 0; f < n_frames; ++f) class_host[f] = frame_support_class(frame_left[f], frame_right[f], fft_len);
    return MPX_OK;
}

// The flags of mpx_roundtrip_lossless_ola_flags; the store bits change nothing about what a frame adds to the ring, so
// mpx_roundtrip_frame_extents takes the same word and ignores them.
// Neither does MPX_RT_INVERSE_TRANSFORM: both arms add the same rows of a frame.
static constexpr uint32_t kRtFlagsKnown = MPX_RT_FULL_SUPPORT | MPX_RT_STORE_ROWS | MPX_RT_STORE_NT | MPX_RT_INVERSE_TRANSFORM;

// The row float every lane writes in every store of one plane of one frame, for a row of phase `phase`, from the helpers
// the kernel's line-aligned forms take their bases and predicates from (mpx_common.hpp, "Row stores by line").
int mpx_roundtrip_store_map(int fft_len, int phase, int32_t* out) {
    if (fft_len != 4096) return fail(MPX_ERR_ARG, "mpx_roundtrip_store_map: only fft_len 4096 has the line-aligned stores%s");
    if (phase < 0 || phase > 31 || !out) return fail(MPX_ERR_ARG, "mpx_roundtrip_store_map: bad arguments%s");
    const int P = p_of(fft_len);
    for (int st = 0; st < row_store_count(P); ++st)
        for (int lane = 0; lane < 64; ++lane) out[64 * st + lane] = row_store_index(st, lane, phase, P);
    return MPX_OK;
}

// What the instance that mpx_roundtrip_lossless_ola_flags launches for (fft_len, flags) can add to the ring, per frame: the
// samples of the rows support_row_live names for a frame the kernel takes as narrow, the whole frame otherwise -- and the
// whole frame throughout where that instance has no pruned passes (the launch's own choice of CLS, roundtrip_prunes).
int mpx_roundtrip_frame_extents(int fft_len, const int32_t* frame_left, const int32_t* frame_right, int64_t n_frames,
                                uint32_t flags, int32_t* extents_host) {
    if (flags & ~kRtFlagsKnown) return fail(MPX_ERR_ARG, "mpx_roundtrip_frame_extents: unknown flag%s");
    const int P = p_of(fft_len);
    if (!P) return fail(MPX_ERR_ARG, "mpx_roundtrip_frame_extents: fft_len must be 1024, 2048 or 4096%s");
    if (n_frames < 0 || (n_frames > 0 && (!frame_left || !frame_right || !extents_host)))
        return fail(MPX_ERR_ARG, "mpx_roundtrip_frame_extents: bad arguments%s");
    const bool cls = (P == 32) && !(flags & MPX_RT_FULL_SUPPORT);   // MPX_LAUNCH_RT's choice below
    const bool prunes = (P == 32) && roundtrip_prunes<32>(cls);
    int n_lo = fft_len, n_hi = 0;   // the samples of the narrow class's live rows
    for (int q = 0; q < P; ++q)
        if (support_row_live(q, kSupportNarrow, P)) {
            n_lo = (128 * q < n_lo) ? 128 * q : n_lo;
            n_hi = (128 * q + 128 > n_hi) ? 128 * q + 128 : n_hi;
        }
    for (int64_t f = 0; f < n_frames; ++f) {
        const bool narrow = prunes && (MPX_RT_FORCE_NARROW ||
                                       frame_support_class(frame_left[f], frame_right[f], fft_len) == kSupportNarrow);
        extents_host[2 * f + 0] = narrow ? n_lo : 0;
        extents_host[2 * f + 1] = narrow ? n_hi : fft_len;
    }
    return MPX_OK;
}

int mpx_roundtrip_lossless_ola(void* stream, int fft_len, const void* tables, const float* sig, const int64_t* frame_pos,
                               const int32_t* frame_left, const int32_t* frame_right, int64_t n_frames,
                               const mpx_ola_run* runs, int32_t n_runs, const int32_t* slot_off, const int32_t* slot_runs,
                               int32_t n_slots, const int32_t* pm_rel, float* out_mag, float* out_real, float* out_imag,
                               float* strips, float* pcm_out, int64_t ld) {
    return mpx_roundtrip_lossless_ola_flags(stream, fft_len, tables, sig, frame_pos, frame_left, frame_right, n_frames, runs,
                                            n_runs, slot_off, slot_runs, n_slots, pm_rel, out_mag, out_real, out_imag, strips,
                                            pcm_out, ld, 0u);
}

int mpx_roundtrip_lossless_ola_flags(void* stream, int fft_len, const void* tables, const float* sig,
                                     const int64_t* frame_pos, const int32_t* frame_left, const int32_t* frame_right,
                                     int64_t n_frames, const mpx_ola_run* runs, int32_t n_runs, const int32_t* slot_off,
                                     const int32_t* slot_runs, int32_t n_slots, const int32_t* pm_rel, float* out_mag,
                                     float* out_real, float* out_imag, float* strips, float* pcm_out, int64_t ld,
                                     uint32_t flags) {
    if (flags & ~kRtFlagsKnown) return fail(MPX_ERR_ARG, "mpx_roundtrip_lossless_ola: unknown flag%s");
    if ((flags & MPX_RT_STORE_ROWS) && (flags & MPX_RT_STORE_NT))
        return fail(MPX_ERR_ARG, "mpx_roundtrip_lossless_ola: MPX_RT_STORE_NT needs the line-aligned stores%s");
    const int P = p_of(fft_len);
    if (!P) return fail(MPX_ERR_ARG, "mpx_roundtrip_lossless_ola: fft_len must be 1024, 2048 or 4096%s");
    if (n_frames < 0 || n_runs < 0 || n_slots < 0) return fail(MPX_ERR_ARG, "mpx_roundtrip_lossless_ola: negative count%s");
    if (ld < fft_len / 2 + 1) return fail(MPX_ERR_ARG, "mpx_roundtrip_lossless_ola: ld < fft_len/2 + 1%s");
    if (n_frames == 0 || n_runs == 0 || n_slots == 0) return MPX_OK;
    if (!tables || !sig || !frame_pos || !frame_left || !frame_right || !runs || !slot_off || !slot_runs || !pm_rel ||
        !out_mag || !out_real || !out_imag || !strips || !pcm_out)
        return fail(MPX_ERR_ARG, "mpx_roundtrip_lossless_ola: null pointer%s");
    hipStream_t s = (hipStream_t)stream;
    const dim3 pgrid((n_slots + kCompPairs - 1) / kCompPairs), pblock(kCompPairWaves * 64);
#define MPX_LAUNCH_RT(PP, CLS) MPX_LAUNCH_RT_K(PP, (k_roundtrip_pair<PP, CLS>))
#define MPX_LAUNCH_RT_K(PP, KERNEL)                                                                                    \
    do {                                                                                                             \
        auto KK = KERNEL;                                                                                            \
        if (int rc = set_lds(KK, lds_bytes_comp_pair<PP>())) return rc;                                              \
        hipLaunchKernelGGL(KK, pgrid, pblock, lds_bytes_comp_pair<PP>(), s, sig,                                     \
                           (const long long*)frame_pos, frame_left, frame_right, (const RunDesc*)runs, slot_off,     \
                           slot_runs, (int)n_slots, pm_rel, (const float*)tables, out_mag, out_real, out_imag, strips, \
                           pcm_out, (long long)ld);                                                                  \
    } while (0)
    // support classes (k_roundtrip_pair's CLS): only N = 4096 has a narrow class
    // store forms (k_roundtrip_pair's ST): only that instance has the line-aligned ones, every other ignores the bits
    // arms (k_roundtrip_pair's DIRECT): only N = 4096 has the direct one, every other N ignores the bit
    if constexpr (kRtDirectBuilt) {
        if (P == 32 && !(flags & MPX_RT_INVERSE_TRANSFORM)) {
            if (flags & MPX_RT_FULL_SUPPORT) MPX_LAUNCH_RT_K(32, (k_roundtrip_pair<32, false, kStoreRows, true>));
            else if (flags & MPX_RT_STORE_ROWS) MPX_LAUNCH_RT_K(32, (k_roundtrip_pair<32, true, kStoreRows, true>));
            else if (flags & MPX_RT_STORE_NT) MPX_LAUNCH_RT_K(32, (k_roundtrip_pair<32, true, kStoreLinesNT, true>));
            else MPX_LAUNCH_RT_K(32, (k_roundtrip_pair<32, true, kStoreLines, true>));
            MPX_HIP_CHECK(hipGetLastError());
            return MPX_OK;
        }
    }
    if (P == 32 && !(flags & MPX_RT_FULL_SUPPORT)) {
        if (flags & MPX_RT_STORE_ROWS) MPX_LAUNCH_RT(32, true);
        else if (flags & MPX_RT_STORE_NT) MPX_LAUNCH_RT_K(32, (k_roundtrip_pair<32, true, kStoreLinesNT>));
        else MPX_LAUNCH_RT_K(32, (k_roundtrip_pair<32, true, kStoreLines>));
    } else if (P == 32) MPX_LAUNCH_RT(32, false);
    else if (P == 16) MPX_LAUNCH_RT(16, false);
    else MPX_LAUNCH_RT(8, false);
#undef MPX_LAUNCH_RT
#undef MPX_LAUNCH_RT_K
    MPX_HIP_CHECK(hipGetLastError());
    return MPX_OK;
}

int mpx_griffin_lim_ola(void* stream, int fft_len, const void* tables, const float* sig_in, const int64_t* frame_pos,
                        const int32_t* frame_left, const int32_t* frame_right, int64_t n_frames, const float* target_mag,
                        const mpx_ola_run* runs, int32_t n_runs, const int32_t* slot_off, const int32_t* slot_runs,
                        int32_t n_slots, const int32_t* pm_rel, float* phase_out, float* strips, float* sig_out,
                        int64_t ld) {
    const int P = p_of(fft_len);
    if (!P) return fail(MPX_ERR_ARG, "mpx_griffin_lim_ola: fft_len must be 1024, 2048 or 4096%s");
    if (n_frames < 0 || n_runs < 0 || n_slots < 0) return fail(MPX_ERR_ARG, "mpx_griffin_lim_ola: negative count%s");
    if (ld < fft_len / 2 + 1) return fail(MPX_ERR_ARG, "mpx_griffin_lim_ola: ld < fft_len/2 + 1%s");
    if (n_frames == 0 || n_runs == 0 || n_slots == 0) return MPX_OK;
    if (!tables || !sig_in || !frame_pos || !frame_left || !frame_right || !target_mag || !runs || !slot_off ||
        !slot_runs || !pm_rel || !strips || !sig_out)
        return fail(MPX_ERR_ARG, "mpx_griffin_lim_ola: null pointer%s");
    if (sig_in == sig_out) return fail(MPX_ERR_ARG, "mpx_griffin_lim_ola: sig_in and sig_out must be different buffers%s");
    hipStream_t s = (hipStream_t)stream;
    const dim3 pgrid((n_slots + kCompPairs - 1) / kCompPairs), pblock(kCompPairWaves * 64);
#define MPX_LAUNCH_GL(PP)                                                                                              \
    do {                                                                                                             \
        auto KK = k_griffin_lim_pair<PP>;                                                                            \
        if (int rc = set_lds(KK, lds_bytes_comp_pair<PP>())) return rc;                                              \
        hipLaunchKernelGGL(KK, pgrid, pblock, lds_bytes_comp_pair<PP>(), s, sig_in,                                  \
                           (const long long*)frame_pos, frame_left, frame_right, (const RunDesc*)runs, slot_off,     \
                           slot_runs, (int)n_slots, pm_rel, (const float*)tables, target_mag, phase_out, strips,     \
                           sig_out, (long long)ld);                                                                  \
    } while (0)
    if (P == 32) MPX_LAUNCH_GL(32);
    else if (P == 16) MPX_LAUNCH_GL(16);
    else MPX_LAUNCH_GL(8);
#undef MPX_LAUNCH_GL
    MPX_HIP_CHECK(hipGetLastError());
    return MPX_OK;
}

int mpx_min_phase(void* stream, int fft_len, const void* tables, const float* mag, const int32_t* row0,
                  const int32_t* row1, const float* row_t, int64_t n_frames, float* out_mag, float* out_real,
                  float* out_imag, int64_t ld) {
    const int P = p_of(fft_len);
    if (!P) return fail(MPX_ERR_ARG, "mpx_min_phase: fft_len must be 1024, 2048 or 4096%s");
    if (n_frames < 0) return fail(MPX_ERR_ARG, "mpx_min_phase: negative n_frames%s");
    if (n_frames == 0) return MPX_OK;
    if (!tables || !mag || !row0 || !row1 || !row_t || !out_mag || !out_real || !out_imag)
        return fail(MPX_ERR_ARG, "mpx_min_phase: null pointer%s");
    const dim3 grid(grid_for(n_frames)), block(kThreads);
    hipStream_t s = (hipStream_t)stream;
    if (P == 32) {
        if (int rc = set_lds(k_min_phase<32>, lds_bytes<32>())) return rc;
        hipLaunchKernelGGL(k_min_phase<32>, grid, block, lds_bytes<32>(), s, mag, row0, row1, row_t,
                           (long long)n_frames, (const float*)tables, out_mag, out_real, out_imag, (long long)ld);
    } else if (P == 16) {
        if (int rc = set_lds(k_min_phase<16>, lds_bytes<16>())) return rc;
        hipLaunchKernelGGL(k_min_phase<16>, grid, block, lds_bytes<16>(), s, mag, row0, row1, row_t,
                           (long long)n_frames, (const float*)tables, out_mag, out_real, out_imag, (long long)ld);
    } else {
        if (int rc = set_lds(k_min_phase<8>, lds_bytes<8>())) return rc;
        hipLaunchKernelGGL(k_min_phase<8>, grid, block, lds_bytes<8>(), s, mag, row0, row1, row_t,
                           (long long)n_frames, (const float*)tables, out_mag, out_real, out_imag, (long long)ld);
    }
    MPX_HIP_CHECK(hipGetLastError());
    return MPX_OK;
}

int mpx_noise_gains(void* stream, const float* sums, const int32_t* voiced, const int32_t* utt_frame_off,
                    int32_t n_utts, int32_t bins_per_frame, float* inv_gain, double* gains) {
    if (n_utts < 0 || bins_per_frame <= 0) return fail(MPX_ERR_ARG, "mpx_noise_gains: bad size%s");
    if (n_utts == 0) return MPX_OK;
    if (!sums || !voiced || !utt_frame_off || !inv_gain) return fail(MPX_ERR_ARG, "mpx_noise_gains: null pointer%s");
    hipLaunchKernelGGL(k_noise_gains, dim3((unsigned)n_utts), dim3(256), 0, (hipStream_t)stream, sums, voiced,
                       utt_frame_off, (int)bins_per_frame, inv_gain, gains);
    MPX_HIP_CHECK(hipGetLastError());
    return MPX_OK;
}

}  // extern "C"
