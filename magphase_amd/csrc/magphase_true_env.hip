// magphase_true_env.hip -- true-envelope spectral estimation (la.true_envelope, libaudio.py:295-340).
//
//   k_true_envelope<P>   per frame (one wavefront): to dB in the load -> up to max_iters smoothing passes, each
//                        even extension -> real IFFT -> cepstral weights w[n] -> real FFT (la.spectral_smoothing_rceps,
//                        libaudio.py:203-238), the mean-abs stop rule and v = max(v, sm), all in registers -> back
//                        from dB in the store.  DESIGN.md section 3.3d.
#include "mpx_common.hpp"

namespace mpx {

// Cepstral weight table in LDS: one padded row per lane in register order, entry i = (w[n0], w[n0 + 1]) with
// n0 = 2 (kappa(lane) + 64 brev(i)) -- the cepstrum samples the lane holds after the inverse transform -- so that a lane
// reads its 2P weights as P/2 ds_read_b128 (rows padded like the twiddle table: conflict-free across lanes).
template <int P>
constexpr int te_w_stride() { return 2 * P + 4; }
template <int P>
constexpr int te_w_floats() { return 64 * te_w_stride<P>(); }
template <int P>
constexpr size_t te_lds_bytes() {
    return sizeof(float) * (size_t)(tw_floats<P>() + te_w_floats<P>() + kWavesPerBlock * P * kXStride);
}

// in_type of mpx_true_envelope: 0 'abs' (20 log10 x), 1 'db' (x), 2 'log' ((20 / ln 10) x); in_type is uniform
template <int P>
__device__ __forceinline__ void te_to_db(float (&v)[P], float& vM, int in_type) {
    if (in_type == 0) {
#pragma unroll
        for (int j = 0; j < P; ++j) v[j] = 20.0f * log10f(v[j]);
        vM = 20.0f * log10f(vM);
    } else if (in_type == 2) {
#pragma unroll
        for (int j = 0; j < P; ++j) v[j] *= 8.68588963806503655f;
        vM *= 8.68588963806503655f;
    }
}
template <int P>
__device__ __forceinline__ void te_from_db(float (&v)[P], float& vM, int in_type) {
    if (in_type == 0) {
#pragma unroll
        for (int j = 0; j < P; ++j) v[j] = exp10f(0.05f * v[j]);
        vM = exp10f(0.05f * vM);
    } else if (in_type == 2) {
#pragma unroll
        for (int j = 0; j < P; ++j) v[j] *= 0.115129254649702284f;
        vM *= 0.115129254649702284f;
    }
}

// hermitian_merge (mpx_common.hpp) for a REAL half spectrum x (lane l, register j <-> bin l + 64 j, pre-scaled; xm =
// Nyquist bin on lane 0): with Im X = 0, E = X + Xp and T = X - Xp are real, Z = E - Im(W) T + i Re(W) T -- half the
// partner exchanges and no imaginary input registers.
template <int P>
__device__ __forceinline__ void hermitian_merge_real(const float (&x)[P], float xm, float (&zr)[P], float (&zi)[P],
                                                     int lane, float wl_c, float wl_s) {
    const int src_lane = (64 - lane) & 63;
    const bool lane0 = (lane == 0);
#pragma unroll
    for (int j = 0; j < P; ++j) zi[j] = __shfl(x[P - 1 - j], src_lane);
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const float p = lane0 ? ((j == 0) ? xm : x[(P - j) % P]) : zi[j];
        const float e = x[j] + p, t = x[j] - p;
        const float cq = cos2p<P>(j), sq = sin2p<P>(j);
        const float wr = wl_c * cq - wl_s * sq, wi = wl_c * sq + wl_s * cq;
        zr[j] = fmaf(-wi, t, e);
        zi[j] = wr * t;
    }
}

// One smoothing pass on the half spectrum v (lane l, register j <-> bin l + 64 j; vM = Nyquist bin on lane 0):
// sm = Re FFT(w . IFFT(even extension of v))[0..M], returned in the same layout.
template <int P>
__device__ __forceinline__ void te_smooth(const float (&v)[P], float vM, float (&sm)[P], float& smM, const float* tw,
                                          const float* wrow, float* xbuf, int lane, int kap, int src_lane, float ws_c,
                                          float ws_s, float wa_c, float wa_s) {
    constexpr int M = 64 * P, LB = ilog2(P);
    const float scale = 0.5f / (float)M;
    // opaque per pass: otherwise the compiler hoists the 4P lane twiddles of the merge and the split out of the pass
    // loop and spills them (as k_min_phase does per frame)
    asm volatile("" : "+v"(lane), "+v"(kap), "+v"(src_lane), "+v"(ws_c), "+v"(ws_s), "+v"(wa_c), "+v"(wa_s));
    float xr[P], xi[P];
#pragma unroll
    for (int j = 0; j < P; ++j) sm[j] = v[j] * scale;   // sm: scratch registers until the split writes it
    hermitian_merge_real<P>(sm, vM * scale, xr, xi, lane, ws_c, ws_s);
    wave_fft<P, +1>(xr, xi, tw, xbuf, lane);
    // ---- real cepstrum c[n0], c[n0 + 1] (n0 = 2 (kap + 64 brev(i))) times the weights
    const float4* wq = reinterpret_cast<const float4*>(wrow);
#pragma unroll
    for (int i = 0; i < P; i += 2) {
        const float4 q = wq[i / 2];
        xr[i] *= q.x;
        xi[i] *= q.y;
        xr[i + 1] *= q.z;
        xi[i + 1] *= q.w;
    }
    // ---- forward real FFT of the weighted cepstrum: input register j must hold z[lane + 64 j] (as k_min_phase)
    float re[P], im[P];
#pragma unroll
    for (int i = 0; i < P; ++i) {
        re[brev(i, LB)] = xr[i];
        im[brev(i, LB)] = xi[i];
    }
    if (P != 32) {
#pragma unroll
        for (int j = 0; j < P; ++j) {
            re[j] = __shfl(re[j], kap);
            im[j] = __shfl(im[j], kap);
        }
    }
    wave_fft<P, -1>(re, im, tw, xbuf, lane);
    // ---- split: Re S[k] = Re E[k] + Re(W_N^k O[k]) for k = kap + 64 q, stored in register q
    const bool lane0 = (kap == 0);
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
            const float er = 0.5f * (re[i] + pr);
            const float orr = 0.5f * (im[i] + pi), oi = -0.5f * (re[i] - pr);
            const float cq = cos2p<P>(q), sq = -sin2p<P>(q);
            const float wr = wa_c * cq - wa_s * sq, wi = wa_c * sq + wa_s * cq;
            sm[q] = er + (wr * orr - wi * oi);
        }
    }
    smM = re[0] - im[0];   // S[M] = Re Z[0] - Im Z[0] (meaningful on lane 0, where Z[0] is)
    // ---- lane l register q holds bin kappa(l) + 64 q: back to bin l + 64 q (kappa is an involution)
    if (P != 32) {
#pragma unroll
        for (int q = 0; q < P; ++q) sm[q] = __shfl(sm[q], kap);
    }
}

// Sum over the wave by an xor butterfly: lane l adds s_l + s_{l^m}, its partner s_{l^m} + s_l -- the same float, so
// every lane ends with the same value.
__device__ __forceinline__ float te_wave_sum(float s) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
    return s;
}

// ---------------------------------------------------------------------------------------------
// One wavefront per frame; frames by grid stride (TICKET = false) or by a device ticket counter (TICKET = true: one
// atomicAdd per frame from lane 0, the next ticket taken while the current frame runs).  thres_sum = thres_db * H: the
// reference's mean(|v - sm|) < thres_db as sum < thres_db * H (sum in fp32).  forced (optional): run
// exactly clamp(forced[f], 1, max_iters) passes, no stop test.  A frame whose dB values are not all finite (a zero,
// negative or non-finite magnitude for 'abs') is written as NaN without passes, like the reference's all-NaN row.
// ---------------------------------------------------------------------------------------------
template <int P, bool TICKET>
__global__ __launch_bounds__(kThreads) void k_true_envelope(const float* __restrict__ x, long long ldx,
                                                            long long nframes, const float* __restrict__ tw_g,
                                                            const float* __restrict__ w_g, int in_type,
                                                            float thres_sum, int max_iters,
                                                            const int* __restrict__ forced, float* __restrict__ out,
                                                            long long ldo, int* __restrict__ iters_out,
                                                            int* __restrict__ ticket) {
    constexpr int M = 64 * P, LB = ilog2(P), WS = te_w_stride<P>();
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* tw = smem;
    float* wl = smem + tw_floats<P>();
    const int lane_id = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    float* xbuf = wl + te_w_floats<P>() + wave * (P * kXStride);
    for (int i = threadIdx.x; i < tw_floats<P>(); i += kThreads) tw[i] = tw_g[i];
    for (int e = threadIdx.x; e < 64 * P; e += kThreads) {
        const int l = e / P, i = e % P;
        const int n0 = 2 * (kappa<P>(l) + 64 * brev(i, LB));
        wl[l * WS + 2 * i] = w_g[n0];
        wl[l * WS + 2 * i + 1] = w_g[n0 + 1];
    }
    __syncthreads();
    const int kap = kappa<P>(lane_id);
    const int src_lane = kappa<P>((64 - kap) & 63);
    float wa_s, wa_c, ws_s, ws_c;
    sincospif(-2.0f * (float)kap / (float)(2 * M), &wa_s, &wa_c);
    sincospif(2.0f * (float)lane_id / (float)(2 * M), &ws_s, &ws_c);
    const float* wrow = wl + lane_id * WS;

    auto take = [&]() -> long long {
        int t = 0;
        if (lane_id == 0) t = atomicAdd(ticket, 1);
        return (long long)rfl(__shfl(t, 0));
    };
    long long f = TICKET ? take() : (long long)blockIdx.x * kWavesPerBlock + rfl(wave);
    while (f < nframes) {
        const long long f_next = TICKET ? take() : f + (long long)gridDim.x * kWavesPerBlock;
        int lane = lane_id;
        asm volatile("" : "+v"(lane));
        const float* xp = x + f * ldx;
        float v[P], sm[P];
        float vM = 0.0f, smM = 0.0f;
        bool bad = false;
#pragma unroll
        for (int j = 0; j < P; ++j) v[j] = xp[lane + 64 * j];
        if (lane == 0) vM = xp[M];
        te_to_db<P>(v, vM, in_type);
#pragma unroll
        for (int j = 0; j < P; ++j) bad |= !isfinite(v[j]);
        if (lane == 0) bad |= !isfinite(vM);
        const int n_fixed = forced ? min(max(forced[f], 1), max_iters) : 0;
        int it = n_fixed ? n_fixed : max_iters;
        if (__ballot(bad) != 0) {
#pragma unroll
            for (int j = 0; j < P; ++j) sm[j] = __builtin_nanf("");
            smM = __builtin_nanf("");
        } else {
            for (int pass = 1;; ++pass) {
                te_smooth<P>(v, vM, sm, smM, tw, wrow, xbuf, lane, kap, src_lane, ws_c, ws_s, wa_c, wa_s);
                bool stop = (pass >= it);
                if (!n_fixed) {
                    float d = (lane == 0) ? fabsf(vM - smM) : 0.0f;
#pragma unroll
                    for (int j = 0; j < P; ++j) d += fabsf(v[j] - sm[j]);
                    d = __int_as_float(rfl(__float_as_int(te_wave_sum(d))));
                    stop = stop || (d < thres_sum);
                }
                if (stop) {
                    it = pass;
                    break;
                }
#pragma unroll
                for (int j = 0; j < P; ++j) v[j] = fmaxf(v[j], sm[j]);
                vM = fmaxf(vM, smM);
            }
        }
        te_from_db<P>(sm, smM, in_type);
        float* op = out + f * ldo;
#pragma unroll
        for (int j = 0; j < P; ++j) op[lane + 64 * j] = sm[j];
        if (lane == 0) {
            op[M] = smM;
            if (iters_out) iters_out[f] = it;
        }
        f = f_next;
    }
}

// ---------------------------------------------------------------------------------------------
// k_true_envelope_bwd<P>: the exact adjoint of k_true_envelope as the device decided it.
// One wavefront per frame, in the register layout above.  The K = clamp(iters[f], 1, max_iters) passes are recomputed
// with the same te_smooth; pass k < K records m_k[b] = (s_k[b] > a_k[b]) -- where fmaxf takes the smoothed value; a tie
// keeps a -- as one bit per held bin in a per-wave LDS history (32 / P passes per word and lane; the Nyquist bin one word
// per pass).  Then, with S^T g = D^-1 S (D g), D = diag(2, 1, ..., 1, 2):
//     g_s = g_y dy/ds_K;  g_a = 0;  for k = K .. 1: g_a += S^T g_s;  if k > 1: (g_s, g_a) = m_{k-1} ? (g_a, 0) : (0, g_a)
// and the dB chain rule in the store.  The stop test is not differentiated.  A frame the forward wrote as NaN gets a zero
// gradient row.  decisions / env_out (optional, tests): the bits as int32 [nframes x max_iters x (2P + 1)] (bit b % 32 of
// word b / 32 of pass k's words = m_k[b]; zero for the passes that decide nothing) and the recomputed envelope rows.
// ---------------------------------------------------------------------------------------------
constexpr int kTeBwdMaxPasses = 100;   // capacity of the decision history (la.true_envelope's n_maxiter)
template <int P>
constexpr int te_bwd_waves() { return P == 32 ? 3 : 8; }   // what fits the 160 KiB of a CU with a full history
template <int P>
constexpr int te_hist_words() { return ((kTeBwdMaxPasses + 32 / P - 1) / (32 / P)) * 64; }
template <int P>
constexpr int te_bwd_wave_floats() { return P * kXStride + te_hist_words<P>() + kTeBwdMaxPasses; }
template <int P>
constexpr size_t te_bwd_lds_bytes() {
    return sizeof(float) * (size_t)(tw_floats<P>() + te_w_floats<P>() + te_bwd_waves<P>() * te_bwd_wave_floats<P>());
}
static_assert(te_bwd_lds_bytes<32>() <= 160 * 1024 && te_bwd_lds_bytes<16>() <= 160 * 1024 &&
                  te_bwd_lds_bytes<8>() <= 160 * 1024,
              "decision history");

template <int P, bool TICKET>
__global__ __launch_bounds__(te_bwd_waves<P>() * 64) void k_true_envelope_bwd(
    const float* __restrict__ x, long long ldx, long long nframes, const float* __restrict__ tw_g,
    const float* __restrict__ w_g, int in_type, int max_iters, const int* __restrict__ iters,
    const float* __restrict__ gy, long long ldgy, float* __restrict__ gx, long long ldgx, int* __restrict__ decisions,
    float* __restrict__ env_out, long long lde, int* __restrict__ ticket) {
    constexpr int M = 64 * P, LB = ilog2(P), WS = te_w_stride<P>(), NW = te_bwd_waves<P>(), NT = NW * 64;
    constexpr int PER = 32 / P, DW = 2 * P + 1;   // passes per history word; decision words per pass
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* tw = smem;
    float* wl = smem + tw_floats<P>();
    const int lane_id = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    float* xbuf = wl + te_w_floats<P>() + wave * (P * kXStride);
    unsigned* hist = reinterpret_cast<unsigned*>(wl + te_w_floats<P>() + NW * (P * kXStride)) +
                     wave * (te_hist_words<P>() + kTeBwdMaxPasses);
    unsigned* nyq = hist + te_hist_words<P>();
    for (int i = threadIdx.x; i < tw_floats<P>(); i += NT) tw[i] = tw_g[i];
    for (int e = threadIdx.x; e < 64 * P; e += NT) {
        const int l = e / P, i = e % P;
        const int n0 = 2 * (kappa<P>(l) + 64 * brev(i, LB));
        wl[l * WS + 2 * i] = w_g[n0];
        wl[l * WS + 2 * i + 1] = w_g[n0 + 1];
    }
    __syncthreads();
    const int kap = kappa<P>(lane_id);
    const int src_lane = kappa<P>((64 - kap) & 63);
    float wa_s, wa_c, ws_s, ws_c;
    sincospif(-2.0f * (float)kap / (float)(2 * M), &wa_s, &wa_c);
    sincospif(2.0f * (float)lane_id / (float)(2 * M), &ws_s, &ws_c);
    const float* wrow = wl + lane_id * WS;

    auto take = [&]() -> long long {
        int t = 0;
        if (lane_id == 0) t = atomicAdd(ticket, 1);
        return (long long)rfl(__shfl(t, 0));
    };
    long long f = TICKET ? take() : (long long)blockIdx.x * NW + rfl(wave);
    while (f < nframes) {
        const long long f_next = TICKET ? take() : f + (long long)gridDim.x * NW;
        int lane = lane_id;
        asm volatile("" : "+v"(lane));
        const float* xp = x + f * ldx;
        float* gxp = gx + f * ldgx;
        int* dec = decisions ? decisions + f * ((long long)max_iters * DW) : nullptr;
        const int K = min(max(iters[f], 1), max_iters);
        float a[P], t[P];
        float aM = 0.0f, tM = 0.0f;
        bool bad = false;
#pragma unroll
        for (int j = 0; j < P; ++j) a[j] = xp[lane + 64 * j];
        if (lane == 0) aM = xp[M];
        te_to_db<P>(a, aM, in_type);
#pragma unroll
        for (int j = 0; j < P; ++j) bad |= !isfinite(a[j]);
        if (lane == 0) bad |= !isfinite(aM);
        if (__ballot(bad) != 0) {
#pragma unroll
            for (int j = 0; j < P; ++j) gxp[lane + 64 * j] = 0.0f;
            if (lane == 0) gxp[M] = 0.0f;
            if (env_out) {
                float* ep = env_out + f * lde;
#pragma unroll
                for (int j = 0; j < P; ++j) ep[lane + 64 * j] = __builtin_nanf("");
                if (lane == 0) ep[M] = __builtin_nanf("");
            }
            if (dec)
                for (int i = lane; i < max_iters * DW; i += 64) dec[i] = 0;
            f = f_next;
            continue;
        }
        // ---- the forward's K passes again; passes 1 .. K - 1 decide
        unsigned cur = 0;
        for (int pass = 1;; ++pass) {
            te_smooth<P>(a, aM, t, tM, tw, wrow, xbuf, lane, kap, src_lane, ws_c, ws_s, wa_c, wa_s);
            if (pass >= K) break;
            const int d = pass - 1;
            unsigned bits = 0;
#pragma unroll
            for (int j = 0; j < P; ++j) bits |= (t[j] > a[j] ? 1u : 0u) << j;
            const unsigned bitM = (tM > aM) ? 1u : 0u;
            cur = (d % PER == 0 ? 0u : cur) | (bits << ((d % PER) * P));
            hist[(d / PER) * 64 + lane] = cur;
            if (lane == 0) nyq[d] = bitM;
            if (dec) {
                int* dp = dec + d * DW;
#pragma unroll
                for (int j = 0; j < P; ++j) {
                    const unsigned long long b = __ballot((bits >> j) & 1u);   // bins 64 j .. 64 j + 63
                    if (lane < 2) dp[2 * j + lane] = (int)(unsigned)(lane ? (b >> 32) : b);
                }
                if (lane == 0) dp[2 * P] = (int)bitM;
            }
#pragma unroll
            for (int j = 0; j < P; ++j) a[j] = fmaxf(a[j], t[j]);
            aM = fmaxf(aM, tM);
        }
        if (dec)
            for (int i = (K - 1) * DW + lane; i < max_iters * DW; i += 64) dec[i] = 0;
        te_from_db<P>(t, tM, in_type);   // y = the envelope row, as the forward stored it
        if (env_out) {
            float* ep = env_out + f * lde;
#pragma unroll
            for (int j = 0; j < P; ++j) ep[lane + 64 * j] = t[j];
            if (lane == 0) ep[M] = tM;
        }
        // ---- g_s = g_y dy/ds_K: y ln 10 / 20 ('abs'), 1 ('db'), ln 10 / 20 ('log')
        const float* gyp = gy + f * ldgy;
        float gs[P], gsM = 0.0f;
#pragma unroll
        for (int j = 0; j < P; ++j) gs[j] = gyp[lane + 64 * j];
        if (lane == 0) gsM = gyp[M];
        if (in_type == 0) {
#pragma unroll
            for (int j = 0; j < P; ++j) gs[j] *= 0.115129254649702284f * t[j];
            gsM *= 0.115129254649702284f * tM;
        } else if (in_type == 2) {
#pragma unroll
            for (int j = 0; j < P; ++j) gs[j] *= 0.115129254649702284f;
            gsM *= 0.115129254649702284f;
        }
#pragma unroll
        for (int j = 0; j < P; ++j) a[j] = 0.0f;   // a: now g_a
        aM = 0.0f;
        // ---- the K adjoint passes, last first
        for (int k = K;; --k) {
            if (lane == 0) gs[0] *= 2.0f;
            gsM *= 2.0f;
            te_smooth<P>(gs, gsM, t, tM, tw, wrow, xbuf, lane, kap, src_lane, ws_c, ws_s, wa_c, wa_s);
            if (lane == 0) t[0] *= 0.5f;
            tM *= 0.5f;
#pragma unroll
            for (int j = 0; j < P; ++j) a[j] += t[j];
            aM += tM;
            if (k <= 1) break;
            const int d = k - 2;
            const unsigned bits = hist[(d / PER) * 64 + lane] >> ((d % PER) * P);
            const bool mM = nyq[d] != 0u;
#pragma unroll
            for (int j = 0; j < P; ++j) {
                const bool m = ((bits >> j) & 1u) != 0u;
                gs[j] = m ? a[j] : 0.0f;
                a[j] = m ? 0.0f : a[j];
            }
            gsM = mM ? aM : 0.0f;
            aM = mM ? 0.0f : aM;
        }
        // ---- g_x = g_a da_1/dx: 20 / (ln 10 x) ('abs'), 1 ('db'), 20 / ln 10 ('log')
        if (in_type == 0) {
#pragma unroll
            for (int j = 0; j < P; ++j) a[j] = 8.68588963806503655f * a[j] / xp[lane + 64 * j];
            if (lane == 0) aM = 8.68588963806503655f * aM / xp[M];
        } else if (in_type == 2) {
#pragma unroll
            for (int j = 0; j < P; ++j) a[j] *= 8.68588963806503655f;
            aM *= 8.68588963806503655f;
        }
#pragma unroll
        for (int j = 0; j < P; ++j) gxp[lane + 64 * j] = a[j];
        if (lane == 0) gxp[M] = aM;
        f = f_next;
    }
}

}  // namespace mpx

using namespace mpx;

template <int P, bool TICKET>
static int te_launch(hipStream_t s, long long n, const float* tables, const float* weights, const float* in,
                     long long ld_in, int in_type, float thres_sum, int max_iters, const int32_t* forced, float* out,
                     long long ld_out, int32_t* iters, int32_t* ticket) {
    auto K = k_true_envelope<P, TICKET>;
    if (int rc = set_lds(K, te_lds_bytes<P>())) return rc;
    hipLaunchKernelGGL(K, dim3(grid_for(n)), dim3(kThreads), te_lds_bytes<P>(), s, in, ld_in, n, tables, weights,
                       in_type, thres_sum, max_iters, forced, out, ld_out, iters, ticket);
    return MPX_OK;
}

template <int P, bool TICKET>
static int te_bwd_launch(hipStream_t s, long long n, const float* tables, const float* weights, const float* in,
                         long long ld_in, int in_type, int max_iters, const int32_t* iters, const float* gy,
                         long long ldgy, float* gx, long long ldgx, int32_t* decisions, float* env_out, long long lde,
                         int32_t* ticket) {
    auto K = k_true_envelope_bwd<P, TICKET>;
    if (int rc = set_lds(K, te_bwd_lds_bytes<P>())) return rc;
    hipLaunchKernelGGL(K, dim3(grid_for(n, te_bwd_waves<P>())), dim3(te_bwd_waves<P>() * 64), te_bwd_lds_bytes<P>(), s,
                       in, ld_in, n, tables, weights, in_type, max_iters, iters, gy, ldgy, gx, ldgx, decisions, env_out,
                       lde, ticket);
    return MPX_OK;
}

extern "C" {

int mpx_true_envelope(void* stream, int fft_len, const void* tables, const float* weights, const float* in,
                      int64_t ld_in, int64_t n_frames, int32_t in_type, double thres_db, int32_t max_iters, float* out,
                      int64_t ld_out, int32_t* iters, const int32_t* forced_iters, int32_t* ticket) {
    const int P = p_of(fft_len);
    if (!P) return fail(MPX_ERR_ARG, "mpx_true_envelope: fft_len must be 1024, 2048 or 4096%s");
    const int64_t H = fft_len / 2 + 1;
    if (n_frames < 0) return fail(MPX_ERR_ARG, "mpx_true_envelope: negative n_frames%s");
    if (ld_in < H || ld_out < H) return fail(MPX_ERR_ARG, "mpx_true_envelope: row pitch below fft_len / 2 + 1%s");
    if (in_type < 0 || in_type > 2) return fail(MPX_ERR_ARG, "mpx_true_envelope: in_type must be 0, 1 or 2%s");
    if (max_iters < 1) return fail(MPX_ERR_ARG, "mpx_true_envelope: max_iters must be >= 1%s");
    if (ticket && n_frames > (int64_t)INT32_MAX - (1 << 24))
        return fail(MPX_ERR_ARG, "mpx_true_envelope: too many frames for a 32-bit ticket counter%s");
    if (n_frames == 0) return MPX_OK;
    if (!tables || !weights || !in || !out) return fail(MPX_ERR_ARG, "mpx_true_envelope: null pointer%s");
    hipStream_t s = (hipStream_t)stream;
    if (ticket) MPX_HIP_CHECK(hipMemsetAsync(ticket, 0, sizeof(int32_t), s));
    const float thres_sum = (float)(thres_db * (double)H);
    const float* tab = (const float*)tables;
    int rc;
#define MPX_TE_LAUNCH(PP, T)                                                                                             \
    rc = te_launch<PP, T>(s, (long long)n_frames, tab, weights, in, (long long)ld_in, (int)in_type, thres_sum,        \
                          (int)max_iters, forced_iters, out, (long long)ld_out, iters, ticket)
    if (P == 32) {
        if (ticket) MPX_TE_LAUNCH(32, true); else MPX_TE_LAUNCH(32, false);
    } else if (P == 16) {
        if (ticket) MPX_TE_LAUNCH(16, true); else MPX_TE_LAUNCH(16, false);
    } else {
        if (ticket) MPX_TE_LAUNCH(8, true); else MPX_TE_LAUNCH(8, false);
    }
#undef MPX_TE_LAUNCH
    if (rc) return rc;
    MPX_HIP_CHECK(hipGetLastError());
    return MPX_OK;
}

int mpx_true_envelope_backward(void* stream, int fft_len, const void* tables, const float* weights, const float* in,
                               int64_t ld_in, int64_t n_frames, int32_t in_type, int32_t max_iters, const int32_t* iters,
                               const float* grad_out, int64_t ld_grad_out, float* grad_in, int64_t ld_grad_in,
                               int32_t* decisions, float* env_out, int64_t ld_env_out, int32_t* ticket) {
    const int P = p_of(fft_len);
    if (!P) return fail(MPX_ERR_ARG, "mpx_true_envelope_backward: fft_len must be 1024, 2048 or 4096%s");
    const int64_t H = fft_len / 2 + 1;
    if (n_frames < 0) return fail(MPX_ERR_ARG, "mpx_true_envelope_backward: negative n_frames%s");
    if (ld_in < H || ld_grad_out < H || ld_grad_in < H || (env_out && ld_env_out < H))
        return fail(MPX_ERR_ARG, "mpx_true_envelope_backward: row pitch below fft_len / 2 + 1%s");
    if (in_type < 0 || in_type > 2) return fail(MPX_ERR_ARG, "mpx_true_envelope_backward: in_type must be 0, 1 or 2%s");
    if (max_iters < 1) return fail(MPX_ERR_ARG, "mpx_true_envelope_backward: max_iters must be >= 1%s");
    if (max_iters > kTeBwdMaxPasses)
        return fail(MPX_ERR_ARG, "mpx_true_envelope_backward: max_iters above 100, the decision history's capacity%s");
    if (ticket && n_frames > (int64_t)INT32_MAX - (1 << 24))
        return fail(MPX_ERR_ARG, "mpx_true_envelope_backward: too many frames for a 32-bit ticket counter%s");
    if (n_frames == 0) return MPX_OK;
    if (!tables || !weights || !in || !iters || !grad_out || !grad_in)
        return fail(MPX_ERR_ARG, "mpx_true_envelope_backward: null pointer%s");
    hipStream_t s = (hipStream_t)stream;
    if (ticket) MPX_HIP_CHECK(hipMemsetAsync(ticket, 0, sizeof(int32_t), s));
    const float* tab = (const float*)tables;
    int rc;
#define MPX_TE_LAUNCH(PP, T)                                                                                             \
    rc = te_bwd_launch<PP, T>(s, (long long)n_frames, tab, weights, in, (long long)ld_in, (int)in_type, (int)max_iters, \
                              iters, grad_out, (long long)ld_grad_out, grad_in, (long long)ld_grad_in, decisions,       \
                              env_out, (long long)ld_env_out, ticket)
    if (P == 32) {
        if (ticket) MPX_TE_LAUNCH(32, true); else MPX_TE_LAUNCH(32, false);
    } else if (P == 16) {
        if (ticket) MPX_TE_LAUNCH(16, true); else MPX_TE_LAUNCH(16, false);
    } else {
        if (ticket) MPX_TE_LAUNCH(8, true); else MPX_TE_LAUNCH(8, false);
    }
#undef MPX_TE_LAUNCH
    if (rc) return rc;
    MPX_HIP_CHECK(hipGetLastError());
    return MPX_OK;
}

}  // extern "C"
