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

}  // extern "C"
