// magphase_grad_minphase.hip -- backward pass of k_min_phase (magphase_comp.hip), DESIGN.md section 3.3o.
//
//   k_min_phase_bwd<P>   one wavefront per frame, grid-stride over frames, two wave FFTs: the shape of k_min_phase.
//
// Forward, per frame, N = fft_len, M = N/2, L[k] = ln m[k] (protected: a constant where m <= 0):
//   c[n]   = (1/N) [L[0] + (-1)^n L[M] + 2 sum_{k=1..M-1} L[k] cos(2 pi k n / N)]      real inverse transform
//   phi[k] = -2 sum_{n=1..M-1} c[n] sin(2 pi k n / N),  phi[0] = phi[M] = 0             Im FFT(causal fold c)
//   rows out: (m, cos phi, sin phi)
// Backward, from (g_m, g_a, g_b) = the gradients with respect to those three rows:
//   g_phi[k] = g_b[k] cos phi[k] - g_a[k] sin phi[k]   (0 at k = 0, M and from n_phase on; the stored phasors are read)
//   x[n]     = -(2/N) sum_{k=1..M-1} g_phi[k] sin(2 pi k n / N)
//            = the real inverse transform of the Hermitian spectrum X[k] = i g_phi[k] / N: the forward's own front
//              (hermitian_merge + inverse wave FFT) with a purely imaginary input
//   y[n]     = w[n] x[n], w = the causal fold (1, 2, ..., 2, 1, 0, ..., 0): g_c = (N/2) y
//   g_L[k]   = (e[k]/N) Re FFT(g_c)[k] = (e[k]/2) Re FFT(y)[k], e = 1 at k = 0, M, else 2: the forward's back (forward wave
//              FFT + real split), the real part kept where the forward keeps the imaginary one
//   g_mag[k] = g_m[k] + g_L[k] / m[k] where m[k] > 0, g_m[k] elsewhere.
// No atomics; every element of columns 0 .. M of rows 0 .. n_frames - 1 of g_mag is written exactly once, nothing else is;
// the result does not depend on the grid.  g_mag may BE g_m (same pointer, same pitch): element k of a row is read and
// written by the same lane, the read first, and no other lane touches it.
#include "mpx_common.hpp"

namespace mpx {

struct MinPhaseBwdArgs {
    const float* tw;
    const float* mag;     // the forward's output rows, pitch ld
    const float* real;    // cos phi
    const float* imag;    // sin phi
    long long ld;
    const float* gm;      // may be null: zero; may alias out
    const float* ga;      // may be null: zero
    const float* gb;
    long long ldg;
    int n_phase;          // columns of ga / gb from here on are not read: zero
    long long nframes;
    float* out;
    long long ldo;
};

template <int P>
__global__ __launch_bounds__(kThreads) void k_min_phase_bwd(MinPhaseBwdArgs A) {
    constexpr int M = 64 * P, N = 2 * M, LB = ilog2(P);
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* tw = smem;
    const int lane_id = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    float* xbuf = smem + tw_floats<P>() + wave * (P * kXStride);
    for (int i = threadIdx.x; i < tw_floats<P>(); i += kThreads) tw[i] = A.tw[i];
    __syncthreads();
    float wa_s0, wa_c0, ws_s0, ws_c0;
    sincospif(-2.0f * (float)kappa<P>(lane_id) / (float)N, &wa_s0, &wa_c0);
    sincospif(2.0f * (float)lane_id / (float)N, &ws_s0, &ws_c0);
    const int wave_u = rfl(wave);
    const int n_phase = A.n_phase;
    // no phase gradient at all (bins 0 and M never carry one): g_mag = g_m, no transform
    const bool phase = (A.ga || A.gb) && n_phase > 1;
    for (long long f = (long long)blockIdx.x * kWavesPerBlock + wave_u; f < A.nframes;
         f += (long long)gridDim.x * kWavesPerBlock) {
        int lane = lane_id;
        float wa_s = wa_s0, wa_c = wa_c0, ws_s = ws_s0, ws_c = ws_c0;
        asm volatile("" : "+v"(lane), "+v"(wa_s), "+v"(wa_c), "+v"(ws_s), "+v"(ws_c));
        const float* mrow = A.mag + f * A.ld;
        const float* crow = A.real + f * A.ld;
        const float* srow = A.imag + f * A.ld;
        const float* gmrow = A.gm + f * A.ldg;   // rows of null streams are never dereferenced
        const float* garow = A.ga + f * A.ldg;
        const float* gbrow = A.gb + f * A.ldg;
        float* orow = A.out + f * A.ldo;
        if (!phase) {   // uniform over the launch
            float v[P];
#pragma unroll
            for (int j = 0; j < P; ++j) v[j] = A.gm ? gmrow[lane + 64 * j] : 0.0f;
            const float vM = (A.gm && lane == 0) ? gmrow[M] : 0.0f;
#pragma unroll
            for (int j = 0; j < P; ++j) orow[lane + 64 * j] = v[j];
            if (lane == 0) orow[M] = vM;
            continue;
        }
        // ---- i g_phi / N on bins lane + 64 j (the real part is zero; bin M carries nothing: xm = 0)
        float xr[P], xi[P];
        constexpr float scale = 0.5f / (float)M;
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const int k = lane + 64 * j;
            float v = 0.0f;
            if (k < n_phase) {
                const float c = crow[k], s = srow[k];
                const float ga = A.ga ? garow[k] : 0.0f, gb = A.gb ? gbrow[k] : 0.0f;
                v = (gb * c - ga * s) * scale;
            }
            xr[j] = 0.0f;
            xi[j] = v;
        }
        if (lane == 0) xi[0] = 0.0f;   // bin 0
        hermitian_merge<P>(xr, xi, 0.0f, lane, ws_c, ws_s);
        wave_fft<P, +1>(xr, xi, tw, xbuf, lane);
        // ---- samples n = 2m, 2m+1 with m = kappa + 64 brev(i): the causal fold's weights (k_min_phase's)
        const int kap = kappa<P>(lane);
#pragma unroll
        for (int i = 0; i < P; ++i) {
            const int n0 = 2 * (kap + 64 * brev(i, LB));
            const float w0 = (n0 == 0) ? 1.0f : ((n0 < M) ? 2.0f : ((n0 == M) ? 1.0f : 0.0f));
            const float w1 = (n0 + 1 < M) ? 2.0f : ((n0 + 1 == M) ? 1.0f : 0.0f);
            xr[i] *= w0;
            xi[i] *= w1;
        }
        // ---- forward real FFT: input register j must hold z[lane + 64 j]
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
        // ---- real split, Re S[k] only, and the epilogue on bins k = kappa + 64 q, 8 at a time
#pragma unroll
        for (int ib = 0; ib < P; ib += 8) {
            float prb[8], pib[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                prb[u] = __shfl(re[P - 1 - (ib + u)], src_lane);
                pib[u] = __shfl(im[P - 1 - (ib + u)], src_lane);
            }
            // the batch's row loads stay here (hoisted above the transforms they would spill): the lane's bin offset
            // takes a fake dependency on the batch's partner bins.  All of them before the batch's first store: g_m may
            // be the output row.
            int kapb = kap;
            asm volatile("" : "+v"(kapb) : "v"(prb[0]), "v"(pib[0]), "v"(prb[7]), "v"(pib[7]));
            float mv[8], gv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int k = kapb + 64 * brev(ib + u, LB);
                mv[u] = mrow[k];
                gv[u] = A.gm ? gmrow[k] : 0.0f;
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
                float gl = er + (wr * orr - wi * oi);   // Re S[k]
                if (q == 0) gl = lane0 ? 0.5f * gl : gl;   // e[0] / 2
                orow[kapb + 64 * q] = (mv[u] > 0.0f) ? gv[u] + gl / mv[u] : gv[u];
            }
        }
        if (lane0) {   // bin M: S[M] = E[0] - O[0] = Re Z[0] - Im Z[0], e[M] / 2 = 1/2
            const float mM = mrow[M];
            const float gM = A.gm ? gmrow[M] : 0.0f;
            const float gl = 0.5f * (re[0] - im[0]);
            orow[M] = (mM > 0.0f) ? gM + gl / mM : gM;
        }
    }
}

}  // namespace mpx

using namespace mpx;

extern "C" {

int mpx_min_phase_backward(void* stream, int fft_len, const void* tables, const float* mag, const float* real,
                           const float* imag, int64_t ld, const float* grad_m, const float* grad_a, const float* grad_b,
                           int64_t ld_grad, int32_t n_phase, int64_t n_frames, float* grad_mag, int64_t ld_out) {
    const int P = p_of(fft_len);
    if (!P) return fail(MPX_ERR_ARG, "mpx_min_phase_backward: fft_len must be 1024, 2048 or 4096%s");
    const int H = fft_len / 2 + 1;
    if (n_frames < 0) return fail(MPX_ERR_ARG, "mpx_min_phase_backward: negative n_frames%s");
    if (n_phase < 0 || n_phase > H) return fail(MPX_ERR_ARG, "mpx_min_phase_backward: n_phase outside [0, fft_len/2 + 1]%s");
    if (ld < H || ld_grad < H || ld_out < H) return fail(MPX_ERR_ARG, "mpx_min_phase_backward: ld < fft_len/2 + 1%s");
    if (n_frames == 0) return MPX_OK;
    if (!tables || !mag || !real || !imag || !grad_mag) return fail(MPX_ERR_ARG, "mpx_min_phase_backward: null pointer%s");
    if (grad_mag == grad_m && ld_out != ld_grad)
        return fail(MPX_ERR_ARG, "mpx_min_phase_backward: grad_mag may be grad_m only at the same pitch%s");
    MinPhaseBwdArgs a;
    a.tw = (const float*)tables, a.mag = mag, a.real = real, a.imag = imag, a.ld = (long long)ld;
    a.gm = grad_m, a.ga = grad_a, a.gb = grad_b, a.ldg = (long long)ld_grad, a.n_phase = n_phase;
    a.nframes = (long long)n_frames, a.out = grad_mag, a.ldo = (long long)ld_out;
    const dim3 grid(grid_for(n_frames)), block(kThreads);
    hipStream_t s = (hipStream_t)stream;
#define MPX_LAUNCH_MPB(PP)                                                                  \
    do {                                                                                    \
        if (int rc = set_lds(k_min_phase_bwd<PP>, lds_bytes<PP>())) return rc;              \
        hipLaunchKernelGGL(k_min_phase_bwd<PP>, grid, block, lds_bytes<PP>(), s, a);        \
    } while (0)
    if (P == 32) MPX_LAUNCH_MPB(32);
    else if (P == 16) MPX_LAUNCH_MPB(16);
    else MPX_LAUNCH_MPB(8);
#undef MPX_LAUNCH_MPB
    MPX_HIP_CHECK(hipGetLastError());
    return MPX_OK;
}

}  // extern "C"
