// magphase_mlpg.hip -- maximum-likelihood parameter generation (MLPG) and its stencil.
//
// One utterance of F frames and one feature dimension: K = 1 + n_win streams (static, then n_win three-tap windows
// w_k = (w_k[-1], w_k[0], w_k[+1])), W_k[t, t + j] = w_k[j] with the taps outside [0, F) dropped, P_k = diag(1 / var_k),
//     A = sum_k W_k^T P_k W_k   (symmetric positive definite, pentadiagonal),   b = sum_k W_k^T P_k mu_k,   c = A^-1 b.
//   k_mlpg_solve   one LANE per system (utterance, dimension): forms the band rows of A and b on the fly and runs the LDL^T
//                  factorisation of bandwidth 2 with both substitutions in float64.
//   k_mlpg_apply   one thread per element of y_k = [P_k] W_k x: the tail of the backward pass (with P_k) and the
//                  dynamic-feature computation (without).
#include "mpx_common.hpp"

using namespace mpx;

namespace {

constexpr int kMlpgThreads = 64;      // one wave per workgroup: 3 840 systems (64 utterances x 60) are 60 waves on 256 CUs
constexpr int kMlpgMaxStreams = 3;
constexpr int kFwd = 2, kBwd = 8;     // frames fetched ahead of the forward sweep and of the back substitution

// The windows as the kernels take them (by value): the taps w[k][j + 1] = w_k[j] of all K streams (stream 0 = (0, 1, 0))
// and the products of taps the band of A is made of, formed once in float64 on the host.
struct MlpgTaps {
    double w[kMlpgMaxStreams][3];
    double aa[kMlpgMaxStreams][3];   // diagonal: (w[+1]^2, w[0]^2, w[-1]^2), the weights of p[i - 1], p[i], p[i + 1]
    double e0[kMlpgMaxStreams];      // A[i, i + 1]: w[0] w[+1] on p[i] ...
    double e1[kMlpgMaxStreams];      //              ... and w[-1] w[0] on p[i + 1]
    double ff[kMlpgMaxStreams];      // A[i, i + 2]: w[-1] w[+1] on p[i + 1]
};

__device__ __forceinline__ int utt_of_frame(const int* __restrict__ off, int n_utts, long long t) {
    int lo = 0, hi = n_utts;          // the utterance u with off[u] <= t < off[u + 1] (empty utterances are passed over)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((long long)off[mid] <= t) lo = mid; else hi = mid;
    }
    return lo;
}

// System s = u * D + d of a batch of n_utts utterances.  Frame i of it is row r = off[u] + i of every operand: mean
// [total x K D] (stream k at column k D + d; RHS: the right-hand side itself, [total x D]), var (the same columns; ld_var
// == 0: one row for all frames), out [total x D] and the two workspace planes L1, L2 [total x D] -- consecutive lanes of
// one utterance touch consecutive addresses everywhere.
//
// Step i of the forward sweep holds the precisions p_k and the weighted means q_k = p_k mu_k of the frames i - 1, i, i + 1
// (zero outside [0, F): the truncated windows, and nothing outside the utterance is read); later frames are in flight:
//     a_i = sum_k aa_k . p_k[i-1 .. i+1]         e_i = A[i, i+1] = sum_k e0_k p_k[i] + e1_k p_k[i+1]
//     r_i = sum_k w_k[+1, 0, -1] . q_k[i-1 .. i+1]   f_i = A[i, i+2] = sum_k ff_k p_k[i+1]
//     l2_i = f_{i-2} / d_{i-2}      v = e_{i-1} - f_{i-2} l1_{i-1}      l1_i = v / d_{i-1}
//     d_i = a_i - l1_i v - l2_i f_{i-2}         y_i = r_i - l1_i y_{i-1} - l2_i y_{i-2}        z_i = y_i / d_i
// l1_i, l2_i go to the workspace, z_i to out; the backward sweep c_i = z_i - l1_{i+1} c_{i+1} - l2_{i+2} c_{i+2} overwrites
// out in place.  The initial state (d = 1, everything else 0) makes the first two steps the general one.
template <typename TM, typename TV, int NW, bool RHS>
__global__ __launch_bounds__(kMlpgThreads) void k_mlpg_solve(const TM* __restrict__ mean, long long ld_mean,
                                                            const TV* __restrict__ var, long long ld_var,
                                                            const int* __restrict__ off, int n_utts, int D,
                                                            long long total, MlpgTaps tp, double* __restrict__ out,
                                                            long long ld_out, double* __restrict__ work) {
    constexpr int K = NW + 1;
    const long long s = (long long)blockIdx.x * kMlpgThreads + threadIdx.x;
    if (s >= (long long)n_utts * D) return;
    const int u = (int)(s / D), d = (int)(s - (long long)u * D);
    const long long r0 = off[u];
    const int F = off[u + 1] - off[u];
    if (F <= 0) return;
    double* __restrict__ wl1 = work;
    double* __restrict__ wl2 = work + total * (long long)D;

    // A global variance row is read and inverted once.
    const bool gvar = ld_var == 0;
    double pg[K];
#pragma unroll
    for (int k = 0; k < K; ++k) pg[k] = gvar ? 1.0 / (double)var[(long long)k * D + d] : 0.0;

    // The operands of kFwd frames are fetched a chunk ahead as they lie in memory (raw), so that the latency of a load is
    // spread over kFwd steps of the chain instead of being paid once per step; converted to p, q when their chunk begins.
    TV rv[kFwd][K];
    TM rm[kFwd][K];
    TM rg[kFwd];
    auto fetch = [&](int base) {   // frames base + 2 .. base + 2 + kFwd - 1 of every stream; RHS: g of base .. base + kFwd - 1
#pragma unroll
        for (int j = 0; j < kFwd; ++j) {
            const int t = base + 2 + j;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                rv[j][k] = (TV)1;
                rm[j][k] = (TM)0;
                if (t < F) {
                    if (!gvar) rv[j][k] = var[(r0 + t) * ld_var + (long long)k * D + d];
                    if (!RHS) rm[j][k] = mean[(r0 + t) * ld_mean + (long long)k * D + d];
                }
            }
            rg[j] = (TM)0;
            if (RHS && base + j < F) rg[j] = mean[(r0 + base + j) * ld_mean + d];
        }
    };
    auto convert = [&](int t, int j, int k, double& pk, double& qk) {   // frame t = raw slot j
        pk = qk = 0.0;
        if (t < F) {
            pk = gvar ? pg[k] : 1.0 / (double)rv[j][k];
            qk = RHS ? 0.0 : pk * (double)rm[j][k];
        }
    };

    double p[K][3], q[K][3];   // [k][0 .. 2] = frames i - 1, i, i + 1
    fetch(-2);                 // frames 0 .. kFwd - 1 (kFwd >= 2)
#pragma unroll
    for (int k = 0; k < K; ++k) {
        p[k][0] = q[k][0] = 0.0;
        convert(0, 0, k, p[k][1], q[k][1]);
        convert(1, 1, k, p[k][2], q[k][2]);
    }
    fetch(0);
    double d1 = 1.0, d2 = 1.0, l1p = 0.0, y1 = 0.0, y2 = 0.0, e1 = 0.0, f1 = 0.0, f2 = 0.0;
    for (int i0 = 0; i0 < F; i0 += kFwd) {
        double pn[kFwd][K], qn[kFwd][K], gc[kFwd];   // frames i0 + 2 + j; g of frames i0 + j
#pragma unroll
        for (int j = 0; j < kFwd; ++j) {
#pragma unroll
            for (int k = 0; k < K; ++k) convert(i0 + 2 + j, j, k, pn[j][k], qn[j][k]);
            gc[j] = (double)rg[j];
        }
        fetch(i0 + kFwd);      // the next chunk's operands, in flight while this chunk's steps run
#pragma unroll
        for (int j = 0; j < kFwd; ++j) {
            const int i = i0 + j;
            if (i < F) {
                double a = 0.0, e = 0.0, f = 0.0, r = 0.0;
#pragma unroll
                for (int k = 0; k < K; ++k) {
#pragma unroll
                    for (int t = 0; t < 3; ++t) {
                        a = fma(tp.aa[k][t], p[k][t], a);
                        if (!RHS) r = fma(tp.w[k][2 - t], q[k][t], r);
                    }
                    e = fma(tp.e0[k], p[k][1], e);
                    e = fma(tp.e1[k], p[k][2], e);
                    f = fma(tp.ff[k], p[k][2], f);
                }
                if (RHS) r = gc[j];
                const double l2 = f2 / d2;
                const double v = fma(-f2, l1p, e1);
                const double l1 = v / d1;
                const double dd = fma(-l2, f2, fma(-l1, v, a));
                const double y = fma(-l2, y2, fma(-l1, y1, r));
                const long long wi = (r0 + i) * (long long)D + d;
                wl1[wi] = l1;
                wl2[wi] = l2;
                out[(r0 + i) * ld_out + d] = y / dd;
                d2 = d1; d1 = dd; l1p = l1; y2 = y1; y1 = y; f2 = f1; f1 = f; e1 = e;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    p[k][0] = p[k][1]; p[k][1] = p[k][2]; p[k][2] = pn[j][k];
                    q[k][0] = q[k][1]; q[k][1] = q[k][2]; q[k][2] = qn[j][k];
                }
            }
        }
    }
    // back substitution: c_i = z_i - l1_{i+1} c_{i+1} - l2_{i+2} c_{i+2}, kBwd frames fetched a chunk ahead; the rows i + 1,
    // i + 2 >= F do not exist and are not read (they belong to the next utterance, or lie past the workspace)
    double zr[kBwd], m1r[kBwd], m2r[kBwd];
    auto fetch_back = [&](int top) {   // frames top, top - 1, ..., top - kBwd + 1
#pragma unroll
        for (int j = 0; j < kBwd; ++j) {
            const int i = top - j;
            zr[j] = m1r[j] = m2r[j] = 0.0;
            if (i >= 0) {
                zr[j] = out[(r0 + i) * ld_out + d];
                if (i + 1 < F) m1r[j] = wl1[(r0 + i + 1) * (long long)D + d];
                if (i + 2 < F) m2r[j] = wl2[(r0 + i + 2) * (long long)D + d];
            }
        }
    };
    fetch_back(F - 1);
    double c1 = 0.0, c2 = 0.0;
    for (int top = F - 1; top >= 0; top -= kBwd) {
        double zc[kBwd], m1c[kBwd], m2c[kBwd];
#pragma unroll
        for (int j = 0; j < kBwd; ++j) {
            zc[j] = zr[j];
            m1c[j] = m1r[j];
            m2c[j] = m2r[j];
        }
        fetch_back(top - kBwd);
#pragma unroll
        for (int j = 0; j < kBwd; ++j) {
            const int i = top - j;
            if (i >= 0) {
                const double c = fma(-m2c[j], c2, fma(-m1c[j], c1, zc[j]));
                out[(r0 + i) * ld_out + d] = c;
                c2 = c1;
                c1 = c;
            }
        }
    }
}

// y[r, k D + d] = [1 / var[r, k D + d]] sum_j w_k[j] x[r + j, d] over the taps that stay inside the utterance of row r; one
// thread per element of y.  The sum is (w[-1] x[-1]) then fma(w[0], x[0], .) then fma(w[+1], x[+1], .): a dropped tap is
// skipped, not added as a zero, and the precision is ONE division, so an element carries at most four roundings.
template <typename TX, typename TV, bool PREC>
__global__ __launch_bounds__(256) void k_mlpg_apply(const TX* __restrict__ x, long long ld_x, const TV* __restrict__ var,
                                                    long long ld_var, const int* __restrict__ off, int n_utts, int D, int K,
                                                    long long total, MlpgTaps tp, double* __restrict__ y,
                                                    long long ld_y) {
    const long long KD = (long long)K * D;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total * KD) return;
    const long long r = e / KD;
    const int col = (int)(e - r * KD), k = col / D, d = col - k * D;
    const int u = utt_of_frame(off, n_utts, r);
    const bool has_prev = r > (long long)off[u], has_next = r + 1 < (long long)off[u + 1];
    double acc = 0.0;
    bool any = false;
    if (has_prev) {
        acc = tp.w[k][0] * (double)x[(r - 1) * ld_x + d];
        any = true;
    }
    {
        const double x0 = (double)x[r * ld_x + d];
        acc = any ? fma(tp.w[k][1], x0, acc) : tp.w[k][1] * x0;
    }
    if (has_next) acc = fma(tp.w[k][2], (double)x[(r + 1) * ld_x + d], acc);
    if (PREC) acc = acc / (double)var[(ld_var ? r * ld_var : 0) + col];
    y[r * ld_y + col] = acc;
}

int mlpg_taps(const char* who, int n_win, const double* windows, MlpgTaps& tp) {
    memset(&tp, 0, sizeof(tp));
    for (int k = 0; k <= n_win; ++k) {
        for (int j = 0; j < 3; ++j) {
            tp.w[k][j] = (k == 0) ? (j == 1 ? 1.0 : 0.0) : windows[3 * (k - 1) + j];
            if (!std::isfinite(tp.w[k][j])) return fail(MPX_ERR_ARG, "%s: a window tap is not finite", who);
        }
        tp.aa[k][0] = tp.w[k][2] * tp.w[k][2];
        tp.aa[k][1] = tp.w[k][1] * tp.w[k][1];
        tp.aa[k][2] = tp.w[k][0] * tp.w[k][0];
        tp.e0[k] = tp.w[k][1] * tp.w[k][2];
        tp.e1[k] = tp.w[k][0] * tp.w[k][1];
        tp.ff[k] = tp.w[k][0] * tp.w[k][2];
    }
    return MPX_OK;
}

int mlpg_check(const char* who, int64_t total_frames, int32_t n_utts, int32_t D, int32_t n_win) {
    if (D < 1) return fail(MPX_ERR_ARG, "%s: D must be >= 1", who);
    if (n_win != 1 && n_win != 2) return fail(MPX_ERR_ARG, "%s: n_win must be 1 or 2", who);
    if (total_frames < 0) return fail(MPX_ERR_ARG, "%s: negative total_frames", who);
    if (n_utts < 0) return fail(MPX_ERR_ARG, "%s: negative n_utts", who);
    if (total_frames > 0x7fffffffLL) return fail(MPX_ERR_ARG, "%s: total_frames above 2^31 - 1 (int32 frame offsets)", who);
    if ((long long)n_utts * D > 0x7fffffffLL * (long long)kMlpgThreads)
        return fail(MPX_ERR_ARG, "%s: too many systems for one launch", who);
    return MPX_OK;
}

template <typename TM, typename TV>
void solve_launch(hipStream_t s, int n_win, bool rhs, const void* mean, long long ld_mean, const void* var,
                  long long ld_var, const int* off, int n_utts, int D, long long total, const MlpgTaps& tp, double* out,
                  long long ld_out, double* work) {
    const long long systems = (long long)n_utts * D;
    const dim3 grid((unsigned)((systems + kMlpgThreads - 1) / kMlpgThreads)), block(kMlpgThreads);
#define MPX_MLPG_GO(NW, R)                                                                                             \
    hipLaunchKernelGGL((k_mlpg_solve<TM, TV, NW, R>), grid, block, 0, s, (const TM*)mean, ld_mean, (const TV*)var,      \
                       ld_var, off, n_utts, D, total, tp, out, ld_out, work)
    if (n_win == 1) {
        if (rhs) MPX_MLPG_GO(1, true); else MPX_MLPG_GO(1, false);
    } else {
        if (rhs) MPX_MLPG_GO(2, true); else MPX_MLPG_GO(2, false);
    }
#undef MPX_MLPG_GO
}

template <typename TX, typename TV>
void apply_launch(hipStream_t s, bool prec, const void* x, long long ld_x, const void* var, long long ld_var,
                  const int* off, int n_utts, int D, int K, long long total, const MlpgTaps& tp, double* y,
                  long long ld_y) {
    const long long n = total * K * D;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (prec)
        hipLaunchKernelGGL((k_mlpg_apply<TX, TV, true>), grid, block, 0, s, (const TX*)x, ld_x, (const TV*)var, ld_var,
                           off, n_utts, D, K, total, tp, y, ld_y);
    else
        hipLaunchKernelGGL((k_mlpg_apply<TX, TV, false>), grid, block, 0, s, (const TX*)x, ld_x, (const TV*)var, ld_var,
                           off, n_utts, D, K, total, tp, y, ld_y);
}

}  // namespace

extern "C" {

int64_t mpx_mlpg_work_doubles(int64_t total_frames, int32_t D) {
    if (total_frames < 0 || D < 1) return 0;
    return 2 * total_frames * (int64_t)D;   // the planes l1, l2 of the factor, [total_frames x D] each
}

int mpx_mlpg_solve(void* stream, const void* mean, int32_t mean_f64, int64_t ld_mean, const void* var, int32_t var_f64,
                   int64_t ld_var, const int32_t* utt_frame_off, int32_t n_utts, int64_t total_frames, int32_t D,
                   int32_t n_win, const double* windows, int32_t rhs_direct, double* out, int64_t ld_out, double* work) {
    static const char* who = "mpx_mlpg_solve";
    if (int rc = mlpg_check(who, total_frames, n_utts, D, n_win)) return rc;
    const int K = n_win + 1;
    if (ld_mean < (rhs_direct ? (int64_t)D : (int64_t)K * D)) return fail(MPX_ERR_ARG, "%s: ld_mean below the row width", who);
    if (ld_var != 0 && ld_var < (int64_t)K * D) return fail(MPX_ERR_ARG, "%s: ld_var must be 0 (one row) or >= K * D", who);
    if (ld_out < D) return fail(MPX_ERR_ARG, "%s: ld_out below D", who);
    if (!windows) return fail(MPX_ERR_ARG, "%s: null pointer (windows)", who);
    MlpgTaps tp;
    if (int rc = mlpg_taps(who, n_win, windows, tp)) return rc;
    if (total_frames == 0 || n_utts == 0) return MPX_OK;
    if (!mean || !var || !utt_frame_off || !out || !work) return fail(MPX_ERR_ARG, "%s: null pointer", who);
    const hipStream_t s = (hipStream_t)stream;
    const int* off = (const int*)utt_frame_off;
    if (mean_f64) {
        if (var_f64) solve_launch<double, double>(s, n_win, rhs_direct != 0, mean, ld_mean, var, ld_var, off, n_utts, D, total_frames, tp, out, ld_out, work);
        else solve_launch<double, float>(s, n_win, rhs_direct != 0, mean, ld_mean, var, ld_var, off, n_utts, D, total_frames, tp, out, ld_out, work);
    } else {
        if (var_f64) solve_launch<float, double>(s, n_win, rhs_direct != 0, mean, ld_mean, var, ld_var, off, n_utts, D, total_frames, tp, out, ld_out, work);
        else solve_launch<float, float>(s, n_win, rhs_direct != 0, mean, ld_mean, var, ld_var, off, n_utts, D, total_frames, tp, out, ld_out, work);
    }
    MPX_HIP_CHECK(hipGetLastError());
    return MPX_OK;
}

int mpx_mlpg_apply(void* stream, const void* x, int32_t x_f64, int64_t ld_x, const void* var, int32_t var_f64,
                   int64_t ld_var, const int32_t* utt_frame_off, int32_t n_utts, int64_t total_frames, int32_t D,
                   int32_t n_win, const double* windows, double* y, int64_t ld_y) {
    static const char* who = "mpx_mlpg_apply";
    if (int rc = mlpg_check(who, total_frames, n_utts, D, n_win)) return rc;
    const int K = n_win + 1;
    if (ld_x < D) return fail(MPX_ERR_ARG, "%s: ld_x below D", who);
    if (ld_var != 0 && ld_var < (int64_t)K * D) return fail(MPX_ERR_ARG, "%s: ld_var must be 0 (one row) or >= K * D", who);
    if (ld_y < (int64_t)K * D) return fail(MPX_ERR_ARG, "%s: ld_y below K * D", who);
    if (total_frames * K > 0x7fffffffLL * 256 / D) return fail(MPX_ERR_ARG, "%s: too many elements for one launch", who);
    if (!windows) return fail(MPX_ERR_ARG, "%s: null pointer (windows)", who);
    MlpgTaps tp;
    if (int rc = mlpg_taps(who, n_win, windows, tp)) return rc;
    if (total_frames == 0 || n_utts == 0) return MPX_OK;
    if (!x || !utt_frame_off || !y) return fail(MPX_ERR_ARG, "%s: null pointer", who);
    const hipStream_t s = (hipStream_t)stream;
    const int* off = (const int*)utt_frame_off;
    const bool prec = var != nullptr;
    if (x_f64) {
        if (var_f64) apply_launch<double, double>(s, prec, x, ld_x, var, ld_var, off, n_utts, D, K, total_frames, tp, y, ld_y);
        else apply_launch<double, float>(s, prec, x, ld_x, var, ld_var, off, n_utts, D, K, total_frames, tp, y, ld_y);
    } else {
        if (var_f64) apply_launch<float, double>(s, prec, x, ld_x, var, ld_var, off, n_utts, D, K, total_frames, tp, y, ld_y);
        else apply_launch<float, float>(s, prec, x, ld_x, var, ld_var, off, n_utts, D, K, total_frames, tp, y, ld_y);
    }
    MPX_HIP_CHECK(hipGetLastError());
    return MPX_OK;
}

}  // extern "C"
