// magphase_mlpg.hip -- maximum-likelihood parameter generation (MLPG) and its stencil.
//
// One utterance of F frames and one feature dimension: K = 1 + n_win streams (static, then n_win three-tap windows
// w_k = (w_k[-1], w_k[0], w_k[+1])), W_k[t, t + j] = w_k[j] with the taps outside [0, F) dropped, P_k = diag(1 / var_k),
//     A = sum_k W_k^T P_k W_k   (symmetric positive definite, pentadiagonal),   b = sum_k W_k^T P_k mu_k,   c = A^-1 b.
//   k_mlpg_solve   one LANE per system (utterance, dimension): forms the band rows of A and b on the fly and runs the LDL^T
//                  factorisation of bandwidth 2 with both substitutions in float64.
//   k_mlpg_apply   one thread per element of y_k = [P_k] W_k x: the tail of the backward pass (with P_k) and the
//                  dynamic-feature computation (without).
// Further down: the variances' gradient (k_mlpg_var_bwd, the column pass) and the trajectory likelihood with its gradients
// (k_mlpg_nll, k_mlpg_nll_bwd).
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

// ---------------------------------------------------------------------------------------------------------------------
// Variance gradients and the trajectory likelihood ("variances").
//   k_mlpg_var_bwd        one thread per element: dL/dvar_k[t] = -p^2 (W_k z)[t] (mu_k[t] - (W_k c)[t]) for z = A^-1 dL/dc
//   k_mlpg_colsum_tiles,  the column sums of a [total x width] float64 plane (the gradient of a global variance row): fixed
//   k_mlpg_colsum_final   tiles of kColTile rows summed in ascending order, then the tiles in ascending order
//   k_mlpg_nll            one LANE per system: -log N(x; c, A^-1) from the pivots of the same LDL^T sweep
//   k_mlpg_nll_bwd        one LANE per system: its gradients; the band of A^-1 by a reverse recursion on the factor
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kColTile = 128;   // rows per partial column sum
constexpr int kRev = 2;         // rows fetched ahead of the reverse recursion of k_mlpg_nll_bwd

// (W_k x)[r, d] as k_mlpg_apply forms it: a dropped tap is skipped, not added as a zero.
__device__ __forceinline__ double mlpg_stencil(const double* __restrict__ x, long long ld_x, long long r, int d,
                                               const double (&w)[3], bool has_prev, bool has_next) {
    double acc = 0.0;
    if (has_prev) acc = w[0] * x[(r - 1) * ld_x + d];
    {
        const double x0 = x[r * ld_x + d];
        acc = has_prev ? fma(w[1], x0, acc) : w[1] * x0;
    }
    if (has_next) acc = fma(w[2], x[(r + 1) * ld_x + d], acc);
    return acc;
}

template <typename TM, typename TV>
__global__ __launch_bounds__(256) void k_mlpg_var_bwd(const double* __restrict__ z, long long ld_z,
                                                      const double* __restrict__ c, long long ld_c,
                                                      const TM* __restrict__ mean, long long ld_mean,
                                                      const TV* __restrict__ var, long long ld_var,
                                                      const int* __restrict__ off, int n_utts, int D, int K,
                                                      long long total, MlpgTaps tp, double* __restrict__ g,
                                                      long long ld_g) {
    const long long KD = (long long)K * D;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total * KD) return;
    const long long r = e / KD;
    const int col = (int)(e - r * KD), k = col / D, d = col - k * D;
    const int u = utt_of_frame(off, n_utts, r);
    const bool has_prev = r > (long long)off[u], has_next = r + 1 < (long long)off[u + 1];
    const double wz = mlpg_stencil(z, ld_z, r, d, tp.w[k], has_prev, has_next);
    const double wc = mlpg_stencil(c, ld_c, r, d, tp.w[k], has_prev, has_next);
    const double p = 1.0 / (double)var[(ld_var ? r * ld_var : 0) + col];
    const double mu = (double)mean[r * ld_mean + col];
    g[r * ld_g + col] = -(p * p) * (wz * (mu - wc));
}

__global__ __launch_bounds__(256) void k_mlpg_colsum_tiles(const double* __restrict__ x, long long ld_x, long long total,
                                                           long long width, long long n_tiles,
                                                           double* __restrict__ part) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_tiles * width) return;
    const long long tile = e / width, col = e - tile * width;
    const long long ra = tile * kColTile, rb = ra + kColTile < total ? ra + kColTile : total;
    double s = 0.0;
    for (long long r = ra; r < rb; ++r) s += x[r * ld_x + col];
    part[e] = s;
}

__global__ __launch_bounds__(256) void k_mlpg_colsum_final(const double* __restrict__ part, long long width,
                                                           long long n_tiles, double* __restrict__ sums) {
    const long long col = (long long)blockIdx.x * 256 + threadIdx.x;
    if (col >= width) return;
    double s = 0.0;
    for (long long t = 0; t < n_tiles; ++t) s += part[t * width + col];
    sums[col] = s;
}

// The band entries of row i of A from the precisions of the frames i - 1, i, i + 1, and one step of the LDL^T
// factorisation: k_mlpg_solve's operations in k_mlpg_solve's order.
struct MlpgLdl {
    double d1, d2, l1p, e1, f1, f2;
};

template <int K>
__device__ __forceinline__ void mlpg_band_terms(const MlpgTaps& tp, const double (&p)[K][3], double& a, double& e,
                                                double& f) {
    a = e = f = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int t = 0; t < 3; ++t) a = fma(tp.aa[k][t], p[k][t], a);
        e = fma(tp.e0[k], p[k][1], e);
        e = fma(tp.e1[k], p[k][2], e);
        f = fma(tp.ff[k], p[k][2], f);
    }
}

__device__ __forceinline__ void mlpg_ldl_step(MlpgLdl& s, double a, double e, double f, double& l1, double& l2,
                                              double& dd) {
    l2 = s.f2 / s.d2;
    const double v = fma(-s.f2, s.l1p, s.e1);
    l1 = v / s.d1;
    dd = fma(-l2, s.f2, fma(-l1, v, a));
    s.d2 = s.d1; s.d1 = dd; s.l1p = l1; s.f2 = s.f1; s.f1 = f; s.e1 = e;
}

// The forward sweep of one system (rows r0 .. r0 + F - 1, column d) shared by k_mlpg_nll and k_mlpg_nll_bwd.  Step i holds
// the precisions, the residuals e = x - c and the trajectory c of the frames i - 1, i, i + 1 (zero outside [0, F)), the
// operands of kFwd later frames are in flight.  (W_k e)[i], (W_k c)[i] are fused multiply-add chains over the three taps; a
// tap outside the utterance multiplies a zero.
//   !BWD: quad += p_k[i] (W_k e)[i]^2, logdet += log d_i
//   BWD:  l1_i, l2_i, 1 / d_i go to the workspace planes; g_mean[i, k] = -go p_k[i] (W_k e)[i];
//         g_var[i, k] = (W_k e)[i] ((W_k e)[i] / 2 - (mu_k[i] - (W_k c)[i])), completed by the reverse sweep
template <typename TM, typename TV, typename TX, int NW, bool BWD>
__device__ __forceinline__ void mlpg_nll_sweep(const TM* __restrict__ mean, long long ld_mean, const TV* __restrict__ var,
                                               long long ld_var, const double* __restrict__ c, long long ld_c,
                                               const TX* __restrict__ x, long long ld_x, long long r0, int F, int D, int d,
                                               const MlpgTaps& tp, const double (&pg)[NW + 1], double go,
                                               double* __restrict__ g_mean, long long ld_gm, double* __restrict__ g_var,
                                               long long ld_gv, double* __restrict__ wl1, double* __restrict__ wl2,
                                               double* __restrict__ wdi, double& quad, double& logdet) {
    constexpr int K = NW + 1;
    const bool gvar = ld_var == 0;
    TV rv[kFwd][K];
    TM rm[kFwd][K];
    TX rx[kFwd];
    double rc[kFwd];
    auto fetch = [&](int base) {   // frames base + 2 .. base + 2 + kFwd - 1
#pragma unroll
        for (int j = 0; j < kFwd; ++j) {
            const int t = base + 2 + j;
            rx[j] = (TX)0;
            rc[j] = 0.0;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                rv[j][k] = (TV)1;
                rm[j][k] = (TM)0;
            }
            if (t < F) {
                rx[j] = x[(r0 + t) * ld_x + d];
                rc[j] = c[(r0 + t) * ld_c + d];
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    if (!gvar) rv[j][k] = var[(r0 + t) * ld_var + (long long)k * D + d];
                    if (BWD) rm[j][k] = mean[(r0 + t) * ld_mean + (long long)k * D + d];
                }
            }
        }
    };
    auto convert = [&](int t, int j, double (&pk)[K], double (&mk)[K], double& ek, double& ck) {   // frame t = raw slot j
        ek = ck = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k) pk[k] = mk[k] = 0.0;
        if (t < F) {
            ck = rc[j];
            ek = (double)rx[j] - ck;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                pk[k] = gvar ? pg[k] : 1.0 / (double)rv[j][k];
                mk[k] = (double)rm[j][k];
            }
        }
    };

    double p[K][3], mu[K][2], ev[3], cv[3];   // [0 .. 2] = frames i - 1, i, i + 1; mu: frames i, i + 1
    {
        double p0[K], m0[K], p1[K], m1[K];
        fetch(-2);
        ev[0] = cv[0] = 0.0;
        convert(0, 0, p0, m0, ev[1], cv[1]);
        convert(1, 1, p1, m1, ev[2], cv[2]);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            p[k][0] = 0.0; p[k][1] = p0[k]; p[k][2] = p1[k];
            mu[k][0] = m0[k]; mu[k][1] = m1[k];
        }
    }
    fetch(0);
    MlpgLdl st = {1.0, 1.0, 0.0, 0.0, 0.0, 0.0};
    for (int i0 = 0; i0 < F; i0 += kFwd) {
        double pn[kFwd][K], mn[kFwd][K], en[kFwd], cn[kFwd];   // frames i0 + 2 + j
#pragma unroll
        for (int j = 0; j < kFwd; ++j) convert(i0 + 2 + j, j, pn[j], mn[j], en[j], cn[j]);
        fetch(i0 + kFwd);
#pragma unroll
        for (int j = 0; j < kFwd; ++j) {
            const int i = i0 + j;
            if (i < F) {
                double a, e, f, l1, l2, dd;
                mlpg_band_terms<K>(tp, p, a, e, f);
                mlpg_ldl_step(st, a, e, f, l1, l2, dd);
                if (BWD) {
                    if (g_var) {
                        const long long wi = (r0 + i) * (long long)D + d;
                        wl1[wi] = l1;
                        wl2[wi] = l2;
                        wdi[wi] = 1.0 / dd;
                    }
                } else {
                    logdet += log(dd);
                }
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const double we = fma(tp.w[k][2], ev[2], fma(tp.w[k][1], ev[1], tp.w[k][0] * ev[0]));
                    if (BWD) {
                        const long long col = (long long)k * D + d;
                        if (g_mean) g_mean[(r0 + i) * ld_gm + col] = -go * (p[k][1] * we);
                        if (g_var) {
                            const double wc = fma(tp.w[k][2], cv[2], fma(tp.w[k][1], cv[1], tp.w[k][0] * cv[0]));
                            g_var[(r0 + i) * ld_gv + col] = we * (0.5 * we - (mu[k][0] - wc));
                        }
                    } else {
                        quad = fma(p[k][1] * we, we, quad);
                    }
                }
                ev[0] = ev[1]; ev[1] = ev[2]; ev[2] = en[j];
                cv[0] = cv[1]; cv[1] = cv[2]; cv[2] = cn[j];
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    p[k][0] = p[k][1]; p[k][1] = p[k][2]; p[k][2] = pn[j][k];
                    mu[k][0] = mu[k][1]; mu[k][1] = mn[j][k];
                }
            }
        }
    }
}

// nll[u D + d] = 1/2 sum_k sum_t p_k[t] (W_k e)[t]^2 - 1/2 sum_i log d_i + F/2 log 2 pi, e = x - c; 0 without frames.
template <typename TV, typename TX, int NW>
__global__ __launch_bounds__(kMlpgThreads) void k_mlpg_nll(const double* __restrict__ c, long long ld_c,
                                                          const TX* __restrict__ x, long long ld_x,
                                                          const TV* __restrict__ var, long long ld_var,
                                                          const int* __restrict__ off, int n_utts, int D, MlpgTaps tp,
                                                          double* __restrict__ nll) {
    constexpr int K = NW + 1;
    const long long s = (long long)blockIdx.x * kMlpgThreads + threadIdx.x;
    if (s >= (long long)n_utts * D) return;
    const int u = (int)(s / D), d = (int)(s - (long long)u * D);
    const long long r0 = off[u];
    const int F = off[u + 1] - off[u];
    if (F <= 0) {
        nll[s] = 0.0;
        return;
    }
    double pg[K];
#pragma unroll
    for (int k = 0; k < K; ++k) pg[k] = ld_var == 0 ? 1.0 / (double)var[(long long)k * D + d] : 0.0;
    double quad = 0.0, logdet = 0.0;
    mlpg_nll_sweep<TV, TV, TX, NW, false>(nullptr, 0, var, ld_var, c, ld_c, x, ld_x, r0, F, D, d, tp, pg, 0.0, nullptr, 0,
                                          nullptr, 0, nullptr, nullptr, nullptr, quad, logdet);
    nll[s] = fma(0.5, quad, fma(-0.5, logdet, (double)F * 0.91893853320467274178));   // log(2 pi) / 2
}

// The gradients of go[u D + d] nll[u D + d]: g_mean[t, k D + d] = -go p_k (W_k e)[t] (the forward sweep; g_mean may be null),
//     g_var[t, k D + d] = -go p_k^2 ((W_k e)^2 / 2 - (W_k e)(mu_k - W_k c) - s_k / 2)[t]        (g_var may be null),
// s_k[t] = (W_k A^-1 W_k^T)[t, t] from the band Z = A^-1 within bandwidth 2: the forward sweep leaves l1, l2, 1 / d in the
// three workspace planes, the reverse sweep i = F - 1 .. -1 (row -1: zeros, the dropped tap of frame 0) runs
//     Z[i,i+1] = -l1_{i+1} Z[i+1,i+1] - l2_{i+2} Z[i+1,i+2]      Z[i,i+2] = -l1_{i+1} Z[i+1,i+2] - l2_{i+2} Z[i+2,i+2]
//     Z[i,i]   = 1 / d_i - l1_{i+1} Z[i,i+1] - l2_{i+2} Z[i,i+2]
// with the rows i, i + 1, i + 2 live, and finishes frame t = i + 1 in the step that finishes row i = t - 1:
//     s_k[t] = aa_k . (Z[t+1,t+1], Z[t,t], Z[t-1,t-1]) + 2 (e1_k Z[t-1,t] + ff_k Z[t-1,t+1] + e0_k Z[t,t+1]).
template <typename TM, typename TV, typename TX, int NW>
__global__ __launch_bounds__(kMlpgThreads) void k_mlpg_nll_bwd(const TM* __restrict__ mean, long long ld_mean,
                                                              const TV* __restrict__ var, long long ld_var,
                                                              const double* __restrict__ c, long long ld_c,
                                                              const TX* __restrict__ x, long long ld_x,
                                                              const double* __restrict__ go_all,
                                                              const int* __restrict__ off, int n_utts, int D,
                                                              long long total, MlpgTaps tp, double* __restrict__ g_mean,
                                                              long long ld_gm, double* __restrict__ g_var,
                                                              long long ld_gv, double* __restrict__ work) {
    constexpr int K = NW + 1;
    const long long s = (long long)blockIdx.x * kMlpgThreads + threadIdx.x;
    if (s >= (long long)n_utts * D) return;
    const int u = (int)(s / D), d = (int)(s - (long long)u * D);
    const long long r0 = off[u];
    const int F = off[u + 1] - off[u];
    if (F <= 0) return;
    double* __restrict__ wl1 = work;
    double* __restrict__ wl2 = work + total * (long long)D;
    double* __restrict__ wdi = work + 2 * total * (long long)D;
    const bool gvar = ld_var == 0;
    const double go = go_all[s];
    double pg[K];
#pragma unroll
    for (int k = 0; k < K; ++k) pg[k] = gvar ? 1.0 / (double)var[(long long)k * D + d] : 0.0;
    double quad = 0.0, logdet = 0.0;
    mlpg_nll_sweep<TM, TV, TX, NW, true>(mean, ld_mean, var, ld_var, c, ld_c, x, ld_x, r0, F, D, d, tp, pg, go, g_mean,
                                         ld_gm, g_var, ld_gv, wl1, wl2, wdi, quad, logdet);
    if (!g_var) return;

    // reverse sweep: row i = top - j, finishing frame t = i + 1; kRev rows fetched a chunk ahead.  Rows and frames >= F do
    // not exist and are not read.
    double m1r[kRev], m2r[kRev], dir[kRev], qr[kRev][K];
    TV vr[kRev][K];
    auto fetch_back = [&](int top) {
#pragma unroll
        for (int j = 0; j < kRev; ++j) {
            const int i = top - j, t = i + 1;
            m1r[j] = m2r[j] = dir[j] = 0.0;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                qr[j][k] = 0.0;
                vr[j][k] = (TV)1;
            }
            if (i >= 0) {
                dir[j] = wdi[(r0 + i) * (long long)D + d];
                if (i + 1 < F) m1r[j] = wl1[(r0 + i + 1) * (long long)D + d];
                if (i + 2 < F) m2r[j] = wl2[(r0 + i + 2) * (long long)D + d];
            }
            if (i >= -1 && t < F) {
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    qr[j][k] = g_var[(r0 + t) * ld_gv + (long long)k * D + d];
                    if (!gvar) vr[j][k] = var[(r0 + t) * ld_var + (long long)k * D + d];
                }
            }
        }
    };
    fetch_back(F - 1);
    double z11 = 0.0, z12 = 0.0, z22 = 0.0;   // Z[i+1,i+1], Z[i+1,i+2], Z[i+2,i+2]
    for (int top = F - 1; top >= -1; top -= kRev) {
        double m1c[kRev], m2c[kRev], dic[kRev], qc[kRev][K], pc[kRev][K];
#pragma unroll
        for (int j = 0; j < kRev; ++j) {
            m1c[j] = m1r[j];
            m2c[j] = m2r[j];
            dic[j] = dir[j];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                qc[j][k] = qr[j][k];
                pc[j][k] = gvar ? pg[k] : 1.0 / (double)vr[j][k];
            }
        }
        fetch_back(top - kRev);
#pragma unroll
        for (int j = 0; j < kRev; ++j) {
            const int i = top - j, t = i + 1;
            if (i >= -1) {
                const double z01 = fma(-m2c[j], z12, -m1c[j] * z11);
                const double z02 = fma(-m2c[j], z22, -m1c[j] * z12);
                const double z00 = fma(-m2c[j], z02, fma(-m1c[j], z01, dic[j]));
                if (t < F) {
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        const double diag = fma(tp.aa[k][2], z00, fma(tp.aa[k][1], z11, tp.aa[k][0] * z22));
                        const double offd = fma(tp.e0[k], z12, fma(tp.ff[k], z02, tp.e1[k] * z01));
                        const double sk = fma(2.0, offd, diag);
                        const double pk = pc[j][k];
                        g_var[(r0 + t) * ld_gv + (long long)k * D + d] = -go * (pk * pk) * fma(-0.5, sk, qc[j][k]);
                    }
                }
                z22 = z11;
                z12 = z01;
                z11 = z00;
            }
        }
    }
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

// (callers have checked that n_tiles * width fits one launch)
void colsum_launch(hipStream_t s, const double* x, long long ld_x, long long total, long long width, double* sums,
                   double* work) {
    const long long n_tiles = (total + kColTile - 1) / kColTile;
    const long long n = n_tiles * width;
    hipLaunchKernelGGL(k_mlpg_colsum_tiles, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, ld_x, total, width,
                       n_tiles, work);
    hipLaunchKernelGGL(k_mlpg_colsum_final, dim3((unsigned)((width + 255) / 256)), dim3(256), 0, s, (const double*)work,
                       width, n_tiles, sums);
}

template <typename TM, typename TV>
void var_bwd_launch(hipStream_t s, const double* z, long long ld_z, const double* c, long long ld_c, const void* mean,
                    long long ld_mean, const void* var, long long ld_var, const int* off, int n_utts, int D, int K,
                    long long total, const MlpgTaps& tp, double* g, long long ld_g) {
    const long long n = total * K * D;
    hipLaunchKernelGGL((k_mlpg_var_bwd<TM, TV>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, z, ld_z, c, ld_c,
                       (const TM*)mean, ld_mean, (const TV*)var, ld_var, off, n_utts, D, K, total, tp, g, ld_g);
}

template <typename TV, typename TX>
void nll_launch(hipStream_t s, int n_win, const double* c, long long ld_c, const void* x, long long ld_x, const void* var,
                long long ld_var, const int* off, int n_utts, int D, const MlpgTaps& tp, double* nll) {
    const long long systems = (long long)n_utts * D;
    const dim3 grid((unsigned)((systems + kMlpgThreads - 1) / kMlpgThreads)), block(kMlpgThreads);
    if (n_win == 1)
        hipLaunchKernelGGL((k_mlpg_nll<TV, TX, 1>), grid, block, 0, s, c, ld_c, (const TX*)x, ld_x, (const TV*)var, ld_var,
                           off, n_utts, D, tp, nll);
    else
        hipLaunchKernelGGL((k_mlpg_nll<TV, TX, 2>), grid, block, 0, s, c, ld_c, (const TX*)x, ld_x, (const TV*)var, ld_var,
                           off, n_utts, D, tp, nll);
}

template <typename TM, typename TV, typename TX>
void nll_bwd_launch(hipStream_t s, int n_win, const void* mean, long long ld_mean, const void* var, long long ld_var,
                    const double* c, long long ld_c, const void* x, long long ld_x, const double* go, const int* off,
                    int n_utts, int D, long long total, const MlpgTaps& tp, double* g_mean, long long ld_gm, double* g_var,
                    long long ld_gv, double* work) {
    const long long systems = (long long)n_utts * D;
    const dim3 grid((unsigned)((systems + kMlpgThreads - 1) / kMlpgThreads)), block(kMlpgThreads);
    if (n_win == 1)
        hipLaunchKernelGGL((k_mlpg_nll_bwd<TM, TV, TX, 1>), grid, block, 0, s, (const TM*)mean, ld_mean, (const TV*)var,
                           ld_var, c, ld_c, (const TX*)x, ld_x, go, off, n_utts, D, total, tp, g_mean, ld_gm, g_var, ld_gv,
                           work);
    else
        hipLaunchKernelGGL((k_mlpg_nll_bwd<TM, TV, TX, 2>), grid, block, 0, s, (const TM*)mean, ld_mean, (const TV*)var,
                           ld_var, c, ld_c, (const TX*)x, ld_x, go, off, n_utts, D, total, tp, g_mean, ld_gm, g_var, ld_gv,
                           work);
}

template <typename TM, typename TV>
void nll_bwd_launch_x(bool x_f64, hipStream_t s, int n_win, const void* mean, long long ld_mean, const void* var,
                      long long ld_var, const double* c, long long ld_c, const void* x, long long ld_x, const double* go,
                      const int* off, int n_utts, int D, long long total, const MlpgTaps& tp, double* g_mean,
                      long long ld_gm, double* g_var, long long ld_gv, double* work) {
    if (x_f64)
        nll_bwd_launch<TM, TV, double>(s, n_win, mean, ld_mean, var, ld_var, c, ld_c, x, ld_x, go, off, n_utts, D, total, tp,
                                       g_mean, ld_gm, g_var, ld_gv, work);
    else
        nll_bwd_launch<TM, TV, float>(s, n_win, mean, ld_mean, var, ld_var, c, ld_c, x, ld_x, go, off, n_utts, D, total, tp,
                                      g_mean, ld_gm, g_var, ld_gv, work);
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

int64_t mpx_mlpg_colsum_work_doubles(int64_t total_frames, int64_t width) {
    if (total_frames < 0 || width < 1) return 0;
    return (total_frames + kColTile - 1) / kColTile * width;   // one partial sum per tile of kColTile rows and column
}

int mpx_mlpg_column_sums(void* stream, const double* x, int64_t ld_x, int64_t total_frames, int64_t width, double* sums,
                         double* work) {
    static const char* who = "mpx_mlpg_column_sums";
    if (width < 1) return fail(MPX_ERR_ARG, "%s: width must be >= 1", who);
    if (total_frames < 0) return fail(MPX_ERR_ARG, "%s: negative total_frames", who);
    if (total_frames > 0x7fffffffLL) return fail(MPX_ERR_ARG, "%s: total_frames above 2^31 - 1", who);
    if (ld_x < width) return fail(MPX_ERR_ARG, "%s: ld_x below the row width", who);
    if ((total_frames + kColTile - 1) / kColTile > 0x7fffffffLL * 256 / width)
        return fail(MPX_ERR_ARG, "%s: too many elements for one launch", who);
    if (total_frames == 0) return MPX_OK;
    if (!x || !sums || !work) return fail(MPX_ERR_ARG, "%s: null pointer", who);
    colsum_launch((hipStream_t)stream, x, ld_x, total_frames, width, sums, work);
    MPX_HIP_CHECK(hipGetLastError());
    return MPX_OK;
}

int mpx_mlpg_var_backward(void* stream, const double* z, int64_t ld_z, const double* c, int64_t ld_c, const void* mean,
                          int32_t mean_f64, int64_t ld_mean, const void* var, int32_t var_f64, int64_t ld_var,
                          const int32_t* utt_frame_off, int32_t n_utts, int64_t total_frames, int32_t D, int32_t n_win,
                          const double* windows, double* g, int64_t ld_g, double* gsum, double* work) {
    static const char* who = "mpx_mlpg_var_backward";
    if (int rc = mlpg_check(who, total_frames, n_utts, D, n_win)) return rc;
    const int K = n_win + 1;
    if (ld_z < D || ld_c < D) return fail(MPX_ERR_ARG, "%s: ld_z or ld_c below D", who);
    if (ld_mean < (int64_t)K * D) return fail(MPX_ERR_ARG, "%s: ld_mean below the row width", who);
    if (ld_var != 0 && ld_var < (int64_t)K * D) return fail(MPX_ERR_ARG, "%s: ld_var must be 0 (one row) or >= K * D", who);
    if (ld_g < (int64_t)K * D) return fail(MPX_ERR_ARG, "%s: ld_g below K * D", who);
    if (total_frames * K > 0x7fffffffLL * 256 / D) return fail(MPX_ERR_ARG, "%s: too many elements for one launch", who);
    if (!windows) return fail(MPX_ERR_ARG, "%s: null pointer (windows)", who);
    MlpgTaps tp;
    if (int rc = mlpg_taps(who, n_win, windows, tp)) return rc;
    if (total_frames == 0 || n_utts == 0) return MPX_OK;
    if (!z || !c || !mean || !var || !utt_frame_off || !g) return fail(MPX_ERR_ARG, "%s: null pointer", who);
    if (ld_var == 0 && (!gsum || !work))
        return fail(MPX_ERR_ARG, "%s: null pointer (gsum, work: the column sums of a global variance row)", who);
    const hipStream_t s = (hipStream_t)stream;
    const int* off = (const int*)utt_frame_off;
    if (mean_f64) {
        if (var_f64) var_bwd_launch<double, double>(s, z, ld_z, c, ld_c, mean, ld_mean, var, ld_var, off, n_utts, D, K, total_frames, tp, g, ld_g);
        else var_bwd_launch<double, float>(s, z, ld_z, c, ld_c, mean, ld_mean, var, ld_var, off, n_utts, D, K, total_frames, tp, g, ld_g);
    } else {
        if (var_f64) var_bwd_launch<float, double>(s, z, ld_z, c, ld_c, mean, ld_mean, var, ld_var, off, n_utts, D, K, total_frames, tp, g, ld_g);
        else var_bwd_launch<float, float>(s, z, ld_z, c, ld_c, mean, ld_mean, var, ld_var, off, n_utts, D, K, total_frames, tp, g, ld_g);
    }
    if (ld_var == 0) colsum_launch(s, g, ld_g, total_frames, (long long)K * D, gsum, work);   // (fewer elements than g has)
    MPX_HIP_CHECK(hipGetLastError());
    return MPX_OK;
}

int mpx_mlpg_trajectory_nll(void* stream, const double* c, int64_t ld_c, const void* x, int32_t x_f64, int64_t ld_x,
                            const void* var, int32_t var_f64, int64_t ld_var, const int32_t* utt_frame_off, int32_t n_utts,
                            int64_t total_frames, int32_t D, int32_t n_win, const double* windows, double* nll) {
    static const char* who = "mpx_mlpg_trajectory_nll";
    if (int rc = mlpg_check(who, total_frames, n_utts, D, n_win)) return rc;
    const int K = n_win + 1;
    if (ld_c < D || ld_x < D) return fail(MPX_ERR_ARG, "%s: ld_c or ld_x below D", who);
    if (ld_var != 0 && ld_var < (int64_t)K * D) return fail(MPX_ERR_ARG, "%s: ld_var must be 0 (one row) or >= K * D", who);
    if (!windows) return fail(MPX_ERR_ARG, "%s: null pointer (windows)", who);
    MlpgTaps tp;
    if (int rc = mlpg_taps(who, n_win, windows, tp)) return rc;
    if (total_frames == 0 || n_utts == 0) return MPX_OK;
    if (!c || !x || !var || !utt_frame_off || !nll) return fail(MPX_ERR_ARG, "%s: null pointer", who);
    const hipStream_t s = (hipStream_t)stream;
    const int* off = (const int*)utt_frame_off;
    if (var_f64) {
        if (x_f64) nll_launch<double, double>(s, n_win, c, ld_c, x, ld_x, var, ld_var, off, n_utts, D, tp, nll);
        else nll_launch<double, float>(s, n_win, c, ld_c, x, ld_x, var, ld_var, off, n_utts, D, tp, nll);
    } else {
        if (x_f64) nll_launch<float, double>(s, n_win, c, ld_c, x, ld_x, var, ld_var, off, n_utts, D, tp, nll);
        else nll_launch<float, float>(s, n_win, c, ld_c, x, ld_x, var, ld_var, off, n_utts, D, tp, nll);
    }
    MPX_HIP_CHECK(hipGetLastError());
    return MPX_OK;
}

int64_t mpx_mlpg_nll_work_doubles(int64_t total_frames, int32_t D) {
    if (total_frames < 0 || D < 1) return 0;
    return 3 * total_frames * (int64_t)D;   // the planes l1, l2, 1 / d of the factor, [total_frames x D] each
}

int mpx_mlpg_trajectory_nll_backward(void* stream, const void* mean, int32_t mean_f64, int64_t ld_mean, const void* var,
                                     int32_t var_f64, int64_t ld_var, const double* c, int64_t ld_c, const void* x,
                                     int32_t x_f64, int64_t ld_x, const double* go, const int32_t* utt_frame_off,
                                     int32_t n_utts, int64_t total_frames, int32_t D, int32_t n_win, const double* windows,
                                     double* g_mean, int64_t ld_gm, double* g_var, int64_t ld_gv, double* work) {
    static const char* who = "mpx_mlpg_trajectory_nll_backward";
    if (int rc = mlpg_check(who, total_frames, n_utts, D, n_win)) return rc;
    const int K = n_win + 1;
    if (ld_mean < (int64_t)K * D) return fail(MPX_ERR_ARG, "%s: ld_mean below the row width", who);
    if (ld_var != 0 && ld_var < (int64_t)K * D) return fail(MPX_ERR_ARG, "%s: ld_var must be 0 (one row) or >= K * D", who);
    if (ld_c < D || ld_x < D) return fail(MPX_ERR_ARG, "%s: ld_c or ld_x below D", who);
    if ((g_mean && ld_gm < (int64_t)K * D) || (g_var && ld_gv < (int64_t)K * D))
        return fail(MPX_ERR_ARG, "%s: ld_gm or ld_gv below K * D", who);
    if (!windows) return fail(MPX_ERR_ARG, "%s: null pointer (windows)", who);
    MlpgTaps tp;
    if (int rc = mlpg_taps(who, n_win, windows, tp)) return rc;
    if (total_frames == 0 || n_utts == 0) return MPX_OK;
    if (!g_mean && !g_var) return fail(MPX_ERR_ARG, "%s: null pointer (g_mean and g_var: nothing to compute)", who);
    if (!mean || !var || !c || !x || !go || !utt_frame_off) return fail(MPX_ERR_ARG, "%s: null pointer", who);
    if (g_var && !work) return fail(MPX_ERR_ARG, "%s: null pointer (work, needed with g_var)", who);
    const hipStream_t s = (hipStream_t)stream;
    const int* off = (const int*)utt_frame_off;
#define MPX_NLL_BWD(TM, TV)                                                                                              \
    nll_bwd_launch_x<TM, TV>(x_f64 != 0, s, n_win, mean, ld_mean, var, ld_var, c, ld_c, x, ld_x, go, off, n_utts, D,      \
                             total_frames, tp, g_mean, ld_gm, g_var, ld_gv, work)
    if (mean_f64) {
        if (var_f64) MPX_NLL_BWD(double, double); else MPX_NLL_BWD(double, float);
    } else {
        if (var_f64) MPX_NLL_BWD(float, double); else MPX_NLL_BWD(float, float);
    }
#undef MPX_NLL_BWD
    MPX_HIP_CHECK(hipGetLastError());
    return MPX_OK;
}

}  // extern "C"
