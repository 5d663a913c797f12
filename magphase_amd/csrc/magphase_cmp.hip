// magphase_cmp.hip -- acoustic composition: the rows an acoustic model is trained on, the inverse of
// mlpg_streams_batch.
//
// The static matrix x [total x SD] holds the streams' statics side by side (stream s of dimension D_s from column s0_s), the
// output y [total x W] holds stream s as [static | delta | acc] in K D_s columns from column K s0_s, then ONE voicing column.
//   k_cmp_neighbours      one workgroup per utterance: per frame the nearest voiced frame at or before and at or after it
//   k_cmp_compose         one thread per element of y: the (interpolated) statics, the window taps, (y - mean) / std
//   k_cmp_compose_bwd     one thread per element of x: the adjoint in gather form
//   k_cmp_moment_tiles,   count, column sums and centred sums of squares in the order of mpx_mlpg_column_sums (tiles of 128
//   k_cmp_moment_final    rows ascending, then the tiles ascending)
//
// THE ROUNDING RULE OF THIS UNIT.  Every float64 expression below is evaluated as it is written: one rounding per product,
// quotient, sum and difference, left to right, and NO fused multiply-add -- the pragma below forbids the compiler to
// contract a * b + c, and no fma() is called.  tests/cmp_model.py writes the same expressions in numpy, which has no fused
// multiply-add either, so model and kernel agree bit for bit in float64 and the float32 store rounds the same number.  With
// taps that are powers of two (the default windows) the products are exact and the values are k_mlpg_apply's as well.
#include "mpx_common.hpp"

#pragma clang fp contract(off)

using namespace mpx;

namespace {

constexpr int kCmpMaxStreams = 16;
constexpr int kCmpMaxWin = 2;
constexpr int kNbThreads = 256;     // four waves: one pass covers 256 frames of the utterance
constexpr int kNbWaves = kNbThreads / 64;
constexpr int kMomTile = 128;       // rows per partial sum (mpx_mlpg_column_sums' tile)
constexpr int kNone = 0x7fffffff;

// The layout as the kernels take it (by value).
struct CmpLayout {
    int n;                       // streams
    int D[kCmpMaxStreams];       // dimension
    int s0[kCmpMaxStreams];      // first static column; the first output column is K * s0
    int SD;                      // sum of D: the width of the static matrix
    int W;                       // K * SD + vuv
    int K;                       // 1 + n_win
    int interp;                  // the stream carried through unvoiced frames, or -1
    int vuv;                     // a voicing column follows the streams
    double w[kCmpMaxWin + 1][3]; // taps (w[-1], w[0], w[+1]); stream 0 = (0, 1, 0)
};

__device__ __forceinline__ int cmp_utt_of_frame(const int* __restrict__ off, int n_utts, long long t) {
    int lo = 0, hi = n_utts;          // the utterance u with off[u] <= t < off[u + 1] (empty utterances are passed over)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((long long)off[mid] <= t) lo = mid; else hi = mid;
    }
    return lo;
}

// Voiced: v > 0.  A NaN compares false: unvoiced.
template <typename TV>
__device__ __forceinline__ bool cmp_voiced(TV v) {
    return (double)v > 0.0;
}

// prev[t] = the last voiced frame <= t, next[t] = the first voiced frame >= t (utterance-relative, -1: none), planes
// nb[0 .. total) and nb[total .. 2 total).  A pass covers 256 frames, a wave 64 of them: the ballot of the voiced mask gives
// a lane its neighbour inside the tile by a leading / trailing zero count, the waves' outermost voiced frames go through
// LDS, and the carry of the earlier (later) passes is the same number in every thread.  Two sweeps: ascending for prev,
// descending for next.  The LDS rows alternate with the pass, so one barrier per pass is enough.
template <typename TV>
__global__ __launch_bounds__(kNbThreads) void k_cmp_neighbours(const TV* __restrict__ v, long long ld_v,
                                                              const int* __restrict__ off, long long total,
                                                              int* __restrict__ nb) {
    __shared__ int edge_p[2][kNbWaves];
    __shared__ int edge_n[2][kNbWaves];
    const int u = blockIdx.x;
    const long long r0 = off[u];
    const int F = off[u + 1] - off[u];
    if (F <= 0) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int* __restrict__ prev = nb + r0;
    int* __restrict__ next = nb + total + r0;
    const int n_pass = (F + kNbThreads - 1) / kNbThreads;

    int carry = -1;
    for (int ps = 0; ps < n_pass; ++ps) {
        const int t = ps * kNbThreads + (int)threadIdx.x;
        const bool voiced = t < F && cmp_voiced(v[(r0 + t) * ld_v]);
        const unsigned long long m = __ballot(voiced);
        const int base = ps * kNbThreads + wave * 64;
        if (lane == 0) edge_p[ps & 1][wave] = m ? base + 63 - __clzll((long long)m) : -1;
        __syncthreads();
        int c = carry;
        for (int w = 0; w < wave; ++w) c = max(c, edge_p[ps & 1][w]);
        const unsigned long long below = m & (~0ull >> (63 - lane));   // lanes 0 .. lane
        if (t < F) prev[t] = below ? base + 63 - __clzll((long long)below) : c;
        for (int w = 0; w < kNbWaves; ++w) carry = max(carry, edge_p[ps & 1][w]);
    }

    carry = kNone;
    for (int ps = n_pass - 1; ps >= 0; --ps) {
        const int t = ps * kNbThreads + (int)threadIdx.x;
        const bool voiced = t < F && cmp_voiced(v[(r0 + t) * ld_v]);
        const unsigned long long m = __ballot(voiced);
        const int base = ps * kNbThreads + wave * 64;
        if (lane == 0) edge_n[ps & 1][wave] = m ? base + __ffsll((long long)m) - 1 : kNone;
        __syncthreads();
        int c = carry;
        for (int w = wave + 1; w < kNbWaves; ++w) c = min(c, edge_n[ps & 1][w]);
        const unsigned long long above = m & (~0ull << lane);          // lanes lane .. 63
        const int n = above ? base + __ffsll((long long)above) - 1 : c;
        if (t < F) next[t] = n == kNone ? -1 : n;
        for (int w = 0; w < kNbWaves; ++w) carry = min(carry, edge_n[ps & 1][w]);
    }
}

// The static value of frame t (0 <= t < F) of column sc as the composition reads it.  interp: the column belongs to the
// stream carried through unvoiced frames -- a voiced frame gives its own value; an unvoiced one zero (zeros), the line
// through the voiced frames p < t < n on either side, the nearest voiced value before the first / after the last voiced
// frame, fill without any.  The value stored in an unvoiced entry is never loaded.  Neighbours outside the utterance
// (a table this kernel did not get from k_cmp_neighbours) count as none.
template <typename TX>
__device__ __forceinline__ double cmp_static(const TX* __restrict__ x, long long ld_x, long long r0, int t, int F, int sc,
                                             bool interp, const int* __restrict__ nb, long long total, int zeros,
                                             double fill) {
    if (!interp) return (double)x[(r0 + t) * ld_x + sc];
    int p = nb[r0 + t], n = nb[total + r0 + t];
    if (p < 0 || p > t) p = -1;
    if (n < t || n >= F) n = -1;
    if (p == t) return (double)x[(r0 + t) * ld_x + sc];
    if (zeros) return 0.0;
    if (p < 0 && n < 0) return fill;
    if (p < 0) return (double)x[(r0 + n) * ld_x + sc];
    if (n < 0) return (double)x[(r0 + p) * ld_x + sc];
    const double lo = (double)x[(r0 + p) * ld_x + sc], hi = (double)x[(r0 + n) * ld_x + sc];
    const double slope = (hi - lo) / (double)(n - p);
    return slope * (double)(t - p) + lo;
}

// y[r, c]: the stream s, window k and dimension d of column c; sum_j w_k[j] x~[t + j, s0_s + d] over the taps inside the
// utterance in the order -1, 0, +1 (a dropped tap is skipped, not added as a zero), then (y - mean[c]) / std[c]; the voicing
// column is 1 where the frame is voiced.  Consecutive threads store consecutive columns.
template <typename TX, typename TO>
__global__ __launch_bounds__(256) void k_cmp_compose(const TX* __restrict__ x, long long ld_x, const int* __restrict__ nb,
                                                     const int* __restrict__ off, int n_utts, long long total,
                                                     CmpLayout L, int zeros, double fill,
                                                     const double* __restrict__ mean, const double* __restrict__ sd,
                                                     TO* __restrict__ y, long long ld_y) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total * (long long)L.W) return;
    const long long r = e / L.W;
    const int c = (int)(e - r * L.W);
    const int u = cmp_utt_of_frame(off, n_utts, r);
    const long long r0 = off[u];
    const int F = off[u + 1] - off[u], t = (int)(r - r0);
    double acc;
    if (c >= L.K * L.SD) {           // the voicing column
        acc = nb[r] == t ? 1.0 : 0.0;
    } else {
        int s = 0;
        while (s + 1 < L.n && c >= L.K * L.s0[s + 1]) ++s;
        const int rel = c - L.K * L.s0[s], k = rel / L.D[s], d = rel - k * L.D[s], sc = L.s0[s] + d;
        const bool interp = s == L.interp;
        if (k == 0) {
            acc = cmp_static(x, ld_x, r0, t, F, sc, interp, nb, total, zeros, fill);
        } else {
            const bool has_prev = t > 0, has_next = t + 1 < F;
            acc = 0.0;
            if (has_prev) acc = L.w[k][0] * cmp_static(x, ld_x, r0, t - 1, F, sc, interp, nb, total, zeros, fill);
            {
                const double x0 = cmp_static(x, ld_x, r0, t, F, sc, interp, nb, total, zeros, fill);
                acc = has_prev ? acc + L.w[k][1] * x0 : L.w[k][1] * x0;
            }
            if (has_next) acc = acc + L.w[k][2] * cmp_static(x, ld_x, r0, t + 1, F, sc, interp, nb, total, zeros, fill);
        }
    }
    if (mean) acc = (acc - mean[c]) / sd[c];
    y[r * ld_y + c] = (TO)acc;
}

// h[s, c] = g[s, c] / std[c]; the gradient of the substituted statics x~[t, sc]: over the windows k in ascending order
//     w_k[+1] h[t - 1, c_k] + w_k[0] h[t, c_k] + w_k[-1] h[t + 1, c_k]       (rows inside the utterance; c_k = K s0 + k D + d)
// -- row s reaches frame t through its tap t - s, which row s never drops because t is inside.
__device__ __forceinline__ double cmp_gx(const float* __restrict__ g, long long ld_g, const double* __restrict__ sd,
                                         long long r0, int t, int F, int c0, int D, const CmpLayout& L) {
    double acc = 0.0;
    for (int k = 0; k < L.K; ++k) {
        const int c = c0 + k * D;
        const double is = sd ? sd[c] : 1.0;
        if (k == 0) {
            acc = (double)g[(r0 + t) * ld_g + c] / is;
            continue;
        }
        if (t > 0) acc = acc + L.w[k][2] * ((double)g[(r0 + t - 1) * ld_g + c] / is);
        acc = acc + L.w[k][1] * ((double)g[(r0 + t) * ld_g + c] / is);
        if (t + 1 < F) acc = acc + L.w[k][0] * ((double)g[(r0 + t + 1) * ld_g + c] / is);
    }
    return acc;
}

// gx[r, sc] = dL/dx[t, sc], one thread (one writer) per element.  A column of the carried stream: an unvoiced frame gets
// exactly 0; a voiced frame v with the voiced frames p < v < n next to it sums, in ascending frame order,
//     (t - p) / (v - p) gx~[t] for p < t < v  (1 without p: the held frames),   gx~[v],
//     (1 - (t - v) / (n - v)) gx~[t] for v < t < n  (1 without n).
__global__ __launch_bounds__(256) void k_cmp_compose_bwd(const float* __restrict__ g, long long ld_g,
                                                         const int* __restrict__ nb, const int* __restrict__ off,
                                                         int n_utts, long long total, CmpLayout L,
                                                         const double* __restrict__ sd, double* __restrict__ gx,
                                                         long long ld_gx) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total * (long long)L.SD) return;
    const long long r = e / L.SD;
    const int sc = (int)(e - r * L.SD);
    const int u = cmp_utt_of_frame(off, n_utts, r);
    const long long r0 = off[u];
    const int F = off[u + 1] - off[u], v = (int)(r - r0);
    int s = 0;
    while (s + 1 < L.n && sc >= L.s0[s + 1]) ++s;
    const int D = L.D[s], c0 = L.K * L.s0[s] + (sc - L.s0[s]);
    double acc;
    if (s != L.interp) {
        acc = cmp_gx(g, ld_g, sd, r0, v, F, c0, D, L);
    } else if (nb[r] != v) {
        acc = 0.0;
    } else {
        int p = v > 0 ? nb[r - 1] : -1;
        int n = v + 1 < F ? nb[total + r + 1] : -1;
        if (p >= v) p = -1;
        if (n <= v || n >= F) n = -1;
        const int lo = p < 0 ? 0 : p + 1, hi = n < 0 ? F - 1 : n - 1;
        acc = 0.0;
        for (int t = lo; t <= hi; ++t) {
            double wt = 1.0;
            if (t < v && p >= 0) wt = (double)(t - p) / (double)(v - p);
            if (t > v && n >= 0) wt = 1.0 - (double)(t - v) / (double)(n - v);
            acc = acc + wt * cmp_gx(g, ld_g, sd, r0, t, F, c0, D, L);
        }
    }
    gx[r * ld_gx + sc] = acc;
}

// part[tile, col] = sum over the rows of the tile, ascending, of x (mean == null) or of (x - mean[col])^2.
template <typename TX>
__global__ __launch_bounds__(256) void k_cmp_moment_tiles(const TX* __restrict__ x, long long ld_x, long long total,
                                                          long long width, long long n_tiles,
                                                          const double* __restrict__ sums, double* __restrict__ part) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_tiles * width) return;
    const long long tile = e / width, col = e - tile * width;
    const long long ra = tile * kMomTile, rb = ra + kMomTile < total ? ra + kMomTile : total;
    double s = 0.0;
    if (sums) {
        const double m = sums[col] / (double)total;
        for (long long r = ra; r < rb; ++r) {
            const double dv = (double)x[r * ld_x + col] - m;
            s = s + dv * dv;
        }
    } else {
        for (long long r = ra; r < rb; ++r) s = s + (double)x[r * ld_x + col];
    }
    part[e] = s;
}

// dst[col] = sum over the tiles, ascending; count (may be null) = total.
__global__ __launch_bounds__(256) void k_cmp_moment_final(const double* __restrict__ part, long long width,
                                                          long long n_tiles, long long total, double* __restrict__ count,
                                                          double* __restrict__ dst) {
    const long long col = (long long)blockIdx.x * 256 + threadIdx.x;
    if (col >= width) return;
    double s = 0.0;
    for (long long t = 0; t < n_tiles; ++t) s = s + part[t * width + col];
    dst[col] = s;
    if (count && col == 0) count[0] = (double)total;
}

int cmp_layout(const char* who, const int32_t* dims, int32_t n_streams, int32_t interp_stream, int32_t vuv, int32_t n_win,
               const double* windows, int64_t total_frames, int32_t n_utts, CmpLayout& L) {
    memset(&L, 0, sizeof(L));
    if (!dims) return fail(MPX_ERR_ARG, "%s: null pointer (dims)", who);
    if (n_streams < 1 || n_streams > kCmpMaxStreams) return fail(MPX_ERR_ARG, "%s: 1 to 16 streams", who);
    if (n_win < 0 || n_win > kCmpMaxWin) return fail(MPX_ERR_ARG, "%s: n_win must be 0, 1 or 2", who);
    if (n_win > 0 && !windows) return fail(MPX_ERR_ARG, "%s: null pointer (windows)", who);
    if (interp_stream < -1 || interp_stream >= n_streams) return fail(MPX_ERR_ARG, "%s: interp_stream out of range", who);
    if (vuv && interp_stream < 0) return fail(MPX_ERR_ARG, "%s: the voicing column needs the carried stream", who);
    if (total_frames < 0) return fail(MPX_ERR_ARG, "%s: negative total_frames", who);
    if (n_utts < 0) return fail(MPX_ERR_ARG, "%s: negative n_utts", who);
    if (total_frames > 0x7fffffffLL) return fail(MPX_ERR_ARG, "%s: total_frames above 2^31 - 1 (int32 frame offsets)", who);
    L.n = n_streams;
    L.K = n_win + 1;
    L.interp = interp_stream;
    L.vuv = vuv ? 1 : 0;
    long long sd = 0;
    for (int s = 0; s < n_streams; ++s) {
        if (dims[s] < 1) return fail(MPX_ERR_ARG, "%s: every stream dimension must be >= 1", who);
        L.D[s] = dims[s];
        L.s0[s] = (int)sd;
        sd += dims[s];
        if (sd > (1 << 20)) return fail(MPX_ERR_ARG, "%s: more than 2^20 static columns", who);
    }
    L.SD = (int)sd;
    L.W = L.K * L.SD + L.vuv;
    for (int k = 0; k <= n_win; ++k)
        for (int j = 0; j < 3; ++j) {
            L.w[k][j] = (k == 0) ? (j == 1 ? 1.0 : 0.0) : windows[3 * (k - 1) + j];
            if (!std::isfinite(L.w[k][j])) return fail(MPX_ERR_ARG, "%s: a window tap is not finite", who);
        }
    if (total_frames > 0x7fffffffLL * 256 / L.W) return fail(MPX_ERR_ARG, "%s: too many elements for one launch", who);
    return MPX_OK;
}

template <typename TX>
void compose_launch(hipStream_t st, bool out_f64, const void* x, long long ld_x, const int* nb, const int* off, int n_utts,
                    long long total, const CmpLayout& L, int zeros, double fill, const double* mean, const double* sd,
                    void* y, long long ld_y) {
    const long long n = total * L.W;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (out_f64)
        hipLaunchKernelGGL((k_cmp_compose<TX, double>), grid, block, 0, st, (const TX*)x, ld_x, nb, off, n_utts, total, L,
                           zeros, fill, mean, sd, (double*)y, ld_y);
    else
        hipLaunchKernelGGL((k_cmp_compose<TX, float>), grid, block, 0, st, (const TX*)x, ld_x, nb, off, n_utts, total, L,
                           zeros, fill, mean, sd, (float*)y, ld_y);
}

template <typename TX>
void moments_launch(hipStream_t st, const void* x, long long ld_x, long long total, long long width, double* out,
                    double* work) {
    const long long n_tiles = (total + kMomTile - 1) / kMomTile;
    const long long n = n_tiles * width;
    const dim3 tg((unsigned)((n + 255) / 256)), fg((unsigned)((width + 255) / 256)), block(256);
    hipLaunchKernelGGL((k_cmp_moment_tiles<TX>), tg, block, 0, st, (const TX*)x, ld_x, total, width, n_tiles,
                       (const double*)nullptr, work);
    hipLaunchKernelGGL(k_cmp_moment_final, fg, block, 0, st, (const double*)work, width, n_tiles, total, out, out + 1);
    hipLaunchKernelGGL((k_cmp_moment_tiles<TX>), tg, block, 0, st, (const TX*)x, ld_x, total, width, n_tiles,
                       (const double*)(out + 1), work);
    hipLaunchKernelGGL(k_cmp_moment_final, fg, block, 0, st, (const double*)work, width, n_tiles, total,
                       (double*)nullptr, out + 1 + width);
}

}  // namespace

extern "C" {

int mpx_cmp_voiced_neighbours(void* stream, const void* v, int32_t v_f64, int64_t ld_v, const int32_t* utt_frame_off,
                              int32_t n_utts, int64_t total_frames, int32_t* nb) {
    static const char* who = "mpx_cmp_voiced_neighbours";
    if (total_frames < 0) return fail(MPX_ERR_ARG, "%s: negative total_frames", who);
    if (n_utts < 0) return fail(MPX_ERR_ARG, "%s: negative n_utts", who);
    if (total_frames > 0x7fffffffLL) return fail(MPX_ERR_ARG, "%s: total_frames above 2^31 - 1 (int32 frame offsets)", who);
    if (ld_v < 1) return fail(MPX_ERR_ARG, "%s: ld_v below 1", who);
    if (total_frames == 0 || n_utts == 0) return MPX_OK;
    if (!v || !utt_frame_off || !nb) return fail(MPX_ERR_ARG, "%s: null pointer", who);
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)n_utts), block(kNbThreads);
    if (v_f64)
        hipLaunchKernelGGL((k_cmp_neighbours<double>), grid, block, 0, st, (const double*)v, (long long)ld_v,
                           (const int*)utt_frame_off, (long long)total_frames, (int*)nb);
    else
        hipLaunchKernelGGL((k_cmp_neighbours<float>), grid, block, 0, st, (const float*)v, (long long)ld_v,
                           (const int*)utt_frame_off, (long long)total_frames, (int*)nb);
    MPX_HIP_CHECK(hipGetLastError());
    return MPX_OK;
}

int mpx_cmp_compose(void* stream, const void* x, int32_t x_f64, int64_t ld_x, const int32_t* dims, int32_t n_streams,
                    int32_t interp_stream, int32_t interp_zeros, double unv_fill, int32_t vuv, const int32_t* nb,
                    const int32_t* utt_frame_off, int32_t n_utts, int64_t total_frames, int32_t n_win,
                    const double* windows, const double* mean, const double* std_dev, void* out, int32_t out_f64,
                    int64_t ld_out) {
    static const char* who = "mpx_cmp_compose";
    CmpLayout L;
    if (int rc = cmp_layout(who, dims, n_streams, interp_stream, vuv, n_win, windows, total_frames, n_utts, L)) return rc;
    if (ld_x < L.SD) return fail(MPX_ERR_ARG, "%s: ld_x below the width of the static matrix", who);
    if (ld_out < L.W) return fail(MPX_ERR_ARG, "%s: ld_out below the row width", who);
    if ((mean == nullptr) != (std_dev == nullptr)) return fail(MPX_ERR_ARG, "%s: mean and std come together", who);
    if (!std::isfinite(unv_fill)) return fail(MPX_ERR_ARG, "%s: unv_fill is not finite", who);
    if (total_frames == 0 || n_utts == 0) return MPX_OK;
    if (!x || !utt_frame_off || !out) return fail(MPX_ERR_ARG, "%s: null pointer", who);
    if (interp_stream >= 0 && !nb) return fail(MPX_ERR_ARG, "%s: null pointer (nb, needed with a carried stream)", who);
    const hipStream_t st = (hipStream_t)stream;
    if (x_f64)
        compose_launch<double>(st, out_f64 != 0, x, ld_x, (const int*)nb, (const int*)utt_frame_off, n_utts, total_frames, L,
                               interp_zeros != 0, unv_fill, mean, std_dev, out, ld_out);
    else
        compose_launch<float>(st, out_f64 != 0, x, ld_x, (const int*)nb, (const int*)utt_frame_off, n_utts, total_frames, L,
                              interp_zeros != 0, unv_fill, mean, std_dev, out, ld_out);
    MPX_HIP_CHECK(hipGetLastError());
    return MPX_OK;
}

int mpx_cmp_compose_backward(void* stream, const float* g, int64_t ld_g, const int32_t* dims, int32_t n_streams,
                             int32_t interp_stream, int32_t vuv, const int32_t* nb, const int32_t* utt_frame_off,
                             int32_t n_utts, int64_t total_frames, int32_t n_win, const double* windows,
                             const double* std_dev, double* gx, int64_t ld_gx) {
    static const char* who = "mpx_cmp_compose_backward";
    CmpLayout L;
    if (int rc = cmp_layout(who, dims, n_streams, interp_stream, vuv, n_win, windows, total_frames, n_utts, L)) return rc;
    if (ld_g < L.W) return fail(MPX_ERR_ARG, "%s: ld_g below the row width", who);
    if (ld_gx < L.SD) return fail(MPX_ERR_ARG, "%s: ld_gx below the width of the static matrix", who);
    if (total_frames == 0 || n_utts == 0) return MPX_OK;
    if (!g || !utt_frame_off || !gx) return fail(MPX_ERR_ARG, "%s: null pointer", who);
    if (interp_stream >= 0 && !nb) return fail(MPX_ERR_ARG, "%s: null pointer (nb, needed with a carried stream)", who);
    const long long n = (long long)total_frames * L.SD;
    hipLaunchKernelGGL(k_cmp_compose_bwd, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g,
                       (long long)ld_g, (const int*)nb, (const int*)utt_frame_off, n_utts, (long long)total_frames, L,
                       std_dev, gx, (long long)ld_gx);
    MPX_HIP_CHECK(hipGetLastError());
    return MPX_OK;
}

int64_t mpx_cmp_moments_work_doubles(int64_t total_frames, int64_t width) {
    if (total_frames < 0 || width < 1) return 0;
    return (total_frames + kMomTile - 1) / kMomTile * width;   // one partial sum per tile of kMomTile rows and column
}

int mpx_cmp_column_moments(void* stream, const void* x, int32_t x_f64, int64_t ld_x, int64_t total_frames, int64_t width,
                           double* out, double* work) {
    static const char* who = "mpx_cmp_column_moments";
    if (width < 1) return fail(MPX_ERR_ARG, "%s: width must be >= 1", who);
    if (total_frames < 0) return fail(MPX_ERR_ARG, "%s: negative total_frames", who);
    if (total_frames > 0x7fffffffLL) return fail(MPX_ERR_ARG, "%s: total_frames above 2^31 - 1", who);
    if (ld_x < width) return fail(MPX_ERR_ARG, "%s: ld_x below the row width", who);
    if ((total_frames + kMomTile - 1) / kMomTile > 0x7fffffffLL * 256 / width)
        return fail(MPX_ERR_ARG, "%s: too many elements for one launch", who);
    if (total_frames == 0) return MPX_OK;
    if (!x || !out || !work) return fail(MPX_ERR_ARG, "%s: null pointer", who);
    if (x_f64) moments_launch<double>((hipStream_t)stream, x, ld_x, total_frames, width, out, work);
    else moments_launch<float>((hipStream_t)stream, x, ld_x, total_frames, width, out, work);
    MPX_HIP_CHECK(hipGetLastError());
    return MPX_OK;
}

}  // extern "C"
