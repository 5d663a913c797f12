// magphase_gl.hip -- k_gl_fold: the first synthesis of Griffin-Lim reads (mag', phasor real, phasor imag) rows; this is
// hostmath.griffin_lim_fold on the device (C ABI: mpx_griffin_lim_fold), so that neither the initial phase nor the fold
// passes through the host.  The initial phase comes as
//   HALF   float32 [F x H] rows of a Hermitian extension (columns 0 and H - 1 count as 0),
//   FULL   float32 [F x N] rows: c_k = (e^{j phi_k} + e^{-j phi_{N-k}}) / 2,
//   WORDS  numpy's raw MT19937 words, two per sample of rand(F, N): phi = 2 pi (r - 0.5), then the FULL fold -- the
//          [F x N] phase matrix never exists in memory.
//
// Indexing: one thread per output element (frame, bin), elements numbered row-major over [n_frames x H]: a wave stores 64
// consecutive floats of a row (rows are 513 .. 2049 elements; a row's end falls inside at most one wave per row).  Every
// output element is written exactly once, by the thread that owns it.  All arithmetic is float64 (sincos, the fold, the
// modulus), rounded once to float32.  No LDS, no atomics.
#include "mpx_common.hpp"

namespace mpx {

constexpr int kGlFoldThreads = 256;

struct GlFoldArgs {
    const float* mag;      // [.. x H] at pitch ld, row frame0 + r
    const void* phase;     // row r of the range: float [H] (HALF) / float [N] (FULL) at pitch ld_phase, uint32 [2 N] (WORDS)
    float *out_mag, *out_real, *out_imag, *out_phase;   // row frame0 + r at pitch ld; out_phase may be null
    long long ld, ld_phase, frame0, n_frames;
    int H, form;
};

// phi_i of row `row` (i < N) as float64: the float32 element widened, or numpy's random_sample() of the two words
// (genrand_res53: (a >> 5, b >> 6) -> (a 2^26 + b) / 2^53; all of it exact in float64 up to the product with 2 pi)
template <int FORM>
__device__ __forceinline__ double gl_phase_at(const void* base, long long row_off, int i) {
    if (FORM == MPX_GL_FOLD_WORDS) {
        const uint2 w = reinterpret_cast<const uint2*>(static_cast<const unsigned*>(base) + row_off)[i];
        const double r = ((double)(w.x >> 5) * 67108864.0 + (double)(w.y >> 6)) / 9007199254740992.0;
        return 2.0 * 3.141592653589793 * (r - 0.5);
    }
    return (double)(static_cast<const float*>(base) + row_off)[i];
}

template <int FORM>
__global__ __launch_bounds__(kGlFoldThreads) void k_gl_fold(const GlFoldArgs a) {
    const int H = a.H, N = 2 * (H - 1);
    const long long i = (long long)blockIdx.x * kGlFoldThreads + threadIdx.x;
    if (i >= a.n_frames * H) return;
    const long long r = i / H;
    const int k = (int)(i - r * H);
    const long long o = (a.frame0 + r) * a.ld + k;
    const double m = (double)a.mag[o];
    const double sgn = (k & 1) ? -1.0 : 1.0;
    double om, ore, oim, ph;
    if (FORM == MPX_GL_FOLD_HALF) {
        ph = (k == 0 || k == H - 1) ? 0.0 : (double)(static_cast<const float*>(a.phase) + r * a.ld_phase)[k];
        double s, c;
        sincos(ph, &s, &c);
        om = m;
        ore = c * sgn;
        oim = s * sgn;
    } else {
        const long long row_off = (FORM == MPX_GL_FOLD_WORDS) ? r * 2 * N : r * a.ld_phase;
        ph = gl_phase_at<FORM>(a.phase, row_off, k);
        const int km = (k == 0) ? 0 : N - k;   // (N - k) mod N; at k = 0 and k = N/2 the mirror is the bin itself: c = cos phi
        const double pm = gl_phase_at<FORM>(a.phase, row_off, km);
        double s0, c0, s1, c1;
        sincos(ph, &s0, &c0);
        sincos(pm, &s1, &c1);
        const double cr = 0.5 * (c0 + c1), ci = 0.5 * (s0 - s1);
        const double mod = hypot(cr, ci);
        const double inv = mod > 0.0 ? 1.0 / mod : 0.0;
        om = m * mod;
        ore = cr * inv * sgn;
        oim = ci * inv * sgn;
    }
    a.out_mag[o] = (float)om;
    a.out_real[o] = (float)ore;
    a.out_imag[o] = (float)oim;
    if (a.out_phase) a.out_phase[o] = (float)ph;
}

}  // namespace mpx

using namespace mpx;

extern "C" int mpx_griffin_lim_fold(void* stream, int fft_len, int32_t form, const float* mag, const void* phase,
                                    int64_t ld_phase, int64_t frame0, int64_t n_frames, float* out_mag, float* out_real,
                                    float* out_imag, float* out_phase, int64_t ld) {
    if (!p_of(fft_len)) return fail(MPX_ERR_ARG, "mpx_griffin_lim_fold: fft_len must be 1024, 2048 or 4096 (no tables for another)%s");
    if (form != MPX_GL_FOLD_HALF && form != MPX_GL_FOLD_FULL && form != MPX_GL_FOLD_WORDS)
        return fail(MPX_ERR_ARG, "mpx_griffin_lim_fold: unknown form of the phase (MPX_GL_FOLD_HALF, _FULL or _WORDS)%s");
    const int H = fft_len / 2 + 1;
    if (frame0 < 0 || n_frames < 0 || ld < 0 || ld_phase < 0)
        return fail(MPX_ERR_ARG, "mpx_griffin_lim_fold: negative size%s");
    if (ld < H) return fail(MPX_ERR_ARG, "mpx_griffin_lim_fold: row pitch ld smaller than H = fft_len / 2 + 1%s");
    if (form != MPX_GL_FOLD_WORDS && ld_phase < (form == MPX_GL_FOLD_HALF ? H : fft_len))
        return fail(MPX_ERR_ARG, "mpx_griffin_lim_fold: ld_phase smaller than the phase rows (H for HALF, fft_len for FULL)%s");
    if (n_frames == 0) return MPX_OK;
    if (!mag || !phase || !out_mag || !out_real || !out_imag)
        return fail(MPX_ERR_ARG, "mpx_griffin_lim_fold: null pointer with rows to fold%s");
    if (form == MPX_GL_FOLD_WORDS && (reinterpret_cast<uintptr_t>(phase) & 7))
        return fail(MPX_ERR_ARG, "mpx_griffin_lim_fold: the words must be 8-byte aligned (a sample is a pair)%s");
    if (frame0 > ((int64_t)1 << 40) || n_frames > ((int64_t)1 << 40))
        return fail(MPX_ERR_ARG, "mpx_griffin_lim_fold: too many frames%s");
    const long long blocks = (n_frames * H + kGlFoldThreads - 1) / kGlFoldThreads;
    if (blocks > 0x7fffffffLL) return fail(MPX_ERR_ARG, "mpx_griffin_lim_fold: too many elements for one launch%s");
    GlFoldArgs a;
    a.mag = mag;
    a.phase = phase;
    a.out_mag = out_mag;
    a.out_real = out_real;
    a.out_imag = out_imag;
    a.out_phase = out_phase;
    a.ld = ld;
    a.ld_phase = ld_phase;
    a.frame0 = frame0;
    a.n_frames = n_frames;
    a.H = H;
    a.form = form;
    const dim3 grid((unsigned)blocks), block(kGlFoldThreads);
    hipStream_t s = (hipStream_t)stream;
    if (form == MPX_GL_FOLD_HALF) hipLaunchKernelGGL(k_gl_fold<MPX_GL_FOLD_HALF>, grid, block, 0, s, a);
    else if (form == MPX_GL_FOLD_FULL) hipLaunchKernelGGL(k_gl_fold<MPX_GL_FOLD_FULL>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(k_gl_fold<MPX_GL_FOLD_WORDS>, grid, block, 0, s, a);
    MPX_HIP_CHECK(hipGetLastError());
    return MPX_OK;
}
