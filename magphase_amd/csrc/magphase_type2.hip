// magphase_type2.hip -- the per-frame gain of the type-2 analysis (analysis_with_del_comp_from_pm_type2,
// magphase.py:236-242).
//
//   k_frame_gain   one wavefront per pitch-synchronous frame (grid stride): the frame's Hann-windowed samples are
//                  evaluated in float64 straight from the signal (no FFT input is materialised), then
//                    voiced   (voi == 1): max |x| over the first fft_len/2 + 1 samples of the rotated, zero-padded or
//                                          truncated FFT input (np.hstack((c[s:], c[:s])), s = left; s >= fft_len: no
//                                          rotation, as python slicing gives);
//                    unvoiced:             np.std (population) of the whole windowed frame, all left + right + 1
//                                          samples, before any padding or truncation: mean first, then the mean squared
//                                          deviation, both accumulated in float64.
//                  DESIGN.md section 3.3e.
#include "mpx_common.hpp"

namespace mpx {

constexpr int kGainWaves = 8;        // waves per workgroup of k_frame_gain
constexpr int kGainBlocksPerCu = 3;  // default workgroups per CU (6 waves per SIMD); tools/type2_probe.py measures 1 and 3

// np.hanning(1 + 2 half)[half + d] (d <= 0, rising half) / the mirrored falling half (d > 0), in float64:
// 0.5 + 0.5 cos(pi d / half); the centre sample (d == 0) is 1, also for a zero-length half.
__device__ __forceinline__ double gain_window(int d, int L, int R) {
    if (d == 0) return 1.0;
    const int half = d < 0 ? L : R;
    return 0.5 + 0.5 * cos(3.141592653589793 * (double)d / (double)half);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

__global__ __launch_bounds__(kGainWaves * 64) void k_frame_gain(const float* __restrict__ sig,
                                                                 const long long* __restrict__ pos,
                                                                 const int* __restrict__ left,
                                                                 const int* __restrict__ right,
                                                                 const float* __restrict__ voi, long long n_frames,
                                                                 int N, double* __restrict__ gain) {
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * kGainWaves;
    for (long long f = (long long)blockIdx.x * kGainWaves + (threadIdx.x >> 6); f < n_frames; f += stride) {
        const int L = left[f], R = right[f];
        const float* base = sig + (pos[f] - L);   // sample k of the frame: base[k], 0 <= k <= L + R
        double g;
        if (voi[f] == 1.0f) {
            const int len = min(L + R + 1, N);    // samples of the padded / truncated FFT input that are not zero
            const int rot = (L < N) ? L : 0;
            const int H = N / 2 + 1;
            double m = 0.0;
            for (int j = lane; j < H; j += 64) {
                int k = j + rot;
                k = (k >= N) ? k - N : k;
                if (k < len) m = fmax(m, fabs((double)base[k] * gain_window(k - L, L, R)));
            }
            g = wave_max(m);
        } else {
            const int n = L + R + 1;
            double s = 0.0;
            for (int k = lane; k < n; k += 64) s += (double)base[k] * gain_window(k - L, L, R);
            const double mean = wave_sum(s) / (double)n;
            double q = 0.0;
            for (int k = lane; k < n; k += 64) {
                const double d = (double)base[k] * gain_window(k - L, L, R) - mean;
                q += d * d;
            }
            g = sqrt(wave_sum(q) / (double)n);
        }
        if (lane == 0) gain[f] = g;
    }
}

}  // namespace mpx

using namespace mpx;

extern "C" {

int mpx_frame_gain(void* stream, int fft_len, const float* sig, const int64_t* frame_pos, const int32_t* frame_left,
                   const int32_t* frame_right, const float* voi, int64_t n_frames, double* gain, int32_t blocks_per_cu) {
    if (!p_of(fft_len)) return fail(MPX_ERR_ARG, "mpx_frame_gain: fft_len must be 1024, 2048 or 4096%s");
    if (n_frames < 0) return fail(MPX_ERR_ARG, "mpx_frame_gain: negative n_frames%s");
    if (blocks_per_cu > 8) return fail(MPX_ERR_ARG, "mpx_frame_gain: blocks_per_cu must be <= 8%s");
    if (n_frames == 0) return MPX_OK;
    if (!sig || !frame_pos || !frame_left || !frame_right || !voi || !gain)
        return fail(MPX_ERR_ARG, "mpx_frame_gain: null pointer%s");
    // no LDS, 78 VGPRs (6 waves per SIMD): three 8-wave workgroups per CU fit; the frames are dealt by grid stride
    const long long need = (n_frames + kGainWaves - 1) / kGainWaves;
    const long long cap = (long long)(blocks_per_cu > 0 ? blocks_per_cu : kGainBlocksPerCu) * device_cus();
    const int grid = (int)std::max<long long>(1, std::min(need, cap));
    hipLaunchKernelGGL(k_frame_gain, dim3(grid), dim3(kGainWaves * 64), 0,
                       (hipStream_t)stream, sig, (const long long*)frame_pos, (const int*)frame_left,
                       (const int*)frame_right, voi, (long long)n_frames, (int)fft_len, gain);
    MPX_HIP_CHECK(hipGetLastError());
    return MPX_OK;
}

}  // extern "C"
