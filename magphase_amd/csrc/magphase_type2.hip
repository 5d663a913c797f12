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
//   k_noise_power  the noise statistic of the type-2 synthesis (synthesis_from_compressed_type2, magphase.py:1530-1541):
//                  one wavefront per synthesis frame; sum_{k=0}^{N/2} |Ns[k]|^2 of the windowed noise frame WITHOUT a
//                  transform, from three float64 sums over the frame's samples (Parseval + the DC and Nyquist bins).
//   k_noise_rms    one workgroup per utterance: rms = sqrt(sum / (frames * (N/2 + 1))), inv_gain[f] = 1 / rms.
//                  DESIGN.md section 3.3f.
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

// np.hanning(1 + 2 half) (wtype 0) or np.bartlett(1 + 2 half)**2.5 (wtype 1: voi_noise_window, magphase.py:67-68) at
// offset d from the centre, float64; the centre sample is 1 for both, also for a zero-length half.
__device__ __forceinline__ double noise_window(int d, int L, int R, int wtype) {
    if (d == 0) return 1.0;
    if (wtype == 0) return gain_window(d, L, R);
    const double t = d < 0 ? (double)(L + d) / (double)L : (double)(R - d) / (double)R;
    return t * t * sqrt(t);
}

// For a real frame x of length N (zero padding, truncation and the fftshift of magphase.py:1532-1534 only move samples
// inside the frame or change the bins' phase):
//   sum_{k=0}^{N/2} |X_k|^2 = (N sum x^2 + (sum x)^2 + (sum (-1)^n x[n])^2) / 2
// (Parseval over all N bins, plus the two bins the half spectrum does not count twice: X_0 = sum x, X_{N/2} = sum (-1)^n x).
// The alternating sum's overall sign depends on where the frame sits in the FFT input; it enters squared.
__global__ __launch_bounds__(kGainWaves * 64) void k_noise_power(const float* __restrict__ noise,
                                                                  const long long* __restrict__ pos,
                                                                  const int* __restrict__ left,
                                                                  const int* __restrict__ right,
                                                                  const int* __restrict__ wtype, long long n_frames,
                                                                  int N, double* __restrict__ power) {
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * kGainWaves;
    for (long long f = (long long)blockIdx.x * kGainWaves + (threadIdx.x >> 6); f < n_frames; f += stride) {
        const int L = left[f], R = right[f], wt = wtype[f];
        const float* base = noise + (pos[f] - L);   // sample k of the frame: base[k], 0 <= k <= L + R
        const int len = min(L + R + 1, N);          // a frame longer than the FFT input is truncated
        double s2 = 0.0, s1 = 0.0, sa = 0.0;
        for (int k = lane; k < len; k += 64) {      // k and lane have the same parity: the sign is the lane's
            const double x = (double)base[k] * noise_window(k - L, L, R, wt);
            s2 = fma(x, x, s2);
            s1 += x;
            sa += x;
        }
        sa = (lane & 1) ? -sa : sa;
        s2 = wave_sum(s2);
        s1 = wave_sum(s1);
        sa = wave_sum(sa);
        if (lane == 0) power[f] = 0.5 * ((double)N * s2 + s1 * s1 + sa * sa);
    }
}

// One workgroup per utterance; the frames are added in a fixed order (thread t takes frames t, t + 256, ..., then a
// fixed tree), so an utterance's rms does not depend on the batch it is in.  An utterance without frames gets NaN.
__global__ __launch_bounds__(256) void k_noise_rms(const double* __restrict__ power, const int* __restrict__ utt_frame_off,
                                                   int bins_per_frame, float* __restrict__ inv_gain,
                                                   double* __restrict__ rms) {
    __shared__ double s_sum[256];
    const int u = blockIdx.x;
    const int f0 = utt_frame_off[u], f1 = utt_frame_off[u + 1];
    double acc = 0.0;
    for (int f = f0 + threadIdx.x; f < f1; f += 256) acc += power[f];
    s_sum[threadIdx.x] = acc;
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
        if (threadIdx.x < off) s_sum[threadIdx.x] += s_sum[threadIdx.x + off];
        __syncthreads();
    }
    const double r = (f1 > f0) ? sqrt(s_sum[0] / ((double)(f1 - f0) * (double)bins_per_frame)) : nan("");
    if (threadIdx.x == 0 && rms) rms[u] = r;
    const float ig = (float)(1.0 / r);
    for (int f = f0 + threadIdx.x; f < f1; f += 256) inv_gain[f] = ig;
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

int mpx_noise_power(void* stream, int fft_len, const float* noise, const int64_t* frame_pos, const int32_t* frame_left,
                    const int32_t* frame_right, const int32_t* frame_wtype, int64_t n_frames, double* power) {
    if (!p_of(fft_len)) return fail(MPX_ERR_ARG, "mpx_noise_power: fft_len must be 1024, 2048 or 4096%s");
    if (n_frames < 0) return fail(MPX_ERR_ARG, "mpx_noise_power: negative n_frames%s");
    if (n_frames == 0) return MPX_OK;
    if (!noise || !frame_pos || !frame_left || !frame_right || !frame_wtype || !power)
        return fail(MPX_ERR_ARG, "mpx_noise_power: null pointer%s");
    // k_frame_gain's launch shape: no LDS, the frames dealt by grid stride over at most kGainBlocksPerCu workgroups per CU
    const long long need = (n_frames + kGainWaves - 1) / kGainWaves;
    const long long cap = (long long)kGainBlocksPerCu * device_cus();
    const int grid = (int)std::max<long long>(1, std::min(need, cap));
    hipLaunchKernelGGL(k_noise_power, dim3(grid), dim3(kGainWaves * 64), 0, (hipStream_t)stream, noise,
                       (const long long*)frame_pos, (const int*)frame_left, (const int*)frame_right,
                       (const int*)frame_wtype, (long long)n_frames, (int)fft_len, power);
    MPX_HIP_CHECK(hipGetLastError());
    return MPX_OK;
}

int mpx_noise_rms(void* stream, int fft_len, const double* power, const int32_t* utt_frame_off, int32_t n_utts,
                  float* inv_gain, double* rms) {
    if (!p_of(fft_len)) return fail(MPX_ERR_ARG, "mpx_noise_rms: fft_len must be 1024, 2048 or 4096%s");
    if (n_utts < 0) return fail(MPX_ERR_ARG, "mpx_noise_rms: negative n_utts%s");
    if (n_utts == 0) return MPX_OK;
    if (!power || !utt_frame_off || !inv_gain) return fail(MPX_ERR_ARG, "mpx_noise_rms: null pointer%s");
    hipLaunchKernelGGL(k_noise_rms, dim3((unsigned)n_utts), dim3(256), 0, (hipStream_t)stream, power,
                       (const int*)utt_frame_off, (int)(fft_len / 2 + 1), inv_gain, rms);
    MPX_HIP_CHECK(hipGetLastError());
    return MPX_OK;
}

}  // extern "C"
