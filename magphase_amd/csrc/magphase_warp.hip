// magphase_warp.hip -- the mel warp / unwarp GEMMs of the compressed features on the f32 matrix instructions.
//
//   k_mel_warp_mfma, k_warp_phase_rows     mel warp of the compressed analysis as a GEMM on the f32 matrix instructions
//   k_mel_unwarp_bwd                       backward of the mel unwarp (compressed synthesis): [rows x K] x [K x n_out]
//   k_mel_unwarp_mfma / _tiled             [F x K] x [K x H] -> exp / identity: la.sp_mel_unwarp and
//                                          phase_uncompress_type1_mcep as the linear maps they are, K <= 64
#include "mpx_common.hpp"

namespace mpx {

// ---------------------------------------------------------------------------------------------
// mel unwarp GEMM
// ---------------------------------------------------------------------------------------------
struct UnwarpJob {
    const float* A;  // [F x K] mel-domain features
    const float* U;  // [K x H] unwarp matrix
    float* out;      // [F x H]
    int K;
    int op;          // 0: identity, 1: exp
};
struct UnwarpJobs {
    UnwarpJob j[3];
};

constexpr int kGemmFrames = 64;   // frames per block
constexpr int kGemmKMax = 64;

// ---------------------------------------------------------------------------------------------
// mel warp GEMM (compressed analysis): out[f][i] = post( sum_k W[i][k] * pre(x[f][k]) ), i < nout <= 64, k < H
// ---------------------------------------------------------------------------------------------
// la.sp_mel_warp (libaudio.py:643-661) = SPTK ``mcep -j 0`` (log-periodogram -> real IFFT -> halve c0, c_{N/2} ->
// freqt) followed by the alpha = 0 cosine matrix: a LINEAR map of the log-periodogram, precomputed on the host as W
// (hostmath.warp_matrix).  pre: mode 0 (|f(w)|, mcep -q 3): ln(x^2 + 1e-8); mode 1 (ln|f(w)|, -q 2): ln(exp(x)^2 + 1e-8).
// Rows may be interpolated on the fly (variable -> constant frame rate, magphase.py:2219-2239) BEFORE pre().
// post: mode 0: none (the reference's exp followed by la.log); mode 1: * voiced, clip to [-1, 1] (magphase.py:2527-2532).
struct WarpJob {
    const float* x;      // [rows x H]
    const float* W;      // [nout x H]
    float* out;          // [F x nout]
    const float* voi;    // [F] or null
    int nout;
    int mode;
    long long F;         // frames (rows of out) of THIS job: the phase jobs may run on other rows than the magnitudes
};
struct WarpJobs {
    WarpJob j[3];
};

// Prologue of the mel warp's operand (WarpJob::mode) and the matching epilogue:
//   0  magnitudes, cepstral warp: ln(x^2 + 1e-8)                                   (mcep -q 3 -e 1e-8 on x, libaudio.py:575-661)
//   1  phase streams (mcep -q 2 on exp(x), |x| <= 1): ln(e^{2x} + 1e-8) = 2x + 1e-8 e^{-2x} (the next term is 5e-17);
//      epilogue voicing mask + clip
//   3  phase streams on the VARIABLE-rate rows (mpx_mel_warp_rows): prologue of mode 1, no epilogue -- the 45 outputs
//      are interpolated to the constant rate, masked and clipped by k_warp_phase_rows; ``voi`` = the rows in use
//   2  magnitudes, filter bank: la.log(x) = ln x with -1e10 for x == 0 (libaudio.py:241-248, :763-769); the reference then
//      takes exp and la.log again (magphase.py:2505-2510): the identity unless the exp underflows to 0 (sum < ln of the
//      smallest float64, -745.13), which comes back as -1e10
__device__ __forceinline__ float warp_prologue(int mode, float x) {
    // the argument is >= 1e-8 (never a denormal): the hardware log2 as it is, without __logf's denormal rescaling
    if (mode == 0) return __builtin_amdgcn_logf(fmaf(x, x, 1.0e-8f)) * 0.69314718055994531f;
    if (mode == 1 || mode == 3) return fmaf(1.0e-8f, __expf(-2.0f * x), 2.0f * x);
    return (x > 0.0f) ? __logf(x) : -1.0e10f;
}
__device__ __forceinline__ float warp_epilogue(int mode, float y, float vo) {
    if (mode == 1) return (vo == 0.0f) ? 0.0f : fminf(fmaxf(y * vo, -1.0f), 1.0f);   // +0 for unvoiced frames, always
    if (mode == 2) return (y < -745.13321f) ? -1.0e10f : y;
    return y;
}

constexpr int kWarpTile = 64;
#ifndef MPX_WARP_STRIDE
#define MPX_WARP_STRIDE 68
#endif
constexpr int kWarpStride = MPX_WARP_STRIDE;   // floats per LDS row (multiple of 4 for float4 reads)
#ifndef MPX_WARP_KC
#define MPX_WARP_KC 64
#endif
constexpr int kWarpKC = MPX_WARP_KC;                 // bins per staged chunk of the MFMA warp (64 or 128)
// LDS rows of the MFMA warp.  Round 2 padded them to 68 floats and measured SQ_LDS_BANK_CONFLICT = 31 % of the kernel's
// LDS cycles: a ds_read_b128 is served in groups of 16 lanes ({0-3, 12-15, 20-27}, ...; MI355X_MICROARCH.md, LDS), a
// group holds every fragment row li = lane & 15 once but from TWO k groups g = lane >> 4, and with the k offset 16 g
// added to the row's padding offset 4 li two rows of a group always met in a bank.  Now: dense rows (64 floats: every
// row starts in bank 0) and the 16-byte chunk c of row r stored at chunk c ^ swz(r & 15), swz even for r in 4..11 and
// odd otherwise -- within a lane group the g = 0 lanes then read the odd (even) chunks ^ q and the g = 1 lanes the even
// (odd) ones: 16 distinct chunks, conflict-free; the staging writes (8 lanes = 8 consecutive chunks of one row) stay so.
#ifndef MPX_WARP_SWIZZLE
#define MPX_WARP_SWIZZLE (MPX_WARP_KC == 64)
#endif
constexpr bool kWarpSwizzle = MPX_WARP_SWIZZLE;
constexpr int kWarpKStride = kWarpSwizzle ? kWarpKC : kWarpKC + (kWarpStride - 64);
static_assert(!kWarpSwizzle || kWarpKC == 64, "the chunk swizzle is defined for 64-bin chunks (16 chunks of 16 bytes per row)");
__device__ __forceinline__ int warp_swz(int r15) {
    if (!kWarpSwizzle) return 0;
    const bool mid = (r15 >= 4) && (r15 < 12);
    return mid ? 2 * (r15 - 4) : 2 * ((r15 < 4) ? r15 : r15 - 8) + 1;
}

// ---------------------------------------------------------------------------------------------
// Mel warp on the matrix cores: out[F x nout] = ln-prologue(x)[F x H] . W^T[H x nout], v_mfma_f32_16x16x4_f32.
// One workgroup = 64 output frames x up to 64 outputs; the reduction runs over the H bins in chunks of 64.  Per chunk
// the 256 threads stage the prologue values and the W slab into LDS as [row][k] (k contiguous, row stride 68 floats:
// conflict-free dword writes with k across lanes, 16-byte fragment reads); wave w then owns the frames
// 16 w .. 16 w + 15 and every 16-wide column tile.  The MFMA sums over k in any order, so lane group g = lane >> 4
// takes k = 16 g + 4 q + {0..3} for the four instructions of step q: a lane's fragment is one ds_read_b128 per step.
// Instructions of the column tiles are interleaved (dependent-accumulator latency 40 cycles > issue 32).
// ---------------------------------------------------------------------------------------------
typedef float f32x4 __attribute__((ext_vector_type(4)));

// NT: 16-wide column tiles in use, ceil(nout / 16); INTERP: rows interpolated (row0 given); MODE: the job's prologue /
// epilogue at compile time (as a run-time value it was a scalar branch per staged element: a third of the kernel's
// instructions were SALU, and the kernel is bound by instruction issue)
template <int NT, bool INTERP, int MODE>
__device__ __forceinline__ void mel_warp_block(const WarpJob& job, float (*As)[kWarpKStride], float (*Ws)[kWarpKStride],
                                               long long* s_o0, long long* s_o1, float* s_rt, long long F, int H,
                                               const int* __restrict__ row0, const int* __restrict__ row1,
                                               const float* __restrict__ rowt, long long ld) {
    const long long f0 = (long long)blockIdx.x * kWarpTile;   // row tiles on x: no 65535 limit on the frame count
    if (f0 >= F) return;                                      // the jobs of a launch need not have the same frame count
    const int kk = threadIdx.x & 63, fq = threadIdx.x >> 6;   // staging roles: bin within the chunk, frame quarter
    const int wave = rfl((int)(threadIdx.x >> 6));
    const int li = kk & 15, g = kk >> 4;                      // fragment roles
    if ((MODE == 1 || MODE == 3) && job.voi) {   // phase streams are masked by the voicing (magphase.py:2527-2529): a tile without a
        // voiced frame is all zeros -- written as such, nothing read
        const int pred = (threadIdx.x < kWarpTile) && (job.voi[min(f0 + (long long)threadIdx.x, F - 1)] != 0.0f);
        if (!__syncthreads_or(pred)) {
            const long long n_el = min((long long)kWarpTile, F - f0) * job.nout;
            for (long long i = threadIdx.x; i < n_el; i += 256) job.out[f0 * job.nout + i] = 0.0f;
            return;
        }
    }
    if (threadIdx.x < kWarpTile) {
        const long long f = min(f0 + (long long)threadIdx.x, F - 1);
        s_o0[threadIdx.x] = (long long)(row0 ? row0[f] : (int)f) * ld;
        s_o1[threadIdx.x] = (long long)(row0 ? row1[f] : (int)f) * ld;
        s_rt[threadIdx.x] = row0 ? rowt[f] : 0.0f;
    }
    __syncthreads();
    // Two-level accumulation over the H bins.  The operands are log spectra (|v| ~ 10): one fp32 chain over 2049 terms
    // carries partial sums of that size and loses ~sqrt(2049) * 6e-7 = 3e-5 -- measured 4e-5 against a float64 product of
    // the same device features, the whole residual error of the compressed analysis once its FFT is float64.  So every
    // 64-bin chunk is summed in a fresh MFMA accumulator (small partial sums) and the 33 chunk sums are added up
    // separately: ~sqrt(33) * 6e-7.  (An error-free TwoSum of the totals costs 16 more registers: the kernel, capped at
    // 128 VGPRs for four workgroups per CU, spills.)
    f32x4 tot[NT];
#pragma unroll
    for (int jt = 0; jt < NT; ++jt) tot[jt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    // Staging roles: thread (c4, rr) handles the 4 consecutive bins k0 + 4 c4 .. + 3 of the rows rr + 16 p, p < 4: one
    // 16-byte load per row and operand (12 per thread and chunk instead of 48 dword loads: the kernel issued 19 M VMEM
    // instructions per launch) and one ds_write_b128 per row (16 lanes cover a row's 256 bytes: conflict-free).  Rows
    // are dense (pitch H floats): the loads are 4-byte aligned only, which global_load_dwordx4 allows.  Every load is
    // unconditional; the chunk that crosses the end of the row (H = 64 q + 1: the last bin alone) clamps per element.
    // The NEXT chunk's loads are issued right after this chunk's values are in LDS, so they fly behind the fragment
    // reads and the MFMAs.
    constexpr int LPR = kWarpKC / 4, RPT = 256 / LPR, NP = kWarpTile / RPT;   // lanes per row, rows per pass, passes
    constexpr int NPW = (16 * NT + RPT - 1) / RPT;                            // passes that touch a W row in use
    const int c4 = threadIdx.x % LPR, rr = threadIdx.x / LPR;
    static_assert(!kWarpSwizzle || RPT == 16, "swizzle: a staging thread's rows rr + 16 p share rr & 15");
    const int swz_w = warp_swz(rr & 15), swz_r = warp_swz(li);
    typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));   // 16-byte load from a 4-byte aligned address
    auto ld4 = [](const float* q) {
        const f32x4u v = *reinterpret_cast<const f32x4u*>(q);
        return make_float4(v[0], v[1], v[2], v[3]);
    };
    float4 xv[NP], xw[NP], wv4[NP];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int fl = rr + RPT * p;
            const int k = k0 + 4 * c4;
#ifdef MPX_PROBE_WARP_NOLOAD   // ablation (tools/ab_bench.py): operands faked, no global loads in the chunk loop
            xv[p] = xw[p] = make_float4(1.0f + 0.001f * (float)(k + fl), 1.1f, 1.2f, 1.3f);
            wv4[p] = make_float4(0.001f * (float)fl, 0.002f, 0.003f, 0.004f);
            asm volatile("" : "+v"(xv[p].x), "+v"(xw[p].y), "+v"(wv4[p].z));
#else
            xv[p] = ld4(job.x + s_o0[fl] + k);
            if (INTERP) xw[p] = ld4(job.x + s_o1[fl] + k);
            if (p < NPW) wv4[p] = ld4(job.W + (long long)min(fl, job.nout - 1) * H + k);
#endif
        }
    };
    const int Hfull = H & ~(kWarpKC - 1);   // bins covered by whole chunks; the rest (one bin for H = 64 q + 1) below
    if (Hfull > 0) fetch(0);
    for (int k0 = 0; k0 < Hfull; k0 += kWarpKC) {
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int fl = rr + RPT * p;
            // No masking of the padding: frames past F repeat the last frame's rows (s_o0 / s_o1 are clamped) and W rows
            // past nout repeat the last row -- rows and columns of the product are independent, and the epilogue stores
            // neither (a select per staged element was 32 of the 180 instructions of this block).
            const float rt = INTERP ? s_rt[fl] : 0.0f;
            const float xin[4] = {xv[p].x, xv[p].y, xv[p].z, xv[p].w};
            const float xin1[4] = {xw[p].x, xw[p].y, xw[p].z, xw[p].w};
            float av[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float x = INTERP ? fmaf(xin1[e] - xin[e], rt, xin[e]) : xin[e];
                av[e] = warp_prologue(MODE, x);
            }
            const int cw = kWarpSwizzle ? 4 * (c4 ^ swz_w) : 4 * c4;   // (fl & 15 == rr & 15: RPT is 16 for 64-bin chunks)
            *reinterpret_cast<float4*>(&As[fl][cw]) = make_float4(av[0], av[1], av[2], av[3]);
            if (p < NPW) *reinterpret_cast<float4*>(&Ws[fl][cw]) = wv4[p];
        }
        __syncthreads();
        if (k0 + kWarpKC < Hfull) fetch(k0 + kWarpKC);
#ifdef MPX_PROBE_WARP_NOMFMA   // ablation: staging, barriers and fragment reads only
#define MPX_WARP_MFMA(a_, b_, c_) ((c_) + f32x4{(a_) * (b_), 0.0f, 0.0f, 0.0f})
#else
#define MPX_WARP_MFMA(a_, b_, c_) __builtin_amdgcn_mfma_f32_16x16x4f32((a_), (b_), (c_), 0, 0, 0)
#endif
#pragma unroll
        for (int h = 0; h < kWarpKC / 64; ++h) {   // a fresh accumulator per 64 bins (two-level accumulation, above)
            const float* arow = &As[16 * wave + li][kWarpSwizzle ? 0 : 64 * h + 16 * g];
            f32x4 acc[NT];
#pragma unroll
            for (int jt = 0; jt < NT; ++jt) acc[jt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int q = 0; q < 4; ++q) {   // 4 k per lane group and step: one 16-byte read per fragment
                // column of the fragment: k = 16 g + 4 q .. + 3, i.e. chunk 4 g + q (swizzled: ^ swz(li), one v_xor per step)
                const int col = kWarpSwizzle ? 4 * (((4 * g) ^ swz_r) ^ q) : 64 * h + 16 * g + 4 * q;
                const float4 aq = *reinterpret_cast<const float4*>(arow + (kWarpSwizzle ? col : 4 * q));
                float4 bq[NT];
#pragma unroll
                for (int jt = 0; jt < NT; ++jt)
                    bq[jt] = *reinterpret_cast<const float4*>(&Ws[16 * jt + li][col]);
#pragma unroll
                for (int jt = 0; jt < NT; ++jt) acc[jt] = MPX_WARP_MFMA(aq.x, bq[jt].x, acc[jt]);
#pragma unroll
                for (int jt = 0; jt < NT; ++jt) acc[jt] = MPX_WARP_MFMA(aq.y, bq[jt].y, acc[jt]);
#pragma unroll
                for (int jt = 0; jt < NT; ++jt) acc[jt] = MPX_WARP_MFMA(aq.z, bq[jt].z, acc[jt]);
#pragma unroll
                for (int jt = 0; jt < NT; ++jt) acc[jt] = MPX_WARP_MFMA(aq.w, bq[jt].w, acc[jt]);
            }
#pragma unroll
            for (int jt = 0; jt < NT; ++jt) tot[jt] += acc[jt];
        }
        __syncthreads();
    }
    // C: column li of tile jt, row 4 g + r of this wave's 16 frames.  The bins past the last whole chunk are added here,
    // one fmaf per bin and output (H = 64 q + 1 for every transform size: the Nyquist bin).
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long long f = f0 + 16 * wave + 4 * g + r;
        if (f >= F) continue;
        const int fl = 16 * wave + 4 * g + r;
        for (int k = Hfull; k < H; ++k) {
            const float x0 = job.x[s_o0[fl] + k];
            const float x = INTERP ? fmaf(job.x[s_o1[fl] + k] - x0, s_rt[fl], x0) : x0;
            const float v = warp_prologue(MODE, x);
#pragma unroll
            for (int jt = 0; jt < NT; ++jt) {
                const int i = 16 * jt + li;
                tot[jt][r] = fmaf(v, job.W[(long long)min(i, job.nout - 1) * H + k], tot[jt][r]);
            }
        }
        const float vo = (MODE == 1 && job.voi) ? job.voi[f] : 1.0f;
#pragma unroll
        for (int jt = 0; jt < NT; ++jt) {
            const int i = 16 * jt + li;
            if (i >= job.nout) continue;
            float y = tot[jt][r];
            y = warp_epilogue(MODE, y, vo);
            job.out[f * job.nout + i] = y;
        }
    }
}

// One launch for the three jobs (separate launches end in a half-empty last round of workgroups); the magnitude job
// (blockIdx.y == 0) and the two phase jobs get their own column-tile count (60 outputs -> 4 tiles, 45 -> 3: a quarter
// fewer MFMAs on two thirds of the workgroups).
// PHV: the phase jobs run on the variable-rate rows themselves (mode 3, no row interpolation, their own frame count);
// k_warp_phase_rows then interpolates their outputs to the constant rate.
template <int NTM, int NTP, bool INTERP, int MAGMODE, bool PHV>
#if MPX_WARP_KC == 64
__attribute__((amdgpu_waves_per_eu(4, 4)))   // <= 128 VGPRs: four workgroups (35 KB of LDS each) per CU, measured -5 %
#else
__attribute__((amdgpu_waves_per_eu(2, 2)))   // 128-bin chunks: 68 KB of LDS, two workgroups per CU
#endif
__global__ __launch_bounds__(256) void k_mel_warp_mfma(WarpJobs jobs, int H, const int* __restrict__ row0,
                                                       const int* __restrict__ row1, const float* __restrict__ rowt,
                                                       long long ld) {
    __shared__ __attribute__((aligned(16))) float As[kWarpTile][kWarpKStride];   // As[f][k]
    __shared__ __attribute__((aligned(16))) float Ws[kWarpTile][kWarpKStride];   // Ws[i][k]
    __shared__ long long s_o0[kWarpTile], s_o1[kWarpTile];   // element offsets of the two input rows of a frame
    __shared__ float s_rt[kWarpTile];
    if (blockIdx.y == 0)
        mel_warp_block<NTM, INTERP, MAGMODE>(jobs.j[0], As, Ws, s_o0, s_o1, s_rt, jobs.j[0].F, H, row0, row1, rowt, ld);
    else if (PHV)
        mel_warp_block<NTP, false, 3>(jobs.j[blockIdx.y], As, Ws, s_o0, s_o1, s_rt, jobs.j[blockIdx.y].F, H, nullptr, nullptr,
                                      nullptr, ld);
    else
        mel_warp_block<NTP, INTERP, 1>(jobs.j[blockIdx.y], As, Ws, s_o0, s_o1, s_rt, jobs.j[blockIdx.y].F, H, row0, row1, rowt,
                                       ld);
}

// Phase streams of the compressed analysis at the constant rate from their variable-rate warp (mode 3): row
// interpolation of the phase_dim outputs, then the epilogue of mode 1 (voicing mask, clip; magphase.py:2527-2532).
// The warp is linear up to its 1e-8 e^{-2x} floor term, so interpolating after it instead of before differs by < 1e-8 per
// bin; rows no voiced frame uses were not computed and are not read (the select discards them).
__global__ __launch_bounds__(256) void k_warp_phase_rows(const float* __restrict__ tr, const float* __restrict__ ti,
                                                         const int* __restrict__ row0, const int* __restrict__ row1,
                                                         const float* __restrict__ rowt, const float* __restrict__ voi,
                                                         long long F, int nout, float* __restrict__ out_r,
                                                         float* __restrict__ out_i) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= F * nout) return;
    const long long f = idx / nout;
    const int i = (int)(idx - f * nout);
    const float vo = voi[f];
    float yr = 0.0f, yi = 0.0f;
    if (vo != 0.0f) {
        const long long a = (long long)row0[f] * nout + i, b = (long long)row1[f] * nout + i;
        const float t = rowt[f];
        yr = warp_epilogue(1, fmaf(tr[b] - tr[a], t, tr[a]), vo);
        yi = warp_epilogue(1, fmaf(ti[b] - ti[a], t, ti[a]), vo);
    }
    out_r[idx] = yr;
    out_i[idx] = yi;
}

// ---------------------------------------------------------------------------------------------
// Backward pass of the mel warp: grad_x[r][k] = d(x~[r][k]) * sum_{i < nout} g[r][i] W[i][k], the product
// [rows x nout <= 64] . [nout x H] on v_mfma_f32_16x16x4_f32 -- a short reduction and a wide output: the kernel is made of
// the rows x H floats it writes (and the rows x H operands it reads for d).  One workgroup = 64 rows: the g tile is staged
// in LDS once (zeros past nout and past the last row), every wave takes its A fragments of the four 16-row sub-tiles from
// there into registers and then walks the bins in 16-wide column tiles (wave w: tiles w, w + 4, ...), so the workgroup reads
// each column of W once.  Oriented C[row][bin]: register r of a lane is row 4 (lane >> 4) + r, bin lane & 15 -- a store
// instruction writes four rows' 64 contiguous bytes.  The reduction index of instruction e of step q in lane group
// g = lane >> 4 is i = 16 q + 4 g + e (any order sums the same set): a lane's A fragment of a step is one ds_read_b128.
// The last column tile (H = 64 q + 1: the Nyquist bin alone) runs like the others on clamped addresses with its stores
// masked.  d, by the job's mode:
//   0  magnitudes, x~ = the row itself or fma(x[row1] - x[row0], t, x[row0]) (the forward's arithmetic): d = 2 x~ / (x~^2 + 1e-8)
//   1  phase streams: d = 2 - 2e-8 e^{-2 x}
// g of a phase job arrives already masked (k_phase_grad_mask; at the constant rate folded onto the variable-rate rows by
// k_rows_lerp_adjoint in between).  live: optional per-row flags of a phase job -- a row whose flag is 0 has g == 0 by
// construction and is written as zeros whatever its operand row holds; a tile without a live row is written as zeros and
// reads nothing.  Plain vector stores, every output element written exactly once: deterministic.
// ---------------------------------------------------------------------------------------------
struct WarpBwdJob {
    const float* g;      // [rows x nout] upstream gradient (phase jobs: masked)
    const float* W;      // [nout x H]
    const float* x;      // operand rows of the forward, pitch ldx
    float* out;          // [rows x H], pitch ldo
    const float* live;   // [rows] or null
    const int* row0;     // row tables of the magnitude job, or null
    const int* row1;
    const float* rowt;
    long long rows;
    int nout;
    int mode;
};
struct WarpBwdJobs {
    WarpBwdJob j[3];
};

constexpr int kBwdGStride = 68;   // floats per LDS row of the g tile (16-byte aligned rows)

template <int MODE>
__device__ __forceinline__ float warp_bwd_deriv(float x) {
    if (MODE == 0) return (2.0f * x) / fmaf(x, x, 1.0e-8f);   // 0 at x == 0
    return fmaf(-2.0e-8f, __expf(-2.0f * x), 2.0f);
}

template <int MODE, bool INTERP>
__device__ __forceinline__ void mel_warp_bwd_block(const WarpBwdJob& job, float (*Gs)[kBwdGStride], long long* s_o0,
                                                   long long* s_o1, float* s_rt, float* s_live, int H, long long ldx,
                                                   long long ldo) {
    const long long rows = job.rows;
    const long long f0 = (long long)blockIdx.x * kWarpTile;
    if (f0 >= rows) return;   // the jobs of a launch need not have the same row count
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = rfl((int)(tid >> 6));
    const int li = lane & 15, g = lane >> 4;
    const int nrows = (int)min((long long)kWarpTile, rows - f0);
    const int nout = job.nout;
    if (job.live) {
        const int pred = (tid < nrows) && (job.live[f0 + min(tid, nrows - 1)] != 0.0f);
        if (!__syncthreads_or(pred)) {   // no live row: zeros, nothing read
            for (int r = wave; r < nrows; r += 4) {
                float* orow = job.out + (f0 + r) * ldo;
                for (int c = lane; c < H; c += 64) orow[c] = 0.0f;
            }
            return;
        }
    }
    if (tid < kWarpTile) {
        const long long f = f0 + min(tid, nrows - 1);   // rows past the last repeat it: read, never stored
        s_o0[tid] = (INTERP ? (long long)job.row0[f] : f) * ldx;
        s_o1[tid] = INTERP ? (long long)job.row1[f] * ldx : 0;
        s_rt[tid] = INTERP ? job.rowt[f] : 0.0f;
        s_live[tid] = (tid < nrows && (!job.live || job.live[f] != 0.0f)) ? 1.0f : 0.0f;
    }
#pragma unroll
    for (int p = 0; p < (kWarpTile * 64) / 256; ++p) {
        const int idx = tid + 256 * p;
        const int r = idx >> 6, c = idx & 63;
        Gs[r][c] = (r < nrows && c < nout) ? job.g[(f0 + r) * nout + c] : 0.0f;
    }
    __syncthreads();
    const int nq = (nout + 15) >> 4;   // 16-wide steps of the reduction in use
    const int nct = (H + 15) >> 4;
    for (int ct = wave; ct < nct; ct += 4) {
        const int bin = 16 * ct + li;
        const int binc = min(bin, H - 1);
        float b[4][4];   // the column tile's W fragments, shared by the four sub-tiles
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e)   // rows past nout meet a zero of g: any finite value of W will do
                b[q][e] = (q < nq) ? job.W[(long long)min(16 * q + 4 * g + e, nout - 1) * H + binc] : 0.0f;
#pragma unroll 1   // (unrolled, the compiler keeps every sub-tile's row offsets and addresses in registers and spills)
        for (int s = 0; s < 4; ++s) {   // rows 16 s .. 16 s + 15
            float x0[4], x1[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int fl = 16 * s + 4 * g + r;
                x0[r] = job.x[s_o0[fl] + binc];
                x1[r] = INTERP ? job.x[s_o1[fl] + binc] : 0.0f;
            }
            f32x4 acc = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (q < nq) {   // wave-uniform
                    const float4 aq = *reinterpret_cast<const float4*>(&Gs[16 * s + li][16 * q + 4 * g]);
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(aq.x, b[q][0], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(aq.y, b[q][1], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(aq.z, b[q][2], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(aq.w, b[q][3], acc, 0, 0, 0);
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int fl = 16 * s + 4 * g + r;
                const float x = INTERP ? fmaf(x1[r] - x0[r], s_rt[fl], x0[r]) : x0[r];
                const float v = (s_live[fl] != 0.0f) ? warp_bwd_deriv<MODE>(x) * acc[r] : 0.0f;
                if (fl < nrows && bin < H) job.out[(f0 + fl) * ldo + bin] = v;
            }
        }
    }
}

// <= 128 VGPRs: four workgroups (19 KB of LDS each) per CU -- the kernel waits on memory, not on its 64 MFMAs per tile
__attribute__((amdgpu_waves_per_eu(4, 4)))
__global__ __launch_bounds__(256) void k_mel_warp_bwd(WarpBwdJobs jobs, int H, long long ldx, long long ldo) {
    __shared__ __attribute__((aligned(16))) float Gs[kWarpTile][kBwdGStride];
    __shared__ long long s_o0[kWarpTile], s_o1[kWarpTile];
    __shared__ float s_rt[kWarpTile], s_live[kWarpTile];
    const WarpBwdJob& job = jobs.j[blockIdx.y];
    if (job.mode != 0)
        mel_warp_bwd_block<1, false>(job, Gs, s_o0, s_o1, s_rt, s_live, H, ldx, ldo);
    else if (job.row0)
        mel_warp_bwd_block<0, true>(job, Gs, s_o0, s_o1, s_rt, s_live, H, ldx, ldo);
    else
        mel_warp_bwd_block<0, false>(job, Gs, s_o0, s_o1, s_rt, s_live, H, ldx, ldo);
}

// The upstream gradient of the two phase streams through the forward's voicing mask and clip (warp_epilogue, mode 1):
// h = g where the frame is voiced and the forward's output lies strictly inside (-1, 1), else 0 -- a clipped output is
// exactly +-1.0f, and the gradient there is defined as zero.  A null g / h pair is skipped.
__global__ __launch_bounds__(256) void k_phase_grad_mask(long long n_el, int nout, const float* __restrict__ voi,
                                                         const float* __restrict__ out_r, const float* __restrict__ out_i,
                                                         const float* __restrict__ g_r, const float* __restrict__ g_i,
                                                         float* __restrict__ h_r, float* __restrict__ h_i) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n_el) return;
    const bool voiced = voi[idx / nout] != 0.0f;
    if (h_r) h_r[idx] = (voiced && fabsf(out_r[idx]) < 1.0f) ? g_r[idx] : 0.0f;
    if (h_i) h_i[idx] = (voiced && fabsf(out_i[idx]) < 1.0f) ? g_i[idx] : 0.0f;
}

// ---------------------------------------------------------------------------------------------
// Backward of the mel unwarp (compressed synthesis): out[rows x nout] = A[rows x K] . W^T, W the
// forward's unwarp matrix as it lies ([nout x K'], pitch ldw, K <= K'), nout <= 64, on v_mfma_f32_16x16x4_f32 in the
// shape of k_mel_warp_mfma above: one workgroup = 64 rows x up to 64 outputs, the reduction in chunks of 64 staged into
// LDS as [row][k], wave w owns rows 16 w .. 16 w + 15 and every 16-wide column tile, lane group g takes
// k = 16 g + 4 q + {0..3} of step q (one 16-byte fragment read per step), a fresh accumulator per chunk and the chunk
// sums added up separately.  Up to three jobs per launch (blockIdx.y):
//   magnitude job: A = E * gE elementwise, formed while staging (E = exp(U^T a), the forward's unwarped magnitudes at the
//                  rows' rate; gE the gradient with respect to them), K = H;
//   phase jobs:    A = grad a / grad b as k_synth_comp_bwd wrote them, K = the phase bins written.
// Rows past the last, outputs past nout and bins past K are staged as zeros (nothing outside the matrices is read: the
// operands carry row padding that nobody initialised).  Plain stores, one writer per element.
// ---------------------------------------------------------------------------------------------
struct UnwarpBwdJob {
    const float* x;      // [rows x K], pitch ldx
    const float* y;      // second factor of the operand, pitch ldy, or null
    const float* W;      // [nout x K], pitch ldw
    float* out;          // [rows x nout], dense
    long long ldx, ldy, ldw;
    long long rows;
    int K;
    int nout;
};
struct UnwarpBwdJobs {
    UnwarpBwdJob j[3];
};

template <int NT>
__device__ __forceinline__ void mel_unwarp_bwd_block(const UnwarpBwdJob& job, float (*As)[kWarpStride],
                                                     float (*Ws)[kWarpStride]) {
    const long long f0 = (long long)blockIdx.x * kWarpTile;
    if (f0 >= job.rows) return;   // the jobs of a launch need not have the same row count
    const int kk = threadIdx.x & 63, fq = threadIdx.x >> 6;   // staging roles: bin within the chunk, row quarter
    const int wave = rfl((int)(threadIdx.x >> 6));
    const int li = kk & 15, g = kk >> 4;                      // fragment roles
    const int K = job.K, nout = job.nout;
    f32x4 tot[NT];
#pragma unroll
    for (int jt = 0; jt < NT; ++jt) tot[jt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int k0 = 0; k0 < K; k0 += 64) {
        const int k = k0 + kk;
        const bool kin = k < K;
        float av[16], wv[4 * NT];
#pragma unroll
        for (int p = 0; p < 16; ++p) {   // rows fq + 4 p: a wave's 64 lanes read 64 consecutive bins of one row
            const long long f = f0 + fq + 4 * p;
            const bool in = kin && f < job.rows;
            float v = in ? job.x[f * job.ldx + k] : 0.0f;
            if (job.y) v *= in ? job.y[f * job.ldy + k] : 0.0f;
            av[p] = v;
        }
#pragma unroll
        for (int p = 0; p < 4 * NT; ++p) {
            const int i = fq + 4 * p;
            wv[p] = (kin && i < nout) ? job.W[(long long)i * job.ldw + k] : 0.0f;
        }
#pragma unroll
        for (int p = 0; p < 16; ++p) As[fq + 4 * p][kk] = av[p];
#pragma unroll
        for (int p = 0; p < 4 * NT; ++p) Ws[fq + 4 * p][kk] = wv[p];
        __syncthreads();
        f32x4 acc[NT];
#pragma unroll
        for (int jt = 0; jt < NT; ++jt) acc[jt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int col = 16 * g + 4 * q;
            const float4 aq = *reinterpret_cast<const float4*>(&As[16 * wave + li][col]);
            float4 bq[NT];
#pragma unroll
            for (int jt = 0; jt < NT; ++jt) bq[jt] = *reinterpret_cast<const float4*>(&Ws[16 * jt + li][col]);
#pragma unroll
            for (int jt = 0; jt < NT; ++jt) acc[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(aq.x, bq[jt].x, acc[jt], 0, 0, 0);
#pragma unroll
            for (int jt = 0; jt < NT; ++jt) acc[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(aq.y, bq[jt].y, acc[jt], 0, 0, 0);
#pragma unroll
            for (int jt = 0; jt < NT; ++jt) acc[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(aq.z, bq[jt].z, acc[jt], 0, 0, 0);
#pragma unroll
            for (int jt = 0; jt < NT; ++jt) acc[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(aq.w, bq[jt].w, acc[jt], 0, 0, 0);
        }
#pragma unroll
        for (int jt = 0; jt < NT; ++jt) tot[jt] += acc[jt];
        __syncthreads();
    }
    // C: column li of tile jt, row 4 g + r of this wave's 16 rows
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long long f = f0 + 16 * wave + 4 * g + r;
        if (f >= job.rows) continue;
#pragma unroll
        for (int jt = 0; jt < NT; ++jt) {
            const int i = 16 * jt + li;
            if (i < nout) job.out[f * nout + i] = tot[jt][r];
        }
    }
}

__global__ __launch_bounds__(256) void k_mel_unwarp_bwd(UnwarpBwdJobs jobs) {
    __shared__ __attribute__((aligned(16))) float As[kWarpTile][kWarpStride];   // As[row][k]
    __shared__ __attribute__((aligned(16))) float Ws[kWarpTile][kWarpStride];   // Ws[i][k]
    const UnwarpBwdJob& job = jobs.j[blockIdx.y];
    const int nt = (job.nout + 15) >> 4;   // wave-uniform (a kernel argument)
    if (nt == 1) mel_unwarp_bwd_block<1>(job, As, Ws);
    else if (nt == 2) mel_unwarp_bwd_block<2>(job, As, Ws);
    else if (nt == 3) mel_unwarp_bwd_block<3>(job, As, Ws);
    else mel_unwarp_bwd_block<4>(job, As, Ws);
}

// ---------------------------------------------------------------------------------------------
// Mel unwarp on the matrix cores: out[F x H] = op(A[F x K] . U[K x H]) with v_mfma_f32_32x32x2_f32 (f32 in, f32
// accumulate: bit-for-bit an fmaf chain in k order, so the result equals the VALU form's).  One wave = one task =
// 32 frames x kUnwarpColTiles column tiles of 32 bins.  Nothing is staged in LDS: A (F x K, a few MB) and U (K x H,
// < 0.5 MB) are L2 resident and a lane's fragment element is one dword either way; the kernel is bound by the
// 12 H bytes per frame it writes.  A fragment: lane l holds A[f0 + (l & 31)][2t + (l >> 5)] for t < KH (kept for
// the whole task); B fragment: U[2t + (l >> 5)][j0 + (l & 31)], the next tile's loads in flight behind this
// tile's KH MFMAs; C: column j0 + (l & 31), row (r & 3) + 8 (r >> 2) + 4 (l >> 5) of register r.
// ---------------------------------------------------------------------------------------------
typedef float f32x16 __attribute__((ext_vector_type(16)));
#ifndef MPX_UNWARP_COL_TILES
#define MPX_UNWARP_COL_TILES 16
#endif
constexpr int kUnwarpColTiles = MPX_UNWARP_COL_TILES;   // 512 bins per task

// MODE 0: one output row per row of A.  MODE 1 / 2 (constant -> variable frame rate, magphase.py:2242-2252 folded in):
// output row f is the interpolation between rows row0[f] and row1[f] of the unwarped A with weight rowt[f] --
//   MODE 1 (linear maps, op 0): the coefficient rows are interpolated, out = U . lerp(A[r0], A[r1]) (the unwarp is
//          linear: equal to lerp(U A[r0], U A[r1]) up to rounding);
//   MODE 2 (op 1, exp): both products are formed (the A fragments of r0 and r1 share every B fragment) and the
//          interpolation runs on the exponentials, lerp(exp(U A[r0]), exp(U A[r1])), as the reference does on m_mag.
// The synthesis kernel then reads ONE row per frame instead of two, and the spectra are written at the variable rate only.
template <int KH, int MODE>
__global__ __launch_bounds__(256) void k_mel_unwarp_mfma(UnwarpJobs jobs, int job0, long long F, int H,
                                                         int col_parts, long long n_tasks, int ld,
                                                         const int* __restrict__ row0, const int* __restrict__ row1,
                                                         const float* __restrict__ rowt, const int* __restrict__ voiced,
                                                         int Hc) {   // Hc <= H: output columns produced
    const UnwarpJob job = jobs.j[job0 + blockIdx.y];
    const int lane = threadIdx.x & 63;
    const long long task = (long long)blockIdx.x * 4 + rfl((int)(threadIdx.x >> 6));   // wave-uniform, and known to be
    if (task >= n_tasks) return;
    // row tile fastest: the 4 waves of a workgroup work on the same columns at the same time and share their B
    // fragments (the U slab) through the vector L1 -- with the column part fastest the kernel is bound by L2 -> L1 traffic
    const long long row_tiles = n_tasks / col_parts;
    const int cp = (int)(task / row_tiles);
    const long long rt = task - cp * row_tiles;
    const long long f0 = rt * 32;
    const int K = job.K;
    const int kk = lane >> 5, li = lane & 31;
    if (MODE == 1 && voiced) {   // phase rows of unvoiced frames are never read: skip tiles without a voiced frame
        if (!__any(voiced[min(f0 + li, F - 1)] != 0)) return;
    }

    float a[KH];
    float a1[MODE == 2 ? KH : 1];   // MODE 2: fragment of the second row
    float tr[MODE == 2 ? 16 : 1];   // MODE 2: interpolation weight of the output row of accumulator register r
    {
        const long long f = min(f0 + li, F - 1);   // rows past F are computed on a copy of the last row, never stored
        const float* arow = job.A + (MODE == 0 ? f : (long long)row0[f]) * K;
        const float* arow1 = (MODE == 0) ? arow : job.A + (long long)row1[f] * K;
        const float wt = (MODE == 0) ? 0.0f : rowt[f];
#pragma unroll
        for (int t = 0; t < KH; ++t) {
            const int k = 2 * t + kk;
            a[t] = arow[min(k, K - 1)];
            a[t] = (k < K) ? a[t] : 0.0f;
            if (MODE != 0) {
                float x1 = arow1[min(k, K - 1)];
                x1 = (k < K) ? x1 : 0.0f;
                if (MODE == 1) a[t] = fmaf(x1 - a[t], wt, a[t]);
                else a1[t] = x1;
            }
        }
        if (MODE == 2) {
#pragma unroll
            for (int r = 0; r < 16; ++r) tr[r] = rowt[min(f0 + (r & 3) + 8 * (r >> 2) + 4 * kk, F - 1)];
        }
    }
    const int jbeg = cp * (kUnwarpColTiles * 32);
    const int jend = min(Hc, jbeg + kUnwarpColTiles * 32);
    if (jbeg >= jend) return;
    // Two column tiles (64 bins) per step: their stores go out back to back, so every row gets 256 contiguous bytes at
    // once.  The B fragments are refilled for the NEXT step right behind the MFMA that consumed them (a whole step of
    // MFMA time for the L2 round trip, no second register set).
    float b0[KH], b1[KH];
    // U[2t + kk][col] through a buffer descriptor: wave-uniform scalar offset 2t H (bytes) + one per-lane offset
    // (kk H + col) -- no per-t address registers; rows >= K fall outside the descriptor and read as 0 (their A element
    // is 0 anyway), columns >= H read the next row's start and are never stored.
    const __amdgpu_buffer_rsrc_t urs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(job.U), 0, K * H * 4, 0x00020000);
    const int row2 = 8 * H;   // bytes between rows 2t and 2t + 2
    // MODE 1 is the linear (phase) jobs, MODE 2 the exp (magnitude) job: known at compile time (as a run-time flag both
    // values are computed and selected for every output element)
    const bool op_exp = (MODE == 1) ? false : ((MODE == 2) ? true : (rfl(job.op) != 0));
    const int nrows = (int)min((long long)32, F - f0);
    const int HO = ld;   // output row pitch
    const __amdgpu_buffer_rsrc_t ors = __builtin_amdgcn_make_buffer_rsrc(job.out + f0 * HO, 0, nrows * HO * 4, 0x00020000);
    // rows k >= K (K odd, or K/2 rounded up to the even KH) multiply a zero of A but must still read finite memory
    // inside U: 2t >= K reads rows 0/1 (scalar select), 2t + 1 == K reads row 2t in both half-waves.
    auto soff = [&](int t) { return (2 * t < K) ? t * row2 : 0; };
    {
        const int v0 = 4 * (kk * H + jbeg + li), v0e = 4 * (jbeg + li);
#pragma unroll
        for (int t = 0; t < KH; ++t) {
            const int v = (2 * t + 1 == K) ? v0e : v0;
            b0[t] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(urs, v, soff(t), 0));
            b1[t] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(urs, v + 128, soff(t), 0));
        }
    }
    const bool full_rows = nrows == 32;
    for (int j0 = jbeg; j0 < jend; j0 += 64) {
        const int vn0 = 4 * (kk * H + j0 + 64 + li), vn0e = 4 * (j0 + 64 + li);
        f32x16 acc0, acc1, acc2, acc3;   // acc2 / acc3: the second row's products (MODE 2)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = acc2[r] = acc3[r] = 0.0f;
#pragma unroll
        for (int t = 0; t < KH; ++t) {
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], b0[t], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], b1[t], acc1, 0, 0, 0);
            if (MODE == 2) {
                acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[t], b0[t], acc2, 0, 0, 0);
                acc3 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[t], b1[t], acc3, 0, 0, 0);
            }
            const int v = (2 * t + 1 == K) ? vn0e : vn0;
            b0[t] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(urs, v, soff(t), 0));
            b1[t] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(urs, v + 128, soff(t), 0));
        }
        // (Forming the product transposed -- lane = frame, four consecutive bins in four registers, one 16-byte store per
        // lane and 8 instead of 32 store instructions per tile -- was measured: 0.61 -> 0.74 ms.  A row then gets 32 bytes
        // per instruction; what this memory system rewards is whole 128-byte lines per instruction, cf. k_analysis.)
        // Stores through a descriptor of this task's output rows: one wave-uniform scalar offset per accumulator
        // register, no address arithmetic.  The bounds check of a raw buffer does not see the scalar offset, so the
        // rows >= F of the last row tile are masked through the per-lane offset (out of range = dropped), like the
        // columns >= H of the last column part.
        const int c0 = j0 + li, c1 = c0 + 32;
        const int vo0 = (c0 < jend) ? 4 * (4 * kk * HO + c0) : 0x7ffffff0;
        const int vo1 = (c1 < jend) ? 4 * (4 * kk * HO + c1) : 0x7ffffff0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2);
            const int so = row * (4 * HO);
            const bool ok = full_rows || (row + 4 * kk < nrows);
            float v0 = op_exp ? __expf(acc0[r]) : acc0[r];
            float v1 = op_exp ? __expf(acc1[r]) : acc1[r];
            if (MODE == 2) {   // fmaf(m1 - m0, t, m0): the form the synthesis kernel used on the two rows
                const float w0 = op_exp ? __expf(acc2[r]) : acc2[r];
                const float w1 = op_exp ? __expf(acc3[r]) : acc3[r];
                v0 = fmaf(w0 - v0, tr[r], v0);
                v1 = fmaf(w1 - v1, tr[r], v1);
            }
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v0), ors, ok ? vo0 : 0x7ffffff0, so, 0);
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v1), ors, ok ? vo1 : 0x7ffffff0, so, 0);
        }
    }
}

struct UnwarpRows {   // constant -> variable rate interpolation tables (all null: one output row per input row)
    const int* row0;
    const int* row1;
    const float* rowt;
    const int* voiced;   // optional (MODE 1): a tile of 32 frames none of which is voiced is skipped -- the synthesis does
                         // not read the phase rows of unvoiced frames
    int phase_cols;      // MODE 1: only the first phase_cols bins of the phase rows are produced (0: all)
};

template <int KH>
static int launch_unwarp_mfma(hipStream_t s, const UnwarpJobs& jobs, int job0, int njobs, long long F, int H, int ld,
                              const UnwarpRows& rw) {
    // the phase rows are only needed below the periodic / aperiodic crossfade (rw.phase_cols, rounded up to a 64-bin step)
    const bool phase = rw.row0 && jobs.j[job0].op == 0;
    const int Hc = (phase && rw.phase_cols > 0) ? min(H, (rw.phase_cols + 63) / 64 * 64) : H;
    const int col_parts = (Hc + kUnwarpColTiles * 32 - 1) / (kUnwarpColTiles * 32);
    const long long n_tasks = ((F + 31) / 32) * col_parts;
    const dim3 grid((unsigned)((n_tasks + 3) / 4), (unsigned)njobs);
    if (!rw.row0)
        hipLaunchKernelGGL((k_mel_unwarp_mfma<KH, 0>), grid, dim3(256), 0, s, jobs, job0, F, H, col_parts, n_tasks, ld,
                           rw.row0, rw.row1, rw.rowt, rw.voiced, Hc);
    else if (phase)
        hipLaunchKernelGGL((k_mel_unwarp_mfma<KH, 1>), grid, dim3(256), 0, s, jobs, job0, F, H, col_parts, n_tasks, ld,
                           rw.row0, rw.row1, rw.rowt, rw.voiced, Hc);
    else
        hipLaunchKernelGGL((k_mel_unwarp_mfma<KH, 2>), grid, dim3(256), 0, s, jobs, job0, F, H, col_parts, n_tasks, ld,
                           rw.row0, rw.row1, rw.rowt, rw.voiced, Hc);
    return MPX_OK;
}

static int dispatch_unwarp_mfma(hipStream_t s, const UnwarpJobs& jobs, int job0, int njobs, int K, long long F, int H,
                                int ld, const UnwarpRows& rw) {
    switch ((K + 3) / 4) {   // KH = K/2 rounded up to even: 16 instantiations cover K <= 64
#define MPX_UNWARP_CASE(q) case q: return launch_unwarp_mfma<2 * q>(s, jobs, job0, njobs, F, H, ld, rw);
        MPX_UNWARP_CASE(1) MPX_UNWARP_CASE(2) MPX_UNWARP_CASE(3) MPX_UNWARP_CASE(4) MPX_UNWARP_CASE(5) MPX_UNWARP_CASE(6)
        MPX_UNWARP_CASE(7) MPX_UNWARP_CASE(8) MPX_UNWARP_CASE(9) MPX_UNWARP_CASE(10) MPX_UNWARP_CASE(11) MPX_UNWARP_CASE(12)
        MPX_UNWARP_CASE(13) MPX_UNWARP_CASE(14) MPX_UNWARP_CASE(15) MPX_UNWARP_CASE(16)
#undef MPX_UNWARP_CASE
    }
    return fail(MPX_ERR_ARG, "mpx_mel_unwarp: coefficient count must be in 1..64%s");
}

// Magnitude unwarp with the constant -> variable rate interpolation, ONE product per constant-rate row (MODE 2 above
// forms two per variable-rate frame: adjacent frames share their rows, 44 % of its MFMAs are repeats).  A task = 32
// constant-rate rows (tiles advance by 31 rows: a frame's two rows are adjacent, so both lie in the tile its row0 falls
// into) x kUnwarpColTiles column tiles.  Per 64-bin step the exp'd 32 x 64 tile goes through a per-wave LDS buffer
// (row stride 72 floats: the accumulator's two half-waves write rows a and a + 4, 32 banks apart) and every
// variable-rate frame of the tile -- [tile_first[T], tile_first[T + 1]), planned on the host -- reads its two rows
// back (lane = bin: 256 contiguous bytes), interpolates with fmaf(m1 - m0, t, m0) and stores its 256-byte row segment.
// Same values as MODE 2 (each row's product is the same fmaf chain).
#ifndef MPX_UNWARP_QUADS
#define MPX_UNWARP_QUADS 1
#endif
constexpr int kTileRows = 31;          // new constant-rate rows per tile
constexpr int kTileStride = 72;        // floats per LDS row

// (Dropping the two special cases for U rows past K when K == 2 KH -- fewer instructions -- made the kernel SLOWER,
// 271 -> 350 us: the selects space the B-fragment loads out between the MFMAs; without them the compiler batches them.)
template <int KH>
__global__ __launch_bounds__(256) void k_mel_unwarp_tiled(UnwarpJob job, long long F, long long n_rows, int H,
                                                          int col_parts, long long n_tasks, int ld,
                                                          const int* __restrict__ row0, const int* __restrict__ row1,
                                                          const float* __restrict__ rowt,
                                                          const int* __restrict__ tile_first) {
    __shared__ __attribute__((aligned(16))) float tiles[4][32 * kTileStride];
    __shared__ __attribute__((aligned(16))) float4 tabs[4][64];
    const int lane = threadIdx.x & 63;
    const int wave = rfl((int)(threadIdx.x >> 6));
    const long long task = (long long)blockIdx.x * 4 + wave;
    if (task >= n_tasks) return;
    const long long row_tiles = n_tasks / col_parts;
    const int cp = (int)(task / row_tiles);
    const long long T = task - cp * row_tiles;
    const long long rb = T * kTileRows;
    const int K = job.K;
    const int kk = lane >> 5, li = lane & 31;
    float* tile = tiles[wave];
    float4* tab = tabs[wave];

    float a[KH];
    {
        const float* arow = job.A + min(rb + li, n_rows - 1) * K;
#pragma unroll
        for (int t = 0; t < KH; ++t) {
            const int k = 2 * t + kk;
            a[t] = arow[min(k, K - 1)];
            a[t] = (k < K) ? a[t] : 0.0f;
        }
    }
    const int fa = rfl(tile_first[T]), fb = rfl(tile_first[T + 1]);
    const int jbeg = cp * (kUnwarpColTiles * 32);
    const int jend = min(H, jbeg + kUnwarpColTiles * 32);
    if (jbeg >= jend || fa >= fb) return;
    float b0[KH], b1[KH];
    const __amdgpu_buffer_rsrc_t urs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(job.U), 0, K * H * 4, 0x00020000);
    const int row2 = 8 * H;
    constexpr bool op_exp = true;   // the tiled form is the magnitudes' (exp epilogue)
    auto soff = [&](int t) { return (2 * t < K) ? t * row2 : 0; };
    {
        const int v0 = 4 * (kk * H + jbeg + li), v0e = 4 * (jbeg + li);
#pragma unroll
        for (int t = 0; t < KH; ++t) {
            const int v = (2 * t + 1 == K) ? v0e : v0;
            b0[t] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(urs, v, soff(t), 0));
            b1[t] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(urs, v + 128, soff(t), 0));
        }
    }
    for (int j0 = jbeg; j0 < jend; j0 += 64) {
        const int vn0 = 4 * (kk * H + j0 + 64 + li), vn0e = 4 * (j0 + 64 + li);
        f32x16 acc0, acc1;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.0f;
#pragma unroll
        for (int t = 0; t < KH; ++t) {
#ifdef MPX_PROBE_UNWARP_NOMFMA   // ablation (timing only): one VALU op per step instead of the two matrix instructions
            acc0[t & 15] = fmaf(a[t], b0[t], acc0[t & 15]);
            acc1[t & 15] = fmaf(a[t], b1[t], acc1[t & 15]);
#else
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], b0[t], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], b1[t], acc1, 0, 0, 0);
#endif
#ifndef MPX_PROBE_UNWARP_NOBLOAD   // ablation: the first step's U fragments for every step
            const int v = (2 * t + 1 == K) ? vn0e : vn0;
            b0[t] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(urs, v, soff(t), 0));
            b1[t] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(urs, v + 128, soff(t), 0));
#else
            asm volatile("" : "+v"(b0[t]), "+v"(b1[t]) : "s"(vn0 + vn0e));
#endif
        }
        wave_sync();   // the previous step's readers are done with the tile
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * kk;
            tile[row * kTileStride + li] = op_exp ? __expf(acc0[r]) : acc0[r];
            tile[row * kTileStride + 32 + li] = op_exp ? __expf(acc1[r]) : acc1[r];
        }
        wave_sync();
        const bool col_ok = j0 + lane < jend;
#ifdef MPX_PROBE_UNWARP_NOINTERP   // ablation (timing only): no interpolation / store phase
        if (tile[lane] == 123.456f) job.out[lane] = 1.0f;
        const int fb_ = fa;
#else
        const int fb_ = fb;
#endif
        for (int fc = fa; fc < fb_; fc += 64) {
            // lane i writes the tables of frame fc + i (tile offsets of its two rows, weight) into a small per-wave LDS
            // table; the loop below reads one entry per frame as a broadcast -- no v_readlane / SGPR round trips (that
            // form spent its time in scalar hazards: 26 M SALU instructions per launch)
            const int fl = min(fc + lane, fb - 1);
            const int r_ = row0[fl] - (int)rb;
            const int d_ = row1[fl] - row0[fl];
            wave_sync();
            tab[lane] = make_float4(__builtin_bit_cast(float, r_ * kTileStride), __builtin_bit_cast(float, (r_ + d_) * kTileStride),
                                    rowt[fl], 0.0f);
            wave_sync();
            const int cnt = min(64, fb - fc);
#if MPX_UNWARP_QUADS
            // FOUR frames per wave instruction (round 5): lane = (frame i + (lane >> 4), bin quad lane & 15) reads 16 bytes of
            // each of its two rows (a 16-lane group reads one row's 256 contiguous bytes: conflict-free), interpolates four
            // bins and stores them as one 16-byte store -- a quarter of the LDS reads and store instructions of the
            // lane-per-bin form, the same values.  Rows are ld floats apart (ld a multiple of 32: 16-byte aligned); the quad
            // that holds bin H - 1 writes up to three floats of the row's padding.
            const int fq = lane >> 4, q4 = 4 * (lane & 15);
            const bool q_ok = j0 + q4 < jend;
            (void)col_ok;
            float* obase = job.out + (long long)fc * ld + j0 + q4;
            for (int i = 0; i < cnt; i += 8) {   // two batches of four frames in flight
                float4 e[2], m0[2], m1[2];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    e[u] = tab[min(i + 4 * u + fq, cnt - 1)];
                    m0[u] = *reinterpret_cast<const float4*>(tile + __builtin_bit_cast(int, e[u].x) + q4);
                    m1[u] = *reinterpret_cast<const float4*>(tile + __builtin_bit_cast(int, e[u].y) + q4);
                }
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int f = i + 4 * u + fq;
                    const float w = e[u].z;
                    float4 v;
                    v.x = fmaf(m1[u].x - m0[u].x, w, m0[u].x);
                    v.y = fmaf(m1[u].y - m0[u].y, w, m0[u].y);
                    v.z = fmaf(m1[u].z - m0[u].z, w, m0[u].z);
                    v.w = fmaf(m1[u].w - m0[u].w, w, m0[u].w);
                    if (q_ok && f < cnt) *reinterpret_cast<float4*>(obase + (long long)f * ld) = v;
                }
            }
#else
            float* orow = job.out + (long long)fc * ld + j0 + lane;
            for (int i = 0; i < cnt; i += 4) {   // four frames per iteration: their LDS reads are in flight together
                float m0[4], m1[4], w[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float4 e = tab[min(i + u, cnt - 1)];
                    m0[u] = tile[__builtin_bit_cast(int, e.x) + lane];
                    m1[u] = tile[__builtin_bit_cast(int, e.y) + lane];
                    w[u] = e.z;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
#ifdef MPX_PROBE_UNWARP_NOSTORE    // ablation: everything but the global stores
                    asm volatile("" ::"v"(fmaf(m1[u] - m0[u], w[u], m0[u])), "v"(orow));
#else
                    if (col_ok && i + u < cnt) orow[(long long)(i + u) * ld] = fmaf(m1[u] - m0[u], w[u], m0[u]);
#endif
                }
            }
#endif
        }
    }
}

template <int KH>
static int launch_unwarp_tiled(hipStream_t s, const UnwarpJob& job, long long F, long long n_rows, int H, int ld,
                               const UnwarpRows& rw, const int* tile_first) {
    const int col_parts = (H + kUnwarpColTiles * 32 - 1) / (kUnwarpColTiles * 32);
    const long long row_tiles = (n_rows + kTileRows - 1) / kTileRows;
    const long long n_tasks = row_tiles * col_parts;
    hipLaunchKernelGGL((k_mel_unwarp_tiled<KH>), dim3((unsigned)((n_tasks + 3) / 4)), dim3(256), 0, s, job, F, n_rows, H,
                       col_parts, n_tasks, ld, rw.row0, rw.row1, rw.rowt, tile_first);
    return MPX_OK;
}

static int dispatch_unwarp_tiled(hipStream_t s, const UnwarpJob& job, int K, long long F, long long n_rows, int H, int ld,
                                 const UnwarpRows& rw, const int* tile_first) {
    if (job.op != 1) return fail(MPX_ERR_ARG, "mpx_mel_unwarp_rows: the tiled form is the exp job's%s");
    if (MPX_UNWARP_QUADS && ((ld & 3) || (reinterpret_cast<uintptr_t>(job.out) & 15)))
        return fail(MPX_ERR_ARG, "mpx_mel_unwarp_rows: with tile_first the output rows must be 16-byte aligned (ld a multiple of 4: mpx_spec_ld)%s");
    switch ((K + 3) / 4) {
#define MPX_UNWARP_CASE(q) case q: return launch_unwarp_tiled<2 * q>(s, job, F, n_rows, H, ld, rw, tile_first);
        MPX_UNWARP_CASE(1) MPX_UNWARP_CASE(2) MPX_UNWARP_CASE(3) MPX_UNWARP_CASE(4) MPX_UNWARP_CASE(5) MPX_UNWARP_CASE(6)
        MPX_UNWARP_CASE(7) MPX_UNWARP_CASE(8) MPX_UNWARP_CASE(9) MPX_UNWARP_CASE(10) MPX_UNWARP_CASE(11) MPX_UNWARP_CASE(12)
        MPX_UNWARP_CASE(13) MPX_UNWARP_CASE(14) MPX_UNWARP_CASE(15) MPX_UNWARP_CASE(16)
#undef MPX_UNWARP_CASE
    }
    return fail(MPX_ERR_ARG, "mpx_mel_unwarp: coefficient count must be in 1..64%s");
}

}  // namespace mpx

using namespace mpx;

extern "C" {

static int mel_unwarp_impl(void* stream, int64_t n_frames, int32_t n_bins, const float* a_mag, int32_t k_mag,
                           const float* u_mag, float* out_mag, const float* a_real, const float* a_imag, int32_t k_phase,
                           const float* u_phase, float* out_real, float* out_imag, int64_t ld, const UnwarpRows& rw,
                           int64_t n_rows = 0, const int32_t* tile_first = nullptr) {
    if (n_frames < 0 || n_bins <= 0 || ld < n_bins || ld > (1 << 20)) return fail(MPX_ERR_ARG, "mpx_mel_unwarp: bad size%s");
    if (k_mag <= 0 || k_mag > kGemmKMax || k_phase <= 0 || k_phase > kGemmKMax)
        return fail(MPX_ERR_ARG, "mpx_mel_unwarp: coefficient count must be in 1..64%s");
    if (n_frames == 0) return MPX_OK;
    if (!a_mag || !u_mag || !out_mag || !a_real || !a_imag || !u_phase || !out_real || !out_imag)
        return fail(MPX_ERR_ARG, "mpx_mel_unwarp: null pointer%s");
    UnwarpJobs jobs;
    jobs.j[0] = {a_mag, u_mag, out_mag, (int)k_mag, 1};
    jobs.j[1] = {a_real, u_phase, out_real, (int)k_phase, 0};
    jobs.j[2] = {a_imag, u_phase, out_imag, (int)k_phase, 0};
    if (tile_first) {   // magnitudes: one product per constant-rate row, interpolated out of an LDS tile
        if (int rc = dispatch_unwarp_tiled((hipStream_t)stream, jobs.j[0], (int)k_mag, (long long)n_frames, (long long)n_rows,
                                           (int)n_bins, (int)ld, rw, tile_first)) return rc;
    } else {
        if (int rc = dispatch_unwarp_mfma((hipStream_t)stream, jobs, 0, 1, (int)k_mag, (long long)n_frames, (int)n_bins, (int)ld, rw)) return rc;
    }
    if (int rc = dispatch_unwarp_mfma((hipStream_t)stream, jobs, 1, 2, (int)k_phase, (long long)n_frames, (int)n_bins, (int)ld, rw)) return rc;
    MPX_HIP_CHECK(hipGetLastError());
    return MPX_OK;
}

int mpx_mel_unwarp(void* stream, int64_t n_frames, int32_t n_bins, const float* a_mag, int32_t k_mag,
                   const float* u_mag, float* out_mag, const float* a_real, const float* a_imag, int32_t k_phase,
                   const float* u_phase, float* out_real, float* out_imag, int64_t ld) {
    return mel_unwarp_impl(stream, n_frames, n_bins, a_mag, k_mag, u_mag, out_mag, a_real, a_imag, k_phase, u_phase,
                           out_real, out_imag, ld, UnwarpRows{nullptr, nullptr, nullptr, nullptr, 0});
}

int mpx_mel_unwarp_rows(void* stream, int64_t n_frames, int32_t n_bins, const float* a_mag, int32_t k_mag,
                        const float* u_mag, float* out_mag, const float* a_real, const float* a_imag, int32_t k_phase,
                        const float* u_phase, float* out_real, float* out_imag, int64_t ld, const int32_t* row0,
                        const int32_t* row1, const float* row_t, int64_t n_rows, const int32_t* tile_first,
                        const int32_t* voiced, int32_t n_phase_bins) {
    if (!row0 || !row1 || !row_t) return fail(MPX_ERR_ARG, "mpx_mel_unwarp_rows: null row table%s");
    if (n_phase_bins < 0) return fail(MPX_ERR_ARG, "mpx_mel_unwarp_rows: negative n_phase_bins%s");
    if (tile_first && n_rows <= 0) return fail(MPX_ERR_ARG, "mpx_mel_unwarp_rows: tile_first needs n_rows%s");
    return mel_unwarp_impl(stream, n_frames, n_bins, a_mag, k_mag, u_mag, out_mag, a_real, a_imag, k_phase, u_phase,
                           out_real, out_imag, ld, UnwarpRows{row0, row1, row_t, voiced, (int)n_phase_bins}, n_rows, tile_first);
}

// n_var_rows / need / tmp_real / tmp_imag: the phase jobs on the variable-rate rows (mpx_mel_warp_rows), or 0 / null
static int mel_warp_impl(void* stream, int64_t n_frames, int32_t n_bins, const float* mag, const float* real,
                         const float* imag, const int32_t* row0, const int32_t* row1, const float* row_t,
                         const float* w_mag, int32_t mag_dim, const float* w_phase, int32_t phase_dim, const float* voiced,
                         float* out_mag, float* out_real, float* out_imag, int64_t ld, int mag_mode,
                         int64_t n_var_rows = 0, const float* need = nullptr, float* tmp_real = nullptr,
                         float* tmp_imag = nullptr) {
    if (n_frames < 0 || n_bins <= 0 || ld < n_bins) return fail(MPX_ERR_ARG, "mpx_mel_warp: bad size%s");
    if (mag_dim <= 0 || mag_dim > kWarpTile || phase_dim <= 0 || phase_dim > kWarpTile)
        return fail(MPX_ERR_ARG, "mpx_mel_warp: output dimension must be in 1..64%s");
    if (n_frames == 0) return MPX_OK;
    if (!mag || !real || !imag || !w_mag || !w_phase || !voiced || !out_mag || !out_real || !out_imag)
        return fail(MPX_ERR_ARG, "mpx_mel_warp: null pointer%s");
    if ((row0 == nullptr) != (row1 == nullptr) || (row0 == nullptr) != (row_t == nullptr))
        return fail(MPX_ERR_ARG, "mpx_mel_warp: row0/row1/row_t must be all null or all given%s");
    const bool phv = tmp_real != nullptr;
    if (phv && (!row0 || !tmp_imag || !need || n_var_rows <= 0))
        return fail(MPX_ERR_ARG, "mpx_mel_warp_rows: the variable-rate phase warp needs row tables, both scratch matrices and the row flags%s");
    WarpJobs jobs;
    jobs.j[0] = {mag, w_mag, out_mag, nullptr, (int)mag_dim, mag_mode, (long long)n_frames};
    if (phv) {
        jobs.j[1] = {real, w_phase, tmp_real, need, (int)phase_dim, 3, (long long)n_var_rows};
        jobs.j[2] = {imag, w_phase, tmp_imag, need, (int)phase_dim, 3, (long long)n_var_rows};
    } else {
        jobs.j[1] = {real, w_phase, out_real, voiced, (int)phase_dim, 1, (long long)n_frames};
        jobs.j[2] = {imag, w_phase, out_imag, voiced, (int)phase_dim, 1, (long long)n_frames};
    }
    const long long max_f = phv ? ((long long)n_frames > (long long)n_var_rows ? (long long)n_frames : (long long)n_var_rows) : (long long)n_frames;
    const dim3 grid((unsigned)((max_f + kWarpTile - 1) / kWarpTile), 3);
    {
        const dim3 g2(grid.x, 3);
        const int ntm = ((int)mag_dim + 15) / 16, ntp = ((int)phase_dim + 15) / 16;
#define MPX_WARP_GO(NTM, NTP, IN, MM, PV)                                                                              \
    hipLaunchKernelGGL((k_mel_warp_mfma<NTM, NTP, IN, MM, PV>), g2, dim3(256), 0, (hipStream_t)stream, jobs, (int)n_bins, \
                       row0, row1, row_t, (long long)ld)
#define MPX_WARP_LAUNCH(NTM, NTP)                                   \
    do {                                                            \
        if (phv && mag_mode == 0) MPX_WARP_GO(NTM, NTP, true, 0, true);      \
        else if (phv) MPX_WARP_GO(NTM, NTP, true, 2, true);         \
        else if (row0 && mag_mode == 0) MPX_WARP_GO(NTM, NTP, true, 0, false);  \
        else if (row0) MPX_WARP_GO(NTM, NTP, true, 2, false);       \
        else if (mag_mode == 0) MPX_WARP_GO(NTM, NTP, false, 0, false);      \
        else MPX_WARP_GO(NTM, NTP, false, 2, false);                \
    } while (0)
#define MPX_WARP_ROW(NTM)                       \
    switch (ntp) {                              \
        case 1: MPX_WARP_LAUNCH(NTM, 1); break; \
        case 2: MPX_WARP_LAUNCH(NTM, 2); break; \
        case 3: MPX_WARP_LAUNCH(NTM, 3); break; \
        default: MPX_WARP_LAUNCH(NTM, 4); break; \
    }
        switch (ntm) {
            case 1: MPX_WARP_ROW(1) break;
            case 2: MPX_WARP_ROW(2) break;
            case 3: MPX_WARP_ROW(3) break;
            default: MPX_WARP_ROW(4) break;
        }
#undef MPX_WARP_ROW
#undef MPX_WARP_LAUNCH
#undef MPX_WARP_GO
    }
    if (phv) {
        const long long n_el = (long long)n_frames * phase_dim;
        hipLaunchKernelGGL(k_warp_phase_rows, dim3((unsigned)((n_el + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                           (const float*)tmp_real, (const float*)tmp_imag, row0, row1, row_t, voiced, (long long)n_frames,
                           (int)phase_dim, out_real, out_imag);
    }
    MPX_HIP_CHECK(hipGetLastError());
    return MPX_OK;
}

// The second half of the constant-rate phase streams on its own (mpx_analysis_compressed_fused_cr leaves their
// variable-rate warp in tmp_real / tmp_imag): row interpolation, voicing mask, clip.
int mpx_warp_phase_rows(void* stream, int64_t n_frames, int32_t phase_dim, const float* tmp_real, const float* tmp_imag,
                        const int32_t* row0, const int32_t* row1, const float* row_t, const float* voiced, float* out_real,
                        float* out_imag) {
    if (n_frames < 0 || phase_dim <= 0) return fail(MPX_ERR_ARG, "mpx_warp_phase_rows: bad size%s");
    if (n_frames == 0) return MPX_OK;
    if (!tmp_real || !tmp_imag || !row0 || !row1 || !row_t || !voiced || !out_real || !out_imag)
        return fail(MPX_ERR_ARG, "mpx_warp_phase_rows: null pointer%s");
    const long long n_el = (long long)n_frames * phase_dim;
    hipLaunchKernelGGL(k_warp_phase_rows, dim3((unsigned)((n_el + 255) / 256)), dim3(256), 0, (hipStream_t)stream, tmp_real,
                       tmp_imag, row0, row1, row_t, voiced, (long long)n_frames, (int)phase_dim, out_real, out_imag);
    MPX_HIP_CHECK(hipGetLastError());
    return MPX_OK;
}

int mpx_mel_warp_backward(void* stream, int32_t n_bins, const float* g_mag, const float* w_mag, int32_t mag_dim,
                          const float* mag, int64_t n_mag_rows, const int32_t* row0, const int32_t* row1,
                          const float* row_t, float* grad_mag, const float* h_real, const float* h_imag,
                          const float* w_phase, int32_t phase_dim, const float* real, const float* imag,
                          int64_t n_phase_rows, const float* live, float* grad_real, float* grad_imag, int64_t ld,
                          int64_t ld_grad) {
    const bool do_mag = grad_mag != nullptr, do_ph = grad_real != nullptr || grad_imag != nullptr;
    if (n_bins <= 0 || n_mag_rows < 0 || n_phase_rows < 0) return fail(MPX_ERR_ARG, "mpx_mel_warp_backward: bad size%s");
    if (ld < n_bins || ld_grad < n_bins) return fail(MPX_ERR_ARG, "mpx_mel_warp_backward: row pitch < n_bins%s");
    if ((do_mag && (mag_dim <= 0 || mag_dim > kWarpTile)) || (do_ph && (phase_dim <= 0 || phase_dim > kWarpTile)))
        return fail(MPX_ERR_ARG, "mpx_mel_warp_backward: n_out must be in 1..64%s");
    if ((row0 == nullptr) != (row1 == nullptr) || (row0 == nullptr) != (row_t == nullptr))
        return fail(MPX_ERR_ARG, "mpx_mel_warp_backward: row0/row1/row_t must be all null or all given%s");
    const long long max_rows = (long long)kWarpTile * 0x7fffffffLL;
    if (n_mag_rows > max_rows || n_phase_rows > max_rows) return fail(MPX_ERR_ARG, "mpx_mel_warp_backward: too many rows%s");
    WarpBwdJobs jobs;
    int n_jobs = 0;
    long long max_f = 0;
    if (do_mag && n_mag_rows > 0) {
        if (!g_mag || !w_mag || !mag) return fail(MPX_ERR_ARG, "mpx_mel_warp_backward: null pointer (magnitude job)%s");
        jobs.j[n_jobs++] = {g_mag, w_mag, mag, grad_mag, nullptr, row0, row1, row_t, (long long)n_mag_rows, (int)mag_dim, 0};
        max_f = (long long)n_mag_rows;
    }
    if (do_ph && n_phase_rows > 0) {
        if (!w_phase || (grad_real && (!h_real || !real)) || (grad_imag && (!h_imag || !imag)))
            return fail(MPX_ERR_ARG, "mpx_mel_warp_backward: null pointer (phase job)%s");
        if (grad_real)
            jobs.j[n_jobs++] = {h_real, w_phase, real, grad_real, live, nullptr, nullptr, nullptr, (long long)n_phase_rows,
                                (int)phase_dim, 1};
        if (grad_imag)
            jobs.j[n_jobs++] = {h_imag, w_phase, imag, grad_imag, live, nullptr, nullptr, nullptr, (long long)n_phase_rows,
                                (int)phase_dim, 1};
        max_f = max_f > (long long)n_phase_rows ? max_f : (long long)n_phase_rows;
    }
    if (n_jobs == 0) return MPX_OK;   // nothing asked for, or no rows: nothing launched
    for (int k = n_jobs; k < 3; ++k) jobs.j[k] = jobs.j[0];   // (never indexed: the grid has n_jobs rows)
    const dim3 grid((unsigned)((max_f + kWarpTile - 1) / kWarpTile), (unsigned)n_jobs);
    hipLaunchKernelGGL(k_mel_warp_bwd, grid, dim3(256), 0, (hipStream_t)stream, jobs, (int)n_bins, (long long)ld,
                       (long long)ld_grad);
    MPX_HIP_CHECK(hipGetLastError());
    return MPX_OK;
}

int mpx_phase_grad_mask(void* stream, int64_t n_frames, int32_t phase_dim, const float* voiced, const float* out_real,
                        const float* out_imag, const float* g_real, const float* g_imag, float* h_real, float* h_imag) {
    if (n_frames < 0 || phase_dim <= 0) return fail(MPX_ERR_ARG, "mpx_phase_grad_mask: bad size%s");
    if (n_frames == 0 || (!h_real && !h_imag)) return MPX_OK;
    if (!voiced || (h_real && (!out_real || !g_real)) || (h_imag && (!out_imag || !g_imag)))
        return fail(MPX_ERR_ARG, "mpx_phase_grad_mask: null pointer%s");
    const long long n_el = (long long)n_frames * phase_dim;
    if ((n_el + 255) / 256 > 0x7fffffffLL) return fail(MPX_ERR_ARG, "mpx_phase_grad_mask: too many elements%s");
    hipLaunchKernelGGL(k_phase_grad_mask, dim3((unsigned)((n_el + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n_el,
                       (int)phase_dim, voiced, out_real, out_imag, g_real, g_imag, h_real, h_imag);
    MPX_HIP_CHECK(hipGetLastError());
    return MPX_OK;
}

int mpx_mel_unwarp_backward(void* stream, int32_t n_bins, const float* e_mag, int64_t ld_e, const float* g_mag,
                            int64_t ld_g, const float* u_mag, int32_t mag_dim, int64_t n_mag_rows, float* grad_a_mag,
                            const float* g_real, const float* g_imag, int64_t ld_phase, int32_t n_phase_bins,
                            const float* u_phase, int32_t phase_dim, int64_t n_phase_rows, float* grad_a_real,
                            float* grad_a_imag) {
    const bool do_mag = grad_a_mag != nullptr, do_ph = grad_a_real != nullptr || grad_a_imag != nullptr;
    if (n_bins <= 0 || n_mag_rows < 0 || n_phase_rows < 0) return fail(MPX_ERR_ARG, "mpx_mel_unwarp_backward: bad size%s");
    if (do_mag && (ld_e < n_bins || ld_g < n_bins)) return fail(MPX_ERR_ARG, "mpx_mel_unwarp_backward: row pitch < n_bins%s");
    if (do_ph && (n_phase_bins < 0 || n_phase_bins > n_bins || ld_phase < n_phase_bins))
        return fail(MPX_ERR_ARG, "mpx_mel_unwarp_backward: n_phase_bins outside [0, n_bins] or above the row pitch%s");
    if ((do_mag && (mag_dim <= 0 || mag_dim > kWarpTile)) || (do_ph && (phase_dim <= 0 || phase_dim > kWarpTile)))
        return fail(MPX_ERR_ARG, "mpx_mel_unwarp_backward: n_out must be in 1..64%s");
    const long long max_rows = (long long)kWarpTile * 0x7fffffffLL;
    if (n_mag_rows > max_rows || n_phase_rows > max_rows) return fail(MPX_ERR_ARG, "mpx_mel_unwarp_backward: too many rows%s");
    UnwarpBwdJobs jobs;
    int n_jobs = 0;
    long long max_f = 0;
    if (do_mag && n_mag_rows > 0) {
        if (!e_mag || !g_mag || !u_mag) return fail(MPX_ERR_ARG, "mpx_mel_unwarp_backward: null pointer (magnitude job)%s");
        jobs.j[n_jobs++] = {e_mag, g_mag, u_mag, grad_a_mag, (long long)ld_e, (long long)ld_g, (long long)n_bins,
                            (long long)n_mag_rows, (int)n_bins, (int)mag_dim};
        max_f = (long long)n_mag_rows;
    }
    if (do_ph && n_phase_rows > 0) {
        if (!u_phase || (grad_a_real && !g_real) || (grad_a_imag && !g_imag))
            return fail(MPX_ERR_ARG, "mpx_mel_unwarp_backward: null pointer (phase job)%s");
        if (grad_a_real)
            jobs.j[n_jobs++] = {g_real, nullptr, u_phase, grad_a_real, (long long)ld_phase, 0, (long long)n_bins,
                                (long long)n_phase_rows, (int)n_phase_bins, (int)phase_dim};
        if (grad_a_imag)
            jobs.j[n_jobs++] = {g_imag, nullptr, u_phase, grad_a_imag, (long long)ld_phase, 0, (long long)n_bins,
                                (long long)n_phase_rows, (int)n_phase_bins, (int)phase_dim};
        max_f = max_f > (long long)n_phase_rows ? max_f : (long long)n_phase_rows;
    }
    if (n_jobs == 0) return MPX_OK;   // nothing asked for, or no rows: nothing launched
    for (int k = n_jobs; k < 3; ++k) jobs.j[k] = jobs.j[0];   // (never indexed: the grid has n_jobs rows)
    const dim3 grid((unsigned)((max_f + kWarpTile - 1) / kWarpTile), (unsigned)n_jobs);
    hipLaunchKernelGGL(k_mel_unwarp_bwd, grid, dim3(256), 0, (hipStream_t)stream, jobs);
    MPX_HIP_CHECK(hipGetLastError());
    return MPX_OK;
}

int mpx_mel_warp_rows(void* stream, int64_t n_frames, int32_t n_bins, const float* mag, const float* real,
                      const float* imag, const int32_t* row0, const int32_t* row1, const float* row_t, const float* w_mag,
                      int32_t mag_dim, const float* w_phase, int32_t phase_dim, const float* voiced, float* out_mag,
                      float* out_real, float* out_imag, int64_t ld, int32_t mag_fbank, int64_t n_var_rows,
                      const float* rows_in_use, float* tmp_real, float* tmp_imag) {
    return mel_warp_impl(stream, n_frames, n_bins, mag, real, imag, row0, row1, row_t, w_mag, mag_dim, w_phase, phase_dim,
                         voiced, out_mag, out_real, out_imag, ld, mag_fbank ? 2 : 0, n_var_rows, rows_in_use, tmp_real,
                         tmp_imag);
}

int mpx_mel_warp(void* stream, int64_t n_frames, int32_t n_bins, const float* mag, const float* real, const float* imag,
                 const int32_t* row0, const int32_t* row1, const float* row_t, const float* w_mag, int32_t mag_dim,
                 const float* w_phase, int32_t phase_dim, const float* voiced, float* out_mag, float* out_real,
                 float* out_imag, int64_t ld) {
    return mel_warp_impl(stream, n_frames, n_bins, mag, real, imag, row0, row1, row_t, w_mag, mag_dim, w_phase, phase_dim,
                         voiced, out_mag, out_real, out_imag, ld, 0);
}

int mpx_mel_warp_fbank(void* stream, int64_t n_frames, int32_t n_bins, const float* mag, const float* real,
                       const float* imag, const int32_t* row0, const int32_t* row1, const float* row_t,
                       const float* w_fbank, int32_t mag_dim, const float* w_phase, int32_t phase_dim, const float* voiced,
                       float* out_mag, float* out_real, float* out_imag, int64_t ld) {
    return mel_warp_impl(stream, n_frames, n_bins, mag, real, imag, row0, row1, row_t, w_fbank, mag_dim, w_phase,
                         phase_dim, voiced, out_mag, out_real, out_imag, ld, 2);
}

}  // extern "C"
