// magphase_pack.hip -- k_rows_pack: the feature rows of a batch, as they lie in device memory, gathered into a plan's
// dense float32 buffers (C ABI: mpx_rows_pack).  The caller's rows are anywhere: one tensor per utterance and stream,
// any row stride (column slices of one wide model output), float32 / float16 / bfloat16 / float64.  One launch serves up
// to three streams of different widths (mag | real | imag).
//
// Indexing: by OUTPUT element.  A workgroup owns kPackChunk consecutive elements of one stream's output (row-major,
// `width` columns); thread t takes elements t, t + 256, ... of the chunk, so that every store instruction of a wave
// writes 64 consecutive floats (rows are 10 .. 2049 elements: a wave per row would idle most lanes on the short ones).
// (row, column) of a thread's first element is one 64-bit division; from there it steps by 256 elements with the
// quotient / remainder of 256 / width.  The utterance of the first element is found by a binary search of the stream's
// descriptors (first output rows ascending), the following ones by walking on -- a thread's elements ascend.  No LDS, no
// scratch; loads are element-wide (rows start at any element alignment).
#include <hip/hip_fp16.h>

#include "mpx_common.hpp"

namespace mpx {

constexpr int kPackThreads = 256;
constexpr int kPackPerThread = 8;
constexpr int kPackChunk = kPackThreads * kPackPerThread;

static_assert(sizeof(mpx_pack_desc) == 32, "mpx_pack_desc is 32 bytes (hostmath.ROWS_PACK_DTYPE)");

struct PackStream {
    float* out;
    long long ld, rows;
    int width, blk_end;   // blk_end: workgroups of this and the earlier streams
};

struct PackArgs {
    const mpx_pack_desc* desc;
    int n_utts;
    PackStream s0, s1, s2;
};

// element `idx` of a row block of type `dtype` as the bits of its float32 value: f32 unchanged (NaN payloads, -0), f16 /
// bf16 widened (exact), f64 narrowed (round to nearest even)
__device__ __forceinline__ unsigned pack_load(const void* base, int dtype, long long idx) {
    switch (dtype) {
        case MPX_PACK_F32:
            return static_cast<const unsigned*>(base)[idx];
        case MPX_PACK_F16:
            return __float_as_uint(__half2float(__ushort_as_half(static_cast<const unsigned short*>(base)[idx])));
        case MPX_PACK_BF16:
            return (unsigned)static_cast<const unsigned short*>(base)[idx] << 16;
        default:
            return __float_as_uint((float)static_cast<const double*>(base)[idx]);
    }
}

__global__ __launch_bounds__(kPackThreads) void k_rows_pack(const PackArgs a) {
    const int b = blockIdx.x;
    // (selects, not an indexed array: the arguments stay in scalar registers)
    const bool in0 = b < a.s0.blk_end, in1 = b < a.s1.blk_end;
    const PackStream st = in0 ? a.s0 : (in1 ? a.s1 : a.s2);
    const int b0 = in0 ? 0 : (in1 ? a.s0.blk_end : a.s1.blk_end);
    const mpx_pack_desc* __restrict__ d = a.desc + (long long)(in0 ? 0 : (in1 ? 1 : 2)) * a.n_utts;
    const int w = st.width;
    const long long n_el = st.rows * w;
    long long i = (long long)(b - b0) * kPackChunk + threadIdx.x;
    if (i >= n_el) return;
    long long row = i / w;
    int col = (int)(i - row * w);
    const int dq = kPackThreads / w, dr = kPackThreads % w;
    // the last utterance whose first output row is <= row (zero-row utterances share their successor's first row)
    int lo = 0, hi = a.n_utts;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (d[mid].out_row0 <= row) lo = mid + 1;
        else hi = mid;
    }
    int u = max(lo - 1, 0);
    mpx_pack_desc cur = d[u];
    long long row_end = cur.out_row0 + cur.n_rows;
    unsigned* __restrict__ out = reinterpret_cast<unsigned*>(st.out);
#pragma unroll 1
    for (int k = 0; k < kPackPerThread && i < n_el; ++k) {
        while (row >= row_end && u + 1 < a.n_utts) {
            cur = d[++u];
            row_end = cur.out_row0 + cur.n_rows;
        }
        if (row < row_end)   // (always, for a table mpx_rows_pack has checked)
            out[row * st.ld + col] = pack_load(cur.base, cur.dtype, (row - cur.out_row0) * cur.row_stride + col);
        i += kPackThreads;
        row += dq;
        col += dr;
        if (col >= w) {
            col -= w;
            ++row;
        }
    }
}

}  // namespace mpx

using namespace mpx;

extern "C" int mpx_rows_pack(void* stream, const mpx_pack_desc* table, const mpx_pack_desc* table_host, int32_t n_utts,
                             int32_t n_streams, float* out0, int32_t width0, int64_t ld0, int64_t rows0, float* out1,
                             int32_t width1, int64_t ld1, int64_t rows1, float* out2, int32_t width2, int64_t ld2,
                             int64_t rows2) {
    if (n_utts < 0 || n_streams < 0 || n_streams > 3)
        return fail(MPX_ERR_ARG, "mpx_rows_pack: n_utts must be >= 0 and n_streams 0 .. 3%s");
    float* outs[3] = {out0, out1, out2};
    const int32_t widths[3] = {width0, width1, width2};
    const int64_t lds[3] = {ld0, ld1, ld2}, rows[3] = {rows0, rows1, rows2};
    for (int s = 0; s < n_streams; ++s) {
        if (widths[s] < 0 || lds[s] < 0 || rows[s] < 0) return fail(MPX_ERR_ARG, "mpx_rows_pack: negative size%s");
        if (rows[s] > 0 && widths[s] == 0) return fail(MPX_ERR_ARG, "mpx_rows_pack: rows of width 0%s");
        if (lds[s] < widths[s]) return fail(MPX_ERR_ARG, "mpx_rows_pack: row pitch smaller than the width%s");
        if (rows[s] > (int64_t)1 << 40) return fail(MPX_ERR_ARG, "mpx_rows_pack: too many rows%s");
    }
    if (n_utts == 0 || n_streams == 0) {   // nothing to gather -- but then there must be nothing to fill either
        for (int s = 0; s < n_streams; ++s)
            if (rows[s] != 0) return fail(MPX_ERR_ARG, "mpx_rows_pack: output rows without utterances%s");
        return MPX_OK;
    }
    if (!table || !table_host) return fail(MPX_ERR_ARG, "mpx_rows_pack: null descriptor table%s");
    // the host image of the table is checked in full: the kernel's stores then stay inside [0, rows) of every stream
    for (int s = 0; s < n_streams; ++s) {
        int64_t next = 0;
        for (int u = 0; u < n_utts; ++u) {
            const mpx_pack_desc& e = table_host[(size_t)s * n_utts + u];
            if (e.dtype < MPX_PACK_F32 || e.dtype > MPX_PACK_F64)
                return fail(MPX_ERR_ARG, "mpx_rows_pack: unknown element type code%s");
            if (e.n_rows < 0 || e.row_stride < 0) return fail(MPX_ERR_ARG, "mpx_rows_pack: negative size in the table%s");
            if (e.out_row0 != next)
                return fail(MPX_ERR_ARG, "mpx_rows_pack: first output rows must follow one another from 0%s");
            if (e.n_rows > 0 && !e.base) return fail(MPX_ERR_ARG, "mpx_rows_pack: null row pointer%s");
            next += e.n_rows;
        }
        if (next != rows[s]) return fail(MPX_ERR_ARG, "mpx_rows_pack: the table's rows do not fill the output%s");
        if (rows[s] > 0 && !outs[s]) return fail(MPX_ERR_ARG, "mpx_rows_pack: null output%s");
    }
    PackArgs a;
    a.desc = table;
    a.n_utts = n_utts;
    PackStream* ps[3] = {&a.s0, &a.s1, &a.s2};
    long long blocks = 0;
    for (int s = 0; s < 3; ++s) {
        const bool on = s < n_streams;
        ps[s]->out = on ? outs[s] : nullptr;
        ps[s]->ld = on ? lds[s] : 0;
        ps[s]->rows = on ? rows[s] : 0;
        ps[s]->width = on && widths[s] > 0 ? widths[s] : 1;
        if (on) blocks += (rows[s] * widths[s] + kPackChunk - 1) / kPackChunk;
        if (blocks > 0x7fffffffLL) return fail(MPX_ERR_ARG, "mpx_rows_pack: too many elements for one launch%s");
        ps[s]->blk_end = (int)blocks;
    }
    if (blocks == 0) return MPX_OK;   // zero-row utterances only
    hipLaunchKernelGGL(k_rows_pack, dim3((unsigned)blocks), dim3(kPackThreads), 0, (hipStream_t)stream, a);
    MPX_HIP_CHECK(hipGetLastError());
    return MPX_OK;
}
