// Decimal text of a device matrix, for the `fea` files of cpc2_amd/eval/build_zeroSpeech_features.py (the reference's
// cpc/eval/build_zeroSpeech_features.py:70-77: one line per frame, the time and then str(x) of every value).
//
//   row r of the output = prefix[r] ' '  v(r, 0) ' ' v(r, 1) ... v(r, cols - 1) '\n'      (without prefixes: no leading blank)
//
//   text_f32_kernel / text_i64_kernel   one thread per value: its text -- repr(float(v)) byte for byte (text_digits.h), or the
//                       plain decimal integer -- goes to a slot of 24 bytes (three 8-byte words), its length to a byte
//   text_row_bytes_kernel   one wave per row: the bytes of the row (texts, separators, prefix, newline) as an int64.  The
//                       caller's exclusive scan of them gives where every row starts
//   text_pack_kernel    one workgroup per row: an exclusive scan of (length + 1) along the row, 256 values at a time, gives where
//                       every value starts; each thread copies its slot's bytes and the separator behind them, the threads together
//                       the prefix
// All offsets are 64-bit: 256 values a frame pass 2 GB of text after 67 minutes of audio.
#include "common.h"
#include "text_digits.h"

#include <algorithm>

namespace cpc {

constexpr int TX_THREADS = 256;

__global__ __launch_bounds__(TX_THREADS) void text_f32_kernel(const float *x, long count, unsigned long long *slots, unsigned char *len)
{
    for (long i = (long)blockIdx.x * TX_THREADS + threadIdx.x; i < count; i += (long)gridDim.x * TX_THREADS) {
        const text::Slot s = text::format_f32_bits(__float_as_uint(x[i]));
        slots[3 * i] = s.w0;
        slots[3 * i + 1] = s.w1;
        slots[3 * i + 2] = s.w2;
        len[i] = (unsigned char)s.len;
    }
}

__global__ __launch_bounds__(TX_THREADS) void text_i64_kernel(const long *x, long count, unsigned long long *slots, unsigned char *len)
{
    for (long i = (long)blockIdx.x * TX_THREADS + threadIdx.x; i < count; i += (long)gridDim.x * TX_THREADS) {
        const text::Slot s = text::format_i64((int64_t)x[i]);
        slots[3 * i] = s.w0;
        slots[3 * i + 1] = s.w1;
        slots[3 * i + 2] = s.w2;
        len[i] = (unsigned char)s.len;
    }
}

// bytes in front of the first value of row r: the prefix and the blank behind it
__device__ __forceinline__ long text_lead(const long *prefix_off, long r)
{
    return prefix_off != nullptr ? prefix_off[r + 1] - prefix_off[r] + 1 : 0;
}

__global__ __launch_bounds__(TX_THREADS) void text_row_bytes_kernel(const unsigned char *len, long rows, int cols, const long *prefix_off,
                                                                    long *row_bytes)
{
    const int lane = threadIdx.x & 63;
    const long waves = (long)gridDim.x * (TX_THREADS / 64);
    for (long r = (long)blockIdx.x * (TX_THREADS / 64) + (threadIdx.x >> 6); r < rows; r += waves) {
        unsigned sum = 0;                                              // (<= 24 cols < 2^31: the entry refuses cols >= 2^26)
        for (int c = lane; c < cols; c += 64) sum += len[r * cols + c];
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d, 64);
        if (lane == 0) row_bytes[r] = (long)sum + cols + text_lead(prefix_off, r);     // (a blank or the newline behind every value)
    }
}

__global__ __launch_bounds__(TX_THREADS) void text_pack_kernel(const unsigned long long *slots, const unsigned char *len, long rows, int cols,
                                                               const unsigned char *prefix, const long *prefix_off, const long *row_off,
                                                               unsigned char *out, long out_total)
{
    __shared__ unsigned wave_sum[TX_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long r = blockIdx.x; r < rows; r += gridDim.x) {
        const long lead = text_lead(prefix_off, r);
        long at = row_off[r];
        const long row_end = r + 1 < rows ? row_off[r + 1] : out_total;
        if (at < 0 || row_end > out_total || at + lead > row_end) continue;          // (offsets that do not fit the buffer: nothing is written)
        if (prefix_off != nullptr) {
            const long p0 = prefix_off[r];
            for (long j = threadIdx.x; j < lead - 1; j += TX_THREADS) out[at + j] = prefix[p0 + j];
            if (threadIdx.x == 0) out[at + lead - 1] = ' ';
        }
        at += lead;
        for (int c0 = 0; c0 < cols; c0 += TX_THREADS) {
            const int c = c0 + threadIdx.x;
            const long i = r * cols + c;
            const unsigned n = c < cols ? len[i] : 0u;
            const unsigned mine = c < cols ? n + 1u : 0u;
            unsigned incl = mine;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned up = __shfl_up(incl, d, 64);
                if (lane >= d) incl += up;
            }
            __syncthreads();                                           // (the previous round's wave_sum has been read)
            if (lane == 63) wave_sum[wave] = incl;
            __syncthreads();
            unsigned before = 0, total = 0;
#pragma unroll
            for (int w = 0; w < TX_THREADS / 64; ++w) {
                before += w < wave ? wave_sum[w] : 0u;
                total += wave_sum[w];
            }
            const long o = at + before + incl - mine;
            if (c < cols && n <= (unsigned)text::SLOT_BYTES && o + mine <= row_end) {
                text::Slot s;
                s.w0 = slots[3 * i];
                s.w1 = slots[3 * i + 1];
                s.w2 = slots[3 * i + 2];
                for (unsigned j = 0; j < n; ++j) out[o + j] = (unsigned char)s.byte((int)j);
                out[o + n] = c + 1 < cols ? ' ' : '\n';
            }
            at += total;
        }
    }
}

static unsigned text_blocks(long work_items, long per_block)
{
    return (unsigned)std::min<long>(std::max<long>(cdiv(work_items, per_block), 1), 1L << 20);
}

}  // namespace cpc

extern "C" int cpc_text_format_f32(const float *x, long count, unsigned long long *slots, unsigned char *len, cpc_stream_t stream)
{
    CPC_REQUIRE(x != nullptr && slots != nullptr && len != nullptr && count >= 0, "text_format_f32: bad arguments (count=%ld)", count);
    if (count == 0) return CPC_OK;
    hipLaunchKernelGGL(cpc::text_f32_kernel, dim3(cpc::text_blocks(count, cpc::TX_THREADS)), dim3(cpc::TX_THREADS), 0,
                       static_cast<hipStream_t>(stream), x, count, slots, len);
    CPC_CHECK_LAUNCH("text_f32_kernel");
    return CPC_OK;
}

extern "C" int cpc_text_format_i64(const long *x, long count, unsigned long long *slots, unsigned char *len, cpc_stream_t stream)
{
    CPC_REQUIRE(x != nullptr && slots != nullptr && len != nullptr && count >= 0, "text_format_i64: bad arguments (count=%ld)", count);
    if (count == 0) return CPC_OK;
    hipLaunchKernelGGL(cpc::text_i64_kernel, dim3(cpc::text_blocks(count, cpc::TX_THREADS)), dim3(cpc::TX_THREADS), 0,
                       static_cast<hipStream_t>(stream), x, count, slots, len);
    CPC_CHECK_LAUNCH("text_i64_kernel");
    return CPC_OK;
}

extern "C" int cpc_text_row_bytes(const unsigned char *len, long rows, int cols, const long *prefix_off, long *row_bytes,
                                  cpc_stream_t stream)
{
    CPC_REQUIRE(len != nullptr && row_bytes != nullptr && rows >= 0 && cols >= 1 && cols < (1 << 26),
                "text_row_bytes: bad arguments (rows=%ld cols=%d)", rows, cols);
    if (rows == 0) return CPC_OK;
    hipLaunchKernelGGL(cpc::text_row_bytes_kernel, dim3(cpc::text_blocks(rows, cpc::TX_THREADS / 64)), dim3(cpc::TX_THREADS), 0,
                       static_cast<hipStream_t>(stream), len, rows, cols, prefix_off, row_bytes);
    CPC_CHECK_LAUNCH("text_row_bytes_kernel");
    return CPC_OK;
}

extern "C" int cpc_text_pack(const unsigned long long *slots, const unsigned char *len, long rows, int cols, const unsigned char *prefix,
                             const long *prefix_off, const long *row_off, unsigned char *out, long out_total, cpc_stream_t stream)
{
    CPC_REQUIRE(slots != nullptr && len != nullptr && row_off != nullptr && rows >= 0 && cols >= 1 && cols < (1 << 26) && out_total >= 0 &&
                (out != nullptr || out_total == 0) && (prefix_off == nullptr) == (prefix == nullptr),
                "text_pack: bad arguments (rows=%ld cols=%d out_total=%ld)", rows, cols, out_total);
    if (rows == 0 || out_total == 0) return CPC_OK;
    hipLaunchKernelGGL(cpc::text_pack_kernel, dim3(cpc::text_blocks(rows, 1)), dim3(cpc::TX_THREADS), 0, static_cast<hipStream_t>(stream),
                       slots, len, rows, cols, prefix, prefix_off, row_off, out, out_total);
    CPC_CHECK_LAUNCH("text_pack_kernel");
    return CPC_OK;
}
