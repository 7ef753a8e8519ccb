// Streaming second moments of windows of f32 frames and of their frame-to-frame differences in f64 (the PCA / SFA of
// cpc2_amd/dim_reduction.py).  x is [b][s][d]; of each sequence the frames t = skip .. s-1 are kept:
//   sums[d] += sum x_t,   gram[d][d] += sum x_t x_t^T            over the kept frames,
//   dgram[d][d] += sum (x_{t+1} - x_t)(x_{t+1} - x_t)^T          over t = skip .. s-2 of each sequence.
//
//   seq_moments_partial_kernel  the plan of moments_partial_kernel (moments.hip): one workgroup per (64 x 64 tile of the upper
//                               block triangle, row range) over the b * s rows in slabs of 32.  The stager loads x[r] and, where
//                               row r has a successor in its sequence, x[r + 1]; it writes an f32 level image and an f64
//                               difference image (the difference of the two f32 values taken in f64: exact) to LDS.  A skipped
//                               frame is staged as zero in both, and so is the difference of a sequence's last frame: nothing is
//                               read across a sequence boundary, from the gap behind a sequence or from the columns beyond d,
//                               and what is not read cannot reach a result (no multiplication by a mask).
//                               Both images go through v_mfma_f64_16x16x4_f64, a fresh chain per slab added to the running tile
//                               in plain f64 (the instruction's own accumulation truncates: DESIGN.md section 17).
//   seq_moments_reduce_kernel   per element of the upper triangle of gram and of dgram: the partial tiles of the S row ranges
//                               added in range order, the total added to the running matrix and stored at the mirrored position
//                               too; sums likewise.
// S depends on (b * s, d) alone and there is no float atomic: the same call gives the same bits, both triangles equal.
//
//   center_scale_rows_kernel    y = (x - mean) / (scale + 1e-8f) per column in f32, each step rounded once (the reference's two
//                               in-place steps in one pass, out of place or exactly in place).
#include "common.h"

#include <algorithm>

namespace cpc {
namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int SQ_THREADS = 256;
constexpr int SQ_T = 64;             // tile edge
constexpr int SQ_SLAB = 32;          // rows per LDS slab
constexpr int SQ_LS = SQ_T + 16;     // LDS row stride in elements, for the f32 and the f64 images (moments.hip: MO_LS)
constexpr int SQ_PF = SQ_SLAB * SQ_T / SQ_THREADS;      // staged elements per thread and operand
constexpr int SQ_MAX_D = 512;
constexpr int SQ_TARGET_WGS = 1024;  // workgroups wanted (4 per CU)
constexpr int SQ_MIN_ROWS = 256;     // smallest row range worth a workgroup
constexpr int CS_MAX_D = 512;

static_assert(SQ_THREADS / SQ_T * SQ_PF == SQ_SLAB, "each thread stages one column");
static_assert(2 * SQ_SLAB * SQ_LS * (sizeof(float) + sizeof(double)) + SQ_THREADS * sizeof(double) <= 64 * 1024,
              "the four images and the column sums fit the static LDS");

struct SeqMomentsPlan {
    int T;               // tiles per edge
    int P;               // tiles of the upper block triangle
    int S;               // row ranges
    long rows_per;       // rows per range (multiple of SQ_SLAB)
};

SeqMomentsPlan seq_moments_plan(long n, int d)
{
    SeqMomentsPlan p;
    p.T = (d + SQ_T - 1) / SQ_T;
    p.P = p.T * (p.T + 1) / 2;
    const long want = std::max(1L, std::min(cdiv(SQ_TARGET_WGS, p.P), cdiv(n, SQ_MIN_ROWS)));
    p.rows_per = cdiv(cdiv(n, want), SQ_SLAB) * SQ_SLAB;
    p.S = (int)cdiv(n, p.rows_per);
    return p;
}

bool seq_moments_sizes_ok(int b, int s, int skip, int d)
{
    return b >= 1 && s >= 1 && skip >= 0 && skip < s && d >= 1 && d <= SQ_MAX_D && (long)b * s < (1L << 31);
}

// one 64 x 64 tile of A^T B over the 32 staged rows: four waves, each a 32 x 32 quadrant = 2 x 2 accumulators, from zero
template <typename T>
__device__ __forceinline__ void slab_product(const T *za, const T *zb, int wi, int wj, int kr, int kc, f64x4 (&tot)[2][2])
{
    f64x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (f64x4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int kk = 0; kk < SQ_SLAB / 4; ++kk) {
        const int row = (kk * 4 + kr) * SQ_LS;
        const double a0 = (double)za[row + wi * 32 + kc];
        const double a1 = (double)za[row + wi * 32 + 16 + kc];
        const double b0 = (double)zb[row + wj * 32 + kc];
        const double b1 = (double)zb[row + wj * 32 + 16 + kc];
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) tot[i][j] += acc[i][j];
}

__device__ __forceinline__ void store_tile(double *out, const f64x4 (&tot)[2][2], int wi, int wj, int kr, int kc)
{
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int row = wi * 32 + i * 16 + kr + 4 * reg;        // the f64 result map (moments.hip)
                const int col = wj * 32 + j * 16 + kc;
                out[row * SQ_T + col] = tot[i][j][reg];
            }
}

// partial: [range][tile pair][level, difference][64][64]
__global__ void __launch_bounds__(SQ_THREADS)
seq_moments_partial_kernel(const float *__restrict__ x, long ld, long seq_stride, int s, int skip, int d, long n, long rows_per,
                           int T, double *__restrict__ partial, double *__restrict__ psums)
{
    __shared__ float za[SQ_SLAB * SQ_LS];
    __shared__ float zb[SQ_SLAB * SQ_LS];
    __shared__ double da[SQ_SLAB * SQ_LS];
    __shared__ double db[SQ_SLAB * SQ_LS];
    __shared__ double cs[SQ_THREADS / SQ_T][SQ_T];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wi = wave >> 1, wj = wave & 1;         // the wave's 32 x 32 quadrant
    int ti = 0, tj = blockIdx.x;                     // tile pair blockIdx.x of the upper block triangle, row-major
    while (tj >= T - ti) {
        tj -= T - ti;
        ++ti;
    }
    tj += ti;
    const bool diag = ti == tj;
    const long r_begin = (long)blockIdx.y * rows_per;
    const long r_end = min(n, r_begin + rows_per);

    // this thread stages column c of both operand tiles, rows r_off + 4 i of each slab
    const int c = tid & (SQ_T - 1), r_off = tid / SQ_T;
    const int ga = ti * SQ_T + c, gb = tj * SQ_T + c;
    const bool has_a = ga < d, has_b = gb < d && !diag;

    // (the successors stay f32 in registers and the subtraction waits until the slab is stored: taken here it would hold the
    //  wave at the loads, which are meant to be in flight while the slab before is consumed)
    float va[SQ_PF], vb[SQ_PF], na[SQ_PF], nb[SQ_PF];
    unsigned has_next = 0;                           // bit i: row i of the slab is kept and has a successor in its sequence
    auto fetch = [&](long r0) {
        has_next = 0;
#pragma unroll
        for (int i = 0; i < SQ_PF; ++i) {
            const long r = r0 + r_off + (SQ_THREADS / SQ_T) * i;
            va[i] = 0.0f;
            vb[i] = 0.0f;
            na[i] = 0.0f;
            nb[i] = 0.0f;
            if (r < r_end) {
                const unsigned q = (unsigned)r / (unsigned)s;           // r < n < 2^31
                const int t = (int)((unsigned)r - q * (unsigned)s);
                if (t >= skip) {
                    const float *row = x + (long)q * seq_stride + (long)t * ld;
                    const bool next = t + 1 < s;                        // the successor lies in the same sequence
                    if (next) has_next |= 1u << i;
                    if (has_a) {
                        va[i] = row[ga];
                        if (next) na[i] = row[ld + ga];
                    }
                    if (has_b) {
                        vb[i] = row[gb];
                        if (next) nb[i] = row[ld + gb];
                    }
                }
            }
        }
    };

    f64x4 tot[2][2], dtot[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            tot[i][j] = (f64x4){0.0, 0.0, 0.0, 0.0};
            dtot[i][j] = (f64x4){0.0, 0.0, 0.0, 0.0};
        }
    double csum = 0.0;
    const float *zbp = diag ? za : zb;
    const double *dbp = diag ? da : db;
    const int kr = lane >> 4, kc = lane & 15;

    fetch(r_begin);
    for (long r0 = r_begin; r0 < r_end; r0 += SQ_SLAB) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < SQ_PF; ++i) {
            const int e = (r_off + (SQ_THREADS / SQ_T) * i) * SQ_LS + c;
            const bool next = (has_next >> i) & 1u;
            za[e] = va[i];
            da[e] = next ? (double)na[i] - (double)va[i] : 0.0;
            if (!diag) {
                zb[e] = vb[i];
                db[e] = next ? (double)nb[i] - (double)vb[i] : 0.0;
            } else {
                csum += (double)va[i];
            }
        }
        __syncthreads();
        if (r0 + SQ_SLAB < r_end) fetch(r0 + SQ_SLAB);   // in flight while this slab is consumed
        slab_product(za, zbp, wi, wj, kr, kc, tot);
        slab_product(da, dbp, wi, wj, kr, kc, dtot);
    }

    double *out = partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (2 * SQ_T * SQ_T);
    store_tile(out, tot, wi, wj, kr, kc);
    store_tile(out + SQ_T * SQ_T, dtot, wi, wj, kr, kc);

    if (diag) {
        cs[r_off][c] = csum;
        __syncthreads();
        if (tid < SQ_T) {
            double sum = cs[0][tid];
#pragma unroll
            for (int g = 1; g < SQ_THREADS / SQ_T; ++g) sum += cs[g][tid];
            psums[((size_t)blockIdx.y * T + ti) * SQ_T + tid] = sum;
        }
    }
}

// blocks [0, 32 P): 256 elements of (tile pair, level or difference) blockIdx.x / 16; the blocks behind them: the sums.
// with_diff == 0 (one kept frame per sequence): dgram is not touched.
__global__ void __launch_bounds__(SQ_THREADS)
seq_moments_reduce_kernel(const double *__restrict__ partial, const double *__restrict__ psums, int S, int T, int P, int d,
                          int with_diff, double *__restrict__ gram, double *__restrict__ dgram, double *__restrict__ sums)
{
    constexpr int PER_TILE = SQ_T * SQ_T / SQ_THREADS;
    const int blk = blockIdx.x;
    if (blk >= 2 * P * PER_TILE) {
        const int g = (blk - 2 * P * PER_TILE) * SQ_THREADS + threadIdx.x;
        if (g < d) {
            double acc = 0.0;
            for (int r = 0; r < S; ++r) acc += psums[(size_t)r * T * SQ_T + g];
            sums[g] += acc;
        }
        return;
    }
    const int which = blk / (P * PER_TILE);           // 0: levels, 1: differences
    if (which == 1 && !with_diff) return;
    const int rest = blk - which * P * PER_TILE;
    const int p = rest / PER_TILE;
    int ti = 0, tj = p;
    while (tj >= T - ti) {
        tj -= T - ti;
        ++ti;
    }
    tj += ti;
    const int e = (rest % PER_TILE) * SQ_THREADS + threadIdx.x;
    const int a = e / SQ_T, b = e % SQ_T;
    const int gi = ti * SQ_T + a, gj = tj * SQ_T + b;
    if (gi >= d || gj >= d || gi > gj) return;       // (gi > gj: the lower half of a diagonal tile -- written by its mirror)
    double acc = 0.0;
    for (int r = 0; r < S; ++r) acc += partial[(((size_t)r * P + p) * 2 + which) * (SQ_T * SQ_T) + e];
    double *dst = which ? dgram : gram;
    const double v = dst[(size_t)gi * d + gj] + acc;
    dst[(size_t)gi * d + gj] = v;
    if (gi != gj) dst[(size_t)gj * d + gi] = v;
}

// thread (cx, ry) of block (bx, by): column bx * 64 + cx of the rows by * 4 + ry + k * 4 * gridDim.y
__global__ void __launch_bounds__(256)
center_scale_rows_kernel(const float *x, long ldx, const float *__restrict__ mean, const float *__restrict__ scale, float *y,
                         long ldy, long n, int d)
{
    const int col = blockIdx.x * 64 + threadIdx.x;
    if (col >= d) return;
    const float m = mean[col];
    const long step = (long)gridDim.y * 4;
    if (scale != nullptr) {
        const float den = scale[col] + 1e-8f;
        for (long r = (long)blockIdx.y * 4 + threadIdx.y; r < n; r += step) y[r * ldy + col] = __fdiv_rn(x[r * ldx + col] - m, den);
    } else {
        for (long r = (long)blockIdx.y * 4 + threadIdx.y; r < n; r += step) y[r * ldy + col] = x[r * ldx + col] - m;
    }
}

}  // namespace
}  // namespace cpc

extern "C" size_t cpc_seq_moments_scratch_bytes(int b, int s, int skip, int d)
{
    if (!cpc::seq_moments_sizes_ok(b, s, skip, d)) return 0;
    const cpc::SeqMomentsPlan p = cpc::seq_moments_plan((long)b * s, d);
    cpc::Carver cv(nullptr);
    cv.take<double>((size_t)p.S * p.P * 2 * cpc::SQ_T * cpc::SQ_T);      // partial tiles, levels and differences
    cv.take<double>((size_t)p.S * p.T * cpc::SQ_T);                      // partial sums
    return cv.used();
}

extern "C" int cpc_seq_moments_accumulate(const float *x, long ld, long seq_stride, int b, int s, int skip, int d, double *sums,
                                          double *gram, double *dgram, void *scratch, size_t scratch_bytes, cpc_stream_t stream)
{
    CPC_REQUIRE(cpc::seq_moments_sizes_ok(b, s, skip, d), "seq_moments_accumulate: sizes outside the supported limits (b=%d s=%d "
                "skip=%d d=%d; need b >= 1, 0 <= skip < s, b * s < 2^31, 1 <= d <= 512)", b, s, skip, d);
    CPC_REQUIRE(ld >= d && seq_stride >= (long)s * ld, "seq_moments_accumulate: stride below the width (ld=%ld d=%d seq_stride=%ld "
                "s=%d; need ld >= d and seq_stride >= s * ld)", ld, d, seq_stride, s);
    CPC_REQUIRE(x != nullptr && sums != nullptr && gram != nullptr && dgram != nullptr, "seq_moments_accumulate: null buffer");
    const size_t need = cpc_seq_moments_scratch_bytes(b, s, skip, d);
    CPC_REQUIRE(scratch != nullptr && scratch_bytes >= need, "seq_moments_accumulate: scratch of %zu bytes, %zu needed",
                scratch_bytes, need);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long n = (long)b * s;
    const cpc::SeqMomentsPlan p = cpc::seq_moments_plan(n, d);
    cpc::Carver cv(scratch);
    double *partial = cv.take<double>((size_t)p.S * p.P * 2 * cpc::SQ_T * cpc::SQ_T);
    double *psums = cv.take<double>((size_t)p.S * p.T * cpc::SQ_T);
    hipLaunchKernelGGL(cpc::seq_moments_partial_kernel, dim3((unsigned)p.P, (unsigned)p.S), dim3(cpc::SQ_THREADS), 0, st, x, ld,
                       seq_stride, s, skip, d, n, p.rows_per, p.T, partial, psums);
    CPC_CHECK_LAUNCH("seq_moments_partial_kernel");
    const unsigned blocks = (unsigned)(2 * p.P * (cpc::SQ_T * cpc::SQ_T / cpc::SQ_THREADS) + cpc::cdiv(d, cpc::SQ_THREADS));
    hipLaunchKernelGGL(cpc::seq_moments_reduce_kernel, dim3(blocks), dim3(cpc::SQ_THREADS), 0, st, partial, psums, p.S, p.T, p.P, d,
                       s - skip > 1 ? 1 : 0, gram, dgram, sums);
    CPC_CHECK_LAUNCH("seq_moments_reduce_kernel");
    return CPC_OK;
}

extern "C" int cpc_center_scale_rows(const float *x, long ldx, const float *mean, const float *scale, float *y, long ldy, long n,
                                     int d, cpc_stream_t stream)
{
    CPC_REQUIRE(n >= 1 && d >= 1 && d <= cpc::CS_MAX_D, "center_scale_rows: sizes outside the supported limits (n=%ld d=%d; need "
                "n >= 1, 1 <= d <= 512)", n, d);
    CPC_REQUIRE(ldx >= d && ldy >= d, "center_scale_rows: row stride below the width (ldx=%ld ldy=%ld d=%d)", ldx, ldy, d);
    CPC_REQUIRE(x != nullptr && mean != nullptr && y != nullptr, "center_scale_rows: null buffer");
    CPC_REQUIRE(y != x || ldy == ldx, "center_scale_rows: in place needs ldy == ldx (ldx=%ld ldy=%ld)", ldx, ldy);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const unsigned gy = (unsigned)std::min(cpc::cdiv(n, 4), 4096L);
    hipLaunchKernelGGL(cpc::center_scale_rows_kernel, dim3((unsigned)cpc::cdiv(d, 64), gy), dim3(64, 4), 0, st, x, ldx, mean, scale,
                       y, ldy, n, d);
    CPC_CHECK_LAUNCH("center_scale_rows_kernel");
    return CPC_OK;
}
