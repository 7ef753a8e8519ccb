// Streaming second moments of one or two f32 feature streams in f64 (the CCA of cpc2_amd/cca).
// With row z = [x row, y row] and D = dx + dy:  sums[D] += sum z,  gram[D][D] += sum z z^T.
//
//   moments_partial_kernel  one workgroup per (64 x 64 tile of the upper block triangle, row range).  It walks its rows in
//                           slabs of 32 staged through LDS as f32 (one image per operand tile, one for a diagonal tile),
//                           converts on the way to registers and accumulates on v_mfma_f64_16x16x4_f64: four waves, each a
//                           32 x 32 quadrant = 2 x 2 accumulators, a fresh chain per slab added to the running tile in plain
//                           f64.  A product of two f32 values is exact in f64, so the only rounding is the accumulation.
//                           Columns beyond D and rows beyond the range are staged as zeros.
//                           The operand map is the f32 16x16x4 one (lane l: row / column l & 15, k = l >> 4), the RESULT map
//                           is f64's own: column l & 15, row (l >> 4) + 4 * reg.  A diagonal tile's workgroup also sums its
//                           columns (each thread stages one column, so the sum is taken from its registers).
//   moments_reduce_kernel   per element of the upper triangle: the partial tiles of the S row ranges added in range order,
//                           gram += that, and the same value stored at the mirrored position; sums likewise.
// S depends on (n, dx + dy) alone and there is no float atomic: the same call gives the same bits, and both triangles of gram
// are equal bit for bit.
#include "common.h"

#include <algorithm>

namespace cpc {
namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int MO_THREADS = 256;
constexpr int MO_T = 64;             // tile edge
constexpr int MO_SLAB = 32;          // rows per LDS slab
constexpr int MO_LS = MO_T + 16;     // LDS row stride (floats): the 4 rows of one k-step land on 4 different groups of 16 banks
constexpr int MO_PF = MO_SLAB * MO_T / MO_THREADS;      // staged elements per thread and operand
constexpr int MO_MAX_D = 512;        // per stream
constexpr int MO_TARGET_WGS = 1024;  // workgroups wanted (4 per CU)
constexpr int MO_MIN_ROWS = 256;     // smallest row range worth a workgroup

static_assert(MO_THREADS / MO_T * MO_PF == MO_SLAB, "each thread stages one column");

struct MomentsPlan {
    int T;               // tiles per edge
    int P;               // tiles of the upper block triangle
    int S;               // row ranges
    long rows_per;       // rows per range (multiple of MO_SLAB)
};

MomentsPlan moments_plan(long n, int D)
{
    MomentsPlan p;
    p.T = (D + MO_T - 1) / MO_T;
    p.P = p.T * (p.T + 1) / 2;
    const long want = std::max(1L, std::min(cdiv(MO_TARGET_WGS, p.P), cdiv(n, MO_MIN_ROWS)));
    p.rows_per = cdiv(cdiv(n, want), MO_SLAB) * MO_SLAB;
    p.S = (int)cdiv(n, p.rows_per);
    return p;
}

bool moments_sizes_ok(long n, int dx, int dy)
{
    return n >= 1 && n < (1L << 31) && dx >= 1 && dx <= MO_MAX_D && dy >= 0 && dy <= MO_MAX_D;
}

__global__ void __launch_bounds__(MO_THREADS)
moments_partial_kernel(const float *__restrict__ x, long ldx, int dx, const float *__restrict__ y, long ldy, int dy, long n,
                       long rows_per, int T, double *__restrict__ partial, double *__restrict__ psums)
{
    __shared__ float za[MO_SLAB * MO_LS];
    __shared__ float zb[MO_SLAB * MO_LS];
    __shared__ double cs[MO_THREADS / MO_T][MO_T];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wi = wave >> 1, wj = wave & 1;         // the wave's 32 x 32 quadrant
    const int D = dx + dy;
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
    const int c = tid & (MO_T - 1), r_off = tid / MO_T;
    const int ga = ti * MO_T + c, gb = tj * MO_T + c;
    const float *pa = ga < dx ? x + ga : (ga < D ? y + (ga - dx) : nullptr);
    const float *pb = gb < dx ? x + gb : (gb < D ? y + (gb - dx) : nullptr);
    const long lda = ga < dx ? ldx : ldy, ldb = gb < dx ? ldx : ldy;

    float va[MO_PF], vb[MO_PF];
    auto fetch = [&](long r0) {
#pragma unroll
        for (int i = 0; i < MO_PF; ++i) {
            const long r = r0 + r_off + (MO_THREADS / MO_T) * i;
            va[i] = (pa != nullptr && r < r_end) ? pa[r * lda] : 0.0f;
            if (!diag) vb[i] = (pb != nullptr && r < r_end) ? pb[r * ldb] : 0.0f;
        }
    };

    f64x4 tot[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) tot[i][j] = (f64x4){0.0, 0.0, 0.0, 0.0};
    double csum = 0.0;
    const float *zbp = diag ? za : zb;
    const int kr = lane >> 4, kc = lane & 15;

    fetch(r_begin);
    for (long r0 = r_begin; r0 < r_end; r0 += MO_SLAB) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < MO_PF; ++i) {
            const int e = (r_off + (MO_THREADS / MO_T) * i) * MO_LS + c;
            za[e] = va[i];
            if (!diag) zb[e] = vb[i];
            else csum += (double)va[i];
        }
        __syncthreads();
        if (r0 + MO_SLAB < r_end) fetch(r0 + MO_SLAB);   // in flight while this slab is consumed

        // The matrix instruction's own accumulation is not round-to-nearest: on rows of one sign a chain of it loses about half
        // an ulp of the running sum per step, all in one direction (measured: DESIGN.md section 17).  So a chain lasts one slab,
        // from zero, and the slab's tile joins the running total by an ordinary f64 addition.
        f64x4 acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = (f64x4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kk = 0; kk < MO_SLAB / 4; ++kk) {
            const int row = (kk * 4 + kr) * MO_LS;
            const double a0 = (double)za[row + wi * 32 + kc];
            const double a1 = (double)za[row + wi * 32 + 16 + kc];
            const double b0 = (double)zbp[row + wj * 32 + kc];
            const double b1 = (double)zbp[row + wj * 32 + 16 + kc];
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

    double *out = partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (MO_T * MO_T);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int row = wi * 32 + i * 16 + kr + 4 * reg;        // the f64 result map, not the f32 one
                const int col = wj * 32 + j * 16 + kc;
                out[row * MO_T + col] = tot[i][j][reg];
            }

    if (diag) {
        cs[r_off][c] = csum;
        __syncthreads();
        if (tid < MO_T) {
            double s = cs[0][tid];
#pragma unroll
            for (int g = 1; g < MO_THREADS / MO_T; ++g) s += cs[g][tid];
            psums[((size_t)blockIdx.y * T + ti) * MO_T + tid] = s;
        }
    }
}

// blocks [0, 16 P): 256 elements of tile pair blockIdx.x / 16; the blocks behind them: the sums
__global__ void __launch_bounds__(MO_THREADS)
moments_reduce_kernel(const double *__restrict__ partial, const double *__restrict__ psums, int S, int T, int P, int D,
                      double *__restrict__ gram, double *__restrict__ sums)
{
    constexpr int PER_TILE = MO_T * MO_T / MO_THREADS;
    const int blk = blockIdx.x;
    if (blk >= P * PER_TILE) {
        const int g = (blk - P * PER_TILE) * MO_THREADS + threadIdx.x;
        if (g < D) {
            double acc = 0.0;
            for (int s = 0; s < S; ++s) acc += psums[(size_t)s * T * MO_T + g];
            sums[g] += acc;
        }
        return;
    }
    const int p = blk / PER_TILE;
    int ti = 0, tj = p;
    while (tj >= T - ti) {
        tj -= T - ti;
        ++ti;
    }
    tj += ti;
    const int e = (blk % PER_TILE) * MO_THREADS + threadIdx.x;
    const int a = e / MO_T, b = e % MO_T;
    const int gi = ti * MO_T + a, gj = tj * MO_T + b;
    if (gi >= D || gj >= D || gi > gj) return;       // (gi > gj: the lower half of a diagonal tile -- written by its mirror)
    double acc = 0.0;
    for (int s = 0; s < S; ++s) acc += partial[((size_t)s * P + p) * (MO_T * MO_T) + e];
    const double v = gram[(size_t)gi * D + gj] + acc;
    gram[(size_t)gi * D + gj] = v;
    if (gi != gj) gram[(size_t)gj * D + gi] = v;
}

}  // namespace
}  // namespace cpc

extern "C" size_t cpc_moments_scratch_bytes(long n, int dx, int dy)
{
    if (!cpc::moments_sizes_ok(n, dx, dy)) return 0;
    const cpc::MomentsPlan p = cpc::moments_plan(n, dx + dy);
    cpc::Carver cv(nullptr);
    cv.take<double>((size_t)p.S * p.P * cpc::MO_T * cpc::MO_T);      // partial tiles
    cv.take<double>((size_t)p.S * p.T * cpc::MO_T);                  // partial sums
    return cv.used();
}

extern "C" int cpc_moments_accumulate(const float *x, long ldx, int dx, const float *y, long ldy, int dy, long n,
                                      double *sums, double *gram, void *scratch, size_t scratch_bytes, cpc_stream_t stream)
{
    CPC_REQUIRE(cpc::moments_sizes_ok(n, dx, dy), "moments_accumulate: sizes outside the supported limits (n=%ld dx=%d dy=%d; "
                "need 1 <= n < 2^31, 1 <= dx <= 512, 0 <= dy <= 512)", n, dx, dy);
    CPC_REQUIRE(ldx >= dx && (dy == 0 || ldy >= dy), "moments_accumulate: row stride below the width (ldx=%ld dx=%d ldy=%ld dy=%d)",
                ldx, dx, ldy, dy);
    CPC_REQUIRE(x != nullptr && (dy == 0 || y != nullptr) && sums != nullptr && gram != nullptr, "moments_accumulate: null buffer");
    const size_t need = cpc_moments_scratch_bytes(n, dx, dy);
    CPC_REQUIRE(scratch != nullptr && scratch_bytes >= need, "moments_accumulate: scratch of %zu bytes, %zu needed", scratch_bytes,
                need);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const cpc::MomentsPlan p = cpc::moments_plan(n, dx + dy);
    cpc::Carver cv(scratch);
    double *partial = cv.take<double>((size_t)p.S * p.P * cpc::MO_T * cpc::MO_T);
    double *psums = cv.take<double>((size_t)p.S * p.T * cpc::MO_T);
    hipLaunchKernelGGL(cpc::moments_partial_kernel, dim3((unsigned)p.P, (unsigned)p.S), dim3(cpc::MO_THREADS), 0, s, x, ldx, dx,
                       y, ldy, dy, n, p.rows_per, p.T, partial, psums);
    CPC_CHECK_LAUNCH("moments_partial_kernel");
    const unsigned blocks = (unsigned)(p.P * (cpc::MO_T * cpc::MO_T / cpc::MO_THREADS) + cpc::cdiv(dx + dy, cpc::MO_THREADS));
    hipLaunchKernelGGL(cpc::moments_reduce_kernel, dim3(blocks), dim3(cpc::MO_THREADS), 0, s, partial, psums, p.S, p.T, p.P,
                       dx + dy, gram, sums);
    CPC_CHECK_LAUNCH("moments_reduce_kernel");
    return CPC_OK;
}
