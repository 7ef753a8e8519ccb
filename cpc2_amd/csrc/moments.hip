// Streaming second moments of one or two f32 feature streams in f64 (the CCA of cpc2_amd/cca).
// With row z = [x row, y row] and D = dx + dy:  sums[D] += sum z,  gram[D][D] += sum z z^T.
//
//   moments_partial_kernel  the tile plan of moment_tiles.h with this file's stager: one workgroup per (64 x 64 tile of the
//                           upper block triangle, row range); the rows in slabs of 32 staged through LDS as f32 (one image per
//                           operand tile, one for a diagonal tile), a tile taken from x, from y or from both where it straddles
//                           the streams.  A product of two f32 values is exact in f64, so the only rounding is the
//                           accumulation.  Columns beyond D and rows beyond the range are staged as zeros.  A diagonal tile's
//                           workgroup also sums its columns (each thread stages one column, so the sum is taken from its
//                           registers).
//   moment_reduce_kernel    (declared in moment_tiles.h, also seqmoments.hip's) per element of the upper triangle: the partial
//                           tiles of the S row ranges added in range order, gram += that, and the same value stored at the
//                           mirrored position; sums likewise.
// S depends on (n, dx + dy) alone and there is no float atomic: the same call gives the same bits, and both triangles of gram
// are equal bit for bit.
#include "moment_tiles.h"

namespace cpc {
namespace {

bool moments_sizes_ok(long n, int dx, int dy)
{
    return n >= 1 && n < (1L << 31) && dx >= 1 && dx <= MT_MAX_D && dy >= 0 && dy <= MT_MAX_D;
}

__global__ void __launch_bounds__(MT_THREADS)
moments_partial_kernel(const float *__restrict__ x, long ldx, int dx, const float *__restrict__ y, long ldy, int dy, long n,
                       long rows_per, int T, double *__restrict__ partial, double *__restrict__ psums)
{
    __shared__ float za[MT_SLAB * MT_LS];
    __shared__ float zb[MT_SLAB * MT_LS];
    __shared__ double cs[MT_THREADS / MT_T][MT_T];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wi = wave >> 1, wj = wave & 1;         // the wave's 32 x 32 quadrant
    const int D = dx + dy;
    CPC_TILE_PAIR(blockIdx.x, T, ti, tj);
    const bool diag = ti == tj;
    const long r_begin = (long)blockIdx.y * rows_per;
    const long r_end = min(n, r_begin + rows_per);

    // this thread stages column c of both operand tiles, rows r_off + 4 i of each slab
    const int c = tid & (MT_T - 1), r_off = tid / MT_T;
    const int ga = ti * MT_T + c, gb = tj * MT_T + c;
    const float *pa = ga < dx ? x + ga : (ga < D ? y + (ga - dx) : nullptr);
    const float *pb = gb < dx ? x + gb : (gb < D ? y + (gb - dx) : nullptr);
    const long lda = ga < dx ? ldx : ldy, ldb = gb < dx ? ldx : ldy;

    float va[MT_PF], vb[MT_PF];
    auto fetch = [&](long r0) {
#pragma unroll
        for (int i = 0; i < MT_PF; ++i) {
            const long r = r0 + r_off + (MT_THREADS / MT_T) * i;
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
    for (long r0 = r_begin; r0 < r_end; r0 += MT_SLAB) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < MT_PF; ++i) {
            const int e = (r_off + (MT_THREADS / MT_T) * i) * MT_LS + c;
            za[e] = va[i];
            if (!diag) zb[e] = vb[i];
            else csum += (double)va[i];
        }
        __syncthreads();
        if (r0 + MT_SLAB < r_end) fetch(r0 + MT_SLAB);   // in flight while this slab is consumed
        slab_product(za, zbp, wi, wj, kr, kc, tot);
    }

    store_tile(partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (MT_T * MT_T), tot, wi, wj, kr, kc);
    if (diag) store_column_sums(cs, csum, psums + ((size_t)blockIdx.y * T + ti) * MT_T);
}

}  // namespace

__global__ void __launch_bounds__(MT_THREADS)
moment_reduce_kernel(const double *__restrict__ partial, const double *__restrict__ psums, int S, int T, int P, int D, int nmat,
                     int with_diff, double *__restrict__ gram, double *__restrict__ dgram, double *__restrict__ sums)
{
    constexpr int PER_TILE = MT_T * MT_T / MT_THREADS;
    const int blk = blockIdx.x;
    if (blk >= nmat * P * PER_TILE) {
        const int g = (blk - nmat * P * PER_TILE) * MT_THREADS + threadIdx.x;
        if (g < D) {
            double acc = 0.0;
            for (int r = 0; r < S; ++r) acc += psums[(size_t)r * T * MT_T + g];
            sums[g] += acc;
        }
        return;
    }
    const int which = blk / (P * PER_TILE);           // 0: levels, 1: differences
    if (which == 1 && !with_diff) return;
    const int rest = blk - which * P * PER_TILE;
    const int p = rest / PER_TILE;
    CPC_TILE_PAIR(p, T, ti, tj);
    const int e = (rest % PER_TILE) * MT_THREADS + threadIdx.x;
    const int a = e / MT_T, b = e % MT_T;
    const int gi = ti * MT_T + a, gj = tj * MT_T + b;
    if (gi >= D || gj >= D || gi > gj) return;       // (gi > gj: the lower half of a diagonal tile -- written by its mirror)
    double acc = 0.0;
    for (int r = 0; r < S; ++r) acc += partial[(((size_t)r * P + p) * nmat + which) * (MT_T * MT_T) + e];
    double *dst = which ? dgram : gram;
    const double v = dst[(size_t)gi * D + gj] + acc;
    dst[(size_t)gi * D + gj] = v;
    if (gi != gj) dst[(size_t)gj * D + gi] = v;
}

}  // namespace cpc

extern "C" size_t cpc_moments_scratch_bytes(long n, int dx, int dy)
{
    if (!cpc::moments_sizes_ok(n, dx, dy)) return 0;
    const cpc::MomentPlan p = cpc::moment_plan(n, dx + dy);
    cpc::Carver cv(nullptr);
    cv.take<double>((size_t)p.S * p.P * cpc::MT_T * cpc::MT_T);      // partial tiles
    cv.take<double>((size_t)p.S * p.T * cpc::MT_T);                  // partial sums
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
    const cpc::MomentPlan p = cpc::moment_plan(n, dx + dy);
    cpc::Carver cv(scratch);
    double *partial = cv.take<double>((size_t)p.S * p.P * cpc::MT_T * cpc::MT_T);
    double *psums = cv.take<double>((size_t)p.S * p.T * cpc::MT_T);
    hipLaunchKernelGGL(cpc::moments_partial_kernel, dim3((unsigned)p.P, (unsigned)p.S), dim3(cpc::MT_THREADS), 0, s, x, ldx, dx,
                       y, ldy, dy, n, p.rows_per, p.T, partial, psums);
    CPC_CHECK_LAUNCH("moments_partial_kernel");
    const unsigned blocks = (unsigned)(p.P * (cpc::MT_T * cpc::MT_T / cpc::MT_THREADS) + cpc::cdiv(dx + dy, cpc::MT_THREADS));
    hipLaunchKernelGGL(cpc::moment_reduce_kernel, dim3(blocks), dim3(cpc::MT_THREADS), 0, s, partial, psums, p.S, p.T, p.P,
                       dx + dy, 1, 0, gram, nullptr, sums);
    CPC_CHECK_LAUNCH("moment_reduce_kernel");
    return CPC_OK;
}
