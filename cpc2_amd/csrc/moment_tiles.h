// The f64 moment tile that moments.hip (two streams side by side) and seqmoments.hip (frames and their successor differences)
// share: the plan, the tile pair of a workgroup, the MFMA slab product, the result-map store, the column sums of a diagonal
// tile and the reduce kernel.  Each file keeps its own stager.  DESIGN.md section 17 has the layout and the measurements.
//
// One workgroup per (64 x 64 tile of the upper block triangle, row range).  It walks its rows in slabs of 32 staged through
// LDS, converts on the way to registers and accumulates on v_mfma_f64_16x16x4_f64: four waves, each a 32 x 32 quadrant = 2 x 2
// accumulators.  The operand map is the f32 16x16x4 one (lane l: row / column l & 15, k = l >> 4), the RESULT map is f64's
// own: column l & 15, row (l >> 4) + 4 * reg.
#pragma once
#include "common.h"

#include <algorithm>

namespace cpc {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int MT_THREADS = 256;
constexpr int MT_T = 64;             // tile edge
constexpr int MT_SLAB = 32;          // rows per LDS slab
constexpr int MT_LS = MT_T + 16;     // LDS row stride (elements): the 4 rows of one k-step land on 4 different groups of 16 banks
constexpr int MT_PF = MT_SLAB * MT_T / MT_THREADS;      // staged elements per thread and operand
constexpr int MT_MAX_D = 512;        // widest stream
constexpr int MT_TARGET_WGS = 1024;  // workgroups wanted (4 per CU)
constexpr int MT_MIN_ROWS = 256;     // smallest row range worth a workgroup

static_assert(MT_THREADS / MT_T * MT_PF == MT_SLAB, "each thread stages one column");

struct MomentPlan {
    int T;               // tiles per edge
    int P;               // tiles of the upper block triangle
    int S;               // row ranges
    long rows_per;       // rows per range (multiple of MT_SLAB)
};

// S depends on (n, D) alone
static inline MomentPlan moment_plan(long n, int D)
{
    MomentPlan p;
    p.T = (D + MT_T - 1) / MT_T;
    p.P = p.T * (p.T + 1) / 2;
    const long want = std::max(1L, std::min(cdiv(MT_TARGET_WGS, p.P), cdiv(n, MT_MIN_ROWS)));
    p.rows_per = cdiv(cdiv(n, want), MT_SLAB) * MT_SLAB;
    p.S = (int)cdiv(n, p.rows_per);
    return p;
}

// Declares (ti, tj), ti <= tj: tile pair p of the upper block triangle of T x T tiles, row-major.  A macro, not a function: with
// the loop behind a call (by reference or by value) hipcc's output for the partial kernels changes -- it no longer marks the
// staged columns ti * 64 + c, tj * 64 + c as non-negative and sign-extends every staged address -- and
// seq_moments_partial_kernel takes 2.8 % longer (measured: profiles/eval_kernels_ab.md).
#define CPC_TILE_PAIR(p, T, ti, tj) \
    int ti = 0, tj = (p);           \
    while (tj >= (T) - ti) {        \
        tj -= (T) - ti;             \
        ++ti;                       \
    }                               \
    tj += ti

// one 64 x 64 tile of A^T B over the 32 staged rows, added to tot.  The matrix instruction's own accumulation is not
// round-to-nearest: on rows of one sign a chain of it loses about half an ulp of the running sum per step, all in one direction
// (measured: DESIGN.md section 17).  So a chain lasts one slab, from zero, and the slab's tile joins the running total by an
// ordinary f64 addition.
template <typename T>
__device__ __forceinline__ void slab_product(const T *za, const T *zb, int wi, int wj, int kr, int kc, f64x4 (&tot)[2][2])
{
    f64x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (f64x4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int kk = 0; kk < MT_SLAB / 4; ++kk) {
        const int row = (kk * 4 + kr) * MT_LS;
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
                const int row = wi * 32 + i * 16 + kr + 4 * reg;        // the f64 result map, not the f32 one
                const int col = wj * 32 + j * 16 + kc;
                out[row * MT_T + col] = tot[i][j][reg];
            }
}

// The column sums of a diagonal tile: thread tid has summed the rows it staged of column tid % 64 (csum); the four threads of
// a column are added in thread order and column c goes to dst[c].  Called by the whole workgroup.
__device__ __forceinline__ void store_column_sums(double (&cs)[MT_THREADS / MT_T][MT_T], double csum, double *dst)
{
    const int tid = threadIdx.x;
    cs[tid / MT_T][tid & (MT_T - 1)] = csum;
    __syncthreads();
    if (tid < MT_T) {
        double s = cs[0][tid];
#pragma unroll
        for (int g = 1; g < MT_THREADS / MT_T; ++g) s += cs[g][tid];
        dst[tid] = s;
    }
}

// partial [S][P][nmat][64][64], psums [S][T][64].  Per element of the upper triangle of each of the nmat (1 or 2) matrices:
// the partial tiles of the S row ranges added in range order, the total added to the running matrix (0: gram, 1: dgram) and the
// same value stored at the mirrored position; sums likewise.  with_diff == 0: dgram is not touched.  Grid: 16 nmat P blocks
// of 256 elements, matrix-major, and behind them cdiv(D, 256) blocks for the sums.  (Defined in moments.hip.)
__global__ void moment_reduce_kernel(const double *partial, const double *psums, int S, int T, int P, int D, int nmat, int with_diff,
                                     double *gram, double *dgram, double *sums);

}  // namespace cpc
