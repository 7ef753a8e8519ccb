// Streaming second moments of windows of f32 frames and of their frame-to-frame differences in f64 (the PCA / SFA of
// cpc2_amd/dim_reduction.py).  x is [b][s][d]; of each sequence the frames t = skip .. s-1 are kept:
//   sums[d] += sum x_t,   gram[d][d] += sum x_t x_t^T            over the kept frames,
//   dgram[d][d] += sum (x_{t+1} - x_t)(x_{t+1} - x_t)^T          over t = skip .. s-2 of each sequence.
//
//   seq_moments_partial_kernel  the tile plan of moment_tiles.h with this file's stager: one workgroup per (64 x 64 tile of the
//                               upper block triangle, row range) over the b * s rows in slabs of 32.  The stager loads x[r] and, where
//                               row r has a successor in its sequence, x[r + 1]; it writes an f32 level image and an f64
//                               difference image (the difference of the two f32 values taken in f64: exact) to LDS.  A skipped
//                               frame is staged as zero in both, and so is the difference of a sequence's last frame: nothing is
//                               read across a sequence boundary, from the gap behind a sequence or from the columns beyond d,
//                               and what is not read cannot reach a result (no multiplication by a mask).
//                               Both images go through v_mfma_f64_16x16x4_f64, a fresh chain per slab added to the running tile
//                               in plain f64 (the instruction's own accumulation truncates: DESIGN.md section 17).
//   moment_reduce_kernel        (moment_tiles.h, with two matrices per tile pair) per element of the upper triangle of gram and
//                               of dgram: the partial tiles of the S row ranges added in range order, the total added to the
//                               running matrix and stored at the mirrored position too; sums likewise.  With one kept frame per
//                               sequence dgram is not touched.
// S depends on (b * s, d) alone and there is no float atomic: the same call gives the same bits, both triangles equal.
//
//   center_scale_rows_kernel    y = (x - mean) / (scale + 1e-8f) per column in f32, each step rounded once (the reference's two
//                               in-place steps in one pass, out of place or exactly in place).
#include "moment_tiles.h"

namespace cpc {
namespace {

constexpr int CS_MAX_D = 512;

static_assert(2 * MT_SLAB * MT_LS * (sizeof(float) + sizeof(double)) + MT_THREADS * sizeof(double) <= 64 * 1024,
              "the four images and the column sums fit the static LDS");

bool seq_moments_sizes_ok(int b, int s, int skip, int d)
{
    return b >= 1 && s >= 1 && skip >= 0 && skip < s && d >= 1 && d <= MT_MAX_D && (long)b * s < (1L << 31);
}

// partial: [range][tile pair][level, difference][64][64]
__global__ void __launch_bounds__(MT_THREADS)
seq_moments_partial_kernel(const float *__restrict__ x, long ld, long seq_stride, int s, int skip, int d, long n, long rows_per,
                           int T, double *__restrict__ partial, double *__restrict__ psums)
{
    __shared__ float za[MT_SLAB * MT_LS];
    __shared__ float zb[MT_SLAB * MT_LS];
    __shared__ double da[MT_SLAB * MT_LS];
    __shared__ double db[MT_SLAB * MT_LS];
    __shared__ double cs[MT_THREADS / MT_T][MT_T];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wi = wave >> 1, wj = wave & 1;         // the wave's 32 x 32 quadrant
    CPC_TILE_PAIR(blockIdx.x, T, ti, tj);
    const bool diag = ti == tj;
    const long r_begin = (long)blockIdx.y * rows_per;
    const long r_end = min(n, r_begin + rows_per);

    // this thread stages column c of both operand tiles, rows r_off + 4 i of each slab
    const int c = tid & (MT_T - 1), r_off = tid / MT_T;
    const int ga = ti * MT_T + c, gb = tj * MT_T + c;
    const bool has_a = ga < d, has_b = gb < d && !diag;

    // (the successors stay f32 in registers and the subtraction waits until the slab is stored: taken here it would hold the
    //  wave at the loads, which are meant to be in flight while the slab before is consumed)
    float va[MT_PF], vb[MT_PF], na[MT_PF], nb[MT_PF];
    unsigned has_next = 0;                           // bit i: row i of the slab is kept and has a successor in its sequence
    auto fetch = [&](long r0) {
        has_next = 0;
#pragma unroll
        for (int i = 0; i < MT_PF; ++i) {
            const long r = r0 + r_off + (MT_THREADS / MT_T) * i;
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
    for (long r0 = r_begin; r0 < r_end; r0 += MT_SLAB) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < MT_PF; ++i) {
            const int e = (r_off + (MT_THREADS / MT_T) * i) * MT_LS + c;
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
        if (r0 + MT_SLAB < r_end) fetch(r0 + MT_SLAB);   // in flight while this slab is consumed
        slab_product(za, zbp, wi, wj, kr, kc, tot);
        slab_product(da, dbp, wi, wj, kr, kc, dtot);
    }

    double *out = partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (2 * MT_T * MT_T);
    store_tile(out, tot, wi, wj, kr, kc);
    store_tile(out + MT_T * MT_T, dtot, wi, wj, kr, kc);

    if (diag) store_column_sums(cs, csum, psums + ((size_t)blockIdx.y * T + ti) * MT_T);
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
    const cpc::MomentPlan p = cpc::moment_plan((long)b * s, d);
    cpc::Carver cv(nullptr);
    cv.take<double>((size_t)p.S * p.P * 2 * cpc::MT_T * cpc::MT_T);      // partial tiles, levels and differences
    cv.take<double>((size_t)p.S * p.T * cpc::MT_T);                      // partial sums
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
    const cpc::MomentPlan p = cpc::moment_plan(n, d);
    cpc::Carver cv(scratch);
    double *partial = cv.take<double>((size_t)p.S * p.P * 2 * cpc::MT_T * cpc::MT_T);
    double *psums = cv.take<double>((size_t)p.S * p.T * cpc::MT_T);
    hipLaunchKernelGGL(cpc::seq_moments_partial_kernel, dim3((unsigned)p.P, (unsigned)p.S), dim3(cpc::MT_THREADS), 0, st, x, ld,
                       seq_stride, s, skip, d, n, p.rows_per, p.T, partial, psums);
    CPC_CHECK_LAUNCH("seq_moments_partial_kernel");
    const unsigned blocks = (unsigned)(2 * p.P * (cpc::MT_T * cpc::MT_T / cpc::MT_THREADS) + cpc::cdiv(d, cpc::MT_THREADS));
    hipLaunchKernelGGL(cpc::moment_reduce_kernel, dim3(blocks), dim3(cpc::MT_THREADS), 0, st, partial, psums, p.S, p.T, p.P, d, 2,
                       s - skip > 1 ? 1 : 0, gram, dgram, sums);
    CPC_CHECK_LAUNCH("moment_reduce_kernel");
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
