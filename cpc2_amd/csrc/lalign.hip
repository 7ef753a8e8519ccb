// Spoken term discovery: batched LOCAL-ALIGNMENT DTW of a row item against column items, both ends free on both sides
// (cpc2_hip.h).  The walk is that of dtw_strip.h and the distance tile that of dist_tile.h; the recurrence
// is lalign_rule.h's, shared with lalign_units.hip: a cell holds a GAIN H >= 0 that a path collects (theta - d per cell, gamma
// per horizontal or vertical step), a path opens wherever no predecessor is worth continuing, and the best cell of the whole
// matrix is the result.
//
//   lalign_kernel  one workgroup per segment (a row item and a list of column items).  No cost matrix, no backtrack, no atomics.
#include "common.h"
#include "dist_tile.h"
#include "lalign_rule.h"

#include <cmath>

namespace cpc {
namespace {

__global__ void __launch_bounds__(DTW_THREADS)
lalign_kernel(const float *__restrict__ frames, int dp, const int *__restrict__ item_off, const int *__restrict__ item_len,
              int n_items, const int *__restrict__ seg_a, const int *__restrict__ seg_start, const int *__restrict__ pair_b,
              int n_seg, int max_len_a, int max_len_b, int euclid, float theta, float gamma, float *__restrict__ score,
              int *__restrict__ span, char *scratch)
{
    __shared__ __attribute__((aligned(16))) float xs[SD_KC][SD_LS];      // row frames of the strip, [k][row]
    __shared__ __attribute__((aligned(16))) float ys[SD_KC][SD_LS];      // column frames of the tile, [k][column]
    __shared__ float dt[DTW_T][DTW_DT_STRIDE];

    const int tid = threadIdx.x;
    const DtwBoundary<LA_W> bnd(scratch, max_len_b);
    for (int seg = blockIdx.x; seg < n_seg; seg += gridDim.x) {
        const DtwItem a = dtw_item(item_off, item_len, n_items, seg_a[seg]);
        for (int p = seg_start[seg]; p < seg_start[seg + 1]; ++p) {
            const DtwItem b = dtw_item(item_off, item_len, n_items, pair_b[p]);
            // a.len > 64 implies max_len_a > 64, for which the host insists on the scratch; b.len <= max_len_b fits a boundary row
            if (a.len < 1 || b.len < 1 || a.len > max_len_a || b.len > max_len_b) {
                if (tid == 0) {                                  // not computable
                    score[p] = __builtin_nanf("");
                    for (int k = 0; k < 5; ++k) span[5 * (long)p + k] = -1;
                }
                continue;
            }
            LaRule rule{theta, gamma};
            dtw_walk_pair(bnd, a.len, b.len, dt, rule, [&](int rs, int R, int cb, int C) {
                sd_distance_tile(frames, dp, a.off + rs, R, b.off + cb, C, euclid, xs, ys, dt, rs, cb);
            });
            if (tid == 0) {
                const bool found = rule.pair_h > 0.f;
                score[p] = found ? rule.pair_h : 0.f;
                span[5 * (long)p] = found ? (rule.pair_s >> 16) : -1;
                span[5 * (long)p + 1] = found ? rule.pair_i : -1;
                span[5 * (long)p + 2] = found ? (rule.pair_s & 0xffff) : -1;
                span[5 * (long)p + 3] = found ? rule.pair_j : -1;
                span[5 * (long)p + 4] = found ? rule.pair_l : -1;
            }
        }
    }
}

}  // namespace
}  // namespace cpc

extern "C" size_t cpc_local_align_scratch_bytes(int n_seg, int max_len_a, int max_len_b)
{
    if (n_seg < 0 || max_len_a < 0 || max_len_b < 0) {
        cpc::set_error("local_align: negative size (n_seg=%d max_len_a=%d max_len_b=%d)", n_seg, max_len_a, max_len_b);
        return 0;
    }
    if (n_seg == 0 || max_len_b == 0) return 0;
    if (max_len_a <= cpc::DTW_T) return 0;                       // one strip per row item: no boundary row is stored
    return cpc::dtw_boundary_bytes(n_seg, max_len_b, cpc::LA_W);
}

extern "C" int cpc_local_align(const float *frames, int dp, const int *item_off, const int *item_len, int n_items, const int *seg_a,
                               const int *seg_start, const int *pair_b, int n_seg, int max_len_a, int max_len_b, int distance,
                               float theta, float gamma, float *score, int *span, void *scratch, size_t scratch_bytes,
                               cpc_stream_t stream)
{
    CPC_TRY(cpc::dtw_check_args("local_align",
                                frames != nullptr && item_off != nullptr && item_len != nullptr && seg_a != nullptr &&
                                    seg_start != nullptr && pair_b != nullptr && score != nullptr && span != nullptr,
                                dp, distance, n_items, n_seg, "max_len_a", max_len_a, "max_len_b", max_len_b));
    CPC_REQUIRE(max_len_a <= cpc::LA_MAX_FRAMES && max_len_b <= cpc::LA_MAX_FRAMES,
                "local_align: items have at most %d frames (max_len_a=%d max_len_b=%d)", cpc::LA_MAX_FRAMES, max_len_a, max_len_b);
    CPC_REQUIRE(std::isfinite(theta) && theta > 0.f, "local_align: the threshold theta=%g must be finite and > 0", (double)theta);
    CPC_REQUIRE(std::isfinite(gamma) && gamma >= 0.f, "local_align: the step penalty gamma=%g must be finite and >= 0", (double)gamma);
    const size_t need = cpc_local_align_scratch_bytes(n_seg, max_len_a, max_len_b);
    if (scratch_bytes < need || (need != 0 && scratch == nullptr)) {
        cpc::set_error("local_align: scratch of %zu bytes, cpc_local_align_scratch_bytes(%d, %d, %d) = %zu",
                       scratch ? scratch_bytes : (size_t)0, n_seg, max_len_a, max_len_b, need);
        return CPC_ERR_WORKSPACE;
    }
    if (n_seg == 0) return CPC_OK;
    hipLaunchKernelGGL(cpc::lalign_kernel, dim3((unsigned)cpc::dtw_grid(n_seg)), dim3(cpc::DTW_THREADS), 0,
                       static_cast<hipStream_t>(stream), frames, dp, item_off, item_len, n_items, seg_a, seg_start, pair_b, n_seg,
                       max_len_a, max_len_b, distance == CPC_ABX_EUCLIDIAN ? 1 : 0, theta, gamma, score, span,
                       need ? static_cast<char *>(scratch) : nullptr);
    CPC_CHECK_LAUNCH("lalign_kernel");
    return CPC_OK;
}
