// Spoken term discovery: batched LOCAL-ALIGNMENT DTW of a row item against column items, both ends free on both sides
// (cpc2_hip.h).  The walk is that of dtw_strip.h and the distance tile that of dist_tile.h; what is this
// file's: a cell holds a GAIN H >= 0 that a path collects (theta - d per cell, gamma per horizontal or vertical step), a path
// opens wherever no predecessor is worth continuing, and the best cell of the whole matrix is the result.
//
//   lalign_kernel  one workgroup per segment (a row item and a list of column items).  A cell is (H, length, start) with the two
//                  start indices in one word (items have at most 32767 frames); a closed cell is H = 0 and carries nothing.
//                  Every lane keeps the best cell of its own row (strict >: the first column among equals); at the end of a
//                  strip the lanes are reduced to (largest H, smallest row) and the result replaces the pair's best on a strict
//                  > only, so the answer is (largest H, smallest i, smallest j) however strips and tiles are walked.
//                  No cost matrix, no backtrack, no atomics.
#include "common.h"
#include "dist_tile.h"

#include <cmath>

namespace cpc {
namespace {

constexpr int LA_W = 3;                // (H, length, start): 12 bytes per boundary-row column
constexpr int LA_MAX_FRAMES = 32767;   // start_i and start_j share one word: 15 bits each
using LaCell = DtwCell<LA_W>;

struct LaRule {
    float theta, gamma;
    float best_h = 0.f;                // the best cell of this lane's row so far: a closed cell cannot win
    int best_j = -1, best_l = -1, best_s = -1;
    float pair_h = 0.f;                // the same in every lane: the pair's best so far
    int pair_i = -1, pair_j = -1, pair_l = -1, pair_s = -1;

    __device__ __forceinline__ LaCell cell(int gi, int gj, float d, const LaCell &diag, const LaCell &left, const LaCell &up) const
    {
        const float g = theta - d;
        // candidates: diag, left - gamma, up - gamma; one that does not exist cannot be continued
        const float cd = (gi > 0 && gj > 0) ? diag.v : -INFINITY;
        const float cl = gj > 0 ? left.v - gamma : -INFINITY;
        const float cu = gi > 0 ? up.v - gamma : -INFINITY;
        const bool take_d = cd >= cl && cd >= cu, take_l = cl >= cu;     // the largest; ties: diag, then left, then up
        const float b_h = take_d ? cd : take_l ? cl : cu;
        const LaCell b = dtw_pick(take_d, diag, dtw_pick(take_l, left, up));
        // nothing worth continuing: the cell opens a path
        const LaCell c = dtw_pick(b_h <= 0.f, LaCell{g, {1, (gi << 16) | gj}}, LaCell{g + b_h, {b.n[DTW_LEN] + 1, b.n[DTW_START]}});
        return dtw_pick(c.v > 0.f, c, LaCell{});         // closed (also by a NaN distance): carries nothing
    }
    __device__ __forceinline__ void visit(int, int gj, const LaCell &c)
    {
        if (c.v > best_h) {            // strict: the first column among equals (a closed cell is 0 and never wins)
            best_h = c.v;
            best_j = gj;
            best_l = c.n[DTW_LEN];
            best_s = c.n[DTW_START];
        }
    }
    // (largest H, smallest row) over the lanes of the strip; the lanes' bests start afresh for the next strip
    __device__ __forceinline__ void strip_done(int rs, int, bool)
    {
        float m = best_h;
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        const int src = __ffsll((unsigned long long)__ballot(best_h == m)) - 1;
        const int w_j = __shfl(best_j, src), w_l = __shfl(best_l, src), w_s = __shfl(best_s, src);
        if (m > pair_h) {              // strict: the earlier strip wins ties
            pair_h = m;
            pair_i = rs + src;
            pair_j = w_j;
            pair_l = w_l;
            pair_s = w_s;
        }
        best_h = 0.f;
        best_j = best_l = best_s = -1;
    }
};

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
