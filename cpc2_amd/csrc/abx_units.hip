// ABX on quantized units: batched DTW between sequences of unit ids (cpc/eval/eval_ABX_clustering.py of the reference, which
// expands every frame to a one-hot row and runs the dense DTW).  On one-hot frames the frame distance takes two values,
// d_same (equal units) and d_diff, so there is no distance tile, no LDS and no workgroup barrier.  The recurrence is that of
// cpc_abx_dtw (abx_rule.h, the same copy: addition order d + predecessor, ties diag, left, up) and the walk that of
// dtw_units_walk.h: one wave per (x, y) pair.  DESIGN.md section 7.1 has the exactness argument, section 29 the walk.
//
//   abx_dtw_units_kernel   one workgroup per x item (a "segment"); its four waves take the segment's y items round robin.
#include "common.h"
#include "abx_rule.h"
#include "dtw_units_walk.h"

namespace cpc {
namespace {

__global__ void __launch_bounds__(DTWU_THREADS)
abx_dtw_units_kernel(const int *__restrict__ units, const int *__restrict__ item_off, const int *__restrict__ item_len,
                     int n_items, const int *__restrict__ seg_x, const int *__restrict__ seg_start,
                     const int *__restrict__ pair_y, int n_seg, int max_len_y, float d_same, float d_diff,
                     float *__restrict__ out, int *__restrict__ path_len, char *scratch)
{
    const int lane = threadIdx.x & 63;
    // the wave's index as a scalar: everything below that depends on the pair (lengths, loop bounds) is then wave-uniform
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const DtwWaveBoundary<ABX_W> bnd(scratch, wave, max_len_y);
    for (int seg = blockIdx.x; seg < n_seg; seg += gridDim.x) {
        const DtwItem x = dtw_item(item_off, item_len, n_items, seg_x[seg]);
        const int p_end = seg_start[seg + 1];
        for (int p = seg_start[seg] + wave; p < p_end; p += DTWU_WAVES) {
            const DtwItem y = dtw_item(item_off, item_len, n_items, pair_y[p]);
            // a one-strip x touches no boundary row: it is computed against a y of any length, with or without scratch
            if (x.len < 1 || y.len < 1 || (x.len > DTWU_T && (scratch == nullptr || y.len > max_len_y))) {
                if (lane == 0) {                                 // not computable: NaN never compares < or ==
                    out[p] = __builtin_nanf("");
                    if (path_len) path_len[p] = -1;
                }
                continue;
            }
            AbxRule rule;
            const AbxCell last = dtw_units_walk_pair(bnd, units, x.off, x.len, y.off, y.len, d_same, d_diff, rule);
            if (lane == (x.len - 1) % DTWU_T) {                  // the last row's lane: its newest cell is (lx-1, ly-1)
                out[p] = last.v / (float)last.n[DTW_LEN];
                if (path_len) path_len[p] = last.n[DTW_LEN];
            }
        }
    }
}

}  // namespace
}  // namespace cpc

// The grid cap of the dense kernels (dtw_units_walk.h says why it is not DTWU_MAX_BLOCKS).
extern "C" size_t cpc_abx_dtw_units_scratch_bytes(int n_seg, int max_len_x, int max_len_y)
{
    return cpc::dtw_units_scratch_bytes("abx_dtw_units", n_seg, "max_len_x", max_len_x, "max_len_y", max_len_y, cpc::ABX_W,
                                        cpc::DTW_MAX_BLOCKS);
}

extern "C" int cpc_abx_dtw_units(const int *units, const int *item_off, const int *item_len, int n_items, const int *seg_x,
                                 const int *seg_start, const int *pair_y, int n_seg, int max_len_x, int max_len_y,
                                 float d_same, float d_diff, float *out, int *path_len, void *scratch,
                                 size_t scratch_bytes, cpc_stream_t stream)
{
    CPC_TRY(cpc::dtw_units_check_args("abx_dtw_units",
                                      units != nullptr && item_off != nullptr && item_len != nullptr && seg_x != nullptr &&
                                          seg_start != nullptr && pair_y != nullptr && out != nullptr,
                                      d_same, d_diff, n_items, n_seg, "max_len_x", max_len_x, "max_len_y", max_len_y));
    const size_t need = cpc_abx_dtw_units_scratch_bytes(n_seg, max_len_x, max_len_y);
    CPC_REQUIRE(scratch_bytes >= need && (need == 0 || scratch != nullptr), "abx_dtw_units: scratch of %zu bytes, %zu needed",
                scratch_bytes, need);
    if (n_seg == 0) return CPC_OK;
    hipLaunchKernelGGL(cpc::abx_dtw_units_kernel, dim3((unsigned)cpc::dtw_units_grid(n_seg, cpc::DTW_MAX_BLOCKS)),
                       dim3(cpc::DTWU_THREADS), 0, static_cast<hipStream_t>(stream), units, item_off, item_len, n_items, seg_x,
                       seg_start, pair_y, n_seg, max_len_y, d_same, d_diff, out, path_len,
                       need ? static_cast<char *>(scratch) : nullptr);
    CPC_CHECK_LAUNCH("abx_dtw_units_kernel");
    return CPC_OK;
}
