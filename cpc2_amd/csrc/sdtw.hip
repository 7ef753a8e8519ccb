// Query-by-example term detection: batched SUBSEQUENCE DTW of a query item inside document items (cpc2_hip.h, DESIGN.md
// section 26).  The walk is that of dtw_strip.h and the distance tile that of dist_tile.h (a QbE run spends its time there); what
// is sdtw_rule.h's, shared with sdtw_units.hip: the recurrence (free start on row 0, every cell carries (cost, length, start)) and the
// best end column of the last query row, kept in that row's lane while the columns stream: no cost matrix, no backtrack, no atomics.
//
//   sdtw_kernel   one workgroup per segment (a query item and a list of document items).
#include "common.h"
#include "dist_tile.h"
#include "sdtw_rule.h"

namespace cpc {
namespace {

__global__ void __launch_bounds__(DTW_THREADS)
sdtw_kernel(const float *__restrict__ frames, int dp, const int *__restrict__ item_off, const int *__restrict__ item_len,
            int n_items, const int *__restrict__ seg_q, const int *__restrict__ seg_start, const int *__restrict__ pair_doc,
            int n_seg, int max_len_doc, int euclid, float *__restrict__ score, int *__restrict__ span, char *scratch)
{
    __shared__ __attribute__((aligned(16))) float xs[SD_KC][SD_LS];      // query frames of the strip, [k][row]
    __shared__ __attribute__((aligned(16))) float ys[SD_KC][SD_LS];      // document frames of the tile, [k][column]
    __shared__ float dt[DTW_T][DTW_DT_STRIDE];

    const int tid = threadIdx.x;
    const DtwBoundary<SD_W> bnd(scratch, max_len_doc);
    for (int seg = blockIdx.x; seg < n_seg; seg += gridDim.x) {
        const DtwItem q = dtw_item(item_off, item_len, n_items, seg_q[seg]);
        for (int p = seg_start[seg]; p < seg_start[seg + 1]; ++p) {
            const DtwItem doc = dtw_item(item_off, item_len, n_items, pair_doc[p]);
            if (q.len < 1 || doc.len < 1 || (q.len > DTW_T && (scratch == nullptr || doc.len > max_len_doc))) {
                if (tid == 0) {                                  // not computable
                    score[p] = __builtin_nanf("");
                    span[3 * (long)p] = -1;
                    span[3 * (long)p + 1] = -1;
                    span[3 * (long)p + 2] = -1;
                }
                continue;
            }
            SdRule rule{q.len};
            dtw_walk_pair(bnd, q.len, doc.len, dt, rule, [&](int rs, int R, int cb, int C) {
                sd_distance_tile(frames, dp, q.off + rs, R, doc.off + cb, C, euclid, xs, ys, dt, rs, cb);
            });
            if (tid == (q.len - 1) % DTW_T) {                    // the last query row's lane of wave 0
                score[p] = rule.best_v;
                span[3 * (long)p] = rule.best_s;
                span[3 * (long)p + 1] = rule.best_j;
                span[3 * (long)p + 2] = rule.best_l;
            }
        }
    }
}

}  // namespace
}  // namespace cpc

extern "C" size_t cpc_sdtw_scratch_bytes(int n_seg, int max_len_q, int max_len_doc)
{
    if (n_seg < 0 || max_len_q < 0 || max_len_doc < 0) {
        cpc::set_error("sdtw: negative size (n_seg=%d max_len_q=%d max_len_doc=%d)", n_seg, max_len_q, max_len_doc);
        return 0;
    }
    if (n_seg == 0 || max_len_doc == 0) return 0;
    if (max_len_q <= cpc::DTW_T) return 0;                       // one strip per query: no boundary row is stored
    return cpc::dtw_boundary_bytes(n_seg, max_len_doc, cpc::SD_W);
}

extern "C" int cpc_sdtw(const float *frames, int dp, const int *item_off, const int *item_len, int n_items, const int *seg_q,
                        const int *seg_start, const int *pair_doc, int n_seg, int max_len_q, int max_len_doc, int distance,
                        float *score, int *span, void *scratch, size_t scratch_bytes, cpc_stream_t stream)
{
    CPC_TRY(cpc::dtw_check_args("sdtw",
                                frames != nullptr && item_off != nullptr && item_len != nullptr && seg_q != nullptr &&
                                    seg_start != nullptr && pair_doc != nullptr && score != nullptr && span != nullptr,
                                dp, distance, n_items, n_seg, "max_len_q", max_len_q, "max_len_doc", max_len_doc));
    const size_t need = cpc_sdtw_scratch_bytes(n_seg, max_len_q, max_len_doc);
    CPC_REQUIRE(scratch_bytes >= need && (need == 0 || scratch != nullptr), "sdtw: scratch of %zu bytes, %zu needed",
                scratch_bytes, need);
    if (n_seg == 0) return CPC_OK;
    hipLaunchKernelGGL(cpc::sdtw_kernel, dim3((unsigned)cpc::dtw_grid(n_seg)), dim3(cpc::DTW_THREADS), 0,
                       static_cast<hipStream_t>(stream), frames, dp, item_off, item_len, n_items, seg_q, seg_start, pair_doc,
                       n_seg, max_len_doc, distance == CPC_ABX_EUCLIDIAN ? 1 : 0, score, span,
                       need ? static_cast<char *>(scratch) : nullptr);
    CPC_CHECK_LAUNCH("sdtw_kernel");
    return CPC_OK;
}
