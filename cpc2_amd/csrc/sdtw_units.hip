// Query-by-example term detection on quantized units: batched SUBSEQUENCE DTW of a query item inside document items whose frames
// are unit ids (cpc2_hip.h).  The recurrence is that of cpc_sdtw (sdtw_rule.h, the same copy) and the walk
// that of dtw_units_walk.h: one wave per (query, document) pair, no distance tile, no LDS, no barrier, no atomics.
//
//   sdtw_units_kernel   one workgroup per segment (a query item and a list of document items); its four waves take the
//                       segment's documents round robin.
#include "common.h"
#include "dtw_units_walk.h"
#include "sdtw_rule.h"

namespace cpc {
namespace {

__global__ void __launch_bounds__(DTWU_THREADS)
sdtw_units_kernel(const int *__restrict__ units, const int *__restrict__ item_off, const int *__restrict__ item_len, int n_items,
                  const int *__restrict__ seg_q, const int *__restrict__ seg_start, const int *__restrict__ pair_doc, int n_seg,
                  int max_len_q, int max_len_doc, float d_same, float d_diff, float *__restrict__ score, int *__restrict__ span,
                  char *scratch)
{
    const int lane = threadIdx.x & 63;
    // the wave's index as a scalar: everything below that depends on the pair (lengths, loop bounds) is then wave-uniform
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const DtwWaveBoundary<SD_W> bnd(scratch, wave, max_len_doc);
    for (int seg = blockIdx.x; seg < n_seg; seg += gridDim.x) {
        const DtwItem q = dtw_item(item_off, item_len, n_items, seg_q[seg]);
        const int p_end = seg_start[seg + 1];
        for (int p = seg_start[seg] + wave; p < p_end; p += DTWU_WAVES) {
            const DtwItem doc = dtw_item(item_off, item_len, n_items, pair_doc[p]);
            // q.len > 64 implies max_len_q > 64, for which the host insists on the scratch; doc.len <= max_len_doc fits a boundary row
            if (q.len < 1 || doc.len < 1 || q.len > max_len_q || doc.len > max_len_doc) {
                if (lane == 0) {                                 // not computable
                    score[p] = __builtin_nanf("");
                    span[3 * (long)p] = -1;
                    span[3 * (long)p + 1] = -1;
                    span[3 * (long)p + 2] = -1;
                }
                continue;
            }
            SdRule rule{q.len};
            dtw_units_walk_pair(bnd, units, q.off, q.len, doc.off, doc.len, d_same, d_diff, rule);
            if (lane == (q.len - 1) % DTWU_T) {                  // the last query row's lane
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

extern "C" size_t cpc_sdtw_units_scratch_bytes(int n_seg, int max_len_q, int max_len_doc)
{
    return cpc::dtw_units_scratch_bytes("sdtw_units", n_seg, "max_len_q", max_len_q, "max_len_doc", max_len_doc, cpc::SD_W,
                                        cpc::DTWU_MAX_BLOCKS);
}

extern "C" int cpc_sdtw_units(const int *units, const int *item_off, const int *item_len, int n_items, const int *seg_q,
                              const int *seg_start, const int *pair_doc, int n_seg, int max_len_q, int max_len_doc, float d_same,
                              float d_diff, float *score, int *span, void *scratch, size_t scratch_bytes, cpc_stream_t stream)
{
    CPC_TRY(cpc::dtw_units_check_args("sdtw_units",
                                      units != nullptr && item_off != nullptr && item_len != nullptr && seg_q != nullptr &&
                                          seg_start != nullptr && pair_doc != nullptr && score != nullptr && span != nullptr,
                                      d_same, d_diff, n_items, n_seg, "max_len_q", max_len_q, "max_len_doc", max_len_doc));
    const size_t need = cpc_sdtw_units_scratch_bytes(n_seg, max_len_q, max_len_doc);
    CPC_REQUIRE(scratch_bytes >= need && (need == 0 || scratch != nullptr), "sdtw_units: scratch of %zu bytes, %zu needed",
                scratch_bytes, need);
    if (n_seg == 0) return CPC_OK;
    hipLaunchKernelGGL(cpc::sdtw_units_kernel, dim3((unsigned)cpc::dtw_units_grid(n_seg, cpc::DTWU_MAX_BLOCKS)),
                       dim3(cpc::DTWU_THREADS), 0, static_cast<hipStream_t>(stream), units, item_off, item_len, n_items, seg_q,
                       seg_start, pair_doc, n_seg, max_len_q, max_len_doc, d_same, d_diff, score, span,
                       need ? static_cast<char *>(scratch) : nullptr);
    CPC_CHECK_LAUNCH("sdtw_units_kernel");
    return CPC_OK;
}
