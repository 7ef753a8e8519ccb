// Spoken term discovery on quantized units: batched LOCAL-ALIGNMENT DTW of a row item against column items whose frames are unit
// ids (cpc2_hip.h).  The recurrence is that of cpc_local_align (lalign_rule.h, the same copy) and the walk
// that of dtw_units_walk.h: one wave per (row item, column item) pair, no distance tile, no LDS, no barrier, no atomics.
//
//   lalign_units_kernel   one workgroup per segment (a row item and a list of column items); its four waves take the segment's
//                         column items round robin.
#include "common.h"
#include "dtw_units_walk.h"
#include "lalign_rule.h"

#include <cmath>

namespace cpc {
namespace {

// 8 waves per SIMD, which the grid cap of dtw_units_walk.h counts on: 64 VGPRs (68 and 7 waves without the attribute), no scratch
__global__ void __launch_bounds__(DTWU_THREADS) __attribute__((amdgpu_waves_per_eu(8, 8)))
lalign_units_kernel(const int *__restrict__ units, const int *__restrict__ item_off, const int *__restrict__ item_len, int n_items,
                    const int *__restrict__ seg_a, const int *__restrict__ seg_start, const int *__restrict__ pair_b, int n_seg,
                    int max_len_a, int max_len_b, float d_same, float d_diff, float theta, float gamma, float *__restrict__ score,
                    int *__restrict__ span, char *scratch)
{
    const int lane = threadIdx.x & 63;
    // the wave's index as a scalar: everything below that depends on the pair (lengths, loop bounds) is then wave-uniform
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const DtwWaveBoundary<LA_W> bnd(scratch, wave, max_len_b);
    for (int seg = blockIdx.x; seg < n_seg; seg += gridDim.x) {
        const DtwItem a = dtw_item(item_off, item_len, n_items, seg_a[seg]);
        const int p_end = seg_start[seg + 1];
        for (int p = seg_start[seg] + wave; p < p_end; p += DTWU_WAVES) {
            const DtwItem b = dtw_item(item_off, item_len, n_items, pair_b[p]);
            // a.len > 64 implies max_len_a > 64, for which the host insists on the scratch; b.len <= max_len_b fits a boundary row
            if (a.len < 1 || b.len < 1 || a.len > max_len_a || b.len > max_len_b) {
                if (lane == 0) {                                 // not computable
                    score[p] = __builtin_nanf("");
                    for (int k = 0; k < 5; ++k) span[5 * (long)p + k] = -1;
                }
                continue;
            }
            LaRule rule{theta, gamma};
            dtw_units_walk_pair(bnd, units, a.off, a.len, b.off, b.len, d_same, d_diff, rule);
            if (lane == 0) {                                     // the pair's best is the same in every lane
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

extern "C" size_t cpc_local_align_units_scratch_bytes(int n_seg, int max_len_a, int max_len_b)
{
    return cpc::dtw_units_scratch_bytes("local_align_units", n_seg, "max_len_a", max_len_a, "max_len_b", max_len_b, cpc::LA_W,
                                        cpc::DTWU_MAX_BLOCKS);
}

extern "C" int cpc_local_align_units(const int *units, const int *item_off, const int *item_len, int n_items, const int *seg_a,
                                     const int *seg_start, const int *pair_b, int n_seg, int max_len_a, int max_len_b, float d_same,
                                     float d_diff, float theta, float gamma, float *score, int *span, void *scratch,
                                     size_t scratch_bytes, cpc_stream_t stream)
{
    CPC_TRY(cpc::dtw_units_check_args("local_align_units",
                                      units != nullptr && item_off != nullptr && item_len != nullptr && seg_a != nullptr &&
                                          seg_start != nullptr && pair_b != nullptr && score != nullptr && span != nullptr,
                                      d_same, d_diff, n_items, n_seg, "max_len_a", max_len_a, "max_len_b", max_len_b));
    CPC_REQUIRE(max_len_a <= cpc::LA_MAX_FRAMES && max_len_b <= cpc::LA_MAX_FRAMES,
                "local_align_units: items have at most %d frames (max_len_a=%d max_len_b=%d)", cpc::LA_MAX_FRAMES, max_len_a,
                max_len_b);
    CPC_REQUIRE(std::isfinite(theta) && theta > 0.f, "local_align_units: the threshold theta=%g must be finite and > 0", (double)theta);
    CPC_REQUIRE(std::isfinite(gamma) && gamma >= 0.f, "local_align_units: the step penalty gamma=%g must be finite and >= 0",
                (double)gamma);
    const size_t need = cpc_local_align_units_scratch_bytes(n_seg, max_len_a, max_len_b);
    if (scratch_bytes < need || (need != 0 && scratch == nullptr)) {
        cpc::set_error("local_align_units: scratch of %zu bytes, cpc_local_align_units_scratch_bytes(%d, %d, %d) = %zu",
                       scratch ? scratch_bytes : (size_t)0, n_seg, max_len_a, max_len_b, need);
        return CPC_ERR_WORKSPACE;
    }
    if (n_seg == 0) return CPC_OK;
    hipLaunchKernelGGL(cpc::lalign_units_kernel, dim3((unsigned)cpc::dtw_units_grid(n_seg, cpc::DTWU_MAX_BLOCKS)),
                       dim3(cpc::DTWU_THREADS), 0, static_cast<hipStream_t>(stream), units, item_off, item_len, n_items, seg_a,
                       seg_start, pair_b, n_seg, max_len_a, max_len_b, d_same, d_diff, theta, gamma, score, span,
                       need ? static_cast<char *>(scratch) : nullptr);
    CPC_CHECK_LAUNCH("lalign_units_kernel");
    return CPC_OK;
}
