// Query-by-example term detection: batched SUBSEQUENCE DTW of a query item inside document items (cpc2_hip.h, DESIGN.md
// section 26).  The work-list layout, the frame distances and the strip / boundary-row scheme are those of abx.hip; the
// recurrence differs (free start on row 0, every cell carries (cost, length, start), the best end column of the last query
// row is kept while the columns stream), and the distance tile is register-blocked: a QbE run spends its time there.
//
//   sdtw_kernel   one workgroup per segment (a query item and a list of document items).  Per pair the n x m frame-distance
//                 matrix is formed 64 x 64 tile by tile in LDS by dist_tile.h (shared with lalign.hip): each thread owns a
//                 4 x 4 block of the tile; every entry is its own k-ordered f32 fma chain.  The DP runs over the tile on
//                 the anti-diagonal in wave 0 with lane = query row (DPP wave_shr:1 hands a cell to the row below).
//                 Queries longer than 64 frames go in
//                 64-row strips whose boundary row (cost, length, start: 12 bytes per document column) lives in
//                 per-workgroup scratch, double-buffered.  The lane of the last query row keeps the running best
//                 (v, end, start, length) in registers: no cost matrix, no backtrack, no atomics.
#include "common.h"
#include "dist_tile.h"

#include <algorithm>

namespace cpc {
namespace {

constexpr int SD_MAX_BLOCKS = 8192;
constexpr int SD_CELL_BYTES = 12;  // (cost, length, start) of a boundary-row column

__global__ void __launch_bounds__(SD_THREADS)
sdtw_kernel(const float *__restrict__ frames, int dp, const int *__restrict__ item_off, const int *__restrict__ item_len,
            int n_items, const int *__restrict__ seg_q, const int *__restrict__ seg_start, const int *__restrict__ pair_doc,
            int n_seg, int max_len_doc, int euclid, float *__restrict__ score, int *__restrict__ span, char *scratch)
{
    __shared__ __attribute__((aligned(16))) float xs[SD_KC][SD_LS];      // query frames of the strip, [k][row]
    __shared__ __attribute__((aligned(16))) float ys[SD_KC][SD_LS];      // document frames of the tile, [k][column]
    __shared__ float dt[SD_T][SD_DT_STRIDE];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const bool dp_wave = tid < 64;
    // boundary rows of this workgroup: two (cost, length, start) rows of max_len_doc, swapped per strip
    float *bc[2];
    int *bl[2], *bs[2];
    {
        char *base = scratch ? scratch + (size_t)blockIdx.x * 2 * (size_t)max_len_doc * SD_CELL_BYTES : nullptr;
        for (int b = 0; b < 2; ++b) {
            char *row = base + (size_t)b * (size_t)max_len_doc * SD_CELL_BYTES;
            bc[b] = reinterpret_cast<float *>(row);
            bl[b] = reinterpret_cast<int *>(row + (size_t)max_len_doc * 4);
            bs[b] = reinterpret_cast<int *>(row + (size_t)max_len_doc * 8);
        }
    }

    for (int seg = blockIdx.x; seg < n_seg; seg += gridDim.x) {
        const int qi = seg_q[seg];
        const bool q_ok = qi >= 0 && qi < n_items;
        const int lq = q_ok ? item_len[qi] : 0;
        const long qo = q_ok ? (long)item_off[qi] : 0;
        for (int p = seg_start[seg]; p < seg_start[seg + 1]; ++p) {
            const int di = pair_doc[p];
            const bool d_ok = di >= 0 && di < n_items;
            const int ld = d_ok ? item_len[di] : 0;
            const long dof = d_ok ? (long)item_off[di] : 0;
            if (lq < 1 || ld < 1 || (lq > SD_T && (scratch == nullptr || ld > max_len_doc))) {
                if (tid == 0) {                                  // not computable
                    score[p] = __builtin_nanf("");
                    span[3 * (long)p] = -1;
                    span[3 * (long)p + 1] = -1;
                    span[3 * (long)p + 2] = -1;
                }
                continue;
            }
            int cur = 0;                                         // boundary buffer read by this strip
            for (int rs = 0; rs < lq; rs += SD_T) {
                const int R = min(SD_T, lq - rs);
                const bool more_strips = rs + SD_T < lq;
                float cur_c = 0.f;                               // DP wave: this lane's newest cell in its row
                int cur_l = 0, cur_s = 0;
                float pup_c = 0.f;                               // the up value of the previous step (= this step's diag)
                int pup_l = 0, pup_s = 0;
                float best_v = 0.f;                              // lane of the last query row: the best end column so far
                int best_j = 0, best_l = 0, best_s = 0;
                for (int cb = 0; cb < ld; cb += SD_T) {
                    const int C = min(SD_T, ld - cb);
                    // ---- distance tile (dist_tile.h): a 4 x 4 block per thread, k-ordered fma chain per entry ----
                    sd_distance_tile(frames, dp, qo + rs, R, dof + cb, C, euclid, xs, ys, dt, rs, cb);
                    // ---- DP over the tile: wave 0, lane = query row, step t = anti-diagonal ----
                    if (dp_wave) {
                        const int r = lane;
                        const int gi = rs + r;
                        const float *in_c = bc[cur];
                        const int *in_l = bl[cur], *in_s = bs[cur];
                        float *out_c = bc[cur ^ 1];
                        int *out_l = bl[cur ^ 1], *out_s = bs[cur ^ 1];
                        for (int t = 0; t < R + C - 1; ++t) {
                            const int c = t - r;
                            float up_c = sd_shr1(cur_c, 0.f);    // lane r-1's newest cell: (r-1, c)
                            int up_l = sd_shr1(cur_l, 0);
                            int up_s = sd_shr1(cur_s, 0);
                            if (r < R && c >= 0 && c < C) {
                                const int gj = cb + c;
                                const float d = dt[r][c];
                                float dg_c = pup_c;
                                int dg_l = pup_l, dg_s = pup_s;
                                if (r == 0 && rs > 0) {          // the row above is the previous strip's last row
                                    up_c = in_c[gj];
                                    up_l = in_l[gj];
                                    up_s = in_s[gj];
                                    if (gj > 0) {
                                        dg_c = in_c[gj - 1];
                                        dg_l = in_l[gj - 1];
                                        dg_s = in_s[gj - 1];
                                    }
                                }
                                float nc;
                                int nl, ns;
                                if (gi == 0) {                   // free start: no predecessor on the first query row
                                    nc = d;
                                    nl = 1;
                                    ns = gj;
                                } else if (gj == 0) {
                                    nc = d + up_c;
                                    nl = up_l + 1;
                                    ns = up_s;
                                } else if (dg_c <= cur_c && dg_c <= up_c) {   // ties: diag, then left, then up
                                    nc = d + dg_c;
                                    nl = dg_l + 1;
                                    ns = dg_s;
                                } else if (cur_c <= up_c) {
                                    nc = d + cur_c;
                                    nl = cur_l + 1;
                                    ns = cur_s;
                                } else {
                                    nc = d + up_c;
                                    nl = up_l + 1;
                                    ns = up_s;
                                }
                                cur_c = nc;
                                cur_l = nl;
                                cur_s = ns;
                                if (r == R - 1) {
                                    if (more_strips) {
                                        out_c[gj] = nc;
                                        out_l[gj] = nl;
                                        out_s[gj] = ns;
                                    } else {                     // the last query row: v[j], the first smallest wins
                                        const float v = nc / (float)nl;
                                        if (gj == 0 || v < best_v) {
                                            best_v = v;
                                            best_j = gj;
                                            best_l = nl;
                                            best_s = ns;
                                        }
                                    }
                                }
                            }
                            pup_c = up_c;
                            pup_l = up_l;
                            pup_s = up_s;
                        }
                    }
                }
                if (dp_wave && !more_strips && lane == R - 1) {
                    score[p] = best_v;
                    span[3 * (long)p] = best_s;
                    span[3 * (long)p + 1] = best_j;
                    span[3 * (long)p + 2] = best_l;
                }
                cur ^= 1;
                __threadfence_block();                           // boundary row visible to the next strip's lane 0
            }
        }
    }
}

int sdtw_grid(int n) { return std::min(n, SD_MAX_BLOCKS); }

}  // namespace
}  // namespace cpc

extern "C" size_t cpc_sdtw_scratch_bytes(int n_seg, int max_len_q, int max_len_doc)
{
    if (n_seg < 0 || max_len_q < 0 || max_len_doc < 0) {
        cpc::set_error("sdtw: negative size (n_seg=%d max_len_q=%d max_len_doc=%d)", n_seg, max_len_q, max_len_doc);
        return 0;
    }
    if (n_seg == 0 || max_len_doc == 0) return 0;
    if (max_len_q <= cpc::SD_T) return 0;                        // one strip per query: no boundary row is stored
    return (size_t)cpc::sdtw_grid(n_seg) * 2 * (size_t)max_len_doc * cpc::SD_CELL_BYTES;
}

extern "C" int cpc_sdtw(const float *frames, int dp, const int *item_off, const int *item_len, int n_items, const int *seg_q,
                        const int *seg_start, const int *pair_doc, int n_seg, int max_len_q, int max_len_doc, int distance,
                        float *score, int *span, void *scratch, size_t scratch_bytes, cpc_stream_t stream)
{
    CPC_REQUIRE(frames != nullptr && item_off != nullptr && item_len != nullptr && seg_q != nullptr && seg_start != nullptr &&
                    pair_doc != nullptr && score != nullptr && span != nullptr,
                "sdtw: null buffer");
    CPC_REQUIRE(dp >= 4 && dp % 4 == 0, "sdtw: the frame stride dp=%d must be a positive multiple of 4", dp);
    CPC_REQUIRE(distance == CPC_ABX_COSINE || distance == CPC_ABX_EUCLIDIAN, "sdtw: unknown distance %d", distance);
    CPC_REQUIRE(n_items > 0 && n_seg >= 0 && max_len_q >= 1 && max_len_doc >= 1,
                "sdtw: bad sizes (n_items=%d n_seg=%d max_len_q=%d max_len_doc=%d)", n_items, n_seg, max_len_q, max_len_doc);
    const size_t need = cpc_sdtw_scratch_bytes(n_seg, max_len_q, max_len_doc);
    CPC_REQUIRE(scratch_bytes >= need && (need == 0 || scratch != nullptr), "sdtw: scratch of %zu bytes, %zu needed",
                scratch_bytes, need);
    if (n_seg == 0) return CPC_OK;
    hipLaunchKernelGGL(cpc::sdtw_kernel, dim3((unsigned)cpc::sdtw_grid(n_seg)), dim3(cpc::SD_THREADS), 0,
                       static_cast<hipStream_t>(stream), frames, dp, item_off, item_len, n_items, seg_q, seg_start, pair_doc,
                       n_seg, max_len_doc, distance == CPC_ABX_EUCLIDIAN ? 1 : 0, score, span,
                       need ? static_cast<char *>(scratch) : nullptr);
    CPC_CHECK_LAUNCH("sdtw_kernel");
    return CPC_OK;
}
