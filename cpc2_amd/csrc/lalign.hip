// Spoken term discovery: batched LOCAL-ALIGNMENT DTW of a row item against column items, both ends free on both sides
// (cpc2_hip.h).  The work-list layout, the frame distances, the distance tile (dist_tile.h) and the
// strip / boundary-row scheme are those of sdtw.hip; the recurrence differs: a cell holds a GAIN H >= 0 that a path collects
// (theta - d per cell, gamma per horizontal or vertical step), a path opens wherever no predecessor is worth continuing, and
// the best cell of the whole matrix is the result, not the best end column of the last row.
//
//   lalign_kernel  one workgroup per segment (a row item and a list of column items).  Per pair the n x m distance matrix is
//                  formed 64 x 64 tile by tile in LDS; the DP runs over the tile on the anti-diagonal in wave 0 with lane = row
//                  of the strip (DPP wave_shr:1 hands a cell to the row below).  A cell is (H, length, start) with the two
//                  start indices in one word (items have at most 32767 frames); a closed cell is H = 0 and carries nothing.
//                  Every lane keeps the best cell of its own row (strict >: the first column among equals); at the end of a
//                  strip the lanes are reduced to (largest H, smallest row) and the result replaces the pair's best on a strict
//                  > only, so the answer is (largest H, smallest i, smallest j) however strips and tiles are walked.  Row items
//                  longer than 64 frames go in 64-row strips whose boundary row (12 bytes per column) lives in per-workgroup
//                  scratch, double-buffered, and is written before it is read.  No cost matrix, no backtrack, no atomics.
#include "common.h"
#include "dist_tile.h"

#include <algorithm>
#include <cmath>

namespace cpc {
namespace {

constexpr int LA_MAX_BLOCKS = 8192;
constexpr int LA_CELL_BYTES = 12;      // (H, length, start) of a boundary-row column
constexpr int LA_MAX_FRAMES = 32767;   // start_i and start_j share one word: 15 bits each

__global__ void __launch_bounds__(SD_THREADS)
lalign_kernel(const float *__restrict__ frames, int dp, const int *__restrict__ item_off, const int *__restrict__ item_len,
              int n_items, const int *__restrict__ seg_a, const int *__restrict__ seg_start, const int *__restrict__ pair_b,
              int n_seg, int max_len_a, int max_len_b, int euclid, float theta, float gamma, float *__restrict__ score,
              int *__restrict__ span, char *scratch)
{
    __shared__ __attribute__((aligned(16))) float xs[SD_KC][SD_LS];      // row frames of the strip, [k][row]
    __shared__ __attribute__((aligned(16))) float ys[SD_KC][SD_LS];      // column frames of the tile, [k][column]
    __shared__ float dt[SD_T][SD_DT_STRIDE];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const bool dp_wave = tid < 64;
    // boundary rows of this workgroup: two (H, length, start) rows of max_len_b, swapped per strip
    float *bh[2] = {nullptr, nullptr};
    int *bl[2] = {nullptr, nullptr}, *bs[2] = {nullptr, nullptr};
    if (scratch != nullptr) {
        char *base = scratch + (size_t)blockIdx.x * 2 * (size_t)max_len_b * LA_CELL_BYTES;
        for (int b = 0; b < 2; ++b) {
            char *row = base + (size_t)b * (size_t)max_len_b * LA_CELL_BYTES;
            bh[b] = reinterpret_cast<float *>(row);
            bl[b] = reinterpret_cast<int *>(row + (size_t)max_len_b * 4);
            bs[b] = reinterpret_cast<int *>(row + (size_t)max_len_b * 8);
        }
    }

    for (int seg = blockIdx.x; seg < n_seg; seg += gridDim.x) {
        const int ai = seg_a[seg];
        const bool a_ok = ai >= 0 && ai < n_items;
        const int la = a_ok ? item_len[ai] : 0;
        const long ao = a_ok ? (long)item_off[ai] : 0;
        for (int p = seg_start[seg]; p < seg_start[seg + 1]; ++p) {
            const int bi = pair_b[p];
            const bool b_ok = bi >= 0 && bi < n_items;
            const int lb = b_ok ? item_len[bi] : 0;
            const long bo = b_ok ? (long)item_off[bi] : 0;
            // la > 64 implies max_len_a > 64, for which the host insists on the scratch; lb <= max_len_b fits a boundary row
            if (la < 1 || lb < 1 || la > max_len_a || lb > max_len_b) {
                if (tid == 0) {                                  // not computable
                    score[p] = __builtin_nanf("");
                    for (int k = 0; k < 5; ++k) span[5 * (long)p + k] = -1;
                }
                continue;
            }
            int cur = 0;                                         // boundary buffer read by this strip
            float pair_h = 0.f;                                  // DP wave, the same in every lane: the pair's best so far
            int pair_i = -1, pair_j = -1, pair_l = -1, pair_s = -1;
            for (int rs = 0; rs < la; rs += SD_T) {
                const int R = min(SD_T, la - rs);
                const bool more_strips = rs + SD_T < la;
                float cur_h = 0.f;                               // DP wave: this lane's newest cell in its row
                int cur_l = 0, cur_s = 0;
                float pup_h = 0.f;                               // the up value of the previous step (= this step's diag)
                int pup_l = 0, pup_s = 0;
                float best_h = 0.f;                              // the best cell of this lane's row so far: a closed cell cannot win
                int best_j = -1, best_l = -1, best_s = -1;
                for (int cb = 0; cb < lb; cb += SD_T) {
                    const int C = min(SD_T, lb - cb);
                    // ---- distance tile (dist_tile.h): a 4 x 4 block per thread, k-ordered fma chain per entry ----
                    sd_distance_tile(frames, dp, ao + rs, R, bo + cb, C, euclid, xs, ys, dt, rs, cb);
                    // ---- DP over the tile: wave 0, lane = row of the strip, step t = anti-diagonal ----
                    if (dp_wave) {
                        const int r = lane;
                        const int gi = rs + r;
                        const float *in_h = bh[cur];
                        const int *in_l = bl[cur], *in_s = bs[cur];
                        float *out_h = bh[cur ^ 1];
                        int *out_l = bl[cur ^ 1], *out_s = bs[cur ^ 1];
                        for (int t = 0; t < R + C - 1; ++t) {
                            const int c = t - r;
                            float up_h = sd_shr1(cur_h, 0.f);    // lane r-1's newest cell: (r-1, c)
                            int up_l = sd_shr1(cur_l, 0);
                            int up_s = sd_shr1(cur_s, 0);
                            if (r < R && c >= 0 && c < C) {
                                const int gj = cb + c;
                                const float g = theta - dt[r][c];
                                float dg_h = pup_h;
                                int dg_l = pup_l, dg_s = pup_s;
                                if (r == 0 && rs > 0) {          // the row above is the previous strip's last row
                                    up_h = in_h[gj];
                                    up_l = in_l[gj];
                                    up_s = in_s[gj];
                                    if (gj > 0) {
                                        dg_h = in_h[gj - 1];
                                        dg_l = in_l[gj - 1];
                                        dg_s = in_s[gj - 1];
                                    }
                                }
                                // candidates: diag, left - gamma, up - gamma; one that does not exist cannot be continued
                                const float cd = (gi > 0 && gj > 0) ? dg_h : -INFINITY;
                                const float cl = gj > 0 ? cur_h - gamma : -INFINITY;
                                const float cu = gi > 0 ? up_h - gamma : -INFINITY;
                                float b_h;
                                int b_l, b_s;
                                if (cd >= cl && cd >= cu) {      // the largest; ties: diag, then left, then up
                                    b_h = cd;
                                    b_l = dg_l;
                                    b_s = dg_s;
                                } else if (cl >= cu) {
                                    b_h = cl;
                                    b_l = cur_l;
                                    b_s = cur_s;
                                } else {
                                    b_h = cu;
                                    b_l = up_l;
                                    b_s = up_s;
                                }
                                float h;
                                int nl, ns;
                                if (b_h <= 0.f) {                // nothing worth continuing: the cell opens a path
                                    h = g;
                                    nl = 1;
                                    ns = (gi << 16) | gj;
                                } else {
                                    h = g + b_h;
                                    nl = b_l + 1;
                                    ns = b_s;
                                }
                                if (h > 0.f) {
                                    cur_h = h;
                                    cur_l = nl;
                                    cur_s = ns;
                                    if (h > best_h) {            // strict: the first column among equals
                                        best_h = h;
                                        best_j = gj;
                                        best_l = nl;
                                        best_s = ns;
                                    }
                                } else {                         // closed (also by a NaN distance): carries nothing
                                    cur_h = 0.f;
                                    cur_l = 0;
                                    cur_s = 0;
                                }
                                if (more_strips && r == R - 1) {
                                    out_h[gj] = cur_h;
                                    out_l[gj] = cur_l;
                                    out_s[gj] = cur_s;
                                }
                            }
                            pup_h = up_h;
                            pup_l = up_l;
                            pup_s = up_s;
                        }
                    }
                }
                if (dp_wave) {                                   // (largest H, smallest row) over the lanes of the strip
                    float m = best_h;
                    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
                    const int src = __ffsll((unsigned long long)__ballot(best_h == m)) - 1;
                    const int w_j = __shfl(best_j, src), w_l = __shfl(best_l, src), w_s = __shfl(best_s, src);
                    if (m > pair_h) {                            // strict: the earlier strip wins ties
                        pair_h = m;
                        pair_i = rs + src;
                        pair_j = w_j;
                        pair_l = w_l;
                        pair_s = w_s;
                    }
                }
                cur ^= 1;
                __threadfence_block();                           // boundary row visible to the next strip's lane 0
            }
            if (tid == 0) {
                const bool found = pair_h > 0.f;
                score[p] = found ? pair_h : 0.f;
                span[5 * (long)p] = found ? (pair_s >> 16) : -1;
                span[5 * (long)p + 1] = found ? pair_i : -1;
                span[5 * (long)p + 2] = found ? (pair_s & 0xffff) : -1;
                span[5 * (long)p + 3] = found ? pair_j : -1;
                span[5 * (long)p + 4] = found ? pair_l : -1;
            }
        }
    }
}

int lalign_grid(int n) { return std::min(n, LA_MAX_BLOCKS); }

}  // namespace
}  // namespace cpc

extern "C" size_t cpc_local_align_scratch_bytes(int n_seg, int max_len_a, int max_len_b)
{
    if (n_seg < 0 || max_len_a < 0 || max_len_b < 0) {
        cpc::set_error("local_align: negative size (n_seg=%d max_len_a=%d max_len_b=%d)", n_seg, max_len_a, max_len_b);
        return 0;
    }
    if (n_seg == 0 || max_len_b == 0) return 0;
    if (max_len_a <= cpc::SD_T) return 0;                        // one strip per row item: no boundary row is stored
    return (size_t)cpc::lalign_grid(n_seg) * 2 * (size_t)max_len_b * cpc::LA_CELL_BYTES;
}

extern "C" int cpc_local_align(const float *frames, int dp, const int *item_off, const int *item_len, int n_items, const int *seg_a,
                               const int *seg_start, const int *pair_b, int n_seg, int max_len_a, int max_len_b, int distance,
                               float theta, float gamma, float *score, int *span, void *scratch, size_t scratch_bytes,
                               cpc_stream_t stream)
{
    CPC_REQUIRE(frames != nullptr && item_off != nullptr && item_len != nullptr && seg_a != nullptr && seg_start != nullptr &&
                    pair_b != nullptr && score != nullptr && span != nullptr,
                "local_align: null buffer");
    CPC_REQUIRE(dp >= 4 && dp % 4 == 0, "local_align: the frame stride dp=%d must be a positive multiple of 4", dp);
    CPC_REQUIRE(distance == CPC_ABX_COSINE || distance == CPC_ABX_EUCLIDIAN, "local_align: unknown distance %d", distance);
    CPC_REQUIRE(n_items > 0 && n_seg >= 0 && max_len_a >= 1 && max_len_b >= 1,
                "local_align: bad sizes (n_items=%d n_seg=%d max_len_a=%d max_len_b=%d)", n_items, n_seg, max_len_a, max_len_b);
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
    hipLaunchKernelGGL(cpc::lalign_kernel, dim3((unsigned)cpc::lalign_grid(n_seg)), dim3(cpc::SD_THREADS), 0,
                       static_cast<hipStream_t>(stream), frames, dp, item_off, item_len, n_items, seg_a, seg_start, pair_b, n_seg,
                       max_len_a, max_len_b, distance == CPC_ABX_EUCLIDIAN ? 1 : 0, theta, gamma, score, span,
                       need ? static_cast<char *>(scratch) : nullptr);
    CPC_CHECK_LAUNCH("lalign_kernel");
    return CPC_OK;
}
