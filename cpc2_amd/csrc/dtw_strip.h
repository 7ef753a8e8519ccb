// The walk that the dense DTW kernels share (abx.hip, sdtw.hip, lalign.hip), in one copy: a row item against a column item in
// 64 x 64 tiles of frame distances, the DP of a tile on wave 0 with lane = row and step = anti-diagonal, row items longer than 64
// frames in 64-row strips whose last row waits for the next strip in per-workgroup scratch.  DESIGN.md section 7 has the scheme.
// A kernel brings a Rule: its cell (how many words), its recurrence, what it notes of a finished cell and of a finished strip.
// Everything here inlines: a cell and a rule's state live in registers.  The kernels on unit ids (abx_units.hip, sdtw_units.hip,
// lalign_units.hip) walk differently (one wave per pair, no tiles): dtw_units_walk.h, which takes the cell, shr1, dtw_pick and
// dtw_item from here.
#pragma once

#include "common.h"

#include <algorithm>

namespace cpc {

constexpr int DTW_T = 64;                    // tile edge (rows = lanes of the DP wave)
constexpr int DTW_THREADS = 256;
constexpr int DTW_DT_STRIDE = DTW_T + 2;     // (65 r + t) % 32: the DP wave's column reads hit 32 banks
constexpr int DTW_MAX_BLOCKS = 8192;

// lane i receives lane i-1's value (DPP wave_shr:1); lane 0 keeps `own`
__device__ __forceinline__ float shr1(float v, float own)
{
    return __builtin_amdgcn_update_dpp(own, v, 0x138, 0xf, 0xf, false);
}
__device__ __forceinline__ int shr1(int v, int own)
{
    return __builtin_amdgcn_update_dpp(own, v, 0x138, 0xf, 0xf, false);
}

// A DP cell of W 32-bit words: the value a path accumulates and W - 1 integers that travel with it.
template <int W>
struct DtwCell {
    float v;
    int n[W - 1];
};
constexpr int DTW_LEN = 0, DTW_START = 1;    // n[DTW_LEN]: cells on the path; n[DTW_START] (W = 3): where it started

// lane i receives lane i-1's cell, word by word; lane 0 receives zeros
template <int W>
__device__ __forceinline__ DtwCell<W> shr1(const DtwCell<W> &c)
{
    DtwCell<W> o;
    o.v = shr1(c.v, 0.f);
#pragma unroll
    for (int w = 0; w < W - 1; ++w) o.n[w] = shr1(c.n[w], 0);
    return o;
}

// a or b, word by word: selects between registers (a choice between two cells by reference or by branch can leave them in memory)
template <int W>
__device__ __forceinline__ DtwCell<W> dtw_pick(bool take_a, const DtwCell<W> &a, const DtwCell<W> &b)
{
    DtwCell<W> o;
    o.v = take_a ? a.v : b.v;
#pragma unroll
    for (int w = 0; w < W - 1; ++w) o.n[w] = take_a ? a.n[w] : b.n[w];
    return o;
}

// The predecessor of smallest value; ties go to diag, then left, then up (dtw.pyx:65-72 of the reference).
template <int W>
__device__ __forceinline__ DtwCell<W> dtw_cheapest(const DtwCell<W> &diag, const DtwCell<W> &left, const DtwCell<W> &up)
{
    return dtw_pick(diag.v <= left.v && diag.v <= up.v, diag, dtw_pick(left.v <= up.v, left, up));
}

// The boundary rows of this workgroup: two buffers, swapped per strip, of W planes of max_len_col words each.  Word w of column
// j of buffer b is word (b W + w) max_len_col + j behind the workgroup's base.  Without scratch the base is null and is never
// offset: a kernel calls load / store only for a row item of more than one strip, which it refuses without scratch.
template <int W>
struct DtwBoundary {
    int *base;
    size_t plane;                            // words per plane

    __device__ __forceinline__ DtwBoundary(char *scratch, int max_len_col)
        : base(scratch ? reinterpret_cast<int *>(scratch) + (size_t)blockIdx.x * 2 * W * (size_t)max_len_col : nullptr),
          plane((size_t)max_len_col)
    {
    }
    __device__ __forceinline__ int *word(int b, int w, int j) const { return base + (size_t)(b * W + w) * plane + j; }
    __device__ __forceinline__ DtwCell<W> load(int b, int j) const
    {
        DtwCell<W> c;
        c.v = __int_as_float(*word(b, 0, j));
#pragma unroll
        for (int w = 1; w < W; ++w) c.n[w - 1] = *word(b, w, j);
        return c;
    }
    __device__ __forceinline__ void store(int b, int j, const DtwCell<W> &c) const
    {
        *word(b, 0, j) = __float_as_int(c.v);
#pragma unroll
        for (int w = 1; w < W; ++w) *word(b, w, j) = c.n[w - 1];
    }
};

// Item idx of the work list, bounds-checked: an index out of range is an item of length 0.
struct DtwItem {
    int len;
    long off;
};
__device__ __forceinline__ DtwItem dtw_item(const int *__restrict__ item_off, const int *__restrict__ item_len, int n_items, int idx)
{
    const bool ok = idx >= 0 && idx < n_items;
    return {ok ? item_len[idx] : 0, ok ? (long)item_off[idx] : 0};
}

// One pair: len_row x len_col cells, walked strip by strip and tile by tile.  Called by all DTW_THREADS threads of the workgroup
// with the same arguments.  fill_tile(rs, R, cb, C) is called by all of them and leaves the distances of rows rs .. rs + R - 1
// against columns cb .. cb + C - 1 in dt[r][c] behind a workgroup barrier (and opens with one, before it rewrites dt).
// Wave 0 then runs the tile's cells, and for each cell (gi, gj), in an order in which diag, left and up are finished:
//     cell = rule.cell(gi, gj, d, diag, left, up)     the new cell; a neighbour outside the matrix is not a cell: the rule ignores
//                                                     it, but may count on `left` being the zero cell at column 0
//     rule.visit(gi, gj, cell)                        by the lane of row gi % 64
// and after the last tile of a strip, in all 64 lanes, rule.strip_done(rs, R, more_strips).
template <int W, class Rule, class FillTile>
__device__ __forceinline__ void dtw_walk_pair(const DtwBoundary<W> &bnd, int len_row, int len_col, const float (*dt)[DTW_DT_STRIDE],
                                              Rule &rule, FillTile &&fill_tile)
{
    const int r = threadIdx.x & 63;
    const bool dp_wave = threadIdx.x < 64;
    int cur = 0;                                         // boundary buffer read by this strip
    for (int rs = 0; rs < len_row; rs += DTW_T) {
        const int R = min(DTW_T, len_row - rs);
        const bool more_strips = rs + DTW_T < len_row;
        const int gi = rs + r;
        DtwCell<W> cell = {};                            // DP wave: this lane's newest cell in its row
        DtwCell<W> pup = {};                             // the up value of the previous step (= this step's diag)
        for (int cb = 0; cb < len_col; cb += DTW_T) {
            const int C = min(DTW_T, len_col - cb);
            fill_tile(rs, R, cb, C);
            if (dp_wave) {
                for (int t = 0; t < R + C - 1; ++t) {
                    const int c = t - r;
                    DtwCell<W> up = shr1(cell);          // lane r-1's newest cell: (r-1, c)
                    if (r < R && c >= 0 && c < C) {
                        const int gj = cb + c;
                        DtwCell<W> diag = pup;
                        if (r == 0 && rs > 0) {          // the row above is the previous strip's last row
                            up = bnd.load(cur, gj);
                            if (gj > 0) diag = bnd.load(cur, gj - 1);
                        }
                        cell = rule.cell(gi, gj, dt[r][c], diag, cell, up);
                        if (r == R - 1 && more_strips) bnd.store(cur ^ 1, gj, cell);
                        rule.visit(gi, gj, cell);
                    }
                    pup = up;
                }
            }
        }
        if (dp_wave) rule.strip_done(rs, R, more_strips);
        cur ^= 1;
        __threadfence_block();                           // boundary row visible to the next strip's lane 0
    }
}

// ---- host side ----
inline int dtw_grid(int n) { return std::min(n, DTW_MAX_BLOCKS); }

// Bytes of the boundary rows of a launch over n_seg segments: per workgroup two buffers of max_len_col cells of W words.
inline size_t dtw_boundary_bytes(int n_seg, int max_len_col, int W)
{
    return (size_t)dtw_grid(n_seg) * 2 * (size_t)max_len_col * 4 * (size_t)W;
}

// The checks that the dense entry points repeat.  `what` is the entry point's label and row / col its names of the two size
// arguments, as the messages spell them.  CPC_OK or CPC_ERR_INVALID.
inline int dtw_check_args(const char *what, bool buffers_ok, int dp, int distance, int n_items, int n_seg, const char *row,
                          int max_len_row, const char *col, int max_len_col)
{
    CPC_REQUIRE(buffers_ok, "%s: null buffer", what);
    CPC_REQUIRE(dp >= 4 && dp % 4 == 0, "%s: the frame stride dp=%d must be a positive multiple of 4", what, dp);
    CPC_REQUIRE(distance == CPC_ABX_COSINE || distance == CPC_ABX_EUCLIDIAN, "%s: unknown distance %d", what, distance);
    CPC_REQUIRE(n_items > 0 && n_seg >= 0 && max_len_row >= 1 && max_len_col >= 1, "%s: bad sizes (n_items=%d n_seg=%d %s=%d %s=%d)",
                what, n_items, n_seg, row, max_len_row, col, max_len_col);
    return CPC_OK;
}

}  // namespace cpc
