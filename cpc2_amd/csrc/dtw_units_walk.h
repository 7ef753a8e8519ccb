// The walk of the DTW kernels on UNIT IDS (abx_units.hip, sdtw_units.hip, lalign_units.hip), in one copy.  On units the frame distance takes two
// values, d_same (equal units) and d_diff, so there is no distance tile, no LDS and no workgroup barrier: a kernel is its
// recurrence alone, and every wave runs it.  DESIGN.md section 29 has the scheme:
//   - one workgroup of 256 threads per segment, ONE WAVE PER (row item, column item) PAIR: the four waves take the segment's
//     pairs round robin and never synchronise;
//   - lane = row of the row item (strips of 64 rows), step t = one anti-diagonal over ALL columns of the column item;
//   - the lane keeps its row's unit in a register.  The column item's units travel like the DP's `up` cell: lane r needs y[t - r],
//     which lane r - 1 used one step earlier, so one wave_shr:1 move per step feeds every lane and only lane 0 takes a new y[t],
//     by v_readlane from a register that holds 64 units (refilled every 64 steps, fetched one refill ahead);
//   - the previous strip's last row reaches lane 0 the same way, from per-wave scratch that is double-buffered per strip;
//   - lanes outside the matrix are masked by selects, not branches; the caller takes its wave index through readfirstlane, so
//     lengths and loop bounds are scalars.
// A kernel brings a Rule with the interface of dtw_walk_pair (dtw_strip.h): cell, visit, strip_done; the dense and the unit
// kernels share their Rules (abx_rule.h, sdtw_rule.h, lalign_rule.h).
#pragma once

#include "dtw_strip.h"

namespace cpc {

constexpr int DTWU_T = 64;                       // strip height (rows = lanes)
constexpr int DTWU_THREADS = 256;
constexpr int DTWU_WAVES = DTWU_THREADS / 64;
// The grid cap is the entry point's (the kernels loop over segments with a grid stride, and the scratch grows with the grid).
// 2048 workgroups = 8192 waves: every wave slot of 256 CUs x 4 SIMDs at 8 waves per SIMD; the two term kernels take it.
// cpc_abx_dtw_units keeps the 8192 of the dense kernels (DTW_MAX_BLOCKS), with which it was written and measured.  The two caps
// have not been measured against each other on that kernel.
constexpr int DTWU_MAX_BLOCKS = 2048;

// The boundary rows of one wave: two buffers, swapped per strip, of W planes of max_len_col words each.  Word w of column j of
// buffer b is word (b W + w) max_len_col + j behind the wave's base.  Without scratch the base is null and is never offset:
// load / store run only for a row item of more than one strip.  The host sizes (and insists on) the scratch from max_len_row, and
// the kernels write NaN for a row item longer than that maximum or a column item longer than max_len_col before they walk it.
template <int W>
struct DtwWaveBoundary {
    int *base;
    size_t plane;                                // words per plane

    __device__ __forceinline__ DtwWaveBoundary(char *scratch, int wave, int max_len_col)
        : base(scratch ? reinterpret_cast<int *>(scratch) + ((size_t)blockIdx.x * DTWU_WAVES + wave) * 2 * W * (size_t)max_len_col
                       : nullptr),
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

// lane l's cell in every lane (l is wave-uniform)
template <int W>
__device__ __forceinline__ DtwCell<W> dtw_lane_cell(const DtwCell<W> &c, int l)
{
    DtwCell<W> o;
    o.v = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(c.v), l));
#pragma unroll
    for (int w = 0; w < W - 1; ++w) o.n[w] = __builtin_amdgcn_readlane(c.n[w], l);
    return o;
}

// lane i receives lane i-1's cell, word by word; lane 0 receives `own`
template <int W>
__device__ __forceinline__ DtwCell<W> shr1(const DtwCell<W> &c, const DtwCell<W> &own)
{
    DtwCell<W> o;
    o.v = shr1(c.v, own.v);
#pragma unroll
    for (int w = 0; w < W - 1; ++w) o.n[w] = shr1(c.n[w], own.n[w]);
    return o;
}

// One pair: len_row x len_col cells, walked strip by strip by ONE WAVE, whose 64 lanes call this with the same arguments
// (1 <= len_col <= the max_len_col of bnd; len_row > 64 only with scratch).  The row item is units[row_off ..], the column item
// units[col_off ..]; nothing outside them is read.  For each cell (gi, gj), in an order in which diag, left and up are finished:
//     cell = rule.cell(gi, gj, d, diag, left, up)     d = d_same where the two units are equal, else d_diff; a neighbour outside
//                                                     the matrix is not a cell: the rule ignores it, but may count on
//                                                     `left` being the zero cell at column 0
//     rule.visit(gi, gj, cell)                        by the lane of row gi % 64
// and after the last step of a strip, in all 64 lanes, rule.strip_done(rs, R, more_strips).
// Returns the calling lane's newest cell of the last strip: in lane (len_row - 1) % 64 the cell (len_row - 1, len_col - 1).
template <int W, class Rule>
__device__ __forceinline__ DtwCell<W> dtw_units_walk_pair(const DtwWaveBoundary<W> &bnd, const int *__restrict__ units, long row_off,
                                                          int len_row, long col_off, int len_col, float d_same, float d_diff,
                                                          Rule &rule)
{
    const int r = threadIdx.x & 63;
    int cur = 0;                                             // boundary buffer read by this strip
    DtwCell<W> cell = {};                                    // this lane's newest cell in its row
    for (int rs = 0; rs < len_row; rs += DTWU_T) {
        const int R = min(DTWU_T, len_row - rs);
        const bool more_strips = rs + DTWU_T < len_row;
        const int gi = rs + r;
        const int xu = r < R ? units[row_off + gi] : 0;      // (a lane without a row is never active: its unit is not looked at)
        cell = {};
        DtwCell<W> pup = {};                                 // the up cell of the previous step (= this step's diag)
        int yu = 0;                                          // y[t - r]
        const int steps = R + len_col - 1;
        // 64 columns of y (and of the previous strip's last row) per register, fetched one chunk ahead
        int y_next = r < len_col ? units[col_off + r] : 0;
        DtwCell<W> b_next = {};
        if (rs > 0 && r < len_col) b_next = bnd.load(cur, r);
        for (int t0 = 0; t0 < steps; t0 += DTWU_T) {
            const int y_chunk = y_next;
            const DtwCell<W> b_chunk = b_next;
            {
                const int cn = t0 + DTWU_T + r;
                const bool in = cn < len_col;
                y_next = in ? units[col_off + cn] : 0;
                if (rs > 0 && in) b_next = bnd.load(cur, cn);
            }
            const int n_t = min(DTWU_T, steps - t0);
            for (int tl = 0; tl < n_t; ++tl) {
                const int gj = t0 + tl - r;
                // lane 0's inputs of this step, wave-uniform: y[t] and the cell above it (the previous strip's last row; in the
                // first strip zeros that no rule looks at)
                const int y_t = __builtin_amdgcn_readlane(y_chunk, tl);
                const DtwCell<W> up = shr1(cell, dtw_lane_cell(b_chunk, tl));    // lane r-1's newest cell: (gi-1, gj)
                yu = shr1(yu, y_t);
                const bool active = r < R && (unsigned)gj < (unsigned)len_col;
                const float d = yu == xu ? d_same : d_diff;
                const DtwCell<W> nc = rule.cell(gi, gj, d, pup, cell, up);
                cell = dtw_pick(active, nc, cell);
                if (active) {
                    if (more_strips && r == DTWU_T - 1) bnd.store(cur ^ 1, gj, nc);
                    rule.visit(gi, gj, nc);
                }
                pup = up;
            }
        }
        rule.strip_done(rs, R, more_strips);
        cur ^= 1;
        __threadfence_block();                               // boundary row visible to the next strip's reads
    }
    return cell;
}

// ---- host side ----
inline int dtw_units_grid(int n, int max_blocks) { return std::min(n, max_blocks); }

// Bytes of the boundary rows of a launch over n_seg segments on at most max_blocks workgroups: per wave two buffers of
// max_len_col cells of W words; nothing when one strip holds every row item.  Negative sizes give 0 with a message that names `what`.
inline size_t dtw_units_scratch_bytes(const char *what, int n_seg, const char *row, int max_len_row, const char *col, int max_len_col,
                                      int W, int max_blocks)
{
    if (n_seg < 0 || max_len_row < 0 || max_len_col < 0) {
        set_error("%s: negative size (n_seg=%d %s=%d %s=%d)", what, n_seg, row, max_len_row, col, max_len_col);
        return 0;
    }
    if (n_seg == 0 || max_len_col == 0 || max_len_row <= DTWU_T) return 0;
    return (size_t)dtw_units_grid(n_seg, max_blocks) * DTWU_WAVES * 2 * (size_t)max_len_col * 4 * (size_t)W;
}

// The checks that the unit entry points repeat.  `what` is the entry point's label and row / col its names of the two size
// arguments, as the messages spell them.  CPC_OK or CPC_ERR_INVALID.
inline int dtw_units_check_args(const char *what, bool buffers_ok, float d_same, float d_diff, int n_items, int n_seg, const char *row,
                                int max_len_row, const char *col, int max_len_col)
{
    CPC_REQUIRE(buffers_ok, "%s: null buffer", what);
    CPC_REQUIRE(d_same == d_same && d_diff == d_diff, "%s: the frame distances (d_same=%g d_diff=%g) must not be NaN", what,
                (double)d_same, (double)d_diff);
    CPC_REQUIRE(n_items > 0 && n_seg >= 0 && max_len_row >= 1 && max_len_col >= 1, "%s: bad sizes (n_items=%d n_seg=%d %s=%d %s=%d)",
                what, n_items, n_seg, row, max_len_row, col, max_len_col);
    return CPC_OK;
}

}  // namespace cpc
