// ABX on quantized units: batched DTW between sequences of unit ids (cpc/eval/eval_ABX_clustering.py of the reference, which
// expands every frame to a one-hot row and runs the dense DTW).  On one-hot frames the frame distance takes two values,
// d_same (equal units) and d_diff, so there is no distance tile, no LDS and no workgroup barrier: the kernel is the DP
// recursion of abx_dtw_kernel (abx.hip) alone.  DESIGN.md section 7.1 has the layout and the exactness argument.
//
//   abx_dtw_units_kernel   one workgroup per x item (a "segment"), ONE WAVE PER (x, y) PAIR: the four waves of a workgroup
//                          take the segment's y items round robin and never synchronise.  lane = row of x (strips of 64
//                          rows; the boundary row of a strip lives in per-wave scratch, double-buffered), step t = one
//                          anti-diagonal over ALL columns of y.  The lane keeps its x unit in a register.  y travels like
//                          the DP's `up` value: lane r needs y[t - r], which lane r - 1 used one step earlier, so one
//                          wave_shr:1 move per step feeds every lane and only lane 0 takes a new y[t] -- read with
//                          v_readlane from a register that holds 64 units of y (refilled every 64 steps, fetched one refill ahead).
//                          The previous strip's boundary row reaches lane 0 the same way.  Each cell carries (cost, path
//                          length) with abx_dtw_kernel's addition order (d + predecessor) and tie rule (diag, left, up).
#include "common.h"
#include "dtw_strip.h"

namespace cpc {
namespace {

constexpr int ABXU_T = 64;          // strip height (rows = lanes)
constexpr int ABXU_THREADS = 256;
constexpr int ABXU_WAVES = ABXU_THREADS / 64;

__device__ __forceinline__ float lane_value(float v, int l)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

__global__ void __launch_bounds__(ABXU_THREADS)
abx_dtw_units_kernel(const int *__restrict__ units, const int *__restrict__ item_off, const int *__restrict__ item_len,
                     int n_items, const int *__restrict__ seg_x, const int *__restrict__ seg_start,
                     const int *__restrict__ pair_y, int n_seg, int max_len_y, float d_same, float d_diff,
                     float *__restrict__ out, int *__restrict__ path_len, char *scratch)
{
    const int lane = threadIdx.x & 63;
    // the wave's index as a scalar: everything below that depends on the pair (lengths, loop bounds) is then wave-uniform,
    // so the loops run on the scalar unit and no lane is masked off by control flow inside a step
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // boundary rows of this wave: two (cost, length) rows of max_len_y, swapped per strip
    float *bc[2];
    int *bl[2];
    {
        char *base = scratch ? scratch + ((size_t)blockIdx.x * ABXU_WAVES + wave) * 2 * (size_t)max_len_y * 8 : nullptr;
        bc[0] = reinterpret_cast<float *>(base);
        bl[0] = reinterpret_cast<int *>(base + (size_t)max_len_y * 4);
        bc[1] = reinterpret_cast<float *>(base + (size_t)max_len_y * 8);
        bl[1] = reinterpret_cast<int *>(base + (size_t)max_len_y * 12);
    }

    for (int seg = blockIdx.x; seg < n_seg; seg += gridDim.x) {
        const int xi = seg_x[seg];
        const bool x_ok = xi >= 0 && xi < n_items;
        const int lx = x_ok ? item_len[xi] : 0;
        const long xo = x_ok ? (long)item_off[xi] : 0;
        const int p_end = seg_start[seg + 1];
        for (int p = seg_start[seg] + wave; p < p_end; p += ABXU_WAVES) {
            const int yi = pair_y[p];
            const bool y_ok = yi >= 0 && yi < n_items;
            const int ly = y_ok ? item_len[yi] : 0;
            const long yo = y_ok ? (long)item_off[yi] : 0;
            if (lx < 1 || ly < 1 || (lx > ABXU_T && (scratch == nullptr || ly > max_len_y))) {
                if (lane == 0) {                                 // not computable: NaN never compares < or ==
                    out[p] = __builtin_nanf("");
                    if (path_len) path_len[p] = -1;
                }
                continue;
            }
            int cur = 0;                                         // boundary buffer read by this strip
            float cur_c = 0.f;                                   // this lane's newest cell in its row
            int cur_l = 0;
            for (int rs = 0; rs < lx; rs += ABXU_T) {
                const int R = min(ABXU_T, lx - rs);
                const bool more_strips = rs + ABXU_T < lx;
                const int r = lane;
                const bool first_row = rs == 0 && r == 0;
                const int xu = r < R ? units[xo + rs + r] : -1;
                const float *in_c = bc[cur];
                const int *in_l = bl[cur];
                float *out_c = bc[cur ^ 1];
                int *out_l = bl[cur ^ 1];
                cur_c = 0.f;
                cur_l = 0;
                float pup_c = 0.f;                               // the up value of the previous step (= this step's diag)
                int pup_l = 0;
                int yu = -1;                                     // y[t - r]
                const int steps = R + ly - 1;
                // 64 columns of y (and of the previous strip's last row) per register, fetched one chunk ahead
                int y_next = lane < ly ? units[yo + lane] : -1;
                float b_next_c = 0.f;
                int b_next_l = 0;
                if (rs > 0 && lane < ly) {
                    b_next_c = in_c[lane];
                    b_next_l = in_l[lane];
                }
                for (int t0 = 0; t0 < steps; t0 += ABXU_T) {
                    const int y_chunk = y_next;
                    const float b_chunk_c = b_next_c;
                    const int b_chunk_l = b_next_l;
                    {
                        const int cn = t0 + ABXU_T + lane;
                        const bool in = cn < ly;
                        y_next = in ? units[yo + cn] : -1;
                        if (rs > 0 && in) {
                            b_next_c = in_c[cn];
                            b_next_l = in_l[cn];
                        }
                    }
                    const int n_t = min(ABXU_T, steps - t0);
                    for (int tl = 0; tl < n_t; ++tl) {
                        const int c = t0 + tl - r;
                        // lane 0's inputs of this step, wave-uniform: y[t] and the cell above it (the previous strip's last row)
                        const int y_t = __builtin_amdgcn_readlane(y_chunk, tl);
                        const float b_c = lane_value(b_chunk_c, tl);
                        const int b_l = __builtin_amdgcn_readlane(b_chunk_l, tl);
                        const float up_c = shr1(cur_c, b_c);     // lane r-1's newest cell: (r-1, c)
                        const int up_l = shr1(cur_l, b_l);
                        yu = shr1(yu, y_t);
                        const bool active = r < R && (unsigned)c < (unsigned)ly;
                        const bool first_col = c == 0;
                        const float d = yu == xu ? d_same : d_diff;
                        // predecessor: left along the first row (cost 0, length 0 before the first cell), up along the
                        // first column, else dtw.pyx:65-72: diag, then left, then up
                        const bool diag = !first_row && !first_col && pup_c <= cur_c && pup_c <= up_c;
                        const bool left = first_row || (!first_col && cur_c <= up_c);
                        const float pc = diag ? pup_c : (left ? cur_c : up_c);
                        const int pl = diag ? pup_l : (left ? cur_l : up_l);
                        const float nc = d + pc;
                        const int nl = pl + 1;
                        cur_c = active ? nc : cur_c;
                        cur_l = active ? nl : cur_l;
                        if (more_strips && active && r == ABXU_T - 1) {
                            out_c[c] = nc;
                            out_l[c] = nl;
                        }
                        pup_c = up_c;
                        pup_l = up_l;
                    }
                }
                cur ^= 1;
                __threadfence_block();                           // boundary row visible to the next strip's reads
            }
            if (lane == (lx - 1) % ABXU_T) {                     // the last row's lane: its newest cell is (lx-1, ly-1)
                out[p] = cur_c / (float)cur_l;
                if (path_len) path_len[p] = cur_l;
            }
        }
    }
}

}  // namespace
}  // namespace cpc

extern "C" size_t cpc_abx_dtw_units_scratch_bytes(int n_seg, int max_len_x, int max_len_y)
{
    if (n_seg <= 0 || max_len_x <= 0 || max_len_y <= 0) return 0;
    if (max_len_x <= cpc::ABXU_T) return 0;                      // one strip per item: no boundary row is stored
    return (size_t)cpc::dtw_grid(n_seg) * cpc::ABXU_WAVES * 2 * (size_t)max_len_y * 8;
}

extern "C" int cpc_abx_dtw_units(const int *units, const int *item_off, const int *item_len, int n_items, const int *seg_x,
                                 const int *seg_start, const int *pair_y, int n_seg, int max_len_x, int max_len_y,
                                 float d_same, float d_diff, float *out, int *path_len, void *scratch,
                                 size_t scratch_bytes, cpc_stream_t stream)
{
    CPC_REQUIRE(units != nullptr && item_off != nullptr && item_len != nullptr && seg_x != nullptr && seg_start != nullptr &&
                    pair_y != nullptr && out != nullptr,
                "abx_dtw_units: null buffer");
    CPC_REQUIRE(d_same == d_same && d_diff == d_diff, "abx_dtw_units: the frame distances (d_same=%g d_diff=%g) must not be NaN",
                (double)d_same, (double)d_diff);
    CPC_REQUIRE(n_items > 0 && n_seg >= 0 && max_len_x >= 1 && max_len_y >= 1,
                "abx_dtw_units: bad sizes (n_items=%d n_seg=%d max_len_x=%d max_len_y=%d)", n_items, n_seg, max_len_x,
                max_len_y);
    const size_t need = cpc_abx_dtw_units_scratch_bytes(n_seg, max_len_x, max_len_y);
    CPC_REQUIRE(scratch_bytes >= need && (need == 0 || scratch != nullptr), "abx_dtw_units: scratch of %zu bytes, %zu needed",
                scratch_bytes, need);
    if (n_seg == 0) return CPC_OK;
    hipLaunchKernelGGL(cpc::abx_dtw_units_kernel, dim3((unsigned)cpc::dtw_grid(n_seg)), dim3(cpc::ABXU_THREADS), 0,
                       static_cast<hipStream_t>(stream), units, item_off, item_len, n_items, seg_x, seg_start, pair_y, n_seg,
                       max_len_y, d_same, d_diff, out, path_len, need ? static_cast<char *>(scratch) : nullptr);
    CPC_CHECK_LAUNCH("abx_dtw_units_kernel");
    return CPC_OK;
}
