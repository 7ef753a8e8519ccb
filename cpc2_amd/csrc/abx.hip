// ABX phone discriminability: batched DTW over frame-distance tiles and the per-triplet comparison counts
// (cpc/eval/ABX/abx_group_computation.py + dtw.pyx of the reference).  DESIGN.md section "ABX" has the layout and the
// exactness argument.
//
//   abx_dtw_kernel     one workgroup per x item (a "segment") and its list of y items.  For each (x, y) pair the Lx x Ly
//                      frame-distance matrix is formed 64 x 64 tile by tile in LDS (true f32 FMAs, k-ordered), and the
//                      DTW recursion runs over the tile on the anti-diagonal in wave 0 with lane = row.  Each cell carries
//                      (cost, path length); the length follows the reference's backtrack tie rule, so no cost matrix and
//                      no backtrack are needed.  Items longer than 64 frames go in 64-row strips whose boundary row lives
//                      in per-workgroup scratch (double-buffered).
//   abx_counts_kernel  one workgroup per triplet: counts dxa < dxb and dxa == dxb over its Nx x Na x Nb comparisons,
//                      reading the pair results through index lists (-1 = excluded diagonal).  Integer counts: deterministic.
#include "common.h"

#include <algorithm>

namespace cpc {
namespace {

constexpr int ABX_T = 64;          // tile edge (rows = lanes of the DP wave)
constexpr int ABX_KC = 32;         // feature chunk staged in LDS per pass
constexpr int ABX_THREADS = 256;
constexpr int ABX_ACC = ABX_T * ABX_T / ABX_THREADS;   // distance entries per thread
constexpr int ABX_DT_STRIDE = ABX_T + 2;               // (65 r + t) % 32: the DP wave's column reads hit 32 banks
constexpr int ABX_MAX_BLOCKS = 8192;

// lane i receives lane i-1's value (DPP wave_shr:1); lane 0 keeps `own`
__device__ __forceinline__ float shr1(float v, float own)
{
    return __builtin_amdgcn_update_dpp(own, v, 0x138, 0xf, 0xf, false);
}
__device__ __forceinline__ int shr1(int v, int own)
{
    return __builtin_amdgcn_update_dpp(own, v, 0x138, 0xf, 0xf, false);
}

__global__ void __launch_bounds__(ABX_THREADS)
abx_dtw_kernel(const float *__restrict__ frames, int dp, const int *__restrict__ item_off, const int *__restrict__ item_len,
               int n_items, const int *__restrict__ seg_x, const int *__restrict__ seg_start, const int *__restrict__ pair_y,
               int n_seg, int max_len_y, int euclid, float *__restrict__ out, int *__restrict__ path_len, char *scratch)
{
    __shared__ float xs[ABX_T][ABX_KC + 1];
    __shared__ float ys[ABX_T][ABX_KC + 1];
    __shared__ float dt[ABX_T][ABX_DT_STRIDE];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const bool dp_wave = tid < 64;
    // boundary rows of this workgroup: two (cost, length) rows of max_len_y, swapped per strip
    float *bc[2];
    int *bl[2];
    {
        char *base = scratch ? scratch + (size_t)blockIdx.x * 2 * (size_t)max_len_y * 8 : nullptr;
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
        for (int p = seg_start[seg]; p < seg_start[seg + 1]; ++p) {
            const int yi = pair_y[p];
            const bool y_ok = yi >= 0 && yi < n_items;
            const int ly = y_ok ? item_len[yi] : 0;
            const long yo = y_ok ? (long)item_off[yi] : 0;
            if (lx < 1 || ly < 1 || (lx > ABX_T && (scratch == nullptr || ly > max_len_y))) {
                if (tid == 0) {                                  // not computable: NaN never compares < or ==
                    out[p] = __builtin_nanf("");
                    if (path_len) path_len[p] = -1;
                }
                continue;
            }
            int cur = 0;                                         // boundary buffer read by this strip
            for (int rs = 0; rs < lx; rs += ABX_T) {
                const int R = min(ABX_T, lx - rs);
                const bool more_strips = rs + ABX_T < lx;
                float cur_c = 0.f;                               // DP wave: this lane's newest cell in its row
                int cur_l = 0;
                float pup_c = 0.f;                               // the up value of the previous step (= this step's diag)
                int pup_l = 0;
                for (int cb = 0; cb < ly; cb += ABX_T) {
                    const int C = min(ABX_T, ly - cb);
                    const int RC = R * C;
                    // ---- distance tile: acc over the feature dim, k-ordered fma chain per entry ----
                    float acc[ABX_ACC];
#pragma unroll
                    for (int j = 0; j < ABX_ACC; ++j) acc[j] = 0.f;
                    for (int k0 = 0; k0 < dp; k0 += ABX_KC) {
                        const int kc4 = min(ABX_KC, dp - k0) >> 2;      // dp is a multiple of 4
                        __syncthreads();                                 // previous users of xs / ys / dt are done
                        for (int e = tid; e < R * kc4; e += ABX_THREADS) {
                            const int r = e / kc4, k = (e - r * kc4) * 4;
                            const float4 v = *reinterpret_cast<const float4 *>(frames + (xo + rs + r) * dp + k0 + k);
                            xs[r][k] = v.x; xs[r][k + 1] = v.y; xs[r][k + 2] = v.z; xs[r][k + 3] = v.w;
                        }
                        for (int e = tid; e < C * kc4; e += ABX_THREADS) {
                            const int c = e / kc4, k = (e - c * kc4) * 4;
                            const float4 v = *reinterpret_cast<const float4 *>(frames + (yo + cb + c) * dp + k0 + k);
                            ys[c][k] = v.x; ys[c][k + 1] = v.y; ys[c][k + 2] = v.z; ys[c][k + 3] = v.w;
                        }
                        __syncthreads();
                        const int kc = kc4 * 4;
#pragma unroll
                        for (int j = 0; j < ABX_ACC; ++j) {
                            const int e = tid + j * ABX_THREADS;
                            if (e < RC) {
                                const int r = e / C, c = e - (e / C) * C;
                                float a = acc[j];
                                if (euclid) {
                                    for (int k = 0; k < kc; ++k) {
                                        const float df = xs[r][k] - ys[c][k];
                                        a = fmaf(df, df, a);
                                    }
                                } else {
                                    for (int k = 0; k < kc; ++k) a = fmaf(xs[r][k], ys[c][k], a);
                                }
                                acc[j] = a;
                            }
                        }
                    }
#pragma unroll
                    for (int j = 0; j < ABX_ACC; ++j) {
                        const int e = tid + j * ABX_THREADS;
                        if (e < RC) {
                            const int r = e / C, c = e - (e / C) * C;
                            dt[r][c] = euclid ? sqrtf(acc[j]) : acosf(fminf(fmaxf(acc[j], -1.f), 1.f)) / 3.14159265358979323846f;
                        }
                    }
                    __syncthreads();
                    // ---- DTW over the tile: wave 0, lane = row, step t = anti-diagonal ----
                    if (dp_wave) {
                        const int r = lane;
                        const int gi = rs + r;
                        const float *in_c = bc[cur];
                        const int *in_l = bl[cur];
                        float *out_c = bc[cur ^ 1];
                        int *out_l = bl[cur ^ 1];
                        for (int t = 0; t < R + C - 1; ++t) {
                            const int c = t - r;
                            float up_c = shr1(cur_c, 0.f);       // lane r-1's newest cell: (r-1, c)
                            int up_l = shr1(cur_l, 0);
                            if (r < R && c >= 0 && c < C) {
                                const int gj = cb + c;
                                const float d = dt[r][c];
                                float nc;
                                int nl;
                                float dg_c = pup_c;
                                int dg_l = pup_l;
                                if (r == 0 && rs > 0) {          // the row above is the previous strip's last row
                                    up_c = in_c[gj];
                                    up_l = in_l[gj];
                                    if (gj > 0) {
                                        dg_c = in_c[gj - 1];
                                        dg_l = in_l[gj - 1];
                                    }
                                }
                                if (gi == 0 && gj == 0) {
                                    nc = d;
                                    nl = 1;
                                } else if (gi == 0) {
                                    nc = d + cur_c;
                                    nl = cur_l + 1;
                                } else if (gj == 0) {
                                    nc = d + up_c;
                                    nl = up_l + 1;
                                } else if (dg_c <= cur_c && dg_c <= up_c) {   // dtw.pyx:65-72: diag, then left, then up
                                    nc = d + dg_c;
                                    nl = dg_l + 1;
                                } else if (cur_c <= up_c) {
                                    nc = d + cur_c;
                                    nl = cur_l + 1;
                                } else {
                                    nc = d + up_c;
                                    nl = up_l + 1;
                                }
                                cur_c = nc;
                                cur_l = nl;
                                if (r == R - 1 && more_strips) {
                                    out_c[gj] = nc;
                                    out_l[gj] = nl;
                                }
                                if (gi == lx - 1 && gj == ly - 1) {
                                    out[p] = nc / (float)nl;
                                    if (path_len) path_len[p] = nl;
                                }
                            }
                            pup_c = up_c;
                            pup_l = up_l;
                        }
                    }
                }
                cur ^= 1;
                __threadfence_block();                           // boundary row visible to the next strip's lane 0
            }
        }
    }
}

__global__ void __launch_bounds__(ABX_THREADS)
abx_counts_kernel(const float *__restrict__ dist, int n_pairs, const int *__restrict__ idx_a, const int *__restrict__ idx_b,
                  const int *__restrict__ shape, int n_trip, int *__restrict__ lt, int *__restrict__ eq)
{
    __shared__ int s_lt, s_eq;
    for (int tr = blockIdx.x; tr < n_trip; tr += gridDim.x) {
        const int nx = shape[tr * 5], na = shape[tr * 5 + 1], nb = shape[tr * 5 + 2];
        const int *ia_row = idx_a + shape[tr * 5 + 3];
        const int *ib_row = idx_b + shape[tr * 5 + 4];
        if (threadIdx.x == 0) {
            s_lt = 0;
            s_eq = 0;
        }
        __syncthreads();
        int my_lt = 0, my_eq = 0;
        const int nab = na * nb;
        const int total = nx * nab;
        for (int e = threadIdx.x; e < total; e += ABX_THREADS) {
            const int i = e / nab;
            const int rem = e - i * nab;
            const int j = rem / nb, k = rem - (rem / nb) * nb;
            const int ia = ia_row[i * na + j];
            const int ib = ib_row[i * nb + k];
            if (ia < 0 || ia >= n_pairs || ib < 0 || ib >= n_pairs) continue;     // excluded diagonal
            const float va = dist[ia], vb = dist[ib];
            my_lt += va < vb;
            my_eq += va == vb;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            my_lt += __shfl_xor(my_lt, o);
            my_eq += __shfl_xor(my_eq, o);
        }
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(&s_lt, my_lt);
            atomicAdd(&s_eq, my_eq);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            lt[tr] = s_lt;
            eq[tr] = s_eq;
        }
        __syncthreads();
    }
}

int abx_grid(int n) { return std::min(n, ABX_MAX_BLOCKS); }

}  // namespace
}  // namespace cpc

extern "C" size_t cpc_abx_dtw_scratch_bytes(int n_seg, int max_len_x, int max_len_y)
{
    if (n_seg <= 0 || max_len_x <= 0 || max_len_y <= 0) return 0;
    if (max_len_x <= cpc::ABX_T) return 0;                       // one strip per item: no boundary row is stored
    return (size_t)cpc::abx_grid(n_seg) * 2 * (size_t)max_len_y * 8;
}

extern "C" int cpc_abx_dtw(const float *frames, int dp, const int *item_off, const int *item_len, int n_items,
                           const int *seg_x, const int *seg_start, const int *pair_y, int n_seg, int max_len_x,
                           int max_len_y, int distance, float *out, int *path_len, void *scratch, size_t scratch_bytes,
                           cpc_stream_t stream)
{
    CPC_REQUIRE(frames != nullptr && item_off != nullptr && item_len != nullptr && seg_x != nullptr && seg_start != nullptr &&
                    pair_y != nullptr && out != nullptr,
                "abx_dtw: null buffer");
    CPC_REQUIRE(dp >= 4 && dp % 4 == 0, "abx_dtw: the frame stride dp=%d must be a positive multiple of 4", dp);
    CPC_REQUIRE(distance == CPC_ABX_COSINE || distance == CPC_ABX_EUCLIDIAN, "abx_dtw: unknown distance %d", distance);
    CPC_REQUIRE(n_items > 0 && n_seg >= 0 && max_len_x >= 1 && max_len_y >= 1,
                "abx_dtw: bad sizes (n_items=%d n_seg=%d max_len_x=%d max_len_y=%d)", n_items, n_seg, max_len_x, max_len_y);
    const size_t need = cpc_abx_dtw_scratch_bytes(n_seg, max_len_x, max_len_y);
    CPC_REQUIRE(scratch_bytes >= need && (need == 0 || scratch != nullptr), "abx_dtw: scratch of %zu bytes, %zu needed",
                scratch_bytes, need);
    if (n_seg == 0) return CPC_OK;
    hipLaunchKernelGGL(cpc::abx_dtw_kernel, dim3((unsigned)cpc::abx_grid(n_seg)), dim3(cpc::ABX_THREADS), 0,
                       static_cast<hipStream_t>(stream), frames, dp, item_off, item_len, n_items, seg_x, seg_start, pair_y,
                       n_seg, max_len_y, distance == CPC_ABX_EUCLIDIAN ? 1 : 0, out, path_len,
                       need ? static_cast<char *>(scratch) : nullptr);
    CPC_CHECK_LAUNCH("abx_dtw_kernel");
    return CPC_OK;
}

extern "C" int cpc_abx_counts(const float *dist, int n_pairs, const int *idx_a, const int *idx_b, const int *shape,
                              int n_trip, int *lt, int *eq, cpc_stream_t stream)
{
    CPC_REQUIRE(dist != nullptr && idx_a != nullptr && idx_b != nullptr && shape != nullptr && lt != nullptr && eq != nullptr,
                "abx_counts: null buffer");
    CPC_REQUIRE(n_pairs > 0 && n_trip >= 0, "abx_counts: bad sizes (n_pairs=%d n_trip=%d)", n_pairs, n_trip);
    if (n_trip == 0) return CPC_OK;
    hipLaunchKernelGGL(cpc::abx_counts_kernel, dim3((unsigned)cpc::abx_grid(n_trip)), dim3(cpc::ABX_THREADS), 0,
                       static_cast<hipStream_t>(stream), dist, n_pairs, idx_a, idx_b, shape, n_trip, lt, eq);
    CPC_CHECK_LAUNCH("abx_counts_kernel");
    return CPC_OK;
}
