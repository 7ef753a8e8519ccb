// ABX phone discriminability: batched DTW over frame-distance tiles and the per-triplet comparison counts
// (cpc/eval/ABX/abx_group_computation.py + dtw.pyx of the reference).  DESIGN.md section "ABX" has the layout and the
// exactness argument.
//
//   abx_dtw_kernel     one workgroup per x item (a "segment") and its list of y items, walked as dtw_strip.h says.  What is
//                      this file's: the distance tile (one entry per thread, true f32 FMAs, k-ordered: ABX items have 3 to 25
//                      frames).  The recurrence is abx_rule.h's, shared with abx_units.hip; AbxDenseRule adds the write of the
//                      result, from `visit` of the last cell.
//   abx_counts_kernel  one workgroup per triplet: counts dxa < dxb and dxa == dxb over its Nx x Na x Nb comparisons,
//                      reading the pair results through index lists (-1 = excluded diagonal).  Integer counts: deterministic.
#include "common.h"
#include "abx_rule.h"
#include "dtw_strip.h"

namespace cpc {
namespace {

constexpr int ABX_KC = 32;         // feature chunk staged in LDS per pass
constexpr int ABX_ACC = DTW_T * DTW_T / DTW_THREADS;   // distance entries per thread

// dt[r][c] = distance of frame row0 + r to frame col0 + c for r < R, c < C: acc over the feature dim, a k-ordered fma chain per
// entry.  Called by all threads of the workgroup; opens with a barrier before xs / ys / dt are rewritten, ends with one.
__device__ __forceinline__ void abx_distance_tile(const float *__restrict__ frames, int dp, long row0, int R, long col0, int C, int euclid,
                                                  float (*xs)[ABX_KC + 1], float (*ys)[ABX_KC + 1], float (*dt)[DTW_DT_STRIDE])
{
    const int tid = threadIdx.x;
    const int RC = R * C;
    float acc[ABX_ACC];
#pragma unroll
    for (int j = 0; j < ABX_ACC; ++j) acc[j] = 0.f;
    for (int k0 = 0; k0 < dp; k0 += ABX_KC) {
        const int kc4 = min(ABX_KC, dp - k0) >> 2;      // dp is a multiple of 4
        __syncthreads();                                 // previous users of xs / ys / dt are done
        for (int e = tid; e < R * kc4; e += DTW_THREADS) {
            const int r = e / kc4, k = (e - r * kc4) * 4;
            const float4 v = *reinterpret_cast<const float4 *>(frames + (row0 + r) * dp + k0 + k);
            xs[r][k] = v.x; xs[r][k + 1] = v.y; xs[r][k + 2] = v.z; xs[r][k + 3] = v.w;
        }
        for (int e = tid; e < C * kc4; e += DTW_THREADS) {
            const int c = e / kc4, k = (e - c * kc4) * 4;
            const float4 v = *reinterpret_cast<const float4 *>(frames + (col0 + c) * dp + k0 + k);
            ys[c][k] = v.x; ys[c][k + 1] = v.y; ys[c][k + 2] = v.z; ys[c][k + 3] = v.w;
        }
        __syncthreads();
        const int kc = kc4 * 4;
#pragma unroll
        for (int j = 0; j < ABX_ACC; ++j) {
            const int e = tid + j * DTW_THREADS;
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
        const int e = tid + j * DTW_THREADS;
        if (e < RC) {
            const int r = e / C, c = e - (e / C) * C;
            dt[r][c] = euclid ? sqrtf(acc[j]) : acosf(fminf(fmaxf(acc[j], -1.f), 1.f)) / 3.14159265358979323846f;
        }
    }
    __syncthreads();
}

// The shared recurrence and, for this walk, which returns nothing, the result written when the last cell is visited.  (A walk
// that returned the last cell instead left abx_dtw_kernel faster and sdtw_kernel 1 to 2 % slower: profiles/dtw_units_refactor.md.)
struct AbxDenseRule : AbxRule {
    int lx, ly, p;
    float *__restrict__ out;
    int *__restrict__ path_len;

    __device__ __forceinline__ AbxDenseRule(int lx, int ly, int p, float *out, int *path_len)
        : lx(lx), ly(ly), p(p), out(out), path_len(path_len)
    {
    }
    __device__ __forceinline__ void visit(int gi, int gj, const AbxCell &c) const
    {
        if (gi == lx - 1 && gj == ly - 1) {
            out[p] = c.v / (float)c.n[DTW_LEN];
            if (path_len) path_len[p] = c.n[DTW_LEN];
        }
    }
};

__global__ void __launch_bounds__(DTW_THREADS)
abx_dtw_kernel(const float *__restrict__ frames, int dp, const int *__restrict__ item_off, const int *__restrict__ item_len,
               int n_items, const int *__restrict__ seg_x, const int *__restrict__ seg_start, const int *__restrict__ pair_y,
               int n_seg, int max_len_y, int euclid, float *__restrict__ out, int *__restrict__ path_len, char *scratch)
{
    __shared__ float xs[DTW_T][ABX_KC + 1];
    __shared__ float ys[DTW_T][ABX_KC + 1];
    __shared__ float dt[DTW_T][DTW_DT_STRIDE];

    const DtwBoundary<ABX_W> bnd(scratch, max_len_y);
    for (int seg = blockIdx.x; seg < n_seg; seg += gridDim.x) {
        const DtwItem x = dtw_item(item_off, item_len, n_items, seg_x[seg]);
        for (int p = seg_start[seg]; p < seg_start[seg + 1]; ++p) {
            const DtwItem y = dtw_item(item_off, item_len, n_items, pair_y[p]);
            if (x.len < 1 || y.len < 1 || (x.len > DTW_T && (scratch == nullptr || y.len > max_len_y))) {
                if (threadIdx.x == 0) {                          // not computable: NaN never compares < or ==
                    out[p] = __builtin_nanf("");
                    if (path_len) path_len[p] = -1;
                }
                continue;
            }
            AbxDenseRule rule(x.len, y.len, p, out, path_len);
            dtw_walk_pair(bnd, x.len, y.len, dt, rule, [&](int rs, int R, int cb, int C) {
                abx_distance_tile(frames, dp, x.off + rs, R, y.off + cb, C, euclid, xs, ys, dt);
            });
        }
    }
}

__global__ void __launch_bounds__(DTW_THREADS)
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
        for (int e = threadIdx.x; e < total; e += DTW_THREADS) {
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

}  // namespace
}  // namespace cpc

extern "C" size_t cpc_abx_dtw_scratch_bytes(int n_seg, int max_len_x, int max_len_y)
{
    if (n_seg <= 0 || max_len_x <= 0 || max_len_y <= 0) return 0;
    if (max_len_x <= cpc::DTW_T) return 0;                       // one strip per item: no boundary row is stored
    return cpc::dtw_boundary_bytes(n_seg, max_len_y, cpc::ABX_W);
}

extern "C" int cpc_abx_dtw(const float *frames, int dp, const int *item_off, const int *item_len, int n_items,
                           const int *seg_x, const int *seg_start, const int *pair_y, int n_seg, int max_len_x,
                           int max_len_y, int distance, float *out, int *path_len, void *scratch, size_t scratch_bytes,
                           cpc_stream_t stream)
{
    CPC_TRY(cpc::dtw_check_args("abx_dtw",
                                frames != nullptr && item_off != nullptr && item_len != nullptr && seg_x != nullptr &&
                                    seg_start != nullptr && pair_y != nullptr && out != nullptr,
                                dp, distance, n_items, n_seg, "max_len_x", max_len_x, "max_len_y", max_len_y));
    const size_t need = cpc_abx_dtw_scratch_bytes(n_seg, max_len_x, max_len_y);
    CPC_REQUIRE(scratch_bytes >= need && (need == 0 || scratch != nullptr), "abx_dtw: scratch of %zu bytes, %zu needed",
                scratch_bytes, need);
    if (n_seg == 0) return CPC_OK;
    hipLaunchKernelGGL(cpc::abx_dtw_kernel, dim3((unsigned)cpc::dtw_grid(n_seg)), dim3(cpc::DTW_THREADS), 0,
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
    hipLaunchKernelGGL(cpc::abx_counts_kernel, dim3((unsigned)cpc::dtw_grid(n_trip)), dim3(cpc::DTW_THREADS), 0,
                       static_cast<hipStream_t>(stream), dist, n_pairs, idx_a, idx_b, shape, n_trip, lt, eq);
    CPC_CHECK_LAUNCH("abx_counts_kernel");
    return CPC_OK;
}
