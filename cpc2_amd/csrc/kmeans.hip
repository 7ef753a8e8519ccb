// k-means on CPC features (cpc/clustering/clustering.py of the reference): fused distance + argmin, the full distance
// matrix, and deterministic per-cluster sums.  DESIGN.md section 8 has the layout and the exactness argument.
//
//   kmeans_assign_kernel   one workgroup per 64 rows; centroids stream through LDS in 128-wide tiles, 16 features at a
//   kmeans_dist_kernel     time.  Each thread holds a 4 x 8 (rows x centroids) block of accumulators and reads its operands
//                          with ds_read_b128 (3 reads per 64 VALU).  Every distance is ONE f32 chain in ascending feature
//                          order, t = x - c; acc = fmaf(t, t, acc) -- never |x|^2 - 2 x.c + |c|^2.  Zero padding of the
//                          last feature chunk (both operands) adds exact zeros.  assign keeps (value, index) per row and
//                          merges across the 16 threads of a row group by comparing both, so the lowest index wins a tie
//                          (torch.argmin); dist stores the same accumulators, so the two agree bit for bit.
//   kmeans_bucket_kernel   stable bucketing of the rows by cluster.  Each wave owns a fixed range of rows and walks it 64
//                          at a time; lanes of one cluster find each other by ballots over the cluster id's bits.  Pass 1
//                          counts (integer atomics into hist[cluster][wave]); kmeans_scan_kernel turns the counts into
//                          start positions; pass 2 places each row at its cluster's start + its rank, so row ids land in
//                          ascending order inside every cluster whatever the arrival order.
//   kmeans_partial_kernel  one workgroup per chunk of <= 256 rows of one cluster: the chunk's row sum, rows in ascending
//                          order.  A cluster that owns every row is spread over n / 256 workgroups.
//   kmeans_combine_kernel  per cluster: its chunks' sums in chunk order, then sums += that, counts += rows.
// No float atomic anywhere: every result is bitwise reproducible.
#include "common.h"

#include <algorithm>

namespace cpc {
namespace {

constexpr int KM_THREADS = 256;
constexpr int KM_BM = 64;            // rows per workgroup
constexpr int KM_BN = 128;           // centroids per LDS tile
constexpr int KM_DK = 16;            // features per LDS chunk
constexpr int KM_TM = 4;             // rows per thread
constexpr int KM_TN = 8;             // centroids per thread (two groups of 4, 64 apart)
constexpr int KM_XS = KM_BM + 4;     // LDS row strides (floats): multiples of 4 for ds_read_b128, +4 against store conflicts
constexpr int KM_CS = KM_BN + 4;
constexpr int KM_XL = KM_BM * KM_DK / KM_THREADS;    // staged x elements per thread
constexpr int KM_CL = KM_BN * KM_DK / KM_THREADS;    // staged centroid elements per thread
constexpr int KM_CHUNK = 256;        // rows per partial sum
constexpr int KM_MAX_D = 4096;
constexpr int KM_MAX_K = 1 << 20;
constexpr long KM_HIST_MAX = 1 << 20;   // bound on k x waves of the bucketing (the scan runs in one workgroup)
constexpr int KM_WAVE_ROWS = 256;       // smallest row range of one bucketing wave
constexpr int KM_MAX_BLOCKS = 65536;

static_assert(KM_TM * KM_THREADS / 16 == KM_BM && KM_TN * 16 == KM_BN, "thread tile");

__device__ __forceinline__ bool better(float v, int i, float bv, int bi)
{
    return v < bv || (v == bv && i < bi);
}

// the shared tile: STORE = false -> index / min_sq, true -> dist [n][k]
template <bool STORE>
__device__ __forceinline__ void kmeans_tile(const float *__restrict__ x, long n, int d, const float *__restrict__ ck, int k, int *__restrict__ index,
            float *__restrict__ min_sq, float *__restrict__ dist)
{
    __shared__ __attribute__((aligned(16))) float xs[KM_DK * KM_XS];
    __shared__ __attribute__((aligned(16))) float cs[KM_DK * KM_CS];
    const int tid = threadIdx.x;
    const int tc = tid & 15;                       // centroid group: columns tc*4 .. +3 and 64 + tc*4 .. +3
    const int tr = tid >> 4;                       // row group: rows tr*4 .. +3
    const long row0 = (long)blockIdx.x * KM_BM;
    const int n_dc = (d + KM_DK - 1) / KM_DK;
    const int n_tiles = (k + KM_BN - 1) / KM_BN;
    const int n_steps = n_dc * n_tiles;

    float px[KM_XL], pc[KM_CL];
    auto fetch = [&](int step) {
        const int t0 = (step / n_dc) * KM_BN;
        const int d0 = (step % n_dc) * KM_DK;
#pragma unroll
        for (int i = 0; i < KM_XL; ++i) {
            const int e = tid + i * KM_THREADS;
            const long r = row0 + e / KM_DK;
            const int f = d0 + e % KM_DK;
            px[i] = (r < n && f < d) ? x[r * d + f] : 0.0f;
        }
#pragma unroll
        for (int i = 0; i < KM_CL; ++i) {
            const int e = tid + i * KM_THREADS;
            const int c = t0 + e / KM_DK;
            const int f = d0 + e % KM_DK;
            pc[i] = (c < k && f < d) ? ck[(long)c * d + f] : 0.0f;
        }
    };

    float acc[KM_TM][KM_TN];
    float bv[KM_TM];
    int bi[KM_TM];
#pragma unroll
    for (int i = 0; i < KM_TM; ++i) {
        bv[i] = __builtin_inff();
        bi[i] = 0x7fffffff;
#pragma unroll
        for (int j = 0; j < KM_TN; ++j) acc[i][j] = 0.0f;
    }

    fetch(0);
    for (int step = 0; step < n_steps; ++step) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < KM_XL; ++i) {
            const int e = tid + i * KM_THREADS;
            xs[(e % KM_DK) * KM_XS + e / KM_DK] = px[i];
        }
#pragma unroll
        for (int i = 0; i < KM_CL; ++i) {
            const int e = tid + i * KM_THREADS;
            cs[(e % KM_DK) * KM_CS + e / KM_DK] = pc[i];
        }
        __syncthreads();
        if (step + 1 < n_steps) fetch(step + 1);   // in flight while this chunk is consumed

#pragma unroll 4
        for (int kk = 0; kk < KM_DK; ++kk) {
            const float4 xv = *reinterpret_cast<const float4 *>(&xs[kk * KM_XS + tr * 4]);
            const float4 c0 = *reinterpret_cast<const float4 *>(&cs[kk * KM_CS + tc * 4]);
            const float4 c1 = *reinterpret_cast<const float4 *>(&cs[kk * KM_CS + 64 + tc * 4]);
            const float xa[KM_TM] = {xv.x, xv.y, xv.z, xv.w};
            const float ca[KM_TN] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
#pragma unroll
            for (int i = 0; i < KM_TM; ++i)
#pragma unroll
                for (int j = 0; j < KM_TN; ++j) {
                    const float t = xa[i] - ca[j];
                    acc[i][j] = fmaf(t, t, acc[i][j]);
                }
        }

        if (step % n_dc == n_dc - 1) {             // the tile's last feature chunk: epilogue, then fresh accumulators
            const int t0 = (step / n_dc) * KM_BN;
#pragma unroll
            for (int i = 0; i < KM_TM; ++i) {
                const long r = row0 + tr * 4 + i;
#pragma unroll
                for (int j = 0; j < KM_TN; ++j) {
                    const int c = t0 + (j < 4 ? tc * 4 + j : 64 + tc * 4 + j - 4);
                    if (STORE) {
                        if (r < n && c < k) dist[r * k + c] = acc[i][j];
                    } else if (c < k && better(acc[i][j], c, bv[i], bi[i])) {
                        bv[i] = acc[i][j];
                        bi[i] = c;
                    }
                    acc[i][j] = 0.0f;
                }
            }
        }
    }

    if (!STORE) {
#pragma unroll
        for (int i = 0; i < KM_TM; ++i) {
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) {       // the 16 lanes of a row group are consecutive
                const float ov = __shfl_xor(bv[i], o);
                const int oi = __shfl_xor(bi[i], o);
                if (better(ov, oi, bv[i], bi[i])) {
                    bv[i] = ov;
                    bi[i] = oi;
                }
            }
            const long r = row0 + tr * 4 + i;
            if (tc == 0 && r < n) {
                index[r] = bi[i] < k ? bi[i] : 0;   // (only NaN distances everywhere leave no winner)
                if (min_sq) min_sq[r] = bv[i];
            }
        }
    }
}

__global__ void __launch_bounds__(KM_THREADS)
kmeans_assign_kernel(const float *__restrict__ x, long n, int d, const float *__restrict__ ck, int k, int *__restrict__ index,
                     float *__restrict__ min_sq)
{
    kmeans_tile<false>(x, n, d, ck, k, index, min_sq, nullptr);
}

__global__ void __launch_bounds__(KM_THREADS)
kmeans_dist_kernel(const float *__restrict__ x, long n, int d, const float *__restrict__ ck, int k, float *__restrict__ dist)
{
    kmeans_tile<true>(x, n, d, ck, k, nullptr, nullptr, dist);
}

// Wave w owns rows [w * rows_per_wave, ...).  scatter = 0: hist[c * n_waves + w] += rows of cluster c in the range.
// scatter = 1: hist holds start positions (kmeans_scan_kernel); each row goes to perm[start + rank] and the start advances.
// One wave is the only user of its hist entries and walks its rows in order, so the placement is a function of the input.
__global__ void __launch_bounds__(KM_THREADS)
kmeans_bucket_kernel(const int *__restrict__ index, long n, int k, int bits, long rows_per_wave, int n_waves,
                     int *__restrict__ hist, int *__restrict__ perm, int scatter)
{
    const int w = blockIdx.x * (KM_THREADS / 64) + threadIdx.x / 64;
    if (w >= n_waves) return;
    const int lane = threadIdx.x & 63;
    const long begin = (long)w * rows_per_wave;
    const long end = min(n, begin + rows_per_wave);
    const unsigned long long below = (1ull << lane) - 1ull;
    for (long r0 = begin; r0 < end; r0 += 64) {
        const long row = r0 + lane;
        int c = -1;
        if (row < end) {
            c = index[row];
            if (c < 0 || c >= k) c = -1;             // out of range: skipped, counted nowhere
        }
        unsigned long long match = __ballot(c >= 0);
        for (int b = 0; b < bits; ++b) {
            const bool on = (c >> b) & 1;
            const unsigned long long m = __ballot(on);
            match &= on ? m : ~m;
        }
        const int leader = match ? __ffsll((long long)match) - 1 : lane;
        int base = 0;
        if (c >= 0 && lane == leader) {
            const int cnt = __popcll(match);
            if (scatter) base = atomicAdd(&hist[(long)c * n_waves + w], cnt);
            else atomicAdd(&hist[(long)c * n_waves + w], cnt);
        }
        if (scatter) {
            base = __shfl(base, c >= 0 ? leader : lane);
            if (c >= 0) perm[base + __popcll(match & below)] = (int)row;
        }
    }
}

// exclusive scan of v[0..len) in place by one workgroup; returns the total (to every thread)
__device__ long block_scan_inplace(int *v, long len, long *s_part)
{
    const int tid = threadIdx.x;
    const long per = (len + KM_THREADS - 1) / KM_THREADS;
    const long a = min(len, tid * per), b = min(len, a + per);
    long sum = 0;
    for (long i = a; i < b; ++i) sum += v[i];
    s_part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        long run = 0;
        for (int t = 0; t < KM_THREADS; ++t) {
            const long s = s_part[t];
            s_part[t] = run;
            run += s;
        }
        s_part[KM_THREADS] = run;
    }
    __syncthreads();
    long run = s_part[tid];
    for (long i = a; i < b; ++i) {
        const int s = v[i];
        v[i] = (int)run;
        run += s;
    }
    const long total = s_part[KM_THREADS];
    __syncthreads();
    return total;
}

// hist [k][n_waves] counts -> start positions (in place); off[c] = first position of cluster c, off[k] = rows placed;
// cstart[c] = first chunk of cluster c, cstart[k] = chunks in all
__global__ void __launch_bounds__(KM_THREADS)
kmeans_scan_kernel(int *__restrict__ hist, int k, int n_waves, int *__restrict__ off, int *__restrict__ cstart)
{
    __shared__ long s_part[KM_THREADS + 1];
    const long total = block_scan_inplace(hist, (long)k * n_waves, s_part);
    for (int c = threadIdx.x; c < k; c += KM_THREADS) off[c] = hist[(long)c * n_waves];
    if (threadIdx.x == 0) off[k] = (int)total;
    __syncthreads();
    for (int c = threadIdx.x; c < k; c += KM_THREADS) {
        const int rows = (c + 1 < k ? off[c + 1] : (int)total) - off[c];
        cstart[c] = (rows + KM_CHUNK - 1) / KM_CHUNK;
    }
    __syncthreads();
    const long chunks = block_scan_inplace(cstart, k, s_part);
    if (threadIdx.x == 0) cstart[k] = (int)chunks;
}

// chunk j -> partial[j][0..d): the sum of its <= KM_CHUNK rows in ascending row order
__global__ void __launch_bounds__(KM_THREADS)
kmeans_partial_kernel(const float *__restrict__ x, int d, int k, const int *__restrict__ perm, const int *__restrict__ off,
                      const int *__restrict__ cstart, float *__restrict__ partial)
{
    __shared__ int s_rows[KM_CHUNK];
    __shared__ int s_n;
    const int n_chunks = cstart[k];
    for (int j = blockIdx.x; j < n_chunks; j += gridDim.x) {
        if (threadIdx.x == 0) {
            int lo = 0, hi = k - 1;                  // the cluster c with cstart[c] <= j < cstart[c + 1]
            while (lo < hi) {
                const int mid = (lo + hi + 1) / 2;
                if (cstart[mid] <= j) lo = mid;
                else hi = mid - 1;
            }
            const int first = off[lo] + (j - cstart[lo]) * KM_CHUNK;
            s_n = min(KM_CHUNK, off[lo + 1] - first);
            s_rows[0] = first;
        }
        __syncthreads();
        const int first = s_rows[0], cnt = s_n;
        __syncthreads();
        if (threadIdx.x < cnt) s_rows[threadIdx.x] = perm[first + threadIdx.x];
        __syncthreads();
        for (int f = threadIdx.x; f < d; f += KM_THREADS) {
            float acc = 0.0f;
            for (int r = 0; r < cnt; ++r) acc += x[(long)s_rows[r] * d + f];
            partial[(long)j * d + f] = acc;
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(KM_THREADS)
kmeans_combine_kernel(int d, int k, const int *__restrict__ off, const int *__restrict__ cstart,
                      const float *__restrict__ partial, float *__restrict__ sums, int64_t *__restrict__ counts)
{
    for (int c = blockIdx.x; c < k; c += gridDim.x) {
        const int rows = off[c + 1] - off[c];
        if (rows == 0) continue;                     // sums and counts untouched
        const int j0 = cstart[c], j1 = cstart[c + 1];
        for (int f = threadIdx.x; f < d; f += KM_THREADS) {
            float acc = 0.0f;
            for (int j = j0; j < j1; ++j) acc += partial[(long)j * d + f];
            sums[(long)c * d + f] += acc;
        }
        if (threadIdx.x == 0) counts[c] += rows;
    }
}

struct BucketPlan {
    long rows_per_wave;
    int n_waves;
    long max_chunks;
};

BucketPlan bucket_plan(long n, int k)
{
    const long max_waves = std::max(1L, KM_HIST_MAX / k);
    long rpw = std::max((long)KM_WAVE_ROWS, cdiv(n, max_waves));
    rpw = cdiv(rpw, 64) * 64;
    return {rpw, (int)std::max(1L, cdiv(n, rpw)), n / KM_CHUNK + std::min((long)k, n) + 1};
}

bool kmeans_sizes_ok(long n, int d, int k)
{
    return n >= 0 && n < (1L << 31) && d >= 1 && d <= KM_MAX_D && k >= 1 && k <= KM_MAX_K;
}

}  // namespace
}  // namespace cpc

#define KM_REQUIRE_SIZES(what, n, d, k)                                                                               \
    CPC_REQUIRE(cpc::kmeans_sizes_ok(n, d, k), what ": sizes outside the supported limits (n=%ld d=%d k=%d; need "    \
                "0 <= n < 2^31, 1 <= d <= 4096, 1 <= k <= 2^20)", (long)(n), (int)(d), (int)(k))

extern "C" size_t cpc_kmeans_scratch_bytes(long n, int d, int k)
{
    if (!cpc::kmeans_sizes_ok(n, d, k)) return 0;
    const cpc::BucketPlan p = cpc::bucket_plan(n, k);
    cpc::Carver cv(nullptr);
    cv.take<int>((size_t)k * p.n_waves);             // hist / start positions
    cv.take<int>((size_t)k + 1);                     // off
    cv.take<int>((size_t)k + 1);                     // cstart
    cv.take<int>((size_t)std::max(1L, n));           // perm
    cv.take<float>((size_t)p.max_chunks * d);        // partial
    return cv.used();
}

extern "C" int cpc_kmeans_assign(const float *x, long n, int d, const float *ck, int k, int *index, float *min_sq,
                                 cpc_stream_t stream)
{
    KM_REQUIRE_SIZES("kmeans_assign", n, d, k);
    CPC_REQUIRE(x != nullptr && ck != nullptr && index != nullptr, "kmeans_assign: null buffer");
    if (n == 0) return CPC_OK;
    hipLaunchKernelGGL(cpc::kmeans_assign_kernel, dim3((unsigned)cpc::cdiv(n, cpc::KM_BM)), dim3(cpc::KM_THREADS), 0,
                       static_cast<hipStream_t>(stream), x, n, d, ck, k, index, min_sq);
    CPC_CHECK_LAUNCH("kmeans_assign_kernel");
    return CPC_OK;
}

extern "C" int cpc_kmeans_distances(const float *x, long n, int d, const float *ck, int k, float *dist, cpc_stream_t stream)
{
    KM_REQUIRE_SIZES("kmeans_distances", n, d, k);
    CPC_REQUIRE(x != nullptr && ck != nullptr && dist != nullptr, "kmeans_distances: null buffer");
    if (n == 0) return CPC_OK;
    hipLaunchKernelGGL(cpc::kmeans_dist_kernel, dim3((unsigned)cpc::cdiv(n, cpc::KM_BM)), dim3(cpc::KM_THREADS), 0,
                       static_cast<hipStream_t>(stream), x, n, d, ck, k, dist);
    CPC_CHECK_LAUNCH("kmeans_dist_kernel");
    return CPC_OK;
}

extern "C" int cpc_kmeans_accumulate(const float *x, long n, int d, const int *index, int k, float *sums, int64_t *counts,
                                     void *scratch, size_t scratch_bytes, cpc_stream_t stream)
{
    KM_REQUIRE_SIZES("kmeans_accumulate", n, d, k);
    CPC_REQUIRE(x != nullptr && index != nullptr && sums != nullptr && counts != nullptr, "kmeans_accumulate: null buffer");
    if (n == 0) return CPC_OK;
    const size_t need = cpc_kmeans_scratch_bytes(n, d, k);
    CPC_REQUIRE(scratch != nullptr && scratch_bytes >= need, "kmeans_accumulate: scratch of %zu bytes, %zu needed",
                scratch_bytes, need);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const cpc::BucketPlan p = cpc::bucket_plan(n, k);
    cpc::Carver cv(scratch);
    int *hist = cv.take<int>((size_t)k * p.n_waves);
    int *off = cv.take<int>((size_t)k + 1);
    int *cstart = cv.take<int>((size_t)k + 1);
    int *perm = cv.take<int>((size_t)std::max(1L, n));
    float *partial = cv.take<float>((size_t)p.max_chunks * d);
    int bits = 0;
    while ((1L << bits) < k) ++bits;
    const unsigned bucket_blocks = (unsigned)cpc::cdiv(p.n_waves, cpc::KM_THREADS / 64);
    CPC_CHECK_HIP(hipMemsetAsync(hist, 0, sizeof(int) * (size_t)k * p.n_waves, s));
    hipLaunchKernelGGL(cpc::kmeans_bucket_kernel, dim3(bucket_blocks), dim3(cpc::KM_THREADS), 0, s, index, n, k, bits,
                       p.rows_per_wave, p.n_waves, hist, perm, 0);
    CPC_CHECK_LAUNCH("kmeans_bucket_kernel");
    hipLaunchKernelGGL(cpc::kmeans_scan_kernel, dim3(1), dim3(cpc::KM_THREADS), 0, s, hist, k, p.n_waves, off, cstart);
    CPC_CHECK_LAUNCH("kmeans_scan_kernel");
    hipLaunchKernelGGL(cpc::kmeans_bucket_kernel, dim3(bucket_blocks), dim3(cpc::KM_THREADS), 0, s, index, n, k, bits,
                       p.rows_per_wave, p.n_waves, hist, perm, 1);
    CPC_CHECK_LAUNCH("kmeans_bucket_kernel");
    hipLaunchKernelGGL(cpc::kmeans_partial_kernel, dim3((unsigned)std::min<long>(p.max_chunks, cpc::KM_MAX_BLOCKS)),
                       dim3(cpc::KM_THREADS), 0, s, x, d, k, perm, off, cstart, partial);
    CPC_CHECK_LAUNCH("kmeans_partial_kernel");
    hipLaunchKernelGGL(cpc::kmeans_combine_kernel, dim3((unsigned)std::min(k, cpc::KM_MAX_BLOCKS)), dim3(cpc::KM_THREADS), 0,
                       s, d, k, off, cstart, partial, sums, counts);
    CPC_CHECK_LAUNCH("kmeans_combine_kernel");
    return CPC_OK;
}
