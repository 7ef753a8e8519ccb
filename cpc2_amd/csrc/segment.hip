// Unsupervised phone segmentation and its counts (cpc2_amd/segmentation.py): a boundary is hypothesised where
// consecutive frames stop resembling each other, and the hypotheses are matched against reference boundaries at a tolerance.
//
// The definition (restated from include/cpc2_hip.h).  One utterance has frames x[0..L) of D float32 columns.
//   d[t]   = 1 - dot(x_t, x_t+1) / sqrt(|x_t|^2 |x_t+1|^2) for t < L - 1, 1 when the product of the squared norms is 0; the three sums
//            in f64 (every product of two f32 values is exact there), then ONE product, square root, division and subtraction.
//   peaks  of d (n = L - 1 entries): i in [1, n - 2] starts one when d[i-1] < d[i] and the run of entries equal to d[i] is followed by
//            a smaller entry; its position is (first + last) / 2 of the run.  The first and last entries are never peaks.
//   prom   of a peak at q: walk left from q while d[i] <= d[q], keeping the minimum, the same to the right;
//            prom = d[q] - max(left minimum, right minimum).
//   kept   at threshold p: prom >= p * (max d - min d), ONE product (the file is built with -ffp-contract=off: a product fused
//            into a later operation would move the comparison); a kept peak at q is a boundary at frame q + 1.
//   counts per threshold against the sorted reference frames: n_hyp, the two-pointer one-to-one matching `hits`, and the lenient
//            hyp_near / ref_near (hypotheses with a reference within tol, references with a hypothesis within tol).
//
//   seg_dissimilarity_kernel   one wave per frame pair: lane j sums the columns j, j + 64, ... in order, then a fixed xor butterfly
//                              over the 64 lanes.  The tree depends on D alone and is symmetric in the two rows, so equal pairs
//                              of rows give equal bits wherever they stand.  A non-finite row makes its pairs NaN and the
//                              utterance's status 2 (an integer atomicMax: the order does not matter).
//   seg_boundaries_kernel      one workgroup per utterance.  d is staged in LDS up to SEG_LDS_CAP entries (read in place beyond),
//                              min / max by shuffles, one candidate per thread with the plateau scan, compaction in index order by
//                              a ballot + prefix over the waves, one thread per peak for the two walks, then ONE LANE PER
//                              THRESHOLD for the sequential selection and matching: the K thresholds run side by side and the
//                              counts are plain integer stores.
// No float atomic: two launches give the same bytes.
#include "common.h"

namespace cpc {
namespace {

constexpr int SEG_THREADS = 256;
constexpr int SEG_WAVES = SEG_THREADS / 64;
constexpr int SEG_ROWS_PER_BLOCK = 32;              // frame pairs per workgroup of the dissimilarity kernel (8 per wave)
constexpr int SEG_LDS_CAP = 6144;                   // entries of d staged in LDS: 48 KiB of the 64 KiB a workgroup may take
constexpr int SEG_MAX_K = 64;                       // thresholds: one lane of the first wave each
constexpr int SEG_MAX_LEN = 1 << 20;                // frames per utterance (2.9 h at 10 ms)
constexpr int SEG_MAX_UTT = 1 << 20;
constexpr int SEG_MAX_TOL = 1 << 30;
enum { SEG_OK = 0, SEG_BAD = 2 };

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

__device__ __forceinline__ bool finite64(double v) { return v - v == 0.0; }

__global__ void __launch_bounds__(SEG_THREADS)
seg_dissimilarity_kernel(const float *__restrict__ x, long total_rows, long ld, int D, const int64_t *__restrict__ offsets,
                         const int *__restrict__ lengths, int max_len, double *__restrict__ d, int *__restrict__ status)
{
    const int utt = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t off = offsets[utt];
    const int L = lengths[utt];
    if (L < 0 || L > max_len || off < 0 || off > total_rows || (int64_t)L > total_rows - off) {
        if (blockIdx.y == 0 && threadIdx.x == 0) atomicMax(&status[utt], (int)SEG_BAD);
        return;
    }
    const int t0 = blockIdx.y * SEG_ROWS_PER_BLOCK;
    // row t < L: its pair with row t + 1 when there is one; the last row is only looked at (a single-frame utterance has no pair)
    for (int t = t0 + wave; t < min(t0 + SEG_ROWS_PER_BLOCK, L); t += SEG_WAVES) {
        const float *a = x + (size_t)(off + t) * ld;
        const bool pair = t + 1 < L;
        const float *b = pair ? a + ld : a;
        double dot = 0.0, na = 0.0, nb = 0.0;
        for (int c = lane; c < D; c += 64) {
            const double va = (double)a[c], vb = (double)b[c];
            dot += va * vb;
            na += va * va;
            nb += vb * vb;
        }
        dot = wave_sum(dot);
        na = wave_sum(na);
        nb = wave_sum(nb);
        const bool ok = finite64(na) && finite64(nb);      // (a sum of f32 squares in f64 cannot overflow: non-finite <=> an element is)
        if (lane == 0) {
            if (!ok) atomicMax(&status[utt], (int)SEG_BAD);
            if (pair) {
                const double prod = na * nb;
                double v = 1.0;
                if (!ok) v = __builtin_nan("");
                else if (prod != 0.0) v = 1.0 - dot / sqrt(prod);
                d[off + t] = v;
            }
        }
    }
}

// exclusive prefix of one flag per thread in thread order, and the total; s_cnt has SEG_WAVES + 1 ints
__device__ __forceinline__ int block_rank(bool flag, int *s_cnt, int *total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(flag);
    if (lane == 0) s_cnt[wave] = __popcll(m);
    __syncthreads();
    int base = 0, all = 0;
#pragma unroll
    for (int w = 0; w < SEG_WAVES; ++w) {
        const int c = s_cnt[w];
        if (w < wave) base += c;
        all += c;
    }
    __syncthreads();                                                 // (s_cnt is written again by the next call)
    *total = all;
    return base + __popcll(m & ((1ull << lane) - 1ull));
}

__global__ void __launch_bounds__(SEG_THREADS)
seg_boundaries_kernel(const double *__restrict__ d_all, long total_rows, const int64_t *__restrict__ offsets,
                      const int *__restrict__ lengths, const double *__restrict__ thresholds, int K, const int *__restrict__ ref,
                      long total_ref, const int64_t *__restrict__ ref_offsets, const int *__restrict__ ref_counts,
                      const int *__restrict__ hyp_limit, int tol, int *__restrict__ n_peaks, int *__restrict__ peak_pos,
                      double *__restrict__ peak_prom, double *__restrict__ range, int *__restrict__ counts, int *__restrict__ status)
{
    __shared__ double s_d[SEG_LDS_CAP];
    __shared__ double s_lo[SEG_WAVES], s_hi[SEG_WAVES];
    __shared__ int s_cnt[SEG_WAVES + 1];
    __shared__ int s_bad;
    const int tid = threadIdx.x;
    const int utt = blockIdx.x;
    const int64_t off = offsets[utt];
    const int L = lengths[utt];
    bool bad = L < 0 || L > SEG_MAX_LEN || off < 0 || off > total_rows || (int64_t)L > total_rows - off;
    int n_ref = 0;
    const int *refs = nullptr;
    if (ref != nullptr) {
        const int64_t ro = ref_offsets[utt];
        n_ref = ref_counts[utt];
        if (n_ref < 0 || ro < 0 || ro > total_ref || (int64_t)n_ref > total_ref - ro) { bad = true; n_ref = 0; }
        else refs = ref + ro;
    }
    const int n = (bad || L < 1) ? 0 : L - 1;
    const double *dg = d_all + (bad ? 0 : off);
    int *pos = peak_pos + (bad ? 0 : off);
    double *prom = peak_prom + (bad ? 0 : off);

    // ---- stage, min / max, finiteness
    const bool staged = n <= SEG_LDS_CAP;
    double lo = __builtin_inf(), hi = -__builtin_inf();
    int nonfinite = 0;
    for (int i = tid; i < n; i += SEG_THREADS) {
        const double v = dg[i];
        if (staged) s_d[i] = v;
        if (!finite64(v)) nonfinite = 1;
        lo = fmin(lo, v);
        hi = fmax(hi, v);
    }
    if (tid == 0) s_bad = 0;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {                              // (min and max are exact: any order gives the same value)
        lo = fmin(lo, __shfl_xor(lo, m, 64));
        hi = fmax(hi, __shfl_xor(hi, m, 64));
    }
    if ((tid & 63) == 0) { s_lo[tid >> 6] = lo; s_hi[tid >> 6] = hi; }
    __syncthreads();
    if (nonfinite) s_bad = 1;                                        // (benign race: all store 1)
    __syncthreads();
#pragma unroll
    for (int w = 0; w < SEG_WAVES; ++w) {
        lo = fmin(lo, s_lo[w]);
        hi = fmax(hi, s_hi[w]);
    }
    bad = bad || s_bad != 0;
    if (bad || n == 0) {
        if (tid == 0) {
            n_peaks[utt] = 0;
            range[utt] = bad ? __builtin_nan("") : 0.0;
            status[utt] = bad ? SEG_BAD : SEG_OK;
        }
        if (tid < K)
            for (int c = 0; c < 4; ++c) counts[((size_t)utt * K + tid) * 4 + c] = 0;
        return;
    }
    const double rng = hi - lo;
    const double *dp = staged ? s_d : dg;                            // (a generic pointer: LDS or global)

    // ---- candidates in index order: thread i looks at entry i of the chunk, the peaks' positions go out compacted
    int found = 0;
    for (int base = 0; base < n; base += SEG_THREADS) {
        const int i = base + tid;
        bool is_peak = false;
        int q = 0;
        if (i >= 1 && i <= n - 2) {
            const double v = dp[i];
            if (dp[i - 1] < v) {
                int r = i + 1;
                while (r < n && dp[r] == v) ++r;                     // r: the first entry behind the run, or n
                if (r < n && dp[r] < v) { is_peak = true; q = (i + r - 1) / 2; }
            }
        }
        int total;
        const int rank = block_rank(is_peak, s_cnt, &total);
        if (is_peak) pos[found + rank] = q;
        found += total;
    }
    __syncthreads();                                                 // (orders the workgroup's global writes of pos before its reads)

    // ---- prominences: one thread per peak
    for (int j = tid; j < found; j += SEG_THREADS) {
        const int q = pos[j];
        const double v = dp[q];
        double lmin = v, rmin = v;
        for (int i = q - 1; i >= 0; --i) {
            const double w = dp[i];
            if (w > v) break;
            lmin = fmin(lmin, w);
        }
        for (int i = q + 1; i < n; ++i) {
            const double w = dp[i];
            if (w > v) break;
            rmin = fmin(rmin, w);
        }
        prom[j] = v - fmax(lmin, rmin);
    }
    if (tid == 0) {
        n_peaks[utt] = found;
        range[utt] = rng;
        status[utt] = SEG_OK;
    }
    __syncthreads();                                                 // (orders the workgroup's global writes of prom before its reads)

    // ---- one lane per threshold: selection, the one-to-one matching and the lenient counts, all in one pass over the peaks.  The
    //      lanes walk the peaks in step (a broadcast) and each its own three reference pointers
    if (tid < K) {
        const double cut = thresholds[tid] * rng;
        const int limit = hyp_limit != nullptr ? hyp_limit[utt] : L;  // hypotheses at frames >= limit are dropped
        const long long tl = tol;
        int n_hyp = 0, hits = 0, hyp_near = 0, ref_near = 0;
        int im = 0, ia = 0, ib = 0;                                  // the matching's, hyp_near's and ref_near's reference pointers
        for (int j = 0; j < found; ++j) {
            const long long h = (long long)pos[j] + 1;
            const double pr = prom[j];
            if (!(pr >= cut) || h >= limit) continue;
            ++n_hyp;
            while (im < n_ref) {
                const long long r = refs[im];
                const long long gap = h > r ? h - r : r - h;
                if (gap <= tl) { ++hits; ++im; break; }
                if (h < r) break;
                ++im;
            }
            while (ia < n_ref && refs[ia] < h - tl) ++ia;
            if (ia < n_ref && refs[ia] <= h + tl) ++hyp_near;
            while (ib < n_ref && refs[ib] < h - tl) ++ib;
            while (ib < n_ref && refs[ib] <= h + tl) { ++ref_near; ++ib; }
        }
        int *c = counts + ((size_t)utt * K + tid) * 4;
        c[0] = n_hyp;
        c[1] = hits;
        c[2] = hyp_near;
        c[3] = ref_near;
    }
}

}  // namespace
}  // namespace cpc

extern "C" int cpc_seg_dissimilarity(const float *x, long total_rows, long ld, int dim, const int64_t *offsets, const int *lengths,
                                     int n_utt, int max_len, double *d, int *status, cpc_stream_t stream)
{
    CPC_REQUIRE(dim >= 1 && ld >= dim && total_rows >= 0 && n_utt >= 1 && n_utt <= cpc::SEG_MAX_UTT && max_len >= 0 &&
                    max_len <= cpc::SEG_MAX_LEN,
                "seg_dissimilarity: sizes outside the supported limits (total_rows=%ld ld=%ld dim=%d n_utt=%d max_len=%d; need dim >= 1, "
                "ld >= dim, total_rows >= 0, 1 <= n_utt <= %d, 0 <= max_len <= %d)", total_rows, ld, dim, n_utt, max_len,
                cpc::SEG_MAX_UTT, cpc::SEG_MAX_LEN);
    CPC_REQUIRE(offsets && lengths && d && status && (x || total_rows == 0), "seg_dissimilarity: null buffer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    CPC_CHECK_HIP(hipMemsetAsync(status, 0, sizeof(int) * (size_t)n_utt, st));
    const unsigned tiles = (unsigned)cpc::cdiv(max_len > 0 ? max_len : 1, cpc::SEG_ROWS_PER_BLOCK);
    hipLaunchKernelGGL(cpc::seg_dissimilarity_kernel, dim3((unsigned)n_utt, tiles), dim3(cpc::SEG_THREADS), 0, st, x, total_rows, ld,
                       dim, offsets, lengths, max_len, d, status);
    CPC_CHECK_LAUNCH("seg_dissimilarity_kernel");
    return CPC_OK;
}

extern "C" int cpc_seg_lds_entries(void) { return cpc::SEG_LDS_CAP; }

extern "C" int cpc_seg_boundaries(const double *d, long total_rows, const int64_t *offsets, const int *lengths, int n_utt,
                                  const double *thresholds, int k, const int *ref, long total_ref, const int64_t *ref_offsets,
                                  const int *ref_counts, const int *hyp_limit, int tol, int *n_peaks, int *peak_pos, double *peak_prom,
                                  double *range, int *counts, int *status, cpc_stream_t stream)
{
    CPC_REQUIRE(total_rows >= 0 && n_utt >= 1 && n_utt <= cpc::SEG_MAX_UTT && k >= 1 && k <= cpc::SEG_MAX_K && tol >= 0 &&
                    tol <= cpc::SEG_MAX_TOL && total_ref >= 0,
                "seg_boundaries: sizes outside the supported limits (total_rows=%ld n_utt=%d k=%d tol=%d total_ref=%ld; need "
                "total_rows >= 0, 1 <= n_utt <= %d, 1 <= k <= %d, 0 <= tol <= %d, total_ref >= 0)", total_rows, n_utt, k, tol,
                total_ref, cpc::SEG_MAX_UTT, cpc::SEG_MAX_K, cpc::SEG_MAX_TOL);
    CPC_REQUIRE(offsets && lengths && thresholds && n_peaks && range && counts && status &&
                    ((d && peak_pos && peak_prom) || total_rows == 0),
                "seg_boundaries: null buffer");
    CPC_REQUIRE(ref == nullptr || (ref_offsets && ref_counts), "seg_boundaries: ref given without ref_offsets and ref_counts");
    hipLaunchKernelGGL(cpc::seg_boundaries_kernel, dim3((unsigned)n_utt), dim3(cpc::SEG_THREADS), 0, static_cast<hipStream_t>(stream),
                       d, total_rows, offsets, lengths, thresholds, k, ref, total_ref, ref_offsets, ref_counts, hyp_limit, tol,
                       n_peaks, peak_pos, peak_prom, range, counts, status);
    CPC_CHECK_LAUNCH("seg_boundaries_kernel");
    return CPC_OK;
}
