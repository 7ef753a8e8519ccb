// Loss heads of the linear-separability probe (cpc/eval/linear_separability.py of the reference): softmax cross-entropy
// with accuracy (PhoneCriterion / SpeakerCriterion), CTC (CTCPhoneCriterion) and the label collapse in front of it.
// DESIGN.md section 9 has the layout and the exactness argument.
//
//   probe_xent_kernel      one wave64 per row of logits [n][c]: lane j visits columns j, j + 64, ... in order keeping an online
//                          (max, sum of exp) pair and the first maximum; the 64 lanes merge by a butterfly whose merge is
//                          symmetric, so every lane ends with the same bits.  nll = max + log(sum) - x[label]; the prediction
//                          is the LOWEST index among equal maxima (predictions.max(1)[1]).  With a gradient wanted the row is
//                          overwritten by (softmax - onehot) / n.
//   cpc_probe_ctc          no kernel of its own: the CTC loss of ctc_head.hip (cpc::ctc_loss_run) with every frame of every
//                          sequence counted and the mean reduction.
//   probe_reduce_kernel    the mean cross-entropy as one workgroup's fixed-order sum, and the number of correct rows (integers).
//   probe_collapse_kernel  one wave64 per row: consecutive repeats removed (ballot + popcount), zero padded.
//   probe_scale_kernel     dlogits *= the loss's incoming gradient (a device scalar: no host read).
// No float atomic anywhere: every result is bitwise reproducible.
#include "common.h"

#include <algorithm>

namespace cpc {
namespace {

constexpr int PR_THREADS = 256;
constexpr int PR_ROWS = PR_THREADS / 64;     // xent / collapse rows per workgroup (one wave each)
constexpr int PR_MAX_C = 1 << 20;
constexpr int PR_CTC_MAX_B = 65535;          // the probe's own CTC limits, inside cpc_ctc_loss's
constexpr int PR_CTC_MAX_T = 1024;
constexpr int PR_CTC_MAX_K = 1 << 16;

__device__ __forceinline__ bool first_max(float v, int i, float bv, int bi)
{
    return v > bv || (v == bv && i < bi);
}

// (m, s) <- the pair of the union: m = max, s = sum of exp(x - m); an empty side has m = -inf, s = 0
__device__ __forceinline__ void lse_merge(float &m, float &s, float om, float os)
{
    const float nm = fmaxf(m, om);
    if (nm == -__builtin_inff()) return;
    const float a = m == -__builtin_inff() ? 0.0f : s * expf(m - nm);
    const float b = om == -__builtin_inff() ? 0.0f : os * expf(om - nm);
    m = nm;
    s = a + b;
}

__global__ void __launch_bounds__(PR_THREADS)
probe_xent_kernel(float *logits, const int64_t *__restrict__ labels, long n, int c, int want_grad, float *__restrict__ nll,
                  int *__restrict__ correct)
{
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * PR_ROWS + (threadIdx.x >> 6);
    if (row >= n) return;                              // (the whole wave)
    float *x = logits + row * c;
    const int64_t y64 = labels[row];
    const int y = (y64 >= 0 && y64 < c) ? (int)y64 : -1;
    float m = -__builtin_inff(), s = 0.0f, bv = -__builtin_inff(), xy = 0.0f;
    int bi = 0x7fffffff;
    for (int j = lane; j < c; j += 64) {
        const float v = x[j];
        if (j == y) xy = v;
        if (first_max(v, j, bv, bi)) {
            bv = v;
            bi = j;
        }
        if (v > m) {
            s = (m == -__builtin_inff() ? 0.0f : s * expf(m - v)) + 1.0f;
            m = v;
        } else {
            s += expf(v - m);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lse_merge(m, s, __shfl_xor(m, o), __shfl_xor(s, o));
        const float ov = __shfl_xor(bv, o);
        const int oi = __shfl_xor(bi, o);
        if (first_max(ov, oi, bv, bi)) {
            bv = ov;
            bi = oi;
        }
    }
    const float lse = m + logf(s);
    if (y >= 0) xy = __shfl(xy, y & 63);
    if (lane == 0) {
        nll[row] = y >= 0 ? lse - xy : __builtin_nanf("");
        correct[row] = (y >= 0 && bi == y) ? 1 : 0;
    }
    if (want_grad) {
        const float inv_n = 1.0f / (float)n;
        for (int j = lane; j < c; j += 64) {
            const float p = expf(x[j] - lse);
            x[j] = ((j == y ? p - 1.0f : p)) * inv_n;
        }
    }
}

// loss[0] = (sum_i vals[i]) / n, fixed order; acc[0] = (sum_i correct[i]) / n in double
__global__ void __launch_bounds__(PR_THREADS)
probe_reduce_kernel(const float *__restrict__ vals, const int *__restrict__ correct, long n, float *__restrict__ loss,
                    double *__restrict__ acc)
{
    __shared__ float s_sum[PR_THREADS];
    __shared__ long s_cnt[PR_THREADS];
    const int tid = threadIdx.x;
    float sum = 0.0f;
    long cnt = 0;
    for (long i = tid; i < n; i += PR_THREADS) {
        sum += vals[i];
        cnt += correct[i];
    }
    s_sum[tid] = sum;
    s_cnt[tid] = cnt;
    __syncthreads();
    for (int w = PR_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) {
            s_sum[tid] += s_sum[tid + w];
            s_cnt[tid] += s_cnt[tid + w];
        }
        __syncthreads();
    }
    if (tid == 0) {
        loss[0] = s_sum[0] / (float)n;
        acc[0] = (double)s_cnt[0] / (double)n;
    }
}

__global__ void probe_scale_kernel(float *x, long n, const float *__restrict__ scale)
{
    const float f = scale[0];
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) x[i] *= f;
}

__global__ void __launch_bounds__(PR_THREADS)
probe_collapse_kernel(const int64_t *__restrict__ in, int b, int t, int64_t *__restrict__ out, long ldo,
                      int64_t *__restrict__ lengths)
{
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * PR_ROWS + (threadIdx.x >> 6);
    if (row >= b) return;
    const int64_t *x = in + row * t;
    int64_t *o = out + row * ldo;
    const unsigned long long below = (1ull << lane) - 1ull;
    long base = 0;
    for (int t0 = 0; t0 < t; t0 += 64) {
        const int i = t0 + lane;
        const int64_t v = i < t ? x[i] : 0;
        const bool keep = i < t && (i == 0 || v != x[i - 1]);
        const unsigned long long mask = __ballot(keep);
        if (keep) o[base + __popcll(mask & below)] = v;
        base += __popcll(mask);
    }
    for (long p = base + lane; p < ldo; p += 64) o[p] = 0;
    if (lane == 0) lengths[row] = base;
}

}  // namespace
}  // namespace cpc

extern "C" size_t cpc_probe_xent_backward_scratch_bytes(int c)
{
    return c >= 1 && c <= cpc::PR_MAX_C ? cpc::colsum_rows_scratch_bytes(c) : 0;
}

extern "C" int cpc_probe_xent(float *logits, const int64_t *labels, long n, int c, int want_grad, float *nll, int *correct,
                              float *loss, double *acc, cpc_stream_t stream)
{
    CPC_REQUIRE(n >= 1 && n < (1L << 31) && c >= 1 && c <= cpc::PR_MAX_C,
                "probe_xent: sizes outside the supported limits (n=%ld c=%d; need 1 <= n < 2^31, 1 <= c <= 2^20)", n, c);
    CPC_REQUIRE(logits && labels && nll && correct && loss && acc, "probe_xent: null buffer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(cpc::probe_xent_kernel, dim3((unsigned)cpc::cdiv(n, cpc::PR_ROWS)), dim3(cpc::PR_THREADS), 0, st, logits,
                       labels, n, c, want_grad, nll, correct);
    CPC_CHECK_LAUNCH("probe_xent_kernel");
    hipLaunchKernelGGL(cpc::probe_reduce_kernel, dim3(1), dim3(cpc::PR_THREADS), 0, st, nll, correct, n, loss, acc);
    CPC_CHECK_LAUNCH("probe_reduce_kernel");
    return CPC_OK;
}

extern "C" int cpc_probe_head_backward(float *dlogits, long n, int c, const float *dloss, float *db, void *scratch,
                                       size_t scratch_bytes, cpc_stream_t stream)
{
    CPC_REQUIRE(n >= 1 && c >= 1 && c <= cpc::PR_MAX_C, "probe_head_backward: sizes outside the supported limits (n=%ld c=%d)", n, c);
    CPC_REQUIRE(dlogits != nullptr, "probe_head_backward: null buffer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dloss != nullptr) {
        const long total = n * c;
        const unsigned blocks = (unsigned)std::min<long>(cpc::cdiv(total, 256), 2048);
        hipLaunchKernelGGL(cpc::probe_scale_kernel, dim3(blocks), dim3(256), 0, st, dlogits, total, dloss);
        CPC_CHECK_LAUNCH("probe_scale_kernel");
    }
    if (db != nullptr) {
        CPC_REQUIRE(scratch != nullptr && scratch_bytes >= cpc::colsum_rows_scratch_bytes(c),
                    "probe_head_backward: scratch of %zu bytes, %zu needed", scratch_bytes, cpc::colsum_rows_scratch_bytes(c));
        CPC_TRY(cpc::colsum_rows(dlogits, c, n, c, db, scratch, st));
    }
    return CPC_OK;
}

extern "C" size_t cpc_probe_ctc_scratch_bytes(int b, int t, int max_l)
{
    if (b < 1 || b > cpc::PR_CTC_MAX_B || t < 1 || t > cpc::PR_CTC_MAX_T || max_l < 0 || max_l > t) return 0;
    return cpc_ctc_loss_scratch_bytes(b, t, max_l);      // (the same kernels' room: these sizes lie inside its limits)
}

extern "C" int cpc_probe_ctc(const float *logits, int b, int t, int k, const int64_t *targets, int max_l, const int64_t *lengths,
                             float *nll, float *loss, float *dlogits, void *scratch, size_t scratch_bytes, cpc_stream_t stream)
{
    CPC_REQUIRE(b >= 1 && b <= cpc::PR_CTC_MAX_B && t >= 1 && t <= cpc::PR_CTC_MAX_T && k >= 2 && k <= cpc::PR_CTC_MAX_K &&
                max_l >= 0 && max_l <= t,
                "probe_ctc: sizes outside the supported limits (b=%d t=%d k=%d max_l=%d; need 1 <= b <= %d, 1 <= t <= %d, "
                "2 <= k <= %d, 0 <= max_l <= t)", b, t, k, max_l, cpc::PR_CTC_MAX_B, cpc::PR_CTC_MAX_T, cpc::PR_CTC_MAX_K);
    CPC_REQUIRE(logits && lengths && nll && loss && (targets || max_l == 0), "probe_ctc: null buffer");
    const size_t need = cpc_probe_ctc_scratch_bytes(b, t, max_l);
    CPC_REQUIRE(scratch != nullptr && scratch_bytes >= need, "probe_ctc: scratch of %zu bytes, %zu needed", scratch_bytes, need);
    // every frame of every sequence counts (no input lengths), mean reduction
    return cpc::ctc_loss_run(logits, b, t, k, nullptr, targets, max_l, lengths, 1, nll, loss, dlogits, scratch,
                             static_cast<hipStream_t>(stream));
}

extern "C" int cpc_probe_collapse(const int64_t *labels, int b, int t, int64_t *out, long ldo, int64_t *lengths,
                                  cpc_stream_t stream)
{
    CPC_REQUIRE(b >= 1 && t >= 1 && ldo >= t, "probe_collapse: sizes outside the supported limits (b=%d t=%d ldo=%ld; need ldo >= t)",
                b, t, ldo);
    CPC_REQUIRE(labels && out && lengths, "probe_collapse: null buffer");
    hipLaunchKernelGGL(cpc::probe_collapse_kernel, dim3((unsigned)cpc::cdiv(b, cpc::PR_ROWS)), dim3(cpc::PR_THREADS), 0,
                       static_cast<hipStream_t>(stream), labels, b, t, out, ldo, lengths);
    CPC_CHECK_LAUNCH("probe_collapse_kernel");
    return CPC_OK;
}
