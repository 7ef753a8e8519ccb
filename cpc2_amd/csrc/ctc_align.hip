// CTC forced alignment of whole utterances (cpc2_amd/seq_alignment.py: ctc_forced_align): the best path
// through the lattice that cpc_ctc_loss sums over, with max in place of log-sum-exp and a backtrace.
//
// The definition (restated from include/cpc2_hip.h).  One sequence has logits x [T][k] (f32), targets y[0..L), blank = k - 1.
// Extended states s in [0, 2 L + 1): sym(s) = blank for even s, y[s / 2] for odd s.  Every alignment emits exactly one symbol per
// frame, so sum_t lse_t is the same for all paths: the maximisation runs on the raw logits, no exp or log inside the recurrence.
//   start  v[0][0] = (double) x[0][blank]; v[0][1] = (double) x[0][y0] when L >= 1; every other state -inf
//   step   v[t][s] = max(v[t-1][s], v[t-1][s-1] when s >= 1, v[t-1][s-2] when s is odd, s >= 3 and y[s/2] != y[s/2 - 1])
//                    + (double) x[t][sym(s)]: all f64, the max first, then ONE addition.  The file is built with
//          -ffp-contract=off like seqalign.hip, so a host program with the same operation order gives the same bits.
//   ties   among equal finite candidates staying in s wins over s - 1, which wins over s - 2; at the end state 2 L wins over
//          2 L - 1 unless v[T-1][2L-1] is strictly larger.  ties = 1 when a maximum ON THE RETURNED PATH (the end included) had an
//          equal finite competitor.
//
//   ctc_align_kernel     one workgroup per sequence.  The extended states and the frames' log-sum-exp in f64 first (one wave per
//                        frame, max-shifted: ctc_lattice.h, shared with ctc_len_kernel), then the recurrence: the 2 L + 1 values double-buffered in LDS next to the symbol table
//                        (41 KB at 1024 labels), threads strided over the states, one barrier per frame; the logit a state adds
//                        in frame t + 1 is fetched while frame t is computed.  Only the states of the reachable band
//                        2 L - 2 (T - 1 - t) - 1 <= s <= 2 t + 1 are computed: a state reads only states of the previous
//                        frame's band or -inf, so the band's values are the full table's.  A back-pointer (2 bits of move, 1 tie
//                        bit) per (frame, state) goes to global scratch, one byte per cell.  The backtrace takes blocks of 32
//                        frames: a state moves by at most 2 per frame, so the workgroup fetches 32 frames x 65 states below the
//                        current state into LDS and one lane walks them there.
//   ctc_segments_kernel  per token the first and last frame in its state and the mean of x[t][y] - lse_t over them, summed in f64
//                        in frame order by one thread.
// No float atomic: two launches give the same bytes.  Frames at or beyond an input length and target padding are never read.
#include "common.h"
#include "ctc_lattice.h"

#include <algorithm>

namespace cpc {
namespace {

constexpr int CA_THREADS = 256;
constexpr int CA_MAX_T = 4096;
constexpr int CA_MAX_L = 1024;
constexpr int CA_MAX_S = 2 * CA_MAX_L + 1;
constexpr int CA_MAX_K = 1 << 16;
constexpr int CA_PER = (CA_MAX_S + CA_THREADS - 1) / CA_THREADS;     // states per thread
constexpr int CA_BLOCK_T = 32;                                      // frames per block of the backtrace
constexpr int CA_BLOCK_S = 2 * CA_BLOCK_T + 1;                      // states a walk of CA_BLOCK_T frames can visit
enum { CA_ALIGNED = 0, CA_NO_ALIGNMENT = 1, CA_BAD = 2 };

__global__ void __launch_bounds__(CA_THREADS)
ctc_align_kernel(const float *__restrict__ logits, int t_max, int K, const int64_t *__restrict__ in_lengths,
                 const int64_t *__restrict__ targets, int max_l, const int64_t *__restrict__ tgt_lengths, int *__restrict__ path,
                 double *__restrict__ score, int *__restrict__ status, int *__restrict__ ties, double *__restrict__ lse_all,
                 unsigned char *__restrict__ bp_all)
{
    __shared__ double s_v[2][CA_MAX_S];
    __shared__ int s_ext[CA_MAX_S];
    __shared__ unsigned char s_tile[CA_BLOCK_T][CA_BLOCK_S + 3];
    __shared__ double s_red[CA_THREADS];
    __shared__ int s_bad, s_rep, s_state, s_tie;
    const int tid = threadIdx.x;
    const int seq = blockIdx.x;
    const int blank = K - 1;
    const int sw = 2 * max_l + 1;
    const float *x = logits + (size_t)seq * t_max * K;
    unsigned char *bp = bp_all + (size_t)seq * t_max * sw;
    double *lse = lse_all + (size_t)seq * t_max;
    int *pth = path + (size_t)seq * t_max;
    const int64_t l64 = tgt_lengths[seq];
    const int64_t t64 = in_lengths[seq];
    const bool len_ok = l64 >= 0 && l64 <= max_l && t64 >= 0 && t64 <= t_max;
    const int L = len_ok ? (int)l64 : 0;
    const int T = len_ok ? (int)t64 : 0;
    const int S = 2 * L + 1;
    const double neg_inf = -__builtin_inf();

    if (tid == 0) { s_bad = len_ok ? 0 : 1; s_rep = 0; }
    __syncthreads();
    if (load_ext_states<CA_THREADS>(targets + (size_t)seq * max_l, S, blank, s_ext)) s_bad = 1;      // (benign race: all store 1)
    __syncthreads();
    for (int i = 1 + tid; i < L; i += CA_THREADS)
        if (s_ext[2 * i + 1] == s_ext[2 * i - 1]) atomicAdd(&s_rep, 1);      // (an integer count: the order does not matter)
    __syncthreads();
    const int st = s_bad != 0 ? CA_BAD : ((T == 0 || T < L + s_rep) ? CA_NO_ALIGNMENT : CA_ALIGNED);
    if (st != CA_ALIGNED) {
        for (int t = tid; t < t_max; t += CA_THREADS) { pth[t] = -1; lse[t] = __builtin_nan(""); }
        if (tid == 0) {
            score[2 * (size_t)seq] = __builtin_nan("");
            score[2 * (size_t)seq + 1] = __builtin_nan("");
            status[seq] = st;
            ties[seq] = 0;
        }
        return;
    }

    // log-sum-exp of every frame < T (one wave per frame, f64)
    for (int f = tid >> 6; f < T; f += CA_THREADS / 64) {
        const double v = frame_lse(x + (size_t)f * K, K, tid & 63);
        if ((tid & 63) == 0) lse[f] = v;
    }
    for (int t = T + tid; t < t_max; t += CA_THREADS) { pth[t] = -1; lse[t] = __builtin_nan(""); }

    // ---- the recurrence
    int ext[CA_PER];
    float xe[CA_PER];
    const int nper = (S + CA_THREADS - 1) / CA_THREADS;
#pragma unroll
    for (int j = 0; j < CA_PER; ++j) {
        const int s = tid + j * CA_THREADS;
        ext[j] = s < S ? s_ext[s] : blank;
        xe[j] = (s < S && T > 1) ? x[(size_t)K + ext[j]] : 0.0f;
        if (s < S) {
            s_v[0][s] = s == 0 ? (double)x[blank] : (s == 1 ? (double)x[ext[j]] : neg_inf);
            s_v[1][s] = neg_inf;
        }
    }
    __syncthreads();                                     // (orders the workgroup's global writes of lse before its reads too)
    for (int t = 1; t < T; ++t) {
        const double *prev = s_v[(t - 1) & 1];
        double *cur = s_v[t & 1];
        unsigned char *row = bp + (size_t)t * sw;
        const bool more = t + 1 < T;
        const int lo = max(0, 2 * L - 2 * (T - 1 - t) - 1), hi = min(S - 1, 2 * t + 1);
        float xn[CA_PER];
#pragma unroll
        for (int j = 0; j < CA_PER; ++j) {
            const int s = tid + j * CA_THREADS;
            xn[j] = (j < nper && more && s < S) ? x[(size_t)(t + 1) * K + ext[j]] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < CA_PER; ++j) {
            const int s = tid + j * CA_THREADS;
            if (j < nper && s >= lo && s <= hi) {
                double a = prev[s];
                int mv = 0, tie = 0;
                if (s >= 1) {
                    const double c = prev[s - 1];
                    if (c > a) { a = c; mv = 1; }
                    else if (c == a && a != neg_inf) tie = 1;
                }
                if ((s & 1) && s >= 3 && ext[j] != s_ext[s - 2]) {
                    const double c = prev[s - 2];
                    if (c > a) { a = c; mv = 2; tie = 0; }
                    else if (c == a && a != neg_inf) tie = 1;
                }
                cur[s] = a + (double)xe[j];
                row[s] = (unsigned char)(mv | (tie << 2));
            }
        }
#pragma unroll
        for (int j = 0; j < CA_PER; ++j) xe[j] = xn[j];
        __syncthreads();
    }

    // ---- the end, and sum_t lse_t in a fixed order
    double part = 0.0;
    for (int t = tid; t < T; t += CA_THREADS) part += lse[t];
    s_red[tid] = part;
    if (tid == 0) {
        const double *last = s_v[(T - 1) & 1];
        int e = S - 1, tie = 0;
        if (L >= 1) {
            const double a = last[S - 1], c = last[S - 2];
            if (c > a) e = S - 2;
            else if (c == a && a != neg_inf) tie = 1;
        }
        score[2 * (size_t)seq] = last[e];
        s_state = e;
        s_tie = tie;
    }
    __syncthreads();
    for (int w = CA_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) s_red[tid] += s_red[tid + w];
        __syncthreads();
    }

    // ---- the backtrace, CA_BLOCK_T frames at a time (frames t0 .. t0 - rows + 1, all >= 1: frame 0 has no back-pointer)
    for (int t0 = T - 1; t0 >= 1; t0 -= CA_BLOCK_T) {
        const int s0 = s_state;
        const int base = s0 - 2 * CA_BLOCK_T;                            // the state of the tile's column 0
        const int rows = min(CA_BLOCK_T, t0);
        for (int idx = tid; idx < rows * CA_BLOCK_S; idx += CA_THREADS) {
            const int d = idx / CA_BLOCK_S, c = idx - d * CA_BLOCK_S;
            const int s = base + c;
            if (s >= 0 && s >= s0 - 2 * d) s_tile[d][c] = bp[(size_t)(t0 - d) * sw + s];
        }
        __syncthreads();
        if (tid == 0) {
            int s = s0, tie = s_tie;
            for (int d = 0; d < rows; ++d) {
                pth[t0 - d] = s;
                const int cell = s_tile[d][s - base];
                tie |= (cell >> 2) & 1;
                s = max(s - min(cell & 3, 2), max(s0 - 2 * (d + 1), 0));   // (a move is 0, 1 or 2: the walk stays in the tile)
            }
            s_state = s;
            s_tie = tie;
        }
        __syncthreads();
    }
    if (tid == 0) {
        pth[0] = s_state;
        score[2 * (size_t)seq + 1] = score[2 * (size_t)seq] - s_red[0];
        status[seq] = CA_ALIGNED;
        ties[seq] = s_tie;
    }
}

// One workgroup per sequence.  The input length is not needed: path is -1 from it on.
__global__ void __launch_bounds__(CA_THREADS)
ctc_segments_kernel(const float *__restrict__ logits, int t_max, int K, const int64_t *__restrict__ targets, int max_l,
                    const int64_t *__restrict__ tgt_lengths, const int *__restrict__ path, const int *__restrict__ status,
                    const double *__restrict__ lse_all, int *__restrict__ first, int *__restrict__ last, float *__restrict__ conf)
{
    __shared__ int s_first[CA_MAX_L], s_last[CA_MAX_L];
    const int tid = threadIdx.x;
    const int seq = blockIdx.x;
    const float *x = logits + (size_t)seq * t_max * K;
    const int *pth = path + (size_t)seq * t_max;
    const double *lse = lse_all + (size_t)seq * t_max;
    const int64_t l64 = tgt_lengths[seq];
    const int L = (status[seq] == CA_ALIGNED && l64 >= 0 && l64 <= max_l) ? (int)l64 : 0;
    for (int i = tid; i < max_l; i += CA_THREADS) { s_first[i] = -1; s_last[i] = -1; }
    __syncthreads();
    if (L > 0) {
        for (int t = tid; t < t_max; t += CA_THREADS) {
            const int s = pth[t];
            if (s > 0 && (s & 1) && (s >> 1) < L) {
                if (t == 0 || pth[t - 1] != s) s_first[s >> 1] = t;
                if (t == t_max - 1 || pth[t + 1] != s) s_last[s >> 1] = t;
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < max_l; i += CA_THREADS) {
        int f = s_first[i], l = s_last[i];
        float c = __builtin_nanf("");
        const int64_t y = (i < L && f >= 0 && l >= f) ? targets[(size_t)seq * max_l + i] : -1;
        if (y >= 0 && y < K - 1) {
            double acc = 0.0;
            for (int t = f; t <= l; ++t) acc += (double)x[(size_t)t * K + y] - lse[t];
            c = (float)(acc / (double)(l - f + 1));
        } else {
            f = -1;
            l = -1;
        }
        first[(size_t)seq * max_l + i] = f;
        last[(size_t)seq * max_l + i] = l;
        conf[(size_t)seq * max_l + i] = c;
    }
}

static bool align_sizes_ok(int b, int t_max, int max_l)
{
    return b >= 1 && b <= 65535 && t_max >= 1 && t_max <= CA_MAX_T && max_l >= 0 && max_l <= t_max && max_l <= CA_MAX_L;
}

static size_t align_lse_bytes(int b, int t_max) { return align_up(sizeof(double) * (size_t)b * t_max, 256); }

}  // namespace
}  // namespace cpc

extern "C" size_t cpc_ctc_align_scratch_bytes(int b, int t_max, int max_l)
{
    if (!cpc::align_sizes_ok(b, t_max, max_l)) {
        cpc::set_error("ctc_align: sizes outside the supported limits (b=%d t_max=%d max_l=%d; need 1 <= b <= 65535, 1 <= t_max <= %d, "
                       "0 <= max_l <= min(t_max, %d))", b, t_max, max_l, cpc::CA_MAX_T, cpc::CA_MAX_L);
        return 0;
    }
    return cpc::align_lse_bytes(b, t_max) + cpc::align_up((size_t)b * t_max * (2 * (size_t)max_l + 1), 256);
}

extern "C" int cpc_ctc_align(const float *logits, int b, int t_max, int k, const int64_t *in_lengths, const int64_t *targets, int max_l,
                             const int64_t *tgt_lengths, int *path, double *score, int *status, int *ties, double *lse, void *scratch,
                             size_t scratch_bytes, cpc_stream_t stream)
{
    CPC_REQUIRE(cpc::align_sizes_ok(b, t_max, max_l) && k >= 2 && k <= cpc::CA_MAX_K,
                "ctc_align: sizes outside the supported limits (b=%d t_max=%d k=%d max_l=%d; need 1 <= b <= 65535, 1 <= t_max <= %d, "
                "2 <= k <= %d, 0 <= max_l <= min(t_max, %d))", b, t_max, k, max_l, cpc::CA_MAX_T, cpc::CA_MAX_K, cpc::CA_MAX_L);
    CPC_REQUIRE(logits && in_lengths && tgt_lengths && path && score && status && ties && (targets || max_l == 0),
                "ctc_align: null buffer");
    const size_t need = cpc_ctc_align_scratch_bytes(b, t_max, max_l);
    if (scratch == nullptr || scratch_bytes < need) {
        cpc::set_error("ctc_align: scratch of %zu B given, %zu B needed", scratch ? scratch_bytes : (size_t)0, need);
        return CPC_ERR_WORKSPACE;
    }
    double *lse_buf = lse ? lse : static_cast<double *>(scratch);
    unsigned char *bp = static_cast<unsigned char *>(scratch) + cpc::align_lse_bytes(b, t_max);
    hipLaunchKernelGGL(cpc::ctc_align_kernel, dim3((unsigned)b), dim3(cpc::CA_THREADS), 0, static_cast<hipStream_t>(stream), logits,
                       t_max, k, in_lengths, targets, max_l, tgt_lengths, path, score, status, ties, lse_buf, bp);
    CPC_CHECK_LAUNCH("ctc_align_kernel");
    return CPC_OK;
}

extern "C" int cpc_ctc_align_segments(const float *logits, int b, int t_max, int k, const int64_t *targets, int max_l,
                                      const int64_t *tgt_lengths, const int *path, const int *status, const double *lse, int *first,
                                      int *last, float *conf, cpc_stream_t stream)
{
    CPC_REQUIRE(cpc::align_sizes_ok(b, t_max, max_l) && k >= 2 && k <= cpc::CA_MAX_K,
                "ctc_align_segments: sizes outside the supported limits (b=%d t_max=%d k=%d max_l=%d; need 1 <= b <= 65535, "
                "1 <= t_max <= %d, 2 <= k <= %d, 0 <= max_l <= min(t_max, %d))", b, t_max, k, max_l, cpc::CA_MAX_T, cpc::CA_MAX_K,
                cpc::CA_MAX_L);
    if (max_l == 0) return CPC_OK;                       // no token: nothing to write
    CPC_REQUIRE(logits && targets && tgt_lengths && path && status && lse && first && last && conf, "ctc_align_segments: null buffer");
    hipLaunchKernelGGL(cpc::ctc_segments_kernel, dim3((unsigned)b), dim3(cpc::CA_THREADS), 0, static_cast<hipStream_t>(stream), logits,
                       t_max, k, targets, max_l, tgt_lengths, path, status, lse, first, last, conf);
    CPC_CHECK_LAUNCH("ctc_segments_kernel");
    return CPC_OK;
}
