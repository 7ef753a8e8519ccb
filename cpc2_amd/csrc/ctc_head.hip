// The whole-utterance CTC phone recogniser of the reference's cpc/eval/common_voices_eval.py (CTCphone_criterion): what its head
// needs beyond the GEMMs and the LSTM.  DESIGN.md section 16 has the layout.
//
//   ctc_len_kernel            one workgroup per sequence: log-sum-exp of the frames < len in f64 (global scratch, not LDS: t_max
//                             reaches 4096), alpha and beta in f64 log space over the 2 L + 1 extended states (two LDS rows), alpha
//                             + beta of every (t, s) in global scratch.  f64 because the log-probabilities reach |log alpha| ~
//                             T log K (~480 at T = 128, K = 42), where one f32 ulp is 3e-5 -- an error the occupancy exp(alpha +
//                             beta - log p - log y) would carry whole.  Frames >= len are never read; without an array of input
//                             lengths every length is t_max.
//   ctc_grad_kernel           the gradient softmax - occupancy per (t, class), the occupancy summed over the states of that class in
//                             ascending state order (a label that occurs several times in the target shares its class's bin); 1024
//                             elements of one sequence per workgroup, so the gradient fills the chip where the sequential passes
//                             cannot.  Frames >= len get exactly 0.
//   ctc_reduce_kernel         the loss as one workgroup's fixed-order sum.
//   ctc_loss_run              the three launches; cpc_ctc_loss calls it, and cpc_probe_ctc (probe.hip) with no input lengths and
//                             the mean reduction.  The lattice's shared pieces (extended states, frame log-sum-exp, log_add) are
//                             in ctc_lattice.h.
//   seqnorm_len_*_kernel      per (utterance, channel) statistics over the frames < len, applied to all frames; a workgroup owns 64
//                             channels of one utterance, four waves share the frames, f64 sums merged in a fixed order.
//   cpc_conv_head_forward     no kernel: cpc_gemm_nt's launcher once per utterance over the overlapping rows of the features, with
//                             room lent for an ordered sum of a K split (the public cpc_gemm_nt would add the parts with atomics).
//   conv_head_bwd_data_kernel dx of Conv1d(H, C, ks, stride = ks / 2) on channel-last data: every input frame takes the first half of
//                             the taps from output frame f / stride and the second half from the one before -- written once, no
//                             atomic, no unfolded buffer.
//   gather_utt_kernel         the zero-padded batch of whole utterances out of the resident pack.
// No float atomic anywhere: every result is bitwise reproducible.
#include "common.h"
#include "ctc_lattice.h"

#include <algorithm>

namespace cpc {
namespace {

constexpr int CH_THREADS = 256;
constexpr int CH_MAX_T = 4096;
constexpr int CH_MAX_L = 1024;               // the states live in LDS: 20 bytes each, 2 L + 1 of them (40 KB at 1024)
constexpr int CH_MAX_S = 2 * CH_MAX_L + 1;
constexpr int CH_MAX_K = 1 << 16;
constexpr int CTC_GRAD_PER_WG = 4 * CH_THREADS;       // gradient elements per workgroup
enum { CTC_NO_ALIGNMENT = 0, CTC_FEASIBLE = 1, CTC_BAD = 2 };
constexpr int SN_CH = 64;                    // channels per workgroup (one per lane)
constexpr int SN_SL = CH_THREADS / SN_CH;    // waves sharing the frames

// logits [b][t_max][k] (blank = k - 1); in_lengths [b] or null (every length t_max); targets [b][max_l], tgt_lengths [b]; lse_all [b][t_max], work
// [b][t_max][2 max_l + 1] (f64).  nll[seq] = -log p, 0 when no alignment exists (zero_infinity; an input length of 0 included)
// and NaN for a length or label out of range; logp_out[seq] and status[seq] hand log p and the sequence's kind to ctc_grad_kernel.
__global__ void __launch_bounds__(CH_THREADS)
ctc_len_kernel(const float *logits, int t_max, int K, const int64_t *__restrict__ in_lengths, const int64_t *__restrict__ targets,
               int max_l, const int64_t *__restrict__ tgt_lengths, double *__restrict__ lse_all, double *__restrict__ work,
               float *__restrict__ nll, double *__restrict__ logp_out, int *__restrict__ status)
{
    __shared__ double s_a[2][CH_MAX_S];
    __shared__ int s_ext[CH_MAX_S];
    __shared__ int s_bad;
    const int tid = threadIdx.x;
    const int seq = blockIdx.x;
    const int blank = K - 1;
    const int sw = 2 * max_l + 1;
    const float *x = logits + (long)seq * t_max * K;
    double *wk = work + (long)seq * t_max * sw;
    double *s_lse = lse_all + (long)seq * t_max;
    const int64_t l64 = tgt_lengths[seq];
    const int64_t t64 = in_lengths ? in_lengths[seq] : t_max;
    const bool len_ok = l64 >= 0 && l64 <= max_l && t64 >= 0 && t64 <= t_max;
    const int L = len_ok ? (int)l64 : 0;
    const int T = len_ok ? (int)t64 : 0;
    const int S = 2 * L + 1;

    if (tid == 0) s_bad = len_ok ? 0 : 1;
    __syncthreads();
    if (load_ext_states<CH_THREADS>(targets + (long)seq * max_l, S, blank, s_ext)) s_bad = 1;      // (benign race: all store 1)
    // log-sum-exp of every frame < T (one wave per frame, f64)
    for (int f = tid >> 6; f < T; f += CH_THREADS / 64) {
        const double v = frame_lse(x + (long)f * K, K, tid & 63);
        if ((tid & 63) == 0) s_lse[f] = v;
    }
    __syncthreads();                                     // (orders the workgroup's global writes of s_lse before its reads too)
    const bool bad = s_bad != 0;
    const bool run = !bad && T >= 1;
    auto lp = [&](int f, int lab) { return (double)x[(long)f * K + lab] - s_lse[f]; };

    // alpha, with wk[t][s] = alpha[t][s]
    if (run) {
        for (int s = tid; s < S; s += CH_THREADS) {
            const double a = s == 0 ? lp(0, blank) : (s == 1 ? lp(0, s_ext[1]) : -__builtin_inf());
            s_a[0][s] = a;
            wk[s] = a;
        }
    }
    __syncthreads();
    for (int f = 1; f < T && run; ++f) {
        const double *prev = s_a[(f - 1) & 1];
        double *cur = s_a[f & 1];
        for (int s = tid; s < S; s += CH_THREADS) {
            double a = prev[s];
            if (s >= 1) a = log_add(a, prev[s - 1]);
            if (s >= 2 && s_ext[s] != blank && s_ext[s] != s_ext[s - 2]) a = log_add(a, prev[s - 2]);
            if (a != -__builtin_inf()) a += lp(f, s_ext[s]);
            cur[s] = a;
            wk[(long)f * sw + s] = a;
        }
        __syncthreads();
    }
    double logp = 0.0;
    if (run) {
        const double *last = s_a[(T - 1) & 1];
        logp = log_add(last[S - 1], S >= 2 ? last[S - 2] : -__builtin_inf());
    }
    const bool feasible = run && logp != -__builtin_inf();
    __syncthreads();                                     // (everyone has read `last` before beta reuses the buffers)

    // beta; wk[t][s] becomes alpha + beta (each thread owns the same states as in the alpha pass)
    if (feasible) {
        for (int s = tid; s < S; s += CH_THREADS) {
            const double bt = s >= S - 2 ? lp(T - 1, s_ext[s]) : -__builtin_inf();
            s_a[(T - 1) & 1][s] = bt;
            wk[(long)(T - 1) * sw + s] += bt;
        }
        __syncthreads();
        for (int f = T - 2; f >= 0; --f) {
            const double *next = s_a[(f + 1) & 1];
            double *cur = s_a[f & 1];
            for (int s = tid; s < S; s += CH_THREADS) {
                double bt = next[s];
                if (s + 1 < S) bt = log_add(bt, next[s + 1]);
                if (s + 2 < S && s_ext[s] != blank && s_ext[s + 2] != s_ext[s]) bt = log_add(bt, next[s + 2]);
                if (bt != -__builtin_inf()) bt += lp(f, s_ext[s]);
                cur[s] = bt;
                wk[(long)f * sw + s] += bt;
            }
            __syncthreads();
        }
    }
    if (tid == 0) {
        nll[seq] = bad ? __builtin_nanf("") : (feasible ? (float)(-logp) : 0.0f);
        logp_out[seq] = logp;
        status[seq] = bad ? CTC_BAD : (feasible ? CTC_FEASIBLE : CTC_NO_ALIGNMENT);
    }
}

// The gradient, CTC_GRAD_PER_WG elements (frame, class) of one sequence per workgroup: (softmax - occupancy) * scale on the frames
// < len of a feasible sequence, scale = 1 / (gridDim.y * max(L, 1)) for the mean and 1 for the sum; 0 beyond and without an
// alignment, NaN for a bad sequence.  An element reads the logits at its own place only, so grad may be the logits' buffer.  The
// occupancy of a class is summed over its states in ascending order by ONE thread: the bits do not depend on the grid.
__global__ void __launch_bounds__(CH_THREADS)
ctc_grad_kernel(const float *logits, int t_max, int K, const int64_t *__restrict__ in_lengths, const int64_t *__restrict__ targets,
                int max_l, const int64_t *__restrict__ tgt_lengths, const double *__restrict__ lse_all, const double *__restrict__ work,
                const double *__restrict__ logp_in, const int *__restrict__ status, float *grad, int mean)
{
    __shared__ int s_ext[CH_MAX_S];
    const int tid = threadIdx.x;
    const int seq = blockIdx.y;
    const int blank = K - 1;
    const int sw = 2 * max_l + 1;
    const long total = (long)t_max * K;
    const long first = (long)blockIdx.x * CTC_GRAD_PER_WG;
    const int st = status[seq];
    const bool feasible = st == CTC_FEASIBLE;
    const int L = feasible ? (int)tgt_lengths[seq] : 0;      // (in range: the forward kernel checked both lengths)
    const int T = feasible ? (in_lengths ? (int)in_lengths[seq] : t_max) : 0;
    const int S = 2 * L + 1;
    // (uniform per workgroup; the labels are needed only then, and the forward kernel found them all in range)
    if (feasible && first < (long)T * K) load_ext_states<CH_THREADS>(targets + (long)seq * max_l, S, blank, s_ext);
    __syncthreads();
    const float *x = logits + (long)seq * total;
    const double *wk = work + (long)seq * t_max * sw;
    const double *s_lse = lse_all + (long)seq * t_max;
    const double logp = logp_in[seq];
    const double scale = mean ? 1.0 / ((double)gridDim.y * (double)max(L, 1)) : 1.0;
    float *g = grad + (long)seq * total;
    for (long idx = first + tid; idx < min(first + CTC_GRAD_PER_WG, total); idx += CH_THREADS) {
        const int f = (int)(idx / K), k = (int)(idx % K);
        float out = 0.0f;
        if (st == CTC_BAD) {
            out = __builtin_nanf("");
        } else if (feasible && f < T) {
            const double l = (double)x[idx] - s_lse[f];
            double occ = -__builtin_inf();
            const double *row = wk + (long)f * sw;
            if (k == blank) {
                for (int s = 0; s < S; s += 2) occ = log_add(occ, row[s]);
            } else {
                for (int s = 1; s < S; s += 2)
                    if (s_ext[s] == k) occ = log_add(occ, row[s]);
            }
            const double o = occ == -__builtin_inf() ? 0.0 : exp(occ - logp - l);
            out = (float)((exp(l) - o) * scale);
        }
        g[idx] = out;
    }
}

// mean: loss[0] = (sum_i vals[i] / max(lengths[i], 1)) / n; sum: loss[0] = sum_i vals[i]; fixed order
__global__ void __launch_bounds__(CH_THREADS)
ctc_reduce_kernel(const float *__restrict__ vals, const int64_t *__restrict__ lengths, long n, int mean, float *__restrict__ loss)
{
    __shared__ float s_sum[CH_THREADS];
    const int tid = threadIdx.x;
    float sum = 0.0f;
    for (long i = tid; i < n; i += CH_THREADS) {
        float v = vals[i];
        if (mean) v /= (float)max((int64_t)1, lengths[i]);
        sum += v;
    }
    s_sum[tid] = sum;
    __syncthreads();
    for (int w = CH_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) s_sum[tid] += s_sum[tid + w];
        __syncthreads();
    }
    if (tid == 0) loss[0] = mean ? s_sum[0] / (float)n : s_sum[0];
}

// ---------------------------------------------------------------- normalisation over the first len frames
// the four waves' partial sums of a channel, merged in wave order (every thread gets the same bits)
__device__ __forceinline__ double sn_merge(double (*s_p)[SN_CH], double v)
{
    const int ch = threadIdx.x & (SN_CH - 1), sl = threadIdx.x / SN_CH;
    __syncthreads();                                     // (the previous merge's readers are done)
    s_p[sl][ch] = v;
    __syncthreads();
    double t = s_p[0][ch];
#pragma unroll
    for (int i = 1; i < SN_SL; ++i) t += s_p[i][ch];
    return t;
}

__global__ void __launch_bounds__(CH_THREADS)
seqnorm_len_fwd_kernel(const float *__restrict__ x, const int64_t *__restrict__ lengths, int s, int h, float eps,
                       float *__restrict__ y, float *__restrict__ mean, float *__restrict__ rstd)
{
    __shared__ double s_p[SN_SL][SN_CH];
    const int sl = threadIdx.x / SN_CH;
    const int c = blockIdx.x * SN_CH + (threadIdx.x & (SN_CH - 1));
    const int b = blockIdx.y;
    const bool live = c < h;
    const int64_t n64 = lengths[b];
    const bool ok = n64 >= 1 && n64 <= s;
    const int n = ok ? (int)n64 : 0;
    const float *xb = x + (long)b * s * h;
    double acc = 0.0;
    if (live)
        for (int f = sl; f < n; f += SN_SL) acc += (double)xb[(long)f * h + c];
    const double m = sn_merge(s_p, acc) / (double)n;
    acc = 0.0;
    if (live)
        for (int f = sl; f < n; f += SN_SL) {
            const double d = (double)xb[(long)f * h + c] - m;
            acc += d * d;
        }
    const double v = sn_merge(s_p, acc) / (double)(n - 1);      // (n = 1: 0 / 0, NaN as torch.var gives)
    const double r = ok ? 1.0 / sqrt(v + (double)eps) : __builtin_nan("");
    if (!live) return;
    float *yb = y + (long)b * s * h;
    for (int f = sl; f < s; f += SN_SL) yb[(long)f * h + c] = (float)(((double)xb[(long)f * h + c] - m) * r);
    if (sl == 0) {
        mean[(long)b * h + c] = ok ? (float)m : __builtin_nanf("");
        rstd[(long)b * h + c] = (float)r;
    }
}

// dx[f] = r (dy[f] - [f < n] (A / n + B y[f] / (n - 1))), A = sum_f dy[f], B = sum_f dy[f] y[f] over ALL frames
__global__ void __launch_bounds__(CH_THREADS)
seqnorm_len_bwd_kernel(const float *__restrict__ dy, const float *__restrict__ y, const float *__restrict__ rstd,
                       const int64_t *__restrict__ lengths, int s, int h, float *__restrict__ dx)
{
    __shared__ double s_p[SN_SL][SN_CH];
    const int sl = threadIdx.x / SN_CH;
    const int c = blockIdx.x * SN_CH + (threadIdx.x & (SN_CH - 1));
    const int b = blockIdx.y;
    const bool live = c < h;
    const int64_t n64 = lengths[b];
    const bool ok = n64 >= 1 && n64 <= s;
    const int n = ok ? (int)n64 : 0;
    const float *dyb = dy + (long)b * s * h;
    const float *yb = y + (long)b * s * h;
    double a = 0.0, bb = 0.0;
    if (live)
        for (int f = sl; f < s; f += SN_SL) {
            const double g = (double)dyb[(long)f * h + c];
            a += g;
            bb += g * (double)yb[(long)f * h + c];
        }
    const double A = sn_merge(s_p, a) / (double)n;
    const double B = sn_merge(s_p, bb) / (double)(n - 1);
    if (!live) return;
    const double r = ok ? (double)rstd[(long)b * h + c] : __builtin_nan("");
    float *dxb = dx + (long)b * s * h;
    for (int f = sl; f < s; f += SN_SL) {
        double g = (double)dyb[(long)f * h + c];
        if (f < n) g -= A + B * (double)yb[(long)f * h + c];
        dxb[(long)f * h + c] = (float)(r * g);
    }
}

// ---------------------------------------------------------------- the strided classifier's backward-data
// dout [b][P][C], wp [C][ks][h] (the Conv1d weight with taps before channels), dx [b][s][h]; stride = ks / 2.  Frame f = stride j + u
// is tap u of output frame j and tap stride + u of output frame j - 1; frames behind stride (P + 1) belong to no output frame.
__global__ void __launch_bounds__(CH_THREADS)
conv_head_bwd_data_kernel(const float *__restrict__ dout, const float *__restrict__ wp, int s, int h, int C, int ks, int P,
                          float *__restrict__ dx)
{
    const int c = blockIdx.x * SN_CH + (threadIdx.x & (SN_CH - 1));
    const int f = blockIdx.y * SN_SL + threadIdx.x / SN_CH;
    const int b = blockIdx.z;
    if (c >= h || f >= s) return;
    const int stride = ks / 2;
    const int j = f / stride, u = f - j * stride;
    float acc = 0.0f;
    if (j < P) {
        const float *d = dout + ((long)b * P + j) * C;
        for (int k = 0; k < C; ++k) acc = fmaf(d[k], wp[((long)k * ks + u) * h + c], acc);
    }
    if (j >= 1 && j - 1 < P) {
        const float *d = dout + ((long)b * P + j - 1) * C;
        for (int k = 0; k < C; ++k) acc = fmaf(d[k], wp[((long)k * ks + stride + u) * h + c], acc);
    }
    dx[((long)b * s + f) * h + c] = acc;
}

// ---------------------------------------------------------------- the utterance gather
__global__ void __launch_bounds__(CH_THREADS)
gather_utt_kernel(const float *__restrict__ pack, long total, const int64_t *__restrict__ offsets, const int64_t *__restrict__ lengths,
                  const int64_t *__restrict__ roffset, float *__restrict__ out, long max_len)
{
    const int i = blockIdx.y;
    const int64_t off = offsets[i], len = lengths[i], ro = roffset ? roffset[i] : 0;
    const bool ok = off >= 0 && len >= 0 && ro >= 0 && ro <= len && off <= total && len <= total - off;
    const long count = !ok ? 0 : (len - ro < max_len ? (long)(len - ro) : max_len);
    const float *src = pack + (ok ? off + ro : 0);
    float *dst = out + (long)i * max_len;
    for (long p = (long)blockIdx.x * CH_THREADS + threadIdx.x; p < max_len; p += (long)gridDim.x * CH_THREADS)
        dst[p] = p < count ? src[p] : 0.0f;
}

static bool ctc_sizes_ok(int b, int t_max, int max_l)
{
    return b >= 1 && b <= 65535 && t_max >= 1 && t_max <= CH_MAX_T && max_l >= 0 && max_l <= t_max && max_l <= CH_MAX_L;
}

}  // namespace

// The three launches of the CTC loss, for cpc_ctc_loss and cpc_probe_ctc: the callers have checked the sizes and that scratch
// holds cpc_ctc_loss_scratch_bytes(b, t_max, max_l).
int ctc_loss_run(const float *logits, int b, int t_max, int k, const int64_t *in_lengths, const int64_t *targets, int max_l,
                 const int64_t *tgt_lengths, int reduction, float *nll, float *loss, float *dlogits, void *scratch, hipStream_t st)
{
    Carver carve(scratch);
    double *lse = carve.take<double>((size_t)b * t_max);
    double *work = carve.take<double>((size_t)b * t_max * (2 * (size_t)max_l + 1));
    double *logp = carve.take<double>((size_t)b);
    int *status = carve.take<int>((size_t)b);
    hipLaunchKernelGGL(ctc_len_kernel, dim3((unsigned)b), dim3(CH_THREADS), 0, st, logits, t_max, k, in_lengths, targets, max_l,
                       tgt_lengths, lse, work, nll, logp, status);
    CPC_CHECK_LAUNCH("ctc_len_kernel");
    if (dlogits != nullptr) {
        const unsigned chunks = (unsigned)cdiv((long)t_max * k, CTC_GRAD_PER_WG);
        hipLaunchKernelGGL(ctc_grad_kernel, dim3(chunks, (unsigned)b), dim3(CH_THREADS), 0, st, logits, t_max, k, in_lengths, targets,
                           max_l, tgt_lengths, lse, work, logp, status, dlogits, reduction);
        CPC_CHECK_LAUNCH("ctc_grad_kernel");
    }
    hipLaunchKernelGGL(ctc_reduce_kernel, dim3(1), dim3(CH_THREADS), 0, st, nll, tgt_lengths, (long)b, reduction, loss);
    CPC_CHECK_LAUNCH("ctc_reduce_kernel");
    return CPC_OK;
}

}  // namespace cpc

extern "C" size_t cpc_ctc_loss_scratch_bytes(int b, int t_max, int max_l)
{
    if (!cpc::ctc_sizes_ok(b, t_max, max_l)) {
        cpc::set_error("ctc_loss: sizes outside the supported limits (b=%d t_max=%d max_l=%d; need 1 <= b <= 65535, 1 <= t_max <= %d, "
                       "0 <= max_l <= min(t_max, %d))", b, t_max, max_l, cpc::CH_MAX_T, cpc::CH_MAX_L);
        return 0;
    }
    return cpc::align_up(sizeof(double) * (size_t)b * t_max, 256) +
           cpc::align_up(sizeof(double) * (size_t)b * t_max * (2 * (size_t)max_l + 1), 256) +
           cpc::align_up(sizeof(double) * (size_t)b, 256) + cpc::align_up(sizeof(int) * (size_t)b, 256);
}

extern "C" int cpc_ctc_loss(const float *logits, int b, int t_max, int k, const int64_t *in_lengths, const int64_t *targets, int max_l,
                            const int64_t *tgt_lengths, int reduction, float *nll, float *loss, float *dlogits, void *scratch,
                            size_t scratch_bytes, cpc_stream_t stream)
{
    CPC_REQUIRE(cpc::ctc_sizes_ok(b, t_max, max_l) && k >= 2 && k <= cpc::CH_MAX_K,
                "ctc_loss: sizes outside the supported limits (b=%d t_max=%d k=%d max_l=%d; need 1 <= b <= 65535, 1 <= t_max <= %d, "
                "2 <= k <= %d, 0 <= max_l <= min(t_max, %d))", b, t_max, k, max_l, cpc::CH_MAX_T, cpc::CH_MAX_K, cpc::CH_MAX_L);
    CPC_REQUIRE(reduction == 0 || reduction == 1, "ctc_loss: reduction %d (0 = sum, 1 = mean)", reduction);
    CPC_REQUIRE(logits && in_lengths && tgt_lengths && nll && loss && (targets || max_l == 0), "ctc_loss: null buffer");
    const size_t need = cpc_ctc_loss_scratch_bytes(b, t_max, max_l);
    CPC_REQUIRE(scratch != nullptr && scratch_bytes >= need, "ctc_loss: scratch of %zu bytes, %zu needed", scratch_bytes, need);
    return cpc::ctc_loss_run(logits, b, t_max, k, in_lengths, targets, max_l, tgt_lengths, reduction, nll, loss, dlogits, scratch,
                             static_cast<hipStream_t>(stream));
}

static int seqnorm_len_check(const char *name, int b, int s, int h)
{
    CPC_REQUIRE(b >= 1 && b <= 65535 && s >= 1 && h >= 1, "%s: sizes outside the supported limits (b=%d s=%d h=%d; need 1 <= b <= 65535, "
                "s >= 1, h >= 1)", name, b, s, h);
    return CPC_OK;
}

extern "C" int cpc_seqnorm_len_forward(const float *x, const int64_t *lengths, int b, int s, int h, float eps, float *y, float *mean,
                                       float *rstd, cpc_stream_t stream)
{
    CPC_TRY(seqnorm_len_check("seqnorm_len_forward", b, s, h));
    CPC_REQUIRE(x && lengths && y && mean && rstd, "seqnorm_len_forward: null buffer");
    hipLaunchKernelGGL(cpc::seqnorm_len_fwd_kernel, dim3((unsigned)cpc::cdiv(h, cpc::SN_CH), (unsigned)b), dim3(cpc::CH_THREADS), 0,
                       static_cast<hipStream_t>(stream), x, lengths, s, h, eps, y, mean, rstd);
    CPC_CHECK_LAUNCH("seqnorm_len_fwd_kernel");
    return CPC_OK;
}

extern "C" int cpc_seqnorm_len_backward(const float *dy, const float *y, const float *rstd, const int64_t *lengths, int b, int s, int h,
                                        float *dx, cpc_stream_t stream)
{
    CPC_TRY(seqnorm_len_check("seqnorm_len_backward", b, s, h));
    CPC_REQUIRE(dy && y && rstd && lengths && dx, "seqnorm_len_backward: null buffer");
    hipLaunchKernelGGL(cpc::seqnorm_len_bwd_kernel, dim3((unsigned)cpc::cdiv(h, cpc::SN_CH), (unsigned)b), dim3(cpc::CH_THREADS), 0,
                       static_cast<hipStream_t>(stream), dy, y, rstd, lengths, s, h, dx);
    CPC_CHECK_LAUNCH("seqnorm_len_bwd_kernel");
    return CPC_OK;
}

static int conv_head_check(const char *name, int b, int s, int h, int c, int ks)
{
    CPC_REQUIRE(ks >= 2 && ks % 2 == 0, "%s: kernel size %d (an even size >= 2 is needed: stride = ks / 2)", name, ks);
    CPC_REQUIRE(b >= 1 && b <= 65535 && h >= 1 && c >= 1 && s >= ks && s <= 4 * 65535 && (long)ks * h <= 2147483647L,
                "%s: sizes outside the supported limits (b=%d s=%d h=%d c=%d ks=%d; need 1 <= b <= 65535, ks <= s <= 262140)", name,
                b, s, h, c, ks);
    return CPC_OK;
}

extern "C" size_t cpc_conv_head_forward_scratch_bytes(int b, int s, int h, int c, int ks)
{
    if (conv_head_check("conv_head_forward", b, s, h, c, ks) != CPC_OK) return 0;
    // (one utterance's product at a time: the room is reused; never 0, so that 0 means "refused")
    return std::max<size_t>(256, cpc::gemm_nt_scratch_bytes((s - ks) / (ks / 2) + 1, c, ks * h));
}

extern "C" int cpc_conv_head_forward(const float *x, const float *wp, const float *bias, float *out, int b, int s, int h, int c, int ks,
                                     void *scratch, size_t scratch_bytes, cpc_stream_t stream)
{
    CPC_TRY(conv_head_check("conv_head_forward", b, s, h, c, ks));
    CPC_REQUIRE(x && wp && out, "conv_head_forward: null buffer");
    const size_t need = cpc_conv_head_forward_scratch_bytes(b, s, h, c, ks);
    CPC_REQUIRE(scratch != nullptr && scratch_bytes >= need, "conv_head_forward: scratch of %zu bytes, %zu needed", scratch_bytes, need);
    const int stride = ks / 2;
    const long P = (s - ks) / stride + 1;
    cpc::RowMap map{};
    map.splitk_scratch = scratch;          // a K split (ks h >= 2048 with few output tiles) is summed from slabs in a fixed order
    map.splitk_bytes = scratch_bytes;
    for (int i = 0; i < b; ++i)
        CPC_TRY(cpc::gemm_nt(x + (long)i * s * h, (long)stride * h, wp, (long)ks * h, out + (long)i * P * c, c, bias, P, c, ks * h, map,
                             static_cast<hipStream_t>(stream)));
    return CPC_OK;
}

extern "C" int cpc_conv_head_backward_data(const float *dout, const float *wp, int b, int s, int h, int c, int ks, float *dx,
                                           cpc_stream_t stream)
{
    CPC_TRY(conv_head_check("conv_head_backward_data", b, s, h, c, ks));
    CPC_REQUIRE(dout && wp && dx, "conv_head_backward_data: null buffer");
    const int P = (s - ks) / (ks / 2) + 1;
    hipLaunchKernelGGL(cpc::conv_head_bwd_data_kernel,
                       dim3((unsigned)cpc::cdiv(h, cpc::SN_CH), (unsigned)cpc::cdiv(s, cpc::SN_SL), (unsigned)b), dim3(cpc::CH_THREADS), 0,
                       static_cast<hipStream_t>(stream), dout, wp, s, h, c, ks, P, dx);
    CPC_CHECK_LAUNCH("conv_head_bwd_data_kernel");
    return CPC_OK;
}

extern "C" int cpc_gather_utterances(const float *pack, long total, const int64_t *offsets, const int64_t *lengths,
                                     const int64_t *roffset, float *out, int n, long max_len, cpc_stream_t stream)
{
    CPC_REQUIRE(n >= 1 && n <= 65535 && max_len >= 1 && total >= 1,
                "gather_utterances: sizes outside the supported limits (n=%d max_len=%ld total=%ld; need 1 <= n <= 65535)", n, max_len, total);
    CPC_REQUIRE(pack && offsets && lengths && out, "gather_utterances: null buffer");
    hipLaunchKernelGGL(cpc::gather_utt_kernel, dim3((unsigned)std::min<long>(cpc::cdiv(max_len, cpc::CH_THREADS), 1024), (unsigned)n),
                       dim3(cpc::CH_THREADS), 0, static_cast<hipStream_t>(stream), pack, total, offsets, lengths, roffset, out, max_len);
    CPC_CHECK_LAUNCH("gather_utt_kernel");
    return CPC_OK;
}
