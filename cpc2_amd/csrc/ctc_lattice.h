// The pieces of the CTC lattice that the loss (ctc_head.hip) and the forced alignment (ctc_align.hip) state once: the
// extended-state table, the f64 log-sum-exp of a frame and log(exp a + exp b).  A function here is compiled under the flags
// of the file that includes it (ctc_align.hip is built with -ffp-contract=off, ctc_head.hip is not).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace cpc {

__device__ __forceinline__ double log_add(double a, double b)
{
    const double m = fmax(a, b);
    if (m == -__builtin_inf()) return m;
    return m + log1p(exp(fmin(a, b) - m));
}

// log sum_j exp(row[j]) over the K logits of one frame by ONE wave64 (lane = the caller's lane in it): lane j visits columns
// j, j + 64, ... in order keeping a max-shifted (max, sum of exp) pair, and the 64 lanes merge by a butterfly whose merge is
// symmetric, so every lane returns the same bits.
__device__ __forceinline__ double frame_lse(const float *row, int K, int lane)
{
    const double neg_inf = -__builtin_inf();
    double m = neg_inf, acc = 0.0;
    for (int j = lane; j < K; j += 64) {
        const double v = (double)row[j];
        if (v > m) {
            acc = (m == neg_inf ? 0.0 : acc * exp(m - v)) + 1.0;
            m = v;
        } else {
            acc += exp(v - m);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double om = __shfl_xor(m, o), oa = __shfl_xor(acc, o);
        const double nm = fmax(m, om);
        if (nm != neg_inf) {
            acc = (m == neg_inf ? 0.0 : acc * exp(m - nm)) + (om == neg_inf ? 0.0 : oa * exp(om - nm));
            m = nm;
        }
    }
    return m + log(acc);
}

// ext[s] for the S = 2 L + 1 extended states of one sequence with labels tgt[0..L): blank for even s, tgt[s / 2] for odd s,
// the workgroup's THREADS threads strided over the states.  A label outside [0, blank) is stored as blank; the return value says
// whether THIS thread met one.  The caller places the barrier.
template <int THREADS>
__device__ __forceinline__ bool load_ext_states(const int64_t *tgt, int S, int blank, int *ext)
{
    bool bad = false;
    for (int s = threadIdx.x; s < S; s += THREADS) {
        int lab = blank;
        if (s & 1) {
            const int64_t v = tgt[s >> 1];
            if (v < 0 || v >= blank) bad = true;
            lab = (v >= 0 && v < blank) ? (int)v : blank;
        }
        ext[s] = lab;
    }
    return bad;
}

}  // namespace cpc
