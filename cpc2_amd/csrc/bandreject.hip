// Band-reject filtering of device windows (the `bandreject_sinc` augmentation; the definition is in include/cpc2_hip.h): a
// Kaiser-windowed sinc band-reject FIR of 2 H + 1 taps, symmetric about the output sample, one band (low, high) per window.  The
// definition is this package's own; it is the textbook filter behind sox's `sinc -a 120 high-low` but claims no agreement with
// sox's output (unmeasured), and there is no dither.
//   br_tap              h[j] of one band in f64: I0 from its power series until a term falls below 2^-60 of the sum, the sine from
//                       an argument reduced exactly.  The one place the design is written down: both kernels call it.
//   bandreject_taps_kernel   h[0 .. H] of every row to global memory (cpc_bandreject_taps: the design on its own, for the tests).
//   bandreject_kernel   one workgroup per (row, tile of BR_TILE outputs).  The H + 1 taps are designed into LDS in f64 and the
//                       tile's samples plus 2 H of halo are staged in LDS as f32.  A thread owns BR_R = 8 consecutive outputs and
//                       walks j = 1 .. H with two sliding register windows, x[t - j] on the left and x[t + j] on the right: a
//                       step reads ONE new sample per side and does 8 additions and 8 FMAs, acc = fma(h[j], x[t - j] + x[t + j],
//                       acc) -- the sum of two f32 values is exact in f64.  The j loop is unrolled by 8 so that the windows rotate
//                       by renaming, and a block's sixteen samples and eight taps are read ahead of its steps.  A thread's
//                       samples are 8 apart from its neighbour's, so the staged row is padded by one float in 8 (stride 9 across
//                       lanes: conflict-free), and it starts where a thread's first output falls on a multiple of 8, which puts
//                       a block's reads at fixed offsets from two pointers.  The sums are rounded once, passed through LDS and
//                       stored coalesced.  A row whose band is empty (low == high) or not a band at all is copied, no arithmetic.
// One fixed summation order (the centre tap, then j ascending), no atomics, no global scratch: a row's bits depend on nothing but
// the row, its band and the scalars.
#include "common.h"

#include <cmath>

namespace cpc {

constexpr int BR_THREADS = 256;
constexpr int BR_R = 8;                                     // consecutive outputs per thread
constexpr int BR_TILE = BR_THREADS * BR_R;                  // outputs per workgroup
constexpr int BR_MAX_HALF = 1024;
constexpr int BR_STAGED = BR_TILE + 2 * BR_MAX_HALF;        // the tile and its halo
constexpr int BR_FRONT = 15;                                // at most this many floats in front of the staged samples
constexpr int BR_SERIES = 256;                              // terms of I0's series allowed for (beta <= 50 needs fewer than 100)

// v[k - 1] = 1 / k^2, so that the series has no division in its loop (read with a uniform index: scalar loads)
struct BrInvK2 {
    double v[BR_SERIES];
    constexpr BrInvK2() : v()
    {
        for (int k = 1; k <= BR_SERIES; ++k) v[k - 1] = 1.0 / ((double)k * (double)k);
    }
};
__constant__ BrInvK2 br_inv_k2 = BrInvK2();

// I0(x) = sum_k ((x / 2)^2)^k / (k!)^2 for x >= 0: every term is positive, nothing cancels.  The terms are added eight at a time
// (the eight reciprocals are one scalar load, and the loop waits for memory once per eight terms) and the sum ends once a term
// has fallen below 2^-60 of it: beyond their largest the terms only shrink.
__device__ __forceinline__ double br_i0(double x)
{
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 0; k < BR_SERIES; k += 8) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            term = term * q * br_inv_k2.v[k + i];
            sum += term;
        }
        if (term < 0x1p-60 * sum) break;
    }
    return sum;
}

// (2 f / sr) sinc(2 f j / sr), sinc(u) = sin(pi u) / (pi u).  u - 2 rint(u / 2) is exact and lies in [-1, 1].
__device__ __forceinline__ double br_lowpass(double f, int j, double sr)
{
    const double c = 2.0 * f / sr;
    const double u = 2.0 * f * (double)j / sr;
    if (u == 0.0) return c;
    const double r = u - 2.0 * rint(0.5 * u);
    return c * (sinpi(r) / (M_PI * u));
}

__device__ __forceinline__ bool br_is_band(double low, double high, double sr) { return low >= 0.0 && low <= high && high <= 0.5 * sr; }

// h[j], 0 <= j <= H, of the band (low, high): [j == 0] - w[j] (lp_high[j] - lp_low[j]).  An empty band, or a pair that is no band
// (NaN included), gives the identity: 1 followed by zeros.
__device__ __forceinline__ double br_tap(int j, int H, double beta, double sr, double low, double high)
{
    const double delta = j == 0 ? 1.0 : 0.0;
    if (!br_is_band(low, high, sr) || low == high) return delta;
    const double rel = (double)j / (double)H;
    const double w = br_i0(beta * sqrt(1.0 - rel * rel)) / br_i0(beta);
    return delta - w * (br_lowpass(high, j, sr) - br_lowpass(low, j, sr));
}

__global__ __launch_bounds__(BR_THREADS) void bandreject_taps_kernel(const double *band, int H, double beta, double sr, double *taps)
{
    const int b = blockIdx.x;
    const double low = band[2 * (long)b], high = band[2 * (long)b + 1];
    for (int j = threadIdx.x; j <= H; j += BR_THREADS) taps[(long)b * (H + 1) + j] = br_tap(j, H, beta, sr, low, high);
}

// a window of a [batch][window] buffer (offs == NULL) or of a flat vector: sample i, zero outside [0, W) and outside the vector
struct BrSrc {
    const float *p;          // first sample of the window
    long lo, hi;             // readable indices [lo, hi) relative to p, already cut to [0, W)
};
__device__ __forceinline__ BrSrc br_src(const float *base, long total, const long *offs, int b, int W)
{
    BrSrc s;
    if (offs == nullptr) {
        s.p = base + (long)b * W; s.lo = 0; s.hi = W;
    } else {
        const long off = offs[b];
        s.p = base + off;
        s.lo = off < 0 ? -off : 0;
        s.hi = total - off < (long)W ? total - off : (long)W;
    }
    return s;
}
__device__ __forceinline__ float br_read(const BrSrc &s, long i) { return (i >= s.lo && i < s.hi) ? s.p[i] : 0.f; }

__device__ __forceinline__ int br_pad(int s) { return s + (s >> 3); }          // where staged sample s >= 0 lives in LDS

// Step j (j % 8 == JJ) of a thread's eight sums, t0 its first output.  L[m & 7] holds x[t0 + m] for m in [-j, 7 - j] once the new
// left sample x[t0 - j] is in, R[m & 7] holds x[t0 + m] for m in [j, j + 7] once the new right sample x[t0 + 7 + j] is.
template <int JJ>
__device__ __forceinline__ void br_step(double h, float left, float right, double (&acc)[BR_R], double (&L)[BR_R], double (&R)[BR_R])
{
    L[(BR_R - JJ) & 7] = (double)left;
    R[(JJ + 7) & 7] = (double)right;
#pragma unroll
    for (int i = 0; i < BR_R; ++i) acc[i] = fma(h, L[(i - JJ) & 7] + R[(i + JJ) & 7], acc[i]);
}

// Steps j0 .. j0 + 7 (j0 a multiple of 8).  lp / rp point at the thread's staged samples x[t0 - j0] / x[t0 + j0], both at a
// multiple of 8 in the staged row, so the block's sixteen samples sit at fixed distances: x[t0 - j0 - jj] at -jj - (jj > 0),
// x[t0 + j0 + 7 + jj] at 7 + jj + (jj > 0).  They and the eight taps are read ahead of the steps.  EDGE: the first block, which
// has no step 0, or the last, which may pass H -- what such a step would read is inside the arrays and is not used.
template <bool EDGE>
__device__ __forceinline__ void br_block(int j0, int H, const float *lp, const float *rp, const double *taps, double (&acc)[BR_R],
                                         double (&L)[BR_R], double (&R)[BR_R])
{
    float xl[8], xr[8];
    double h[8];
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) {
        xl[jj] = lp[-jj - (jj > 0)];
        xr[jj] = rp[7 + jj + (jj > 0)];
        h[jj] = taps[j0 + jj];
    }
    if (!EDGE || j0 >= 1)          br_step<0>(h[0], xl[0], xr[0], acc, L, R);
    if (!EDGE || j0 + 1 <= H)      br_step<1>(h[1], xl[1], xr[1], acc, L, R);
    if (!EDGE || j0 + 2 <= H)      br_step<2>(h[2], xl[2], xr[2], acc, L, R);
    if (!EDGE || j0 + 3 <= H)      br_step<3>(h[3], xl[3], xr[3], acc, L, R);
    if (!EDGE || j0 + 4 <= H)      br_step<4>(h[4], xl[4], xr[4], acc, L, R);
    if (!EDGE || j0 + 5 <= H)      br_step<5>(h[5], xl[5], xr[5], acc, L, R);
    if (!EDGE || j0 + 6 <= H)      br_step<6>(h[6], xl[6], xr[6], acc, L, R);
    if (!EDGE || j0 + 7 <= H)      br_step<7>(h[7], xl[7], xr[7], acc, L, R);
}

__global__ __launch_bounds__(BR_THREADS) void bandreject_kernel(const float *src, long total, const long *offs, const double *band,
                                                                int H, double beta, double sr, float *out, int W)
{
    __shared__ double taps[BR_MAX_HALF + 8];
    __shared__ float xs[BR_STAGED + BR_FRONT + 16 + (BR_STAGED + BR_FRONT + 16) / 8 + 1];
    const int b = blockIdx.y, tid = threadIdx.x;
    const long base = (long)blockIdx.x * BR_TILE;               // the tile's first output
    const int n = W - base < (long)BR_TILE ? (int)(W - base) : BR_TILE;
    const double low = band[2 * (long)b], high = band[2 * (long)b + 1];
    const BrSrc x = br_src(src, total, offs, b, W);
    float *o = out + (long)b * W + base;

    if (!br_is_band(low, high, sr) || low == high) {            // (uniform) the identity: copied, no arithmetic
        for (int s = tid; s < n; s += BR_THREADS) o[s] = br_read(x, base + s);
        return;
    }
    for (int j = tid; j <= H; j += BR_THREADS) taps[j] = br_tap(j, H, beta, sr, low, high);
    // x[base - H + s], s in [0, BR_TILE + 2 H), is staged at s + front; zero outside the row's own [0, W).  front, 8 to 15, puts
    // the tile's first output at a multiple of 8 and leaves room for what the first block's unused steps read.
    const int front = ((8 - (H & 7)) & 7) + 8;
    for (int s = tid; s < BR_TILE + 2 * H; s += BR_THREADS) xs[br_pad(s + front)] = br_read(x, base - H + s);
    __syncthreads();

    // The thread's first output is staged at 8 tid + H + front, and br_pad(8 tid + c) = 9 tid + br_pad(c) for c >= 0: a thread's
    // part of every address is 9 tid, and br_pad(c) = 9 c / 8 for a multiple of 8.
    const float *mine = xs + 9 * tid;
    const float *lp = mine + 9 * ((H + front) >> 3), *rp = lp;
    double acc[BR_R], L[BR_R], R[BR_R];
    const double h0 = taps[0];
#pragma unroll
    for (int i = 0; i < BR_R; ++i) {
        L[i] = R[i] = (double)lp[i];
        acc[i] = h0 * L[i];
    }
    br_block<true>(0, H, lp, rp, taps, acc, L, R);
    int j0 = 8;
    for (; j0 + 7 <= H; j0 += 8) br_block<false>(j0, H, lp -= 9, rp += 9, taps, acc, L, R);
    if (j0 <= H) br_block<true>(j0, H, lp - 9, rp + 9, taps, acc, L, R);
    __syncthreads();                                            // everybody has read its samples: the sums take their place
#pragma unroll
    for (int i = 0; i < BR_R; ++i) xs[br_pad(tid * BR_R + i)] = (float)acc[i];
    __syncthreads();
    for (int s = tid; s < n; s += BR_THREADS) o[s] = xs[br_pad(s)];
}

static int br_check(const char *who, int batch, int window, int half, double beta, double sample_rate)
{
    CPC_REQUIRE(window > 0 && batch >= 0 && batch <= 65535, "%s: bad arguments (batch=%d window=%d)", who, batch, window);
    CPC_REQUIRE(half >= 1 && half <= BR_MAX_HALF, "%s: half=%d, filters of half length 1 to %d are built", who, half, BR_MAX_HALF);
    CPC_REQUIRE(std::isfinite(beta) && beta >= 0.0 && beta <= 50.0, "%s: beta=%g outside [0, 50]", who, beta);
    CPC_REQUIRE(std::isfinite(sample_rate) && sample_rate > 0.0, "%s: sample_rate=%g is not a positive finite rate", who, sample_rate);
    return CPC_OK;
}

}  // namespace cpc

extern "C" int cpc_bandreject_tile(void) { return cpc::BR_TILE; }
extern "C" int cpc_bandreject_max_half(void) { return cpc::BR_MAX_HALF; }

extern "C" int cpc_bandreject_taps(const double *band, int batch, int half, double beta, double sample_rate, double *taps,
                                   cpc_stream_t stream)
{
    CPC_TRY(cpc::br_check("bandreject_taps", batch, 1, half, beta, sample_rate));
    if (batch == 0) return CPC_OK;
    CPC_REQUIRE(band != nullptr && taps != nullptr, "bandreject_taps: a null pointer with batch=%d", batch);
    hipLaunchKernelGGL(cpc::bandreject_taps_kernel, dim3((unsigned)batch), dim3(cpc::BR_THREADS), 0, static_cast<hipStream_t>(stream),
                       band, half, beta, sample_rate, taps);
    CPC_CHECK_LAUNCH("bandreject_taps_kernel");
    return CPC_OK;
}

extern "C" int cpc_augment_bandreject(const float *src, long src_total, const long *src_off, const double *band, int half, double beta,
                                      double sample_rate, float *out, int batch, int window, cpc_stream_t stream)
{
    CPC_TRY(cpc::br_check("augment_bandreject", batch, window, half, beta, sample_rate));
    if (batch == 0) return CPC_OK;
    CPC_REQUIRE(src != nullptr && band != nullptr && out != nullptr, "augment_bandreject: a null pointer with batch=%d", batch);
    CPC_REQUIRE(src_off == nullptr || src_total > 0, "augment_bandreject: a source read by offsets needs its vector's length");
    CPC_REQUIRE(src != out, "augment_bandreject: the output must not be the input");
    const unsigned tiles = (unsigned)cpc::cdiv(window, cpc::BR_TILE);
    hipLaunchKernelGGL(cpc::bandreject_kernel, dim3(tiles, (unsigned)batch), dim3(cpc::BR_THREADS), 0, static_cast<hipStream_t>(stream),
                       src, src_total, src_off, band, half, beta, sample_rate, out, window);
    CPC_CHECK_LAUNCH("bandreject_kernel");
    return CPC_OK;
}
