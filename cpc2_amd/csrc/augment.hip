// Audio augmentation on device batches (cpc/data_augmentation.py: AdditiveNoiseAugment :157-228, NaturalReverb :278-318,
// TimeDropoutAugment :268-275; cpc/dataset.py:433-438 PeakNorm).  A batch's windows are slices of flat HBM-resident vectors
// (speech pack, noise pack, impulse responses): every kernel reads them by offset, no separate gather pass.
//   additive_kernel      one workgroup per window, both windows held in registers: global memory read once, written once
//   fir_kernel           causal truncated convolution, direct form: 1024 outputs per workgroup, 8 per thread, the response
//                        and the signal segment staged through LDS, 64-tap partial sums
//   peak_norm_kernel     w / (max|w| + 1e-8) of a window (PeakNorm of the noise; the second stage of the FIR)
//   time_dropout_kernel  zeros on [start, start + length)
// No float atomics anywhere: every reduction runs in a fixed order, so two launches on the same inputs give the same bits.
#include "common.h"

#include <algorithm>

namespace cpc {

constexpr int AUG_THREADS = 1024;            // additive / peak_norm: one workgroup per window
constexpr int AUG_HOLD = 8;                  // float4 per thread and operand held in registers: windows up to 32768 samples
constexpr float AUG_EPS = 1e-8f;

// ---- workgroup reductions in a fixed order: xor butterfly inside a wave, the wave results through LDS, summed in wave order
__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}
template <bool MAX> __device__ __forceinline__ float block_reduce(float v, float *red)
{
    v = MAX ? wave_max(v) : wave_sum(v);
    const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();                           // (red may still be read by the previous reduction)
    if ((threadIdx.x & 63) == 0) red[wave] = v;
    __syncthreads();
    float r = red[0];
    for (int i = 1; i < nw; ++i) r = MAX ? fmaxf(r, red[i]) : r + red[i];
    return r;
}

// elements [i, i + 4) of a window that starts at sample `off` of a vector of `total` samples (off < 0: the operand is a plain
// [batch][window] buffer and `p` already points at the window).  vec: the window lies inside the vector and is 16-byte aligned
struct WindowSrc {
    const float *p;          // first sample of the window
    long lo, hi;             // valid element indices [lo, hi) relative to p (zeros outside, as cpc_window_gather)
    bool vec;
};
__device__ __forceinline__ WindowSrc window_src(const float *base, long total, const long *offs, int b, int W)
{
    WindowSrc s;
    if (offs == nullptr) {
        s.p = base + (long)b * W; s.lo = 0; s.hi = W;
    } else {
        const long off = offs[b];
        s.p = base + off; s.lo = -off; s.hi = total - off;
    }
    s.vec = s.lo <= 0 && s.hi >= W && (reinterpret_cast<uintptr_t>(s.p) & 15) == 0 && (W & 3) == 0;
    return s;
}
__device__ __forceinline__ float4 window_load4(const WindowSrc &s, int i, int W)
{
    if (s.vec) return *reinterpret_cast<const float4 *>(s.p + i);
    float4 v;
    v.x = (i + 0 < W && i + 0 >= s.lo && i + 0 < s.hi) ? s.p[i + 0] : 0.f;
    v.y = (i + 1 < W && i + 1 >= s.lo && i + 1 < s.hi) ? s.p[i + 1] : 0.f;
    v.z = (i + 2 < W && i + 2 >= s.lo && i + 2 < s.hi) ? s.p[i + 2] : 0.f;
    v.w = (i + 3 < W && i + 3 >= s.lo && i + 3 < s.hi) ? s.p[i + 3] : 0.f;
    return v;
}
__device__ __forceinline__ void window_store4(float *p, int i, int W, bool vec, float4 v)
{
    if (vec) { *reinterpret_cast<float4 *>(p + i) = v; return; }
    if (i + 0 < W) p[i + 0] = v.x;
    if (i + 1 < W) p[i + 1] = v.y;
    if (i + 2 < W) p[i + 2] = v.z;
    if (i + 3 < W) p[i + 3] = v.w;
}
__device__ __forceinline__ float max4(float4 v) { return fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))); }
__device__ __forceinline__ float sq4(float4 v) { return (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w); }

// ---------------------------------------------------------------- additive noise
// out = peak(e(x) + g e(n')), n' = noise / (max|noise| + 1e-8) when noise_peak_norm (PeakNorm, the noise data set's transform)
// else noise; e(w) = w / (sqrt(mean(w^2)) + 1e-8), peak(m) = m / (max|m| + 1e-8).  Both epsilons sit where the reference has
// them, so an all-zero window gives what the formula gives.  HOLD: both windows stay in registers between the passes;
// otherwise (windows beyond AUG_HOLD * 4096 samples) the later passes read them again.
template <bool HOLD>
__global__ __launch_bounds__(AUG_THREADS) void additive_kernel(const float *speech, long speech_total, const long *speech_off,
                                                               const float *noise, long noise_total, const long *noise_off,
                                                               int noise_peak_norm, const float *gain, float *out, int W)
{
    __shared__ float red[AUG_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const WindowSrc xs = window_src(speech, speech_total, speech_off, b, W);
    const WindowSrc ns = window_src(noise, noise_total, noise_off, b, W);
    const int chunks = HOLD ? AUG_HOLD : (W + 4 * AUG_THREADS - 1) / (4 * AUG_THREADS);
    float4 xr[HOLD ? AUG_HOLD : 1], nr[HOLD ? AUG_HOLD : 1];
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);

    float ssx = 0.f, pkn = 0.f;
#pragma unroll 8
    for (int c = 0; c < chunks; ++c) {
        const int i = (c * AUG_THREADS + tid) * 4;
        const float4 x = i < W ? window_load4(xs, i, W) : zero;
        const float4 n = i < W ? window_load4(ns, i, W) : zero;
        if (HOLD) { xr[c] = x; nr[c] = n; }
        ssx += sq4(x);
        pkn = fmaxf(pkn, max4(n));
    }
    ssx = block_reduce<false>(ssx, red);
    const float nscale = noise_peak_norm ? block_reduce<true>(pkn, red) + AUG_EPS : 1.f;
    float ssn = 0.f;
#pragma unroll 8
    for (int c = 0; c < chunks; ++c) {
        const int i = (c * AUG_THREADS + tid) * 4;
        float4 n = HOLD ? nr[c] : (i < W ? window_load4(ns, i, W) : zero);
        if (noise_peak_norm) { n.x /= nscale; n.y /= nscale; n.z /= nscale; n.w /= nscale; }
        if (HOLD) nr[c] = n;
        ssn += sq4(n);
    }
    ssn = block_reduce<false>(ssn, red);
    const float ex = sqrtf(ssx / (float)W) + AUG_EPS;
    const float en = sqrtf(ssn / (float)W) + AUG_EPS;
    const float g = gain[b];
    float pkm = 0.f;
#pragma unroll 8
    for (int c = 0; c < chunks; ++c) {
        const int i = (c * AUG_THREADS + tid) * 4;
        float4 x = HOLD ? xr[c] : (i < W ? window_load4(xs, i, W) : zero);
        float4 n = HOLD ? nr[c] : (i < W ? window_load4(ns, i, W) : zero);
        if (!HOLD && noise_peak_norm) { n.x /= nscale; n.y /= nscale; n.z /= nscale; n.w /= nscale; }
        x.x = x.x / ex + (n.x / en) * g;
        x.y = x.y / ex + (n.y / en) * g;
        x.z = x.z / ex + (n.z / en) * g;
        x.w = x.w / ex + (n.w / en) * g;
        if (HOLD) xr[c] = x;
        pkm = fmaxf(pkm, max4(x));
    }
    const float pm = block_reduce<true>(pkm, red) + AUG_EPS;
    float *o = out + (long)b * W;
    const bool ovec = (reinterpret_cast<uintptr_t>(o) & 15) == 0 && (W & 3) == 0;
#pragma unroll 8
    for (int c = 0; c < chunks; ++c) {
        const int i = (c * AUG_THREADS + tid) * 4;
        if (i >= W) continue;
        float4 m;
        if (HOLD) m = xr[c];
        else {
            const float4 x = window_load4(xs, i, W);
            float4 n = window_load4(ns, i, W);
            if (noise_peak_norm) { n.x /= nscale; n.y /= nscale; n.z /= nscale; n.w /= nscale; }
            m.x = x.x / ex + (n.x / en) * g;
            m.y = x.y / ex + (n.y / en) * g;
            m.z = x.z / ex + (n.z / en) * g;
            m.w = x.w / ex + (n.w / en) * g;
        }
        m.x /= pm; m.y /= pm; m.z /= pm; m.w /= pm;
        window_store4(o, i, W, ovec, m);
    }
}

// ---------------------------------------------------------------- peak normalisation
// out[b] = w / (max|w| + 1e-8); prescale != NULL: the maximum is the largest of prescale[b * n_pre .. + n_pre) instead of the
// window's own (the FIR's per-tile maxima).  out may be the source buffer.
__global__ __launch_bounds__(AUG_THREADS) void peak_norm_kernel(const float *src, long total, const long *offs, const float *tile_max,
                                                                int n_pre, float *out, int W)
{
    __shared__ float red[AUG_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const WindowSrc s = window_src(src, total, offs, b, W);
    float pk = 0.f;
    if (tile_max != nullptr) {
        for (int i = 0; i < n_pre; ++i) pk = fmaxf(pk, tile_max[(long)b * n_pre + i]);
    } else {
        for (int i = tid * 4; i < W; i += 4 * AUG_THREADS) pk = fmaxf(pk, max4(window_load4(s, i, W)));
        pk = block_reduce<true>(pk, red);
    }
    const float scale = pk + AUG_EPS;
    float *o = out + (long)b * W;
    const bool ovec = (reinterpret_cast<uintptr_t>(o) & 15) == 0 && (W & 3) == 0;
    for (int i = tid * 4; i < W; i += 4 * AUG_THREADS) {
        float4 v = window_load4(s, i, W);
        v.x /= scale; v.y /= scale; v.z /= scale; v.w /= scale;
        window_store4(o, i, W, ovec, v);
    }
}

// ---------------------------------------------------------------- FIR (natural reverberation)
// y[t] = sum_{k <= t, k < L} ir[k] x[t - k], t < W.  A workgroup of 128 threads computes FIR_TILE = 1024 consecutive outputs of
// one window, 8 per thread.  The taps go by in stages of FIR_STAGE: the stage's taps and the FIR_TILE + FIR_STAGE signal samples
// they meet are staged in LDS (zeros in front of the window and beyond the response), then every thread walks the taps eight at
// a time over a sliding register window of 16 samples (two 16-byte LDS reads per 64 multiply-adds).  Partial sums run over 64
// taps, the (up to 8) partial sums of a stage are added up, and the stage sums are added to the output's accumulator: no chain of
// products is longer than 64, and the chains of sums have 8 and L / 512 terms.  Taps beyond the tile's last output are never
// visited.  The un-normalised outputs and the tile's max|y| are written; peak_norm_kernel divides (the maxima of a window's
// tiles combined in tile order).
constexpr int FIR_THREADS = 128, FIR_R = 8, FIR_TILE = FIR_THREADS * FIR_R, FIR_STAGE = 512, FIR_CHAIN = 64;

__device__ __forceinline__ void fir_group(const float *taps, const float (&lo)[8], const float (&hi)[8], float (&p)[FIR_R])
{
    // taps[q] meets sample index 7 + r - q of the 16-sample window (lo = samples 0..7, hi = 8..15)
    float t[8];
    *reinterpret_cast<float4 *>(&t[0]) = *reinterpret_cast<const float4 *>(taps);
    *reinterpret_cast<float4 *>(&t[4]) = *reinterpret_cast<const float4 *>(taps + 4);
#pragma unroll
    for (int q = 0; q < 8; ++q)
#pragma unroll
        for (int r = 0; r < FIR_R; ++r) {
            const int j = 7 + r - q;
            p[r] = fmaf(t[q], j < 8 ? lo[j] : hi[j - 8], p[r]);
        }
}
__device__ __forceinline__ void fir_load8(const float *seg, int at, float (&v)[8])
{
    *reinterpret_cast<float4 *>(&v[0]) = *reinterpret_cast<const float4 *>(seg + at);
    *reinterpret_cast<float4 *>(&v[4]) = *reinterpret_cast<const float4 *>(seg + at + 4);
}

__global__ __launch_bounds__(FIR_THREADS) void fir_kernel(const float *x, const float *ir, long ir_total, const long *ir_off,
                                                          const int *ir_len, float *y, float *tile_max, int W, int n_tiles)
{
    __shared__ __attribute__((aligned(16))) float seg[FIR_TILE + FIR_STAGE];
    __shared__ __attribute__((aligned(16))) float taps[FIR_STAGE];
    __shared__ float red[FIR_THREADS / 64];
    const int b = blockIdx.x, tile = n_tiles - 1 - (int)blockIdx.y, tid = threadIdx.x;     // (the tiles with most taps start first)
    const int t0 = tile * FIR_TILE;
    const float *xb = x + (long)b * W;
    float *yb = y + (long)b * W;
    long off = ir_off[b];
    int L = ir_len[b];
    if (off < 0 || off >= ir_total) L = 0;
    L = (int)min((long)min(L, W), ir_total - off);           // (only the first W taps can reach an output)
    float acc[FIR_R];
    if (L <= 0) {                                            // "leave the window as it is" (apart from the normalisation)
#pragma unroll
        for (int r = 0; r < FIR_R; ++r) { const int t = t0 + tid * FIR_R + r; acc[r] = t < W ? xb[t] : 0.f; }
    } else {
        const float *h = ir + off;
#pragma unroll
        for (int r = 0; r < FIR_R; ++r) acc[r] = 0.f;
        const int kmax = min(L, min(t0 + FIR_TILE, W));      // tap k meets x[t - k]: nothing beyond the tile's last output
        for (int ks = 0; ks < kmax; ks += FIR_STAGE) {
            // seg[j] = x[o + j], o = t0 - ks - (FIR_STAGE - 1): tap ks + kk of output t0 + u reads seg[u + FIR_STAGE - 1 - kk]
            const int o = t0 - ks - (FIR_STAGE - 1);
            __syncthreads();
            for (int j = tid; j < FIR_TILE + FIR_STAGE; j += FIR_THREADS) {
                const int src = o + j;
                seg[j] = (src >= 0 && src < W) ? xb[src] : 0.f;
            }
            for (int j = tid; j < FIR_STAGE; j += FIR_THREADS) taps[j] = ks + j < L ? h[ks + j] : 0.f;
            __syncthreads();
            const int stage_taps = min(FIR_STAGE, kmax - ks);
            float sacc[FIR_R];                               // the stage's sum: chains of 64 products, 8 partial sums, L / 512 stages
#pragma unroll
            for (int r = 0; r < FIR_R; ++r) sacc[r] = 0.f;
            for (int kc = 0; kc < stage_taps; kc += FIR_CHAIN) {
                float p[FIR_R];
#pragma unroll
                for (int r = 0; r < FIR_R; ++r) p[r] = 0.f;
                // group of taps kb .. kb + 7: samples seg[base .. base + 15], base = tid * 8 + FIR_STAGE - 8 - kb
                float wa[8], wb[8];
                fir_load8(seg, tid * FIR_R + FIR_STAGE - kc, wb);
#pragma unroll
                for (int kb = kc; kb < kc + FIR_CHAIN; kb += 16) {
                    fir_load8(seg, tid * FIR_R + FIR_STAGE - 8 - kb, wa);
                    fir_group(taps + kb, wa, wb, p);
                    fir_load8(seg, tid * FIR_R + FIR_STAGE - 16 - kb, wb);
                    fir_group(taps + kb + 8, wb, wa, p);
                }
#pragma unroll
                for (int r = 0; r < FIR_R; ++r) sacc[r] += p[r];
            }
#pragma unroll
            for (int r = 0; r < FIR_R; ++r) acc[r] += sacc[r];
        }
    }
    float pk = 0.f;
#pragma unroll
    for (int r = 0; r < FIR_R; ++r) {
        const int t = t0 + tid * FIR_R + r;
        if (t < W) { yb[t] = acc[r]; pk = fmaxf(pk, fabsf(acc[r])); }
    }
    pk = block_reduce<true>(pk, red);
    if (tid == 0) tile_max[(long)b * n_tiles + tile] = pk;
}

// ---------------------------------------------------------------- time dropout
__global__ void time_dropout_kernel(float *x, const long *start, const long *length, int W)
{
    const int b = blockIdx.y;
    const long s = max(0L, start[b]), e = min((long)W, start[b] + max(0L, length[b]));
    for (long t = s + (long)blockIdx.x * blockDim.x + threadIdx.x; t < e; t += (long)gridDim.x * blockDim.x) x[(long)b * W + t] = 0.f;
}

}  // namespace cpc

extern "C" int cpc_augment_additive(const float *speech, long speech_total, const long *speech_off, const float *noise,
                                    long noise_total, const long *noise_off, int noise_peak_norm, const float *gain, float *out,
                                    int batch, int window, cpc_stream_t stream)
{
    CPC_REQUIRE(speech != nullptr && noise != nullptr && gain != nullptr && out != nullptr && batch > 0 && window > 0,
                "augment_additive: bad arguments (batch=%d window=%d)", batch, window);
    CPC_REQUIRE((speech_off == nullptr || speech_total > 0) && (noise_off == nullptr || noise_total > 0),
                "augment_additive: an operand read by offsets needs its vector's length");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (window <= cpc::AUG_HOLD * 4 * cpc::AUG_THREADS)
        hipLaunchKernelGGL(cpc::additive_kernel<true>, dim3((unsigned)batch), dim3(cpc::AUG_THREADS), 0, st, speech, speech_total,
                           speech_off, noise, noise_total, noise_off, noise_peak_norm, gain, out, window);
    else
        hipLaunchKernelGGL(cpc::additive_kernel<false>, dim3((unsigned)batch), dim3(cpc::AUG_THREADS), 0, st, speech, speech_total,
                           speech_off, noise, noise_total, noise_off, noise_peak_norm, gain, out, window);
    CPC_CHECK_LAUNCH("additive_kernel");
    return CPC_OK;
}

extern "C" int cpc_augment_peak_norm(const float *src, long src_total, const long *src_off, float *out, int batch, int window,
                                     cpc_stream_t stream)
{
    CPC_REQUIRE(src != nullptr && out != nullptr && batch > 0 && window > 0 && (src_off == nullptr || src_total > 0),
                "augment_peak_norm: bad arguments (batch=%d window=%d)", batch, window);
    hipLaunchKernelGGL(cpc::peak_norm_kernel, dim3((unsigned)batch), dim3(cpc::AUG_THREADS), 0, static_cast<hipStream_t>(stream), src,
                       src_total, src_off, (const float *)nullptr, 0, out, window);
    CPC_CHECK_LAUNCH("peak_norm_kernel");
    return CPC_OK;
}

extern "C" size_t cpc_augment_fir_scratch_bytes(int batch, int window)
{
    if (batch <= 0 || window <= 0) return 0;
    return cpc::align_up((size_t)batch * cpc::cdiv(window, cpc::FIR_TILE) * sizeof(float), 256);
}

extern "C" int cpc_augment_fir(const float *x, const float *ir, long ir_total, const long *ir_off, const int *ir_len, float *out,
                               void *scratch, size_t scratch_bytes, int batch, int window, cpc_stream_t stream)
{
    CPC_REQUIRE(x != nullptr && ir != nullptr && ir_off != nullptr && ir_len != nullptr && out != nullptr && batch > 0 &&
                window > 0 && ir_total > 0, "augment_fir: bad arguments (batch=%d window=%d)", batch, window);
    CPC_REQUIRE(x != out, "augment_fir: the output must not be the input (a tile reads samples other tiles write)");
    if (scratch == nullptr || scratch_bytes < cpc_augment_fir_scratch_bytes(batch, window)) {
        cpc::set_error("augment_fir: scratch too small");
        return CPC_ERR_WORKSPACE;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int n_tiles = (int)cpc::cdiv(window, cpc::FIR_TILE);
    float *tile_max = static_cast<float *>(scratch);
    hipLaunchKernelGGL(cpc::fir_kernel, dim3((unsigned)batch, (unsigned)n_tiles), dim3(cpc::FIR_THREADS), 0, st, x, ir, ir_total,
                       ir_off, ir_len, out, tile_max, window, n_tiles);
    CPC_CHECK_LAUNCH("fir_kernel");
    hipLaunchKernelGGL(cpc::peak_norm_kernel, dim3((unsigned)batch), dim3(cpc::AUG_THREADS), 0, st, out, 0L, (const long *)nullptr,
                       tile_max, n_tiles, out, window);
    CPC_CHECK_LAUNCH("peak_norm_kernel");
    return CPC_OK;
}

extern "C" int cpc_augment_time_dropout(float *x, const long *start, const long *length, int batch, int window, cpc_stream_t stream)
{
    CPC_REQUIRE(x != nullptr && start != nullptr && length != nullptr && batch > 0 && batch <= 65535 && window > 0,
                "augment_time_dropout: bad arguments (batch=%d window=%d)", batch, window);
    hipLaunchKernelGGL(cpc::time_dropout_kernel, dim3((unsigned)std::min<long>(cpc::cdiv(window, 256), 16), (unsigned)batch), dim3(256),
                       0, static_cast<hipStream_t>(stream), x, start, length, window);
    CPC_CHECK_LAUNCH("time_dropout_kernel");
    return CPC_OK;
}
