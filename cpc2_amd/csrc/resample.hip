// Sample-rate conversion of a pack of signals (torchaudio's sinc_interp_hann method, the transform behind the reference's
// cpc/eval/utils/adjust_sample_rate.py), and the PCM16 quantiser of the WAV writer.
//
//   o = orig / gcd, n = new / gcd, base = min(o, n) * rolloff, w = ceil(width * o / base), taps = 2 w + o
//   h[p][j] = sinc(t) * cos(t pi / (2 width))^2 * base / o,  t = clamp((-p / n + (j - w) / o) * base, -width, width)
//   y[f n + p] = sum_j h[p][j] * xp[f o + j],  xp = x with w zeros in front and w + o behind,  cut to ceil(n L / o) samples
//
//   cpc_resample_plan / cpc_resample_table_host   the plan and the table, in double on the host, rounded once to f32
//   resample_kernel     a workgroup of 256 threads owns RS_FR * 256 / PX frames x PX phases of one signal (PX = min(64, the
//                       power of two >= n) lanes run along the phases, the rest of the workgroup along the frames): the signal
//                       segment those frames read sits in LDS (zeros outside the signal, filled by index), the table goes by in
//                       slices of 32 taps (row stride 33: lanes on consecutive phases meet 32 distinct banks), and every thread
//                       holds RS_FR frames of one phase, so that a table word serves RS_FR multiply-adds
//   resample_phases_kernel   the same sums for ratios with n >= 64 phases: lanes along the phases, the signal words as scalar
//                       operands, PR phases x RS_FR frames per thread (described at the kernel)
//   pcm16_kernel        q = clamp(rint(32768 y)) and the count of clamped samples (an integer atomic per workgroup)
// Every output sample is ONE chain of fmaf over j = 0 .. taps - 1 in ascending order (taps beyond the table multiply zeros): the
// result does not depend on the launch geometry, on the tile a frame falls in, or on what else is in the pack.
#include "common.h"

#include <cmath>
#include <numeric>

namespace cpc {

constexpr int RS_THREADS = 256, RS_FR = 4, RS_JC = 32, RS_PXMAX = 64;
constexpr int RS_SEG = 8192;                 // floats of signal per workgroup: 16 frames of o = 441 and their 475 taps fit
constexpr double RS_PI = 3.14159265358979323846;

struct ResamplePlan { int o, n, w, taps; };

static int resample_plan(int orig, int target, int width, double rolloff, ResamplePlan *plan)
{
    CPC_REQUIRE(orig > 0 && target > 0 && width > 0 && rolloff > 0.0 && rolloff <= 1.0,
                "resample: bad arguments (orig_freq=%d new_freq=%d lowpass_filter_width=%d rolloff=%g)", orig, target, width, rolloff);
    const int g = std::gcd(orig, target);
    plan->o = orig / g;
    plan->n = target / g;
    const double base = (double)std::min(plan->o, plan->n) * rolloff;
    plan->w = (int)std::ceil((double)width * (double)plan->o / base);
    plan->taps = 2 * plan->w + plan->o;
    return CPC_OK;
}

// frames a workgroup takes: RS_FR per thread along the frames, fewer when the segment would not fit the LDS array
static int resample_tile_frames(int o, int taps, int px)
{
    const long room = ((long)RS_SEG - cdiv(taps, RS_JC) * RS_JC) / o;        // (<= 0: not even one frame fits)
    return (int)std::min<long>((long)RS_FR * (RS_THREADS / px), room);
}
static int resample_px(int n)
{
    int px = 1;
    while (px < n && px < RS_PXMAX) px *= 2;
    return px;
}

__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const float *x, long x_total, const long *in_off, const long *in_len,
                                                              const float *table, int o, int n, int w, int taps, float *y,
                                                              long y_total, const long *out_off, int px_lanes, int tile_frames,
                                                              long frame_tiles)
{
    __shared__ float seg[RS_SEG];
    __shared__ float tab[RS_PXMAX * (RS_JC + 1)];
    const int tid = threadIdx.x;
    const long s = (long)blockIdx.x / frame_tiles, ft = (long)blockIdx.x % frame_tiles;
    const long off = in_off[s], L = in_len[s], yoff = out_off[s];
    if (L <= 0 || off < 0 || yoff < 0 || off + L > x_total) return;
    const long out_len = ((long)n * L + o - 1) / o;                   // ceil(n L / o)
    const long frames = (out_len + n - 1) / n;
    const long f0 = ft * tile_frames;
    if (f0 >= frames) return;                                          // (uniform over the workgroup: before any barrier)
    const int p0 = (int)blockIdx.y * px_lanes;
    const int px = tid % px_lanes, fy = tid / px_lanes, fys = RS_THREADS / px_lanes;
    const int taps_up = (taps + RS_JC - 1) / RS_JC * RS_JC;

    // seg[k] = xp[f0 o + k] = x[f0 o + k - w], zero outside [0, L)
    const float *xs = x + off;
    const long first = f0 * o - w;
    const int seg_n = tile_frames * o + taps_up;
    for (int k = tid; k < seg_n; k += RS_THREADS) {
        const long src = first + k;
        seg[k] = (src >= 0 && src < L) ? xs[src] : 0.f;
    }
    int row[RS_FR];
    float acc[RS_FR];
#pragma unroll
    for (int r = 0; r < RS_FR; ++r) {
        row[r] = min(fy + fys * r, tile_frames - 1) * o;              // (rows beyond the tile read its last frame and store nothing)
        acc[r] = 0.f;
    }
    for (int j0 = 0; j0 < taps_up; j0 += RS_JC) {
        __syncthreads();                                               // (the previous slice is read; the first pass: seg is written)
        for (int e = tid; e < px_lanes * RS_JC; e += RS_THREADS) {
            const int pp = e / RS_JC, jj = e % RS_JC;
            const int p = p0 + pp, j = j0 + jj;
            tab[pp * (RS_JC + 1) + jj] = (p < n && j < taps) ? table[(long)p * taps + j] : 0.f;
        }
        __syncthreads();
        const float *tp = tab + px * (RS_JC + 1);
#pragma unroll 8
        for (int jj = 0; jj < RS_JC; ++jj) {
            const float t = tp[jj];
#pragma unroll
            for (int r = 0; r < RS_FR; ++r) acc[r] = fmaf(t, seg[row[r] + j0 + jj], acc[r]);
        }
    }
    const int p = p0 + px;
    if (p >= n) return;
#pragma unroll
    for (int r = 0; r < RS_FR; ++r) {
        const int fr = fy + fys * r;
        if (fr >= tile_frames) continue;
        const long m = (f0 + fr) * n + p;
        if (m < out_len && yoff + m < y_total) y[yoff + m] = acc[r];
    }
}

// Ratios with many phases (n >= 64: 441 -> 160, 441 -> 320, 160 -> 441): the 64 lanes of a wave run along the phases, RP_PR phases
// each (lane, lane + 64, ...), and a wave holds RS_FR consecutive frames, so every thread keeps RS_FR x PR sums.  The table goes by
// in slices of RP_JC = 16 taps (row stride 20 words: the 16-byte reads of 16 consecutive lanes meet 16 distinct slots); a thread
// reads its PR rows of the slice with 16-byte LDS loads.  The signal words a wave needs are the same for all its lanes: lane l
// loads word l & 15 of each frame's slice once, and the multiply-adds take them as scalar operands (v_readlane), so the LDS
// carries PR / 4 reads per tap instead of PR + RS_FR, and a table word in registers serves RS_FR multiply-adds.  The chain of
// every output is the same fmaf(h, x, acc) over ascending j as in resample_kernel: the two kernels give the same bits.
constexpr int RP_JC = 16, RP_STRIDE = 20, RP_PRMAX = 4;

template <int PR>
__global__ __launch_bounds__(RS_THREADS) void resample_phases_kernel(const float *x, long x_total, const long *in_off,
                                                                     const long *in_len, const float *table, int o, int n, int w,
                                                                     int taps, float *y, long y_total, const long *out_off,
                                                                     int tile_frames, long frame_tiles)
{
    __shared__ __attribute__((aligned(16))) float seg[RS_SEG];
    __shared__ __attribute__((aligned(16))) float tab[64 * PR * RP_STRIDE];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long s = (long)blockIdx.x / frame_tiles, ft = (long)blockIdx.x % frame_tiles;
    const long off = in_off[s], L = in_len[s], yoff = out_off[s];
    if (L <= 0 || off < 0 || yoff < 0 || off + L > x_total) return;
    const long out_len = ((long)n * L + o - 1) / o;
    const long frames = (out_len + n - 1) / n;
    const long f0 = ft * tile_frames;
    if (f0 >= frames) return;                                          // (uniform over the workgroup: before any barrier)
    const int p0 = (int)blockIdx.y * 64 * PR;
    const int taps_up = (taps + RP_JC - 1) / RP_JC * RP_JC;

    const float *xs = x + off;
    const long first = f0 * o - w;
    const int seg_n = tile_frames * o + taps_up;
    for (int k = tid; k < seg_n; k += RS_THREADS) {
        const long src = first + k;
        seg[k] = (src >= 0 && src < L) ? xs[src] : 0.f;
    }
    int row[RS_FR];
    float acc[RS_FR][PR];
#pragma unroll
    for (int r = 0; r < RS_FR; ++r) {
        row[r] = min(wv * RS_FR + r, tile_frames - 1) * o + (lane & (RP_JC - 1));
#pragma unroll
        for (int q = 0; q < PR; ++q) acc[r][q] = 0.f;
    }
    // the slice after the one being summed is on its way from global memory (L2: the table is a few hundred KB) into registers
    // while the sums run; thread `tid` carries elements tid, tid + 256, ... of the slice's 64 PR x 16 words
    constexpr int PER = 64 * PR * RP_JC / RS_THREADS;
    float ahead[PER];
    auto fetch = [&](int j0) {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int e = tid + i * RS_THREADS;
            const int p = p0 + e / RP_JC, j = j0 + e % RP_JC;
            ahead[i] = (p < n && j < taps) ? table[(long)p * taps + j] : 0.f;
        }
    };
    fetch(0);
    for (int j0 = 0; j0 < taps_up; j0 += RP_JC) {
        __syncthreads();                                               // (the previous slice is read; the first pass: seg is written)
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int e = tid + i * RS_THREADS;
            tab[(e / RP_JC) * RP_STRIDE + e % RP_JC] = ahead[i];
        }
        __syncthreads();
        if (j0 + RP_JC < taps_up) fetch(j0 + RP_JC);
        int sv[RS_FR];
#pragma unroll
        for (int r = 0; r < RS_FR; ++r) sv[r] = __float_as_int(seg[row[r] + j0]);
        float t[PR][RP_JC];
#pragma unroll
        for (int q = 0; q < PR; ++q)
#pragma unroll
            for (int c = 0; c < RP_JC; c += 4)
                *reinterpret_cast<float4 *>(&t[q][c]) = *reinterpret_cast<const float4 *>(&tab[(lane + 64 * q) * RP_STRIDE + c]);
#pragma unroll
        for (int jj = 0; jj < RP_JC; ++jj)
#pragma unroll
            for (int r = 0; r < RS_FR; ++r) {
                const float xv = __int_as_float(__builtin_amdgcn_readlane(sv[r], jj));
#pragma unroll
                for (int q = 0; q < PR; ++q) acc[r][q] = fmaf(t[q][jj], xv, acc[r][q]);
            }
    }
#pragma unroll
    for (int r = 0; r < RS_FR; ++r) {
        const int fr = wv * RS_FR + r;
        if (fr >= tile_frames) continue;
#pragma unroll
        for (int q = 0; q < PR; ++q) {
            const int p = p0 + lane + 64 * q;
            const long m = (f0 + fr) * n + p;
            if (p < n && m < out_len && yoff + m < y_total) y[yoff + m] = acc[r][q];
        }
    }
}

// phases per thread: the share of lanes that have a phase, times PR / (PR + 1), the multiply-adds' share of a tap's vector
// instructions (RS_FR v_readlane beside RS_FR x PR v_fma)
static int resample_phases_per_thread(int n)
{
    int best = 1;
    double best_score = 0.0;
    for (int pr = 1; pr <= RP_PRMAX; ++pr) {
        const double used = (double)n / (double)(cdiv(n, 64 * pr) * 64 * pr);
        const double score = used * pr / (pr + 1.0);
        if (score >= best_score) { best_score = score; best = pr; }
    }
    return best;
}

constexpr int PCM_THREADS = 256;

__global__ __launch_bounds__(PCM_THREADS) void pcm16_kernel(const float *y, long count, short *q, unsigned long long *clamped)
{
    __shared__ unsigned red[PCM_THREADS / 64];
    unsigned mine = 0;
    for (long i = (long)blockIdx.x * PCM_THREADS + threadIdx.x; i < count; i += (long)gridDim.x * PCM_THREADS) {
        const float v = rintf(32768.f * y[i]);                         // (ties to even)
        const bool out = !(v >= -32768.f && v <= 32767.f);
        mine += out ? 1u : 0u;
        q[i] = (short)(int)fminf(fmaxf(v, -32768.f), 32767.f);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) mine += __shfl_xor(mine, d, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned total = 0;
        for (int i = 0; i < PCM_THREADS / 64; ++i) total += red[i];
        if (total != 0) atomicAdd(clamped, (unsigned long long)total);
    }
}

}  // namespace cpc

extern "C" int cpc_resample_plan(int orig_freq, int new_freq, int lowpass_filter_width, double rolloff, int *o, int *n, int *w, int *taps)
{
    CPC_REQUIRE(o != nullptr && n != nullptr && w != nullptr && taps != nullptr, "resample_plan: null output");
    cpc::ResamplePlan plan;
    CPC_TRY(cpc::resample_plan(orig_freq, new_freq, lowpass_filter_width, rolloff, &plan));
    *o = plan.o; *n = plan.n; *w = plan.w; *taps = plan.taps;
    return CPC_OK;
}

extern "C" int cpc_resample_table_host(int orig_freq, int new_freq, int lowpass_filter_width, double rolloff, float *table_host,
                                       long capacity)
{
    cpc::ResamplePlan plan;
    CPC_TRY(cpc::resample_plan(orig_freq, new_freq, lowpass_filter_width, rolloff, &plan));
    CPC_REQUIRE(table_host != nullptr && capacity >= (long)plan.n * plan.taps,
                "resample_table_host: the buffer holds %ld floats, the table has %d x %d", capacity, plan.n, plan.taps);
    const double width = (double)lowpass_filter_width;
    const double base = (double)std::min(plan.o, plan.n) * rolloff;
    for (int p = 0; p < plan.n; ++p)
        for (int j = 0; j < plan.taps; ++j) {
            double t = (-(double)p / (double)plan.n + (double)(j - plan.w) / (double)plan.o) * base;
            t = std::min(std::max(t, -width), width);
            const double c = std::cos(t * cpc::RS_PI / width / 2.0);
            const double win = c * c;
            const double sinc = t == 0.0 ? 1.0 : std::sin(cpc::RS_PI * t) / (cpc::RS_PI * t);
            table_host[(long)p * plan.taps + j] = (float)(sinc * win * base / (double)plan.o);
        }
    return CPC_OK;
}

extern "C" int cpc_resample(const float *x, long x_total, const long *in_off, const long *in_len, int count, long max_len,
                            const float *table, int o, int n, int w, float *y, long y_total, const long *out_off, cpc_stream_t stream)
{
    CPC_REQUIRE(x != nullptr && in_off != nullptr && in_len != nullptr && table != nullptr && y != nullptr && out_off != nullptr &&
                count > 0 && x_total > 0 && y_total > 0 && max_len >= 0,
                "resample: bad arguments (count=%d x_total=%ld y_total=%ld max_len=%ld)", count, x_total, y_total, max_len);
    CPC_REQUIRE(o > 0 && n > 0 && w > 0, "resample: bad plan (o=%d n=%d w=%d)", o, n, w);
    if (max_len == 0) return CPC_OK;
    const int taps = 2 * w + o;
    const bool by_phases = n >= 64;                                   // (the two kernels give the same bits; see resample_phases_kernel)
    const int px = by_phases ? 64 : cpc::resample_px(n);
    const int pr = by_phases ? cpc::resample_phases_per_thread(n) : 1;
    const int tile_frames = by_phases ? (int)std::min<long>(cpc::RS_FR * (cpc::RS_THREADS / 64),
                                                            ((long)cpc::RS_SEG - cpc::cdiv(taps, cpc::RP_JC) * cpc::RP_JC) / o)
                                      : cpc::resample_tile_frames(o, taps, px);
    CPC_REQUIRE(tile_frames >= 1, "resample: the reduced ratio o / n = %d / %d needs %d taps and %d input samples per frame, more than a "
                "workgroup's %d floats of LDS hold; choose rates with a larger common divisor", o, n, taps, o, cpc::RS_SEG);
    const long out_max = ((long)n * max_len + o - 1) / o;
    const long frame_tiles = cpc::cdiv(cpc::cdiv(out_max, n), tile_frames);
    const long phase_tiles = cpc::cdiv(n, px * pr);
    CPC_REQUIRE(frame_tiles * count < (1L << 31) && phase_tiles <= 65535,
                "resample: %ld frame tiles x %d signals exceed one launch; split the pack", frame_tiles, count);
    const dim3 grid((unsigned)(frame_tiles * count), (unsigned)phase_tiles), block(cpc::RS_THREADS);
    hipStream_t st = static_cast<hipStream_t>(stream);
#define CPC_RESAMPLE_PHASES(PR)                                                                                                    \
    hipLaunchKernelGGL(cpc::resample_phases_kernel<PR>, grid, block, 0, st, x, x_total, in_off, in_len, table, o, n, w, taps, y,    \
                       y_total, out_off, tile_frames, frame_tiles)
    if (!by_phases)
        hipLaunchKernelGGL(cpc::resample_kernel, grid, block, 0, st, x, x_total, in_off, in_len, table, o, n, w, taps, y, y_total,
                           out_off, px, tile_frames, frame_tiles);
    else if (pr == 1) CPC_RESAMPLE_PHASES(1);
    else if (pr == 2) CPC_RESAMPLE_PHASES(2);
    else if (pr == 3) CPC_RESAMPLE_PHASES(3);
    else CPC_RESAMPLE_PHASES(4);
#undef CPC_RESAMPLE_PHASES
    CPC_CHECK_LAUNCH(by_phases ? "resample_phases_kernel" : "resample_kernel");
    return CPC_OK;
}

extern "C" int cpc_resample_to_pcm16(const float *y, long count, int16_t *q, unsigned long long *clamped, cpc_stream_t stream)
{
    CPC_REQUIRE(y != nullptr && q != nullptr && clamped != nullptr && count >= 0, "resample_to_pcm16: bad arguments (count=%ld)", count);
    if (count == 0) return CPC_OK;
    const unsigned blocks = (unsigned)std::min<long>(cpc::cdiv(count, cpc::PCM_THREADS), 4096);
    hipLaunchKernelGGL(cpc::pcm16_kernel, dim3(blocks), dim3(cpc::PCM_THREADS), 0, static_cast<hipStream_t>(stream), y, count,
                       reinterpret_cast<short *>(q), clamped);
    CPC_CHECK_LAUNCH("pcm16_kernel");
    return CPC_OK;
}
