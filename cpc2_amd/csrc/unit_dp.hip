// Duration-penalized unit segmentation (cpc2_amd/unit_segmentation.py: segment_costs): the unit sequence that
// minimises the summed frame-to-code cost plus lambda per segment (Kamper & van Niekerk 2021, linear penalty), a Viterbi pass over
// the K codes with a switch cost.
//
// The definition (restated from include/cpc2_hip.h).  One utterance has costs c[t][k] (f32), one penalty lambda >= 0 (f64):
//   V[0][k] = (double) c[0][k]
//   m[t]    = min_k V[t][k]          a[t] = the LOWEST k with V[t][k] == m[t]   (m[t] is taken as V[t][a[t]])
//   sw      = m[t-1] + lambda                                  (one f64 add)
//   stay[t][k] = (V[t-1][k] <= sw)                             (a tie stays)
//   V[t][k] = (double) c[t][k] + (stay[t][k] ? V[t-1][k] : sw) (one f64 add)
//   u[T-1] = a[T-1];  u[t-1] = stay[t][u[t]] ? u[t] : a[t-1]
// Every step is one IEEE operation and a min is exact; the file is built with -ffp-contract=off like ctc_align.hip, so the output
// EQUALS a numpy float64 statement of these lines on every finite input, ties included.
//
//   unit_dp_prefix_kernel   one workgroup: the exclusive prefix of the lengths of the utterances that run (0 < T <= 2^24, rows
//                           inside the pack).  It gives every utterance its slot of back-pointers in scratch.
//   unit_dp_wave_kernel<R>  K <= UDP_WAVE_K = 256: one wave64 per (utterance, penalty), UDP_WAVES waves per workgroup which never
//                           meet at a barrier.  Lane l holds the states l + 64 j, j < R (R = 1, 2, 4 by K), in registers; the min
//                           by four DPP steps inside a row of 16 lanes and two xor shuffles across the rows, its lowest index
//                           by a ballot of the states equal to it; the rows of the next UDP_AHEAD frames are
//                           in registers before the current frames' reductions start.
//   unit_dp_wg_kernel<PER>  K <= 16384: one workgroup of 512 threads per (utterance, penalty), thread i holds the states
//                           i + 512 j, j < PER (PER = 2, 8, 32 by K), in registers; a wave reduces by shuffles, its lane 0 leaves
//                           (value, index) in one of two LDS rows chosen by the frame's parity, ONE barrier, every thread folds
//                           the eight entries.  Rows t + 1 and t + 2 are in flight while frame t is reduced.
//   Both write stay[t][.] as one bit per state (a ballot: 64 states are two 32-bit words) and a[t] to scratch, then walk back in
//   the same launch (backtrace): tiles of F frames x W = ceil(K / 32) words are copied to LDS (contiguous in scratch), ONE thread
//   walks the tile there, all threads store the tile's units.  F = 64 in the wave form, clamp(12288 / W, 24, 256) in the
//   workgroup form (at most 48 KiB of dynamic LDS, its base and every carve 16-byte aligned).
// The scan for non-finite costs rides on the row reads; such an utterance finishes its forward pass (nothing is indexed by a value)
// and skips the backtrace.  No atomics, no f32 accumulation, no grid-wide synchronisation; vector stores and plain C++ only.
#include "common.h"

namespace cpc {
namespace {

constexpr int UDP_WAVE_K = 256;                     // the largest K of the wave form
constexpr int UDP_WAVES = 4;                        // waves (grid entries) per workgroup of the wave form
constexpr int UDP_AHEAD = 4;                        // frames whose rows a wave holds ahead of the recurrence
constexpr int UDP_WAVE_TILE = 64;                   // frames per backtrace tile of the wave form
constexpr int UDP_WG_THREADS = 512;
constexpr int UDP_WG_WAVES = UDP_WG_THREADS / 64;
constexpr int UDP_WG_TILE_WORDS = 12288;            // back-pointer words per backtrace tile of the workgroup form (48 KiB)
constexpr int UDP_MAX_K = 16384;
constexpr int UDP_MAX_UTT = 1 << 20;
constexpr int UDP_MAX_PEN = 16;
constexpr int UDP_MAX_T = 1 << 24;
constexpr int UDP_SCAN_THREADS = 1024;
enum { UDP_DONE = 0, UDP_EMPTY = 1, UDP_NONFINITE = 2, UDP_OUTSIDE = 3 };

struct Penalties { double v[UDP_MAX_PEN]; };

__host__ __device__ inline int udp_words(int k) { return (k + 31) / 32; }
__host__ __device__ inline int udp_wg_tile(int w) { const int f = UDP_WG_TILE_WORDS / w; return f < 24 ? 24 : (f > 256 ? 256 : f); }

__device__ __forceinline__ bool udp_finite(float c) { return (__float_as_uint(c) & 0x7F800000u) != 0x7F800000u; }

// the utterance runs: it has frames, not more than the limit, and its rows lie inside the pack
__device__ __forceinline__ bool udp_runs(int64_t off, int T, long n_rows)
{
    return T > 0 && T <= UDP_MAX_T && off >= 0 && off <= (int64_t)n_rows && (int64_t)T <= (int64_t)n_rows - off;
}

__global__ void __launch_bounds__(UDP_SCAN_THREADS)
unit_dp_prefix_kernel(const int64_t *__restrict__ offsets, const int *__restrict__ lengths, int u, long n_rows,
                      int64_t *__restrict__ prefix)
{
    __shared__ int64_t s_sum[UDP_SCAN_THREADS];
    const int tid = threadIdx.x;
    const int per = (u + UDP_SCAN_THREADS - 1) / UDP_SCAN_THREADS;
    const int lo = min(tid * per, u), hi = min(lo + per, u);
    int64_t sum = 0;
    for (int i = lo; i < hi; ++i)
        if (udp_runs(offsets[i], lengths[i], n_rows)) sum += lengths[i];
    s_sum[tid] = sum;
    __syncthreads();
    for (int d = 1; d < UDP_SCAN_THREADS; d <<= 1) {                 // inclusive scan over the threads
        const int64_t v = tid >= d ? s_sum[tid - d] : 0;
        __syncthreads();
        s_sum[tid] += v;
        __syncthreads();
    }
    int64_t run = s_sum[tid] - sum;
    for (int i = lo; i < hi; ++i) {
        prefix[i] = run;
        if (udp_runs(offsets[i], lengths[i], n_rows)) run += lengths[i];
    }
}

// (value, index) of the smaller value, the lower index among equal values: a total order on non-NaN values, so every lane of a
// butterfly ends with the same pair
__device__ __forceinline__ void udp_take(double &bv, int &bi, double ov, int oi)
{
    if (ov < bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
}

__device__ __forceinline__ void udp_wave_min(double &bv, int &bi)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const double ov = __shfl_xor(bv, m, 64);
        const int oi = __shfl_xor(bi, m, 64);
        udp_take(bv, bi, ov, oi);
    }
}

// A row of 16 lanes through the DPP network (quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror: every lane reads a live
// lane), then the four rows by two xor shuffles: the wave's smallest value on every lane, without its index.
template <int CTRL> __device__ __forceinline__ double udp_dpp(double v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double udp_wave_min_value(double v)
{
    v = fmin(v, udp_dpp<0xB1>(v));
    v = fmin(v, udp_dpp<0x4E>(v));
    v = fmin(v, udp_dpp<0x141>(v));
    v = fmin(v, udp_dpp<0x140>(v));
    v = fmin(v, __shfl_xor(v, 16, 64));
    v = fmin(v, __shfl_xor(v, 32, 64));
    return v;
}

// the value of lane `src` (uniform over the wave)
__device__ __forceinline__ double udp_read_lane(double v, int src)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), src), __builtin_amdgcn_readlane(__double2loint(v), src));
}

// the threads that walk back together: a wave of a workgroup whose waves never meet, or a whole workgroup
template <bool WAVE> __device__ __forceinline__ void udp_sync()
{
    if (WAVE) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    } else {
        __syncthreads();
    }
}

// The walk back over frames T-1 .. 0 by `threads` threads (me = 0 .. threads - 1), tiles of F frames.  a_all[t] and the W words
// of frame t at bp_all + t * W were written by these same threads (frame 0 has no words and none is read).  LDS: s_ctl[4],
// s_a[F], s_u[F], s_tile[F * W].  Returns the number of segments (valid on me == 0).
template <bool WAVE>
__device__ __forceinline__ int udp_backtrace(int me, int threads, int T, int W, int F, const int *a_all, const unsigned *bp_all,
                                             int *s_ctl, int *s_a, int *s_u, unsigned *s_tile, int *__restrict__ units)
{
    udp_sync<WAVE>();                                                // the forward pass's global writes before these reads
    if (me == 0) s_ctl[0] = a_all[T - 1];
    int nseg = 1;
    for (int hi = T - 1; hi >= 0; hi -= F) {
        const int lo = max(hi - F + 1, 0), n = hi - lo + 1;
        for (int f = me; f < n; f += threads) s_a[f] = lo + f >= 1 ? a_all[lo + f - 1] : 0;      // a[t - 1] of frame t = lo + f
        const int first = max(lo, 1);                                // (frame 0 has no back-pointer words)
        const unsigned *src = bp_all + (size_t)first * W;
        const int words = (hi - first + 1) * W, skip = (first - lo) * W;
        for (int x = me; x < words; x += threads) s_tile[skip + x] = src[x];
        udp_sync<WAVE>();
        if (me == 0) {
            int u = s_ctl[0];
            for (int t = hi; t >= lo; --t) {
                s_u[t - lo] = u;
                if (t >= 1) {
                    const unsigned word = s_tile[(t - lo) * W + (u >> 5)];
                    const int before = ((word >> (u & 31)) & 1u) ? u : s_a[t - lo];
                    nseg += before != u;
                    u = before;
                }
            }
            s_ctl[0] = u;                                            // u[lo - 1]
        }
        udp_sync<WAVE>();
        for (int f = me; f < n; f += threads) units[lo + f] = s_u[f];
        udp_sync<WAVE>();                                            // (the tile is overwritten next)
    }
    return nseg;
}

struct UdpArgs {
    const float *cost;
    long n_rows, ld;
    int k;
    const int64_t *offsets;
    const int *lengths;
    int n_utt, n_pen;
    Penalties pen;
    int *units;
    double *energy;
    int *n_segments, *status;
    const int64_t *prefix;
    int *a_all;                  // [n_pen][cap]
    unsigned *bp_all;            // [n_pen][cap][W]
    long cap;                    // frames of back-pointers the scratch holds per penalty
};

// What one grid entry does before its frames: 0 when it runs, else the status is written (by `writer`) and nothing is read
__device__ __forceinline__ int udp_entry_status(const UdpArgs &A, int i, int e, bool writer)
{
    const int T = A.lengths[i];
    int st = UDP_DONE;
    if (T <= 0) st = UDP_EMPTY;
    else if (!udp_runs(A.offsets[i], T, A.n_rows) || A.prefix[i] + (int64_t)T > (int64_t)A.cap) st = UDP_OUTSIDE;
    if (st != UDP_DONE && writer) {
        A.energy[e] = st == UDP_EMPTY ? 0.0 : __builtin_nan("");
        A.n_segments[e] = 0;
        A.status[e] = st;
    }
    return st;
}

template <int R>
__global__ void __launch_bounds__(64 * UDP_WAVES)
unit_dp_wave_kernel(const UdpArgs A)
{
    extern __shared__ __attribute__((aligned(16))) char udp_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long entry = (long)blockIdx.x * UDP_WAVES + wave;
    if (entry >= (long)A.n_utt * A.n_pen) return;                    // (a whole wave; the waves of a workgroup never meet)
    const int i = (int)(entry / A.n_pen), p = (int)(entry % A.n_pen);
    const int e = p * A.n_utt + i;
    if (udp_entry_status(A, i, e, lane == 0) != UDP_DONE) return;
    const int K = A.k, W = udp_words(K), T = A.lengths[i];
    const int64_t off = A.offsets[i];
    const float *x = A.cost + (size_t)off * A.ld;
    const size_t slot = (size_t)p * A.cap + (size_t)A.prefix[i];
    int *a_out = A.a_all + slot;
    unsigned *bp = A.bp_all + slot * W;
    int *units = A.units + (size_t)p * A.n_rows + off;
    const double lam = A.pen.v[p];
    const float inf = __builtin_inff();

    bool valid[R];
#pragma unroll
    for (int j = 0; j < R; ++j) valid[j] = lane + 64 * j < K;
    auto load_row = [&](int t, float (&c)[R]) {                      // a frame beyond the end re-reads the last one: never out of bounds
        const float *row = x + (size_t)min(t, T - 1) * A.ld;
#pragma unroll
        for (int j = 0; j < R; ++j) c[j] = valid[j] ? row[lane + 64 * j] : inf;
    };

    double V[R];
    double m = 0.0;
    bool bad = false;
    float cur[UDP_AHEAD][R], nxt[UDP_AHEAD][R];
#pragma unroll
    for (int s = 0; s < UDP_AHEAD; ++s) load_row(s, cur[s]);
    for (int t0 = 0; t0 < T; t0 += UDP_AHEAD) {
#pragma unroll
        for (int s = 0; s < UDP_AHEAD; ++s) load_row(t0 + UDP_AHEAD + s, nxt[s]);
#pragma unroll
        for (int s = 0; s < UDP_AHEAD; ++s) {
            const int t = t0 + s;
            if (t < T) {                                             // (uniform over the wave)
                const double sw = m + lam;
                double low = 0.0;
#pragma unroll
                for (int j = 0; j < R; ++j) {
                    const float c = cur[s][j];
                    bad |= valid[j] && !udp_finite(c);
                    if (t == 0) {
                        V[j] = (double)c;
                    } else {
                        const bool stay = V[j] <= sw;
                        V[j] = (double)c + (stay ? V[j] : sw);
                        const unsigned long long mask = __ballot(stay && valid[j]);
                        if (lane < 2 && 2 * j + lane < W) bp[(size_t)t * W + 2 * j + lane] = (unsigned)(mask >> (32 * lane));
                    }
                    low = j == 0 ? V[0] : fmin(low, V[j]);
                }
                // the value first, then its lowest index: state lane + 64 j, so the first j with a lane at the minimum and the lowest
                // such lane; m is that state's own value (-0.0 and +0.0 compare equal: the one at the lowest index is carried)
                low = udp_wave_min_value(low);
                int bi = 0;
                bool found = false;
#pragma unroll
                for (int j = 0; j < R; ++j) {
                    const unsigned long long at = __ballot(V[j] == low);
                    if (!found && at != 0ull) {                      // (uniform over the wave)
                        const int src = __ffsll((long long)at) - 1;
                        bi = src + 64 * j;
                        low = udp_read_lane(V[j], src);
                        found = true;
                    }
                }
                m = low;
                if (lane == 0) a_out[t] = bi;
            }
        }
#pragma unroll
        for (int s = 0; s < UDP_AHEAD; ++s)
#pragma unroll
            for (int j = 0; j < R; ++j) cur[s][j] = nxt[s][j];
    }

    if (__ballot(bad) != 0ull) {
        for (int t = lane; t < T; t += 64) units[t] = -1;
        if (lane == 0) { A.energy[e] = __builtin_nan(""); A.n_segments[e] = 0; A.status[e] = UDP_NONFINITE; }
        return;
    }
    const int per_wave = 16 + 4 * (2 * UDP_WAVE_TILE + UDP_WAVE_TILE * W);       // bytes; a multiple of 16
    char *mine = udp_lds + (size_t)wave * per_wave;
    int *s_ctl = reinterpret_cast<int *>(mine), *s_a = s_ctl + 4, *s_u = s_a + UDP_WAVE_TILE;
    unsigned *s_tile = reinterpret_cast<unsigned *>(s_u + UDP_WAVE_TILE);
    const int nseg = udp_backtrace<true>(lane, 64, T, W, UDP_WAVE_TILE, a_out, bp, s_ctl, s_a, s_u, s_tile, units);
    if (lane == 0) { A.energy[e] = m; A.n_segments[e] = nseg; A.status[e] = UDP_DONE; }
}

template <int PER>
__global__ void __launch_bounds__(UDP_WG_THREADS)
unit_dp_wg_kernel(const UdpArgs A)
{
    extern __shared__ __attribute__((aligned(16))) char udp_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = (int)(blockIdx.x / (unsigned)A.n_pen), p = (int)(blockIdx.x % (unsigned)A.n_pen);
    const int e = p * A.n_utt + i;
    if (udp_entry_status(A, i, e, tid == 0) != UDP_DONE) return;     // (the whole workgroup)
    const int K = A.k, W = udp_words(K), T = A.lengths[i], F = udp_wg_tile(W);
    const int64_t off = A.offsets[i];
    const float *x = A.cost + (size_t)off * A.ld;
    const size_t slot = (size_t)p * A.cap + (size_t)A.prefix[i];
    int *a_out = A.a_all + slot;
    unsigned *bp = A.bp_all + slot * W;
    int *units = A.units + (size_t)p * A.n_rows + off;
    const double lam = A.pen.v[p];
    const float inf = __builtin_inff();
    // LDS: [2][8] f64 minima | [2][8] their indices | ctl[4] | bad[8] ... then the backtrace's s_a[F] s_u[F] s_tile[F W]
    double *s_rv = reinterpret_cast<double *>(udp_lds);
    int *s_ri = reinterpret_cast<int *>(udp_lds + 128);
    int *s_ctl = reinterpret_cast<int *>(udp_lds + 192);
    int *s_bad = reinterpret_cast<int *>(udp_lds + 208);
    int *s_a = reinterpret_cast<int *>(udp_lds + 256), *s_u = s_a + 256;
    unsigned *s_tile = reinterpret_cast<unsigned *>(s_u + 256);

    const int nper = (K + UDP_WG_THREADS - 1) / UDP_WG_THREADS;      // <= PER
    auto load_row = [&](int t, float (&c)[PER]) {
        const float *row = x + (size_t)min(t, T - 1) * A.ld;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int k = tid + UDP_WG_THREADS * j;
            c[j] = (j < nper && k < K) ? row[k] : inf;
        }
    };

    double V[PER];
    double m = 0.0;
    bool bad = false;
    float c0[PER], c1[PER], cn[PER];
    load_row(0, c0);
    load_row(1, c1);
    for (int t = 0; t < T; ++t) {
        load_row(t + 2, cn);
        const double sw = m + lam;
        double bv = __builtin_inf();
        int bi = tid;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            if (j < nper) {                                          // (uniform over the workgroup)
                const int k = tid + UDP_WG_THREADS * j;
                const bool valid = k < K;
                const float c = c0[j];
                bad |= valid && !udp_finite(c);
                if (t == 0) {
                    V[j] = (double)c;
                } else {
                    const bool stay = V[j] <= sw;
                    V[j] = (double)c + (stay ? V[j] : sw);
                    const unsigned long long mask = __ballot(stay && valid);
                    const int word = 2 * wave + (UDP_WG_THREADS / 32) * j + lane;
                    if (lane < 2 && word < W) bp[(size_t)t * W + word] = (unsigned)(mask >> (32 * lane));
                }
                if (j == 0) { bv = V[0]; bi = k; }
                else udp_take(bv, bi, V[j], k);
            }
        }
        udp_wave_min(bv, bi);
        double *rv = s_rv + (t & 1) * UDP_WG_WAVES;                  // (two rows by parity: a wave a frame ahead writes the other one)
        int *ri = s_ri + (t & 1) * UDP_WG_WAVES;
        if (lane == 0) { rv[wave] = bv; ri[wave] = bi; }
        __syncthreads();
        bv = rv[0];
        bi = ri[0];
#pragma unroll
        for (int w = 1; w < UDP_WG_WAVES; ++w) udp_take(bv, bi, rv[w], ri[w]);
        m = bv;
        if (tid == 0) a_out[t] = bi;
#pragma unroll
        for (int j = 0; j < PER; ++j) { c0[j] = c1[j]; c1[j] = cn[j]; }
    }

    const bool wave_bad = __ballot(bad) != 0ull;
    __syncthreads();
    if (lane == 0) s_bad[wave] = wave_bad ? 1 : 0;
    __syncthreads();
    int any_bad = 0;
#pragma unroll
    for (int w = 0; w < UDP_WG_WAVES; ++w) any_bad |= s_bad[w];
    if (any_bad) {
        for (int t = tid; t < T; t += UDP_WG_THREADS) units[t] = -1;
        if (tid == 0) { A.energy[e] = __builtin_nan(""); A.n_segments[e] = 0; A.status[e] = UDP_NONFINITE; }
        return;
    }
    const int nseg = udp_backtrace<false>(tid, UDP_WG_THREADS, T, W, F, a_out, bp, s_ctl, s_a, s_u, s_tile, units);
    if (tid == 0) { A.energy[e] = m; A.n_segments[e] = nseg; A.status[e] = UDP_DONE; }
}

bool udp_sizes_ok(const char *who, int n_utt, int k, int n_pen)
{
    if (n_utt < 0 || n_utt > UDP_MAX_UTT || k < 1 || k > UDP_MAX_K || n_pen < 1 || n_pen > UDP_MAX_PEN) {
        set_error("%s: sizes outside the supported limits (n_utt=%d k=%d n_pen=%d; need 0 <= n_utt <= %d, 1 <= k <= %d, "
                  "1 <= n_pen <= %d)", who, n_utt, k, n_pen, UDP_MAX_UTT, UDP_MAX_K, UDP_MAX_PEN);
        return false;
    }
    return true;
}

size_t udp_prefix_bytes(int n_utt) { return align_up(sizeof(int64_t) * ((size_t)n_utt + 1), 256); }
// one int of a[t] and W words of stay bits per (penalty, frame)
size_t udp_frame_bytes(int k, int n_pen) { return sizeof(int) * (size_t)n_pen * ((size_t)udp_words(k) + 1); }

template <int R> int launch_wave(const UdpArgs &A, hipStream_t st)
{
    const long entries = (long)A.n_utt * A.n_pen;
    const size_t lds = (size_t)UDP_WAVES * (16 + 4 * (2 * UDP_WAVE_TILE + UDP_WAVE_TILE * udp_words(A.k)));
    hipLaunchKernelGGL(unit_dp_wave_kernel<R>, dim3((unsigned)cdiv(entries, UDP_WAVES)), dim3(64 * UDP_WAVES), lds, st, A);
    CPC_CHECK_LAUNCH("unit_dp_wave_kernel");
    return CPC_OK;
}

template <int PER> int launch_wg(const UdpArgs &A, hipStream_t st)
{
    const int w = udp_words(A.k);
    const size_t lds = 256 + 4 * (size_t)(2 * 256 + udp_wg_tile(w) * w);
    hipLaunchKernelGGL(unit_dp_wg_kernel<PER>, dim3((unsigned)((long)A.n_utt * A.n_pen)), dim3(UDP_WG_THREADS), lds, st, A);
    CPC_CHECK_LAUNCH("unit_dp_wg_kernel");
    return CPC_OK;
}

}  // namespace
}  // namespace cpc

extern "C" int cpc_segment_units_wave_k(void) { return cpc::UDP_WAVE_K; }

extern "C" size_t cpc_segment_units_scratch_bytes(int n_utt, long total_frames, int k, int n_pen)
{
    if (!cpc::udp_sizes_ok("segment_units", n_utt, k, n_pen)) return 0;
    if (total_frames < 0) {
        cpc::set_error("segment_units: total_frames=%ld must be >= 0", total_frames);
        return 0;
    }
    return cpc::udp_prefix_bytes(n_utt) + cpc::align_up(cpc::udp_frame_bytes(k, n_pen) * (size_t)total_frames, 256) + 256;
}

extern "C" int cpc_segment_units(const float *cost, long n_rows, long ld, int k, const int64_t *offsets, const int *lengths, int n_utt,
                           const double *penalties_host, int n_pen, int *units, double *energy, int *n_segments, int *status,
                           void *scratch, size_t scratch_bytes, cpc_stream_t stream)
{
    if (!cpc::udp_sizes_ok("segment_units", n_utt, k, n_pen)) return CPC_ERR_INVALID;
    CPC_REQUIRE(n_rows >= 0 && ld >= k, "segment_units: n_rows=%ld must be >= 0 and ld=%ld >= k=%d", n_rows, ld, k);
    CPC_REQUIRE(penalties_host != nullptr, "segment_units: null penalties");
    cpc::UdpArgs A;
    for (int p = 0; p < n_pen; ++p) {
        const double lam = penalties_host[p];
        CPC_REQUIRE(lam >= 0.0 && lam <= 1.7976931348623157e308, "segment_units: penalty %d = %g must be finite and >= 0", p, lam);
        A.pen.v[p] = lam;
    }
    for (int p = n_pen; p < cpc::UDP_MAX_PEN; ++p) A.pen.v[p] = 0.0;
    if (n_utt == 0) return CPC_OK;
    CPC_REQUIRE(cost && offsets && lengths && units && energy && n_segments && status, "segment_units: null buffer");
    CPC_REQUIRE(scratch != nullptr, "segment_units: null scratch");
    const size_t fixed = cpc::udp_prefix_bytes(n_utt) + 256, per_frame = cpc::udp_frame_bytes(k, n_pen);
    if (scratch_bytes < fixed) {
        cpc::set_error("segment_units: scratch of %zu bytes, cpc_segment_units_scratch_bytes(%d, 0, %d, %d) = %zu", scratch_bytes, n_utt, k, n_pen,
                       fixed);
        return CPC_ERR_WORKSPACE;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    // the frames of back-pointers the scratch holds: what cpc_segment_units_scratch_bytes was asked for, or more
    const size_t cap = (scratch_bytes - fixed) / per_frame;
    char *base = static_cast<char *>(scratch);
    int64_t *prefix = reinterpret_cast<int64_t *>(base);
    A.cost = cost; A.n_rows = n_rows; A.ld = ld; A.k = k; A.offsets = offsets; A.lengths = lengths; A.n_utt = n_utt; A.n_pen = n_pen;
    A.units = units; A.energy = energy; A.n_segments = n_segments; A.status = status; A.prefix = prefix;
    A.cap = (long)cap;
    A.a_all = reinterpret_cast<int *>(base + cpc::udp_prefix_bytes(n_utt));
    A.bp_all = reinterpret_cast<unsigned *>(A.a_all + (size_t)n_pen * cap);
    hipLaunchKernelGGL(cpc::unit_dp_prefix_kernel, dim3(1), dim3(cpc::UDP_SCAN_THREADS), 0, st, offsets, lengths, n_utt, n_rows, prefix);
    CPC_CHECK_LAUNCH("unit_dp_prefix_kernel");
    if (k <= 64) return cpc::launch_wave<1>(A, st);
    if (k <= 128) return cpc::launch_wave<2>(A, st);
    if (k <= cpc::UDP_WAVE_K) return cpc::launch_wave<4>(A, st);
    if (k <= 2 * cpc::UDP_WG_THREADS) return cpc::launch_wg<2>(A, st);
    if (k <= 8 * cpc::UDP_WG_THREADS) return cpc::launch_wg<8>(A, st);
    return cpc::launch_wg<32>(A, st);
}
