// Artificial reverberation of device windows (the `freeverb` augmentation; the definition is in include/cpc2_hip.h): the
// public-domain Freeverb network, eight parallel feedback comb filters with a one-pole low-pass in the loop, then four all-pass
// filters in series, one mono bank, delay lengths scaled to 16 kHz.  The definition is this package's own; it is the algorithm
// behind sox's `reverb` but claims no agreement with sox's output (unmeasured).
//   freeverb_kernel  one workgroup per window; the twelve delay lines live in LDS and the window is streamed through in chunks of
//                    256 samples.  Per chunk: (1) u = g x into LDS, the next chunk's samples already on their way; (2) wave 0
//                    walks the eight combs in blocks of 32 samples: a comb at sample n reads what it wrote at n - D and D >= 40,
//                    so inside a block only the one-pole s = o + (s - o) dmp is serial -- its 32 steps run with a comb per lane,
//                    then 64 lanes write the block's line values u + s fb and hand the comb outputs on; (3) the eight comb
//                    outputs are added in comb order, one thread per sample; (4) each all-pass is walked by one thread per line
//                    POSITION (samples i, i + A, i + 2A, ... of the chunk meet the same position and nothing else does), four
//                    barriers; (5) y = x + v.  A table with a length below 32 (no room of the definition) takes a plain walk.
// Built with -ffp-contract=off: every operation is the statement's, in the statement's order, so the output equals a float32
// evaluation of the definition operation for operation.  No atomics, no global scratch; a window's bits depend on nothing but the
// window, its row of comb_len and the scalars.
#include "common.h"

#include <cmath>

namespace cpc {

constexpr int FV_COMBS = 8, FV_ALLPASS = 4;
constexpr int FV_THREADS = 256;
constexpr int FV_CHUNK = FV_THREADS;                        // one sample per thread in the parallel phases
constexpr int FV_BLOCK = 32;                                // comb samples per block: no valid comb is shorter (D >= 40)
constexpr int FV_SSTRIDE = FV_BLOCK + 8;                    // row stride of the block's one-pole states (16-byte rows, 8 banks apart)
constexpr int FV_OSTRIDE = FV_CHUNK + 1;                    // row stride of the comb outputs (the 8 lanes write 8 different banks)
constexpr int FV_MAX_LEN = 1024;                            // bound on len_bound and on an all-pass length

struct FvAllpass { int len[FV_ALLPASS]; };

static inline size_t fv_lds_floats(int len_bound, const int *allpass)
{
    size_t n = (size_t)FV_COMBS * (len_bound + FV_BLOCK + FV_SSTRIDE) + 2 * FV_CHUNK + (size_t)FV_COMBS * FV_OSTRIDE;
    for (int a = 0; a < FV_ALLPASS; ++a) n += allpass[a];
    return n;
}

// a window of a [batch][window] buffer (offs == NULL) or of a flat vector: sample i, zero outside [0, W) and outside the vector
struct FvSrc {
    const float *p;          // first sample of the window
    long lo, hi;             // readable indices [lo, hi) relative to p, already cut to [0, W)
};
__device__ __forceinline__ FvSrc fv_src(const float *base, long total, const long *offs, int b, int W)
{
    FvSrc s;
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
__device__ __forceinline__ float fv_read(const FvSrc &s, long i) { return (i >= s.lo && i < s.hi) ? s.p[i] : 0.f; }

// One comb, one sample: o = line[p]; s = o + (s - o) dmp; line[p] = u + s fb; p = (p + 1) % D.  (The path of a table with a
// length below FV_BLOCK, which no room of the definition has.)
__device__ __forceinline__ float fv_comb_step(float *line, int &p, int D, float u, float &s, float dmp, float fb)
{
    const float o = line[p];
    s = o + (s - o) * dmp;
    line[p] = u + s * fb;
    p = p + 1 == D ? 0 : p + 1;
    return o;
}

// A block of FV_BLOCK <= D samples of one comb.  A comb reads what it wrote D samples ago, so within a block nothing depends on
// the block's own line writes and only the one-pole is serial.
//   reads   the block's o straight off the line: the mirror of the line's first FV_BLOCK positions behind its end makes
//           p .. p + 31 contiguous
//   chain   s = o + (s - o) dmp, sample after sample; the 32 states go to a row of sbuf
//   update  64 lanes, lane (comb, j) at samples j + 8 k: o to obuf, line[q] = u + s fb, and its mirror where q has one
__device__ __forceinline__ void fv_block_reads(const float *rd, float (&ov)[FV_BLOCK])
{
#pragma unroll
    for (int j = 0; j < FV_BLOCK; ++j) ov[j] = rd[j];
}
__device__ __forceinline__ void fv_block_chain(const float (&ov)[FV_BLOCK], float &s, float dmp, float *srow)
{
#pragma unroll
    for (int j = 0; j < FV_BLOCK; j += 4) {
        float4 sv;
        s = ov[j] + (s - ov[j]) * dmp;             sv.x = s;
        s = ov[j + 1] + (s - ov[j + 1]) * dmp;     sv.y = s;
        s = ov[j + 2] + (s - ov[j + 2]) * dmp;     sv.z = s;
        s = ov[j + 3] + (s - ov[j + 3]) * dmp;     sv.w = s;
        *reinterpret_cast<float4 *>(srow + j) = sv;
    }
}
__device__ __forceinline__ void fv_block_update(float *line2, int p2, int D2, const float *u, const float *srow2, float *orow2, int j2,
                                                float fb)
{
#pragma unroll
    for (int k = 0; k < FV_BLOCK / 8; ++k) {
        const int ii = j2 + 8 * k;
        unsigned q = (unsigned)(p2 + ii);
        q = q < q - (unsigned)D2 ? q : q - (unsigned)D2;      // (p2 + ii) % D2: the difference wraps when q < D2
        const float oo = line2[q];
        const float val = u[ii] + srow2[ii] * fb;
        orow2[ii] = oo;
        line2[q] = val;
        line2[q < (unsigned)FV_BLOCK ? q + (unsigned)D2 : q] = val;          // the mirror (or the same place again)
    }
}
__device__ __forceinline__ int fv_advance(int p, int D) { return p + FV_BLOCK >= D ? p + FV_BLOCK - D : p + FV_BLOCK; }

__device__ __forceinline__ void fv_wave_sync()
{
    // LDS traffic of one wave is served in order; this keeps the compiler from moving it across the hand-over between lanes
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(FV_THREADS) void freeverb_kernel(const float *src, long total, const long *offs, const int *comb_len,
                                                              int len_bound, FvAllpass ap, float fb, float dmp, float g, float *out,
                                                              int W)
{
    extern __shared__ __attribute__((aligned(16))) float fv_lds[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int ap_total = ap.len[0] + ap.len[1] + ap.len[2] + ap.len[3];
    const int stride = len_bound + FV_BLOCK;                  // a comb's row: D[c] positions, then the mirror of its first FV_BLOCK
    float *sbuf = fv_lds;                                     // [8][SSTRIDE] the one-pole states of a block (16-byte rows)
    float *lines = sbuf + FV_COMBS * FV_SSTRIDE;              // [8][stride]
    float *apl = lines + FV_COMBS * stride;                   // the four all-pass lines, one after the other
    float *ubuf = apl + ap_total;                             // [CHUNK] g x
    float *vbuf = ubuf + FV_CHUNK;                            // [CHUNK] the comb sum, then each all-pass's output in place
    float *obuf = vbuf + FV_CHUNK;                            // [8][OSTRIDE] the comb outputs of the chunk
    for (int i = tid; i < FV_COMBS * stride + ap_total; i += FV_THREADS) lines[i] = 0.f;

    // the lengths, clamped into [1, len_bound]: a bad table can cost sense, never an index outside a line
    int min_len = len_bound;
    int D = 1, D2 = 1;
#pragma unroll
    for (int c = 0; c < FV_COMBS; ++c) {
        int d = comb_len[(long)b * FV_COMBS + c];
        d = d < 1 ? 1 : (d > len_bound ? len_bound : d);
        min_len = d < min_len ? d : min_len;
        if (c == (tid & 7)) D = d;
        if (c == ((tid >> 3) & 7)) D2 = d;
    }
    const bool blocked = min_len >= FV_BLOCK;                 // (uniform; every room of the definition has D >= 40)
    // wave 0 walks the combs.  Lane l runs the one-pole of comb l % 8 (serial part) and updates comb l / 8 at the block's samples
    // l % 8 + 8 k (parallel part).  p / p2: the position of the block's first sample, as either part sees its comb.
    const int c1 = tid & 7, c2 = (tid >> 3) & 7, j2 = tid & 7;
    float *line = lines + c1 * stride, *line2 = lines + c2 * stride;
    float *srow = sbuf + c1 * FV_SSTRIDE, *srow2 = sbuf + c2 * FV_SSTRIDE;
    float *orow = obuf + c1 * FV_OSTRIDE, *orow2 = obuf + c2 * FV_OSTRIDE;
    int p = 0, p2 = 0;
    float s = 0.f;
    int pa[FV_ALLPASS] = {0, 0, 0, 0};                        // all-pass positions at the chunk's first sample (uniform)

    const FvSrc x = fv_src(src, total, offs, b, W);
    float *o = out + (long)b * W;
    float xnext = tid < W ? fv_read(x, tid) : 0.f;
    for (int n0 = 0; n0 < W; n0 += FV_CHUNK) {
        const int n = W - n0 < FV_CHUNK ? W - n0 : FV_CHUNK;
        const float xc = xnext;
        ubuf[tid] = g * xc;                                   // (zero beyond the window's end)
        const long nx = (long)n0 + FV_CHUNK + tid;
        xnext = nx < W ? fv_read(x, nx) : 0.f;                // (used in the next round: the load has this chunk to arrive)
        __syncthreads();                                      // B1

        if (tid < 64 && blocked) {
            // Blocks of FV_BLOCK <= D samples (the helpers above).  Every lane of the wave runs the serial part -- lane l repeats
            // comb l % 8 and stores the same values to the same addresses -- so a block is straight-line code.  A last block that
            // passes the window's end computes samples nobody reads from state nobody uses again.
            float ov[FV_BLOCK];
            for (int i = 0; i < n; i += FV_BLOCK) {
                fv_block_reads(line + p, ov);
                fv_block_chain(ov, s, dmp, srow);
                p = fv_advance(p, D);
                fv_wave_sync();
                fv_block_update(line2, p2, D2, ubuf + i, srow2, orow2 + i, j2, fb);
                p2 = fv_advance(p2, D2);
                fv_wave_sync();
            }
        } else if (!blocked && tid < FV_COMBS) {
            for (int i = 0; i < n; ++i) orow[i] = fv_comb_step(line, p, D, ubuf[i], s, dmp, fb);
        }
        __syncthreads();                                      // B2

        if (tid < n) {
            float acc = 0.f;
#pragma unroll
            for (int c = 0; c < FV_COMBS; ++c) acc = acc + obuf[c * FV_OSTRIDE + tid];
            vbuf[tid] = acc;
        }
        __syncthreads();                                      // B3

        // all-pass a: o = line[p]; line[p] = v + o / 2; v = o - v.  Samples j, j + A, ... of the chunk meet position
        // (pa + j) % A and no other sample does: one thread per position walks them with the line value in a register.
        int base = 0;
#pragma unroll
        for (int a = 0; a < FV_ALLPASS; ++a) {
            const int A = ap.len[a];
            float *ln = apl + base;
            for (int j = tid; j < A && j < n; j += FV_THREADS) {
                int pos = pa[a] + j;
                if (pos >= A) pos -= A;
                float held = ln[pos];
                for (int i = j; i < n; i += A) {
                    const float v = vbuf[i];
                    const float w = v + held * 0.5f;
                    vbuf[i] = held - v;
                    held = w;
                }
                ln[pos] = held;
            }
            pa[a] = (pa[a] + n) % A;
            base += A;
            __syncthreads();
        }
        if (tid < n) o[n0 + tid] = xc + vbuf[tid];
    }
}

}  // namespace cpc

extern "C" int cpc_augment_freeverb(const float *src, long src_total, const long *src_off, const int *comb_len, int len_bound,
                                    const int *allpass_len, float feedback, float damping, float gain, float *out, int batch,
                                    int window, cpc_stream_t stream)
{
    CPC_REQUIRE(window > 0 && batch >= 0 && batch <= 65535, "augment_freeverb: bad arguments (batch=%d window=%d)", batch, window);
    CPC_REQUIRE(len_bound >= 1 && len_bound <= cpc::FV_MAX_LEN, "augment_freeverb: len_bound=%d, comb lines of 1 to %d samples are "
                "built", len_bound, cpc::FV_MAX_LEN);
    CPC_REQUIRE(allpass_len != nullptr, "augment_freeverb: no all-pass lengths");
    for (int a = 0; a < cpc::FV_ALLPASS; ++a)
        CPC_REQUIRE(allpass_len[a] >= 1 && allpass_len[a] <= cpc::FV_MAX_LEN, "augment_freeverb: allpass_len[%d]=%d, all-pass lines "
                    "of 1 to %d samples are built", a, allpass_len[a], cpc::FV_MAX_LEN);
    CPC_REQUIRE(std::isfinite(feedback) && std::isfinite(damping) && std::isfinite(gain), "augment_freeverb: a scalar is not finite");
    CPC_REQUIRE(feedback >= 0.f && feedback < 1.f, "augment_freeverb: feedback=%g outside [0, 1)", (double)feedback);
    CPC_REQUIRE(damping >= 0.f && damping <= 1.f, "augment_freeverb: damping=%g outside [0, 1]", (double)damping);
    if (batch == 0) return CPC_OK;
    CPC_REQUIRE(src != nullptr && comb_len != nullptr && out != nullptr, "augment_freeverb: a null pointer with batch=%d", batch);
    CPC_REQUIRE(src_off == nullptr || src_total > 0, "augment_freeverb: a source read by offsets needs its vector's length");
    CPC_REQUIRE(src != out, "augment_freeverb: the output must not be the input");
    cpc::FvAllpass ap;
    for (int a = 0; a < cpc::FV_ALLPASS; ++a) ap.len[a] = allpass_len[a];
    const size_t lds = cpc::fv_lds_floats(len_bound, allpass_len) * sizeof(float);          // at most 61728 bytes
    hipLaunchKernelGGL(cpc::freeverb_kernel, dim3((unsigned)batch), dim3(cpc::FV_THREADS), lds, static_cast<hipStream_t>(stream), src,
                       src_total, src_off, comb_len, len_bound, ap, feedback, damping, gain, out, window);
    CPC_CHECK_LAUNCH("freeverb_kernel");
    return CPC_OK;
}
