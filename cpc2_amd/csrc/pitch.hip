// Pitch shift of device windows by a whole number of cents (the `pitch_wsola` augmentation; the definition is in
// include/cpc2_hip.h): a WSOLA time stretch by r = 2 ** (cents / 1200) followed by a windowed-sinc resampling by r, so that the
// output has the input's length.  The algorithm is this package's own; it is not sox's and claims no agreement with it.
//   pitch_search_kernel  one workgroup per window walks the only serial part, the chain of segment starts q_1, q_2, ...: per
//                        segment the 234 candidates' squared distances to the previous segment's tail (192 samples), one
//                        candidate per thread, one f64 chain per candidate, then the lexicographic minimum of (cost, candidate)
//   pitch_synth_kernel   one thread per output sample.  With the starts known a stretched sample s(m) is two reads of the window,
//                        so the stretched signal is never stored: every tap reads s(m) on the fly
// Built with -ffp-contract=off: the cost is stated as convert, subtract, square, add, and a host program repeats it bit for bit.
// No atomics; a window's bits depend on nothing but the window and its own row of the tables.
#include "common.h"

namespace cpc {

constexpr int PITCH_S = 1312, PITCH_O = 192, PITCH_R = 234, PITCH_HO = PITCH_S - PITCH_O;      // samples at 16 kHz
constexpr int PITCH_L = 6;                                 // half-width of the sinc in zero crossings
constexpr int PITCH_THREADS = 256;
constexpr int PITCH_SPAN = PITCH_R + PITCH_O - 1;          // samples the candidates of one segment meet
constexpr int PITCH_MAX_TAPS = 32;                         // 2 L / c + 1 <= 26 for |cents| <= 1200; the loop never runs beyond this
constexpr int PITCH_QS = 8;                                // starts a synthesis workgroup can meet (<= 3 for |cents| <= 1200)
constexpr double PITCH_PI = 3.14159265358979323846;

// a window of a [batch][window] buffer (offs == NULL) or of a flat vector: sample i, zero outside [0, W) and outside the vector
struct PitchSrc {
    const float *p;          // first sample of the window
    long lo, hi;             // readable indices [lo, hi) relative to p, already cut to [0, W)
};
__device__ __forceinline__ PitchSrc pitch_src(const float *base, long total, const long *offs, int b, int W)
{
    PitchSrc s;
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
__device__ __forceinline__ float pitch_read(const PitchSrc &s, long i) { return (i >= s.lo && i < s.hi) ? s.p[i] : 0.f; }

// ---------------------------------------------------------------- the chain of segment starts
// q[b][0] = 0; q[b][j] = the candidate nominal[b][j] - R / 2 + d, d < R, whose O samples are closest (squared distance, f64, k
// ascending) to the template x[q[j-1] + Ho ..], the lowest d on a tie.
// A segment's candidates start at first_j = nominal[j] - R / 2 whatever the chain does, and q_j lies in [first_j, first_j + R), so
// the template of segment j + 1 lies in x[first_j + Ho .. first_j + Ho + R + O - 1): both spans of the NEXT segment are fetched
// into registers while this segment's costs are added up, and the chain never waits for global memory.  The spans are kept in LDS
// as doubles (the conversion is exact and happens once per sample, not once per term).  Two barriers per segment.
__device__ __forceinline__ void pitch_fetch(const PitchSrc &x, long first, long tail_first, float (&seg)[2], float (&tail)[2])
{
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int i = threadIdx.x + u * PITCH_THREADS;
        seg[u] = i < PITCH_SPAN ? pitch_read(x, first + i) : 0.f;
        tail[u] = i < PITCH_SPAN ? pitch_read(x, tail_first + i) : 0.f;
    }
}
__global__ __launch_bounds__(PITCH_THREADS) void pitch_search_kernel(const float *src, long total, const long *offs,
                                                                     const int *nominal, int *q, int J, int W)
{
    static_assert(PITCH_SPAN <= 2 * PITCH_THREADS, "two samples per thread cover a span");
    __shared__ double seg[PITCH_SPAN];                        // x[first_j ..): candidate d is seg[d .. d + O)
    __shared__ double tail[PITCH_SPAN];                       // x[first_{j-1} + Ho ..): the template is tail[d_{j-1} .. + O)
    __shared__ double red_cost[PITCH_THREADS / 64];
    __shared__ int red_d[PITCH_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const PitchSrc x = pitch_src(src, total, offs, b, W);
    const int *nom = nominal + (long)b * J;
    int *qb = q + (long)b * J;
    if (tid == 0) qb[0] = 0;
    if (J < 2) return;
    long first = (long)nom[1] - PITCH_R / 2;                  // candidate d of segment j starts at first + d
    int dprev = 0;                                            // q_{j-1} = first_{j-1} + dprev (q_0 = 0: first_0 = 0)
    float nseg[2], ntail[2];
    pitch_fetch(x, first, PITCH_HO, nseg, ntail);
    for (int j = 1; j < J; ++j) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int i = tid + u * PITCH_THREADS;
            if (i < PITCH_SPAN) { seg[i] = (double)nseg[u]; tail[i] = (double)ntail[u]; }
        }
        __syncthreads();
        long first_next = 0;
        if (j + 1 < J) {
            first_next = (long)nom[j + 1] - PITCH_R / 2;
            pitch_fetch(x, first_next, first + PITCH_HO, nseg, ntail);
        }
        double cost = 0.0;
        int d = tid;
        if (tid < PITCH_R) {
            const double *cand = seg + tid, *tmpl = tail + dprev;
            for (int k = 0; k < PITCH_O; ++k) {
                const double e = cand[k] - tmpl[k];
                const double e2 = e * e;
                cost = cost + e2;
            }
        } else {
            cost = __longlong_as_double(0x7ff0000000000000LL);          // +inf: never chosen (a cost is finite or the input was not)
            d = PITCH_R;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double oc = __shfl_xor(cost, off, 64);
            const int od = __shfl_xor(d, off, 64);
            if (oc < cost || (oc == cost && od < d)) { cost = oc; d = od; }
        }
        // (red_* is written behind the next segment's first barrier only: every thread has read this segment's results by then;
        //  seg / tail are written behind this segment's second barrier only: every thread has added up its costs by then)
        if ((tid & 63) == 0) { red_cost[tid >> 6] = cost; red_d[tid >> 6] = d; }
        __syncthreads();
        cost = red_cost[0]; d = red_d[0];
#pragma unroll
        for (int w = 1; w < PITCH_THREADS / 64; ++w) {
            const double oc = red_cost[w];
            const int od = red_d[w];
            if (oc < cost || (oc == cost && od < d)) { cost = oc; d = od; }
        }
        if (d >= PITCH_R) d = 0;                              // (only when every cost is NaN: a non-finite window)
        if (tid == 0) qb[j] = (int)(first + d);
        dprev = d;
        first = first_next;
    }
}

// ---------------------------------------------------------------- resampling of the stretched signal
// y[n] = sum_m h(n r - m) s(m), h(t) = c sinc(c t) cos^2(pi c t / (2 L)) for |c t| < L.  The weights in f64, each rounded once to
// f32; the sum is one fmaf chain with m ascending.  sin and cos of the two phases are evaluated at the first tap and turned by
// the per-tap angle from there (a rotation in f64: its error after 26 steps stays below 1e-13 absolute, far below the f32
// rounding of a weight; the taps within 1 rad of the centre, where the sine is divided by a small argument, evaluate their own).
// cents == 0: the window itself, bit for bit.
__global__ __launch_bounds__(PITCH_THREADS) void pitch_synth_kernel(const float *src, long total, const long *offs,
                                                                    const double *ratio, const double *cutoff, const int *cents,
                                                                    const int *q, int J, float *out, int W)
{
    __shared__ int qs[PITCH_QS];
    const int b = blockIdx.y, tid = threadIdx.x;
    const long n0 = (long)blockIdx.x * PITCH_THREADS, n = n0 + tid;
    const PitchSrc x = pitch_src(src, total, offs, b, W);
    float *o = out + (long)b * W;
    if (cents[b] == 0) {
        if (n < W) o[n] = pitch_read(x, n);
        return;
    }
    const double r = ratio[b], c = cutoff[b];
    const double half = (double)PITCH_L / c;
    // the starts this workgroup can meet: from the segment before the one of its first tap
    double mf = ceil((double)n0 * r - half);
    if (mf < 0.0) mf = 0.0;
    long jbase = (long)mf / PITCH_HO - 1;
    if (jbase < 0) jbase = 0;
    if (tid < PITCH_QS) qs[tid] = jbase + tid < J ? q[(long)b * J + jbase + tid] : 0;
    __syncthreads();
    if (n >= W) return;

    const double pos = (double)n * r;
    long m = (long)ceil(pos - half);
    const double t0 = (pos - (double)m) * c;                  // c t of the first tap, about +L; falls by c per tap
    const double th = PITCH_PI * t0, ph = PITCH_PI * t0 / (2.0 * PITCH_L);
    const double dth = PITCH_PI * c, dph = PITCH_PI * c / (2.0 * PITCH_L);
    double s1 = sin(th), c1 = cos(th), s2 = sin(ph), c2 = cos(ph);
    const double ds1 = sin(dth), dc1 = cos(dth), ds2 = sin(dph), dc2 = cos(dph);
    float acc = 0.f;
    for (int i = 0; i < PITCH_MAX_TAPS; ++i, ++m) {
        const double ct = (pos - (double)m) * c;
        if (ct <= -(double)PITCH_L) break;
        if (ct < (double)PITCH_L && m >= 0) {
            const double arg = PITCH_PI * ct;
            // (near the centre the turned sine's ABSOLUTE error would be divided by a small argument: that tap takes its own sine)
            const double sinc = arg == 0.0 ? 1.0 : (fabs(arg) < 1.0 ? sin(arg) : s1) / arg;
            const float h = (float)(c * sinc * (c2 * c2));
            // s(m): segment j = m / Ho, k = m - j Ho; inside the overlap of j >= 1 the cross-fade from the previous segment's tail
            const long j = m / PITCH_HO;
            const int k = (int)(m - j * PITCH_HO);
            long jj = j - jbase;
            jj = jj < 0 ? 0 : (jj > PITCH_QS - 1 ? PITCH_QS - 1 : jj);          // (always inside: the clamp only guards the LDS read)
            const float bv = pitch_read(x, (long)qs[jj] + k);
            float s = bv;
            if (k < PITCH_O && j >= 1) {
                const float av = pitch_read(x, (long)qs[jj > 0 ? jj - 1 : 0] + PITCH_HO + k);
                s = (float)((double)av + ((double)k / (double)PITCH_O) * ((double)bv - (double)av));
            }
            acc = fmaf(h, s, acc);
        }
        // turn both phases by one tap: theta -= dtheta
        const double ns1 = s1 * dc1 - c1 * ds1, nc1 = c1 * dc1 + s1 * ds1;
        const double ns2 = s2 * dc2 - c2 * ds2, nc2 = c2 * dc2 + s2 * ds2;
        s1 = ns1; c1 = nc1; s2 = ns2; c2 = nc2;
    }
    o[n] = acc;
}

}  // namespace cpc

extern "C" int cpc_augment_pitch(const float *src, long src_total, const long *src_off, const double *ratio, const double *cutoff,
                                 const int *cents, int cents_bound, const int *nominal, int segments, float *out, int *q, int batch,
                                 int window, cpc_stream_t stream)
{
    CPC_REQUIRE(window > 0 && segments > 0 && batch >= 0 && batch <= 65535,
                "augment_pitch: bad arguments (batch=%d window=%d segments=%d)", batch, window, segments);
    CPC_REQUIRE(cents_bound >= 0 && cents_bound <= 1200, "augment_pitch: shifts of up to %d cents asked for; at most 1200 (an octave) "
                "either way are built", cents_bound);
    if (batch == 0) return CPC_OK;
    CPC_REQUIRE(src != nullptr && ratio != nullptr && cutoff != nullptr && cents != nullptr && nominal != nullptr &&
                out != nullptr && q != nullptr, "augment_pitch: a null pointer with batch=%d", batch);
    CPC_REQUIRE(src_off == nullptr || src_total > 0, "augment_pitch: a source read by offsets needs its vector's length");
    CPC_REQUIRE(src != out, "augment_pitch: the output must not be the input (every output reads many input samples)");
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(cpc::pitch_search_kernel, dim3((unsigned)batch), dim3(cpc::PITCH_THREADS), 0, st, src, src_total, src_off,
                       nominal, q, segments, window);
    CPC_CHECK_LAUNCH("pitch_search_kernel");
    hipLaunchKernelGGL(cpc::pitch_synth_kernel, dim3((unsigned)cpc::cdiv(window, cpc::PITCH_THREADS), (unsigned)batch),
                       dim3(cpc::PITCH_THREADS), 0, st, src, src_total, src_off, ratio, cutoff, cents, (const int *)q, segments, out,
                       window);
    CPC_CHECK_LAUNCH("pitch_synth_kernel");
    return CPC_OK;
}
