// Log-mel and MFCC baseline features in f64 from exact f32 samples (cpc2_amd/spectral.py; the definition is in
// include/cpc2_hip.h, the argument in DESIGN.md section 18).
//
//   mel_db_kernel      one workgroup per (signal, tile of MF_FT = 16 frames).  It stages the tile's span of samples into LDS as
//                      f32, reflected by index, and forms the windowed DFT on v_mfma_f64_16x16x4_f64 against the twiddle table
//                      in global memory.  cos is even and sin odd about n_fft / 2, so the windowed samples n and n_fft - n are
//                      folded first: re = [16 frames x H] (a[n] + a[n_fft - n]) by [H x n_freqs] cos, im = the differences by
//                      sin, H = n_fft / 2 + 1 rows each -- half the products and half the table of the plain form.  Each wave
//                      owns every fourth tile of 16 frequencies and keeps its cos and its sin accumulator side by side: same
//                      lane map, so re^2 + im^2 is register-local.  It then leaves the power tile in LDS, multiplies it by the filterbank on the same instruction,
//                      takes 10 log10(max(., 1e-10)) and stores the unrounded dB rows in scratch with the tile's maximum.
//                      The operand map is the f32 16x16x4 one (lane l: row / column l & 15, k = l >> 4), the RESULT map is
//                      f64's own: column l & 15, row (l >> 4) + 4 * reg.
//   mel_floor_kernel   floor = (maximum over a signal's tiles, or over the call's) - top_db: a fixed tree, no atomics.
//   mfcc_dct_kernel    per tile: clamp at the floor, [16 frames x n_mels] by the transposed DCT table on the same instruction,
//   mel_finish_kernel  or the clamped dB rows themselves; rounded once to f32 at the store.
//   deltas_kernel      d[t] = ((c[t+1] - c[t-1]) + 2 (c[t+2] - c[t-2])) / 10 over the stored f32 values in f64, replicate edges.
// A frame's order of summation depends on (n_fft, n_freqs, n_mels) alone and there is no float atomic: the same call gives the
// same bits, and a signal in a pack gives the bits it gives alone (floor per signal).
#include "common.h"

#include <cmath>

namespace cpc {
namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int MF_THREADS = 256;
constexpr int MF_WAVES = MF_THREADS / 64;
constexpr int MF_FT = 16;                    // frames per tile: the 16 rows of one matrix instruction
constexpr int MF_MIN_FFT = 32, MF_MAX_FFT = 512, MF_MAX_MELS = 512;
constexpr int MF_MAX_FP = (MF_MAX_FFT / 2 + 1 + 15) / 16 * 16;       // 272 padded frequencies
constexpr int MF_CT_PER_WAVE = (MF_MAX_FP / 16 + MF_WAVES - 1) / MF_WAVES;   // 5 tiles of 16 frequencies per wave at most
constexpr int MF_SPAN = (MF_FT - 1) * MF_MAX_FFT + MF_MAX_FFT;       // samples a tile can span (hop <= n_fft <= 512)
constexpr int MF_POW = MF_FT * (MF_MAX_FP + 1);                      // the power tile, rows padded by one double
constexpr int MF_UNION = MF_POW > MF_SPAN / 2 ? MF_POW : MF_SPAN / 2; // doubles: the span (f32) and the power tile share it
constexpr double MF_AMIN = 1e-10;

// the caller's one table buffer: window [Wp] | cos [Hp][Fp] | sin [Hp][Fp] | filterbank [Fp][Mp] | dct^T [n_mels][n_out]
// (rows n <= n_fft / 2 of the twiddles: the kernel folds sample n_fft - n onto n)
struct MfccLayout {
    int Wp, Hp, F, Fp, Mp;
    long win, cs, sn, fb, dct, total;
};

__host__ __device__ inline MfccLayout mfcc_layout(int n_fft, int n_mels, int n_out)
{
    MfccLayout l;
    l.Wp = (n_fft + 3) / 4 * 4;
    l.F = n_fft / 2 + 1;
    l.Hp = (l.F + 3) / 4 * 4;
    l.Fp = (l.F + 15) / 16 * 16;
    l.Mp = (n_mels + 15) / 16 * 16;
    l.win = 0;
    l.cs = l.win + l.Wp;
    l.sn = l.cs + (long)l.Hp * l.Fp;
    l.fb = l.sn + (long)l.Hp * l.Fp;
    l.dct = l.fb + (long)l.Fp * l.Mp;
    l.total = l.dct + (long)n_mels * n_out;
    return l;
}

bool mfcc_domain_ok(int n_fft, int n_mels, int n_out)
{
    return n_fft >= MF_MIN_FFT && n_fft <= MF_MAX_FFT && n_mels >= 1 && n_mels <= MF_MAX_MELS && n_out >= 1 && n_out <= n_mels;
}

// the signal a tile belongs to: the last i with tile_start[i] <= tile (signals without frames own no tile)
__device__ inline int mfcc_signal_of(const long *__restrict__ tile_start, int count, long tile)
{
    int lo = 0, hi = count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tile_start[mid] <= tile) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ void __launch_bounds__(MF_THREADS)
mel_db_kernel(const float *__restrict__ x, long x_total, const long *__restrict__ in_off, const long *__restrict__ in_len,
              const long *__restrict__ n_frames, const long *__restrict__ tile_start, int count, int n_fft, int hop, int offset,
              int n_mels, const double *__restrict__ tables, double *__restrict__ db, double *__restrict__ tile_max)
{
    __shared__ double un[MF_UNION];
    __shared__ double winl[MF_MAX_FFT];
    __shared__ double red[MF_THREADS];
    float *span = reinterpret_cast<float *>(un);
    double *pw = un;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, kq = lane >> 4;
    const MfccLayout lay = mfcc_layout(n_fft, n_mels, 1);
    const int H = lay.F, Hp = lay.Hp, Fp = lay.Fp, Mp = lay.Mp, ldp = lay.Fp + 1;
    const long tile = blockIdx.x;
    const int sig = mfcc_signal_of(tile_start, count, tile);
    const long first = tile_start[sig];
    const bool mine = tile >= first && tile < tile_start[sig + 1];
    const long off = in_off[sig], L = in_len[sig];
    const long T = mine ? n_frames[sig] : 0;
    const long t0 = (tile - first) * MF_FT;
    // a table entry that leaves x, or a signal too short to reflect, is read as silence (the entry point refuses what the host knows)
    const bool readable = mine && L > n_fft / 2 && off >= 0 && off <= x_total - L;

    const long s0 = t0 * hop + offset - n_fft / 2;
    const int span_len = (MF_FT - 1) * hop + n_fft;
    for (int e = tid; e < span_len; e += MF_THREADS) {
        float v = 0.0f;
        if (readable) {
            long i = s0 + e;
            if (i < 0) i = -i;
            if (i >= L) i = 2 * (L - 1) - i;
            i = i < 0 ? 0 : (i >= L ? L - 1 : i);        // frames past the definition's last one: never outside the signal
            v = x[off + i];
        }
        span[e] = v;
    }
    for (int e = tid; e < n_fft; e += MF_THREADS) winl[e] = tables[lay.win + e];
    __syncthreads();

    // ---- windowed DFT: this wave's tiles of 16 frequencies, cos and sin side by side ----
    const int CT = Fp / 16;
    f64x4 re[MF_CT_PER_WAVE], im[MF_CT_PER_WAVE];
#pragma unroll
    for (int j = 0; j < MF_CT_PER_WAVE; ++j) {
        re[j] = (f64x4){0.0, 0.0, 0.0, 0.0};
        im[j] = (f64x4){0.0, 0.0, 0.0, 0.0};
    }
    {
        const float *sp = span + fr * hop;
        const double *cosT = tables + lay.cs + fr, *sinT = tables + lay.sn + fr;
        for (int kk = 0; kk < Hp; kk += 4) {
            const int n = kk + kq, m = n_fft - n;
            double ev = 0.0, od = 0.0;                   // a[n] + a[n_fft - n] for the cos rows, a[n] - a[n_fft - n] for the sin rows
            if (n < H) {
                ev = winl[n] * (double)sp[n];
                if (n > 0 && m > n) {                    // (n = 0 and, for an even n_fft, n = n_fft / 2 have no partner)
                    const double b = winl[m] * (double)sp[m];
                    od = ev - b;
                    ev = ev + b;
                }
            }
            const long row = (long)n * Fp;
#pragma unroll
            for (int j = 0; j < MF_CT_PER_WAVE; ++j) {
                const int ct = wave + MF_WAVES * j;
                if (ct < CT) {
                    re[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ev, cosT[row + ct * 16], re[j], 0, 0, 0);
                    im[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(od, sinT[row + ct * 16], im[j], 0, 0, 0);
                }
            }
        }
    }
    __syncthreads();                                     // every wave is done with the span: the power tile takes its place
#pragma unroll
    for (int j = 0; j < MF_CT_PER_WAVE; ++j) {
        const int ct = wave + MF_WAVES * j;
        if (ct < CT) {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg)            // the f64 result map: row (l >> 4) + 4 reg, column l & 15
                pw[(kq + 4 * reg) * ldp + ct * 16 + fr] = re[j][reg] * re[j][reg] + im[j][reg] * im[j][reg];
        }
    }
    __syncthreads();

    // ---- filterbank, dB, the tile's maximum ----
    double lmax = -INFINITY;
    const double *fb = tables + lay.fb + fr;
    double *dbt = db + (size_t)tile * MF_FT * n_mels;
    for (int mt = wave; mt < Mp / 16; mt += MF_WAVES) {
        f64x4 acc = (f64x4){0.0, 0.0, 0.0, 0.0};
        for (int kk = 0; kk < Fp; kk += 4) {
            const int k = kk + kq;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(pw[fr * ldp + k], fb[(long)k * Mp + mt * 16], acc, 0, 0, 0);
        }
        const int mel = mt * 16 + fr;
        if (mel < n_mels) {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int f = kq + 4 * reg;
                const double d = 10.0 * log10(fmax(acc[reg], MF_AMIN));
                dbt[(size_t)f * n_mels + mel] = d;
                if (t0 + f < T) lmax = fmax(lmax, d);
            }
        }
    }
    red[tid] = lmax;
    __syncthreads();
    for (int s = MF_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = fmax(red[tid], red[tid + s]);
        __syncthreads();
    }
    if (tid == 0) tile_max[tile] = red[0];
}

// per_call == 0: block i reduces signal i's tiles; per_call != 0: one block reduces every tile and writes every signal's floor
__global__ void __launch_bounds__(MF_THREADS)
mel_floor_kernel(const double *__restrict__ tile_max, const long *__restrict__ tile_start, int count, long total_tiles, int per_call,
                 double top_db, double *__restrict__ floor_db)
{
    __shared__ double red[MF_THREADS];
    const int tid = threadIdx.x;
    long a = per_call ? 0 : tile_start[blockIdx.x], b = per_call ? total_tiles : tile_start[blockIdx.x + 1];
    a = a < 0 ? 0 : a;
    b = b > total_tiles ? total_tiles : b;
    double m = -INFINITY;
    for (long t = a + tid; t < b; t += MF_THREADS) m = fmax(m, tile_max[t]);
    red[tid] = m;
    __syncthreads();
    for (int s = MF_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = fmax(red[tid], red[tid + s]);
        __syncthreads();
    }
    const double fl = red[0] - top_db;
    if (per_call) {
        for (int i = tid; i < count; i += MF_THREADS) floor_db[i] = fl;
    } else if (tid == 0) {
        floor_db[blockIdx.x] = fl;
    }
}

// the dB rows themselves: clamp at the floor, one rounding
__global__ void __launch_bounds__(MF_THREADS)
mel_finish_kernel(const double *__restrict__ db, const double *__restrict__ floor_db, const long *__restrict__ n_frames,
                  const long *__restrict__ row_off, const long *__restrict__ tile_start, int count, int n_mels,
                  float *__restrict__ out, long ldo, long out_rows)
{
    const long tile = blockIdx.x;
    const int sig = mfcc_signal_of(tile_start, count, tile);
    const long first = tile_start[sig];
    if (tile < first || tile >= tile_start[sig + 1]) return;
    const long T = n_frames[sig], r0 = row_off[sig], t0 = (tile - first) * MF_FT;
    const bool clamp = floor_db != nullptr;
    const double fl = clamp ? floor_db[sig] : 0.0;
    const double *dbt = db + (size_t)tile * MF_FT * n_mels;
    for (int e = threadIdx.x; e < MF_FT * n_mels; e += MF_THREADS) {
        const int f = e / n_mels, k = e - f * n_mels;
        const long row = r0 + t0 + f;
        if (t0 + f >= T || row < 0 || row >= out_rows) continue;
        const double v = dbt[e];
        out[row * ldo + k] = (float)(clamp ? fmax(v, fl) : v);
    }
}

// the DCT: [16 frames x n_mels] clamped dB rows by [n_mels x n_out] on the matrix instruction, each wave every fourth tile of 16
// coefficients; rows and columns beyond n_mels / n_out enter as zeros and are never read
__global__ void __launch_bounds__(MF_THREADS)
mfcc_dct_kernel(const double *__restrict__ db, const double *__restrict__ floor_db, const long *__restrict__ n_frames,
                const long *__restrict__ row_off, const long *__restrict__ tile_start, int count, int n_mels, int n_out,
                const double *__restrict__ dctT, float *__restrict__ out, long ldo, long out_rows)
{
    const long tile = blockIdx.x;
    const int sig = mfcc_signal_of(tile_start, count, tile);
    const long first = tile_start[sig];
    if (tile < first || tile >= tile_start[sig + 1]) return;
    const long T = n_frames[sig], r0 = row_off[sig], t0 = (tile - first) * MF_FT;
    const bool clamp = floor_db != nullptr;
    const double fl = clamp ? floor_db[sig] : 0.0;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int fr = lane & 15, kq = lane >> 4;
    const double *d = db + (size_t)tile * MF_FT * n_mels + (size_t)fr * n_mels;
    for (int ct = wave; ct * 16 < n_out; ct += MF_WAVES) {
        const int col = ct * 16 + fr;
        f64x4 acc = (f64x4){0.0, 0.0, 0.0, 0.0};
        for (int kk = 0; kk < n_mels; kk += 4) {
            const int m = kk + kq;
            double a = 0.0, b = 0.0;
            if (m < n_mels) {
                a = clamp ? fmax(d[m], fl) : d[m];
                if (col < n_out) b = dctT[(size_t)m * n_out + col];
            }
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
        }
        if (col < n_out) {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int f = kq + 4 * reg;
                const long row = r0 + t0 + f;
                if (t0 + f < T && row >= 0 && row < out_rows) out[row * ldo + col] = (float)acc[reg];
            }
        }
    }
}

// element e of signal blockIdx.y: frame e / cols, column e % cols.  in and out may be column ranges of one buffer.
__global__ void __launch_bounds__(MF_THREADS)
deltas_kernel(const float *in, long ldi, float *out, long ldo, int cols, const long *__restrict__ n_frames,
              const long *__restrict__ row_off, long rows_total)
{
    const int sig = blockIdx.y;
    const long T = n_frames[sig], r0 = row_off[sig];
    if (T < 1 || r0 < 0 || r0 > rows_total - T) return;
    const long e = (long)blockIdx.x * MF_THREADS + threadIdx.x;
    const long t = e / cols;
    const int c = (int)(e - t * cols);
    if (t >= T) return;
    auto at = [&](long u) { return (double)in[(r0 + (u < 0 ? 0 : (u >= T ? T - 1 : u))) * ldi + c]; };
    const double d1 = at(t + 1) - at(t - 1), d2 = at(t + 2) - at(t - 2);
    out[(r0 + t) * ldo + c] = (float)((d1 + 2.0 * d2) / 10.0);
}

size_t melspec_scratch_bytes(long total_tiles, int count, int n_mels)
{
    Carver cv(nullptr);
    cv.take<double>((size_t)total_tiles * MF_FT * n_mels);       // unrounded dB rows
    cv.take<double>((size_t)total_tiles);                        // tile maxima
    cv.take<double>((size_t)count);                              // floors
    return cv.used();
}

bool melspec_counts_ok(long total_tiles, int count)
{
    return count >= 1 && total_tiles >= 1 && total_tiles < (1L << 31);
}

}  // namespace
}  // namespace cpc

extern "C" int cpc_mfcc_frame_tile(void) { return cpc::MF_FT; }

extern "C" long cpc_mfcc_tables_doubles(int n_fft, int n_mels, int n_out)
{
    if (!cpc::mfcc_domain_ok(n_fft, n_mels, n_out)) {
        cpc::set_error("mfcc_tables_doubles: parameters outside the supported limits (n_fft=%d n_mels=%d n_out=%d; need "
                       "32 <= n_fft <= 512, 1 <= n_mels <= 512, 1 <= n_out <= n_mels)", n_fft, n_mels, n_out);
        return 0;
    }
    return cpc::mfcc_layout(n_fft, n_mels, n_out).total;
}

extern "C" int cpc_mfcc_tables_host(int n_fft, int n_mels, int n_out, int sample_rate, double f_min, double f_max,
                                    double *tables_host, long capacity)
{
    CPC_REQUIRE(cpc::mfcc_domain_ok(n_fft, n_mels, n_out), "mfcc_tables_host: parameters outside the supported limits (n_fft=%d "
                "n_mels=%d n_out=%d; need 32 <= n_fft <= 512, 1 <= n_mels <= 512, 1 <= n_out <= n_mels)", n_fft, n_mels, n_out);
    CPC_REQUIRE(sample_rate >= 2, "mfcc_tables_host: sample_rate=%d", sample_rate);
    CPC_REQUIRE(std::isfinite(f_min) && std::isfinite(f_max) && f_min >= 0.0 && f_min < f_max,
                "mfcc_tables_host: need 0 <= f_min < f_max (f_min=%g f_max=%g)", f_min, f_max);
    const cpc::MfccLayout l = cpc::mfcc_layout(n_fft, n_mels, n_out);
    CPC_REQUIRE(tables_host != nullptr && capacity >= l.total, "mfcc_tables_host: room for %ld doubles, %ld needed", capacity,
                l.total);
    double *t = tables_host;
    for (long i = 0; i < l.total; ++i) t[i] = 0.0;
    for (int n = 0; n < n_fft; ++n) t[l.win + n] = 0.5 - 0.5 * cos(2.0 * M_PI * n / n_fft);
    for (int n = 0; n < l.F; ++n)                       // rows n <= n_fft / 2: the kernel folds n_fft - n onto n
        for (int k = 0; k < l.F; ++k) {
            const double arg = 2.0 * M_PI * (double)((n * k) % n_fft) / n_fft;
            t[l.cs + (long)n * l.Fp + k] = cos(arg);
            t[l.sn + (long)n * l.Fp + k] = sin(arg);
        }
    // linspace as numpy writes it: i * step + start, the last point the stop itself
    auto linspace = [](double start, double stop, int num, double *out) {
        const double step = (stop - start) / (num - 1);
        for (int i = 0; i < num; ++i) out[i] = i * step + start;
        out[num - 1] = stop;
    };
    double freqs[cpc::MF_MAX_FFT / 2 + 1], pts[cpc::MF_MAX_MELS + 2];
    linspace(0.0, (double)(sample_rate / 2), l.F, freqs);
    linspace(2595.0 * log10(1.0 + f_min / 700.0), 2595.0 * log10(1.0 + f_max / 700.0), n_mels + 2, pts);
    volatile double ten = 10.0;          // pow itself, not the exp10 a compiler may put in its place: another last bit
    for (int j = 0; j < n_mels + 2; ++j) pts[j] = 700.0 * (pow(ten, pts[j] / 2595.0) - 1.0);
    for (int k = 0; k < l.F; ++k)
        for (int m = 0; m < n_mels; ++m) {
            const double down = -(pts[m] - freqs[k]) / (pts[m + 1] - pts[m]);
            const double up = (pts[m + 2] - freqs[k]) / (pts[m + 2] - pts[m + 1]);
            t[l.fb + (long)k * l.Mp + m] = fmax(0.0, fmin(down, up));
        }
    const double scale = sqrt(2.0 / n_mels);
    for (int k = 0; k < n_out; ++k)
        for (int m = 0; m < n_mels; ++m) {
            double v = cos(M_PI / n_mels * (m + 0.5) * k) * scale;
            if (k == 0) v *= 1.0 / sqrt(2.0);
            t[l.dct + (long)m * n_out + k] = v;
        }
    return CPC_OK;
}

extern "C" size_t cpc_melspec_scratch_bytes(long total_tiles, int count, int n_mels)
{
    if (!cpc::melspec_counts_ok(total_tiles, count) || n_mels < 1 || n_mels > cpc::MF_MAX_MELS) {
        cpc::set_error("melspec_scratch_bytes: sizes outside the supported limits (total_tiles=%ld count=%d n_mels=%d)", total_tiles,
                       count, n_mels);
        return 0;
    }
    return cpc::melspec_scratch_bytes(total_tiles, count, n_mels);
}

extern "C" int cpc_melspec_db(const float *x, long x_total, const long *in_off, const long *in_len, const long *n_frames,
                              const long *tile_start, int count, long total_tiles, long min_len, int n_fft, int hop, int offset,
                              int n_mels, const double *tables, int floor_mode, double top_db, void *scratch, size_t scratch_bytes,
                              cpc_stream_t stream)
{
    CPC_REQUIRE(n_fft >= cpc::MF_MIN_FFT && n_fft <= cpc::MF_MAX_FFT, "melspec_db: n_fft=%d outside 32..512", n_fft);
    CPC_REQUIRE(hop >= 1 && hop <= n_fft, "melspec_db: hop=%d outside 1..n_fft (n_fft=%d)", hop, n_fft);
    CPC_REQUIRE(offset >= 0 && offset <= hop, "melspec_db: offset=%d outside 0..hop (hop=%d)", offset, hop);
    CPC_REQUIRE(n_mels >= 1 && n_mels <= cpc::MF_MAX_MELS, "melspec_db: n_mels=%d outside 1..512", n_mels);
    CPC_REQUIRE(count >= 1, "melspec_db: count=%d, need at least one signal", count);
    CPC_REQUIRE(cpc::melspec_counts_ok(total_tiles, count), "melspec_db: total_tiles=%ld outside 1..2^31-1", total_tiles);
    CPC_REQUIRE(min_len > n_fft / 2, "melspec_db: a signal of %ld samples is too short: reflection needs more than n_fft // 2 = %d",
                min_len, n_fft / 2);
    CPC_REQUIRE(floor_mode >= 0 && floor_mode <= 2, "melspec_db: floor_mode=%d (0 none, 1 per signal, 2 per call)", floor_mode);
    CPC_REQUIRE(floor_mode == 0 || (std::isfinite(top_db) && top_db >= 0.0), "melspec_db: top_db=%g, need a finite value >= 0", top_db);
    CPC_REQUIRE(x != nullptr && x_total >= 1 && in_off != nullptr && in_len != nullptr && n_frames != nullptr &&
                tile_start != nullptr && tables != nullptr, "melspec_db: null buffer");
    const size_t need = cpc::melspec_scratch_bytes(total_tiles, count, n_mels);
    CPC_REQUIRE(scratch != nullptr && scratch_bytes >= need, "melspec_db: scratch of %zu bytes, %zu needed", scratch_bytes, need);
    hipStream_t s = static_cast<hipStream_t>(stream);
    cpc::Carver cv(scratch);
    double *db = cv.take<double>((size_t)total_tiles * cpc::MF_FT * n_mels);
    double *tile_max = cv.take<double>((size_t)total_tiles);
    double *floor_db = cv.take<double>((size_t)count);
    hipLaunchKernelGGL(cpc::mel_db_kernel, dim3((unsigned)total_tiles), dim3(cpc::MF_THREADS), 0, s, x, x_total, in_off, in_len,
                       n_frames, tile_start, count, n_fft, hop, offset, n_mels, tables, db, tile_max);
    CPC_CHECK_LAUNCH("mel_db_kernel");
    if (floor_mode != 0) {
        hipLaunchKernelGGL(cpc::mel_floor_kernel, dim3(floor_mode == 2 ? 1u : (unsigned)count), dim3(cpc::MF_THREADS), 0, s,
                           tile_max, tile_start, count, total_tiles, floor_mode == 2 ? 1 : 0, top_db, floor_db);
        CPC_CHECK_LAUNCH("mel_floor_kernel");
    }
    return CPC_OK;
}

extern "C" int cpc_mfcc_finish(const void *scratch, size_t scratch_bytes, const long *n_frames, const long *row_off,
                               const long *tile_start, int count, long total_tiles, int n_fft, int n_mels, int n_out, int want_dct,
                               const double *tables, int floor_mode, float *out, long ldo, long out_rows, cpc_stream_t stream)
{
    CPC_REQUIRE(n_fft >= cpc::MF_MIN_FFT && n_fft <= cpc::MF_MAX_FFT, "mfcc_finish: n_fft=%d outside 32..512", n_fft);
    CPC_REQUIRE(n_mels >= 1 && n_mels <= cpc::MF_MAX_MELS, "mfcc_finish: n_mels=%d outside 1..512", n_mels);
    CPC_REQUIRE(n_out >= 1 && n_out <= n_mels, "mfcc_finish: n_out=%d outside 1..n_mels (n_mels=%d)", n_out, n_mels);
    CPC_REQUIRE(want_dct != 0 || n_out == n_mels, "mfcc_finish: the dB rows have n_mels=%d columns, not n_out=%d", n_mels, n_out);
    CPC_REQUIRE(count >= 1, "mfcc_finish: count=%d, need at least one signal", count);
    CPC_REQUIRE(cpc::melspec_counts_ok(total_tiles, count), "mfcc_finish: total_tiles=%ld outside 1..2^31-1", total_tiles);
    CPC_REQUIRE(floor_mode >= 0 && floor_mode <= 2, "mfcc_finish: floor_mode=%d (0 none, 1 per signal, 2 per call)", floor_mode);
    CPC_REQUIRE(ldo >= n_out && out_rows >= 1, "mfcc_finish: row stride below the width, or no rows (ldo=%ld n_out=%d out_rows=%ld)",
                ldo, n_out, out_rows);
    CPC_REQUIRE(n_frames != nullptr && row_off != nullptr && tile_start != nullptr && out != nullptr &&
                (want_dct == 0 || tables != nullptr), "mfcc_finish: null buffer");
    const size_t need = cpc::melspec_scratch_bytes(total_tiles, count, n_mels);
    CPC_REQUIRE(scratch != nullptr && scratch_bytes >= need, "mfcc_finish: scratch of %zu bytes, %zu needed", scratch_bytes, need);
    hipStream_t s = static_cast<hipStream_t>(stream);
    cpc::Carver cv(const_cast<void *>(scratch));
    const double *db = cv.take<double>((size_t)total_tiles * cpc::MF_FT * n_mels);
    cv.take<double>((size_t)total_tiles);
    const double *floor_db = cv.take<double>((size_t)count);
    const double *dctT = want_dct != 0 ? tables + cpc::mfcc_layout(n_fft, n_mels, n_out).dct : nullptr;
    const double *fl = floor_mode != 0 ? floor_db : nullptr;
    if (dctT != nullptr) {
        hipLaunchKernelGGL(cpc::mfcc_dct_kernel, dim3((unsigned)total_tiles), dim3(cpc::MF_THREADS), 0, s, db, fl, n_frames,
                           row_off, tile_start, count, n_mels, n_out, dctT, out, ldo, out_rows);
        CPC_CHECK_LAUNCH("mfcc_dct_kernel");
    } else {
        hipLaunchKernelGGL(cpc::mel_finish_kernel, dim3((unsigned)total_tiles), dim3(cpc::MF_THREADS), 0, s, db, fl, n_frames,
                           row_off, tile_start, count, n_mels, out, ldo, out_rows);
        CPC_CHECK_LAUNCH("mel_finish_kernel");
    }
    return CPC_OK;
}

extern "C" int cpc_deltas(const float *in, long ldi, float *out, long ldo, int cols, const long *n_frames, const long *row_off,
                          int count, long max_frames, long rows_total, cpc_stream_t stream)
{
    CPC_REQUIRE(cols >= 1 && cols <= 3 * cpc::MF_MAX_MELS, "deltas: cols=%d outside 1..1536", cols);
    CPC_REQUIRE(count >= 1 && count <= 65535, "deltas: count=%d outside 1..65535", count);
    CPC_REQUIRE(max_frames >= 1 && max_frames < (1L << 31) / cols, "deltas: max_frames=%ld outside 1..2^31 / cols", max_frames);
    CPC_REQUIRE(ldi >= cols && ldo >= cols && rows_total >= 1, "deltas: row stride below the width, or no rows (ldi=%ld ldo=%ld "
                "cols=%d rows_total=%ld)", ldi, ldo, cols, rows_total);
    CPC_REQUIRE(in != nullptr && out != nullptr && n_frames != nullptr && row_off != nullptr, "deltas: null buffer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(cpc::deltas_kernel, dim3((unsigned)cpc::cdiv(max_frames * cols, cpc::MF_THREADS), (unsigned)count),
                       dim3(cpc::MF_THREADS), 0, s, in, ldi, out, ldo, cols, n_frames, row_off, rows_total);
    CPC_CHECK_LAUNCH("deltas_kernel");
    return CPC_OK;
}
