// CPCAR (mode="GRU") on gfx950.  Reference: /root/reference/cpc/model.py:158-207 -> torch.nn.GRU
// (batch_first, gate order r,z,n):
//     r = sigmoid(W_ir x + b_ir + W_hr h + b_hr)        z = sigmoid(W_iz x + b_iz + W_hz h + b_hz)
//     n = tanh(W_in x + b_in + r * (W_hn h + b_hn))      h' = (1 - z) * n + z * h
//
// Forward per layer: one MFMA GEMM for all input projections GI = X W_ih^T + b_ih, then ONE
// persistent kernel for the T sequential steps.  Windows are independent, so each workgroup owns
// one window for the whole sequence (no inter-workgroup synchronisation); thread (j, q) owns hidden
// unit j and K slice q, h lives in LDS and W_hh (re-laid out so that lanes read consecutive float4s)
// is streamed from L2 every step.  Backward mirrors it (BPTT), then three GEMMs give dW_hh, dW_ih and dX.
#include "common.h"
#include "coop.h"
#include "recurrent.h"

#include <algorithm>
#include <cstdlib>

namespace cpc {

// W_hh [3H][H] -> wf[(k4*3 + g)*H + j] = W[g*H + j][4*k4 .. 4*k4+3]   (forward: thread j, all k)
__global__ void gru_pack_fwd_kernel(const float *w, float4 *wf, int H)
{
    const int total = 3 * H * (H / 4);
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const int j = idx % H;
        const int g = (idx / H) % 3;
        const int k4 = idx / (3 * H);
        const float *src = w + (long)(g * H + j) * H + 4 * k4;
        wf[idx] = make_float4(src[0], src[1], src[2], src[3]);
    }
}

// W_hh [3H][H] -> wb[g4*H + j] = (W[4*g4][j], W[4*g4+1][j], W[4*g4+2][j], W[4*g4+3][j])   (backward)
__global__ void gru_pack_bwd_kernel(const float *w, float4 *wb, int H)
{
    const int total = (3 * H / 4) * H;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const int j = idx % H;
        const int g4 = idx / H;
        wb[idx] = make_float4(w[(long)(4 * g4) * H + j], w[(long)(4 * g4 + 1) * H + j], w[(long)(4 * g4 + 2) * H + j],
                              w[(long)(4 * g4 + 3) * H + j]);
    }
}

struct GruArgs {
    const float *gi;      // [N*T][3H]   input projections incl. b_ih
    const float4 *wpack;  // packed W_hh
    const float *whh;     // W_hh [3H][H] as stored (cooperative kernel)
    const float *bhh;     // [3H]
    const float *h0;      // [N][H] or null
    float *out;           // [N][T][H]
    float *hall;          // [N][T+1][H]  row 0 = h0, row t+1 = h_t
    float *gates;         // [N*T][3H]    r, z, n
    float *hn;            // [N*T][H]     W_hn h + b_hn
    float *hlast;         // [N][H] or null
    int N, T, H;
    int hp, kq;           // threads = kq * hp: hp = H rounded up to 64, kq = K-split factor
    // backward
    const float *dout;    // [N][T][H]
    float *dgi;           // [N*T][3H]
    float *dgh;           // [N][T+1][3H], row T zero
};

// ---- the cell, once: every forward kernel finishes a (window, unit) pair with gru_gates, every backward kernel starts one
// with gru_grad; the kernels differ in how they form the products with W_hh
struct GruGates { float r, z, c, hv; };
// gi: the input projections (b_ih included), g: W_h. h + b_h. of the three gates
__device__ __forceinline__ GruGates gru_gates(float gi0, float gi1, float gi2, float g0, float g1, float g2, float hprev)
{
    GruGates v;
    v.r = coop_sigmoid(gi0 + g0);
    v.z = coop_sigmoid(gi1 + g1);
    v.c = tanhf(gi2 + v.r * g2);
    v.hv = (1.f - v.z) * v.c + v.z * hprev;
    return v;
}
struct GruGrad { float dpr, dpz, dpn, dhn, keep; };      // d pre-activations (dhn: of W_hn h + b_hn), keep = dh z
__device__ __forceinline__ GruGrad gru_grad(float dh, float r, float z, float c, float hnv, float hp_)
{
    GruGrad d;
    const float dc = dh * (1.f - z);
    const float dz = dh * (hp_ - c);
    d.dpn = dc * (1.f - c * c);
    d.dpr = d.dpn * hnv * r * (1.f - r);
    d.dpz = dz * z * (1.f - z);
    d.dhn = d.dpn * r;
    d.keep = dh * z;
    return d;
}

// One workgroup per window; thread (j, q): hidden unit j, K slice q.  The K split puts kq x more waves
// (and W_hh loads) in flight per CU: the step time is the L2 -> CU stream of W_hh (3H*H*4 bytes).
__global__ void gru_fwd_kernel(GruArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];   // hs[H] | red[kq][3][hp]
    const int H = a.H, T = a.T, hp = a.hp, kq = a.kq;
    float *hs = smem;
    float *red = smem + ((H + 3) / 4) * 4;
    const int j = threadIdx.x % hp, q = threadIdx.x / hp;
    const bool act = j < H;
    const int n = blockIdx.x;
    const int k4_per = (H / 4 + kq - 1) / kq;
    const int k4_lo = q * k4_per, k4_hi = min(H / 4, k4_lo + k4_per);

    float hprev = 0.f;
    float bh[3] = {0.f, 0.f, 0.f};
    if (act && q == 0) {
        hprev = a.h0 != nullptr ? a.h0[(long)n * H + j] : 0.f;
        hs[j] = hprev;
        a.hall[((long)n * (T + 1)) * H + j] = hprev;
        bh[0] = a.bhh[j]; bh[1] = a.bhh[H + j]; bh[2] = a.bhh[2 * H + j];
    }
    __syncthreads();

    for (int t = 0; t < T; ++t) {
        float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f;
        if (act) {
            const float4 *wp = a.wpack + j;
#pragma unroll 4
            for (int k4 = k4_lo; k4 < k4_hi; ++k4) {
                const float4 wr = wp[(long)(k4 * 3 + 0) * H];
                const float4 wz = wp[(long)(k4 * 3 + 1) * H];
                const float4 wn = wp[(long)(k4 * 3 + 2) * H];
                const float4 h4 = reinterpret_cast<const float4 *>(hs)[k4];
                acc0 = fmaf(wr.x, h4.x, fmaf(wr.y, h4.y, fmaf(wr.z, h4.z, fmaf(wr.w, h4.w, acc0))));
                acc1 = fmaf(wz.x, h4.x, fmaf(wz.y, h4.y, fmaf(wz.z, h4.z, fmaf(wz.w, h4.w, acc1))));
                acc2 = fmaf(wn.x, h4.x, fmaf(wn.y, h4.y, fmaf(wn.z, h4.z, fmaf(wn.w, h4.w, acc2))));
            }
            red[(q * 3 + 0) * hp + j] = acc0;
            red[(q * 3 + 1) * hp + j] = acc1;
            red[(q * 3 + 2) * hp + j] = acc2;
        }
        __syncthreads();                       // partial sums visible; nobody reads hs any more
        if (act && q == 0) {
            float g0 = bh[0], g1 = bh[1], g2 = bh[2];
            for (int qq = 0; qq < kq; ++qq) {
                g0 += red[(qq * 3 + 0) * hp + j];
                g1 += red[(qq * 3 + 1) * hp + j];
                g2 += red[(qq * 3 + 2) * hp + j];
            }
            const long row = (long)n * T + t;
            const float *g = a.gi + row * 3 * H;
            const GruGates v = gru_gates(g[j], g[H + j], g[2 * H + j], g0, g1, g2, hprev);
            float *gs = a.gates + row * 3 * H;
            gs[j] = v.r; gs[H + j] = v.z; gs[2 * H + j] = v.c;
            a.hn[row * H + j] = g2;
            a.out[row * H + j] = v.hv;
            a.hall[((long)n * (T + 1) + t + 1) * H + j] = v.hv;
            hs[j] = v.hv;
            hprev = v.hv;
        }
        __syncthreads();
    }
    if (act && q == 0 && a.hlast != nullptr) a.hlast[(long)n * H + j] = hprev;
}

__global__ void gru_bwd_kernel(GruArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];   // dgh[3H] | red[kq][hp]
    const int H = a.H, T = a.T, hp = a.hp, kq = a.kq;
    float *dg = smem;
    float *red = smem + 3 * H;
    const int j = threadIdx.x % hp, q = threadIdx.x / hp;
    const bool act = j < H;
    const int n = blockIdx.x;
    const int g4_total = 3 * H / 4;
    const int g4_per = (g4_total + kq - 1) / kq;
    const int g4_lo = q * g4_per, g4_hi = min(g4_total, g4_lo + g4_per);

    float carry = 0.f;
    if (act && q == 0) {                                         // zero junk row T of dGH
        float *zr = a.dgh + ((long)n * (T + 1) + T) * 3 * H;
        zr[j] = 0.f; zr[H + j] = 0.f; zr[2 * H + j] = 0.f;
    }
    for (int t = T - 1; t >= 0; --t) {
        float keep = 0.f;
        if (act && q == 0) {
            const long row = (long)n * T + t;
            const float dh = a.dout[row * H + j] + carry;
            const float *gs = a.gates + row * 3 * H;
            const float r = gs[j], z = gs[H + j], c = gs[2 * H + j];
            const GruGrad d = gru_grad(dh, r, z, c, a.hn[row * H + j], a.hall[((long)n * (T + 1) + t) * H + j]);
            keep = d.keep;
            float *gi = a.dgi + row * 3 * H;
            gi[j] = d.dpr; gi[H + j] = d.dpz; gi[2 * H + j] = d.dpn;
            float *gh = a.dgh + ((long)n * (T + 1) + t) * 3 * H;
            gh[j] = d.dpr; gh[H + j] = d.dpz; gh[2 * H + j] = d.dhn;
            dg[j] = d.dpr; dg[H + j] = d.dpz; dg[2 * H + j] = d.dhn;
        }
        __syncthreads();
        if (act) {
            float acc = 0.f;
            const float4 *wp = a.wpack + j;
#pragma unroll 4
            for (int g4 = g4_lo; g4 < g4_hi; ++g4) {
                const float4 w4 = wp[(long)g4 * H];
                const float4 d4 = reinterpret_cast<const float4 *>(dg)[g4];
                acc = fmaf(w4.x, d4.x, fmaf(w4.y, d4.y, fmaf(w4.z, d4.z, fmaf(w4.w, d4.w, acc))));
            }
            red[q * hp + j] = acc;
        }
        __syncthreads();
        if (act && q == 0) {
            float sum = keep;
            for (int qq = 0; qq < kq; ++qq) sum += red[qq * hp + j];
            carry = sum;
        }
        // the next iteration's writes to dg happen after every thread passed the barrier above; its reads of
        // red happen after the next two barriers -> no extra barrier needed here
    }
}

// ------------------------------------------------------------------------------------------------
// On-chip recurrence for H = 256 and 512: W_hh never leaves the register file.  A GROUP of G workgroups (512
// threads each, one per CU) shares NB windows; every thread holds 96 weights: thread (u, q) = unit u of the member's
// U units, K slice q of 32 columns, 3 gates.  H = 256: 8 slices, U = 64, G = 4;  H = 512: 16 slices, U = 32, G = 16.
// Per step every member multiplies its slice by the full h (LDS), finishes the K reduction with wave shuffles,
// applies the gates for its U units and publishes them; the members exchange the new h through the granules of
// coop.h ("the hand-off": coop_fwd_publish / coop_fwd_gather, backward coop_bwd_publish / coop_bwd_collect).
using GruCoopArgs = CoopArgs<GruArgs>;

template <int H, int NB> __global__ __launch_bounds__(512) void gru_fwd_coop_kernel(GruCoopArgs ca)
{
    using C = CoopCfg<H>;
    constexpr int QS = C::QS, U = C::U, G = C::G;
    static_assert(NB <= QS, "one finishing lane per window");
    __shared__ __attribute__((aligned(16))) float hs[2][NB][C::LDH];
    const GruArgs &a = ca.g;
    const int T = a.T;
    int group, member;
    coop_who<G>(ca.groups, ca.xcd_map, group, member);
    const int tid = threadIdx.x;
    const int q = tid & (QS - 1), u = tid / QS;
    const int j = member * U + u;
    const int n0 = group * NB;

    f32x2 w[3][16];
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int i4 = 0; i4 < 8; ++i4) {
            const float4 v = *reinterpret_cast<const float4 *>(a.whh + (long)(g * H + j) * H + q * 32 + 4 * i4);
            w[g][2 * i4] = pk_lo(v); w[g][2 * i4 + 1] = pk_hi(v);
        }
    const float bh0 = a.bhh[j], bh1 = a.bhh[H + j], bh2 = a.bhh[2 * H + j];

    for (int idx = tid; idx < NB * H; idx += 512) {
        const int s = idx / H, k = idx - s * H;
        const int n = n0 + s;
        const float v = (n < a.N && a.h0 != nullptr) ? a.h0[(long)n * H + k] : 0.f;
        hs[0][s][coop_pad(k)] = v;
        if (n < a.N && (k / U) == member) a.hall[((long)n * (T + 1)) * H + k] = v;
    }
    __syncthreads();

    const int ns = n0 + q;
    const bool mine = q < NB && ns < a.N;
    float gin0 = 0.f, gin1 = 0.f, gin2 = 0.f;
    if (mine) {
        const float *gp = a.gi + (long)ns * T * 3 * H;
        gin0 = gp[j]; gin1 = gp[H + j]; gin2 = gp[2 * H + j];
    }
    bool dead = false;
    for (int t = 0; t < T; ++t) {
        const int cur = t & 1, nxt = cur ^ 1;
        // this lane finishes sample q (if q < NB); its input projections were requested one step ago, the next
        // step's are requested now: a load consumed in the step that issues it puts an L2/HBM round trip on the
        // serial path of every time step
        const float gi0 = gin0, gi1 = gin1, gi2 = gin2;
        if (mine && t + 1 < T) {
            const float *gp = a.gi + ((long)ns * T + t + 1) * 3 * H;
            gin0 = gp[j]; gin1 = gp[H + j]; gin2 = gp[2 * H + j];
        }
        float acc[NB][3];
#pragma unroll
        for (int s = 0; s < NB; ++s) {
            f32x2 a2[3] = {f32x2{0.f, 0.f}, f32x2{0.f, 0.f}, f32x2{0.f, 0.f}};    // even / odd columns of the slice
#pragma unroll
            for (int i4 = 0; i4 < 8; ++i4) {
                const float4 h4 = *reinterpret_cast<const float4 *>(&hs[cur][s][q * 36 + 4 * i4]);
#pragma unroll
                for (int g = 0; g < 3; ++g)
                    a2[g] = pk_fma(w[g][2 * i4 + 1], pk_hi(h4), pk_fma(w[g][2 * i4], pk_lo(h4), a2[g]));
            }
#pragma unroll
            for (int g = 0; g < 3; ++g) acc[s][g] = coop_group_sum<QS>(a2[g].x + a2[g].y);
        }
        if (q < NB) {
            float g0 = 0.f, g1 = 0.f, g2 = 0.f;
#pragma unroll
            for (int s = 0; s < NB; ++s)
                if (s == q) { g0 = acc[s][0]; g1 = acc[s][1]; g2 = acc[s][2]; }
            g0 += bh0; g1 += bh1; g2 += bh2;
            const GruGates v = gru_gates(gi0, gi1, gi2, g0, g1, g2, hs[cur][q][coop_pad(j)]);
            const float hv = dead ? NAN : v.hv;
            // publish first: the other members wait for this store, nobody waits for the saved activations below
            coop_fwd_publish<H, NB>(ca.comm, ca.epoch0 + (unsigned)(t + 1), ca.fault, group, nxt, member, u, q, t, mine,
                                    hv);
            if (mine) {
                const long row = (long)ns * T + t;
                float *gs = a.gates + row * 3 * H;
                gs[j] = v.r; gs[H + j] = v.z; gs[2 * H + j] = v.c;
                a.hn[row * H + j] = g2;
                a.out[row * H + j] = hv;
                a.hall[((long)ns * (T + 1) + t + 1) * H + j] = hv;
            }
        }
        if (t + 1 < T) {
            dead = coop_fwd_gather<H, NB>(ca.comm, ca.epoch0 + (unsigned)(t + 1), ca.err, group, nxt, dead,
                                          [&](int window, int k, float h) { hs[nxt][window][coop_pad(k)] = h; });
            coop_lds_barrier();
        }
    }
    if (a.hlast != nullptr && q < NB && n0 + q < a.N)
        a.hlast[(long)(n0 + q) * H + j] = a.hall[((long)(n0 + q) * (T + 1) + T) * H + j];
}

// ------------------------------------------------------------------------------------------------
// The same recurrence with the step's product on the bf16 matrix pipe (many windows per group: H = 512, NB = 8, where the
// VALU form spends 2.4 of a 5.8 us step on 768 FMAs per thread).  Per member and step out[16][3U] = A[16][H] B[H][3U]:
//   B = the member's 3U rows of W_hh (column c = gate * U + unit) as the three bf16 terms of every weight, held in registers
//       as v_mfma_f32_16x16x32_bf16 operands: the 3U / 16 column tiles x 4 (or 2) K parts make 24 units of 4 K steps, three
//       per wave -- three tiles of ONE K part -- (144 VGPRs);
//   A = the three bf16 terms of h (LDS, [plane][window][H + 8]), with windows 0-7 of term 0 in rows 0-7 and of term 1 -- or 2 --
//       in rows 8-15, so that FOUR products per K step give the six of the exact split (gemm_f32.hip):
//       [h0|h1] w0 -> h0w0, h1w0;  [h0|h1] w1 -> h0w1, h1w1;  [h0|h2] w2 -> h0w2 (+ h2w2: 2^-32, harmless);  [h2|0] w0 -> h2w0.
// The units' 16 x 16 partial tiles go through LDS ([unit][column][row]); the lane that finishes (window q, unit u) adds the
// K parts and the two row halves in a fixed order.  Everything else -- granules, polling, saved activations -- is the
// cooperative kernel's.
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
struct MfmaFrag { unsigned d[4]; };                     // 8 bf16: one operand of v_mfma_f32_16x16x32_bf16

__device__ __forceinline__ unsigned short bf16_rne(float v) { return __builtin_bit_cast(unsigned short, (__bf16)v); }
// v = t0 + t1 + t2 (bf16 each, round to nearest): exact to 2^-27 |v| (gemm_f32.hip)
__device__ __forceinline__ void split3(float v, unsigned short (&t)[3])
{
    t[0] = bf16_rne(v);
    v -= __uint_as_float((unsigned)t[0] << 16);
    t[1] = bf16_rne(v);
    v -= __uint_as_float((unsigned)t[1] << 16);
    t[2] = bf16_rne(v);
}
// eight f32 weights, consecutive in K -> the B operand of each of their three bf16 terms
__device__ __forceinline__ void mfma_pack(const float (&v)[8], MfmaFrag (&w)[3])
{
    unsigned short t[8][3];
#pragma unroll
    for (int e = 0; e < 8; ++e) split3(v[e], t[e]);
#pragma unroll
    for (int pl = 0; pl < 3; ++pl)
#pragma unroll
        for (int d = 0; d < 4; ++d) w[pl].d[d] = (unsigned)t[2 * d][pl] | ((unsigned)t[2 * d + 1][pl] << 16);
}
// the four products of one K step (the note above) into one accumulator: a1 = [x0 | x1], a2 = [x0 | x2], a3 = [x2 | 0]
__device__ __forceinline__ f32x4_t mfma_kstep(bf16x8_t a1, bf16x8_t a2, bf16x8_t a3, const MfmaFrag (&w)[3], f32x4_t acc)
{
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, __builtin_bit_cast(bf16x8_t, w[0]), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, __builtin_bit_cast(bf16x8_t, w[1]), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2, __builtin_bit_cast(bf16x8_t, w[2]), acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a3, __builtin_bit_cast(bf16x8_t, w[0]), acc, 0, 0, 0);
}

template <int H> struct MfmaCfg {
    using C = CoopCfg<H>;
    static constexpr int N3 = 3 * C::U;                  // columns of the member: gate * U + unit
    static constexpr int TILES = N3 / 16;                // 6 (H = 512), 12 (H = 256)
    static constexpr int KS = 24 / TILES;                // K parts per tile: 24 units for 8 waves
    static constexpr int KPU = (H / 32) / KS;            // K steps of 32 per unit
    static constexpr int LDK = H + 8;                    // bf16 per (plane, window) row: rows 4 banks apart
    static_assert(N3 % 16 == 0 && 24 % TILES == 0 && (H / 32) % KS == 0 && KPU == 4, "24 units of 4 K steps");
};

template <int H, int NB> __global__ __launch_bounds__(512) void gru_fwd_mfma_kernel(GruCoopArgs ca)
{
    using C = CoopCfg<H>;
    using M = MfmaCfg<H>;
    constexpr int QS = C::QS, U = C::U, G = C::G;
    constexpr int LDK = M::LDK;
    static_assert(NB <= 8 && NB <= QS, "eight windows fill half the rows of a 16-row tile");
    __shared__ __attribute__((aligned(16))) unsigned short hp[2][3][8][LDK];     // the three terms of h, two steps
    __shared__ __attribute__((aligned(16))) unsigned short zrow[LDK];            // rows 8-15 of the fourth product
    __shared__ __attribute__((aligned(16))) float part[24][16][16];              // [unit][column][row]
    const GruArgs &a = ca.g;
    const int T = a.T;
    int group, member;
    coop_who<G>(ca.groups, ca.xcd_map, group, member);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int q = tid & (QS - 1), u = tid / QS;
    const int j = member * U + u;
    const int n0 = group * NB;

    // ---- this wave's three units: B operands (all three terms) of 4 K steps each
    MfmaFrag bw[3][4][3];
    // (the three units of a wave share their K part: its A fragments are read once per K step, not once per unit -- the
    //  step's arithmetic is bound by LDS reads, 295 KB per member and step otherwise)
    const int kpart = wave % M::KS, tile0 = 3 * (wave / M::KS);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int tile = tile0 + i;
        const int col = tile * 16 + (lane & 15);
        const long row = (long)((col / U) * H + member * U + (col % U)) * H;          // row of W_hh
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int k = (kpart * 4 + ks) * 32 + 8 * (lane >> 4);
            const float4 v0 = *reinterpret_cast<const float4 *>(a.whh + row + k);
            const float4 v1 = *reinterpret_cast<const float4 *>(a.whh + row + k + 4);
            const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
            mfma_pack(v, bw[i][ks]);
        }
    }
    const float bh0 = a.bhh[j], bh1 = a.bhh[H + j], bh2 = a.bhh[2 * H + j];

    // ---- h0 -> planes of step 0 (windows >= NB: zeros), the zero row
    for (int idx = tid; idx < 8 * H; idx += 512) {
        const int s = idx / H, k = idx - s * H;
        const int n = n0 + s;
        const float v = (s < NB && n < a.N && a.h0 != nullptr) ? a.h0[(long)n * H + k] : 0.f;
        unsigned short t[3];
        split3(v, t);
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) { hp[0][pl][s][k] = t[pl]; hp[1][pl][s][k] = 0; }
        if (s < NB && n < a.N && (k / U) == member) a.hall[((long)n * (T + 1)) * H + k] = v;
    }
    for (int k = tid; k < LDK; k += 512) zrow[k] = 0;
    __syncthreads();

    const int ns = n0 + q;
    const bool mine = q < NB && ns < a.N;
    float hprev = (mine && a.h0 != nullptr) ? a.h0[(long)ns * H + j] : 0.f;
    float gin0 = 0.f, gin1 = 0.f, gin2 = 0.f;
    if (mine) {
        const float *gp = a.gi + (long)ns * T * 3 * H;
        gin0 = gp[j]; gin1 = gp[H + j]; gin2 = gp[2 * H + j];
    }
    // A operand addresses (bytes inside one step's planes): lane -> row lane % 16, K group lane / 16
    const int arow = lane & 15, akg = lane >> 4;
    const unsigned aoff0 = (unsigned)(((0 * 8 + (arow & 7)) * LDK + 8 * akg) * 2);
    const unsigned aoff1 = (unsigned)(((1 * 8 + (arow & 7)) * LDK + 8 * akg) * 2);
    const unsigned aoff2 = (unsigned)(((2 * 8 + (arow & 7)) * LDK + 8 * akg) * 2);
    const bool upper = arow >= 8;
    // where this lane's finished sums are: column c = gate * U + u -> tile c / 16, column c % 16 of the tile
    int ptile[3], pcol[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) { ptile[g] = (g * U + u) / 16; pcol[g] = (g * U + u) % 16; }
    bool dead = false;
    for (int t = 0; t < T; ++t) {
        const int cur = t & 1, nxt = cur ^ 1;
        const float gi0 = gin0, gi1 = gin1, gi2 = gin2;
        if (mine && t + 1 < T) {
            const float *gp = a.gi + ((long)ns * T + t + 1) * 3 * H;
            gin0 = gp[j]; gin1 = gp[H + j]; gin2 = gp[2 * H + j];
        }
        const char *planes = reinterpret_cast<const char *>(&hp[cur][0][0][0]);
        const char *pa1 = planes + (upper ? aoff1 : aoff0);                  // [h0 | h1]
        const char *pa2 = planes + (upper ? aoff2 : aoff0);                  // [h0 | h2]
        const char *pa3 = upper ? reinterpret_cast<const char *>(zrow) + 16 * akg : planes + aoff2;   // [h2 | 0]
        f32x4_t acc[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) acc[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int kb = (kpart * 4 + ks) * 64;                                       // bytes: 32 bf16 per K step
            const bf16x8_t a1 = *reinterpret_cast<const bf16x8_t *>(pa1 + kb);
            const bf16x8_t a2 = *reinterpret_cast<const bf16x8_t *>(pa2 + kb);
            const bf16x8_t a3 = *reinterpret_cast<const bf16x8_t *>(pa3 + (upper ? 0 : kb));
#pragma unroll
            for (int i = 0; i < 3; ++i) acc[i] = mfma_kstep(a1, a2, a3, bw[i][ks], acc[i]);    // three independent accumulator chains
        }
        // lane: column lane % 16, rows 4 (lane / 16) .. + 3 of unit (tile, kpart)
#pragma unroll
        for (int i = 0; i < 3; ++i)
            *reinterpret_cast<f32x4_t *>(&part[(tile0 + i) * M::KS + kpart][lane & 15][4 * (lane >> 4)]) = acc[i];
        coop_lds_barrier();
        if (q < NB) {
            float gs[3];
#pragma unroll
            for (int g = 0; g < 3; ++g) {
                float v = 0.f;
#pragma unroll
                for (int p = 0; p < M::KS; ++p) {
                    v += part[ptile[g] * M::KS + p][pcol[g]][q];
                    v += part[ptile[g] * M::KS + p][pcol[g]][q + 8];
                }
                gs[g] = v;
            }
            const float g0 = gs[0] + bh0, g1 = gs[1] + bh1, g2 = gs[2] + bh2;
            const GruGates v = gru_gates(gi0, gi1, gi2, g0, g1, g2, hprev);
            hprev = dead ? NAN : v.hv;
            // before the stores
            coop_fwd_publish<H, NB>(ca.comm, ca.epoch0 + (unsigned)(t + 1), ca.fault, group, nxt, member, u, q, t, mine,
                                    hprev);
            if (mine) {
                const long row = (long)ns * T + t;
                float *gsv = a.gates + row * 3 * H;
                gsv[j] = v.r; gsv[H + j] = v.z; gsv[2 * H + j] = v.c;
                a.hn[row * H + j] = g2;
                a.out[row * H + j] = hprev;
                a.hall[((long)ns * (T + 1) + t + 1) * H + j] = hprev;
            }
        }
        if (t + 1 < T) {
            dead = coop_fwd_gather<H, NB>(ca.comm, ca.epoch0 + (unsigned)(t + 1), ca.err, group, nxt, dead,
                                          [&](int window, int k, float h) {
                unsigned short tt[3];
                split3(h, tt);
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) hp[nxt][pl][window][k] = tt[pl];
            });
            coop_lds_barrier();
        }
    }
    if (a.hlast != nullptr && q < NB && n0 + q < a.N) a.hlast[(long)(n0 + q) * H + j] = hprev;
}

// The elementwise role of the cooperative backward kernels: thread (es, eu), tid < NB * U, turns dh of window n0 + es,
// unit ej = member * U + eu into the step's d pre-activations.  The saved activations of step t - 1 are requested while
// step t runs (p_*: same reason as the forward kernels' gi -- no L2/HBM round trip on a step's serial path).
template <int H, int NB> struct GruBwdRole {
    static constexpr int U = CoopCfg<H>::U;
    int es, eu, ej, en;
    bool ew, emine;                 // has the role; and its window exists
    float p_dout = 0.f, p_r = 0.f, p_z = 0.f, p_c = 0.f, p_hn = 0.f, p_hp = 0.f;

    __device__ __forceinline__ GruBwdRole(const GruArgs &a, int member, int n0)
    {
        const int tid = threadIdx.x;
        es = tid / U; eu = tid - es * U;
        ej = member * U + eu;
        en = n0 + es;
        ew = tid < NB * U;
        emine = ew && en < a.N;
        if (emine) {
            float *zr = a.dgh + ((long)en * (a.T + 1) + a.T) * 3 * H;      // zero junk row T of dGH
            zr[ej] = 0.f; zr[H + ej] = 0.f; zr[2 * H + ej] = 0.f;
            request(a, a.T - 1);
        }
    }
    __device__ __forceinline__ void request(const GruArgs &a, int t)
    {
        const long row = (long)en * a.T + t;
        const float *gs = a.gates + row * 3 * H;
        p_dout = a.dout[row * H + ej];
        p_r = gs[ej]; p_z = gs[H + ej]; p_c = gs[2 * H + ej];
        p_hn = a.hn[row * H + ej];
        p_hp = a.hall[((long)en * (a.T + 1) + t) * H + ej];
    }
    // step t, dh = dout + carry: stores dGI and dGH, hands the member's dGH entries to lds(dpr, dpz, dhn) (zeros for a
    // window that does not exist) and returns dh z, the part of dh_{t-1} that does not go through W_hh
    template <typename Lds> __device__ __forceinline__ float step(const GruArgs &a, int t, float carry, Lds &&lds)
    {
        if (!ew) return 0.f;
        GruGrad d{0.f, 0.f, 0.f, 0.f, 0.f};
        if (emine) {
            d = gru_grad(p_dout + carry, p_r, p_z, p_c, p_hn, p_hp);
            float *gi = a.dgi + ((long)en * a.T + t) * 3 * H;
            gi[ej] = d.dpr; gi[H + ej] = d.dpz; gi[2 * H + ej] = d.dpn;
            float *gh = a.dgh + ((long)en * (a.T + 1) + t) * 3 * H;
            gh[ej] = d.dpr; gh[H + ej] = d.dpz; gh[2 * H + ej] = d.dhn;
        }
        lds(d.dpr, d.dpz, d.dhn);
        // behind the stores: a request in front of them made the compiler wait for it (vmcnt) where a store reused a register
        if (emine && t > 0) request(a, t - 1);
        return d.keep;
    }
};

// Backward twin of gru_fwd_coop_kernel: member m keeps the SAME 3 U rows of W_hh (its U units x 3 gates) in
// registers, now one COLUMN j' per thread (thread (j', half): 96 rows), forms its partial W_hh^T dGH for all H
// columns and the members exchange the U-column pieces the others own.
//   comm: [groups][2][G (sender)][NB][H] granules (their epochs tell the launches apart: coop_comm_acquire).
template <int H, int NB> __global__ __launch_bounds__(512) void gru_bwd_coop_kernel(GruCoopArgs ca)
{
    using C = CoopCfg<H>;
    constexpr int U = C::U, G = C::G, HALVES = C::HALVES;
    static_assert(3 * U / HALVES == 96, "96 weights per thread");
    static_assert(NB * U <= 512, "one elementwise thread per (window, unit)");
    __shared__ __attribute__((aligned(16))) float dgs[NB][3 * U];          // this member's dGH rows (gate, unit)
    __shared__ float part[HALVES][NB][H];
    const GruArgs &a = ca.g;
    const int T = a.T;
    int group, member;
    coop_who<G>(ca.groups, ca.xcd_map, group, member);
    const int tid = threadIdx.x;
    const int jc = tid & (H - 1), half = tid / H;             // column jc, rows half*96 .. +96 of the member's 3 U
    const int n0 = group * NB;

    f32x2 w[48];
#pragma unroll
    for (int i = 0; i < 96; ++i) {
        const int lr = half * 96 + i;                          // local row = gate*U + unit
        w[i / 2][i % 2] = a.whh[(long)((lr / U) * H + member * U + (lr % U)) * H + jc];
    }
    // not a plain declaration: zeroes row T of dGH and requests step T - 1's saved activations, in front of the time loop
    GruBwdRole<H, NB> e(a, member, n0);
    const int es = e.es, eu = e.eu;
    coop_weights_ready(w);                                     // behind the request above, in front of the time loop
    float carry = 0.f;
    bool dead = false;
    for (int t = T - 1; t >= 0; --t) {
        const int par = t & 1;
        const unsigned epoch = ca.epoch0 + (unsigned)(T - t);              // 1, 2, ...
        const float keep = e.step(a, t, carry, [&](float dpr, float dpz, float dhn) {
            dgs[es][eu] = dpr; dgs[es][U + eu] = dpz; dgs[es][2 * U + eu] = dhn;
        });
        coop_lds_barrier();
        // partial[jc] over this thread's 96 rows, all NB windows
        f32x2 acc[NB];                                         // even / odd rows
#pragma unroll
        for (int s = 0; s < NB; ++s) acc[s] = f32x2{0.f, 0.f};
#pragma unroll
        for (int i4 = 0; i4 < 24; ++i4) {
#pragma unroll
            for (int s = 0; s < NB; ++s) {
                const float4 d4 = *reinterpret_cast<const float4 *>(&dgs[s][half * 96 + 4 * i4]);
                acc[s] = pk_fma(w[2 * i4 + 1], pk_hi(d4), pk_fma(w[2 * i4], pk_lo(d4), acc[s]));
            }
        }
#pragma unroll
        for (int s = 0; s < NB; ++s) part[half][s][jc] = acc[s].x + acc[s].y;
        coop_lds_barrier();
        auto column = [&](int s, int k) {
            float v = part[0][s][k];
#pragma unroll
            for (int hh = 1; hh < HALVES; ++hh) v += part[hh][s][k];
            return v;
        };
        if (t > 0) {
            coop_bwd_publish<H, NB>(ca.comm, epoch, group, par, member, dead, column);
            if (e.ew) {
                float sum = keep + column(es, e.ej);
                dead = coop_bwd_collect<H, NB>(ca.comm, epoch, ca.err, group, par, member, es, e.ej, dead, sum);
                carry = dead ? NAN : sum;
            }
        }
    }
}

template <int H, int NB> __global__ __launch_bounds__(512) void gru_bwd_mfma_kernel(GruCoopArgs ca)
{
    using C = CoopCfg<H>;
    constexpr int U = C::U, G = C::G;
    constexpr int K3 = 3 * U, LDK = K3 + 8;                                 // K = the member's 3U rows of W_hh, in steps of 32
    constexpr int TW = H / 16 / 8;                                          // column tiles per wave: 4 (H = 512), 2 (H = 256)
    static_assert(K3 % 32 == 0 && TW * 8 * 16 == H && TW * (K3 / 32) == 12, "twelve (tile, K step) operands per wave, all of K each");
    static_assert(NB <= 8 && NB * U <= 512, "one elementwise thread per (window, unit)");
    __shared__ __attribute__((aligned(16))) unsigned short dgp[3][8][LDK];  // the three bf16 terms of this member's dGH rows
    __shared__ __attribute__((aligned(16))) unsigned short zrow[LDK];
    __shared__ float part[2][8][H];                                          // [row half of the tile][window][column]
    const GruArgs &a = ca.g;
    const int T = a.T;
    int group, member;
    coop_who<G>(ca.groups, ca.xcd_map, group, member);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n0 = group * NB;

    // B operands: B[k = local row (gate * U + unit)][n = column jc] = W_hh[gate * H + member * U + unit][jc]; wave w: column
    // tiles TW w .. TW w + TW - 1, every K step (no K split: the tile's sums are complete in its accumulators)
    MfmaFrag bw[TW][K3 / 32][3];
#pragma unroll
    for (int i = 0; i < TW; ++i) {
        const int jcol = (wave * TW + i) * 16 + (lane & 15);
#pragma unroll
        for (int ks = 0; ks < K3 / 32; ++ks) {
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int lr = ks * 32 + 8 * (lane >> 4) + e;
                v[e] = a.whh[(long)((lr / U) * H + member * U + (lr % U)) * H + jcol];
            }
            mfma_pack(v, bw[i][ks]);
        }
    }
    for (int idx = tid; idx < 3 * 8 * LDK; idx += 512) (&dgp[0][0][0])[idx] = 0;
    for (int kk = tid; kk < LDK; kk += 512) zrow[kk] = 0;
    __syncthreads();
    const int arow = lane & 15, akg = lane >> 4;
    const bool upper = arow >= 8;
    const char *const planes = reinterpret_cast<const char *>(&dgp[0][0][0]);
    const char *const pa1 = planes + (((upper ? 1 : 0) * 8 + (arow & 7)) * LDK + 8 * akg) * 2;      // [d0 | d1]
    const char *const pa2 = planes + (((upper ? 2 : 0) * 8 + (arow & 7)) * LDK + 8 * akg) * 2;      // [d0 | d2]
    const char *const pa3 = upper ? reinterpret_cast<const char *>(zrow) + 16 * akg : planes + ((2 * 8 + arow) * LDK + 8 * akg) * 2;   // [d2 | 0]
    // not a plain declaration: zeroes row T of dGH and requests step T - 1's saved activations, in front of the time loop
    GruBwdRole<H, NB> e(a, member, n0);
    const int es = e.es, eu = e.eu;
    float carry = 0.f;
    bool dead = false;
    for (int t = T - 1; t >= 0; --t) {
        const int par = t & 1;
        const unsigned epoch = ca.epoch0 + (unsigned)(T - t);              // 1, 2, ...
        const float keep = e.step(a, t, carry, [&](float dpr, float dpz, float dhn) {
            unsigned short t0[3], t1[3], t2[3];
            split3(dpr, t0); split3(dpz, t1); split3(dhn, t2);
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) { dgp[pl][es][eu] = t0[pl]; dgp[pl][es][U + eu] = t1[pl]; dgp[pl][es][2 * U + eu] = t2[pl]; }
        });
        coop_lds_barrier();
        // out[window][column] = sum over the member's rows: four products per K step (mfma_kstep), four column tiles per
        // wave sharing the A fragments
        {
            f32x4_t acc[TW];
#pragma unroll
            for (int i = 0; i < TW; ++i) acc[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < K3 / 32; ++ks) {
                const bf16x8_t a1 = *reinterpret_cast<const bf16x8_t *>(pa1 + ks * 64);
                const bf16x8_t a2 = *reinterpret_cast<const bf16x8_t *>(pa2 + ks * 64);
                const bf16x8_t a3 = *reinterpret_cast<const bf16x8_t *>(pa3 + (upper ? 0 : ks * 64));
#pragma unroll
                for (int i = 0; i < TW; ++i) acc[i] = mfma_kstep(a1, a2, a3, bw[i][ks], acc[i]);
            }
            // lane: column lane % 16 of the tile, rows 4 (lane / 16) .. + 3: rows 0-7 = the windows, rows 8-15 = the second half
#pragma unroll
            for (int i = 0; i < TW; ++i) {
                const int col = (wave * TW + i) * 16 + (lane & 15);
#pragma unroll
                for (int e4 = 0; e4 < 4; ++e4) part[lane >> 5][4 * ((lane >> 4) & 1) + e4][col] = acc[i][e4];
            }
        }
        coop_lds_barrier();
        auto column = [&](int s, int k) { return part[0][s][k] + part[1][s][k]; };
        if (t > 0) {
            coop_bwd_publish<H, NB>(ca.comm, epoch, group, par, member, dead, column);
            if (e.ew) {
                float sum = keep + column(es, e.ej);
                dead = coop_bwd_collect<H, NB>(ca.comm, epoch, ca.err, group, par, member, es, e.ej, dead, sum);
                carry = dead ? NAN : sum;
            }
        }
    }
}


// The matrix-pipe form of the step.  Measured (profiles/r03_gru_stamps.txt): H = 512 with 8 windows per group -- forward 1.47 ->
// 1.23 ms, backward 2.03 -> 1.37 ms per CPC-large step; H = 256 with 2 windows per group (CPC-small: a 16-row tile is 3/4
// padding) -- forward 0.28 -> 0.38 ms (the K parts' partial tiles cost a barrier and LDS round trip more than the FMAs they
// replace), backward 0.30 -> 0.275 ms (no K split there).  CPC_GRU_NO_MFMA=1 / CPC_GRU_MFMA_ALL=1: never / always.
static bool mfma_wanted(int H, int nb, bool backward)
{
    static const bool off = getenv("CPC_GRU_NO_MFMA") != nullptr, all = getenv("CPC_GRU_MFMA_ALL") != nullptr;
    if (off) return false;
    return all || (H == 512 && nb == 8) || (backward && H == 256 && nb >= 2);
}

// what the shared host driver (recurrent.h) needs to know about the GRU
struct GruCell {
    static constexpr int G = 3;
    static constexpr const char *name = "gru", *kernel_names[2] = {"gru_fwd_kernel", "gru_bwd_kernel"},
                                *pack_names[2] = {"gru_pack_fwd_kernel", "gru_pack_bwd_kernel"};
    using Args = GruArgs;
    using CoopArgs = GruCoopArgs;
    using CoopKernel = void (*)(GruCoopArgs);
    static constexpr auto fwd_kernel = gru_fwd_kernel, bwd_kernel = gru_bwd_kernel;

    static void take_saved(RecLayout &g, Carver &sv, int l)
    {
        g.gates[l] = sv.take<float>((size_t)g.N * g.T * 3 * g.H);
        g.extra[l] = sv.take<float>((size_t)g.N * g.T * g.H);             // hn
        g.hall[l] = sv.take<float>((size_t)g.N * (g.T + 1) * g.H);
    }
    static void cell_args(GruArgs &a, float *hn, const float *, float *) { a.hn = hn; }
    static void pack(bool backward, const float *w_hh, float4 *wpack, int H, hipStream_t st)
    {
        hipLaunchKernelGGL((backward ? gru_pack_bwd_kernel : gru_pack_fwd_kernel), dim3(256), dim3(256), 0, st, w_hh, wpack, H);
    }
    // the matrix-pipe form where mfma_wanted says so and it fits a CU too
    template <auto Plain, auto Mfma> static CoopKernel pick(bool mfma)
    {
        if (!coop_kernel_fits<Plain>()) return nullptr;
        return mfma && coop_kernel_fits<Mfma>() ? Mfma : Plain;
    }
    static CoopKernel coop_kernel(bool backward, int H, int nb)
    {
        return coop_dispatch(H, nb, [&](auto h, auto n) -> CoopKernel {
            constexpr int HH = decltype(h)::value, NB = decltype(n)::value;
            if (backward) return pick<gru_bwd_coop_kernel<HH, NB>, gru_bwd_mfma_kernel<HH, NB>>(mfma_wanted(HH, NB, true));
            return pick<gru_fwd_coop_kernel<HH, NB>, gru_fwd_mfma_kernel<HH, NB>>(mfma_wanted(HH, NB, false));
        });
    }
};

}  // namespace cpc

using cpc::GruCell;

extern "C" size_t cpc_gru_saved_bytes(int n, int t, int dim_in, int hidden, int layers)
{
    return cpc::rec_bytes<GruCell>(&cpc::RecLayout::saved_bytes, n, t, dim_in, hidden, layers);
}

extern "C" size_t cpc_gru_scratch_bytes(int n, int t, int dim_in, int hidden, int layers)
{
    return cpc::rec_bytes<GruCell>(&cpc::RecLayout::scratch_bytes, n, t, dim_in, hidden, layers);
}

extern "C" int cpc_gru_forward(const float *x, const float *const *params, const float *h0, float *out, float *h_last,
                               void *saved, void *scratch, int n, int t, int dim_in, int hidden, int layers, cpc_stream_t stream)
{
    CPC_TRY(cpc::coop_error_take("cpc_gru_forward"));      // a time-out of an earlier cooperative launch surfaces here
    return cpc::rec_forward<GruCell>(x, params, h0, nullptr, out, h_last, nullptr, saved, scratch, n, t, dim_in, hidden, layers,
                                     static_cast<hipStream_t>(stream));
}

extern "C" int cpc_gru_backward(const float *x, const float *const *params, const float *dout, void *saved, void *scratch,
                                float *dx, float *const *grads, int n, int t, int dim_in, int hidden, int layers, int deferred,
                                cpc_stream_t stream)
{
    cpc::coop_count_backward_call();
    CPC_TRY(cpc::coop_error_take("cpc_gru_backward"));      // a time-out of an earlier cooperative launch surfaces here
    return cpc::rec_backward<GruCell>(x, params, dout, saved, scratch, dx, grads, n, t, dim_in, hidden, layers,
                                      static_cast<hipStream_t>(stream), deferred != 0);
}
