// CPCAR (mode="LSTM", the reference's default arMode) on gfx950.  Reference: /root/reference/cpc/model.py:158-207
// (:180-183) -> torch.nn.LSTM (batch_first, gate order i, f, g, o):
//     i = sigmoid(W_ii x + b_ii + W_hi h + b_hi)      f = sigmoid(W_if x + b_if + W_hf h + b_hf)
//     g = tanh   (W_ig x + b_ig + W_hg h + b_hg)      o = sigmoid(W_io x + b_io + W_ho h + b_ho)
//     c' = f * c + i * g                               h' = o * tanh(c')
//
// mode="RNN" (model.py:174-176 -> torch.nn.RNN, tanh):  h' = tanh(W_ih x + b_ih + W_hh h + b_hh) shares every kernel
// here with G = 1 gate block instead of 4.
//
// Same shape as the streaming GRU path (gru.hip): per layer one GEMM for all input projections
// GI = X W_ih^T + b_ih, then ONE persistent kernel for the T sequential steps -- a workgroup owns a window for the
// whole sequence, thread (j, q) owns hidden unit j and K slice q, h lives in LDS, W_hh (re-laid out so that lanes
// read consecutive float4s) is streamed from L2 every step.  Backward mirrors it (BPTT), then GEMMs give dW_hh,
// dW_ih and dX.  Both bias gradients are column sums of the same pre-activation gradient.
#include "common.h"
#include "coop.h"
#include "recurrent.h"

#include <algorithm>
#include <cstdlib>

namespace cpc {

namespace {

// W_hh [G*H][H] -> wf[(k4*G + g)*H + j] = W[g*H + j][4*k4 .. 4*k4+3]   (forward: thread j, all k)
__global__ void lstm_pack_fwd_kernel(const float *w, float4 *wf, int H, int G)
{
    const int total = G * H * (H / 4);
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const int j = idx % H;
        const int g = (idx / H) % G;
        const int k4 = idx / (G * H);
        const float *src = w + (long)(g * H + j) * H + 4 * k4;
        wf[idx] = make_float4(src[0], src[1], src[2], src[3]);
    }
}

// W_hh [G*H][H] -> wb[g4*H + j] = (W[4*g4][j], .., W[4*g4+3][j])   (backward: thread j = column)
__global__ void lstm_pack_bwd_kernel(const float *w, float4 *wb, int H, int G)
{
    const int total = G * H / 4 * H;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const int j = idx % H;
        const int g4 = idx / H;
        wb[idx] = make_float4(w[(long)(4 * g4) * H + j], w[(long)(4 * g4 + 1) * H + j], w[(long)(4 * g4 + 2) * H + j],
                              w[(long)(4 * g4 + 3) * H + j]);
    }
}

struct LstmArgs {
    const float *gi;      // [N*T][G*H]  input projections incl. b_ih
    const float4 *wpack;  // packed W_hh (streaming kernels)
    const float *whh;     // [G*H][H] as stored (cooperative kernels)
    const float *bhh;     // [G*H]
    const float *h0, *c0; // [N][H] or null
    float *out;           // [N][T][H]
    float *hall;          // [N][T+1][H]  row 0 = h0, row t+1 = h_t
    float *call;          // [N][T+1][H]  row 0 = c0, row t+1 = c_t            (LSTM only)
    float *gates;         // [N*T][4H]    i, f, g, o after the non-linearity    (LSTM only)
    float *hlast, *clast; // [N][H] or null
    int N, T, H;
    int hp, kq;           // threads = kq * hp: hp = H rounded up to 64, kq = K-split factor
    // backward
    const float *dout;    // [N][T][H]
    float *dgi;           // [N*T][G*H]
    float *dgh;           // [N][T+1][G*H], row T zero (same values as dgi, laid out for the W_hh gradient)
};

// G = 4: LSTM, G = 1: tanh RNN
template <int G>
__global__ void lstm_fwd_kernel(LstmArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];   // hs[H] | red[kq][G][hp]
    const int H = a.H, T = a.T, hp = a.hp, kq = a.kq;
    float *hs = smem;
    float *red = smem + ((H + 3) / 4) * 4;
    const int j = threadIdx.x % hp, q = threadIdx.x / hp;
    const bool act = j < H;
    const int n = blockIdx.x;
    const int k4_per = (H / 4 + kq - 1) / kq;
    const int k4_lo = q * k4_per, k4_hi = min(H / 4, k4_lo + k4_per);

    float hprev = 0.f, cprev = 0.f;
    float bh[G];
#pragma unroll
    for (int g = 0; g < G; ++g) bh[g] = 0.f;
    if (act && q == 0) {
        hprev = a.h0 != nullptr ? a.h0[(long)n * H + j] : 0.f;
        hs[j] = hprev;
        a.hall[((long)n * (T + 1)) * H + j] = hprev;
        if (G == 4) {
            cprev = a.c0 != nullptr ? a.c0[(long)n * H + j] : 0.f;
            a.call[((long)n * (T + 1)) * H + j] = cprev;
        }
#pragma unroll
        for (int g = 0; g < G; ++g) bh[g] = a.bhh[g * H + j];
    }
    __syncthreads();

    for (int t = 0; t < T; ++t) {
        float acc[G];
#pragma unroll
        for (int g = 0; g < G; ++g) acc[g] = 0.f;
        if (act) {
            const float4 *wp = a.wpack + j;
#pragma unroll 4
            for (int k4 = k4_lo; k4 < k4_hi; ++k4) {
                const float4 h4 = reinterpret_cast<const float4 *>(hs)[k4];
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const float4 w4 = wp[(long)(k4 * G + g) * H];
                    acc[g] = fmaf(w4.x, h4.x, fmaf(w4.y, h4.y, fmaf(w4.z, h4.z, fmaf(w4.w, h4.w, acc[g]))));
                }
            }
#pragma unroll
            for (int g = 0; g < G; ++g) red[(q * G + g) * hp + j] = acc[g];
        }
        __syncthreads();                       // partial sums visible; nobody reads hs any more
        if (act && q == 0) {
            float pre[G];
#pragma unroll
            for (int g = 0; g < G; ++g) {
                pre[g] = bh[g];
                for (int qq = 0; qq < kq; ++qq) pre[g] += red[(qq * G + g) * hp + j];
            }
            const long row = (long)n * T + t;
            const float *gin = a.gi + row * G * H;
            float hv;
            if (G == 4) {
                const float ig = coop_sigmoid(gin[j] + pre[0]);
                const float fg = coop_sigmoid(gin[H + j] + pre[G > 1 ? 1 : 0]);
                const float gg = tanhf(gin[2 * H + j] + pre[G > 2 ? 2 : 0]);
                const float og = coop_sigmoid(gin[3 * H + j] + pre[G > 3 ? 3 : 0]);
                const float cv = fg * cprev + ig * gg;
                hv = og * tanhf(cv);
                float *gs = a.gates + row * 4 * H;
                gs[j] = ig; gs[H + j] = fg; gs[2 * H + j] = gg; gs[3 * H + j] = og;
                a.call[((long)n * (T + 1) + t + 1) * H + j] = cv;
                cprev = cv;
            } else {
                hv = tanhf(gin[j] + pre[0]);
            }
            a.out[row * H + j] = hv;
            a.hall[((long)n * (T + 1) + t + 1) * H + j] = hv;
            hs[j] = hv;
            hprev = hv;
        }
        __syncthreads();
    }
    if (act && q == 0) {
        if (a.hlast != nullptr) a.hlast[(long)n * H + j] = hprev;
        if (G == 4 && a.clast != nullptr) a.clast[(long)n * H + j] = cprev;
    }
}

template <int G>
__global__ void lstm_bwd_kernel(LstmArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];   // dg[G*H] | red[kq][hp]
    const int H = a.H, T = a.T, hp = a.hp, kq = a.kq;
    float *dg = smem;
    float *red = smem + G * H;
    const int j = threadIdx.x % hp, q = threadIdx.x / hp;
    const bool act = j < H;
    const int n = blockIdx.x;
    const int g4_total = G * H / 4;
    const int g4_per = (g4_total + kq - 1) / kq;
    const int g4_lo = q * g4_per, g4_hi = min(g4_total, g4_lo + g4_per);

    float carry_h = 0.f, carry_c = 0.f;
    if (act && q == 0) {                                         // zero junk row T of dGH
        float *zr = a.dgh + ((long)n * (T + 1) + T) * G * H;
#pragma unroll
        for (int g = 0; g < G; ++g) zr[g * H + j] = 0.f;
    }
    for (int t = T - 1; t >= 0; --t) {
        if (act && q == 0) {
            const long row = (long)n * T + t;
            const float dh = a.dout[row * H + j] + carry_h;
            float dp[G];
            if (G == 4) {
                const float *gs = a.gates + row * 4 * H;
                const float ig = gs[j], fg = gs[H + j], gg = gs[2 * H + j], og = gs[3 * H + j];
                const float cv = a.call[((long)n * (T + 1) + t + 1) * H + j];
                const float cp = a.call[((long)n * (T + 1) + t) * H + j];
                const float tc = tanhf(cv);
                const float dcv = dh * og * (1.f - tc * tc) + carry_c;
                dp[0] = dcv * gg * ig * (1.f - ig);
                dp[G > 1 ? 1 : 0] = dcv * cp * fg * (1.f - fg);
                dp[G > 2 ? 2 : 0] = dcv * ig * (1.f - gg * gg);
                dp[G > 3 ? 3 : 0] = dh * tc * og * (1.f - og);
                carry_c = dcv * fg;
            } else {
                const float hv = a.hall[((long)n * (T + 1) + t + 1) * H + j];
                dp[0] = dh * (1.f - hv * hv);
            }
            float *gi = a.dgi + row * G * H;
            float *gh = a.dgh + ((long)n * (T + 1) + t) * G * H;
#pragma unroll
            for (int g = 0; g < G; ++g) {
                gi[g * H + j] = dp[g];
                gh[g * H + j] = dp[g];
                dg[g * H + j] = dp[g];
            }
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
            float sum = 0.f;
            for (int qq = 0; qq < kq; ++qq) sum += red[qq * hp + j];
            carry_h = sum;                       // dh_{t-1} = W_hh^T dG_t
        }
        // dg is rewritten only after every thread passed the barrier above; red is read again only after the next
        // two barriers
    }
}

// ------------------------------------------------------------------------------------------------
// On-chip LSTM recurrence for H = 256 and 512 (same scheme as gru.hip's cooperative kernels, see coop.h): a group of
// G workgroups shares NB windows and W_hh never leaves the register file -- 4 gates x 32 columns = 128 weights per
// thread.  The cell state of (window q, unit j) stays in the register of the lane that finishes that pair.
using LstmCoopArgs = CoopArgs<LstmArgs>;

template <int H, int NB> __global__ __launch_bounds__(512) void lstm_fwd_coop_kernel(LstmCoopArgs ca)
{
    using C = CoopCfg<H>;
    constexpr int QS = C::QS, U = C::U, G = C::G;
    static_assert(NB <= QS, "one finishing lane per window");
    __shared__ __attribute__((aligned(16))) float hs[2][NB][C::LDH];
    const LstmArgs &a = ca.g;
    const int T = a.T;
    int group, member;
    coop_who<G>(ca.groups, ca.xcd_map, group, member);
    const int tid = threadIdx.x;
    const int q = tid & (QS - 1), u = tid / QS;
    const int j = member * U + u;
    const int n0 = group * NB;

    f32x2 w[4][16];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int i4 = 0; i4 < 8; ++i4) {
            const float4 v = *reinterpret_cast<const float4 *>(a.whh + (long)(g * H + j) * H + q * 32 + 4 * i4);
            w[g][2 * i4] = pk_lo(v); w[g][2 * i4 + 1] = pk_hi(v);
        }
    const float bh0 = a.bhh[j], bh1 = a.bhh[H + j], bh2 = a.bhh[2 * H + j], bh3 = a.bhh[3 * H + j];

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
    float cprev = 0.f;
    float gin0 = 0.f, gin1 = 0.f, gin2 = 0.f, gin3 = 0.f;
    if (mine) {
        cprev = a.c0 != nullptr ? a.c0[(long)ns * H + j] : 0.f;
        a.call[((long)ns * (T + 1)) * H + j] = cprev;
        const float *gp = a.gi + (long)ns * T * 4 * H;
        gin0 = gp[j]; gin1 = gp[H + j]; gin2 = gp[2 * H + j]; gin3 = gp[3 * H + j];
    }
    bool dead = false;
    for (int t = 0; t < T; ++t) {
        const int cur = t & 1, nxt = cur ^ 1;
        // the input projections of step t were requested one step ago; the next step's are requested now, so that no
        // L2/HBM round trip sits on the serial path of a time step
        const float gi0 = gin0, gi1 = gin1, gi2 = gin2, gi3 = gin3;
        if (mine && t + 1 < T) {
            const float *gp = a.gi + ((long)ns * T + t + 1) * 4 * H;
            gin0 = gp[j]; gin1 = gp[H + j]; gin2 = gp[2 * H + j]; gin3 = gp[3 * H + j];
        }
        float g0 = 0.f, g1 = 0.f, g2 = 0.f, g3 = 0.f;          // the pre-activations of window q, for its finishing lane
#pragma unroll
        for (int s = 0; s < NB; ++s) {
            f32x2 a2[4] = {f32x2{0.f, 0.f}, f32x2{0.f, 0.f}, f32x2{0.f, 0.f}, f32x2{0.f, 0.f}};   // even / odd columns
#pragma unroll
            for (int i4 = 0; i4 < 8; ++i4) {
                const float4 h4 = *reinterpret_cast<const float4 *>(&hs[cur][s][q * 36 + 4 * i4]);
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    a2[g] = pk_fma(w[g][2 * i4 + 1], pk_hi(h4), pk_fma(w[g][2 * i4], pk_lo(h4), a2[g]));
            }
            float acc[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[g] = coop_group_sum<QS>(a2[g].x + a2[g].y);
            if (s == q) { g0 = acc[0]; g1 = acc[1]; g2 = acc[2]; g3 = acc[3]; }
        }
        if (q < NB) {
            const float ig = coop_sigmoid(gi0 + g0 + bh0);
            const float fg = coop_sigmoid(gi1 + g1 + bh1);
            const float gg = tanhf(gi2 + g2 + bh2);
            const float og = coop_sigmoid(gi3 + g3 + bh3);
            const float cv = fg * cprev + ig * gg;
            float hv = og * tanhf(cv);
            cprev = cv;
            if (dead) hv = NAN;
            // publish first: the other members wait for this store, nobody waits for the saved activations below
            coop_fwd_publish<H, NB>(ca.comm, ca.epoch0 + (unsigned)(t + 1), ca.fault, group, nxt, member, u, q, t, mine,
                                    hv);
            if (mine) {
                const long row = (long)ns * T + t;
                float *gs = a.gates + row * 4 * H;
                gs[j] = ig; gs[H + j] = fg; gs[2 * H + j] = gg; gs[3 * H + j] = og;
                a.out[row * H + j] = hv;
                a.hall[((long)ns * (T + 1) + t + 1) * H + j] = hv;
                a.call[((long)ns * (T + 1) + t + 1) * H + j] = cv;
            }
        }
        if (t + 1 < T) {
            dead = coop_fwd_gather<H, NB>(ca.comm, ca.epoch0 + (unsigned)(t + 1), ca.err, group, nxt, dead,
                                          [&](int window, int k, float h) { hs[nxt][window][coop_pad(k)] = h; });
            coop_lds_barrier();
        }
    }
    if (mine) {
        // hall row T was written by this same lane
        if (a.hlast != nullptr) a.hlast[(long)ns * H + j] = a.hall[((long)ns * (T + 1) + T) * H + j];
        if (a.clast != nullptr) a.clast[(long)ns * H + j] = cprev;
    }
}

// Backward twin: member m keeps the SAME 4 U rows of W_hh (its U units x 4 gates) in registers, one COLUMN j' per
// thread (thread (j', half): 128 rows), forms its partial W_hh^T dG for all H columns and the members exchange the
// U-column pieces the others own.   comm: [groups][2][G (sender)][NB][H] granules (coop_comm_acquire).
template <int H, int NB> __global__ __launch_bounds__(512) void lstm_bwd_coop_kernel(LstmCoopArgs ca)
{
    using C = CoopCfg<H>;
    constexpr int U = C::U, G = C::G, HALVES = C::HALVES;
    constexpr int RW = 4 * U / HALVES;                                      // rows per thread
    static_assert(RW == 128, "128 weights per thread");
    static_assert(NB * U <= 512, "one elementwise thread per (window, unit)");
    __shared__ __attribute__((aligned(16))) float dgs[NB][4 * U];          // this member's dG rows (gate, unit)
    __shared__ float part[HALVES][NB][H];
    const LstmArgs &a = ca.g;
    const int T = a.T;
    int group, member;
    coop_who<G>(ca.groups, ca.xcd_map, group, member);
    const int tid = threadIdx.x;
    const int jc = tid & (H - 1), half = tid / H;             // column jc, rows half*RW .. +RW of the member's 4 U
    const int n0 = group * NB;

    f32x2 w[RW / 2];
#pragma unroll
    for (int i = 0; i < RW; ++i) {
        const int lr = half * RW + i;                          // local row = gate*U + unit
        w[i / 2][i % 2] = a.whh[(long)((lr / U) * H + member * U + (lr % U)) * H + jc];
    }
    // elementwise role: thread (es, eu) for tid < NB*U
    const int es = tid / U, eu = tid - es * U;
    const int ej = member * U + eu;
    const int en = n0 + es;
    const bool ew = tid < NB * U;
    const bool emine = ew && en < a.N;
    float carry = 0.f, carry_c = 0.f;
    if (emine) {                                               // zero junk row T of dGH
        float *zr = a.dgh + ((long)en * (T + 1) + T) * 4 * H;
        zr[ej] = 0.f; zr[H + ej] = 0.f; zr[2 * H + ej] = 0.f; zr[3 * H + ej] = 0.f;
    }
    // the saved activations of step t-1 are requested while step t runs (same reason as in the forward kernel)
    float p_dout = 0.f, p_i = 0.f, p_f = 0.f, p_g = 0.f, p_o = 0.f, p_c = 0.f, p_cp = 0.f;
    auto request = [&](int t) {
        const long row = (long)en * T + t;
        const float *gs = a.gates + row * 4 * H;
        p_dout = a.dout[row * H + ej];
        p_i = gs[ej]; p_f = gs[H + ej]; p_g = gs[2 * H + ej]; p_o = gs[3 * H + ej];
        p_cp = a.call[((long)en * (T + 1) + t) * H + ej];
    };
    if (emine) {
        p_c = a.call[((long)en * (T + 1) + T) * H + ej];
        request(T - 1);
    }
    coop_weights_ready(w);
    bool dead = false;
    for (int t = T - 1; t >= 0; --t) {
        const int par = t & 1;
        const unsigned epoch = ca.epoch0 + (unsigned)(T - t);              // 1, 2, ...
        if (ew) {
            float dpi = 0.f, dpf = 0.f, dpg = 0.f, dpo = 0.f;
            if (emine) {
                const long row = (long)en * T + t;
                const float dh = p_dout + carry;
                const float ig = p_i, fg = p_f, gg = p_g, og = p_o, cv = p_c, cp = p_cp;
                p_c = cp;                                       // c_{t-1} is the next step's c_t
                const float tc = tanhf(cv);
                const float dcv = dh * og * (1.f - tc * tc) + carry_c;
                dpi = dcv * gg * ig * (1.f - ig);
                dpf = dcv * cp * fg * (1.f - fg);
                dpg = dcv * ig * (1.f - gg * gg);
                dpo = dh * tc * og * (1.f - og);
                carry_c = dcv * fg;
                float *gi = a.dgi + row * 4 * H;
                gi[ej] = dpi; gi[H + ej] = dpf; gi[2 * H + ej] = dpg; gi[3 * H + ej] = dpo;
                float *gh = a.dgh + ((long)en * (T + 1) + t) * 4 * H;
                gh[ej] = dpi; gh[H + ej] = dpf; gh[2 * H + ej] = dpg; gh[3 * H + ej] = dpo;
            }
            dgs[es][eu] = dpi; dgs[es][U + eu] = dpf; dgs[es][2 * U + eu] = dpg; dgs[es][3 * U + eu] = dpo;
            if (emine && t > 0) request(t - 1);                 // behind the stores (see GruBwdRole::step, gru.hip)
        }
        coop_lds_barrier();
        if (t == 0) break;                                      // dh_{-1} is not needed
        // partial[jc] over this thread's RW rows, all NB windows
        f32x2 acc[NB];                                         // even / odd rows
#pragma unroll
        for (int s = 0; s < NB; ++s) acc[s] = f32x2{0.f, 0.f};
#pragma unroll
        for (int i4 = 0; i4 < RW / 4; ++i4) {
#pragma unroll
            for (int s = 0; s < NB; ++s) {
                const float4 d4 = *reinterpret_cast<const float4 *>(&dgs[s][half * RW + 4 * i4]);
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
        coop_bwd_publish<H, NB>(ca.comm, epoch, group, par, member, dead, column);
        if (ew) {
            float sum = column(es, ej);
            dead = coop_bwd_collect<H, NB>(ca.comm, epoch, ca.err, group, par, member, es, ej, dead, sum);
            carry = dead ? NAN : sum;
        }
    }
}

// G = 4: LSTM, G = 1: tanh RNN
template <int GATES> struct LstmCell {
    static constexpr int G = GATES;
    static constexpr const char *name = G == 4 ? "lstm" : "rnn", *kernel_names[2] = {"lstm_fwd_kernel", "lstm_bwd_kernel"},
                                *pack_names[2] = {"lstm_pack_fwd_kernel", "lstm_pack_bwd_kernel"};
    using Args = LstmArgs;
    using CoopArgs = LstmCoopArgs;
    using CoopKernel = void (*)(LstmCoopArgs);
    static constexpr auto fwd_kernel = lstm_fwd_kernel<G>, bwd_kernel = lstm_bwd_kernel<G>;

    static void take_saved(RecLayout &g, Carver &sv, int l)
    {
        if (G == 4) g.gates[l] = sv.take<float>((size_t)g.N * g.T * 4 * g.H);
        g.hall[l] = sv.take<float>((size_t)g.N * (g.T + 1) * g.H);
        if (G == 4) g.extra[l] = sv.take<float>((size_t)g.N * (g.T + 1) * g.H);       // call
    }
    static void cell_args(LstmArgs &a, float *call, const float *c0, float *clast) { a.call = call; a.c0 = c0; a.clast = clast; }
    static void pack(bool backward, const float *w_hh, float4 *wpack, int H, hipStream_t st)
    {
        hipLaunchKernelGGL((backward ? lstm_pack_bwd_kernel : lstm_pack_fwd_kernel), dim3(256), dim3(256), 0, st, w_hh, wpack, H, G);
    }
    // cooperative kernels exist for the LSTM at H = 256 / 512
    static CoopKernel coop_kernel(bool backward, int H, int nb)
    {
        if (G != 4) return nullptr;
        return coop_dispatch(H, nb, [&](auto h, auto n) -> CoopKernel {
            constexpr int HH = decltype(h)::value, NB = decltype(n)::value;
            if (backward) return coop_kernel_fits<lstm_bwd_coop_kernel<HH, NB>>() ? lstm_bwd_coop_kernel<HH, NB> : nullptr;
            return coop_kernel_fits<lstm_fwd_coop_kernel<HH, NB>>() ? lstm_fwd_coop_kernel<HH, NB> : nullptr;
        });
    }
};

}  // namespace

}  // namespace cpc

using cpc::LstmCell;
using cpc::RecLayout;

extern "C" size_t cpc_lstm_saved_bytes(int n, int t, int dim_in, int hidden, int layers)
{
    return cpc::rec_bytes<LstmCell<4>>(&RecLayout::saved_bytes, n, t, dim_in, hidden, layers);
}

extern "C" size_t cpc_lstm_scratch_bytes(int n, int t, int dim_in, int hidden, int layers)
{
    return cpc::rec_bytes<LstmCell<4>>(&RecLayout::scratch_bytes, n, t, dim_in, hidden, layers);
}

extern "C" int cpc_lstm_forward(const float *x, const float *const *params, const float *h0, const float *c0, float *out,
                                float *h_last, float *c_last, void *saved, void *scratch, int n, int t, int dim_in, int hidden,
                                int layers, cpc_stream_t stream)
{
    CPC_TRY(cpc::coop_error_take("cpc_lstm_forward"));      // a time-out of an earlier cooperative launch surfaces here
    return cpc::rec_forward<LstmCell<4>>(x, params, h0, c0, out, h_last, c_last, saved, scratch, n, t, dim_in, hidden, layers,
                                         static_cast<hipStream_t>(stream));
}

extern "C" int cpc_lstm_backward(const float *x, const float *const *params, const float *dout, void *saved, void *scratch,
                                 float *dx, float *const *grads, int n, int t, int dim_in, int hidden, int layers, int deferred,
                                 cpc_stream_t stream)
{
    cpc::coop_count_backward_call();
    CPC_TRY(cpc::coop_error_take("cpc_lstm_backward"));      // a time-out of an earlier cooperative launch surfaces here
    return cpc::rec_backward<LstmCell<4>>(x, params, dout, saved, scratch, dx, grads, n, t, dim_in, hidden, layers,
                                          static_cast<hipStream_t>(stream), deferred != 0);
}

extern "C" size_t cpc_rnn_saved_bytes(int n, int t, int dim_in, int hidden, int layers)
{
    return cpc::rec_bytes<LstmCell<1>>(&RecLayout::saved_bytes, n, t, dim_in, hidden, layers);
}

extern "C" size_t cpc_rnn_scratch_bytes(int n, int t, int dim_in, int hidden, int layers)
{
    return cpc::rec_bytes<LstmCell<1>>(&RecLayout::scratch_bytes, n, t, dim_in, hidden, layers);
}

extern "C" int cpc_rnn_forward(const float *x, const float *const *params, const float *h0, float *out, float *h_last,
                               void *saved, void *scratch, int n, int t, int dim_in, int hidden, int layers,
                               cpc_stream_t stream)
{
    CPC_TRY(cpc::coop_error_take("cpc_rnn_forward"));      // a time-out of an earlier cooperative launch surfaces here
    return cpc::rec_forward<LstmCell<1>>(x, params, h0, nullptr, out, h_last, nullptr, saved, scratch, n, t, dim_in, hidden, layers,
                                         static_cast<hipStream_t>(stream));
}

extern "C" int cpc_rnn_backward(const float *x, const float *const *params, const float *dout, void *saved, void *scratch,
                                float *dx, float *const *grads, int n, int t, int dim_in, int hidden, int layers, int deferred,
                                cpc_stream_t stream)
{
    CPC_REQUIRE(deferred == 0, "cpc_rnn_backward: the RNN cell has no deferred form (deferred = %d)", deferred);
    cpc::coop_count_backward_call();
    CPC_TRY(cpc::coop_error_take("cpc_rnn_backward"));      // a time-out of an earlier cooperative launch surfaces here
    return cpc::rec_backward<LstmCell<1>>(x, params, dout, saved, scratch, dx, grads, n, t, dim_in, hidden, layers,
                                          static_cast<hipStream_t>(stream), false);
}
