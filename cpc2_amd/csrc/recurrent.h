// Host driver of the recurrent context networks: the memory layout, the per-layer forward and backward loops and the choice
// between a cell's cooperative and streaming kernels, written once.  gru.hip and lstm.hip each describe their cell:
//
//     struct Cell {
//         static constexpr int G;                          // gate blocks: rows of W_ih / W_hh are G * H
//         static constexpr const char *name, *kernel_names[2], *pack_names[2];      // error messages: the cell; [backward]: its kernels
//         using Args, CoopArgs, CoopKernel;                // the kernels' arguments; coop.h's CoopArgs<Args>; void (*)(CoopArgs)
//         static constexpr auto fwd_kernel, bwd_kernel;    // the streaming kernels: void (*)(Args)
//         static void take_saved(RecLayout &, Carver &, int l);         // layer l's saved tensors besides outl
//         static void cell_args(Args &, float *extra, const float *c0, float *clast);       // what only this cell's kernels read
//         static void pack(bool backward, const float *w_hh, float4 *wpack, int H, hipStream_t);    // launches the pack kernel
//         static CoopKernel coop_kernel(bool backward, int H, int nb);  // nullptr: none for this shape, or it does not fit a CU
//     };
#pragma once
#include "common.h"
#include "coop.h"

#include <algorithm>
#include <type_traits>

namespace cpc {

struct RecLayout {
    int N, T, Din, H, layers;
    int hp, kq;                            // threads of a streaming kernel = kq * hp: hp = H rounded up to 64, kq = K-split factor
    // saved, per layer (extra: the GRU's hn, the LSTM's call)
    float *gates[8], *hall[8], *extra[8], *outl[8];
    size_t saved_bytes;
    // scratch
    float *gi, *dgi, *dgh, *dxa, *dxb, *wt_l[8], *cs, *tn, *tn2;
    float *dgi_l[8], *dgh_l[8];            // layers 1..: gate gradients of their own (deferred tail: the side stream still reads them)
    size_t tn2_bytes;
    float4 *wpack;
    size_t tn_bytes, scratch_bytes;
};

template <typename Cell>
static int rec_layout(RecLayout &g, int N, int T, int Din, int H, int layers, void *saved, void *scratch)
{
    constexpr int G = Cell::G;
    CPC_REQUIRE(N > 0 && T > 0 && Din > 0, "%s: bad shape n=%d t=%d in=%d", Cell::name, N, T, Din);
    CPC_REQUIRE(H % 4 == 0 && H >= 4 && H <= 1024, "%s: hidden %d must be a multiple of 4 and <= 1024", Cell::name, H);
    CPC_REQUIRE(layers >= 1 && layers <= 8, "%s: 1..8 layers supported (got %d)", Cell::name, layers);
    g = RecLayout{};
    g.N = N; g.T = T; g.Din = Din; g.H = H; g.layers = layers;
    g.hp = std::max(64, (int)cdiv(H, 64) * 64);
    g.kq = std::max(1, std::min(1024 / g.hp, H / 4));
    Carver sv(saved);
    for (int l = 0; l < layers; ++l) {
        Cell::take_saved(g, sv, l);
        g.outl[l] = (l + 1 < layers) ? sv.take<float>((size_t)N * T * H) : nullptr;
    }
    g.saved_bytes = sv.used();
    Carver sc(scratch);
    const int dmax = std::max(Din, H);
    g.gi = sc.take<float>((size_t)N * T * G * H);
    g.dgi = g.gi;                                     // forward's GI and backward's dGI never coexist
    g.dgh = sc.take<float>((size_t)N * (T + 1) * G * H);
    g.dxa = sc.take<float>((size_t)N * T * dmax);
    g.dxb = sc.take<float>((size_t)N * T * dmax);
    for (int l = 0; l < layers; ++l) g.wt_l[l] = sc.take<float>((size_t)G * H * dmax);        // W_ih^T of every layer (backward)
    g.wpack = sc.take<float4>((size_t)G * H * H / 4);
    g.cs = sc.take<float>(colsum_rows_scratch_bytes(G * H) / sizeof(float));
    g.tn_bytes = std::max(gemm_tn_scratch_bytes(G * H, H, (long)N * (T + 1)), gemm_tn_scratch_bytes(G * H, dmax, (long)N * T));
    g.tn_bytes = std::max(g.tn_bytes, gemm_tn_scratch_bytes(G * H, Din, (long)N * T));
    // the same room serves an ordered K split of the projections (GI = X W_ih^T, dX = dGI W_ih) when they have few tiles
    g.tn_bytes = std::max(g.tn_bytes, std::max(gemm_nt_scratch_bytes((long)N * T, G * H, dmax), gemm_nt_scratch_bytes((long)N * T, dmax, G * H)));
    g.tn = sc.take<float>(g.tn_bytes / sizeof(float));
    // (the input-gradient product's K split when the weight-gradient products run beside it on the side stream: rec_backward, defer_tail)
    g.tn2_bytes = gemm_nt_scratch_bytes((long)N * T, dmax, G * H);
    g.tn2 = sc.take<float>(g.tn2_bytes / sizeof(float));
    g.dgi_l[0] = g.dgi; g.dgh_l[0] = g.dgh;
    for (int l = 1; l < layers; ++l) {
        g.dgi_l[l] = sc.take<float>((size_t)N * T * G * H);
        g.dgh_l[l] = sc.take<float>((size_t)N * (T + 1) * G * H);
    }
    g.scratch_bytes = sc.used();
    return CPC_OK;
}

// cpc_*_saved_bytes / cpc_*_scratch_bytes: 0 (and the message set) for a shape the cell does not take
template <typename Cell> static size_t rec_bytes(size_t RecLayout::*which, int N, int T, int Din, int H, int layers)
{
    RecLayout g;
    return rec_layout<Cell>(g, N, T, Din, H, layers, nullptr, nullptr) == CPC_OK ? g.*which : 0;
}

inline int coop_cus() { static const int n = coop_cu_count(); return n; }      // asked once per process

// does the kernel fit a CU?  (cached per instance: the occupancy query is not free)
template <auto Kernel> static bool coop_kernel_fits() { static const bool f = coop_fits(Kernel, 1, 1); return f; }

// the hidden sizes and windows per group that have cooperative kernels, as constants: f(integral_constant<H>, integral_constant<NB>)
template <typename F> static auto coop_dispatch(int H, int nb, F &&f)
{
    auto with_nb = [&](auto h) {
        switch (nb) {
        case 1: return f(h, std::integral_constant<int, 1>{});
        case 2: return f(h, std::integral_constant<int, 2>{});
        case 4: return f(h, std::integral_constant<int, 4>{});
        default: return f(h, std::integral_constant<int, 8>{});
        }
    };
    return H == 256 ? with_nb(std::integral_constant<int, 256>{}) : with_nb(std::integral_constant<int, 512>{});
}

// One layer's T steps: in a cooperative kernel if the cell has one for this shape that fits a CU and whose grid fits the chip (the
// cooperative kernel needs every workgroup resident at once, 1 per CU), else in the streaming kernel, which has no such requirement
template <typename Cell> static int rec_launch(bool backward, const RecLayout &g, const typename Cell::Args &a, hipStream_t st)
{
    constexpr int G = Cell::G;
    const ProfSlot slot = backward ? PROF_GRU_BWD : PROF_GRU_FWD;
    const int n_cus = coop_cus();
    int members = 0;
    const int nb = coop_allowed() ? coop_windows_per_group(a.H, a.N, n_cus, &members) : 0;
    const typename Cell::CoopKernel kernel = nb != 0 ? Cell::coop_kernel(backward, a.H, nb) : nullptr;
    if (kernel == nullptr || cdiv(a.N, nb) * members > n_cus) {
        Cell::pack(backward, a.whh, g.wpack, a.H, st);      // (the streaming kernel's weight layout only)
        CPC_CHECK_LAUNCH(Cell::pack_names[backward]);
        ProfScope prof(slot, st);
        // forward: hs[H] | red[kq][G][hp];  backward: the step's gate gradients [G * H] | red[kq][hp]
        const size_t lds = sizeof(float) * (backward ? (size_t)G * a.H + (size_t)g.kq * g.hp : cdiv(a.H, 4) * 4 + (size_t)g.kq * G * g.hp);
        hipLaunchKernelGGL((backward ? Cell::bwd_kernel : Cell::fwd_kernel), dim3((unsigned)a.N), dim3(g.kq * g.hp), lds, st, a);
        return CPC_OK;
    }
    typename Cell::CoopArgs ca{};
    ca.g = a; ca.groups = (int)cdiv(a.N, nb);
    ca.xcd_map = (ca.groups % 8 == 0) ? 1 : 0;
    ca.err = coop_error_word(); ca.fault = coop_fault_injection();
    // granules: forward [groups][2][G][U][NB] (G * U = H), backward [groups][2][G][NB][H]
    CPC_TRY(coop_comm_acquire(sizeof(gu64_t) * (size_t)ca.groups * 2 * (backward ? members : 1) * nb * a.H, a.T, st, &ca.comm, &ca.epoch0));
    ProfScope prof(slot, st);
    coop_count_launch();
    hipLaunchKernelGGL(kernel, dim3((unsigned)(ca.groups * members)), dim3(512), 0, st, ca);
    return CPC_OK;
}

// c0 / c_last: the LSTM's cell state (null for the other cells)
template <typename Cell>
static int rec_forward(const float *x, const float *const *prm, const float *h0, const float *c0, float *out, float *h_last,
                       float *c_last, void *saved, void *scratch, int N, int T, int Din, int H, int layers, hipStream_t st)
{
    constexpr int G = Cell::G;
    RecLayout g;
    CPC_TRY(rec_layout<Cell>(g, N, T, Din, H, layers, saved, scratch));
    const float *xin = x;
    int din = Din;
    for (int l = 0; l < layers; ++l) {
        const float *w_ih = prm[4 * l], *w_hh = prm[4 * l + 1], *b_ih = prm[4 * l + 2], *b_hh = prm[4 * l + 3];
        RowMap none{};
        none.splitk_scratch = g.tn; none.splitk_bytes = g.tn_bytes;
        CPC_TRY(gemm_nt(xin, din, w_ih, din, g.gi, (long)G * H, b_ih, (long)N * T, G * H, din, none, st));
        const size_t state = (size_t)l * N * H;
        typename Cell::Args a{};
        a.gi = g.gi; a.wpack = g.wpack; a.whh = w_hh; a.bhh = b_hh;
        a.h0 = h0 ? h0 + state : nullptr;
        a.out = (l + 1 < layers) ? g.outl[l] : out;
        a.hall = g.hall[l]; a.gates = g.gates[l];
        a.hlast = h_last ? h_last + state : nullptr;
        a.N = N; a.T = T; a.H = H; a.hp = g.hp; a.kq = g.kq;
        Cell::cell_args(a, g.extra[l], c0 ? c0 + state : nullptr, c_last ? c_last + state : nullptr);
        CPC_TRY(rec_launch<Cell>(false, g, a, st));
        CPC_CHECK_LAUNCH(Cell::kernel_names[0]);
        xin = a.out;
        din = H;
    }
    return CPC_OK;
}

// defer_tail: the weight gradients of every layer (nothing on `st` needs them before the optimiser) are produced on the library's
// side stream: layer l's beside the recurrent kernel of layer l - 1 (latency-bound: the matrix pipe is idle), layer 0's beside what
// the caller enqueues next (the encoder's backward: its normalisation / reduction kernels leave the matrix pipe idle for ~0.3 ms per
// step).  Each layer keeps its gate gradients in a buffer of its own for that.  cpc_side_tail_join makes a stream wait for them
template <typename Cell>
static int rec_backward(const float *x, const float *const *prm, const float *dout, void *saved, void *scratch, float *dx,
                        float *const *grads, int N, int T, int Din, int H, int layers, hipStream_t st, bool defer_tail)
{
    constexpr int G = Cell::G;
    const int GH = G * H;
    RecLayout g;
    CPC_TRY(rec_layout<Cell>(g, N, T, Din, H, layers, saved, scratch));
    const float *dcur = dout;
    // W_ih^T of every layer that has an input gradient, in front of the first recurrent kernel: the transposes depend on the weights
    // only, and a small kernel queued BEHIND a recurrent kernel starts while the deferred criterion sum / the weight-gradient
    // products hold the chip on the side stream -- seen at 212 us (3 MB) on the critical path of CPC-large, 5 us alone
    for (int l = layers - 1; l >= 0; --l)
        if (l > 0 || dx != nullptr) CPC_TRY(transpose2d(prm[4 * l], g.wt_l[l], GH, (l == 0) ? Din : H, st));
    for (int l = layers - 1; l >= 0; --l) {
        const float *w_hh = prm[4 * l + 1];
        const float *xin = (l == 0) ? x : g.outl[l - 1];
        const int din = (l == 0) ? Din : H;
        typename Cell::Args a{};
        a.wpack = g.wpack; a.whh = w_hh; a.hall = g.hall[l]; a.gates = g.gates[l];
        a.N = N; a.T = T; a.H = H; a.hp = g.hp; a.kq = g.kq;
        Cell::cell_args(a, g.extra[l], nullptr, nullptr);
        // (deferred tail: every layer's gate gradients stay where they are until the side stream has used them)
        float *const dgi = defer_tail ? g.dgi_l[l] : g.dgi, *const dgh = defer_tail ? g.dgh_l[l] : g.dgh;
        a.dout = dcur; a.dgi = dgi; a.dgh = dgh;
        CPC_TRY(infonce_deferred_mark(st));       // (see infonce_deferred_start below)
        CPC_TRY(rec_launch<Cell>(true, g, a, st));
        CPC_CHECK_LAUNCH(Cell::kernel_names[1]);
        CPC_TRY(infonce_deferred_start(st));      // (no-op unless a deferred criterion backward is waiting to run beside this)

        hipStream_t wst = st;
        if (defer_tail) CPC_TRY(side_tail_begin(st, &wst));
        // dW_hh[g][k] = sum_{n,t} dGH[n,t][g] * h_{t-1}[n][k]   (hall row t is h_{t-1}; row T of dGH is zero)
        CPC_TRY(gemm_tn(dgh, GH, g.hall[l], H, grads[4 * l + 1], H, GH, H, (long)N * (T + 1), g.tn, g.tn_bytes, 0, 0, wst));
        CPC_TRY(colsum_rows(dgh, GH, (long)N * (T + 1), GH, grads[4 * l + 3], g.cs, wst));
        // dW_ih[g][k] = sum dGI[n,t][g] * x[n,t][k]
        CPC_TRY(gemm_tn(dgi, GH, xin, din, grads[4 * l], din, GH, din, (long)N * T, g.tn, g.tn_bytes, 0, 0, wst));
        CPC_TRY(colsum_rows(dgi, GH, (long)N * T, GH, grads[4 * l + 2], g.cs, wst));
        if (defer_tail) CPC_TRY(side_tail_end());
        // dX = dGI . W_ih
        float *dxl = (l == 0) ? dx : ((l % 2) ? g.dxa : g.dxb);
        if (dxl != nullptr) {
            RowMap none{};
            if (defer_tail) { none.splitk_scratch = g.tn2; none.splitk_bytes = g.tn2_bytes; }        // (g.tn is the side stream's now)
            else { none.splitk_scratch = g.tn; none.splitk_bytes = g.tn_bytes; }
            CPC_TRY(gemm_nt(dgi, GH, g.wt_l[l], GH, dxl, din, nullptr, (long)N * T, din, GH, none, st));
        }
        dcur = dxl;
    }
    return CPC_OK;
}

}  // namespace cpc
