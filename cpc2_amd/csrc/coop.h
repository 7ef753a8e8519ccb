// Pieces shared by the cooperative (weights-in-registers) recurrent kernels of gru.hip and lstm.hip.
#pragma once
#include "common.h"

namespace cpc {

// A GROUP of G workgroups (512 threads each, one per CU) shares NB windows.  Forward: thread (u, q) = unit u of the
// member's U units, K slice q of 32 columns, all gates.  H = 256: 8 slices, U = 64, G = 4;  H = 512: 16 slices,
// U = 32, G = 16.
template <int H> struct CoopCfg {
    static constexpr int QS = H / 32;            // K slices of 32 columns
    static constexpr int U = 512 / QS;           // units per member
    static constexpr int G = H / U;              // workgroups per group
    static constexpr int LDH = QS * 36 + 4;      // padded h row: chunk q of 32 floats at q*36; rows 4 banks apart (the gather
                                                 // writes the NB windows of a unit from neighbouring lanes)
    static constexpr int HALVES = 512 / H;       // backward: threads per W_hh column
};

typedef unsigned long long gu64_t;               // {epoch, value} granule
#define COOP_GLOBAL __attribute__((address_space(1)))

__device__ __forceinline__ int coop_pad(int k) { return (k >> 5) * 36 + (k & 31); }

// Forward granules: [group][set][member][unit u][window].  A member's piece of a set is ONE run of NB * U granules that nobody
// else writes, and what a wave publishes (its 4 or 8 units x NB windows) is whole 128-byte lines.  Round 2 had
// [group][set][window][H]: 32-byte pieces of lines shared with other members, which with a group on one XCD cost 5.4 us per
// step at H = 512 against 2.35 (tools/exchange_probe.hip, profiles/r03_exchange_probe.txt).
template <int H, int NB> __device__ __forceinline__ long coop_fwd_slot(int group, int set, int member, int u, int window)
{
    return (((long)group * 2 + set) * CoopCfg<H>::G + member) * (NB * CoopCfg<H>::U) + u * NB + window;
}
// granule idx (0 .. NB * H) of a set, in memory order -> window and unit k (0 .. H) of the group
template <int H, int NB> __device__ __forceinline__ void coop_fwd_who(int idx, int &window, int &k)
{
    constexpr int U = CoopCfg<H>::U;
    const int g = idx / (NB * U), p = idx - g * (NB * U);
    window = p % NB;
    k = g * U + p / NB;
}

// two f32 lanes as one value.  (Device code is built WITHOUT the packed-f32 VALU instructions -- build.py, DEVICE_FLAGS: round 3's
// launch-to-launch differences -- so pk_fma compiles to two v_fma_f32; the type is kept for the register-pair layout of the weights.)
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 pk_fma(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f32x2 pk_lo(const float4 &v) { return f32x2{v.x, v.y}; }
__device__ __forceinline__ f32x2 pk_hi(const float4 &v) { return f32x2{v.z, v.w}; }

// Barrier between the phases of a time step.  The waves of a member talk to each other through LDS only, so only LDS
// traffic has to have landed: __syncthreads() also waits for every global load and store of the wave (vmcnt(0)) -- the loads
// requested a step ahead, the saved activations nobody waits for -- and put a memory round trip on every step's serial
// path (H = 512: 2.2 us of the backward step's 8.2, profiles/r03_gru_stamps.txt).
__device__ __forceinline__ void coop_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// The weights are loaded once, before the time loop; used here so that the compiler waits for them HERE.  Left alone it waits
// for the last of them at their first use inside the loop, with a vmcnt that counts the memory operations issued behind them
// -- which in steady state are the loop's own requests and stores: every step then sat out a memory round trip in the middle
// of its arithmetic (gru_bwd_coop_kernel<512>: s_waitcnt vmcnt(7) .. vmcnt(1) between the FMAs).
template <int N> __device__ __forceinline__ void coop_weights_ready(f32x2 (&w)[N])
{
#pragma unroll
    for (int i = 0; i < N; ++i) asm volatile("" : "+v"(w[i]));
}

template <int CTRL> __device__ __forceinline__ float dpp_get(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
// sum over an aligned group of QS = 8 or 16 consecutive lanes, left in every lane of the group: data-parallel
// primitives (VALU speed) instead of ds_bpermute round trips through the LDS crossbar
template <int QS> __device__ __forceinline__ float coop_group_sum(float v)
{
    static_assert(QS == 8 || QS == 16, "half a DPP row or a full one");
    v += dpp_get<0xB1>(v);                  // quad_perm [1,0,3,2]
    v += dpp_get<0x4E>(v);                  // quad_perm [2,3,0,1]
    v += dpp_get<0x141>(v);                 // row_half_mirror: the other quad of the 8
    if (QS == 16) v += dpp_get<0x140>(v);   // row_mirror: the other half of the 16
    return v;
}

template <int G> __device__ __forceinline__ void coop_who(int groups, int xcd_map, int &group, int &member)
{
    if (xcd_map) {                          // members of a group on one XCD (speed only: blocks b, b+8 share one)
        const int xcd = blockIdx.x & 7, i = blockIdx.x >> 3;
        group = xcd * (groups / 8) + i / G;
        member = i % G;
    } else {
        group = blockIdx.x / G;
        member = blockIdx.x % G;
    }
}

// window count -> windows per group (0: not covered), for the hidden sizes that have a cooperative kernel; every
// workgroup must be resident at once (1 per CU)
static inline int coop_windows_per_group(int H, int N, int n_cus, int *groups_per)
{
    const int G = H == 256 ? CoopCfg<256>::G : (H == 512 ? CoopCfg<512>::G : 0);
    if (G == 0 || n_cus < G) return 0;
    const int max_groups = n_cus / G;
    for (int nb = 1; nb <= 8; nb *= 2)
        if ((int)cdiv(N, nb) <= max_groups) { *groups_per = G; return nb; }
    return 0;
}

static inline int coop_cu_count()
{
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    return v;
}

// ---- failing loudly -------------------------------------------------------------------------------------------------
// The cooperative kernels need every workgroup of a launch resident at once.  (1) Before choosing them the launcher asks
// the occupancy API whether the kernel fits a CU at all and compares the grid with the CU count (coop_fits).  (2) Every
// wait is bounded; a wave whose wait runs out still poisons its outputs with NaN, and writes a code into ONE host-visible
// word (mapped, coherent host memory: no synchronisation needed to read it).  The recurrent entry points look at that word
// before they launch anything and cpc_async_error_check(stream) after synchronising the stream: both return CPC_ERR_HIP
// with a message and clear the word -- like a HIP asynchronous error, a time-out surfaces at the next call.
int *coop_error_word();                         // device-visible address of the word (nullptr: allocation failed)
int coop_error_take(const char *where);         // host: CPC_OK, or CPC_ERR_HIP (message set, word cleared)
int coop_fault_injection();                     // tests: CPC_COOP_FAULT=1 makes member 0 of group 0 withhold one publish
// Granule memory of the cooperative kernels: ONE buffer per (device, stream) that the library owns and nothing else ever writes,
// zeroed once; every launch gets a range of epochs of its own ([*epoch0 + 1, *epoch0 + T]), so a granule left by an earlier launch
// can never be taken for a current one and nothing has to be cleared between launches (rounds 2-4 carved the granules out of the
// caller's scratch arena -- which other kernels write -- and cleared them in front of every launch: two memsets of 7-14 us on the
// step's critical path).  The buffer grows when a launch needs more; the epoch counter wraps by clearing it once.
int coop_comm_acquire(size_t bytes, int T, hipStream_t st, gu64_t **comm, unsigned *epoch0);
bool coop_allowed();                            // process-wide policy (cpc_coop_set_policy): false = streaming kernels only
void coop_count_launch();                       // every cooperative recurrent launch is counted (cpc_coop_launches)
long coop_launches();
void coop_count_backward_call();                 // every recurrent backward entry (any kernel kind) is counted (cpc_recurrent_backward_calls)
enum { COOP_ERR_FWD_WAIT = 1, COOP_ERR_BWD_WAIT = 2, COOP_ERR_NONFINITE_GRAD = 3, COOP_ERR_BAD_INDEX = 4 };     // 3: the Adam kernel (rowops.hip), 4: the criterion's index check (infonce.hip)
__device__ __forceinline__ void coop_report(int *err, int code)
{
    if (err != nullptr) __hip_atomic_store(err, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
template <typename K> static inline bool coop_fits(K kernel, unsigned grid, int n_cus)
{
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 512, 0) != hipSuccess) return false;
    return per_cu >= 1 && (int)grid <= n_cus;   // one workgroup per CU is what the grouping assumes
}

// ---- the hand-off ---------------------------------------------------------------------------------------------------
// The members of a group exchange a step's results through 8-byte {epoch, value} granules in L2: one relaxed agent-scope
// store each, polled with relaxed agent-scope loads (MI355X guide, Guideline 16 R2).  A member can be at most one step
// ahead of another, so two granule sets (epoch parity) suffice.  Every spin is bounded: on time-out the thread poisons
// what it hands on with NaN, reports, and never waits again.  This is the only place that stores, loads or waits for a
// granule; the kernels of gru.hip and lstm.hip say where a value comes from and where it goes.
// What the functions need of a launch (comm, epoch, err) they take as scalars, and the thread's `dead` flag goes in and
// comes back by value.  Handed over by reference -- the argument struct, a flag the callee sets -- the compiler finds
// them a pass later than the kernels' own locals and makes other code of the same text.  Measured at this change
// (gfx950, -Rpass-analysis=kernel-resource-usage; VGPRs by value, as here and as with the hand-off written out in the
// kernel, against `bool &dead`):  lstm_bwd_coop_kernel<512,1> 227 / 228, <512,2> 229 / 230, <512,4> 228 / 229,
// lstm_fwd_coop_kernel<256,8> 198 / 199, gru_fwd_coop_kernel<256,8> 193 / 194; and with `bool &dead` every poll of one to
// three granules came out unrolled eight times (lstm_fwd_coop_kernel<256,1>: 772 instructions -> 868, eight s_sleep).

// what a cooperative kernel is launched with (recurrent.h fills it in): the cell's own arguments and the hand-off's
template <typename Args> struct CoopArgs {
    Args g;
    gu64_t *comm;          // granules (coop_comm_acquire: the library's own buffer): fwd [groups][2][G][U][NB] (coop_fwd_slot), bwd [groups][2][G][NB][H]
    unsigned epoch0;       // this launch's epochs are epoch0 + 1 .. epoch0 + T: no granule of an earlier launch carries one of them
    int groups, xcd_map;
    int *err;              // host-visible error word, or nullptr
    int fault;             // tests: member 0 of group 0 withholds its publish of step 1
};

__device__ __forceinline__ float coop_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

__device__ __forceinline__ void coop_publish(gu64_t *granule, unsigned epoch, float v)
{
    __hip_atomic_store((COOP_GLOBAL gu64_t *)granule, ((gu64_t)epoch << 32) | (gu64_t)__float_as_uint(v), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}

// The one bounded wait: until all N granules carry `epoch`.  They are loaded together -- one L2 round trip per attempt,
// not N in a row -- and x[] holds what was loaded last.  Returns the thread's new `dead`: true when the wait ran out, now
// (the code is reported) or at an earlier step -- a dead thread never waits again, and the caller poisons what it derives
// from x.  N is a compile-time constant and every loop is unrolled: slot and x stay in registers.
template <int N>
__device__ __forceinline__ bool coop_poll(COOP_GLOBAL gu64_t *const (&slot)[N], unsigned epoch, gu64_t (&x)[N], bool dead, int *err,
                                          int code)
{
    constexpr unsigned BOUND = 1u << 22;
    unsigned spins = dead ? BOUND : 0u;
    for (;;) {
        bool ready = true;
#pragma unroll
        for (int i = 0; i < N; ++i) x[i] = __hip_atomic_load(slot[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int i = 0; i < N; ++i) ready = ready && (unsigned)(x[i] >> 32) == epoch;
        if (ready) break;
        if (++spins > BOUND) { dead = true; coop_report(err, code); break; }
        __builtin_amdgcn_s_sleep(1);
    }
    return dead;
}

// Forward, the lane that finishes (window q, unit u) of step t: publish the new h into set `nxt` under the step's epoch
// (epoch0 + t + 1, formed by the caller, as the backward kernels form theirs: formed in here from epoch0 and t, the same
// arithmetic scheduled differently and gru_fwd's in-situ class time at CPC-large read 0.826-0.835 ms in five alternating
// runs against the parent's 0.801-0.834; formed by the caller, 0.807-0.821).  Padding windows
// (!mine) publish 0, so that every granule of the epoch gets written.  Call it BEFORE the saved activations are stored:
// the other members wait for this store, nobody waits for those.
template <int H, int NB>
__device__ __forceinline__ void coop_fwd_publish(gu64_t *comm, unsigned epoch, int fault, int group, int nxt, int member, int u, int q,
                                                 int t, bool mine, float hv)
{
    if (!(fault && group == 0 && member == 0 && t == 1))
        coop_publish(comm + coop_fwd_slot<H, NB>(group, nxt, member, u, q), epoch, mine ? hv : 0.f);
}

// Forward, all threads: gather the whole new h of the step with this epoch (all members) from set `nxt`; sink(window, k, value) puts it
// into the other LDS buffer, NaN where the wait ran out.  Returns the new `dead`, which stays with the thread that timed
// out.  A thread takes the granules tid, tid + 512, .. of the set: memory order, coalesced.  The caller's
// coop_lds_barrier() follows.
template <int H, int NB, typename Sink>
__device__ __forceinline__ bool coop_fwd_gather(gu64_t *comm, unsigned epoch, int *err, int group, int nxt, bool dead,
                                                Sink &&sink)
{
    constexpr int KP = NB * H / 512 > 0 ? NB * H / 512 : 1;          // granules gathered per thread and step
    const int tid = threadIdx.x;
    if (tid < NB * H) {
        COOP_GLOBAL gu64_t *slot[KP];
#pragma unroll
        for (int i = 0; i < KP; ++i)
            slot[i] = (COOP_GLOBAL gu64_t *)(comm + ((long)group * 2 + nxt) * (NB * H) + (tid + 512 * i));
        gu64_t x[KP];
        dead = coop_poll(slot, epoch, x, dead, err, COOP_ERR_FWD_WAIT);
#pragma unroll
        for (int i = 0; i < KP; ++i) {
            int window, k;
            coop_fwd_who<H, NB>(tid + 512 * i, window, k);
            sink(window, k, dead ? NAN : __uint_as_float((unsigned)x[i]));
        }
    }
    return dead;
}

// Backward granules: [group][set][sender][window][H]; the first granule of a window's row
template <int H, int NB> __device__ __forceinline__ long coop_bwd_row(int group, int par, int sender, int s)
{
    return ((((long)group * 2 + par) * CoopCfg<H>::G + sender) * NB + s) * H;
}

// Backward, all threads: publish the columns of this member's partial W_hh^T dG that other members own (its own stay in
// LDS); column(s, k) reads one of them.
template <int H, int NB, typename Column>
__device__ __forceinline__ void coop_bwd_publish(gu64_t *comm, unsigned epoch, int group, int par, int member, bool dead,
                                                 Column &&column)
{
    for (int idx = threadIdx.x; idx < NB * H; idx += 512) {
        const int s = idx / H, k = idx - s * H;
        if (k / CoopCfg<H>::U == member) continue;
        const float v = column(s, k);
        coop_publish(comm + coop_bwd_row<H, NB>(group, par, member, s) + k, epoch, dead ? NAN : v);
    }
}

// Backward, the elementwise thread of (window es, column ej): wait for the G - 1 partners' pieces and add them to `sum`
// (the thread's own part), in the order they are polled.  Returns the new `dead`; the caller poisons its carry with it.
// `sum` comes in holding the caller's own terms and the pieces are added ONTO it, one by one: float addition does not
// associate, and ((own + x0) + x1) + .. is the order the carry has always been summed in -- returning x0 + x1 + .. for
// the caller to add would change its last bits.
// No barrier is needed behind this: the kernels rewrite dgs before the next step's first barrier and part after it, and
// every thread has finished reading both when it gets there.
template <int H, int NB>
__device__ __forceinline__ bool coop_bwd_collect(gu64_t *comm, unsigned epoch, int *err, int group, int par, int member, int es, int ej,
                                                 bool dead, float &sum)
{
    constexpr int G = CoopCfg<H>::G;
    COOP_GLOBAL gu64_t *slot[G - 1];
#pragma unroll
    for (int d = 1; d < G; ++d)
        slot[d - 1] = (COOP_GLOBAL gu64_t *)(comm + coop_bwd_row<H, NB>(group, par, (member + d) & (G - 1), es) + ej);
    gu64_t x[G - 1];
    dead = coop_poll(slot, epoch, x, dead, err, COOP_ERR_BWD_WAIT);
#pragma unroll
    for (int d = 0; d < G - 1; ++d) sum += __uint_as_float((unsigned)x[d]);
    return dead;
}

}  // namespace cpc
