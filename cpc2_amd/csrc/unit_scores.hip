// Counts that relate quantized units to frame-level phone labels (cpc2_amd/unit_scores.py): the joint table of
// (unit, phone) over frames, the run starts of both streams, and the units' change points matched against the labels' as phone
// boundaries.  Everything is an integer: no floating point on the device, integer sums do not depend on their order, so every
// output EQUALS a numpy statement of the definition on every launch (restated from include/cpc2_hip.h).
//
//   unit_prefix_kernel      one workgroup: the exclusive prefix of the utterances' compared lengths (an utterance whose frames
//                           leave a pack has compared length 0 and its frames are added to `invalid`).  It maps the flat space of
//                           compared frames back to (utterance, frame), so the work is cut by frames and not by utterances.
//   unit_counts_kernel      a fixed grid of workgroups, each taking the chunks c, c + grid, ... of UNIT_CHUNK flat frames.  Lane
//                           after lane holds frame after frame.  Two forms, chosen from the shape alone (unit_form()):
//                             UNIT_FORM_LDS     n_units * n_phones <= UNIT_LDS_CELLS: the whole table lives in LDS as 32-bit
//                                               words, LDS atomics, ONE flush per workgroup of its non-zero cells by 64-bit global
//                                               atomics (and one more every 2^31 frames of a workgroup: the words cannot wrap);
//                             UNIT_FORM_GLOBAL  larger tables: 64-bit atomics on the table in global memory.
//                           In both forms the run-start tables (n_units <= 16384 and n_phones <= 1024 words) live in LDS.
//                           UNIT_LDS_CELLS = 16384: 64 KiB of cells + at most 64 KiB + 4 KiB of run words = 132 KiB of the 160 KiB
//                           a workgroup may take on gfx950, as DYNAMIC LDS sized by the shape: a 50 x 41 table takes 8.4 KiB and
//                           several workgroups share a CU, the largest table takes the CU alone with 512 threads.  No slab of
//                           unit rows: a slab form reads every frame once per slab, and the global form already wins that trade
//                           at 2000 x 41 (DESIGN.md section 24 has the times).
//                           Adjacent lanes very often hit the same cell (a unit run inside a phone): lanes whose cell equals the
//                           lane's before them can be folded into the first lane of their run by one shuffle and one ballot, so
//                           that only that lane adds, the run's length.  Measured: on global atomics the
//                           folding halves the time, on LDS atomics it makes the kernel 38 to 51 % slower.  So the global form
//                           folds and the LDS form does not; UNIT_FORM_PLAIN / UNIT_FORM_FOLD (bits of `form`, for the bench)
//                           force either.
//   unit_boundaries_kernel  one wave per utterance: the change points of both streams are compacted in frame order (ballot +
//                           prefix) into two lists in scratch, then ONE lane runs the two-pointer matching and the lenient counts.
//                           This is the matching of segment.hip's seg_boundaries_kernel, kept here as a SECOND COPY: sharing it
//                           through a header would re-inline it there and that file's code generation is not to move.
// Plain C++ integer atomicAdd on LDS and global words; no float atomic, no inline assembly.
#include "common.h"

namespace cpc {
namespace {

constexpr int UNIT_THREADS = 512;
constexpr int UNIT_CHUNK = 4096;                    // flat frames per chunk of work
constexpr int UNIT_LDS_CELLS = 16384;               // cells of the joint table held in LDS (32-bit words)
constexpr int UNIT_MAX_UNITS = 16384;
constexpr int UNIT_MAX_PHONES = 1024;
constexpr int UNIT_MAX_UTT = 1 << 20;
constexpr int UNIT_MAX_TOL = 1 << 30;
constexpr int UNIT_FLUSH_CHUNKS = (1 << 19);        // 2^19 chunks of 2^12 frames: a 32-bit LDS word is flushed before 2^31
constexpr int UNIT_SCAN_THREADS = 1024;
enum { UNIT_FORM_AUTO = 0, UNIT_FORM_LDS = 1, UNIT_FORM_GLOBAL = 2, UNIT_FORM_PLAIN = 4, UNIT_FORM_FOLD = 8 };

typedef unsigned long long u64;

// the utterance's frames lie inside both packs
__device__ __forceinline__ bool utt_inside(int64_t uo, int64_t lo, int L, long n_unit_words, long n_label_words, bool has_labels)
{
    if (uo < 0 || uo > n_unit_words || (int64_t)L > n_unit_words - uo) return false;
    if (has_labels && (lo < 0 || lo > n_label_words || (int64_t)L > n_label_words - lo)) return false;
    return true;
}

__global__ void __launch_bounds__(UNIT_SCAN_THREADS)
unit_prefix_kernel(const int64_t *__restrict__ unit_off, long n_unit_words, const int64_t *__restrict__ label_off, long n_label_words,
                   bool has_labels, const int *__restrict__ lengths, int u, int64_t *__restrict__ prefix, int64_t *__restrict__ invalid)
{
    __shared__ int64_t s_sum[UNIT_SCAN_THREADS];
    const int tid = threadIdx.x;
    const int per = (u + UNIT_SCAN_THREADS - 1) / UNIT_SCAN_THREADS;
    const int lo = min(tid * per, u), hi = min(lo + per, u);
    int64_t sum = 0, bad = 0;
    for (int i = lo; i < hi; ++i) {
        const int L = lengths[i];
        if (L <= 0) continue;
        if (utt_inside(unit_off[i], has_labels ? label_off[i] : 0, L, n_unit_words, n_label_words, has_labels)) sum += L;
        else bad += L;
    }
    s_sum[tid] = sum;
    __syncthreads();
    for (int d = 1; d < UNIT_SCAN_THREADS; d <<= 1) {                // inclusive scan over the threads
        const int64_t v = tid >= d ? s_sum[tid - d] : 0;
        __syncthreads();
        s_sum[tid] += v;
        __syncthreads();
    }
    int64_t run = s_sum[tid] - sum;
    for (int i = lo; i < hi; ++i) {
        prefix[i] = run;
        const int L = lengths[i];
        if (L > 0 && utt_inside(unit_off[i], has_labels ? label_off[i] : 0, L, n_unit_words, n_label_words, has_labels)) run += L;
    }
    if (tid == UNIT_SCAN_THREADS - 1) prefix[u] = s_sum[tid];
    if (invalid != nullptr && bad != 0) atomicAdd(reinterpret_cast<u64 *>(invalid), (u64)bad);
}

// `key` >= 0 on lanes that count, < 0 on the others.  Returns, on the first lane of a run of equal keys on adjacent lanes, the
// run's length, and 0 on every other lane.  Every lane of the wave calls it.
__device__ __forceinline__ int fold_runs(int key, int lane)
{
    const int before = __shfl_up(key, 1, 64);
    const bool first = key >= 0 && (lane == 0 || before != key);
    const u64 breaks = __ballot(key < 0 || first);
    if (!first) return 0;
    const u64 above = lane == 63 ? 0ull : breaks & ~((2ull << lane) - 1ull);
    return (above != 0ull ? __ffsll((long long)above) - 1 : 64) - lane;
}

template <bool IN_LDS, bool FOLD>
__global__ void __launch_bounds__(UNIT_THREADS)
unit_counts_kernel(const int *__restrict__ units, const int64_t *__restrict__ unit_off, const int *__restrict__ labels,
                   const int64_t *__restrict__ label_off, const int64_t *__restrict__ prefix, int u, int n_units, int n_phones,
                   int64_t *__restrict__ joint, int64_t *__restrict__ unit_runs, int64_t *__restrict__ phone_runs,
                   int64_t *__restrict__ invalid)
{
    extern __shared__ unsigned unit_lds[];                           // [n_units] unit runs | [n_phones] phone runs | IN_LDS: the cells
    unsigned *s_uruns = unit_lds, *s_pruns = unit_lds + n_units, *s_joint = s_pruns + n_phones;
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t total = prefix[u];
    const int64_t n_chunks = (total + UNIT_CHUNK - 1) / UNIT_CHUNK;
    if ((int64_t)blockIdx.x >= n_chunks) return;                     // (the whole workgroup: nothing to zero or flush)
    const int cells = n_units * n_phones;
    const int n_words = n_units + n_phones + (IN_LDS ? cells : 0);
    for (int i = tid; i < n_words; i += UNIT_THREADS) unit_lds[i] = 0u;
    __syncthreads();

    auto flush = [&]() {
        for (int i = tid; i < n_units; i += UNIT_THREADS) {
            const unsigned v = s_uruns[i];
            if (v) atomicAdd(reinterpret_cast<u64 *>(unit_runs) + i, (u64)v);
        }
        for (int i = tid; i < n_phones; i += UNIT_THREADS) {
            const unsigned v = s_pruns[i];
            if (v) atomicAdd(reinterpret_cast<u64 *>(phone_runs) + i, (u64)v);
        }
        if (IN_LDS)
            for (int i = tid; i < cells; i += UNIT_THREADS) {
                const unsigned v = s_joint[i];
                if (v) atomicAdd(reinterpret_cast<u64 *>(joint) + i, (u64)v);
            }
    };

    long long bad = 0;
    int done = 0;
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int64_t g0 = c * UNIT_CHUNK, g1 = min(g0 + UNIT_CHUNK, total);
        int a = 0, b = u;                                            // the last utterance with prefix[i] <= g0: prefix[a] <= g0 < prefix[b]
        while (b - a > 1) {
            const int m = a + (b - a) / 2;
            if (prefix[m] <= g0) a = m; else b = m;
        }
        for (int i = a; i < u; ++i) {
            const int64_t p0 = prefix[i], p1 = prefix[i + 1];
            if (p0 >= g1) break;
            if (p1 <= g0 || p1 == p0) continue;                      // (an utterance of no compared frame)
            const int *un = units + unit_off[i];
            const int *la = labels != nullptr ? labels + label_off[i] : nullptr;
            const int f0 = (int)(max(p0, g0) - p0), f1 = (int)(min(p1, g1) - p0);
            for (int base = f0; base < f1; base += UNIT_THREADS) {   // (uniform over the workgroup: every lane folds)
                const int f = base + tid;
                int cell = -1;
                if (f < f1) {
                    const int z = un[f], y = la != nullptr ? la[f] : 0;
                    if (z < 0 || z >= n_units || y < 0 || y >= n_phones) ++bad;
                    else {
                        cell = z * n_phones + y;
                        if (f == 0 || un[f - 1] != z) atomicAdd(&s_uruns[z], 1u);
                        if (f == 0 || (la != nullptr && la[f - 1] != y)) atomicAdd(&s_pruns[y], 1u);
                    }
                }
                const int n = FOLD ? fold_runs(cell, lane) : (cell >= 0 ? 1 : 0);
                if (n > 0) {
                    if (IN_LDS) atomicAdd(&s_joint[cell], (unsigned)n);
                    else atomicAdd(reinterpret_cast<u64 *>(joint) + cell, (u64)n);
                }
            }
        }
        if (++done == UNIT_FLUSH_CHUNKS) {
            __syncthreads();
            flush();
            __syncthreads();
            for (int i = tid; i < n_words; i += UNIT_THREADS) unit_lds[i] = 0u;
            __syncthreads();
            done = 0;
        }
    }
    __syncthreads();
    flush();
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) bad += __shfl_xor(bad, m, 64);
    if (lane == 0 && bad != 0) atomicAdd(reinterpret_cast<u64 *>(invalid), (u64)bad);
}

__global__ void __launch_bounds__(64)
unit_boundaries_kernel(const int *__restrict__ units, long n_unit_words, const int64_t *__restrict__ unit_off,
                       const int *__restrict__ labels, long n_label_words, const int64_t *__restrict__ label_off,
                       const int *__restrict__ lengths, const int64_t *__restrict__ prefix, long total_frames, int tol,
                       int *__restrict__ hyp_all, int *__restrict__ ref_all, int *__restrict__ out)
{
    const int utt = blockIdx.x, lane = threadIdx.x;
    int *o = out + (size_t)utt * 5;
    const int L = lengths[utt];
    const bool has_labels = labels != nullptr;
    if (L <= 1) {                                                    // (a negative length as well: nothing of it is read)
        if (lane < 5) o[lane] = 0;
        return;
    }
    const int64_t slot = prefix[utt];
    // an utterance whose frames leave a pack (compared length 0 in the prefix), or whose lists would leave the room the caller
    // gave (total_frames below the sum of the lengths): five times -1, nothing of it read
    if (prefix[utt + 1] - slot != (int64_t)L || slot + L > (int64_t)total_frames) {
        if (lane < 5) o[lane] = -1;
        return;
    }
    const int *un = units + unit_off[utt];
    const int *la = has_labels ? labels + label_off[utt] : nullptr;
    int *hyp = hyp_all + slot, *refs = ref_all + slot;
    int n_hyp = 0, n_ref = 0;
    const u64 below = (1ull << lane) - 1ull;
    for (int base = 1; base < L; base += 64) {                       // change points in frame order
        const int f = base + lane;
        const bool h = f < L && un[f] != un[f - 1];
        const bool r = f < L && has_labels && la[f] != la[f - 1];
        const u64 mh = __ballot(h), mr = __ballot(r);
        if (h) hyp[n_hyp + __popcll(mh & below)] = f;
        if (r) refs[n_ref + __popcll(mr & below)] = f;
        n_hyp += __popcll(mh);
        n_ref += __popcll(mr);
    }
    __syncthreads();                                                 // (orders the wave's global writes of the lists before its reads)
    if (lane == 0) {
        const long long tl = tol;
        int hits = 0, hyp_near = 0, ref_near = 0;
        int im = 0, ia = 0, ib = 0;                                  // the matching's, hyp_near's and ref_near's reference pointers
        for (int j = 0; j < n_hyp; ++j) {
            const long long h = hyp[j];
            while (im < n_ref) {
                const long long r = refs[im];
                const long long gap = h > r ? h - r : r - h;
                if (gap <= tl) { ++hits; ++im; break; }
                if (h < r) break;
                ++im;
            }
            while (ia < n_ref && refs[ia] < h - tl) ++ia;
            if (ia < n_ref && refs[ia] <= h + tl) ++hyp_near;
            while (ib < n_ref && refs[ib] < h - tl) ++ib;
            while (ib < n_ref && refs[ib] <= h + tl) { ++ref_near; ++ib; }
        }
        o[0] = n_ref;
        o[1] = n_hyp;
        o[2] = hits;
        o[3] = hyp_near;
        o[4] = ref_near;
    }
}

int unit_form(int n_units, int n_phones) { return (long)n_units * n_phones <= UNIT_LDS_CELLS ? UNIT_FORM_LDS : UNIT_FORM_GLOBAL; }

bool unit_sizes_ok(const char *who, int n_utt, int n_units, int n_phones, bool has_labels)
{
    if (n_utt < 0 || n_utt > UNIT_MAX_UTT || n_units < 1 || n_units > UNIT_MAX_UNITS || n_phones < 1 || n_phones > UNIT_MAX_PHONES) {
        set_error("%s: sizes outside the supported limits (n_utt=%d n_units=%d n_phones=%d; need 0 <= n_utt <= %d, 1 <= n_units <= %d, "
                  "1 <= n_phones <= %d)", who, n_utt, n_units, n_phones, UNIT_MAX_UTT, UNIT_MAX_UNITS, UNIT_MAX_PHONES);
        return false;
    }
    if (!has_labels && n_phones != 1) {
        set_error("%s: labels == NULL means every frame has label 0: n_phones must be 1 (got %d)", who, n_phones);
        return false;
    }
    return true;
}

template <bool IN_LDS, bool FOLD>
int launch_counts(unsigned grid, size_t lds, hipStream_t st, const int *units, const int64_t *unit_off, const int *labels,
                  const int64_t *label_off, const int64_t *prefix, int u, int n_units, int n_phones, int64_t *joint,
                  int64_t *unit_runs, int64_t *phone_runs, int64_t *invalid)
{
    auto kern = unit_counts_kernel<IN_LDS, FOLD>;
    if (lds > 64 * 1024)
        CPC_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(UNIT_THREADS), lds, st, units, unit_off, labels, label_off, prefix, u, n_units, n_phones,
                       joint, unit_runs, phone_runs, invalid);
    CPC_CHECK_LAUNCH("unit_counts_kernel");
    return CPC_OK;
}

}  // namespace
}  // namespace cpc

extern "C" int cpc_unit_counts_lds_cells(void) { return cpc::UNIT_LDS_CELLS; }
extern "C" int cpc_unit_counts_chunk(void) { return cpc::UNIT_CHUNK; }

extern "C" size_t cpc_unit_counts_scratch_bytes(int n_utt)
{
    if (n_utt < 0 || n_utt > cpc::UNIT_MAX_UTT) {
        cpc::set_error("unit_counts: n_utt=%d outside 0 .. %d", n_utt, cpc::UNIT_MAX_UTT);
        return 0;
    }
    cpc::Carver c(nullptr);
    c.take<int64_t>((size_t)n_utt + 1);
    return c.used();
}

extern "C" int cpc_unit_counts(const int *units, long n_unit_words, const int64_t *unit_off, const int *labels, long n_label_words,
                               const int64_t *label_off, const int *lengths, int n_utt, int n_units, int n_phones, int form,
                               int64_t *joint, int64_t *unit_runs, int64_t *phone_runs, int64_t *invalid, void *scratch,
                               size_t scratch_bytes, cpc_stream_t stream)
{
    if (!cpc::unit_sizes_ok("unit_counts", n_utt, n_units, n_phones, labels != nullptr)) return CPC_ERR_INVALID;
    CPC_REQUIRE(n_unit_words >= 0 && n_label_words >= 0, "unit_counts: negative pack size (n_unit_words=%ld n_label_words=%ld)",
                n_unit_words, n_label_words);
    const int base = form & 3, folding = form & (cpc::UNIT_FORM_PLAIN | cpc::UNIT_FORM_FOLD);
    CPC_REQUIRE(form >= 0 && form < 16 && base <= cpc::UNIT_FORM_GLOBAL && folding != (cpc::UNIT_FORM_PLAIN | cpc::UNIT_FORM_FOLD),
                "unit_counts: form=%d is none of 0 (by shape), 1 (LDS), 2 (global), each + 4 (equal adjacent cells are not folded) "
                "or + 8 (they are)", form);
    const int chosen = base == cpc::UNIT_FORM_AUTO ? cpc::unit_form(n_units, n_phones) : base;
    CPC_REQUIRE(chosen != cpc::UNIT_FORM_LDS || (long)n_units * n_phones <= cpc::UNIT_LDS_CELLS,
                "unit_counts: form=1 (LDS) needs n_units * n_phones <= %d (got %d x %d)", cpc::UNIT_LDS_CELLS, n_units, n_phones);
    if (n_utt == 0) return CPC_OK;
    CPC_REQUIRE(units && unit_off && lengths && joint && unit_runs && phone_runs && invalid && (labels == nullptr || label_off),
                "unit_counts: null buffer");
    CPC_REQUIRE(scratch != nullptr, "unit_counts: null scratch");
    if (scratch_bytes < cpc_unit_counts_scratch_bytes(n_utt)) {
        cpc::set_error("unit_counts: scratch of %zu bytes, cpc_unit_counts_scratch_bytes(%d) = %zu", scratch_bytes, n_utt,
                       cpc_unit_counts_scratch_bytes(n_utt));
        return CPC_ERR_WORKSPACE;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    cpc::Carver c(scratch);
    int64_t *prefix = c.take<int64_t>((size_t)n_utt + 1);
    hipLaunchKernelGGL(cpc::unit_prefix_kernel, dim3(1), dim3(cpc::UNIT_SCAN_THREADS), 0, st, unit_off, n_unit_words, label_off,
                       n_label_words, labels != nullptr, lengths, n_utt, prefix, invalid);
    CPC_CHECK_LAUNCH("unit_prefix_kernel");
    const bool in_lds = chosen == cpc::UNIT_FORM_LDS;
    const bool fold = folding == 0 ? !in_lds : folding == cpc::UNIT_FORM_FOLD;      // (by default: what was measured to be faster)
    const size_t lds = sizeof(unsigned) * ((size_t)n_units + n_phones + (in_lds ? (size_t)n_units * n_phones : 0));
    int dev = 0, cus = 0;
    CPC_CHECK_HIP(hipGetDevice(&dev));
    CPC_CHECK_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    // as many workgroups as are resident at once: by LDS, and 2048 threads a CU
    const size_t by_lds = (160 * 1024) / (lds > 1024 ? lds : 1024);
    const unsigned per_cu = (unsigned)(by_lds < 1 ? 1 : by_lds > 4 ? 4 : by_lds);
    const unsigned grid = (unsigned)(cus > 0 ? cus : 1) * per_cu;
#define CPC_UNIT_LAUNCH(L, F)                                                                                                    \
    cpc::launch_counts<L, F>(grid, lds, st, units, unit_off, labels, label_off, prefix, n_utt, n_units, n_phones, joint, unit_runs, \
                             phone_runs, invalid)
    if (in_lds) return fold ? CPC_UNIT_LAUNCH(true, true) : CPC_UNIT_LAUNCH(true, false);
    return fold ? CPC_UNIT_LAUNCH(false, true) : CPC_UNIT_LAUNCH(false, false);
#undef CPC_UNIT_LAUNCH
}

extern "C" size_t cpc_unit_boundaries_scratch_bytes(int n_utt, long total_frames)
{
    if (n_utt < 0 || n_utt > cpc::UNIT_MAX_UTT || total_frames < 0) {
        cpc::set_error("unit_boundaries: sizes outside the supported limits (n_utt=%d total_frames=%ld; need 0 <= n_utt <= %d, "
                       "total_frames >= 0)", n_utt, total_frames, cpc::UNIT_MAX_UTT);
        return 0;
    }
    cpc::Carver c(nullptr);
    c.take<int64_t>((size_t)n_utt + 1);
    c.take<int>((size_t)total_frames + 1);
    c.take<int>((size_t)total_frames + 1);
    return c.used();
}

extern "C" int cpc_unit_boundaries(const int *units, long n_unit_words, const int64_t *unit_off, const int *labels, long n_label_words,
                                   const int64_t *label_off, const int *lengths, int n_utt, long total_frames, int tol, int *out,
                                   void *scratch, size_t scratch_bytes, cpc_stream_t stream)
{
    CPC_REQUIRE(n_utt >= 0 && n_utt <= cpc::UNIT_MAX_UTT && total_frames >= 0 && n_unit_words >= 0 && n_label_words >= 0 && tol >= 0 &&
                    tol <= cpc::UNIT_MAX_TOL,
                "unit_boundaries: sizes outside the supported limits (n_utt=%d total_frames=%ld n_unit_words=%ld n_label_words=%ld "
                "tol=%d; need 0 <= n_utt <= %d, the sizes >= 0, 0 <= tol <= %d)", n_utt, total_frames, n_unit_words, n_label_words, tol,
                cpc::UNIT_MAX_UTT, cpc::UNIT_MAX_TOL);
    if (n_utt == 0) return CPC_OK;
    CPC_REQUIRE(units && unit_off && lengths && out && (labels == nullptr || label_off), "unit_boundaries: null buffer");
    CPC_REQUIRE(scratch != nullptr, "unit_boundaries: null scratch");
    if (scratch_bytes < cpc_unit_boundaries_scratch_bytes(n_utt, total_frames)) {
        cpc::set_error("unit_boundaries: scratch of %zu bytes, cpc_unit_boundaries_scratch_bytes(%d, %ld) = %zu", scratch_bytes, n_utt,
                       total_frames, cpc_unit_boundaries_scratch_bytes(n_utt, total_frames));
        return CPC_ERR_WORKSPACE;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    cpc::Carver c(scratch);
    int64_t *prefix = c.take<int64_t>((size_t)n_utt + 1);
    int *hyp = c.take<int>((size_t)total_frames + 1);
    int *ref = c.take<int>((size_t)total_frames + 1);
    hipLaunchKernelGGL(cpc::unit_prefix_kernel, dim3(1), dim3(cpc::UNIT_SCAN_THREADS), 0, st, unit_off, n_unit_words, label_off,
                       n_label_words, labels != nullptr, lengths, n_utt, prefix, static_cast<int64_t *>(nullptr));
    CPC_CHECK_LAUNCH("unit_prefix_kernel");
    hipLaunchKernelGGL(cpc::unit_boundaries_kernel, dim3((unsigned)n_utt), dim3(64), 0, st, units, n_unit_words, unit_off, labels,
                       n_label_words, label_off, lengths, prefix, total_frames, tol, hyp, ref, out);
    CPC_CHECK_LAUNCH("unit_boundaries_kernel");
    return CPC_OK;
}
