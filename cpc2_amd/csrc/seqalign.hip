// Phone error rate of a CTC probe (cpc/criterion/seq_alignment.py of the reference; cpc2_amd/seq_alignment.py):
//   beam_search_kernel   the CTC prefix beam search (seq_alignment.py:11-61), one workgroup per sequence, frames in sequence.
//   align_score_kernel   NeedlemanWunschAlignScore (seq_alignment.py:89-112), one wave64 per pair, integer arithmetic.
//
// The search does the reference's arithmetic operation for operation in f32 (numpy float32 scalars there): every product and
// sum below is written as __fmul_rn / __fadd_rn and the file is built with -ffp-contract=off (cpc2_amd/build.py: hipcc's default
// fuses a product with the sum behind it whatever the source says), and f32 subnormals are kept (hipcc's default kernel mode; scores at 128 frames reach 1e-40).  Every accumulator of the reference receives at most two addends, and a
// two-term f32 sum does not depend on the order of its terms, so the result equals the reference's bit for bit.
//
// Prefixes are nodes of a per-sequence trie in scratch: node = (parent node, symbol), found through an open-addressed table keyed
// by parent * 128 + symbol, so a label string is one node whichever route produced it and however often it left the beam.  A
// node is created only for a survivor of a frame and takes the number 1 + frame * nKeep + (its rank in that frame's beam): no
// counter that racing threads share, and node numbers never take part in a comparison of scores.
//
// A frame's candidates live in a [beam rank][symbol] array in LDS: slot (i, c) is prefix i extended by c, slot (i, blank) is
// prefix i itself (the reference's "stay").  An extension whose string already is in the beam is folded into that entry's slot,
// as the reference's dictionaries do.  The new beam is the nKeep largest scores -- a radix select over the f32 bit patterns
// (scores are non-negative, so the patterns order like the values), most significant byte first, that stops as soon as a byte
// separates the nKeep-th from the (nKeep + 1)-th -- ordered by score, and among EQUAL scores by slot number (rank of the parent
// in the previous beam, then the symbol, the blank standing for the prefix itself).  The reference orders equal scores by the
// prefixes' decimal strings instead; that order is not reproduced.  ties[n] tells whether any frame of sequence n met equal
// scores among its first nKeep + 1 candidates.
#include "common.h"

#include <algorithm>
#include <climits>

namespace cpc {
namespace {

constexpr int BS_MAX_KEEP = 128;
constexpr int BS_MAX_P = 128;
constexpr int BS_MAX_T = 8192;
constexpr int BS_MAX_THREADS = 1024;
constexpr unsigned long long BS_EMPTY = ~0ull;
constexpr int AL_MAX_LEN = 4096;
constexpr int AL_MAX_COST = 1 << 15;

struct BeamGeom {
    int log_table;          // the (parent, symbol) -> node table of a sequence holds 1 << log_table entries
    size_t nodes;           // 1 + t_max * n_keep
    size_t table_bytes, total_bytes;
};

static BeamGeom beam_geom(int n, int t_max, int n_keep)
{
    BeamGeom g;
    g.nodes = 1 + (size_t)t_max * n_keep;
    g.log_table = 1;
    while (((size_t)1 << g.log_table) < 2 * g.nodes) ++g.log_table;       // at most half full: a probe sequence always ends
    g.table_bytes = align_up(((size_t)n << g.log_table) * sizeof(unsigned long long), 256);
    g.total_bytes = g.table_bytes + align_up((size_t)n * g.nodes * sizeof(unsigned), 256);
    return g;
}

__device__ __forceinline__ int wave_incl_sum(int v, int lane)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(v, off, 64);
        if (lane >= off) v += o;
    }
    return v;
}

// One workgroup per sequence.  keys[i * P + c]: 1 + the f32 bits of the candidate's score, 0 for a slot that holds no candidate.
__global__ void __launch_bounds__(BS_MAX_THREADS)
beam_search_kernel(const float *__restrict__ probs, const int *__restrict__ lengths, int t_max, int P, int n_keep, int blank,
                   int rows_out, unsigned long long *__restrict__ tables, int log_table, unsigned *__restrict__ node_keys,
                   size_t nodes, float *__restrict__ scores, int *__restrict__ out_len, int *__restrict__ labels,
                   int *__restrict__ counts, int *__restrict__ ties)
{
    extern __shared__ unsigned keys[];                      // [n_keep * P]
    __shared__ float sp[BS_MAX_P];                          // the frame's probabilities
    __shared__ int b_node[2][BS_MAX_KEEP], b_par[2][BS_MAX_KEEP], b_sym[2][BS_MAX_KEEP], b_len[2][BS_MAX_KEEP];
    __shared__ float b_pb[2][BS_MAX_KEEP], b_pnb[2][BS_MAX_KEEP];
    __shared__ int b_prank[BS_MAX_KEEP];                    // rank of the entry's parent string in the beam, -1: not in it
    __shared__ float f_tot[BS_MAX_KEEP], f_pb[BS_MAX_KEEP], f_pnb[BS_MAX_KEEP];
    __shared__ unsigned hist[256];
    __shared__ unsigned sel_key[BS_MAX_KEEP], sorted_key[BS_MAX_KEEP];
    __shared__ int sel_slot[BS_MAX_KEEP];
    __shared__ int wave_count[BS_MAX_THREADS / 64];
    __shared__ unsigned s_prefix;
    __shared__ int s_remaining, s_done, s_boundary, s_count, s_merged, s_tie;

    const int n = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, wave = tid >> 6, nwaves = nthr >> 6;
    const float *pr = probs + (size_t)n * t_max * P;
    unsigned long long *table = tables + ((size_t)n << log_table);
    const unsigned table_mask = (1u << log_table) - 1u;
    unsigned *nkey = node_keys + (size_t)n * nodes;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int L = min(max(lengths[n], 0), t_max);

    if (tid == 0) {
        b_node[0][0] = 0; b_par[0][0] = -1; b_sym[0][0] = -1; b_len[0][0] = 0;
        b_pb[0][0] = 1.f; b_pnb[0][0] = 0.f;
        b_prank[0] = -1;
        s_merged = 0; s_tie = 0;
    }
    for (int i = tid; i < BS_MAX_KEEP; i += nthr) { sel_key[i] = 0u; sel_slot[i] = 0; }
    __syncthreads();
    int K = 1, cur = 0;

    for (int t = 0; t < L; ++t) {
        const int nxt = cur ^ 1;
        for (int c = tid; c < P; c += nthr) sp[c] = pr[(size_t)t * P + c];
        if (tid < K) f_tot[tid] = __fadd_rn(b_pb[cur][tid], b_pnb[cur][tid]);
        __syncthreads();
        // the prefix itself: pb' = (pnb + pb) p[blank]; pnb' = pnb p[last] (+ the extension of its parent when that is in the beam)
        if (tid < K) {
            const int s = b_sym[cur][tid], q = b_prank[tid];
            float st = s >= 0 ? __fmul_rn(b_pnb[cur][tid], sp[s]) : 0.f;
            if (q >= 0) st = __fadd_rn(st, __fmul_rn(b_sym[cur][q] == s ? b_pb[cur][q] : f_tot[q], sp[s]));
            f_pnb[tid] = st;
            f_pb[tid] = __fmul_rn(f_tot[tid], sp[blank]);
        }
        if (tid == 0) { s_count = 0; s_done = 0; s_boundary = 0; }
        __syncthreads();
        const int n_cand = K * P;
        const int n_valid = n_cand - s_merged;
        for (int s = tid; s < n_cand; s += nthr) {
            const int i = s / P, c = s - i * P;
            const float v = c == blank ? __fadd_rn(f_pb[i], f_pnb[i])
                                       : __fmul_rn(c == b_sym[cur][i] ? b_pb[cur][i] : f_tot[i], sp[c]);
            const unsigned u = __float_as_uint(v);
            keys[s] = u == 0xffffffffu ? u : u + 1u;
        }
        __syncthreads();
        if (tid < K && b_prank[tid] >= 0) keys[b_prank[tid] * P + b_sym[cur][tid]] = 0u;      // folded into slot (tid, blank)
        __syncthreads();

        // ---- the new beam's size and the key of its last member
        const int k_new = min(n_keep, n_valid);
        int shift = 0;
        unsigned prefix = 1u;                         // all candidates: every key >= 1
        bool boundary = false;                        // equal keys on both sides of the cut
        int remaining = 0;
        if (n_valid > n_keep) {
            remaining = n_keep;
            prefix = 0u;
            for (shift = 24; ; shift -= 8) {
                for (int b = tid; b < 256; b += nthr) hist[b] = 0u;
                __syncthreads();
                for (int s = tid; s < n_cand; s += nthr) {
                    const unsigned k = keys[s];
                    if (shift == 24 || (k >> (shift + 8)) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1u);
                }
                __syncthreads();
                if (wave == 0) {                      // lane l: bins 255 - 4 l down to 252 - 4 l
                    int c4[4], sum = 0;
#pragma unroll
                    for (int q = 0; q < 4; ++q) { c4[q] = (int)hist[255 - 4 * lane - q]; sum += c4[q]; }
                    const int incl = wave_incl_sum(sum, lane);
                    int above = incl - sum;
                    if (above < remaining && remaining <= incl) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            if (above < remaining && remaining <= above + c4[q]) {
                                s_prefix = (prefix << 8) | (unsigned)(255 - 4 * lane - q);
                                s_remaining = remaining - above;
                                s_done = c4[q] == remaining - above;
                                s_boundary = shift == 0 && c4[q] > remaining - above;
                                above = INT_MAX / 2;
                            } else {
                                above += c4[q];
                            }
                        }
                    }
                }
                __syncthreads();
                prefix = s_prefix;
                remaining = s_remaining;
                boundary = s_boundary != 0;
                const bool done = s_done != 0;
                if (done || shift == 0) break;
            }
        }

        // ---- gather the members (any order: they are ranked below)
        for (int s0 = 0; s0 < n_cand; s0 += nthr) {
            const int s = s0 + tid;
            const unsigned k = s < n_cand ? keys[s] : 0u;
            const bool take = s < n_cand && (boundary ? k > prefix : (k >> shift) >= prefix);
            const unsigned long long mask = __ballot(take);
            int base = 0;
            if (lane == 0 && mask) base = atomicAdd(&s_count, __popcll(mask));
            base = __shfl(base, 0, 64);
            const int pos = base + __popcll(mask & below);
            if (take && pos < BS_MAX_KEEP) { sel_key[pos] = k; sel_slot[pos] = s; }
        }
        if (boundary) {
            // more candidates carry the last member's score than fit: the first `remaining` of them in slot order
            __syncthreads();
            int placed = 0;
            const int first = k_new - remaining;
            for (int s0 = 0; s0 < n_cand && placed < remaining; s0 += nthr) {
                const int s = s0 + tid;
                const bool eq = s < n_cand && keys[s] == prefix;
                const unsigned long long mask = __ballot(eq);
                if (lane == 0) wave_count[wave] = __popcll(mask);
                __syncthreads();
                int before = placed, total = 0;
                for (int w = 0; w < nwaves; ++w) {
                    const int cw = wave_count[w];
                    if (w < wave) before += cw;
                    total += cw;
                }
                const int pos = before + __popcll(mask & below);
                if (eq && pos < remaining) { sel_key[first + pos] = prefix; sel_slot[first + pos] = s; }
                placed += total;
                __syncthreads();
            }
        }
        __syncthreads();

        // ---- rank the members (score down, slot up) and write the new beam
        if (tid < k_new) {
            const unsigned k = sel_key[tid];
            const int s = sel_slot[tid];
            int r = 0;
            for (int m = 0; m < k_new; ++m) {
                const unsigned km = sel_key[m];
                r += (km > k || (km == k && sel_slot[m] < s)) ? 1 : 0;
            }
            sorted_key[r] = k;
            const int i = s / P, c = s - i * P;
            if (c == blank) {
                b_node[nxt][r] = b_node[cur][i]; b_par[nxt][r] = b_par[cur][i]; b_sym[nxt][r] = b_sym[cur][i];
                b_len[nxt][r] = b_len[cur][i];
                b_pb[nxt][r] = f_pb[i]; b_pnb[nxt][r] = f_pnb[i];
            } else {
                const int parent = b_node[cur][i];
                const unsigned key = (unsigned)parent * BS_MAX_P + (unsigned)c;
                const unsigned fresh = 1u + (unsigned)t * n_keep + r;
                const unsigned long long want = ((unsigned long long)key << 32) | fresh;
                unsigned h = (key * 2654435761u) >> (32 - log_table);
                unsigned node = fresh;
                for (unsigned probe = 0; probe <= table_mask; ++probe) {
                    const unsigned long long prev = atomicCAS(&table[h], BS_EMPTY, want);
                    if (prev == BS_EMPTY) { nkey[fresh] = key; break; }
                    if ((unsigned)(prev >> 32) == key) { node = (unsigned)prev; break; }
                    h = (h + 1u) & table_mask;
                }
                b_node[nxt][r] = (int)node; b_par[nxt][r] = parent; b_sym[nxt][r] = c;
                b_len[nxt][r] = b_len[cur][i] + 1;
                b_pb[nxt][r] = 0.f; b_pnb[nxt][r] = __uint_as_float(k - 1u);
            }
        }
        if (tid == 0) s_merged = 0;
        __syncthreads();
        if (tid < k_new) {
            const int parent = b_par[nxt][tid];
            int q = -1;
            for (int m = 0; m < k_new; ++m) q = b_node[nxt][m] == parent ? m : q;
            b_prank[tid] = q;
            if (q >= 0) atomicAdd(&s_merged, 1);
            if ((tid + 1 < k_new && sorted_key[tid] == sorted_key[tid + 1]) || (tid == 0 && boundary)) s_tie = 1;
        }
        K = k_new;
        cur = nxt;
        __syncthreads();
    }

    // ---- results: rows_out prefixes per sequence, best first
    const int kept = min(K, rows_out);
    float *sc = scores + (size_t)n * rows_out;
    int *ol = out_len + (size_t)n * rows_out;
    int *lb = labels + (size_t)n * rows_out * t_max;
    for (int r = tid; r < rows_out; r += nthr) {
        sc[r] = r < kept ? __fadd_rn(b_pb[cur][r], b_pnb[cur][r]) : 0.f;
        ol[r] = r < kept ? b_len[cur][r] : 0;
    }
    for (int x = tid; x < rows_out * t_max; x += nthr) {
        const int r = x / t_max, k = x - r * t_max;
        if (r >= kept || k >= b_len[cur][r]) lb[x] = -1;
    }
    if (tid < kept) {
        int node = b_node[cur][tid];
        for (int k = min(b_len[cur][tid], t_max) - 1; k >= 0 && (size_t)node < nodes; --k) {
            const unsigned key = nkey[node];
            lb[(size_t)tid * t_max + k] = (int)(key & (BS_MAX_P - 1));
            node = (int)(key / BS_MAX_P);
        }
    }
    if (tid == 0) { counts[n] = kept; ties[n] = s_tie; }
}

// One wave per pair.  Row i + 1 of the table from row i: H[i+1][j] = max(A[j], H[i+1][j-1] + d) with
// A[j] = max(H[i][j-1] + (match or mismatch), H[i][j] + d), i.e. H[i+1][j] - j d = the running maximum of A[k] - k d over k <= j
// (k = 0 standing for H[i+1][0] = (i + 1) d): a prefix maximum over the wave, carried from one 64-column strip to the next.
__global__ void __launch_bounds__(64)
align_score_kernel(const int *__restrict__ seq1, long ld1, const int *__restrict__ len1, const int *__restrict__ seq2, long ld2,
                   const int *__restrict__ len2, int d, int m, int r, int *__restrict__ out)
{
    __shared__ int row[AL_MAX_LEN + 1];
    const int pair = blockIdx.x, lane = threadIdx.x;
    const int n1 = min(max(len1[pair], 0), (int)min(ld1, (long)AL_MAX_LEN));
    const int n2 = min(max(len2[pair], 0), (int)min(ld2, (long)AL_MAX_LEN));
    const int *a = seq1 + (size_t)pair * ld1, *b = seq2 + (size_t)pair * ld2;
    for (int j = lane; j <= n2; j += 64) row[j] = j * d;
    __syncthreads();
    for (int i = 0; i < n1; ++i) {
        const int ai = a[i];
        int diag0 = row[0];                                 // H[i][j0 - 1] of the strip's first column
        int carry = (i + 1) * d;                            // the running maximum so far
        __syncthreads();
        if (lane == 0) row[0] = (i + 1) * d;
        for (int j0 = 1; j0 <= n2; j0 += 64) {
            const int j = j0 + lane;
            const bool valid = j <= n2;
            const int up = valid ? row[j] : 0;
            int dg = valid && lane > 0 ? row[j - 1] : 0;
            if (lane == 0) dg = diag0;
            int g = INT_MIN / 2;
            if (valid) g = max(dg + (ai == b[j - 1] ? r : m), up + d) - j * d;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int o = __shfl_up(g, off, 64);
                if (lane >= off) g = max(g, o);
            }
            g = max(g, carry);
            carry = __shfl(g, 63, 64);
            diag0 = __shfl(up, 63, 64);
            __syncthreads();
            if (valid) row[j] = g + j * d;
        }
        __syncthreads();
    }
    if (lane == 0) out[pair] = -row[n2];
}

}  // namespace
}  // namespace cpc

static int beam_check(const char *what, int n, int t_max, int p, int n_keep)
{
    CPC_REQUIRE(n >= 1 && t_max >= 1, "%s: needs at least one sequence and one frame (n=%d t_max=%d)", what, n, t_max);
    CPC_REQUIRE(t_max <= cpc::BS_MAX_T, "%s: t_max=%d is beyond the limit of %d frames", what, t_max, cpc::BS_MAX_T);
    CPC_REQUIRE(n_keep >= 1 && n_keep <= cpc::BS_MAX_KEEP, "%s: nKeep=%d is outside [1, %d] (a frame's candidates are held in LDS)",
                what, n_keep, cpc::BS_MAX_KEEP);
    CPC_REQUIRE(p >= 2 && p <= cpc::BS_MAX_P, "%s: P=%d classes is outside [2, %d] (a frame's candidates are held in LDS)", what, p,
                cpc::BS_MAX_P);
    return CPC_OK;
}

extern "C" size_t cpc_ctc_beam_search_scratch_bytes(int n, int t_max, int p, int n_keep)
{
    if (beam_check("ctc_beam_search", n, t_max, p, n_keep) != CPC_OK) return 0;
    return cpc::beam_geom(n, t_max, n_keep).total_bytes;
}

extern "C" int cpc_ctc_beam_search(const float *probs, const int *lengths, int n, int t_max, int p, int n_keep, int blank,
                                   int best_only, float *scores, int *out_lengths, int *labels, int *counts, int *ties,
                                   void *scratch, size_t scratch_bytes, cpc_stream_t stream)
{
    CPC_TRY(beam_check("ctc_beam_search", n, t_max, p, n_keep));
    CPC_REQUIRE(blank >= 0 && blank < p, "ctc_beam_search: blank=%d is outside [0, P=%d)", blank, p);
    CPC_REQUIRE(probs && lengths && scores && out_lengths && labels && counts && ties && scratch, "ctc_beam_search: null buffer");
    const cpc::BeamGeom g = cpc::beam_geom(n, t_max, n_keep);
    if (scratch_bytes < g.total_bytes) {
        cpc::set_error("ctc_beam_search: scratch of %zu B given, %zu B needed", scratch_bytes, g.total_bytes);
        return CPC_ERR_WORKSPACE;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    CPC_CHECK_HIP(hipMemsetAsync(scratch, 0xff, g.table_bytes, st));                  // every table entry empty
    const int cand = n_keep * p;
    const int threads = cand <= 2048 ? 256 : (cand <= 8192 ? 512 : 1024);
    const size_t lds = sizeof(unsigned) * (size_t)cand;
    if (lds > 48 * 1024)
        CPC_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(cpc::beam_search_kernel),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(cpc::beam_search_kernel, dim3((unsigned)n), dim3((unsigned)threads), lds, st, probs, lengths, t_max, p, n_keep,
                       blank, best_only ? 1 : n_keep, static_cast<unsigned long long *>(scratch), g.log_table,
                       reinterpret_cast<unsigned *>(static_cast<char *>(scratch) + g.table_bytes), g.nodes, scores, out_lengths,
                       labels, counts, ties);
    CPC_CHECK_LAUNCH("beam_search_kernel");
    return CPC_OK;
}

extern "C" int cpc_align_score(const int *seq1, long ld1, const int *len1, const int *seq2, long ld2, const int *len2, int n,
                               int d, int m, int r, int *score, cpc_stream_t stream)
{
    CPC_REQUIRE(n >= 1 && ld1 >= 1 && ld2 >= 1, "align_score: needs at least one pair and one column per matrix (n=%d ld1=%ld ld2=%ld)",
                n, ld1, ld2);
    CPC_REQUIRE(ld1 <= cpc::AL_MAX_LEN && ld2 <= cpc::AL_MAX_LEN, "align_score: sequences of up to %d labels (ld1=%ld ld2=%ld)",
                cpc::AL_MAX_LEN, ld1, ld2);
    CPC_REQUIRE(std::abs(d) <= cpc::AL_MAX_COST && std::abs(m) <= cpc::AL_MAX_COST && std::abs(r) <= cpc::AL_MAX_COST,
                "align_score: costs of magnitude up to %d (d=%d m=%d r=%d)", cpc::AL_MAX_COST, d, m, r);
    CPC_REQUIRE(seq1 && len1 && seq2 && len2 && score, "align_score: null buffer");
    hipLaunchKernelGGL(cpc::align_score_kernel, dim3((unsigned)n), dim3(64), 0, static_cast<hipStream_t>(stream), seq1, ld1, len1,
                       seq2, ld2, len2, d, m, r, score);
    CPC_CHECK_LAUNCH("align_score_kernel");
    return CPC_OK;
}
