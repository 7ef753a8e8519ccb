// The recurrence of the local alignment (cpc2_hip.h), in one copy: lalign.hip walks it over distance tiles
// (dtw_strip.h), lalign_units.hip over unit ids (dtw_units_walk.h).  A cell is (H, length, start) with the two start indices in
// one word (items have at most 32767 frames); a closed cell is H = 0 and carries nothing.  Every lane keeps the best cell of its
// own row (strict >: the first column among equals); at the end of a strip the lanes are reduced to (largest H, smallest row)
// and the result replaces the pair's best on a strict > only, so the answer is (largest H, smallest i, smallest j) however
// strips are walked.  Both files are built with -ffp-contract=off (build.py).
#pragma once

#include "dtw_strip.h"

#include <cmath>

namespace cpc {

constexpr int LA_W = 3;                // (H, length, start): 12 bytes per boundary-row column
constexpr int LA_MAX_FRAMES = 32767;   // start_i and start_j share one word: 15 bits each
using LaCell = DtwCell<LA_W>;

struct LaRule {
    float theta, gamma;
    float best_h = 0.f;                // the best cell of this lane's row so far: a closed cell cannot win
    int best_j = -1, best_l = -1, best_s = -1;
    float pair_h = 0.f;                // the same in every lane: the pair's best so far
    int pair_i = -1, pair_j = -1, pair_l = -1, pair_s = -1;

    __device__ __forceinline__ LaCell cell(int gi, int gj, float d, const LaCell &diag, const LaCell &left, const LaCell &up) const
    {
        const float g = theta - d;
        // candidates: diag, left - gamma, up - gamma; one that does not exist cannot be continued
        const float cd = (gi > 0 && gj > 0) ? diag.v : -INFINITY;
        const float cl = gj > 0 ? left.v - gamma : -INFINITY;
        const float cu = gi > 0 ? up.v - gamma : -INFINITY;
        const bool take_d = cd >= cl && cd >= cu, take_l = cl >= cu;     // the largest; ties: diag, then left, then up
        const float b_h = take_d ? cd : take_l ? cl : cu;
        const LaCell b = dtw_pick(take_d, diag, dtw_pick(take_l, left, up));
        // nothing worth continuing: the cell opens a path
        const LaCell c = dtw_pick(b_h <= 0.f, LaCell{g, {1, (gi << 16) | gj}}, LaCell{g + b_h, {b.n[DTW_LEN] + 1, b.n[DTW_START]}});
        return dtw_pick(c.v > 0.f, c, LaCell{});         // closed (also by a NaN distance): carries nothing
    }
    __device__ __forceinline__ void visit(int, int gj, const LaCell &c)
    {
        if (c.v > best_h) {            // strict: the first column among equals (a closed cell is 0 and never wins)
            best_h = c.v;
            best_j = gj;
            best_l = c.n[DTW_LEN];
            best_s = c.n[DTW_START];
        }
    }
    // (largest H, smallest row) over the lanes of the strip; the lanes' bests start afresh for the next strip
    __device__ __forceinline__ void strip_done(int rs, int, bool)
    {
        float m = best_h;
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        const int src = __ffsll((unsigned long long)__ballot(best_h == m)) - 1;
        const int w_j = __shfl(best_j, src), w_l = __shfl(best_l, src), w_s = __shfl(best_s, src);
        if (m > pair_h) {              // strict: the earlier strip wins ties
            pair_h = m;
            pair_i = rs + src;
            pair_j = w_j;
            pair_l = w_l;
            pair_s = w_s;
        }
        best_h = 0.f;
        best_j = best_l = best_s = -1;
    }
};

}  // namespace cpc
