// The recurrence of the subsequence DTW (cpc2_hip.h), in one copy: sdtw.hip walks it over distance tiles
// (dtw_strip.h), sdtw_units.hip over unit ids (dtw_units_walk.h).  Free start on row 0, every cell carries (cost, length, start),
// and the lane of the last query row keeps the best end column while the columns stream.
#pragma once

#include "dtw_strip.h"

namespace cpc {

constexpr int SD_W = 3;            // (cost, length, start): 12 bytes per boundary-row column
using SdCell = DtwCell<SD_W>;

struct SdRule {
    int lq;                        // query frames
    float best_v = 0.f;            // lane of the last query row: the best end column so far
    int best_j = 0, best_l = 0, best_s = 0;

    __device__ __forceinline__ SdCell cell(int gi, int gj, float d, const SdCell &diag, const SdCell &left, const SdCell &up) const
    {
        if (gi == 0) return {d, {1, gj}};                // free start: no predecessor on the first query row
        const SdCell pred = dtw_pick(gj == 0, up, dtw_cheapest(diag, left, up));
        return {d + pred.v, {pred.n[DTW_LEN] + 1, pred.n[DTW_START]}};
    }
    __device__ __forceinline__ void visit(int gi, int gj, const SdCell &c)
    {
        if (gi != lq - 1) return;
        const float v = c.v / (float)c.n[DTW_LEN];       // the last query row: v[j], the first smallest wins
        if (gj == 0 || v < best_v) {
            best_v = v;
            best_j = gj;
            best_l = c.n[DTW_LEN];
            best_s = c.n[DTW_START];
        }
    }
    __device__ __forceinline__ void strip_done(int, int, bool) {}
};

}  // namespace cpc
