// The recurrence of the ABX DTW (cpc2_hip.h), in one copy: abx.hip walks it over distance tiles (dtw_strip.h),
// abx_units.hip over unit ids (dtw_units_walk.h).  Every cell carries (cost, path length); the length follows the reference's
// backtrack tie rule, so no cost matrix and no backtrack are needed.  The rule notes nothing of a cell or a strip and has no
// state.  The unit walk returns the last cell to the lane of the last row, which writes the result; the dense kernel derives a
// rule that writes it from `visit` (abx.hip).  d + 0 is d for every distance but -0, which no frame distance of the dense kernel
// is; the unit kernel has always added the first cell's d to a zero.
#pragma once

#include "dtw_strip.h"

namespace cpc {

constexpr int ABX_W = 2;           // (cost, length): 8 bytes per boundary-row column
using AbxCell = DtwCell<ABX_W>;

struct AbxRule {
    __device__ __forceinline__ AbxCell cell(int gi, int gj, float d, const AbxCell &diag, const AbxCell &left, const AbxCell &up) const
    {
        // first row: left (at (0, 0) the zero cell that both walks hand over: d + 0, length 1); first column: up; else the
        // cheapest, ties to diag, then left, then up.  Two picks on combined conditions, as the unit kernel had them: the
        // conditions meet in scalar masks, where three nested picks cost four more selects in every step.
        const bool take_diag = gi > 0 && gj > 0 && diag.v <= left.v && diag.v <= up.v;
        const bool take_left = gi == 0 || (gj > 0 && left.v <= up.v);
        const AbxCell pred = dtw_pick(take_diag, diag, dtw_pick(take_left, left, up));
        return {d + pred.v, {pred.n[DTW_LEN] + 1}};
    }
    __device__ __forceinline__ void visit(int, int, const AbxCell &) const {}
    __device__ __forceinline__ void strip_done(int, int, bool) const {}
};

}  // namespace cpc
