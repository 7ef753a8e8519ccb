// The 64 x 64 frame-distance tile of the DTW kernels that stream a row item against column items (sdtw.hip, lalign.hip): staging,
// the register-blocked products and the acos / sqrt finish, in one copy.  A workgroup of DTW_THREADS threads forms the tile in LDS:
// each thread owns a 4 x 4 block of it and reads the staged frames TRANSPOSED ([k][row]), one 16-byte LDS read per operand and k
// for 16 FMAs; every entry is still its own k-ordered f32 fma chain, bit for bit the frame distance of cpc_abx_dtw.  The next
// chunk's frames travel from global memory while this chunk is multiplied.  (abx.hip keeps its own tile: one thread per entry of
// a 64 x 64 tile whose rows are not transposed, a different shape.)
#pragma once

#include "dtw_strip.h"

namespace cpc {

constexpr int SD_KC = 32;          // feature chunk staged in LDS per pass
constexpr int SD_LS = DTW_T + 4;   // row stride of the transposed staging tiles: 16-byte aligned rows, 68 k + 4 tc covers 64 banks

// dt[r][c] = distance of frame row0 + r to frame col0 + c for r < R <= 64, c < C <= 64 (rows of `frames`, dp floats each, dp a
// multiple of 4); other entries of dt are left as they were.  Called by all DTW_THREADS threads of the workgroup with the same
// arguments; it opens with a barrier behind which xs / ys / dt are rewritten, and ends with one behind which dt may be read.
// Frames outside the R rows and C columns are never read.  gi0 / gj0: the tile's place in the pair (probe build only).
__device__ __forceinline__ void sd_distance_tile(const float *__restrict__ frames, int dp, long row0, int R, long col0, int C, int euclid,
                                                 float (*xs)[SD_LS], float (*ys)[SD_LS], float (*dt)[DTW_DT_STRIDE], int gi0, int gj0)
{
    const int tid = threadIdx.x;
    const int r4 = (tid >> 4) * 4, c4 = (tid & 15) * 4;                  // this thread's 4 x 4 block of the distance tile
    const bool block_live = r4 < R && c4 < C;
#ifndef CPC_SDTW_SKIP_DISTANCES
    float acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;
    // the next chunk's frames travel from global memory while this chunk is multiplied: two float4 of the
    // strip and two of the tile per thread (64 rows x 8 float4 over 256 threads), kept in registers
    float4 qv[2], yv[2];
    auto fetch = [&](int k0) {
        const int kc4 = min(SD_KC, dp - k0) >> 2;       // dp is a multiple of 4
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int e = tid + s * DTW_THREADS;
            const int r = e / kc4, k = (e - r * kc4) * 4;
            if (e < R * kc4) qv[s] = *reinterpret_cast<const float4 *>(frames + (row0 + r) * dp + k0 + k);
            if (e < C * kc4) yv[s] = *reinterpret_cast<const float4 *>(frames + (col0 + r) * dp + k0 + k);
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < dp; k0 += SD_KC) {
        const int kc4 = min(SD_KC, dp - k0) >> 2;
        __syncthreads();                                 // previous users of xs / ys / dt are done
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int e = tid + s * DTW_THREADS;
            const int r = e / kc4, k = (e - r * kc4) * 4;
            if (e < R * kc4) {
                xs[k][r] = qv[s].x; xs[k + 1][r] = qv[s].y; xs[k + 2][r] = qv[s].z; xs[k + 3][r] = qv[s].w;
            }
            if (e < C * kc4) {
                ys[k][r] = yv[s].x; ys[k + 1][r] = yv[s].y; ys[k + 2][r] = yv[s].z; ys[k + 3][r] = yv[s].w;
            }
        }
        __syncthreads();
        if (k0 + SD_KC < dp) fetch(k0 + SD_KC);
        if (block_live) {                                // rows >= R / columns >= C of the block hold stale
            const int kc = kc4 * 4;                      // LDS: computed, never stored
#pragma unroll 4
            for (int k = 0; k < kc; ++k) {
                const float4 xv = *reinterpret_cast<const float4 *>(&xs[k][r4]);
                const float4 yv = *reinterpret_cast<const float4 *>(&ys[k][c4]);
                const float xa[4] = {xv.x, xv.y, xv.z, xv.w};
                const float ya[4] = {yv.x, yv.y, yv.z, yv.w};
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        if (euclid) {
                            const float df = xa[a] - ya[b];
                            acc[a][b] = fmaf(df, df, acc[a][b]);
                        } else {
                            acc[a][b] = fmaf(xa[a], ya[b], acc[a][b]);
                        }
                    }
            }
        }
    }
    if (block_live) {
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (r4 + a < R && c4 + b < C)
                    dt[r4 + a][c4 + b] = euclid ? sqrtf(acc[a][b])
                                                : acosf(fminf(fmaxf(acc[a][b], -1.f), 1.f)) / 3.14159265358979323846f;
    }
#else
    // probe build of tools/term_detection_bench.py and tools/term_discovery_bench.py: the DP alone, on stand-in distances that are
    // not frame distances but vary from cell to cell, so that the three predecessors all get chosen
    __syncthreads();
    if (block_live) {
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (r4 + a < R && c4 + b < C) dt[r4 + a][c4 + b] = (float)(((gi0 + r4 + a) * 7 + (gj0 + c4 + b) * 13) & 15);
    }
#endif
    __syncthreads();
}

}  // namespace cpc
