// Host-side launch plans of gemm_rows.hip (forward contraction) and gemm_tn.hip (weight gradient): plain arithmetic on
// the sizes, no device code and no HIP header, so that a CPU-only program can compile and sweep them
// (tests/guard/few_row_plans_main.cpp, under the host sanitizers).  The .hip files launch from these plans and the
// "Launch plans" queries of include/tp3d_hip.h report them.
#pragma once
#include <stdint.h>

namespace tp3d {

// tp3d_set_few_row_tiles: 1 = launches that would leave most of the 1024 SIMDs without a wave (the 4096- and 16384-row
// layers) use quarter- or half-size workgroup tiles; 0 = the plans before that rule.  Results are bit-identical.
inline int g_few_row_tiles = 1;

constexpr int GR_BM = 128, GR_BK = 32;
constexpr int GR_GRID = 1024;  // persistent: 4 workgroups per CU, a multiple of 8
constexpr int GR_SMALL_ITEMS = 256;  // most 128 x 128 work items of a launch served by the 64 x 64 form

struct RowsPlan {
    bool wide;  // 128 x 128 tiles (else 128 x 64)
    int tiles_n, wave_rows;
    int64_t row_blocks, items, blocks;
    bool per_workgroup;  // statistics chunks: per (workgroup, wave row) instead of per (128-row block, wave row)
    int64_t chunks;
    int ksplit, kchunk;  // K-ranges of a split launch (1 = no split)
};
inline RowsPlan rows_plan(int64_t M, int N, int K = 0, bool allow_split = false)
{
    RowsPlan p;
    // narrow tiles when they cover N with less padding (N <= 64, or a remainder of at most 64 columns: 192, 320 ...)
    const int rem = N % 128;
    p.wide = !(rem > 0 && rem <= 64);
    const int bn = p.wide ? 128 : 64;
    p.wave_rows = p.wide ? 2 : 4;
    p.tiles_n = (N + bn - 1) / bn;
    p.row_blocks = (M + GR_BM - 1) / GR_BM;
    const int64_t groups = (p.row_blocks + 7) / 8;
    p.items = groups * 8 * p.tiles_n;  // items past the last row block stage zeros and store nothing
    p.blocks = p.items < GR_GRID ? p.items : GR_GRID;
    p.per_workgroup = p.blocks == GR_GRID && GR_GRID % (8 * p.tiles_n) == 0;
    p.chunks = p.wave_rows * (p.per_workgroup ? GR_GRID / p.tiles_n : p.row_blocks);
    p.ksplit = 1;
    p.kchunk = K > 0 ? (K + GR_BK - 1) / GR_BK * GR_BK : 0;
    if (allow_split && K >= 1024 && p.items <= 128) {
        // few output tiles and a very long contraction (the 1280 / 1536-channel decoder layers): K-ranges of >= 128
        // (every range writes an M x N slab that the summing pass reads back, so no more ranges than needed)
        const int want = (int)((512 + p.items - 1) / p.items);
        const int by_k = K / 128;
        int s = want < by_k ? want : by_k;
        if (s > 16) s = 16;
        if (s > 1) {
            p.kchunk = ((K + s - 1) / s + GR_BK - 1) / GR_BK * GR_BK;
            p.ksplit = (K + p.kchunk - 1) / p.kchunk;
        }
    }
    return p;
}

// The 64 x 64 form of the plain wide kernel (gemm_rows_small_kernel): every 128 x 128 work item of `p` becomes four
// (two 64-row halves x two 64-column halves), one workgroup each.  Serves the wide, unsplit launches of at most
// GR_SMALL_ITEMS items, which never keep per-workgroup statistics (those need GR_GRID items): the chunk layout -- one
// per (128-row block, 64-row half) -- is the one `p` reports either way.
struct RowsSmallPlan {
    bool routed;
    int64_t items, blocks;  // 64 x 64 work items (padding items included) = workgroups
};
inline RowsSmallPlan rows_small_plan(const RowsPlan &p)
{
    RowsSmallPlan s;
    s.routed = g_few_row_tiles != 0 && p.wide && p.ksplit == 1 && p.items <= GR_SMALL_ITEMS;
    s.items = s.blocks = s.routed ? 4 * p.items : 0;
    return s;
}

constexpr int TN_BR_MAX = 64;  // most rows staged per step (narrow tiles stage more rows per barrier)
constexpr int TN_FILL = 256;   // workgroups (one per CU) below which the weight gradient takes a smaller tile

struct TnPlan {
    int wm, wn, gn, tn, tk, tiles_n, tiles_k, splits;
    int64_t rows_per_split;
};

inline void tn_set_tile(TnPlan &p, int N, int K)
{
    p.tn = 32 * p.gn * p.wm;
    p.tk = 32 * (4 / p.gn) * p.wn;
    p.tiles_n = (N + p.tn - 1) / p.tn;
    p.tiles_k = (K + p.tk - 1) / p.tk;
}

inline TnPlan plan_tn(int64_t M, int N, int K)
{
    TnPlan p;
    p.wm = N > 64 ? 2 : 1;
    // K just above a multiple of 128 (131 = 128 features + xyz): 192-wide tiles halve the padded columns and read dY
    // once instead of twice; wider K: 192 only where it strictly removes padded columns
    if (K <= 64) p.wn = 1;
    else if (K <= 128) p.wn = 2;
    else if (K <= 192) p.wn = 3;
    else p.wn = ((K + 191) / 192) * 192 < ((K + 127) / 128) * 128 ? 3 : 2;
    p.gn = 2;
    if (N <= 32 && K >= 128) {  // a handful of output rows: one wave row, four wave columns (32 x 128 tiles)
        p.gn = 1;
        p.wm = 1;
        p.wn = 1;
    }
    tn_set_tile(p, N, K);
    const int tiles = p.tiles_n * p.tiles_k;
    // ~4 workgroups per CU (256 CUs) keep the MFMA pipes fed; at least 256 rows per split, at most 512 splits
    // (every split writes an N x K partial tile that the reduction pass reads back)
    int64_t want = (1024 + tiles - 1) / tiles;
    const int min_rows = 256;
    int64_t max_by_rows = (M + min_rows - 1) / min_rows;
    int64_t s = want < max_by_rows ? want : max_by_rows;
    if (s < 1) s = 1;
    if (s > 512) s = 512;
    p.rows_per_split = ((M + s - 1) / s + TN_BR_MAX - 1) / TN_BR_MAX * TN_BR_MAX;
    p.splits = (int)((M + p.rows_per_split - 1) / p.rows_per_split);
    // Few rows cap the splits (M / 256), and tiles x splits then leaves CUs without a workgroup.  The row split -- the
    // summation order of every output element -- stays; the TILE shrinks: the largest of 128 x 64, 64 x 128, 64 x 64
    // below the present one that reaches TN_FILL workgroups, else 64 x 64.  An element's sum over the rows of its split
    // does not depend on the tile it sits in, so dW keeps its bits.  Not for the one-wave-row form, nor where 192-wide
    // tiles were chosen to cut padded columns.
    if (g_few_row_tiles != 0 && p.gn == 2 && p.wn != 3 && (int64_t)tiles * p.splits < TN_FILL) {
        const int cand[3][2] = {{2, 1}, {1, 2}, {1, 1}};
        const int wm0 = p.wm, wn0 = p.wn;
        for (int c = 0; c < 3; ++c) {
            if (cand[c][0] > wm0 || cand[c][1] > wn0 || (cand[c][0] == wm0 && cand[c][1] == wn0)) continue;
            p.wm = cand[c][0];
            p.wn = cand[c][1];
            tn_set_tile(p, N, K);
            if ((int64_t)p.tiles_n * p.tiles_k * p.splits >= TN_FILL) break;
        }
    }
    return p;
}

}  // namespace tp3d
