// What the kernel-point convolutions share (kpconv.hip: rigid, kpconv_deform.hip: deformable): the tile constants and
// the per-query device code of a "one wave owns a query" kernel, plus the host-side argument checks and the routing
// of the matrix-pipe forward.  Device functions are __forceinline__: every kernel keeps its own instruction stream.
#pragma once
#include "tp3d_common.h"

namespace tp3d {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int KP_BLOCK = 256;  // 4 waves, one query per wave
constexpr int KP_MAX = 16;     // kernel points (15 in every reference config)
constexpr int KP_NCH = 48;     // neighbours per LDS pass (covers every max_num_neighbors of the reference configs)
constexpr int KP_GROUP = 16;   // neighbour rows fetched together in the per-lane FMA accumulation
constexpr int KP_NMAX = 64;    // neighbours per matrix-pipe pass (one lane each when they are fetched)
constexpr int KP_CB = 4;       // 16-channel blocks accumulated together on the matrix pipe (64 channels per pass)
static_assert(KP_NCH % KP_GROUP == 0 && KP_NCH <= 64, "phase A pads a chunk to whole groups, one lane per row");

// Every wave owns its slice of the LDS arrays, so the phases of a query only need the wave's own LDS writes to have
// landed: a wave-level barrier, not a workgroup one (which would make four unrelated queries wait for each other).
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

struct KpInfluence {
    float ext2, inv_extent, gden;
    int mode;  // 0 constant, 1 linear, 2 gaussian
};

// ext2 (the squared extent) is read by the deformable kernels only: their in-range test and kp_h<true>
__device__ __forceinline__ KpInfluence kp_influence(float extent, int mode, float ext2 = 0.0f)
{
    const float sigma = extent * 0.3f;
    return KpInfluence{ext2, 1.0f / extent, 2.0f * sigma * sigma + 1e-9f, mode};
}

// Influence of a kernel point at squared distance d2.  CUT names what "constant" means: the rigid convolution gives
// every real neighbour weight 1 (false), the deformable one only those within the extent (true).
template <bool CUT>
__device__ __forceinline__ float kp_h(float d2, const KpInfluence &f)
{
    if (f.mode == 0) return (!CUT || d2 < f.ext2) ? 1.0f : 0.0f;
    // linear: 1-ulp v_sqrt_f32 and a reciprocal multiply (features carry a 1e-5 tolerance; the correctly
    // rounded sqrt + divide sequences cost ~25 instructions per pair)
    if (f.mode == 1) return fmaxf(1.0f - __builtin_amdgcn_sqrtf(d2) * f.inv_extent, 0.0f);
    return expf(-d2 / f.gden);
}

// Lane n of a chunk of `cnt` <= 64 neighbours: its id (-1 = shadow: outside [0, M)) and centred position into the
// wave's LDS slice.  A shadow neighbour gets the centred position `shadow_rel` (rigid: the origin, its weights are
// zero anyway; deformable: (1e6, 1e6, 1e6) - q, it takes part in kp_min); lanes in [cnt, fill) get id -1 and a zero
// position (padding that every caller masks out).
__device__ __forceinline__ void kp_fetch_neighbours(const float *__restrict__ support, const int64_t *__restrict__ nbr_row,
                                                    int cnt, int fill, int64_t M, float qx, float qy, float qz,
                                                    float4 shadow_rel, float4 *rel, int *ids, int lane)
{
    if (lane < fill) {
        const int64_t id = lane < cnt ? nbr_row[lane] : -1;
        const bool shadow = id < 0 || id >= M;
        float4 r = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (!shadow) {
            r.x = support[id * 3 + 0] - qx;
            r.y = support[id * 3 + 1] - qy;
            r.z = support[id * 3 + 2] - qz;
        } else if (lane < cnt) {
            r = shadow_rel;
        }
        ids[lane] = shadow ? -1 : (int)id;
        rel[lane] = r;
    }
}

// Per-lane FMA accumulation (lanes over channels, this lane: channel c): acc[k] += w[n][k] * feat[ids[n]][c] over the
// rows [0, cntg) of a chunk, cntg a multiple of KP_GROUP.
__device__ __forceinline__ void kp_fma_rows(const float *__restrict__ feat, const int *ids, const float (*w)[KP_MAX],
                                            int cntg, int Cin, int c, float (&acc)[KP_MAX])
{
    // KP_GROUP neighbour rows are requested before any is used: the accumulation was a chain of dependent
    // (LDS id -> global row) round trips, ~0.3 us per neighbour (measured with in-kernel clocks)
    for (int g0 = 0; g0 < cntg; g0 += KP_GROUP) {
        float v[KP_GROUP];
#pragma unroll
        for (int u = 0; u < KP_GROUP; ++u)  // shadow rows carry zero weights: row 0 stands in for them
            v[u] = feat[(size_t)max(ids[g0 + u], 0) * Cin + c];
#pragma unroll
        for (int u = 0; u < KP_GROUP; ++u) {
            const int n = g0 + u;
            const float4 w0 = *reinterpret_cast<const float4 *>(&w[n][0]);
            const float4 w1 = *reinterpret_cast<const float4 *>(&w[n][4]);
            const float4 w2 = *reinterpret_cast<const float4 *>(&w[n][8]);
            const float4 w3 = *reinterpret_cast<const float4 *>(&w[n][12]);
            // explicit fused multiply-adds: the translation unit is built with contraction off for the
            // distance expressions, the feature accumulation has no bit-exactness contract (1e-5 relative)
            acc[0] = __builtin_fmaf(w0.x, v[u], acc[0]);   acc[1] = __builtin_fmaf(w0.y, v[u], acc[1]);
            acc[2] = __builtin_fmaf(w0.z, v[u], acc[2]);   acc[3] = __builtin_fmaf(w0.w, v[u], acc[3]);
            acc[4] = __builtin_fmaf(w1.x, v[u], acc[4]);   acc[5] = __builtin_fmaf(w1.y, v[u], acc[5]);
            acc[6] = __builtin_fmaf(w1.z, v[u], acc[6]);   acc[7] = __builtin_fmaf(w1.w, v[u], acc[7]);
            acc[8] = __builtin_fmaf(w2.x, v[u], acc[8]);   acc[9] = __builtin_fmaf(w2.y, v[u], acc[9]);
            acc[10] = __builtin_fmaf(w2.z, v[u], acc[10]); acc[11] = __builtin_fmaf(w2.w, v[u], acc[11]);
            acc[12] = __builtin_fmaf(w3.x, v[u], acc[12]); acc[13] = __builtin_fmaf(w3.y, v[u], acc[13]);
            acc[14] = __builtin_fmaf(w3.z, v[u], acc[14]); acc[15] = __builtin_fmaf(w3.w, v[u], acc[15]);
        }
    }
}

// Matrix-pipe gather-and-contract of one query over the channels [c_lo, c_hi):
//   wq[k][c] = scale[k] * sum_n a[n][k] * feat[n][c]
// with v_mfma_f32_16x16x4_f32: A = a[s] holds the influence weight of (kernel point lane & 15, neighbour 4 s +
// (lane >> 4)), B = the neighbour rows, gathered through roff[s], the FLOAT offset of the row this lane reads in step s
// (host: M * Cin < 2^30).  Per pass of up to 64 channels: gather the rows (a 16-channel block per load, blocks past
// c_hi skipped by wave-uniform branches), accumulate.  Addresses: a wave-uniform base + a 32-bit lane offset.
// `scale`: this lane's four output kernel points 4 (lane >> 4) + j, or null for none.
template <int SMAX>
__device__ __forceinline__ void kp_mfma_contract(const float *__restrict__ feat, const float (&a)[SMAX],
                                                 const unsigned (&roff)[SMAX], int steps, int c_lo, int c_hi, int Cin,
                                                 int KP, int lane, float *__restrict__ wq, const float *scale = nullptr)
{
    const int nsub = lane >> 4, c16 = lane & 15;
    for (int c0 = c_lo; c0 < c_hi; c0 += 16 * KP_CB) {
        const int nblk = min(KP_CB, (c_hi - c0 + 15) / 16);  // (wave-uniform)
        f32x4 acc[KP_CB];
#pragma unroll
        for (int b = 0; b < KP_CB; ++b) acc[b] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
        const float *__restrict__ fb = feat + c0;
        unsigned coff[KP_CB];  // this lane's channel inside the pass, clamped to the row (lanes past Cin are not stored)
#pragma unroll
        for (int b = 0; b < KP_CB; ++b) coff[b] = (unsigned)min(16 * b + c16, Cin - 1 - c0);
#pragma unroll
        for (int s0 = 0; s0 < SMAX; s0 += 4) {  // four steps' loads in flight (16 rows x up to 4 blocks)
            if (s0 < steps) {
                float v[4][KP_CB];
#pragma unroll
                for (int b = 0; b < KP_CB; ++b)
                    if (b < nblk) {
#pragma unroll
                        for (int u = 0; u < 4; ++u) v[u][b] = fb[roff[s0 + u] + coff[b]];
                    }
#pragma unroll
                for (int b = 0; b < KP_CB; ++b)
                    if (b < nblk) {
#pragma unroll
                        for (int u = 0; u < 4; ++u)
                            acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s0 + u], v[u][b], acc[b], 0, 0, 0);
                    }
            }
        }
        // D[kernel point = 4 (lane >> 4) + j][channel = lane & 15]
#pragma unroll
        for (int b = 0; b < KP_CB; ++b)
            if (b < nblk) {
                const int c = c0 + 16 * b + c16;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int kp = 4 * nsub + j;
                    if (kp < KP && c < Cin) wq[(unsigned)(kp * Cin + c)] = scale ? acc[b][j] * scale[j] : acc[b][j];
                }
            }
    }
}

// ---------------------------------------------------------------------------------------------------------- host side
constexpr int KP_WAVES = KP_BLOCK / 64;  // queries per workgroup

// The argument checks every KPConv entry point opens with.  `least`: the smallest M and Mn accepted -- 0 for the rigid
// entry points (an empty table zero-fills), 1 for the deformable ones.
inline int kp_check_args(int64_t Nq, int64_t M, int Mn, int Cin, int KP, int influence, int least)
{
    if (Nq < 0 || M < least || Mn < least || Cin <= 0 || KP <= 0 || influence < 0 || influence > 2) return TP3D_E_BADARG;
    if (KP > KP_MAX) return TP3D_E_TOOBIG;
    if ((Nq + KP_WAVES - 1) / KP_WAVES > 0x7fffffff) return TP3D_E_TOOBIG;  // one wave per query: the grid's x limit
    return TP3D_OK;
}

inline dim3 kp_query_grid(int64_t Nq, int y = 1) { return dim3((unsigned)((Nq + KP_WAVES - 1) / KP_WAVES), y); }

// The matrix-pipe forward (sum aggregation): whether it applies, which instance, its grid and channels per grid row.
struct KpMfmaRoute {
    bool ok;    // <= 64 neighbours and 32-bit float offsets into the features
    bool wide;  // more than 32 neighbours: the 16-step instance instead of the 8-step one
    dim3 grid;
    int cpass;
};

inline KpMfmaRoute kp_mfma_route(int64_t Nq, int64_t M, int Mn, int Cin)
{
    const int passes = (Cin + 16 * KP_CB - 1) / (16 * KP_CB);
    // few queries with many channels -- the deep levels of a U-Net -- spread their channel passes over gridDim.y: a wave
    // per (query, 64 channels) instead of eight serial passes in 27 waves (latency-bound launches)
    const bool spread = passes > 1 && Nq <= 4096;
    return KpMfmaRoute{Mn <= KP_NMAX && M * (int64_t)Cin < ((int64_t)1 << 30),  // (the reference configs ask for 25 ... 38 neighbours)
                       Mn > 32, kp_query_grid(Nq, spread ? passes : 1), spread ? 16 * KP_CB : Cin};
}

}  // namespace tp3d
