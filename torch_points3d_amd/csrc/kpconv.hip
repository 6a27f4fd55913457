// KPConv rigid kernel-point convolution, stage 1: kernel-point weighted neighbourhood features.
//
// Reference: torch_points3d/modules/KPConv/convolution_ops.py:19-107 (KPConv_ops) with the gather of
// core/common_modules/gathering.py:1-33 (index -1 = shadow neighbour: point at 1e6, zero feature).
//   wf[q, k, :] = sum_n h(| (s[nbr[q,n]] - q) - K_k |) * x[nbr[q,n], :]          (convolution_ops.py:49-98)
//   out[q, :]   = sum_k wf[q, k, :] @ W[k]     == (Nq, KP*Cin) @ (KP*Cin, Cout)    (:101-105, one library GEMM)
// The reference materialises (Nq, Mn, KP, 3) differences and (Nq, KP, Mn) weights in HBM; here one wave owns a
// query: the KP x Mn influence weights live in LDS, neighbour feature rows are read as coalesced row segments
// and KP accumulators per lane stay in registers, so HBM sees the neighbour rows once and wf once.
// The per-query pieces shared with the deformable convolution are in kp_common.h; the inverted neighbour table of the
// backward pass is inverse_table.hip, the sum through it run_sum.hip.
#include "inverse_table.h"
#include "kp_common.h"

namespace tp3d {

// Phase A of both per-query kernels: influence weight of every (neighbour, kernel point) pair of a chunk of <= KP_NCH
// neighbours, into the wave's LDS slice.  Two steps so that a query costs two dependent global round trips instead of
// two per group of four neighbours: (a) lane n fetches neighbour n's id and its centred position into LDS; (b) every
// lane owns kernel point (lane & 15) and walks the neighbours four at a time, reading only LDS.  (The kernel was bound
// by exactly that chain: ~6 waves per SIMD each waiting ~14 serial L2 round trips.)
template <bool CLOSEST>
__device__ __forceinline__ void kp_influence_weights(const float *__restrict__ support, const int64_t *__restrict__ nbr_row,
                                                     int cnt, int64_t M, float qx, float qy, float qz,
                                                     const float *__restrict__ kpts, int KP, const KpInfluence &infl,
                                                     float (*w)[KP_MAX], float (*dd)[KP_MAX], float4 *rel, int *ids,
                                                     int lane)
{
    const int cntg = (cnt + KP_GROUP - 1) / KP_GROUP * KP_GROUP;  // rows [cnt, cntg) become shadows (zero weights)
    kp_fetch_neighbours(support, nbr_row, cnt, cntg, M, qx, qy, qz, make_float4(0.0f, 0.0f, 0.0f, 0.0f), rel, ids, lane);
    wave_lds_sync();
    const int k = lane & (KP_MAX - 1);
    const bool kreal = k < KP;
    const float kx = kreal ? kpts[k * 3 + 0] : 0.0f, ky = kreal ? kpts[k * 3 + 1] : 0.0f, kz = kreal ? kpts[k * 3 + 2] : 0.0f;
    for (int n = lane / KP_MAX; n < cntg; n += 64 / KP_MAX) {
        const float4 r = rel[n];
        float wv = 0.0f, d2 = 3.0e38f;
        if (ids[n] >= 0 && kreal) {
            const float dx = r.x - kx, dy = r.y - ky, dz = r.z - kz;
            d2 = (dx * dx + dy * dy) + dz * dz;
            wv = kp_h<false>(d2, infl);
        }
        w[n][k] = wv;
        if (CLOSEST) dd[n][k] = d2;
    }
    wave_lds_sync();
    if (CLOSEST) {  // only the closest kernel point keeps its influence (first minimum)
        if (lane < cnt) {
            int kb = 0;
            float best = dd[lane][0];
            for (int kk = 1; kk < KP; ++kk)
                if (dd[lane][kk] < best) {
                    best = dd[lane][kk];
                    kb = kk;
                }
            for (int kk = 0; kk < KP; ++kk)
                if (kk != kb) w[lane][kk] = 0.0f;
        }
        wave_lds_sync();
    }
}

template <bool CLOSEST>
__global__ __launch_bounds__(KP_BLOCK) void kpconv_weighted_kernel(
    const float *__restrict__ query, const float *__restrict__ support, const int64_t *__restrict__ nbr,
    const float *__restrict__ feat, const float *__restrict__ kpts, int64_t Nq, int64_t M, int Mn, int Cin, int KP,
    float extent, int influence, float *__restrict__ wf)
{
    __shared__ __attribute__((aligned(16))) float s_w[KP_BLOCK / 64][KP_NCH][KP_MAX];
    __shared__ __attribute__((aligned(16))) float4 s_rel[KP_BLOCK / 64][KP_NCH];
    __shared__ float s_d[CLOSEST ? KP_BLOCK / 64 : 1][CLOSEST ? KP_NCH : 1][KP_MAX];  // distances: closest mode only
    __shared__ int s_id[KP_BLOCK / 64][KP_NCH];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t q = (int64_t)blockIdx.x * (KP_BLOCK / 64) + wave;
    if (q >= Nq) return;  // wave-uniform; the kernel has no workgroup barrier
    const float qx = query[q * 3 + 0], qy = query[q * 3 + 1], qz = query[q * 3 + 2];
    float(*w)[KP_MAX] = s_w[wave];
    float(*dd)[KP_MAX] = s_d[CLOSEST ? wave : 0];
    float4 *rel = s_rel[wave];
    int *ids = s_id[wave];
    const KpInfluence infl = kp_influence(extent, influence);

    const bool single_pass = Mn <= KP_NCH;  // then the weights of phase A serve every channel chunk
    for (int c0 = 0; c0 < Cin; c0 += 64) {
        float acc[KP_MAX];
#pragma unroll
        for (int k = 0; k < KP_MAX; ++k) acc[k] = 0.0f;
        const int c = c0 + lane;
        for (int n0 = 0; n0 < Mn; n0 += KP_NCH) {
            const int cnt = min(KP_NCH, Mn - n0);
            // ---- phase A: influence weight of every (neighbour, kernel point) pair of this chunk
            if (!(single_pass && c0 > 0))
                kp_influence_weights<CLOSEST>(support, nbr + q * Mn + n0, cnt, M, qx, qy, qz, kpts, KP, infl, w, dd, rel, ids,
                                              lane);
            // ---- phase B: accumulate the neighbour rows into the KP accumulators (lanes over channels)
            if (c < Cin) kp_fma_rows(feat, ids, w, (cnt + KP_GROUP - 1) / KP_GROUP * KP_GROUP, Cin, c, acc);
            wave_lds_sync();
        }
        if (c < Cin) {
#pragma unroll
            for (int k = 0; k < KP_MAX; ++k)
                if (k < KP) wf[((size_t)q * KP + k) * Cin + c] = acc[k];
        }
    }
}


// The same product on the matrix pipe (sum aggregation, <= 64 neighbours): per query the weighted features are a small GEMM,
//   wf[k][c] = sum_n w[n][k] * f[n][c]          (16 kernel points x Mn neighbours x Cin channels),
// and the kernel above spends its time broadcasting w out of LDS (one ds_read_b128 per four weights and per 64 channel
// lanes: 128 reads = 1024 LDS cycles per query wave, 125 us over 65536 queries whatever Cin is) and on 512 wave-wide FMAs.
// v_mfma_f32_16x16x4_f32 takes A = w[kernel point = lane & 15][neighbour = 4 s + (lane >> 4)] -- exactly the layout phase A
// computes the influence weights in, so they stay in registers -- and B = f[neighbour][channel = lane & 15], a gather of
// four 64-byte row segments per load instruction; exact fp32 multiply-adds, the 16 x 16 result per channel block in four
// registers per lane.  LDS holds only the neighbours' ids and centred positions (1.3 KB per wave).
template <int SMAX>  // most MFMA steps of four neighbours: 8 (Mn <= 32) or 16 (Mn <= 64)
__global__ __launch_bounds__(KP_BLOCK) void kpconv_weighted_mfma_kernel(
    const float *__restrict__ query, const float *__restrict__ support, const int64_t *__restrict__ nbr,
    const float *__restrict__ feat, const float *__restrict__ kpts, int64_t Nq, int64_t M, int Mn, int Cin, int KP,
    float extent, int influence, int cpass, float *__restrict__ wf)
{
    __shared__ __attribute__((aligned(16))) float4 s_rel[KP_BLOCK / 64][KP_NMAX];
    __shared__ int s_id[KP_BLOCK / 64][KP_NMAX];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t q = (int64_t)blockIdx.x * (KP_BLOCK / 64) + wave;
    if (q >= Nq) return;  // wave-uniform; no workgroup barrier below
    float4 *rel = s_rel[wave];
    int *ids = s_id[wave];
    const float qx = query[q * 3 + 0], qy = query[q * 3 + 1], qz = query[q * 3 + 2];
    const KpInfluence infl = kp_influence(extent, influence);
    const int steps = (Mn + 3) / 4;  // MFMA steps of four neighbours (<= SMAX)
    // (a) lane n: neighbour n's id and centred position (rows past Mn and shadow neighbours: id -1, zero weights)
    kp_fetch_neighbours(support, nbr + q * Mn, Mn, 64, M, qx, qy, qz, make_float4(0.0f, 0.0f, 0.0f, 0.0f), rel, ids, lane);
    wave_lds_sync();
    // (b) influence weights in the A-operand layout: lane = (kernel point k = lane & 15, neighbour 4 s + (lane >> 4))
    const int k = lane & 15, nsub = lane >> 4;
    const bool kreal = k < KP;
    const float kx = kreal ? kpts[k * 3 + 0] : 0.0f, ky = kreal ? kpts[k * 3 + 1] : 0.0f, kz = kreal ? kpts[k * 3 + 2] : 0.0f;
    float a[SMAX];
    unsigned roff[SMAX];  // FLOAT offset of the neighbour row this lane gathers in step s (host: M * Cin < 2^30); a shadow
                          // neighbour has zero weights and row 0 stands in for it (as in the kernel above)
#pragma unroll
    for (int s = 0; s < SMAX; ++s) {
        a[s] = 0.0f;
        roff[s] = 0;
        if (s < steps) {
            const int n = 4 * s + nsub;
            const float4 r = rel[n];
            const int id = ids[n];
            roff[s] = (unsigned)max(id, 0) * (unsigned)Cin;
            if (id >= 0 && kreal) {
                const float dx = r.x - kx, dy = r.y - ky, dz = r.z - kz;
                const float d2 = (dx * dx + dy * dy) + dz * dz;
                a[s] = kp_h<false>(d2, infl);
            }
        }
    }
    // (c) gather the rows and accumulate on the matrix pipe, this grid row's channels
    const int c_lo = (int)blockIdx.y * cpass;
    kp_mfma_contract<SMAX>(feat, a, roff, steps, c_lo, min(Cin, c_lo + cpass), Cin, KP, lane, wf + (size_t)q * KP * Cin);
}

}  // namespace tp3d

using namespace tp3d;

TP3D_EXPORT int tp3d_kpconv_weighted_f32(const float *query, const float *support, const int64_t *neighbors,
                                         const float *features, const float *k_points, int64_t Nq, int64_t M,
                                         int Mn, int Cin, int KP, float extent, int influence, int closest,
                                         float *weighted, void *stream)
{
    if (int rc = kp_check_args(Nq, M, Mn, Cin, KP, influence, 0)) return rc;
    if (Nq == 0) return TP3D_OK;
    hipStream_t s = (hipStream_t)stream;
    if (!query || !weighted || !k_points || (Mn > 0 && (!neighbors || !support || !features))) return TP3D_E_BADARG;
    if (M == 0 || Mn == 0)  // no support row to read: every neighbour is a shadow
        return zero_async(weighted, (size_t)Nq * KP * Cin * sizeof(float), s);
    const KpMfmaRoute r = kp_mfma_route(Nq, M, Mn, Cin);
    if (closest)
        hipLaunchKernelGGL(kpconv_weighted_kernel<true>, kp_query_grid(Nq), dim3(KP_BLOCK), 0, s, query, support, neighbors,
                           features, k_points, Nq, M, Mn, Cin, KP, extent, influence, weighted);
    else if (r.ok && !r.wide)
        hipLaunchKernelGGL(kpconv_weighted_mfma_kernel<8>, r.grid, dim3(KP_BLOCK), 0, s, query, support, neighbors, features,
                           k_points, Nq, M, Mn, Cin, KP, extent, influence, r.cpass, weighted);
    else if (r.ok)
        hipLaunchKernelGGL(kpconv_weighted_mfma_kernel<16>, r.grid, dim3(KP_BLOCK), 0, s, query, support, neighbors, features,
                           k_points, Nq, M, Mn, Cin, KP, extent, influence, r.cpass, weighted);
    else
        hipLaunchKernelGGL(kpconv_weighted_kernel<false>, kp_query_grid(Nq), dim3(KP_BLOCK), 0, s, query, support, neighbors,
                           features, k_points, Nq, M, Mn, Cin, KP, extent, influence, weighted);
    return check_launch();
}

// =====================================================================================================
// Backward of stage 1 with respect to the input features:
//   d_x[m, :] = sum over slots (q, n) with nbr[q,n] == m of  sum_k h(|(s_m - q) - K_k|) * d_wf[q, k, :]
// (reference: autograd through convolution_ops.py:92-98).  No float atomics: one wave per query writes the gradient row of
// each of its slots, then one wave per support point sums the rows of the slots that reference it through the inverted
// neighbour table (inverse_table.hip, run_sum.hip), in ascending slot order.
namespace tp3d {

// Backward, step 1 (one wave per query): per-slot gradient rows
//   g[q, n, :] = sum_k h(|(s[nbr[q,n]] - q) - K_k|) * d_wf[q, k, :]
// d_wf[q] (KP x Cin) is read ONCE into registers (lanes over channels) and combined with the KP x Mn influence weights
// recomputed in LDS exactly like the forward pass.  (The first version walked, per support point, every slot that
// references it and re-read the whole d_wf[q] block each time: Mn times the traffic.)
template <bool CLOSEST>
__global__ __launch_bounds__(KP_BLOCK) void kpconv_bwd_slots_kernel(
    const float *__restrict__ query, const float *__restrict__ support, const int64_t *__restrict__ nbr,
    const float *__restrict__ kpts, const float *__restrict__ d_wf, int64_t Nq, int64_t M, int Mn, int Cin, int KP,
    float extent, int influence, float *__restrict__ g)
{
    __shared__ __attribute__((aligned(16))) float s_w[KP_BLOCK / 64][KP_NCH][KP_MAX];
    __shared__ __attribute__((aligned(16))) float4 s_rel[KP_BLOCK / 64][KP_NCH];
    __shared__ float s_d[CLOSEST ? KP_BLOCK / 64 : 1][CLOSEST ? KP_NCH : 1][KP_MAX];
    __shared__ int s_id[KP_BLOCK / 64][KP_NCH];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t q = (int64_t)blockIdx.x * (KP_BLOCK / 64) + wave;
    if (q >= Nq) return;  // wave-uniform; the kernel has no workgroup barrier
    const float qx = query[q * 3 + 0], qy = query[q * 3 + 1], qz = query[q * 3 + 2];
    float(*w)[KP_MAX] = s_w[wave];
    float(*dd)[KP_MAX] = s_d[CLOSEST ? wave : 0];
    float4 *rel = s_rel[wave];
    int *ids = s_id[wave];
    const KpInfluence infl = kp_influence(extent, influence);
    const bool single_pass = Mn <= KP_NCH;
    for (int c0 = 0; c0 < Cin; c0 += 64) {
        const int c = c0 + lane;
        float dk[KP_MAX];
#pragma unroll
        for (int k = 0; k < KP_MAX; ++k) dk[k] = (k < KP && c < Cin) ? d_wf[((size_t)q * KP + k) * Cin + c] : 0.0f;
        for (int n0 = 0; n0 < Mn; n0 += KP_NCH) {
            const int cnt = min(KP_NCH, Mn - n0);
            if (!(single_pass && c0 > 0))
                kp_influence_weights<CLOSEST>(support, nbr + q * Mn + n0, cnt, M, qx, qy, qz, kpts, KP, infl, w, dd, rel, ids,
                                              lane);
            if (c < Cin) {
#pragma unroll 5
                for (int n = 0; n < cnt; ++n) {
                    const float4 w0 = *reinterpret_cast<const float4 *>(&w[n][0]);
                    const float4 w1 = *reinterpret_cast<const float4 *>(&w[n][4]);
                    const float4 w2 = *reinterpret_cast<const float4 *>(&w[n][8]);
                    const float4 w3 = *reinterpret_cast<const float4 *>(&w[n][12]);
                    // same k order as the first version's accumulation (ascending k), fused multiply-adds
                    float acc = w0.x * dk[0];
                    acc = __builtin_fmaf(w0.y, dk[1], acc);   acc = __builtin_fmaf(w0.z, dk[2], acc);
                    acc = __builtin_fmaf(w0.w, dk[3], acc);   acc = __builtin_fmaf(w1.x, dk[4], acc);
                    acc = __builtin_fmaf(w1.y, dk[5], acc);   acc = __builtin_fmaf(w1.z, dk[6], acc);
                    acc = __builtin_fmaf(w1.w, dk[7], acc);   acc = __builtin_fmaf(w2.x, dk[8], acc);
                    acc = __builtin_fmaf(w2.y, dk[9], acc);   acc = __builtin_fmaf(w2.z, dk[10], acc);
                    acc = __builtin_fmaf(w2.w, dk[11], acc);  acc = __builtin_fmaf(w3.x, dk[12], acc);
                    acc = __builtin_fmaf(w3.y, dk[13], acc);  acc = __builtin_fmaf(w3.z, dk[14], acc);
                    acc = __builtin_fmaf(w3.w, dk[15], acc);
                    g[((size_t)q * Mn + n0 + n) * Cin + c] = acc;
                }
            }
            wave_lds_sync();
        }
    }
}

}  // namespace tp3d

TP3D_EXPORT int tp3d_kpconv_bwd_features_f32(const float *query, const float *support, const int64_t *neighbors,
                                             const float *k_points, const float *d_weighted, int64_t Nq, int64_t M,
                                             int Mn, int Cin, int KP, float extent, int influence, int closest,
                                             float *d_features, void *inverse, size_t inverse_bytes, int inverse_ready,
                                             void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = kp_check_args(Nq, M, Mn, Cin, KP, influence, 0)) return rc;
    if (M == 0) return TP3D_OK;
    if (!d_features) return TP3D_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    const int64_t slots = Nq * Mn;
    if (slots == 0) return zero_async(d_features, (size_t)M * Cin * sizeof(float), s);
    if (!query || !support || !neighbors || !k_points || !d_weighted || !workspace || !inverse) return TP3D_E_BADARG;
    if (slots > INT32_MAX || M > INT32_MAX / 2) return TP3D_E_TOOBIG;
    if (inverse_bytes < tp3d_kpconv_bwd_workspace_bytes(M, slots)) return TP3D_E_BADARG;
    if (workspace_bytes < tp3d_kpconv_grad_workspace_bytes(M, slots, Cin)) return TP3D_E_BADARG;
    int *start = nullptr, *order = nullptr;
    if (int rc = invert_neighbors(neighbors, slots, M, inverse, &start, &order, s, inverse_ready != 0)) return rc;
    float *g = static_cast<float *>(workspace);
    if (closest)
        hipLaunchKernelGGL(kpconv_bwd_slots_kernel<true>, kp_query_grid(Nq), dim3(KP_BLOCK), 0, s, query, support, neighbors,
                           k_points, d_weighted, Nq, M, Mn, Cin, KP, extent, influence, g);
    else
        hipLaunchKernelGGL(kpconv_bwd_slots_kernel<false>, kp_query_grid(Nq), dim3(KP_BLOCK), 0, s, query, support, neighbors,
                           k_points, d_weighted, Nq, M, Mn, Cin, KP, extent, influence, g);
    return gather_slot_rows(g, start, order, M, Cin, d_features, s);
}
