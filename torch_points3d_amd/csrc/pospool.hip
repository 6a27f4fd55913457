// PosPool (PPNet) position pooling: a parameter-free gather that multiplies every neighbour's feature row by a geometric
// prior of the relative position and reduces over the neighbours.
//
// Reference: torch_points3d/modules/PPNet/ops.py:44-109 (PosPoolLayer.forward) with the gather of
// core/common_modules/gathering.py (index -1 = shadow neighbour: zero feature row).
//   rel        = (s[nbr[q,n]] - q) / radius
//   xyz:     geo[q,n,c] = rel[c / (C/3)]                                                        (C % 3 == 0)
//   sin_cos: geo[q,n,c] = sin | cos (100 rel[axis] / dim_mat[j]),  c = axis * 2F + t, sine for t < F (j = t), cosine
//            for t >= F (j = t - F), F = C / 6; C == 9: F = 1 and channels 6..8 are rel itself
//   out[q,c]   = sum_n geo[q,n,c] * x[nbr[q,n], c]      (avg: / (n_q + 1e-5), n_q = slots of row q whose index is < P)
// The reference materialises the (Nq, Mn, 3) relative positions, the (Nq, Mn, C) gathered rows and their product (four
// more (Nq, Mn, C) tensors for sin_cos) in HBM; here a group of 16 / 32 / 64 lanes owns a query, channels across the
// lanes (a sine channel and its cosine channel in one lane: one sincosf for both) and the neighbour slots in a loop, so
// HBM sees the neighbour rows once and (Nq, C) once.
//
// The backward pass (features only) sums per support point through the inverted neighbour table (inverse_table.hip): no
// atomics, ascending slot order, the prior recomputed from the two positions.
#include <algorithm>

#include "inverse_table.h"

namespace tp3d {

constexpr int PP_BLOCK = 256;
constexpr int PP_UNROLL = 4;  // neighbour slots whose loads are in flight together

// P = max over the table of the index with shadows (-1 or >= M) mapped to M: what the reference's torch.max(neighbors)
// sees after its gather has rewritten -1 to M in place.  Integer maximum: any order gives the same value.
__global__ __launch_bounds__(PP_BLOCK) void pospool_padding_kernel(const int64_t *__restrict__ nbr, int64_t slots, int64_t M,
                                                                    unsigned long long *__restrict__ padding)
{
    long long best = 0;
    for (int64_t s = (int64_t)blockIdx.x * PP_BLOCK + threadIdx.x; s < slots; s += (int64_t)gridDim.x * PP_BLOCK) {
        const int64_t m = nbr[s];
        best = max(best, (long long)((m < 0 || m >= M) ? M : m));
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) best = max(best, __shfl_xor(best, off));
    if ((threadIdx.x & 63) == 0) atomicMax(padding, (unsigned long long)best);
}

// A lane owns a UNIT of channels that share one evaluation of the prior:
//   xyz      one channel c = u (axis u / (C/3));
//   sin_cos  the sine and the cosine channel of one (axis, wavelength): u = axis * F + j -> channels axis * 2F + j and
//            axis * 2F + F + j, one sincosf for both; C == 9 (F = 1): unit = axis, plus channel 6 + axis (rel itself).
struct PpUnit {
    int axis, c0, c1, c2;  // channels: c0 (rel | sine), c1 (cosine) or -1, c2 (rel of the C == 9 layout) or -1
    float div;             // wavelength divisor dim_mat[j]
};

__host__ __device__ __forceinline__ int pp_units(int C, bool sincos) { return !sincos ? C : (C == 9 ? 3 : C / 2); }

template <bool SINCOS>
__device__ __forceinline__ PpUnit pp_unit(int u, int C, const float *__restrict__ dim_mat)
{
    if (!SINCOS) return PpUnit{u / (C / 3), u, -1, -1, 1.0f};
    if (C == 9) return PpUnit{u, 2 * u, 2 * u + 1, 6 + u, dim_mat[0]};
    const int F = C / 6, axis = u / F, j = u - axis * F;
    return PpUnit{axis, axis * 2 * F + j, axis * 2 * F + F + j, -1, dim_mat[j]};
}

// The reference's order of fp32 operations: (p - q) / radius, then (100 * rel) / dim_mat, then the accurate sine / cosine
// (arguments reach ~100 rad: one ulp of the argument is ~8e-6 of the result, so no fast intrinsic and no reciprocal).
__device__ __forceinline__ float pp_rel(int axis, float px, float py, float pz, float qx, float qy, float qz, float radius)
{
    const float d = axis == 0 ? px - qx : (axis == 1 ? py - qy : pz - qz);
    return d / radius;
}

// Forward: lane = (query of the workgroup: threadIdx.x >> lw, unit lane: threadIdx.x & (W - 1)), W = 1 << lw lanes per
// query; grid row y owns the units [y * upass, (y + 1) * upass).  No LDS, no cross-lane traffic: the slot ids and
// positions a group reads are the same address in every lane (one transaction).
template <bool SINCOS>
__global__ __launch_bounds__(PP_BLOCK) void pospool_fwd_kernel(
    const float *__restrict__ query, const float *__restrict__ support, const int64_t *__restrict__ nbr,
    const float *__restrict__ feat, const unsigned long long *__restrict__ padding, const float *__restrict__ dim_mat,
    int64_t Nq, int64_t M, int Mn, int C, float radius, int avg, int lw, int upass, float *__restrict__ out,
    float *__restrict__ counts)
{
    const int W = 1 << lw, cl = threadIdx.x & (W - 1);
    const int64_t q = (int64_t)blockIdx.x * (PP_BLOCK >> lw) + (threadIdx.x >> lw);
    if (q >= Nq) return;  // no barrier in this kernel
    const float qx = query[q * 3 + 0], qy = query[q * 3 + 1], qz = query[q * 3 + 2];
    const int64_t *__restrict__ row = nbr + q * Mn;
    const int64_t P = (int64_t)*padding;
    const bool third = SINCOS && C == 9;
    const int u_lo = (int)blockIdx.y * upass, u_hi = min(pp_units(C, SINCOS), u_lo + upass);
    for (int u = u_lo + cl; u < u_hi; u += W) {
        const PpUnit un = pp_unit<SINCOS>(u, C, dim_mat);
        float acc0 = 0.0f, acc1 = 0.0f, acc2 = 0.0f;
        int n = 0;
        for (int s0 = 0; s0 < Mn; s0 += PP_UNROLL) {
            int64_t id[PP_UNROLL];
            float px[PP_UNROLL], py[PP_UNROLL], pz[PP_UNROLL], x0[PP_UNROLL], x1[PP_UNROLL], x2[PP_UNROLL];
#pragma unroll
            for (int k = 0; k < PP_UNROLL; ++k) id[k] = s0 + k < Mn ? row[s0 + k] : -1;
#pragma unroll
            for (int k = 0; k < PP_UNROLL; ++k) {
                const bool real = id[k] >= 0 && id[k] < M;
                n += (s0 + k < Mn && (real ? id[k] : M) < P) ? 1 : 0;
                px[k] = real ? support[id[k] * 3 + 0] : 0.0f;
                py[k] = real ? support[id[k] * 3 + 1] : 0.0f;
                pz[k] = real ? support[id[k] * 3 + 2] : 0.0f;
                const float *__restrict__ xr = feat + (size_t)(real ? id[k] : 0) * C;
                x0[k] = real ? xr[un.c0] : 0.0f;
                x1[k] = (SINCOS && real) ? xr[un.c1] : 0.0f;
                x2[k] = (third && real) ? xr[un.c2] : 0.0f;
                if (!real) id[k] = -1;
            }
#pragma unroll
            for (int k = 0; k < PP_UNROLL; ++k)
                if (id[k] >= 0) {
                    const float rel = pp_rel(un.axis, px[k], py[k], pz[k], qx, qy, qz, radius);
                    if (SINCOS) {
                        float sn, cs;
                        sincosf((100.0f * rel) / un.div, &sn, &cs);
                        acc0 = acc0 + sn * x0[k];
                        acc1 = acc1 + cs * x1[k];
                        if (third) acc2 = acc2 + rel * x2[k];
                    } else {
                        acc0 = acc0 + rel * x0[k];
                    }
                }
        }
        const float nf = (float)n + 1e-5f;
        float *__restrict__ o = out + (size_t)q * C;
        o[un.c0] = avg ? acc0 / nf : acc0;
        if (SINCOS) o[un.c1] = avg ? acc1 / nf : acc1;
        if (third) o[un.c2] = avg ? acc2 / nf : acc2;
        if (counts && u == 0) counts[q] = nf;
    }
}

// Backward wrt the features: a group of W lanes owns support point m and walks the slots that reference it (ascending),
//   d_x[m,c] = sum_j geo(q_j, m, c) * (d_out[q_j, c] / (n_qj + 1e-5))            (sum reduction: no division)
template <bool SINCOS>
__global__ __launch_bounds__(PP_BLOCK) void pospool_bwd_kernel(
    const float *__restrict__ query, const float *__restrict__ support, const float *__restrict__ d_out,
    const float *__restrict__ counts, const float *__restrict__ dim_mat, const int *__restrict__ start,
    const int *__restrict__ order, int64_t M, int Mn, int C, float radius, int avg, int lw, int upass,
    float *__restrict__ d_x)
{
    const int W = 1 << lw, cl = threadIdx.x & (W - 1);
    const int64_t m = (int64_t)blockIdx.x * (PP_BLOCK >> lw) + (threadIdx.x >> lw);
    if (m >= M) return;  // no barrier in this kernel
    const float px = support[m * 3 + 0], py = support[m * 3 + 1], pz = support[m * 3 + 2];
    const int j0 = start[m], j1 = start[m + 1];
    const bool third = SINCOS && C == 9;
    const int u_lo = (int)blockIdx.y * upass, u_hi = min(pp_units(C, SINCOS), u_lo + upass);
    for (int u = u_lo + cl; u < u_hi; u += W) {
        const PpUnit un = pp_unit<SINCOS>(u, C, dim_mat);
        float acc0 = 0.0f, acc1 = 0.0f, acc2 = 0.0f;
        for (int j = j0; j < j1; j += PP_UNROLL) {
            int64_t q[PP_UNROLL];
            float qx[PP_UNROLL], qy[PP_UNROLL], qz[PP_UNROLL], g0[PP_UNROLL], g1[PP_UNROLL], g2[PP_UNROLL], nf[PP_UNROLL];
#pragma unroll
            for (int k = 0; k < PP_UNROLL; ++k) q[k] = j + k < j1 ? order[j + k] / Mn : -1;
#pragma unroll
            for (int k = 0; k < PP_UNROLL; ++k) {
                const bool on = q[k] >= 0;
                qx[k] = on ? query[q[k] * 3 + 0] : 0.0f;
                qy[k] = on ? query[q[k] * 3 + 1] : 0.0f;
                qz[k] = on ? query[q[k] * 3 + 2] : 0.0f;
                const float *__restrict__ gr = d_out + (size_t)(on ? q[k] : 0) * C;
                g0[k] = on ? gr[un.c0] : 0.0f;
                g1[k] = (SINCOS && on) ? gr[un.c1] : 0.0f;
                g2[k] = (third && on) ? gr[un.c2] : 0.0f;
                nf[k] = (on && avg) ? counts[q[k]] : 1.0f;
            }
#pragma unroll
            for (int k = 0; k < PP_UNROLL; ++k)
                if (q[k] >= 0) {
                    const float rel = pp_rel(un.axis, px, py, pz, qx[k], qy[k], qz[k], radius);
                    if (SINCOS) {
                        float sn, cs;
                        sincosf((100.0f * rel) / un.div, &sn, &cs);
                        acc0 = acc0 + sn * (avg ? g0[k] / nf[k] : g0[k]);
                        acc1 = acc1 + cs * (avg ? g1[k] / nf[k] : g1[k]);
                        if (third) acc2 = acc2 + rel * (avg ? g2[k] / nf[k] : g2[k]);
                    } else {
                        acc0 = acc0 + rel * (avg ? g0[k] / nf[k] : g0[k]);
                    }
                }
        }
        float *__restrict__ o = d_x + (size_t)m * C;
        o[un.c0] = acc0;
        if (SINCOS) o[un.c1] = acc1;
        if (third) o[un.c2] = acc2;
    }
}

// ---------------------------------------------------------------------------------------------------------- host side
// The route of both kernels, decided once from the row count (queries forward, support points backward), the width and
// the embedding: lanes per row, units per grid row and the grid.  The slot loop is a run-time loop, so Mn does not enter.
struct PpRoute {
    int lw;     // log2 of the lanes that share a row: 16 lanes up to 16 units, 32 up to 32, else a whole wave
    int upass;  // units (pp_units) per grid row
    dim3 grid;
};

inline bool pp_route(int64_t rows, int C, int embedding, PpRoute *r)
{
    const int U = pp_units(C, embedding == 1);  // ppnet.yaml, sin_cos: C = 36 -> 18 units (two rows per wave), 72 -> 36,
    r->lw = U <= 16 ? 4 : (U <= 32 ? 5 : 6);    // 144 -> 72 (two passes), ..., 1152 -> 576 (nine passes)
    const int per_block = PP_BLOCK >> r->lw;
    const int64_t bx = (rows + per_block - 1) / per_block;
    if (bx > 0x7fffffff) return false;
    // few rows with many units -- the deep stages (C = 576, 1152 on a few thousand points) -- spread their 64-unit passes
    // over gridDim.y.  The row limits are estimates read from the code (a sin_cos unit costs one sincosf per slot, an xyz
    // unit one multiply-add), not tuned by measurement.
    const int passes = (U + 63) / 64;
    const bool spread = passes > 1 && rows <= (embedding == 1 ? 32768 : 8192);
    r->upass = spread ? 64 : U;
    r->grid = dim3((unsigned)bx, spread ? passes : 1);
    return true;
}

inline int pp_check_args(int64_t rows, int64_t M, int Mn, int C, float radius, int embedding, int reduction,
                         const float *dim_mat)
{
    if (rows < 0 || M < 0 || Mn < 0 || C <= 0 || !(radius > 0.0f)) return TP3D_E_BADARG;
    if (embedding < 0 || embedding > 1 || reduction < 0 || reduction > 1) return TP3D_E_BADARG;
    if (embedding == 0 && C % 3 != 0) return TP3D_E_BADARG;
    if (embedding == 1 && ((C % 6 != 0 && C != 9) || !dim_mat)) return TP3D_E_BADARG;
    return TP3D_OK;
}

}  // namespace tp3d

using namespace tp3d;

TP3D_EXPORT int tp3d_pospool_padding_i64(const int64_t *neighbors, int64_t slots, int64_t M, int64_t *padding, void *stream)
{
    if (slots < 0 || M < 0 || !padding || (slots > 0 && !neighbors)) return TP3D_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = zero_async(padding, sizeof(int64_t), s)) return rc;
    if (slots == 0) return TP3D_OK;
    const unsigned gs = (unsigned)std::min<int64_t>((slots + PP_BLOCK - 1) / PP_BLOCK, 2048);
    hipLaunchKernelGGL(pospool_padding_kernel, dim3(gs), dim3(PP_BLOCK), 0, s, neighbors, slots, M,
                       reinterpret_cast<unsigned long long *>(padding));
    return check_launch();
}

TP3D_EXPORT int tp3d_pospool_fwd_f32(const float *query, const float *support, const int64_t *neighbors,
                                     const float *features, const int64_t *padding, const float *dim_mat, int64_t Nq,
                                     int64_t M, int Mn, int C, float radius, int embedding, int reduction, float *out,
                                     float *counts, void *stream)
{
    if (int rc = pp_check_args(Nq, M, Mn, C, radius, embedding, reduction, dim_mat)) return rc;
    if (Nq == 0) return TP3D_OK;
    if (!query || !out || !padding || (Mn > 0 && !neighbors) || (M > 0 && (!support || !features))) return TP3D_E_BADARG;
    PpRoute r;
    if (!pp_route(Nq, C, embedding, &r)) return TP3D_E_TOOBIG;
    hipStream_t s = (hipStream_t)stream;
    const unsigned long long *pad = reinterpret_cast<const unsigned long long *>(padding);
    if (embedding == 1)
        hipLaunchKernelGGL(pospool_fwd_kernel<true>, r.grid, dim3(PP_BLOCK), 0, s, query, support, neighbors, features, pad,
                           dim_mat, Nq, M, Mn, C, radius, reduction, r.lw, r.upass, out, counts);
    else
        hipLaunchKernelGGL(pospool_fwd_kernel<false>, r.grid, dim3(PP_BLOCK), 0, s, query, support, neighbors, features, pad,
                           dim_mat, Nq, M, Mn, C, radius, reduction, r.lw, r.upass, out, counts);
    return check_launch();
}

TP3D_EXPORT int tp3d_pospool_bwd_f32(const float *query, const float *support, const int64_t *neighbors,
                                     const float *grad_out, const float *counts, const float *dim_mat, int64_t Nq, int64_t M,
                                     int Mn, int C, float radius, int embedding, int reduction, float *d_features,
                                     void *inverse, size_t inverse_bytes, int inverse_ready, void *stream)
{
    if (int rc = pp_check_args(Nq, M, Mn, C, radius, embedding, reduction, dim_mat)) return rc;
    if (M == 0) return TP3D_OK;
    if (!d_features) return TP3D_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    const int64_t slots = Nq * Mn;
    if (slots == 0) return zero_async(d_features, (size_t)M * C * sizeof(float), s);
    if (!query || !support || !neighbors || !grad_out || !inverse || (reduction == 1 && !counts)) return TP3D_E_BADARG;
    if (slots > INT32_MAX || M > INT32_MAX / 2) return TP3D_E_TOOBIG;
    if (inverse_bytes < tp3d_kpconv_bwd_workspace_bytes(M, slots)) return TP3D_E_BADARG;
    PpRoute r;
    if (!pp_route(M, C, embedding, &r)) return TP3D_E_TOOBIG;
    int *start = nullptr, *order = nullptr;
    if (int rc = invert_neighbors(neighbors, slots, M, inverse, &start, &order, s, inverse_ready != 0)) return rc;
    if (embedding == 1)
        hipLaunchKernelGGL(pospool_bwd_kernel<true>, r.grid, dim3(PP_BLOCK), 0, s, query, support, grad_out, counts, dim_mat,
                           start, order, M, Mn, C, radius, reduction, r.lw, r.upass, d_features);
    else
        hipLaunchKernelGGL(pospool_bwd_kernel<false>, r.grid, dim3(PP_BLOCK), 0, s, query, support, grad_out, counts, dim_mat,
                           start, order, M, Mn, C, radius, reduction, r.lw, r.upass, d_features);
    return check_launch();
}
