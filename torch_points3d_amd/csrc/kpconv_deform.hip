// Deformable kernel-point convolution, stage 1 and its backward.
//
// Reference: torch_points3d/modules/KPConv/convolution_ops.py:110-235 (KPConv_deform_ops).  Per query q the kernel
// points are K_k + offsets[q, k]; a neighbour that lies within `extent` of no deformed kernel point contributes
// nothing (the reference's topk / re-gather moves it onto the shadow row), the weighted features are scaled by
// modulations[q, k], and the smallest squared distance of every kernel point to the neighbourhood feeds the fitting
// loss (modules/KPConv/losses.py:12):
//   d2[q,n,k]     = |(s[nbr[q,n]] - q) - (K_k + off[q,k])|^2         shadow neighbour: the point (1e6, 1e6, 1e6)
//   in_range[q,n] = any_k d2[q,n,k] < extent^2
//   wf[q,k,:]     = mod[q,k] * sum_n in_range[q,n] * h(d2[q,n,k]) * x[nbr[q,n], :]
//   kp_min[q,k]   = min_n d2[q,n,k]  (all Mn slots; first minimum -> kp_arg)
// The reference writes (Nq, Mn, KP, 3) differences, (Nq, Mn, KP) distances, a topk and two gathers to HBM and
// differentiates through all of them; here one wave owns a query as in kpconv.hip: the distances live in registers
// in the A-operand layout of v_mfma_f32_16x16x4_f32 (kernel point = lane & 15, neighbour = 4 s + (lane >> 4)), the
// in-range mask of a neighbour is a ballot over its 16 kernel-point lanes, and the backward contracts features with
// d_wf on the matrix pipe (channels are the contraction index) to get the (kernel point, neighbour) sensitivities
// the offset and modulation gradients are made of.  No atomics; every sum has a fixed order.
// The per-query pieces shared with the rigid convolution are in kp_common.h.
#include "inverse_table.h"
#include "kp_common.h"

namespace tp3d {

constexpr int KD_WPAD = 17;          // row stride of the backward's weight tile (conflict-free column reads)
constexpr float KD_SHADOW = 1.0e6f;  // convolution_ops.py:146

// a shadow neighbour of query q sits at (1e6, 1e6, 1e6) and takes part in kp_min: its centred position
__device__ __forceinline__ float4 kd_shadow_rel(float qx, float qy, float qz)
{
    return make_float4(KD_SHADOW - qx, KD_SHADOW - qy, KD_SHADOW - qz, 0.0f);
}

// the deformable constant influence is cut at the extent (tests/kpconv_deform_ref.py)
__device__ __forceinline__ float kd_h(float d2, const KpInfluence &f) { return kp_h<true>(d2, f); }

// g with  d h / d dk = g * (rel - dk);  linear at d2 == 0 (the reference: NaN) and at the clamp: 0
__device__ __forceinline__ float kd_dh(float d2, float h, const KpInfluence &f)
{
    if (f.mode == 1) return (h > 0.0f && d2 > 0.0f) ? f.inv_extent / __builtin_amdgcn_sqrtf(d2) : 0.0f;
    if (f.mode == 2) return h * (2.0f / f.gden);
    return 0.0f;
}

// first minimum over the four neighbour groups of a kernel-point lane (lanes k, k + 16, k + 32, k + 48)
__device__ __forceinline__ void kd_reduce_min(float &best, int &barg)
{
#pragma unroll
    for (int off = 16; off < 64; off <<= 1) {
        const float ob = __shfl_xor(best, off);
        const int oa = __shfl_xor(barg, off);
        if (ob < best || (ob == best && oa < barg)) {
            best = ob;
            barg = oa;
        }
    }
}

// ------------------------------------------------------------------------------------------------ forward, matrix pipe
template <int SMAX>  // most MFMA steps of four neighbours: 8 (Mn <= 32) or 16 (Mn <= 64)
__global__ __launch_bounds__(KP_BLOCK) void kpconv_deform_mfma_kernel(
    const float *__restrict__ query, const float *__restrict__ support, const int64_t *__restrict__ nbr,
    const float *__restrict__ feat, const float *__restrict__ kpts, const float *__restrict__ offsets,
    const float *__restrict__ mods, int64_t Nq, int64_t M, int Mn, int Cin, int KP, float extent, float ext2,
    int influence, int cpass, float *__restrict__ wf, float *__restrict__ kp_min, int *__restrict__ kp_arg)
{
    __shared__ __attribute__((aligned(16))) float4 s_rel[KP_BLOCK / 64][KP_NMAX];
    __shared__ int s_id[KP_BLOCK / 64][KP_NMAX];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t q = (int64_t)blockIdx.x * (KP_BLOCK / 64) + wave;
    if (q >= Nq) return;  // wave-uniform
    float4 *rel = s_rel[wave];
    int *ids = s_id[wave];
    const float qx = query[q * 3 + 0], qy = query[q * 3 + 1], qz = query[q * 3 + 2];
    const KpInfluence infl = kp_influence(extent, influence, ext2);
    const int steps = (Mn + 3) / 4;
    kp_fetch_neighbours(support, nbr + q * Mn, Mn, 64, M, qx, qy, qz, kd_shadow_rel(qx, qy, qz), rel, ids, lane);
    wave_lds_sync();
    const int k = lane & 15, nsub = lane >> 4;
    const bool kreal = k < KP;
    float kx = 0.0f, ky = 0.0f, kz = 0.0f;
    if (kreal) {  // this query's own kernel point: K_k + offset (torch.add(offsets, K_points), convolution_ops.py:156)
        const float *o = offsets + ((size_t)q * KP + k) * 3;
        kx = o[0] + kpts[k * 3 + 0];
        ky = o[1] + kpts[k * 3 + 1];
        kz = o[2] + kpts[k * 3 + 2];
    }
    float a[SMAX];
    unsigned roff[SMAX];  // float offset of the row gathered in step s (host: M * Cin < 2^30); row 0 stands in for shadows
    float best = 3.0e38f;
    int barg = 0;
#pragma unroll
    for (int s = 0; s < SMAX; ++s) {
        a[s] = 0.0f;
        roff[s] = 0;
        if (s < steps) {
            const int n = 4 * s + nsub;
            const float4 r = rel[n];
            const int id = ids[n];
            roff[s] = (unsigned)max(id, 0) * (unsigned)Cin;
            const float dx = r.x - kx, dy = r.y - ky, dz = r.z - kz;
            const float d2 = (dx * dx + dy * dy) + dz * dz;
            const bool valid = kreal && n < Mn;
            // in range of any deformed kernel point: the 16 kernel-point lanes of this neighbour
            const unsigned long long hit = __ballot(valid && d2 < ext2);
            const bool in_range = ((hit >> (16 * nsub)) & 0xffffull) != 0;
            if (valid && id >= 0 && in_range) a[s] = kd_h(d2, infl);
            if (valid && d2 < best) {
                best = d2;
                barg = n;
            }
        }
    }
    if (kp_min && blockIdx.y == 0) {
        kd_reduce_min(best, barg);
        if (nsub == 0 && kreal) {
            kp_min[q * KP + k] = best;
            if (kp_arg) kp_arg[q * KP + k] = barg;
        }
    }
    float modv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) modv[j] = mods ? mods[q * KP + min(4 * nsub + j, KP - 1)] : 1.0f;
    // gather the rows and accumulate on the matrix pipe, this grid row's channels, modulated on the way out
    const int c_lo = (int)blockIdx.y * cpass;
    kp_mfma_contract<SMAX>(feat, a, roff, steps, c_lo, min(Cin, c_lo + cpass), Cin, KP, lane, wf + (size_t)q * KP * Cin, modv);
}

// ------------------------------------------------------------------------------------- forward, per-lane FMA (any Mn)
__global__ __launch_bounds__(KP_BLOCK) void kpconv_deform_fma_kernel(
    const float *__restrict__ query, const float *__restrict__ support, const int64_t *__restrict__ nbr,
    const float *__restrict__ feat, const float *__restrict__ kpts, const float *__restrict__ offsets,
    const float *__restrict__ mods, int64_t Nq, int64_t M, int Mn, int Cin, int KP, float extent, float ext2,
    int influence, float *__restrict__ wf, float *__restrict__ kp_min, int *__restrict__ kp_arg)
{
    __shared__ __attribute__((aligned(16))) float s_w[KP_BLOCK / 64][KP_NCH][KP_MAX];
    __shared__ __attribute__((aligned(16))) float4 s_rel[KP_BLOCK / 64][KP_NCH];
    __shared__ int s_id[KP_BLOCK / 64][KP_NCH];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t q = (int64_t)blockIdx.x * (KP_BLOCK / 64) + wave;
    if (q >= Nq) return;  // wave-uniform
    float(*w)[KP_MAX] = s_w[wave];
    float4 *rel = s_rel[wave];
    int *ids = s_id[wave];
    const float qx = query[q * 3 + 0], qy = query[q * 3 + 1], qz = query[q * 3 + 2];
    const KpInfluence infl = kp_influence(extent, influence, ext2);
    const int k = lane & 15, nsub = lane >> 4;
    const bool kreal = k < KP;
    float kx = 0.0f, ky = 0.0f, kz = 0.0f;
    if (kreal) {
        const float *o = offsets + ((size_t)q * KP + k) * 3;
        kx = o[0] + kpts[k * 3 + 0];
        ky = o[1] + kpts[k * 3 + 1];
        kz = o[2] + kpts[k * 3 + 2];
    }
    float best = 3.0e38f;
    int barg = 0;
    const bool single_pass = Mn <= KP_NCH;  // then the weights of phase A serve every channel chunk
    for (int c0 = 0; c0 < Cin; c0 += 64) {
        float acc[KP_MAX];
#pragma unroll
        for (int kk = 0; kk < KP_MAX; ++kk) acc[kk] = 0.0f;
        const int c = c0 + lane;
        for (int n0 = 0; n0 < Mn; n0 += KP_NCH) {
            const int cnt = min(KP_NCH, Mn - n0);
            const int cntg = (cnt + KP_GROUP - 1) / KP_GROUP * KP_GROUP;  // rows [cnt, cntg): zero weights
            if (!(single_pass && c0 > 0)) {
                kp_fetch_neighbours(support, nbr + q * Mn + n0, cnt, cntg, M, qx, qy, qz, kd_shadow_rel(qx, qy, qz), rel, ids,
                                    lane);
                wave_lds_sync();
                for (int n = nsub; n < cntg; n += 4) {  // the same trip count in every lane: cntg is a multiple of 16
                    const float4 r = rel[n];
                    const float dx = r.x - kx, dy = r.y - ky, dz = r.z - kz;
                    const float d2 = (dx * dx + dy * dy) + dz * dz;
                    const bool valid = kreal && n < cnt;
                    const unsigned long long hit = __ballot(valid && d2 < ext2);
                    const bool in_range = ((hit >> (16 * nsub)) & 0xffffull) != 0;
                    w[n][k] = (valid && ids[n] >= 0 && in_range) ? kd_h(d2, infl) : 0.0f;
                    if (c0 == 0 && valid && d2 < best) {
                        best = d2;
                        barg = n0 + n;
                    }
                }
                wave_lds_sync();
            }
            if (c < Cin) kp_fma_rows(feat, ids, w, cntg, Cin, c, acc);
            wave_lds_sync();
        }
        if (c < Cin) {
#pragma unroll
            for (int kk = 0; kk < KP_MAX; ++kk)
                if (kk < KP) wf[((size_t)q * KP + kk) * Cin + c] = acc[kk] * (mods ? mods[q * KP + kk] : 1.0f);
        }
    }
    if (kp_min) {
        kd_reduce_min(best, barg);
        if (nsub == 0 && kreal) {
            kp_min[q * KP + k] = best;
            if (kp_arg) kp_arg[q * KP + k] = barg;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ backward
// One wave per query, the neighbours in chunks of 64.  Per chunk:
//  (b) w[n][k] = mod[k] * in_range[n] * h(d2[n,k]) in LDS (phase A of the forward) and the mask of every neighbour;
//  (c) per-slot rows  g[q,n,:] = sum_k w[n][k] * d_wf[q,k,:]                 (16 x 4-step MFMA per 16 x 16 tile),
//      summed per support point afterwards (gather_slot_rows);
//  (d) S[k][n] = sum_c d_wf[q,k,c] * x[nbr[q,n],c]  on the matrix pipe: channels are the contraction index, each
//      lane group takes four consecutive channels of a step of 16 (float4 loads of both operands), result
//      S[k = 4 (lane >> 4) + j][n = 16 nb + (lane & 15)];  then in registers
//        d_mod[k] += in_range[n] * h * S,   d_off[k] += mod[k] * in_range[n] * S * dh/d dk,
//      reduced over the 16 neighbour lanes by a fixed xor tree.
// The arg-min term  d_kp_min[k] * (-2) (rel[arg] - dk)  is added by the storing lane.
template <bool VEC4>
__global__ __launch_bounds__(KP_BLOCK) void kpconv_deform_bwd_kernel(
    const float *__restrict__ query, const float *__restrict__ support, const int64_t *__restrict__ nbr,
    const float *__restrict__ feat, const float *__restrict__ kpts, const float *__restrict__ offsets,
    const float *__restrict__ mods, const float *__restrict__ d_wf, const float *__restrict__ d_kp_min,
    const int *__restrict__ kp_arg, int64_t Nq, int64_t M, int Mn, int Cin, int KP, float extent, float ext2,
    int influence, float *__restrict__ gslots, float *__restrict__ d_off, float *__restrict__ d_mod)
{
    __shared__ float s_w[KP_BLOCK / 64][KP_NMAX][KD_WPAD];
    __shared__ __attribute__((aligned(16))) float4 s_rel[KP_BLOCK / 64][KP_NMAX];
    __shared__ __attribute__((aligned(16))) float4 s_dk[KP_BLOCK / 64][KP_MAX];  // deformed kernel point, modulation
    __shared__ int s_id[KP_BLOCK / 64][KP_NMAX];
    __shared__ float s_msk[KP_BLOCK / 64][KP_NMAX];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t q = (int64_t)blockIdx.x * (KP_BLOCK / 64) + wave;
    if (q >= Nq) return;  // wave-uniform
    float(*w)[KD_WPAD] = s_w[wave];
    float4 *rel = s_rel[wave];
    float4 *dkp = s_dk[wave];
    int *ids = s_id[wave];
    float *msk = s_msk[wave];
    const float qx = query[q * 3 + 0], qy = query[q * 3 + 1], qz = query[q * 3 + 2];
    const KpInfluence infl = kp_influence(extent, influence, ext2);
    const int k16 = lane & 15, g = lane >> 4;
    const bool kreal = k16 < KP;
    float kx = 0.0f, ky = 0.0f, kz = 0.0f, kmod = 0.0f;
    if (kreal) {
        const float *o = offsets + ((size_t)q * KP + k16) * 3;
        kx = o[0] + kpts[k16 * 3 + 0];
        ky = o[1] + kpts[k16 * 3 + 1];
        kz = o[2] + kpts[k16 * 3 + 2];
        kmod = mods ? mods[q * KP + k16] : 1.0f;
    }
    if (lane < KP_MAX) dkp[lane] = make_float4(kx, ky, kz, kmod);
    const float *__restrict__ dq = d_wf + (size_t)q * KP * Cin;  // this query's (KP, Cin) gradient block
    float gx[4], gy[4], gz[4], gm[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) gx[j] = gy[j] = gz[j] = gm[j] = 0.0f;

    for (int n0 = 0; n0 < Mn; n0 += KP_NMAX) {
        const int cnt = min(KP_NMAX, Mn - n0);
        const int nblk = (cnt + 15) / 16;  // 16-neighbour blocks (wave-uniform)
        kp_fetch_neighbours(support, nbr + q * Mn + n0, cnt, 64, M, qx, qy, qz, kd_shadow_rel(qx, qy, qz), rel, ids, lane);
        wave_lds_sync();
        // (b) weights and masks, lane = (kernel point k16, neighbour 4 s + g)
        for (int s = 0; s < 4 * nblk; ++s) {
            const int n = 4 * s + g;
            const float4 r = rel[n];
            const float dx = r.x - kx, dy = r.y - ky, dz = r.z - kz;
            const float d2 = (dx * dx + dy * dy) + dz * dz;
            const bool valid = kreal && n < cnt;
            const unsigned long long hit = __ballot(valid && d2 < ext2);
            const bool live = ((hit >> (16 * g)) & 0xffffull) != 0 && ids[n] >= 0;
            w[n][k16] = (valid && live) ? kd_h(d2, infl) * kmod : 0.0f;
            if (k16 == 0) msk[n] = live ? 1.0f : 0.0f;
        }
        wave_lds_sync();
        // (c) per-slot gradient rows
        if (gslots) {
            float aw[4][4];  // A operand: w[n = 16 nb + k16][k = 4 s + g]
#pragma unroll
            for (int nb = 0; nb < 4; ++nb)
#pragma unroll
                for (int s = 0; s < 4; ++s) aw[nb][s] = nb < nblk ? w[16 * nb + k16][4 * s + g] : 0.0f;
            for (int c0 = 0; c0 < Cin; c0 += 16) {
                const int c = c0 + k16;
                float bd[4];  // B operand: d_wf[k = 4 s + g][c]
#pragma unroll
                for (int s = 0; s < 4; ++s) bd[s] = (4 * s + g < KP && c < Cin) ? dq[(size_t)(4 * s + g) * Cin + c] : 0.0f;
#pragma unroll
                for (int nb = 0; nb < 4; ++nb)
                    if (nb < nblk) {
                        f32x4 acc = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                        for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(aw[nb][s], bd[s], acc, 0, 0, 0);
#pragma unroll
                        for (int j = 0; j < 4; ++j) {  // D[n = 16 nb + 4 g + j][c]
                            const int n = 16 * nb + 4 * g + j;
                            if (n < cnt && c < Cin) gslots[((size_t)q * Mn + n0 + n) * Cin + c] = acc[j];
                        }
                    }
            }
        }
        // (d) sensitivities S[k][n] over the channels, then the offset / modulation gradients
        f32x4 sacc[4];
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) sacc[nb] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
        int idn[4];
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) idn[nb] = nb < nblk ? ids[16 * nb + k16] : -1;
        for (int t0 = 0; t0 < Cin; t0 += 16) {
            const int c = t0 + 4 * g;
            float dv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (kreal) {
                if (VEC4) {
                    if (c < Cin) {
                        const float4 t = *reinterpret_cast<const float4 *>(dq + (size_t)k16 * Cin + c);
                        dv[0] = t.x, dv[1] = t.y, dv[2] = t.z, dv[3] = t.w;
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (c + j < Cin) dv[j] = dq[(size_t)k16 * Cin + c + j];
                }
            }
#pragma unroll
            for (int nb = 0; nb < 4; ++nb)
                if (nb < nblk) {
                    float fv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                    if (idn[nb] >= 0) {
                        const float *row = feat + (size_t)idn[nb] * Cin + c;
                        if (VEC4) {
                            if (c < Cin) {
                                const float4 t = *reinterpret_cast<const float4 *>(row);
                                fv[0] = t.x, fv[1] = t.y, fv[2] = t.z, fv[3] = t.w;
                            }
                        } else {
#pragma unroll
                            for (int j = 0; j < 4; ++j)
                                if (c + j < Cin) fv[j] = row[j];
                        }
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        sacc[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(dv[j], fv[j], sacc[nb], 0, 0, 0);
                }
        }
#pragma unroll
        for (int nb = 0; nb < 4; ++nb)
            if (nb < nblk) {
                const int n = 16 * nb + k16;
                const float4 r = rel[n];
                const float m = msk[n];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float4 p = dkp[4 * g + j];
                    const float dx = r.x - p.x, dy = r.y - p.y, dz = r.z - p.z;
                    const float d2 = (dx * dx + dy * dy) + dz * dz;
                    const float h = kd_h(d2, infl);
                    const float sraw = sacc[nb][j] * m;
                    gm[j] += sraw * h;
                    const float sv = sraw * p.w * kd_dh(d2, h, infl);
                    gx[j] += sv * dx;
                    gy[j] += sv * dy;
                    gz[j] += sv * dz;
                }
            }
        wave_lds_sync();  // the next chunk overwrites the tiles
    }
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            gx[j] += __shfl_xor(gx[j], off);
            gy[j] += __shfl_xor(gy[j], off);
            gz[j] += __shfl_xor(gz[j], off);
            gm[j] += __shfl_xor(gm[j], off);
        }
    }
    if (k16 == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = 4 * g + j;
            if (k < KP) {
                float ox = gx[j], oy = gy[j], oz = gz[j];
                if (d_kp_min) {  // min_n d2[n,k] -> the arg-min slot (shadow slots included, at 1e6)
                    const float gk = d_kp_min[q * KP + k];
                    const int n = min(max(kp_arg[q * KP + k], 0), Mn - 1);
                    const int64_t id = nbr[q * Mn + n];
                    float rx = KD_SHADOW - qx, ry = KD_SHADOW - qy, rz = KD_SHADOW - qz;
                    if (id >= 0 && id < M) {
                        rx = support[id * 3 + 0] - qx;
                        ry = support[id * 3 + 1] - qy;
                        rz = support[id * 3 + 2] - qz;
                    }
                    const float4 p = dkp[k];
                    ox += -2.0f * gk * (rx - p.x);
                    oy += -2.0f * gk * (ry - p.y);
                    oz += -2.0f * gk * (rz - p.z);
                }
                float *o = d_off + ((size_t)q * KP + k) * 3;
                o[0] = ox;
                o[1] = oy;
                o[2] = oz;
                if (d_mod) d_mod[q * KP + k] = gm[j];
            }
        }
    }
}

}  // namespace tp3d

using namespace tp3d;

static inline float kd_ext2(float extent) { return (float)((double)extent * (double)extent); }

TP3D_EXPORT int tp3d_kpconv_deform_weighted_f32(const float *query, const float *support, const int64_t *neighbors,
                                                const float *features, const float *k_points, const float *offsets,
                                                const float *modulations, int64_t Nq, int64_t M, int Mn, int Cin, int KP,
                                                float extent, int influence, float *weighted, float *kp_min_d2,
                                                int32_t *kp_argmin, void *stream)
{
    if (int rc = kp_check_args(Nq, M, Mn, Cin, KP, influence, 1)) return rc;
    if (Nq == 0) return TP3D_OK;
    if (!query || !support || !neighbors || !features || !k_points || !offsets || !weighted) return TP3D_E_BADARG;
    if (kp_argmin && !kp_min_d2) return TP3D_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    const float ext2 = kd_ext2(extent);
    const KpMfmaRoute r = kp_mfma_route(Nq, M, Mn, Cin);
    if (r.ok && !r.wide)
        hipLaunchKernelGGL(kpconv_deform_mfma_kernel<8>, r.grid, dim3(KP_BLOCK), 0, s, query, support, neighbors, features,
                           k_points, offsets, modulations, Nq, M, Mn, Cin, KP, extent, ext2, influence, r.cpass, weighted,
                           kp_min_d2, kp_argmin);
    else if (r.ok)
        hipLaunchKernelGGL(kpconv_deform_mfma_kernel<16>, r.grid, dim3(KP_BLOCK), 0, s, query, support, neighbors, features,
                           k_points, offsets, modulations, Nq, M, Mn, Cin, KP, extent, ext2, influence, r.cpass, weighted,
                           kp_min_d2, kp_argmin);
    else
        hipLaunchKernelGGL(kpconv_deform_fma_kernel, kp_query_grid(Nq), dim3(KP_BLOCK), 0, s, query, support, neighbors,
                           features, k_points, offsets, modulations, Nq, M, Mn, Cin, KP, extent, ext2, influence, weighted,
                           kp_min_d2, kp_argmin);
    return check_launch();
}

TP3D_EXPORT int tp3d_kpconv_deform_bwd_f32(const float *query, const float *support, const int64_t *neighbors,
                                           const float *features, const float *k_points, const float *offsets,
                                           const float *modulations, const float *d_weighted, const float *d_kp_min_d2,
                                           const int32_t *kp_argmin, int64_t Nq, int64_t M, int Mn, int Cin, int KP,
                                           float extent, int influence, float *d_features, float *d_offsets,
                                           float *d_modulations, void *inverse, size_t inverse_bytes, int inverse_ready,
                                           void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = kp_check_args(Nq, M, Mn, Cin, KP, influence, 1)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (Nq == 0) return d_features ? zero_async(d_features, (size_t)M * Cin * sizeof(float), s) : TP3D_OK;
    if (!query || !support || !neighbors || !features || !k_points || !offsets || !d_weighted || !d_offsets)
        return TP3D_E_BADARG;
    if (d_kp_min_d2 && !kp_argmin) return TP3D_E_BADARG;
    if (d_modulations && !modulations) return TP3D_E_BADARG;
    const int64_t slots = Nq * Mn;
    if (slots > INT32_MAX || M > INT32_MAX / 2) return TP3D_E_TOOBIG;
    int *start = nullptr, *order = nullptr;
    float *g = nullptr;
    if (d_features) {
        if (!inverse || !workspace) return TP3D_E_BADARG;
        if (inverse_bytes < tp3d_kpconv_bwd_workspace_bytes(M, slots)) return TP3D_E_BADARG;
        if (workspace_bytes < tp3d_kpconv_grad_workspace_bytes(M, slots, Cin)) return TP3D_E_BADARG;
        if (int rc = invert_neighbors(neighbors, slots, M, inverse, &start, &order, s, inverse_ready != 0)) return rc;
        g = static_cast<float *>(workspace);
    }
    const float ext2 = kd_ext2(extent);
    const bool vec4 = Cin % 4 == 0 && ((uintptr_t)features % 16 == 0) && ((uintptr_t)d_weighted % 16 == 0);
    if (vec4)
        hipLaunchKernelGGL(kpconv_deform_bwd_kernel<true>, kp_query_grid(Nq), dim3(KP_BLOCK), 0, s, query, support,
                           neighbors, features, k_points, offsets, modulations, d_weighted, d_kp_min_d2, kp_argmin, Nq, M, Mn,
                           Cin, KP, extent, ext2, influence, g, d_offsets, d_modulations);
    else
        hipLaunchKernelGGL(kpconv_deform_bwd_kernel<false>, kp_query_grid(Nq), dim3(KP_BLOCK), 0, s, query, support,
                           neighbors, features, k_points, offsets, modulations, d_weighted, d_kp_min_d2, kp_argmin, Nq, M, Mn,
                           Cin, KP, extent, ext2, influence, g, d_offsets, d_modulations);
    if (int rc = check_launch()) return rc;
    if (d_features) return gather_slot_rows(g, start, order, M, Cin, d_features, s);
    return TP3D_OK;
}
