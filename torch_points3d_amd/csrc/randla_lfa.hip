// RandLA-Net local feature aggregation in eval mode, one kernel (DESIGN.md "RandLA-Net: fused edge pass").
//
// Reference: torch_points3d/modules/RandLANet/modules.py:29-52 (RandlaKernel.message + aggr="add").  In eval mode
// BatchNorm is an affine map per channel, so the chain of one edge
//   relative position (10) -> point_pos_nn (P1, P2) -> [x_j | rij] (C) -> attention_nn (A1, C) -> softmax_c -> * [x_j | rij]
// depends on no other edge, and a query's k = 16 edges are one 16-row tile of v_mfma_f32_16x16x4_f32.  One wave owns a
// query: its tiles live in the wave's own slice of LDS, nothing of size E = Nq * 16 is written to memory.  The four
// weight matrices (with their folded scale / shift) are staged once per workgroup; workgroups walk the queries with a
// grid stride.  Products are genuine fp32 (the f32-input MFMA is an fmaf chain); no atomics, one writer per output
// row, the 16 messages of a query are summed in slot order.
#include "tp3d_common.h"

namespace tp3d {

typedef float lfa_f32x4 __attribute__((ext_vector_type(4)));

constexpr int LFA_K = 16;      // neighbours per query = rows of the tile
constexpr int LFA_WAVES = 4;   // queries in flight per workgroup
constexpr int LFA_CMAX = 64;   // C = Cx + P2, P1, P2
constexpr int LFA_AMAX = 128;  // A1
constexpr int LFA_LDS_MAX = 160 * 1024;

// The contraction index is walked in blocks of 16: in block b, MFMA step s, lane (row, g) supplies column
// 16 b + 4 g + s of its row of A and of W -- the same permutation of k on both operands, so the product is the same
// sum -- and one 16-byte LDS read per operand feeds four MFMAs.  K is therefore padded to a multiple of 16 with zero
// columns, and the row stride of a tile is that plus 4 floats: rows stay 16-byte aligned and consecutive rows start
// in different banks.
__host__ __device__ constexpr int lfa_pad16(int K) { return (K + 15) & ~15; }
__host__ __device__ constexpr int lfa_ld(int K) { return lfa_pad16(K) + 4; }
__host__ __device__ constexpr int lfa_max(int a, int b) { return a > b ? a : b; }

// LDS carve (floats).  consts, dense, in this order per layer l = 1..4: W_l (N_l x K_l), scale_l (N_l), shift_l (N_l)
struct LfaPlan {
    int Cx, P1, P2, A1, C;
    int ldw[4], K[4], N[4];
    int w[4], s[4], t[4];  // offsets of the staged matrices / vectors
    int src[4];            // offsets of W_l in the dense consts buffer (scale and shift follow it)
    int ldF, ldA;          // per-wave tiles: F (16 x ldF) relative positions, then [x_j | rij]; A (16 x ldA) hidden rows, messages
    int tiles;             // offset of the first wave's tiles
    int total;             // floats of LDS per workgroup
};

__host__ __device__ inline LfaPlan lfa_plan(int Cx, int P1, int P2, int A1)
{
    LfaPlan p;
    p.Cx = Cx, p.P1 = P1, p.P2 = P2, p.A1 = A1, p.C = Cx + P2;
    p.K[0] = 10, p.N[0] = P1;
    p.K[1] = P1, p.N[1] = P2;
    p.K[2] = p.C, p.N[2] = A1;
    p.K[3] = A1, p.N[3] = p.C;
    int at = 0, from = 0;
    for (int l = 0; l < 4; ++l) {
        p.ldw[l] = lfa_ld(p.K[l]);
        p.w[l] = at, at += p.N[l] * p.ldw[l];
        p.s[l] = at, at += p.N[l];
        p.t[l] = at, at += p.N[l];
        at = (at + 3) & ~3;
        p.src[l] = from, from += p.N[l] * p.K[l] + 2 * p.N[l];
    }
    p.ldF = lfa_ld(p.C);
    p.ldA = lfa_ld(lfa_max(lfa_max(P1, A1), p.C));
    p.tiles = at;
    p.total = at + LFA_WAVES * LFA_K * (p.ldF + p.ldA);
    return p;
}

// the wave's own LDS writes have landed before its next reads (the tiles are private to the wave)
__device__ __forceinline__ void lfa_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// One 16-column block of D = A W^T: A (16 x K16) at a (stride lda), W rows [n0, n0 + 16) at w (stride ldw; rows past
// N are clamped, their columns are discarded by the caller).  Lane l = (row l & 15, g = l >> 4) reads columns
// [16 b + 4 g, 16 b + 4 g + 4) of its rows; it receives D[4 g + r][n0 + (l & 15)], r = 0..3.  Two accumulators keep
// the matrix pipe busy across the 40-cycle dependent latency.
__device__ __forceinline__ lfa_f32x4 lfa_block(const float *a, int lda, const float *w, int ldw, int K16, int N, int n0,
                                               int lane)
{
    const int i16 = lane & 15, g = lane >> 4;
    const int wr = n0 + i16 < N ? n0 + i16 : N - 1;
    const float4 *ap = reinterpret_cast<const float4 *>(a + i16 * lda + 4 * g);
    const float4 *wp = reinterpret_cast<const float4 *>(w + wr * ldw + 4 * g);
    lfa_f32x4 acc0 = {0.0f, 0.0f, 0.0f, 0.0f}, acc1 = acc0;
    for (int b = 0; b < K16 / 16; ++b) {
        const float4 av = ap[4 * b], wv = wp[4 * b];
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, wv.x, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, wv.y, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, wv.z, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, wv.w, acc1, 0, 0, 0);
    }
    return acc0 + acc1;
}

__device__ __forceinline__ float lfa_act(float v, float sc, float sh)
{
    v = v * sc + sh;
    return v > 0.0f ? v : 0.2f * v;
}

// dst[row][col0 + c] = LeakyReLU(scale * (A W^T) + shift) for c < N; the columns [col0 + N, pad16(col0 + N)), which
// the next layer's K-loop reads, are zeroed (pad16(col0 + N) < the tile's stride)
__device__ __forceinline__ void lfa_layer(const float *a, int lda, const float *w, int ldw, int K, int N, const float *sc,
                                          const float *sh, float *dst, int ldd, int col0, int lane)
{
    const int i16 = lane & 15, g = lane >> 4, K16 = lfa_pad16(K);
    const int end = lfa_pad16(col0 + N) - col0;
    for (int n0 = 0; n0 < end; n0 += 16) {
        const int c = n0 + i16;
        const bool live = c < N;
        lfa_f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
        if (n0 < N) acc = lfa_block(a, lda, w, ldw, K16, N, n0, lane);
        const float s = live ? sc[c] : 0.0f, t = live ? sh[c] : 0.0f;
        if (c < end) {
#pragma unroll
            for (int r = 0; r < 4; ++r) dst[(4 * g + r) * ldd + col0 + c] = live ? lfa_act(acc[r], s, t) : 0.0f;
        }
    }
}

__device__ __forceinline__ float lfa_max16(float v)
{
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ float lfa_sum16(float v)
{
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) v += __shfl_xor(v, off);
    return v;
}

// row of the support that is neighbour `slot` of query q; the caller refuses tables with holes, and whatever the table
// holds nothing is read out of bounds
__device__ __forceinline__ int64_t lfa_nbr_row(const int64_t *__restrict__ nbr, int64_t q, int slot, int64_t M)
{
    const int64_t j = nbr[q * LFA_K + slot];
    return j < 0 ? 0 : (j >= M ? M - 1 : j);
}

__global__ __launch_bounds__(LFA_WAVES * 64) void randla_lfa_eval_kernel(
    const float *__restrict__ pos_q, const float *__restrict__ pos_s, const float *__restrict__ x,
    const int64_t *__restrict__ nbr, int64_t Nq, int64_t M, int Cx, int P1, int P2, int A1,
    const float *__restrict__ consts, float *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) float lfa_lds[];
    const LfaPlan p = lfa_plan(Cx, P1, P2, A1);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i16 = lane & 15, g = lane >> 4;
    const int C = p.C;

    // ---- weights: dense rows -> padded rows (zero beyond K), scale, shift
    for (int l = 0; l < 4; ++l) {
        const int K = p.K[l], N = p.N[l], ldw = p.ldw[l];
        const float *src = consts + p.src[l];
        for (int i = tid; i < N * ldw; i += LFA_WAVES * 64) {
            const int n = i / ldw, k = i - n * ldw;
            lfa_lds[p.w[l] + i] = k < K ? src[n * K + k] : 0.0f;
        }
        for (int i = tid; i < 2 * N; i += LFA_WAVES * 64) lfa_lds[p.s[l] + i] = src[N * K + i];  // t follows s in both
    }
    __syncthreads();

    float *F = lfa_lds + p.tiles + wave * LFA_K * (p.ldF + p.ldA);
    float *A = F + LFA_K * p.ldF;
    const int ldF = p.ldF, ldA = p.ldA;
    const float *W1 = lfa_lds + p.w[0], *W2 = lfa_lds + p.w[1], *W3 = lfa_lds + p.w[2], *W4 = lfa_lds + p.w[3];

    // (Fetching the next query's rows and positions one query ahead and holding the feature rows in registers across
    // layer 1 was tried: 163 VGPRs instead of 92 halve the waves per SIMD and the pass got slower at every level.)
    for (int64_t q = (int64_t)blockIdx.x * LFA_WAVES + wave; q < Nq; q += (int64_t)gridDim.x * LFA_WAVES) {
        // ---- relative position rows [pos_i, pos_j, pos_i - pos_j, |.|, 0 x 6] of the 16 edges -> F[:, 0:16]
        const int64_t j = lfa_nbr_row(nbr, q, i16, M);  // lane l holds edge l & 15
        if (lane < LFA_K) {
            const float qx = pos_q[q * 3 + 0], qy = pos_q[q * 3 + 1], qz = pos_q[q * 3 + 2];
            const float sx = pos_s[j * 3 + 0], sy = pos_s[j * 3 + 1], sz = pos_s[j * 3 + 2];
            const float dx = qx - sx, dy = qy - sy, dz = qz - sz;
            float4 *row = reinterpret_cast<float4 *>(F + lane * ldF);
            row[0] = make_float4(qx, qy, qz, sx);
            row[1] = make_float4(sy, sz, dx, dy);
            row[2] = make_float4(dz, sqrtf((dx * dx + dy * dy) + dz * dz), 0.0f, 0.0f);
            row[3] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
        lfa_lds_sync();
        // ---- point_pos_nn layer 1: F[:, 0:10] -> A[:, 0:P1]
        lfa_layer(F, ldF, W1, p.ldw[0], 10, P1, lfa_lds + p.s[0], lfa_lds + p.t[0], A, ldA, 0, lane);
        lfa_lds_sync();
        // ---- F = [x_j | rij | 0]: the gather of the neighbours' feature rows, then point_pos_nn layer 2
        for (int i0 = 0; i0 < LFA_K * Cx; i0 += 64) {
            const int i = i0 + lane;
            const int e = i / Cx < LFA_K ? i / Cx : LFA_K - 1;
            const int64_t je = __shfl(j, e);  // lane e holds the row of edge e
            if (i < LFA_K * Cx) F[e * ldF + (i - e * Cx)] = x[je * Cx + (i - e * Cx)];
        }
        lfa_layer(A, ldA, W2, p.ldw[1], P1, P2, lfa_lds + p.s[1], lfa_lds + p.t[1], F, ldF, Cx, lane);
        lfa_lds_sync();
        // ---- attention_nn layer 1: F[:, 0:C] -> A[:, 0:A1]
        lfa_layer(F, ldF, W3, p.ldw[2], C, A1, lfa_lds + p.s[2], lfa_lds + p.t[2], A, ldA, 0, lane);
        lfa_lds_sync();
        // ---- attention_nn layer 2 -> g (16 x C) in registers: lane (i16, g) holds g[4 g + r][16 nb + i16]
        float gv[4][4];
        const int K16 = lfa_pad16(A1);
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            const int c = 16 * nb + i16;
            const bool live = c < C;
            lfa_f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
            if (16 * nb < C) acc = lfa_block(A, ldA, W4, p.ldw[3], K16, C, 16 * nb, lane);
            const float s = live ? lfa_lds[p.s[3] + c] : 0.0f, t = live ? lfa_lds[p.t[3] + c] : 0.0f;
#pragma unroll
            for (int r = 0; r < 4; ++r) gv[nb][r] = live ? lfa_act(acc[r], s, t) : -INFINITY;
        }
        lfa_lds_sync();  // every lane is done reading A
        // ---- softmax over the channels of each edge row, message = s * F -> A[:, 0:C]
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float m = fmaxf(fmaxf(gv[0][r], gv[1][r]), fmaxf(gv[2][r], gv[3][r]));
            m = lfa_max16(m);
            float z = 0.0f;
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) {
                gv[nb][r] = 16 * nb + i16 < C ? expf(gv[nb][r] - m) : 0.0f;
                z += gv[nb][r];
            }
            z = lfa_sum16(z);
            const float inv = 1.0f / z;
            const int row = 4 * g + r;
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) {
                const int c = 16 * nb + i16;
                if (c < C) A[row * ldA + c] = (gv[nb][r] * inv) * F[row * ldF + c];
            }
        }
        lfa_lds_sync();
        // ---- sum over the 16 edges in slot order; lane c owns out[q, c]
        if (lane < C) {
            float acc = 0.0f;
#pragma unroll
            for (int e = 0; e < LFA_K; ++e) acc += A[e * ldA + lane];
            out[q * C + lane] = acc;
        }
        lfa_lds_sync();
    }
}

}  // namespace tp3d

using namespace tp3d;

TP3D_EXPORT int tp3d_randla_lfa_eval_f32(const float *pos_q, const float *pos_s, const float *x, const int64_t *nbr,
                                         int64_t Nq, int64_t M, int k, int Cx, int P1, int P2, int A1, const float *consts,
                                         float *out, void *stream)
{
    if (Nq < 0 || M < 0 || Cx <= 0 || P1 <= 0 || P2 <= 0 || A1 <= 0) return TP3D_E_BADARG;
    if (k != LFA_K) return TP3D_E_BADARG;
    if (Cx + P2 > LFA_CMAX || P1 > LFA_CMAX || P2 > LFA_CMAX || A1 > LFA_AMAX) return TP3D_E_TOOBIG;
    if (!x && Cx != 3) return TP3D_E_BADARG;  // without features the neighbour's position is its feature row
    if (Nq == 0) return TP3D_OK;
    if (!pos_q || !pos_s || !nbr || !consts || !out || M == 0) return TP3D_E_BADARG;
    const LfaPlan p = lfa_plan(Cx, P1, P2, A1);
    const int bytes = p.total * (int)sizeof(float);
    if (bytes > LFA_LDS_MAX) return TP3D_E_TOOBIG;
    static int cus[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    if (!cus[dev]) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cus[dev] = n;
    }
    int per_cu = LFA_LDS_MAX / bytes;  // workgroups the LDS lets a CU hold; the registers allow 4 waves per SIMD
    per_cu = per_cu > 4 ? 4 : per_cu;
    int64_t grid = (Nq + LFA_WAVES - 1) / LFA_WAVES;
    if (grid > (int64_t)cus[dev] * per_cu) grid = (int64_t)cus[dev] * per_cu;
    allow_large_dynamic_lds<&randla_lfa_eval_kernel>(LFA_LDS_MAX);
    hipLaunchKernelGGL(randla_lfa_eval_kernel, dim3((unsigned)grid), dim3(LFA_WAVES * 64), (size_t)bytes,
                       (hipStream_t)stream, pos_q, pos_s, x ? x : pos_s, nbr, Nq, M, Cx, P1, P2, A1, consts, out);
    return check_launch();
}
