// Neighbour max-pool, the strided shortcut of the KPConv residual blocks: forward over the neighbour table, backward as
// a per-support-point sum through the inverted table (inverse_table.h) -- no float atomics.
#include "inverse_table.h"

namespace tp3d {

constexpr int NBR_BLOCK = 256;  // 4 waves, one support point per wave in the backward kernel

// Strided shortcut of ResnetBBlock (reference modules/KPConv/blocks.py:206-210): max over each query's neighbours of
// the support features, a shadow neighbour (-1 or >= M) contributing the zero row.  arg = winning slot (first max).
__global__ __launch_bounds__(256) void nbr_maxpool_kernel(const float *__restrict__ x, const int64_t *__restrict__ nbr,
                                                           int64_t Nq, int64_t M, int Mn, int C, float *__restrict__ out,
                                                           int *__restrict__ arg)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= Nq * C) return;
    const int64_t q = t / C;
    const int c = (int)(t - q * C);
    float best = -3.4028235e38f;
    int barg = 0;
    for (int n = 0; n < Mn; ++n) {
        const int64_t m = nbr[q * Mn + n];
        const float v = (m >= 0 && m < M) ? x[m * C + c] : 0.0f;
        if (v > best) {
            best = v;
            barg = n;
        }
    }
    out[t] = best;
    if (arg) arg[t] = barg;
}

// d_x[m, c] = sum over the slots (q, n) referencing m (ascending) with arg[q, c] == n of g[q, c]; one wave per point
__global__ __launch_bounds__(NBR_BLOCK) void nbr_maxpool_bwd_kernel(const float *__restrict__ g, const int *__restrict__ arg,
                                                                    const int *__restrict__ start,
                                                                    const int *__restrict__ order, int64_t M, int Mn,
                                                                    int C, float *__restrict__ d_x)
{
    const int lane = threadIdx.x & 63;
    const int64_t m = (int64_t)blockIdx.x * (NBR_BLOCK / 64) + (threadIdx.x >> 6);
    if (m >= M) return;
    const int s0 = start[m], s1 = start[m + 1];
    for (int c = lane; c < C; c += 64) {
        float acc = 0.0f;
        for (int j = s0; j < s1; ++j) {
            const int slot = order[j];
            const int64_t q = slot / Mn;
            const int n = slot - (int)q * Mn;
            if (arg[q * C + c] == n) acc += g[q * C + c];
        }
        d_x[m * C + c] = acc;
    }
}

}  // namespace tp3d

TP3D_EXPORT int tp3d_nbr_maxpool_fwd_f32(const float *x, const int64_t *neighbors, int64_t Nq, int64_t M, int Mn, int C,
                                         float *out, int32_t *argmax, void *stream)
{
    if (Nq < 0 || M < 0 || Mn <= 0 || C <= 0) return TP3D_E_BADARG;
    if (Nq == 0) return TP3D_OK;
    if (!neighbors || !out || (M > 0 && !x)) return TP3D_E_BADARG;
    const int64_t blocks = (Nq * C + 255) / 256;
    if (blocks > 0x7fffffff) return TP3D_E_TOOBIG;
    hipLaunchKernelGGL(tp3d::nbr_maxpool_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, neighbors, Nq,
                       M, Mn, C, out, argmax);
    return tp3d::check_launch();
}

TP3D_EXPORT int tp3d_nbr_maxpool_bwd_f32(const float *grad_out, const int32_t *argmax, const int64_t *neighbors, int64_t Nq,
                                         int64_t M, int Mn, int C, float *d_x, void *inverse, size_t inverse_bytes,
                                         int inverse_ready, void *stream)
{
    if (Nq < 0 || M < 0 || Mn <= 0 || C <= 0) return TP3D_E_BADARG;
    if (M == 0) return TP3D_OK;
    if (!d_x) return TP3D_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    const int64_t slots = Nq * Mn;
    if (slots == 0) return tp3d::zero_async(d_x, (size_t)M * C * sizeof(float), s);
    if (!grad_out || !argmax || !neighbors || !inverse) return TP3D_E_BADARG;
    if (slots > INT32_MAX || M > INT32_MAX / 2) return TP3D_E_TOOBIG;
    if (inverse_bytes < tp3d_kpconv_bwd_workspace_bytes(M, slots)) return TP3D_E_BADARG;
    int *start = nullptr, *order = nullptr;
    if (int rc = tp3d::invert_neighbors(neighbors, slots, M, inverse, &start, &order, s, inverse_ready != 0)) return rc;
    hipLaunchKernelGGL(tp3d::nbr_maxpool_bwd_kernel, dim3((unsigned)((M + tp3d::NBR_BLOCK / 64 - 1) / (tp3d::NBR_BLOCK / 64))),
                       dim3(tp3d::NBR_BLOCK), 0, s, grad_out, argmax, start, order, M, Mn, C, d_x);
    return tp3d::check_launch();
}
