// Multi-scale fusion (the head of MS-SVConv, models/registration/ms_svconv3d.py apply_nn): every scale's rows are
// L2-normalised, xhat_s = x_s / (||x_s||_2 + eps), then concatenated, or max / mean pooled across the scales.  One launch
// forward, one backward.  A group of G lanes (8, 16, 32 or 64, the least that covers C) owns a row; the squared norm and
// the backward's <g, x> are butterfly sums over the group, so every lane holds the same bits and a repeat is bit-equal.
// No atomics.
#include "tp3d_common.h"

namespace tp3d {

constexpr int SF_BLOCK = 256;
constexpr int SF_MAX_S = 8;
constexpr int SF_CAT = 0, SF_MAX = 1, SF_MEAN = 2;

struct SfIn {
    const float *p[SF_MAX_S];
};
struct SfOut {
    float *p[SF_MAX_S];
};

template <int G>
__device__ __forceinline__ float sf_group_sum(float v)
{
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// out (N, S * C) for cat, (N, C) for max / mean; norm (N, S) = ||x_s||_2; xhat (S, N, C) or NULL (max / mean with the scales
// returned); arg (N, C) = the winning scale (max only, ties to the lowest scale)
template <int G>
__global__ __launch_bounds__(SF_BLOCK) void sf_fwd_kernel(SfIn xs, int S, int64_t N, int C, int mode, float eps,
                                                           float *__restrict__ out, float *__restrict__ xhat,
                                                           float *__restrict__ norm, unsigned char *__restrict__ arg)
{
    const int l = threadIdx.x % G;
    const int64_t r = (int64_t)blockIdx.x * (SF_BLOCK / G) + threadIdx.x / G;
    const bool live = r < N;  // (dead rows still take part in the shuffles)
    float den[SF_MAX_S];
#pragma unroll
    for (int s = 0; s < SF_MAX_S; ++s) {
        den[s] = 1.0f;
        if (s < S) {
            float ss = 0.0f;
            if (live)
                for (int c = l; c < C; c += G) {
                    const float v = xs.p[s][r * C + c];
                    ss = __builtin_fmaf(v, v, ss);
                }
            const float n = sqrtf(sf_group_sum<G>(ss));
            den[s] = n + eps;
            if (live && l == 0) norm[r * S + s] = n;
        }
    }
    if (!live) return;
    for (int c = l; c < C; c += G) {
        float best = 0.0f, sum = 0.0f;
        int win = 0;
#pragma unroll
        for (int s = 0; s < SF_MAX_S; ++s) {
            if (s < S) {
                const float h = xs.p[s][r * C + c] / den[s];
                if (mode == SF_CAT) {
                    out[(r * S + s) * C + c] = h;
                } else {
                    if (xhat) xhat[((int64_t)s * N + r) * C + c] = h;
                    if (s == 0 || h > best || (h != h && best == best)) {  // (the first NaN wins and stays, as in torch's max)
                        best = h;
                        win = s;
                    }
                    sum += h;
                }
            }
        }
        if (mode == SF_MAX) {
            out[r * C + c] = best;
            arg[r * C + c] = (unsigned char)win;
        } else if (mode == SF_MEAN) {
            out[r * C + c] = sum / (float)S;
        }
    }
}

// dx_s = g_s / d - x_s <g_s, x_s> / (n d^2), d = n + eps, and g_s / d where n == 0 (the norm's gradient at 0 is 0),
// evaluated as (g_s - h <g_s, h> d / n) / d with h = x_s / d: the two terms cancel at the size of g, not of g / d.
// g_s = the cotangent of xhat_s: the output's columns (cat), gout / S (mean), gout where scale s won (max), plus gxhat_s
template <int G>
__global__ __launch_bounds__(SF_BLOCK) void sf_bwd_kernel(SfIn xs, int S, int64_t N, int C, int mode, float eps,
                                                           const float *__restrict__ gout, const float *__restrict__ gxhat,
                                                           const float *__restrict__ norm, const unsigned char *__restrict__ arg,
                                                           SfOut dxs)
{
    const int l = threadIdx.x % G;
    const int64_t r = (int64_t)blockIdx.x * (SF_BLOCK / G) + threadIdx.x / G;
    const bool live = r < N;
#pragma unroll
    for (int s = 0; s < SF_MAX_S; ++s) {
        if (s < S) {
            float dot = 0.0f;
            const float nl = live ? norm[r * S + s] : 1.0f;
            const float dl = nl + eps;
            if (live)
                for (int c = l; c < C; c += G) {
                    float g = 0.0f;
                    if (gout) {
                        if (mode == SF_CAT) g = gout[(r * S + s) * C + c];
                        else if (mode == SF_MEAN) g = gout[r * C + c] / (float)S;
                        else g = arg[r * C + c] == s ? gout[r * C + c] : 0.0f;
                    }
                    if (gxhat) g += gxhat[((int64_t)s * N + r) * C + c];
                    dot = __builtin_fmaf(g, xs.p[s][r * C + c] / dl, dot);
                }
            dot = sf_group_sum<G>(dot);
            if (live) {
                const float n = nl, d = dl;
                const float q = n > 0.0f ? dot * (d / n) : 0.0f;
                for (int c = l; c < C; c += G) {
                    float g = 0.0f;
                    if (gout) {
                        if (mode == SF_CAT) g = gout[(r * S + s) * C + c];
                        else if (mode == SF_MEAN) g = gout[r * C + c] / (float)S;
                        else g = arg[r * C + c] == s ? gout[r * C + c] : 0.0f;
                    }
                    if (gxhat) g += gxhat[((int64_t)s * N + r) * C + c];
                    const float h = xs.p[s][r * C + c] / d;
                    dxs.p[s][r * C + c] = n > 0.0f ? (g - h * q) / d : g / d;
                }
            }
        }
    }
}

static int sf_group(int C) { return C <= 8 ? 8 : C <= 16 ? 16 : C <= 32 ? 32 : 64; }

static bool sf_args_ok(const void *const *xs, int S, int64_t N, int C, int mode)
{
    if (!xs || S < 1 || S > SF_MAX_S || N < 0 || C < 1 || mode < SF_CAT || mode > SF_MEAN) return false;
    for (int s = 0; s < S; ++s)
        if (N > 0 && !xs[s]) return false;
    return true;
}

}  // namespace tp3d

using namespace tp3d;

#define SF_DISPATCH(kernel, ...)                                                                                            \
    do {                                                                                                                    \
        const int G = sf_group(C);                                                                                          \
        const dim3 grid((unsigned)((N + SF_BLOCK / G - 1) / (SF_BLOCK / G)));                                               \
        if (G == 8) hipLaunchKernelGGL(kernel<8>, grid, dim3(SF_BLOCK), 0, (hipStream_t)stream, __VA_ARGS__);               \
        else if (G == 16) hipLaunchKernelGGL(kernel<16>, grid, dim3(SF_BLOCK), 0, (hipStream_t)stream, __VA_ARGS__);        \
        else if (G == 32) hipLaunchKernelGGL(kernel<32>, grid, dim3(SF_BLOCK), 0, (hipStream_t)stream, __VA_ARGS__);        \
        else hipLaunchKernelGGL(kernel<64>, grid, dim3(SF_BLOCK), 0, (hipStream_t)stream, __VA_ARGS__);                     \
    } while (0)

TP3D_EXPORT int tp3d_scale_fuse_fwd_f32(const float *const *xs, int S, int64_t N, int C, int mode, float eps, float *out,
                                        float *xhat, float *norm, unsigned char *arg, void *stream)
{
    if (!sf_args_ok(reinterpret_cast<const void *const *>(xs), S, N, C, mode)) return TP3D_E_BADARG;
    if (N == 0) return TP3D_OK;
    if (!out || !norm || (mode == SF_MAX && !arg)) return TP3D_E_BADARG;
    if (N >= 0x7fffffff || (int64_t)S * C >= 0x7fffffff) return TP3D_E_TOOBIG;
    SfIn in;
    for (int s = 0; s < SF_MAX_S; ++s) in.p[s] = s < S ? xs[s] : nullptr;
    SF_DISPATCH(sf_fwd_kernel, in, S, N, C, mode, eps, out, xhat, norm, arg);
    return check_launch();
}

TP3D_EXPORT int tp3d_scale_fuse_bwd_f32(const float *const *xs, int S, int64_t N, int C, int mode, float eps, const float *gout,
                                        const float *gxhat, const float *norm, const unsigned char *arg, float *const *dxs,
                                        void *stream)
{
    if (!sf_args_ok(reinterpret_cast<const void *const *>(xs), S, N, C, mode) ||
        !sf_args_ok(reinterpret_cast<const void *const *>(dxs), S, N, C, mode))
        return TP3D_E_BADARG;
    if (N == 0) return TP3D_OK;
    if (!norm || (mode == SF_MAX && gout && !arg)) return TP3D_E_BADARG;
    if (N >= 0x7fffffff || (int64_t)S * C >= 0x7fffffff) return TP3D_E_TOOBIG;
    SfIn in;
    SfOut o;
    for (int s = 0; s < SF_MAX_S; ++s) {
        in.p[s] = s < S ? xs[s] : nullptr;
        o.p[s] = s < S ? dxs[s] : nullptr;
    }
    SF_DISPATCH(sf_bwd_kernel, in, S, N, C, mode, eps, gout, gxhat, norm, arg, o);
    return check_launch();
}
