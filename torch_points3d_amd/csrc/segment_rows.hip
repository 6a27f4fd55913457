// Per-cloud row kernels of PointNet on ragged batches (torch_points3d/core/common_modules/spatial_transform.py:44-49,
// modules/PointNet/modules.py:33-35, :108; torch_geometric's global_mean_pool).  The clouds are the row ranges
// seg[b] .. seg[b + 1) of a sorted batch, seg (B + 1) int64 ascending from 0 to N, empty clouds allowed.
//
//   transform   out[i] = [ x[i, :k] . T[b(i)] (or T[b(i)]^T) | x[i, k:C] | 0 ]     the spatial transformer's bmm over
//                                                                                   trans[batch], and its input gradient
//   wgrad       dT[b]  = sum_{i in cloud b} x[i, :k]^T dy[i, :k]                     its index_add backward
//   bcast_cat   out[i] = [ x[i, :C1] | g[b(i), :C2] | 0 ]                            cat([x, g[batch]], 1)
//   sum         out[b] = scale[b] * sum_{i in cloud b} rows[i, col0 : col0 + C]      dg of bcast_cat, global_mean_pool
//
// Nothing of size N * k * k is written, there are no float atomics, and every sum has one fixed order:
//   * transform: one fp32 fma chain per output, j ascending.  A workgroup owns SEG_TILE_ROWS consecutive rows; their first
//     k columns and the matrix of the current cloud sit in LDS (row stride k | 1: odd, so that the transposing store of
//     T^T and the row-strided reads of x fall on distinct banks; the compute loop reads T with lanes across the output
//     column, consecutive banks).  A tile that crosses a seam reloads the matrix at the seam.  k <= 4: a lane per row, the
//     cloud's matrix in registers.
//   * wgrad and sum: every cloud is cut into chunks of SEG_SUM_CHUNK rows from its first row; a workgroup sums one chunk
//     in ascending row order into its workspace slice, a second kernel adds a cloud's slices in ascending order.  Chunk
//     c of cloud b owns slice seg[b] / SEG_SUM_CHUNK + b + c: computable from seg alone (no scan, no host read), distinct
//     for distinct chunks, below N / SEG_SUM_CHUNK + B.
//   * wgrad is plain fma (4 x 4 outputs per lane, both operand rows read from LDS as float4), not the fp32 matrix
//     instruction: at k = 64 the contraction is 2 k flop per byte of x and dy streamed from HBM, an order of magnitude
//     below what the vector pipe sustains, the fp32 matrix instruction has the vector pipe's peak rate anyway, and the
//     same kernel serves every k from 1 to 64 (padded to a multiple of 4 with zeros in LDS) with the summation order
//     stated above.
// Lanes run across channels in bcast_cat and sum (float4 where widths, strides and addresses are multiples of 16 bytes).
// Every row index is clamped to [0, N) and every cloud index to [0, B): a malformed seg gives wrong numbers, never an
// access outside the buffers.
#include "tp3d_common.h"

namespace tp3d {

constexpr int SEG_BLOCK = 256;
constexpr int SEG_TILE_ROWS = 64;   // rows per workgroup of the transform
constexpr int SEG_SUM_CHUNK = 128;  // rows per chunk of the fixed-order sums
constexpr int SEG_MAX_K = 64;
constexpr int SEG_LDS_LD = SEG_MAX_K + 1;
constexpr int SEG_WG_ROWS = 32;     // rows of x and dy staged per step of the weight gradient
constexpr int SEG_CAT_ROWS = 32;    // rows per workgroup of bcast_cat

// the cloud of `row`: the first b in [0, B) with seg[b + 1] > row, B when there is none
__device__ __forceinline__ int64_t seg_cloud_of(const int64_t *__restrict__ seg, int64_t B, int64_t row)
{
    int64_t lo = 0, hi = B;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (seg[mid + 1] > row) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// first slice of cloud b, b in [0, B]
__device__ __forceinline__ int64_t seg_first_slice(const int64_t *__restrict__ seg, int64_t b)
{
    return seg[b] / SEG_SUM_CHUNK + b;
}

// slice g -> its cloud and rows [r0, r1) (r0 >= r1: the slice belongs to no chunk)
__device__ __forceinline__ void seg_chunk_of(const int64_t *__restrict__ seg, int64_t N, int64_t B, int64_t g, int64_t &r0,
                                             int64_t &r1)
{
    int64_t lo = 0, hi = B;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (seg_first_slice(seg, mid + 1) > g) hi = mid;
        else lo = mid + 1;
    }
    r0 = r1 = 0;
    if (lo >= B) return;
    const int64_t chunk = g - seg_first_slice(seg, lo);
    if (chunk < 0) return;
    r0 = seg[lo] + chunk * SEG_SUM_CHUNK;
    r1 = min(min(r0 + SEG_SUM_CHUNK, seg[lo + 1]), N);
    r0 = max(r0, (int64_t)0);
}

// ------------------------------------------------------------------------------------------------------------ transform
template <int K>
__global__ __launch_bounds__(SEG_BLOCK) void seg_transform_small_kernel(const float *__restrict__ x, const float *__restrict__ T,
                                                                         const int64_t *__restrict__ seg, int64_t N, int64_t B,
                                                                         int C, int ldx, int ldo, int transpose,
                                                                         float *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * SEG_BLOCK + threadIdx.x;
    if (i >= N) return;
    const int64_t b = seg_cloud_of(seg, B, i);
    float t[K * K], xv[K];
#pragma unroll
    for (int e = 0; e < K * K; ++e) t[e] = b < B ? T[b * (K * K) + e] : 0.0f;
    const float *xr = x + i * ldx;
    float *o = out + i * ldo;
#pragma unroll
    for (int j = 0; j < K; ++j) xv[j] = xr[j];
#pragma unroll
    for (int c = 0; c < K; ++c) {
        float acc = 0.0f;
#pragma unroll
        for (int j = 0; j < K; ++j) acc = __builtin_fmaf(xv[j], transpose ? t[c * K + j] : t[j * K + c], acc);
        o[c] = acc;
    }
    for (int c = K; c < C; ++c) o[c] = xr[c];
    for (int c = C; c < ldo; ++c) o[c] = 0.0f;
}

// 5 <= k <= 64; 2^lg >= k lanes per row; vec: k % 4 == 0 and the rows of x are 16-byte aligned
__global__ __launch_bounds__(SEG_BLOCK) void seg_transform_kernel(const float *__restrict__ x, const float *__restrict__ T,
                                                                   const int64_t *__restrict__ seg, int64_t N, int64_t B, int k,
                                                                   int C, int ldx, int ldo, int transpose, int lg, int vec,
                                                                   float *__restrict__ out)
{
    __shared__ float s_T[SEG_MAX_K * SEG_LDS_LD];
    __shared__ float s_x[SEG_TILE_ROWS * SEG_LDS_LD];
    __shared__ int64_t s_b;
    const int tid = threadIdx.x;
    const int ld = k | 1;
    const int64_t tile0 = (int64_t)blockIdx.x * SEG_TILE_ROWS;
    const int64_t tile_end = min(tile0 + SEG_TILE_ROWS, N);
    const int rows = (int)(tile_end - tile0);
    if (vec) {
        const int groups = k >> 2;
        for (int e = tid; e < rows * groups; e += SEG_BLOCK) {
            const int r = e / groups, q = e - r * groups;
            const float4 v = *reinterpret_cast<const float4 *>(x + (tile0 + r) * ldx + 4 * q);
            float *d = s_x + r * ld + 4 * q;
            d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
        }
    } else {
        for (int e = tid; e < rows * k; e += SEG_BLOCK) {
            const int r = e / k, j = e - r * k;
            s_x[r * ld + j] = x[(tile0 + r) * ldx + j];
        }
    }
    if (tid == 0) s_b = seg_cloud_of(seg, B, tile0);
    __syncthreads();
    int64_t b = s_b;
    const int c = tid & ((1 << lg) - 1), rsub = tid >> lg, rg = SEG_BLOCK >> lg;
    int64_t row = tile0;
    while (row < tile_end && b < B) {  // (row and b are the same in every lane)
        const int64_t seg_end = min(seg[b + 1], tile_end);
        if (seg_end <= row) {  // an empty cloud
            ++b;
            continue;
        }
        __syncthreads();  // the previous cloud's rows are done with s_T
        const float *Tb = T + b * (int64_t)(k * k);
        for (int e = tid; e < k * k; e += SEG_BLOCK) {
            const int a = e / k, d = e - a * k;
            s_T[transpose ? d * ld + a : a * ld + d] = Tb[e];
        }
        __syncthreads();
        const int r0 = (int)(row - tile0), r1 = (int)(seg_end - tile0);
        if (c < k) {
            for (int rb = r0 + rsub; rb < r1; rb += 4 * rg) {
                int rr[4];
                float acc[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    rr[u] = min(rb + u * rg, SEG_TILE_ROWS - 1) * ld;
                    acc[u] = 0.0f;
                }
                for (int j = 0; j < k; ++j) {
                    const float t = s_T[j * ld + c];
#pragma unroll
                    for (int u = 0; u < 4; ++u) acc[u] = __builtin_fmaf(s_x[rr[u] + j], t, acc[u]);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (rb + u * rg < r1) out[(tile0 + rb + u * rg) * ldo + c] = acc[u];
            }
        }
        row = seg_end;
        ++b;
    }
    // pass-through columns k .. C and the zero padding C .. ldo
    const int extra = ldo - k;
    for (int e = tid; e < rows * extra; e += SEG_BLOCK) {
        const int r = e / extra, cc = k + (e - r * extra);
        out[(tile0 + r) * ldo + cc] = cc < C ? x[(tile0 + r) * ldx + cc] : 0.0f;
    }
}

// ------------------------------------------------------------------------------------------------------ weight gradient
// one workgroup per slice; lane (tj, tc) of the first (kp4 / 4)^2 owns dT[4 tj .. 4 tj + 3][4 tc .. 4 tc + 3]
__global__ __launch_bounds__(SEG_BLOCK) void seg_wgrad_chunk_kernel(const float *__restrict__ x, const float *__restrict__ dy,
                                                                     const int64_t *__restrict__ seg, int64_t N, int64_t B, int k,
                                                                     int ldx, int lddy, int vec, float *__restrict__ ws)
{
    __shared__ __attribute__((aligned(16))) float s_x[SEG_WG_ROWS * SEG_MAX_K];
    __shared__ __attribute__((aligned(16))) float s_d[SEG_WG_ROWS * SEG_MAX_K];
    const int tid = threadIdx.x;
    int64_t r0, r1;
    seg_chunk_of(seg, N, B, blockIdx.x, r0, r1);
    if (r0 >= r1) return;  // (the whole workgroup)
    const int kp4 = (k + 3) & ~3, nt = kp4 >> 2;
    const bool active = tid < nt * nt;
    const int tj = active ? tid / nt : 0, tc = active ? tid - tj * nt : 0;
    float acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int d = 0; d < 4; ++d) acc[a][d] = 0.0f;
    for (int64_t base = r0; base < r1; base += SEG_WG_ROWS) {
        const int nr = (int)min((int64_t)SEG_WG_ROWS, r1 - base);
        __syncthreads();
        if (vec) {
            for (int e = tid; e < nr * nt; e += SEG_BLOCK) {
                const int r = e / nt, q = e - r * nt;
                *reinterpret_cast<float4 *>(s_x + r * SEG_MAX_K + 4 * q) =
                    *reinterpret_cast<const float4 *>(x + (base + r) * ldx + 4 * q);
                *reinterpret_cast<float4 *>(s_d + r * SEG_MAX_K + 4 * q) =
                    *reinterpret_cast<const float4 *>(dy + (base + r) * lddy + 4 * q);
            }
        } else {
            for (int e = tid; e < nr * kp4; e += SEG_BLOCK) {
                const int r = e / kp4, j = e - r * kp4;
                s_x[r * SEG_MAX_K + j] = j < k ? x[(base + r) * ldx + j] : 0.0f;
                s_d[r * SEG_MAX_K + j] = j < k ? dy[(base + r) * lddy + j] : 0.0f;
            }
        }
        __syncthreads();
        if (active) {
            for (int r = 0; r < nr; ++r) {
                const float4 xa = *reinterpret_cast<const float4 *>(s_x + r * SEG_MAX_K + 4 * tj);
                const float4 da = *reinterpret_cast<const float4 *>(s_d + r * SEG_MAX_K + 4 * tc);
                const float xs[4] = {xa.x, xa.y, xa.z, xa.w}, ds[4] = {da.x, da.y, da.z, da.w};
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int d = 0; d < 4; ++d) acc[a][d] = __builtin_fmaf(xs[a], ds[d], acc[a][d]);
            }
        }
    }
    if (!active) return;
    float *slice = ws + (int64_t)blockIdx.x * (k * k);
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const int j = 4 * tj + a, cc = 4 * tc + d;
            if (j < k && cc < k) slice[j * k + cc] = acc[a][d];
        }
}

// out[b, e] = scale[b] * (slices of cloud b added in ascending order), e < width; `slices` of them exist
__global__ __launch_bounds__(SEG_BLOCK) void seg_add_slices_kernel(const float *__restrict__ ws, const int64_t *__restrict__ seg,
                                                                    const float *__restrict__ scale, int64_t B, int width,
                                                                    int64_t slices, float *__restrict__ out)
{
    const int64_t idx = (int64_t)blockIdx.x * SEG_BLOCK + threadIdx.x;
    if (idx >= B * width) return;
    const int64_t b = idx / width;
    const int e = (int)(idx - b * width);
    const int64_t n = max(seg[b + 1] - seg[b], (int64_t)0);
    const int64_t first = min(max(seg_first_slice(seg, b), (int64_t)0), slices);
    const int64_t count = min((n + SEG_SUM_CHUNK - 1) / SEG_SUM_CHUNK, slices - first);
    float acc = 0.0f;
    for (int64_t s = 0; s < count; ++s) acc = acc + ws[(first + s) * width + e];
    out[idx] = scale ? scale[b] * acc : acc;
}

// ------------------------------------------------------------------------------------------------------------------ sum
template <bool VEC>
struct SegRow;
template <>
struct SegRow<true> {
    typedef float4 T;
    static constexpr int W = 4;
    static __device__ __forceinline__ T zero() { return make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
    static __device__ __forceinline__ T load(const float *p) { return *reinterpret_cast<const float4 *>(p); }
    static __device__ __forceinline__ void store(float *p, T v) { *reinterpret_cast<float4 *>(p) = v; }
    static __device__ __forceinline__ T add(T a, T b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
};
template <>
struct SegRow<false> {
    typedef float T;
    static constexpr int W = 1;
    static __device__ __forceinline__ T zero() { return 0.0f; }
    static __device__ __forceinline__ T load(const float *p) { return *p; }
    static __device__ __forceinline__ void store(float *p, T v) { *p = v; }
    static __device__ __forceinline__ T add(T a, T b) { return a + b; }
};

// grid (slices, column passes); a lane per group of W columns sums the chunk's rows in ascending order
template <bool VEC>
__global__ __launch_bounds__(SEG_BLOCK) void seg_sum_chunk_kernel(const float *__restrict__ rows, const int64_t *__restrict__ seg,
                                                                   int64_t N, int64_t B, int col0, int C, int ld,
                                                                   float *__restrict__ ws)
{
    typedef SegRow<VEC> R;
    const int q = blockIdx.y * blockDim.x + threadIdx.x;
    if (q >= C / R::W) return;
    int64_t r0, r1;
    seg_chunk_of(seg, N, B, blockIdx.x, r0, r1);
    if (r0 >= r1) return;
    const float *src = rows + col0 + q * R::W;
    typename R::T acc = R::zero();
    for (int64_t r = r0; r < r1; r += 4) {  // four row loads in flight, added in row order
        typename R::T v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = r + u < r1 ? R::load(src + (r + u) * ld) : R::zero();
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (r + u < r1) acc = R::add(acc, v[u]);
    }
    R::store(ws + (int64_t)blockIdx.x * C + q * R::W, acc);
}

// ------------------------------------------------------------------------------------------------------------ bcast_cat
template <bool VEC>
__global__ __launch_bounds__(SEG_BLOCK) void seg_bcast_cat_kernel(const float *__restrict__ x, const float *__restrict__ g,
                                                                   const int64_t *__restrict__ seg, int64_t N, int64_t B, int C1,
                                                                   int C2, int ldx, int ldg, int ldo, float *__restrict__ out)
{
    typedef SegRow<VEC> R;
    __shared__ int64_t s_b[SEG_CAT_ROWS];
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * SEG_CAT_ROWS;
    const int nr = (int)min((int64_t)SEG_CAT_ROWS, N - row0);
    if (tid < nr) s_b[tid] = seg_cloud_of(seg, B, row0 + tid);
    __syncthreads();
    const int groups = ldo / R::W, g1 = C1 / R::W, g2 = (C1 + C2) / R::W;
    for (int e = tid; e < nr * groups; e += SEG_BLOCK) {
        const int r = e / groups, q = e - r * groups;
        const int64_t b = s_b[r];
        typename R::T v = R::zero();
        if (q < g1) v = R::load(x + (row0 + r) * ldx + q * R::W);
        else if (q < g2 && b < B) v = R::load(g + b * ldg + (q - g1) * R::W);
        R::store(out + (row0 + r) * ldo + q * R::W, v);
    }
}

static bool seg_aligned16(const void *a, const void *b, const void *c)
{
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15) == 0;
}

static int64_t seg_slices(int64_t N, int64_t B) { return N / SEG_SUM_CHUNK + B; }

static int seg_add_slices(const float *ws, const int64_t *seg, const float *scale, int64_t B, int width, int64_t slices,
                          float *out, hipStream_t s)
{
    const int64_t total = B * width;
    hipLaunchKernelGGL(seg_add_slices_kernel, dim3((unsigned)((total + SEG_BLOCK - 1) / SEG_BLOCK)), dim3(SEG_BLOCK), 0, s, ws, seg,
                       scale, B, width, slices, out);
    return check_launch();
}

}  // namespace tp3d

using namespace tp3d;

TP3D_EXPORT int tp3d_segment_tile_rows(void) { return SEG_TILE_ROWS; }
TP3D_EXPORT int tp3d_segment_sum_chunk(void) { return SEG_SUM_CHUNK; }

TP3D_EXPORT int tp3d_segment_transform_f32(const float *x, const float *T, const int64_t *seg, int64_t N, int64_t B, int k, int C,
                                           int ldx, int ldo, int transpose, float *out, void *stream)
{
    if (N < 0 || B < 0 || k < 1 || k > SEG_MAX_K || C < k || ldx < C || ldo < C) return TP3D_E_BADARG;
    if (N == 0) return TP3D_OK;
    if (!x || !T || !seg || !out || B == 0) return TP3D_E_BADARG;
    if (N >= 0x7fffffff || B >= 0x7fffffff) return TP3D_E_TOOBIG;
    hipStream_t s = (hipStream_t)stream;
    if (k <= 4) {
        const dim3 grid((unsigned)((N + SEG_BLOCK - 1) / SEG_BLOCK));
#define SEG_SMALL(KK)                                                                                                          \
    hipLaunchKernelGGL(seg_transform_small_kernel<KK>, grid, dim3(SEG_BLOCK), 0, s, x, T, seg, N, B, C, ldx, ldo, transpose, out)
        if (k == 1) SEG_SMALL(1);
        else if (k == 2) SEG_SMALL(2);
        else if (k == 3) SEG_SMALL(3);
        else SEG_SMALL(4);
#undef SEG_SMALL
        return check_launch();
    }
    int lg = 3;
    while ((1 << lg) < k) ++lg;
    const int vec = (k & 3) == 0 && (ldx & 3) == 0 && seg_aligned16(x, nullptr, nullptr);
    hipLaunchKernelGGL(seg_transform_kernel, dim3((unsigned)((N + SEG_TILE_ROWS - 1) / SEG_TILE_ROWS)), dim3(SEG_BLOCK), 0, s, x, T,
                       seg, N, B, k, C, ldx, ldo, transpose, lg, vec, out);
    return check_launch();
}

TP3D_EXPORT size_t tp3d_segment_transform_wgrad_workspace_bytes(int64_t N, int64_t B, int k)
{
    if (N < 0 || B <= 0 || k < 1 || k > SEG_MAX_K) return 0;
    return (size_t)seg_slices(N, B) * k * k * sizeof(float);
}

TP3D_EXPORT int tp3d_segment_transform_wgrad_f32(const float *x, const float *dy, const int64_t *seg, int64_t N, int64_t B, int k,
                                                 int ldx, int lddy, float *dT, void *workspace, size_t workspace_bytes,
                                                 void *stream)
{
    if (N < 0 || B < 0 || k < 1 || k > SEG_MAX_K || ldx < k || lddy < k) return TP3D_E_BADARG;
    if (B == 0) return N == 0 ? TP3D_OK : TP3D_E_BADARG;
    if (!seg || !dT) return TP3D_E_BADARG;
    if (N >= 0x7fffffff || B >= 0x7fffffff / (k * k)) return TP3D_E_TOOBIG;
    hipStream_t s = (hipStream_t)stream;
    if (N == 0) return zero_async(dT, (size_t)B * k * k * sizeof(float), s);
    if (!x || !dy || !workspace || workspace_bytes < tp3d_segment_transform_wgrad_workspace_bytes(N, B, k)) return TP3D_E_BADARG;
    const int64_t slices = seg_slices(N, B);
    const int vec = (k & 3) == 0 && ((ldx | lddy) & 3) == 0 && seg_aligned16(x, dy, nullptr);
    float *ws = static_cast<float *>(workspace);
    hipLaunchKernelGGL(seg_wgrad_chunk_kernel, dim3((unsigned)slices), dim3(SEG_BLOCK), 0, s, x, dy, seg, N, B, k, ldx, lddy, vec, ws);
    if (int rc = check_launch()) return rc;
    return seg_add_slices(ws, seg, nullptr, B, k * k, slices, dT, s);
}

TP3D_EXPORT int tp3d_segment_bcast_cat_f32(const float *x, const float *g, const int64_t *seg, int64_t N, int64_t B, int C1, int C2,
                                           int ldx, int ldg, int ldo, float *out, void *stream)
{
    if (N < 0 || B < 0 || C1 < 0 || C2 < 0 || ldo < C1 + C2 || ldo < 1 || ldx < C1 || ldg < C2) return TP3D_E_BADARG;
    if (N == 0) return TP3D_OK;
    if (!seg || !out || B == 0 || (C1 > 0 && !x) || (C2 > 0 && !g)) return TP3D_E_BADARG;
    if (N >= 0x7fffffff || B >= 0x7fffffff) return TP3D_E_TOOBIG;
    hipStream_t s = (hipStream_t)stream;
    const bool vec = ((C1 | C2 | ldx | ldg | ldo) & 3) == 0 && seg_aligned16(x, g, out);
    const dim3 grid((unsigned)((N + SEG_CAT_ROWS - 1) / SEG_CAT_ROWS));
    if (vec)
        hipLaunchKernelGGL(seg_bcast_cat_kernel<true>, grid, dim3(SEG_BLOCK), 0, s, x, g, seg, N, B, C1, C2, ldx, ldg, ldo, out);
    else
        hipLaunchKernelGGL(seg_bcast_cat_kernel<false>, grid, dim3(SEG_BLOCK), 0, s, x, g, seg, N, B, C1, C2, ldx, ldg, ldo, out);
    return check_launch();
}

TP3D_EXPORT size_t tp3d_segment_sum_workspace_bytes(int64_t N, int64_t B, int C)
{
    if (N < 0 || B <= 0 || C < 1) return 0;
    return (size_t)seg_slices(N, B) * C * sizeof(float);
}

TP3D_EXPORT int tp3d_segment_sum_f32(const float *rows, const int64_t *seg, const float *scale, int64_t N, int64_t B, int col0,
                                     int C, int ld, float *out, void *workspace, size_t workspace_bytes, void *stream)
{
    if (N < 0 || B < 0 || col0 < 0 || C < 1 || ld < col0 + C) return TP3D_E_BADARG;
    if (B == 0) return N == 0 ? TP3D_OK : TP3D_E_BADARG;
    if (!seg || !out) return TP3D_E_BADARG;
    if (N >= 0x7fffffff || B >= 0x7fffffff / C) return TP3D_E_TOOBIG;
    hipStream_t s = (hipStream_t)stream;
    if (N == 0) return zero_async(out, (size_t)B * C * sizeof(float), s);
    if (!rows || !workspace || workspace_bytes < tp3d_segment_sum_workspace_bytes(N, B, C)) return TP3D_E_BADARG;
    const int64_t slices = seg_slices(N, B);
    float *ws = static_cast<float *>(workspace);
    const bool vec = ((C | col0 | ld) & 3) == 0 && seg_aligned16(rows, ws, nullptr);
    const int groups = vec ? C / 4 : C;
    const int waves = (groups + kWave - 1) / kWave;
    const int threads = waves * kWave < SEG_BLOCK ? waves * kWave : SEG_BLOCK;
    const dim3 grid((unsigned)slices, (unsigned)((groups + threads - 1) / threads));
    if (vec)
        hipLaunchKernelGGL(seg_sum_chunk_kernel<true>, grid, dim3(threads), 0, s, rows, seg, N, B, col0, C, ld, ws);
    else
        hipLaunchKernelGGL(seg_sum_chunk_kernel<false>, grid, dim3(threads), 0, s, rows, seg, N, B, col0, C, ld, ws);
    if (int rc = check_launch()) return rc;
    return seg_add_slices(ws, seg, scale, B, C, slices, out, s);
}
