// Cluster voxel mean of PointGroup's sparse scorers (reference models/panoptic/pointgroup.py:123-141: backbone_features[cluster]
// of every cluster concatenated, then GridSampling3D(mode="mean") with batch = cluster index).
//
// The clusters are a CSR over member slots (slot e holds point members[e]); the voxels of the slots come from the voxel
// clustering of voxel.hip run over the slots (batch = the slot's cluster), so voxel v owns order[vstart[v] .. vstart[v + 1])
// in ascending slot order.  Both kernels are streaming run sums through two indirections and never hold the gathered
// (slots, C) rows:
//   forward   out[v] = (sum over the voxel's slots e, ascending, of x[members[e]]) / n_v         voxel -> slot -> point
//   backward  dx[p]  = sum over the slots e of point p, ascending, of dout[voxel(e)] / n_voxel(e)   point -> slot -> voxel
// with the point -> slots index (pstart, porder) handed in by the caller: tp3d_pv_invert_i32 over `members`, a stable radix
// sort on the sorted-key core (0.12 ms for 243 548 slots over 345 948 points, where invert_table's one-workgroup scan over
// the points took the backward to 1.04 ms).  A point of two clusters has two slots; a point of none gets an empty run and
// exact zeros.  Lanes run across channels (float4 where C % 4 == 0 and the rows are 16-byte aligned), 256 / lanes-per-row
// rows per workgroup, four row loads in flight per lane.  A run of more
// than CV_LONG_RUN = 64 slots is summed by one workgroup in CV_PIECES = 16 contiguous pieces added in piece order, the
// association of tp3d_pv_runsum_f32 (pointvoxel.hip).  No float atomics: every sum has a fixed order, repeats are bit-equal.
#include "tp3d_common.h"

namespace tp3d {

constexpr int CV_BLOCK = 256;
constexpr int CV_LONG_RUN = 64;
constexpr int CV_PIECES = 16;
constexpr int CV_LONG_LANES = CV_BLOCK / CV_PIECES;

template <bool VEC>
struct CvRow;
template <>
struct CvRow<true> {
    typedef float4 T;
    static constexpr int W = 4;
    static __device__ __forceinline__ T zero() { return make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
    static __device__ __forceinline__ T load(const float *p) { return *reinterpret_cast<const float4 *>(p); }
    static __device__ __forceinline__ void store(float *p, T v) { *reinterpret_cast<float4 *>(p) = v; }
    static __device__ __forceinline__ T div(T v, float d) { return make_float4(v.x / d, v.y / d, v.z / d, v.w / d); }
    static __device__ __forceinline__ T add(T a, T b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
};
template <>
struct CvRow<false> {
    typedef float T;
    static constexpr int W = 1;
    static __device__ __forceinline__ T zero() { return 0.0f; }
    static __device__ __forceinline__ T load(const float *p) { return *p; }
    static __device__ __forceinline__ void store(float *p, T v) { *p = v; }
    static __device__ __forceinline__ T div(T v, float d) { return v / d; }
    static __device__ __forceinline__ T add(T a, T b) { return a + b; }
};

// forward piece: sum of x[members[order[j]]] over j in [b, e), ascending, for this lane's channel group at column `col`
template <bool VEC>
__device__ __forceinline__ typename CvRow<VEC>::T cv_sum_points(const float *__restrict__ x, int ldx,
                                                                const int64_t *__restrict__ members,
                                                                const int64_t *__restrict__ order, int64_t b, int64_t e,
                                                                int64_t N, int64_t E, int col)
{
    typedef CvRow<VEC> R;
    typename R::T acc = R::zero();
    for (int64_t j = b; j < e; j += 4) {  // four independent slot -> point -> row loads in flight, added in slot order
        int64_t r[4];
        bool has[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t slot = j + u < e ? order[j + u] : -1;
            const bool in = slot >= 0 && slot < E;
            const int64_t p = in ? members[slot] : -1;
            has[u] = p >= 0 && p < N;
            r[u] = has[u] ? p : 0;  // (row 0 exists: the entry point returns for N == 0)
        }
        typename R::T v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = R::load(x + r[u] * ldx + col);
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = R::add(acc, has[u] ? v[u] : R::zero());
    }
    return acc;
}

// backward piece: sum of dout[voxel(slot)] / n_voxel over the slots order[j], j in [b, e), ascending
template <bool VEC>
__device__ __forceinline__ typename CvRow<VEC>::T cv_sum_voxels(const float *__restrict__ dout,
                                                                const int64_t *__restrict__ slot_voxel,
                                                                const int64_t *__restrict__ vstart,
                                                                const int *__restrict__ order, int b, int e, int64_t E,
                                                                int64_t V, int C, int col)
{
    typedef CvRow<VEC> R;
    typename R::T acc = R::zero();
    for (int j = b; j < e; j += 4) {
        int64_t r[4];
        float n[4];
        bool has[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t slot = j + u < e ? order[j + u] : -1;
            const bool in = slot >= 0 && slot < E;
            const int64_t v = in ? slot_voxel[slot] : -1;
            has[u] = v >= 0 && v < V;
            r[u] = has[u] ? v : 0;  // (row 0 exists: V > 0 here)
            n[u] = (float)max(vstart[r[u] + 1] - vstart[r[u]], (int64_t)1);
        }
        typename R::T g[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) g[u] = R::load(dout + r[u] * C + col);
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = R::add(acc, has[u] ? R::div(g[u], n[u]) : R::zero());
    }
    return acc;
}

// voxels of at most CV_LONG_RUN slots: one team of 2^tl lanes per voxel
template <bool VEC>
__global__ __launch_bounds__(CV_BLOCK) void cv_mean_fwd_kernel(const float *__restrict__ x, int ldx,
                                                                const int64_t *__restrict__ members,
                                                                const int64_t *__restrict__ order,
                                                                const int64_t *__restrict__ vstart, int64_t N, int64_t E,
                                                                int64_t V, int C, int tl, float *__restrict__ out)
{
    typedef CvRow<VEC> R;
    const int sub = threadIdx.x & ((1 << tl) - 1);
    const int64_t v = (int64_t)blockIdx.x * (CV_BLOCK >> tl) + (threadIdx.x >> tl);
    if (v >= V) return;
    const int64_t b = max(vstart[v], (int64_t)0), e = min(vstart[v + 1], E);
    if (e - b > CV_LONG_RUN) return;  // cv_mean_fwd_long_kernel writes this row
    const float n = (float)max(e - b, (int64_t)1);
    const int groups = C / R::W;
    for (int c = sub; c < groups; c += 1 << tl)
        R::store(out + v * C + c * R::W, R::div(cv_sum_points<VEC>(x, ldx, members, order, b, e, N, E, c * R::W), n));
}

// longer voxels: workgroups stride over the voxels, CV_PIECES teams take one contiguous piece each, pieces added in order
template <bool VEC>
__global__ __launch_bounds__(CV_BLOCK) void cv_mean_fwd_long_kernel(const float *__restrict__ x, int ldx,
                                                                     const int64_t *__restrict__ members,
                                                                     const int64_t *__restrict__ order,
                                                                     const int64_t *__restrict__ vstart, int64_t N,
                                                                     int64_t E, int64_t V, int C, float *__restrict__ out)
{
    typedef CvRow<VEC> R;
    __shared__ typename R::T s_part[CV_PIECES][CV_LONG_LANES];
    const int lane = threadIdx.x & (CV_LONG_LANES - 1), team = threadIdx.x / CV_LONG_LANES;
    const int groups = C / R::W;
    for (int64_t v = blockIdx.x; v < V; v += gridDim.x) {
        const int64_t b = max(vstart[v], (int64_t)0), e = min(vstart[v + 1], E);
        const int64_t n = e - b;
        if (n <= CV_LONG_RUN) continue;  // (workgroup-uniform)
        const int64_t piece = (n + CV_PIECES - 1) / CV_PIECES;
        const int64_t pb = min(e, b + team * piece), pe = min(e, pb + piece);
        for (int c0 = 0; c0 < groups; c0 += CV_LONG_LANES) {
            const int c = c0 + lane;
            s_part[team][lane] = c < groups ? cv_sum_points<VEC>(x, ldx, members, order, pb, pe, N, E, c * R::W) : R::zero();
            __syncthreads();
            if (team == 0 && c < groups) {
                typename R::T acc = s_part[0][lane];
#pragma unroll
                for (int t = 1; t < CV_PIECES; ++t) acc = R::add(acc, s_part[t][lane]);
                R::store(out + v * C + c * R::W, R::div(acc, (float)n));
            }
            __syncthreads();
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(CV_BLOCK) void cv_mean_bwd_kernel(const float *__restrict__ dout,
                                                                const int64_t *__restrict__ slot_voxel,
                                                                const int64_t *__restrict__ vstart,
                                                                const int *__restrict__ pstart, const int *__restrict__ porder,
                                                                int64_t N, int64_t E, int64_t V, int C, int tl,
                                                                float *__restrict__ dx)
{
    typedef CvRow<VEC> R;
    const int sub = threadIdx.x & ((1 << tl) - 1);
    const int64_t p = (int64_t)blockIdx.x * (CV_BLOCK >> tl) + (threadIdx.x >> tl);
    if (p >= N) return;
    const int b = max(pstart[p], 0), e = (int)min((int64_t)pstart[p + 1], E);
    if (e - b > CV_LONG_RUN) return;  // cv_mean_bwd_long_kernel writes this row
    const int groups = C / R::W;
    for (int c = sub; c < groups; c += 1 << tl)
        R::store(dx + p * C + c * R::W, cv_sum_voxels<VEC>(dout, slot_voxel, vstart, porder, b, e, E, V, C, c * R::W));
}

template <bool VEC>
__global__ __launch_bounds__(CV_BLOCK) void cv_mean_bwd_long_kernel(const float *__restrict__ dout,
                                                                     const int64_t *__restrict__ slot_voxel,
                                                                     const int64_t *__restrict__ vstart,
                                                                     const int *__restrict__ pstart,
                                                                     const int *__restrict__ porder, int64_t N, int64_t E,
                                                                     int64_t V, int C, float *__restrict__ dx)
{
    typedef CvRow<VEC> R;
    __shared__ typename R::T s_part[CV_PIECES][CV_LONG_LANES];
    const int lane = threadIdx.x & (CV_LONG_LANES - 1), team = threadIdx.x / CV_LONG_LANES;
    const int groups = C / R::W;
    for (int64_t p = blockIdx.x; p < N; p += gridDim.x) {
        const int b = max(pstart[p], 0), e = (int)min((int64_t)pstart[p + 1], E);
        const int n = e - b;
        if (n <= CV_LONG_RUN) continue;  // (workgroup-uniform)
        const int piece = (n + CV_PIECES - 1) / CV_PIECES;
        const int pb = min(e, b + team * piece), pe = min(e, pb + piece);
        for (int c0 = 0; c0 < groups; c0 += CV_LONG_LANES) {
            const int c = c0 + lane;
            s_part[team][lane] = c < groups ? cv_sum_voxels<VEC>(dout, slot_voxel, vstart, porder, pb, pe, E, V, C, c * R::W)
                                            : R::zero();
            __syncthreads();
            if (team == 0 && c < groups) {
                typename R::T acc = s_part[0][lane];
#pragma unroll
                for (int t = 1; t < CV_PIECES; ++t) acc = R::add(acc, s_part[t][lane]);
                R::store(dx + p * C + c * R::W, acc);
            }
            __syncthreads();
        }
    }
}

// lanes per row: the least power of two covering the row's channel groups, 64 at the most
static int cv_team_log2(int groups)
{
    int tl = 0;
    while ((1 << tl) < groups && tl < 6) ++tl;
    return tl;
}

static bool cv_aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// workgroups of a long-run kernel: at most E / (CV_LONG_RUN + 1) rows have a long run; they stride over the rows
static unsigned cv_long_blocks(int64_t E, int64_t rows)
{
    int64_t n = E / (CV_LONG_RUN + 1);
    if (n > rows) n = rows;
    if (n > 1024) n = 1024;
    return (unsigned)n;
}

}  // namespace tp3d

using namespace tp3d;

TP3D_EXPORT int tp3d_cluster_voxel_mean_fwd_f32(const float *x, int ldx, const int64_t *members, const int64_t *order,
                                                const int64_t *vstart, int64_t N, int64_t E, int64_t V, int C, float *out,
                                                void *stream)
{
    if (N < 0 || E < 0 || V < 0 || C <= 0 || ldx < C) return TP3D_E_BADARG;
    if (V == 0) return TP3D_OK;
    if (!out) return TP3D_E_BADARG;
    if (N >= 0x7fffffff || E >= 0x7fffffff || V >= 0x7fffffff) return TP3D_E_TOOBIG;
    hipStream_t s = (hipStream_t)stream;
    if (N == 0 || E == 0) return zero_async(out, (size_t)V * C * sizeof(float), s);
    if (!x || !members || !order || !vstart) return TP3D_E_BADARG;
    const bool vec = (C & 3) == 0 && (ldx & 3) == 0 && cv_aligned16(x) && cv_aligned16(out);
    const int tl = cv_team_log2(vec ? C / 4 : C);
    const unsigned blocks = (unsigned)((V + (CV_BLOCK >> tl) - 1) / (CV_BLOCK >> tl));
    const unsigned lb = cv_long_blocks(E, V);
    if (vec) {
        hipLaunchKernelGGL(cv_mean_fwd_kernel<true>, dim3(blocks), dim3(CV_BLOCK), 0, s, x, ldx, members, order, vstart, N, E, V,
                           C, tl, out);
        if (lb)
            hipLaunchKernelGGL(cv_mean_fwd_long_kernel<true>, dim3(lb), dim3(CV_BLOCK), 0, s, x, ldx, members, order, vstart, N,
                               E, V, C, out);
    } else {
        hipLaunchKernelGGL(cv_mean_fwd_kernel<false>, dim3(blocks), dim3(CV_BLOCK), 0, s, x, ldx, members, order, vstart, N, E, V,
                           C, tl, out);
        if (lb)
            hipLaunchKernelGGL(cv_mean_fwd_long_kernel<false>, dim3(lb), dim3(CV_BLOCK), 0, s, x, ldx, members, order, vstart, N,
                               E, V, C, out);
    }
    return check_launch();
}

TP3D_EXPORT int tp3d_cluster_voxel_mean_bwd_f32(const float *dout, const int64_t *slot_voxel, const int64_t *vstart,
                                                const int32_t *pstart, const int32_t *porder, int64_t N, int64_t E, int64_t V,
                                                int C, float *dx, void *stream)
{
    if (N < 0 || E < 0 || V < 0 || C <= 0) return TP3D_E_BADARG;
    if (N == 0) return TP3D_OK;
    if (!dx) return TP3D_E_BADARG;
    if (N >= 0x7fffffff || E >= 0x7fffffff || V >= 0x7fffffff) return TP3D_E_TOOBIG;
    hipStream_t s = (hipStream_t)stream;
    if (E == 0 || V == 0) return zero_async(dx, (size_t)N * C * sizeof(float), s);
    if (!dout || !slot_voxel || !vstart || !pstart || !porder) return TP3D_E_BADARG;
    const bool vec = (C & 3) == 0 && cv_aligned16(dout) && cv_aligned16(dx);
    const int tl = cv_team_log2(vec ? C / 4 : C);
    const unsigned blocks = (unsigned)((N + (CV_BLOCK >> tl) - 1) / (CV_BLOCK >> tl));
    const unsigned lb = cv_long_blocks(E, N);
    if (vec) {
        hipLaunchKernelGGL(cv_mean_bwd_kernel<true>, dim3(blocks), dim3(CV_BLOCK), 0, s, dout, slot_voxel, vstart, pstart, porder,
                           N, E, V, C, tl, dx);
        if (lb)
            hipLaunchKernelGGL(cv_mean_bwd_long_kernel<true>, dim3(lb), dim3(CV_BLOCK), 0, s, dout, slot_voxel, vstart, pstart,
                               porder, N, E, V, C, dx);
    } else {
        hipLaunchKernelGGL(cv_mean_bwd_kernel<false>, dim3(blocks), dim3(CV_BLOCK), 0, s, dout, slot_voxel, vstart, pstart,
                           porder, N, E, V, C, tl, dx);
        if (lb)
            hipLaunchKernelGGL(cv_mean_bwd_long_kernel<false>, dim3(lb), dim3(CV_BLOCK), 0, s, dout, slot_voxel, vstart, pstart,
                               porder, N, E, V, C, dx);
    }
    return check_launch();
}
