// Point-voxel operations of PVCNN / SPVCNN (torch_points3d/modules/PVCNN/utils.py over torchsparse 1.x): point -> voxel
// coordinates, trilinear weights, table inversion and the two feature kernels every crossing of the point / voxel boundary
// is made of.  The lookups themselves are tp3d_sparse_kmap_i32 (sparseconv.hip) over the coordinates written here.
//
//   gather-sum (point side)  out[p] = sum_k w[p][k] * src[table[p][k]]            devoxelise forward (K = 8),
//                                                                                voxelise backward (K = 1, scale = 1 / count)
//   run-sum    (voxel side)  out[v] = scale[v] * sum_{l in run(v)} w[l] * src[l / K]   voxelise forward (K = 1),
//                                                                                devoxelise backward (K = 8, w = weights)
//
// run(v) = order[start[v] .. start[v + 1]) lists the slots l = p * K + k that point at row v in ascending l (a stable radix
// sort of the slots by destination; absent slots sort behind row Nv - 1 and belong to no run).  Lanes run across channels
// (float4 where C % 4 == 0 and the rows are 16-byte aligned, one float otherwise), 256 / lanes-per-row rows per workgroup;
// nothing of size N * 8 * C is written and there are no float atomics: every sum has a fixed order and is bit-reproducible.
// A run of more than PV_LONG_RUN = 64 slots (a stride-16 voxel holds hundreds of points) is summed by one workgroup in
// PV_PIECES = 16 contiguous pieces of ceil(n / 16) slots, added in piece order: the association depends on the run length
// only -- reproducible, not the sequential sum bit for bit.  An index outside its row range counts as absent everywhere.
#include "sorted_keys.h"

namespace tp3d {

constexpr int PV_BLOCK = 256;
constexpr int PV_LONG_RUN = 64;  // runs up to this many slots are summed sequentially by one team of lanes
constexpr int PV_PIECES = 16;    // pieces of a longer run (= teams of the long-run workgroup)
constexpr int PV_LONG_LANES = PV_BLOCK / PV_PIECES;

// q = [floor(x / s) * s, floor(y / s) * s, floor(z / s) * s, (int)batch]; division and floor in fp32, as
// torch.floor(C[:, :3] / s).int() * s
__global__ __launch_bounds__(PV_BLOCK) void pv_quantize_kernel(const float *__restrict__ pc, int64_t N, int s,
                                                                int *__restrict__ q)
{
    const int64_t i = (int64_t)blockIdx.x * PV_BLOCK + threadIdx.x;
    if (i >= N) return;
    const float fs = (float)s;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int f = (int)floorf(pc[i * 4 + a] / fs);
        q[i * 4 + a] = (int)((unsigned)f * (unsigned)s);
    }
    q[i * 4 + 3] = (int)pc[i * 4 + 3];
}

// torchsparse 1.x calc_ti_weights (recalled): corner k = 4 dx + 2 dy + dz, w = a_x a_y a_z with a = pc - p (d = 0) or
// p - pf (d = 1), pf = floor(p / s) * s, pc = pf + s; / s^3; 0 where the corner is absent; / (sum + 1e-8)
__global__ __launch_bounds__(PV_BLOCK) void pv_trilinear_kernel(const float *__restrict__ pc, int *__restrict__ idx8, int64_t N,
                                                                 int64_t Nv, int s, int nearest, float *__restrict__ w)
{
    const int64_t i = (int64_t)blockIdx.x * PV_BLOCK + threadIdx.x;
    if (i >= N) return;
    const float fs = (float)s;
    float a[3][2];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const float p = pc[i * 4 + d];
        const float pf = floorf(p / fs) * fs;
        const float pn = pf + fs;
        a[d][0] = pn - p;
        a[d][1] = p - pf;
    }
    const float cube = (fs * fs) * fs;
    float wk[8];
    float sum = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        float v = ((a[0][k >> 2] * a[1][(k >> 1) & 1]) * a[2][k & 1]) / cube;
        const int id = idx8[i * 8 + k];
        if (id < 0 || id >= Nv) v = 0.0f;
        wk[k] = v;
        sum += v;
    }
    const float denom = sum + 1e-8f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        float v = wk[k] / denom;
        if (nearest && k > 0) {  // (after the normalisation, as the reference does: no renormalisation follows)
            v = 0.0f;
            idx8[i * 8 + k] = -1;
        }
        w[i * 8 + k] = v;
    }
}

// ------------------------------------------------------------------------------------------------------ table inversion
__global__ __launch_bounds__(PV_BLOCK) void pv_invert_keys_kernel(const int *__restrict__ table, int64_t slots, int64_t Nv,
                                                                   unsigned long long *__restrict__ keys,
                                                                   unsigned int *__restrict__ vals)
{
    const int64_t l = (int64_t)blockIdx.x * PV_BLOCK + threadIdx.x;
    if (l >= slots) return;
    const int t = table[l];
    keys[l] = (t >= 0 && t < Nv) ? (unsigned long long)t : (unsigned long long)Nv;
    vals[l] = (unsigned int)l;
}

// start[v] = first sorted slot whose destination is >= v, v in [0, Nv]
__global__ __launch_bounds__(PV_BLOCK) void pv_invert_start_kernel(const unsigned long long *__restrict__ sorted, int64_t slots,
                                                                    int64_t Nv, int *__restrict__ start)
{
    const int64_t v = (int64_t)blockIdx.x * PV_BLOCK + threadIdx.x;
    if (v > Nv) return;
    start[v] = (int)lower_bound_u64(sorted, slots, (unsigned long long)v);
}

// ------------------------------------------------------------------------------------------------------ feature kernels
template <bool VEC>
struct PvRow;
template <>
struct PvRow<true> {
    typedef float4 T;
    static constexpr int W = 4;
    static __device__ __forceinline__ T zero() { return make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
    static __device__ __forceinline__ T load(const float *p) { return *reinterpret_cast<const float4 *>(p); }
    static __device__ __forceinline__ void store(float *p, T v) { *reinterpret_cast<float4 *>(p) = v; }
    static __device__ __forceinline__ T mul(float a, T v) { return make_float4(a * v.x, a * v.y, a * v.z, a * v.w); }
    static __device__ __forceinline__ T add(T a, T b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
};
template <>
struct PvRow<false> {
    typedef float T;
    static constexpr int W = 1;
    static __device__ __forceinline__ T zero() { return 0.0f; }
    static __device__ __forceinline__ T load(const float *p) { return *p; }
    static __device__ __forceinline__ void store(float *p, T v) { *p = v; }
    static __device__ __forceinline__ T mul(float a, T v) { return a * v; }
    static __device__ __forceinline__ T add(T a, T b) { return a + b; }
};

// out[p] = sum_k wk * src[table[p][k]], k ascending; 2^tl lanes per row, each taking every 2^tl-th group of W channels
template <int K, bool VEC>
__global__ __launch_bounds__(PV_BLOCK) void pv_gather_kernel(const float *__restrict__ src, const int *__restrict__ table,
                                                              const float *__restrict__ w, const float *__restrict__ scale,
                                                              int64_t N, int64_t Nsrc, int C, int tl, float *__restrict__ out)
{
    typedef PvRow<VEC> R;
    const int sub = threadIdx.x & ((1 << tl) - 1);
    const int64_t p = (int64_t)blockIdx.x * (PV_BLOCK >> tl) + (threadIdx.x >> tl);
    if (p >= N) return;
    int64_t row[K];
    float wk[K];
    bool has[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int id = table[p * K + k];
        has[k] = id >= 0 && id < Nsrc;
        row[k] = has[k] ? id : 0;  // (row 0 exists: the entry point returns zeros for Nsrc == 0)
        wk[k] = w ? w[p * K + k] : (scale ? scale[row[k]] : 1.0f);
    }
    const int groups = C / R::W;
    for (int c = sub; c < groups; c += 1 << tl) {
        typename R::T v[K];
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = R::load(src + row[k] * C + c * R::W);
        typename R::T acc = R::zero();
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const typename R::T t = R::mul(wk[k], v[k]);
            acc = R::add(acc, has[k] ? t : R::zero());
        }
        R::store(out + p * C + c * R::W, acc);
    }
}

// sum of w[l] * src[l >> ks] over the sorted slots [b, e), ascending, for this lane's channel group at column `col`
template <bool VEC>
__device__ __forceinline__ typename PvRow<VEC>::T pv_sum_slots(const float *__restrict__ src, const int *__restrict__ order,
                                                               const float *__restrict__ w, int b, int e, int64_t slots, int ks,
                                                               int64_t Nsrc, int C, int col)
{
    typedef PvRow<VEC> R;
    typename R::T acc = R::zero();
    for (int j = b; j < e; j += 4) {  // four independent slot -> row loads in flight, added in slot order
        int64_t r[4];
        float ww[4];
        bool has[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int l = j + u < e ? order[j + u] : -1;
            const bool ok = l >= 0 && l < slots && (l >> ks) < Nsrc;
            has[u] = ok;
            r[u] = ok ? (l >> ks) : 0;
            ww[u] = (ok && w) ? w[l] : 1.0f;
        }
        typename R::T v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = R::load(src + r[u] * C + col);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const typename R::T t = R::mul(ww[u], v[u]);
            acc = R::add(acc, has[u] ? t : R::zero());
        }
    }
    return acc;
}

// runs of at most PV_LONG_RUN slots: one team of 2^tl lanes per destination row
template <bool VEC>
__global__ __launch_bounds__(PV_BLOCK) void pv_runsum_kernel(const float *__restrict__ src, const int *__restrict__ start,
                                                              const int *__restrict__ order, const float *__restrict__ w,
                                                              const float *__restrict__ scale, int64_t Nv, int64_t slots, int ks,
                                                              int64_t Nsrc, int C, int tl, float *__restrict__ out)
{
    typedef PvRow<VEC> R;
    const int sub = threadIdx.x & ((1 << tl) - 1);
    const int64_t v = (int64_t)blockIdx.x * (PV_BLOCK >> tl) + (threadIdx.x >> tl);
    if (v >= Nv) return;
    const int b = max(start[v], 0);
    const int e = (int)min((int64_t)start[v + 1], slots);
    if (e - b > PV_LONG_RUN) return;  // pv_runsum_long_kernel writes this row
    const float sc = scale ? scale[v] : 1.0f;
    const int groups = C / R::W;
    for (int c = sub; c < groups; c += 1 << tl) {
        const typename R::T acc = pv_sum_slots<VEC>(src, order, w, b, e, slots, ks, Nsrc, C, c * R::W);
        R::store(out + v * C + c * R::W, R::mul(sc, acc));
    }
}

// longer runs: one workgroup per row, PV_PIECES teams of PV_LONG_LANES lanes, one contiguous piece each, pieces added in order
template <bool VEC>
__global__ __launch_bounds__(PV_BLOCK) void pv_runsum_long_kernel(const float *__restrict__ src, const int *__restrict__ start,
                                                                   const int *__restrict__ order, const float *__restrict__ w,
                                                                   const float *__restrict__ scale, int64_t Nv, int64_t slots,
                                                                   int ks, int64_t Nsrc, int C, float *__restrict__ out)
{
    typedef PvRow<VEC> R;
    __shared__ typename R::T s_part[PV_PIECES][PV_LONG_LANES];
    const int lane = threadIdx.x & (PV_LONG_LANES - 1), team = threadIdx.x / PV_LONG_LANES;
    const int groups = C / R::W;
    for (int64_t v = blockIdx.x; v < Nv; v += gridDim.x) {
        const int b = max(start[v], 0);
        const int e = (int)min((int64_t)start[v + 1], slots);
        const int n = e - b;
        if (n <= PV_LONG_RUN) continue;  // (workgroup-uniform)
        const int piece = (n + PV_PIECES - 1) / PV_PIECES;
        const int pb = min(e, b + team * piece), pe = min(e, pb + piece);
        const float sc = scale ? scale[v] : 1.0f;
        for (int c0 = 0; c0 < groups; c0 += PV_LONG_LANES) {
            const int c = c0 + lane;
            s_part[team][lane] = c < groups ? pv_sum_slots<VEC>(src, order, w, pb, pe, slots, ks, Nsrc, C, c * R::W) : R::zero();
            __syncthreads();
            if (team == 0 && c < groups) {
                typename R::T acc = s_part[0][lane];
#pragma unroll
                for (int t = 1; t < PV_PIECES; ++t) acc = R::add(acc, s_part[t][lane]);
                R::store(out + v * C + c * R::W, R::mul(sc, acc));
            }
            __syncthreads();
        }
    }
}

// lanes per row: the least power of two covering the row's channel groups, 64 at the most
static int pv_team_log2(int groups)
{
    int tl = 0;
    while ((1 << tl) < groups && tl < 6) ++tl;
    return tl;
}

static bool pv_vec_ok(int C, const void *a, const void *b)
{
    return (C & 3) == 0 && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0;
}

}  // namespace tp3d

using namespace tp3d;

TP3D_EXPORT int tp3d_pv_quantize_f32(const float *pc, int64_t N, int s, int32_t *q, void *stream)
{
    if (N < 0 || s < 1 || s >= (1 << 18)) return TP3D_E_BADARG;
    if (N == 0) return TP3D_OK;
    if (!pc || !q) return TP3D_E_BADARG;
    if (N >= 0x7fffffff) return TP3D_E_TOOBIG;
    hipLaunchKernelGGL(pv_quantize_kernel, dim3((unsigned)((N + PV_BLOCK - 1) / PV_BLOCK)), dim3(PV_BLOCK), 0, (hipStream_t)stream,
                       pc, N, s, q);
    return check_launch();
}

TP3D_EXPORT int tp3d_pv_trilinear_f32(const float *pc, int32_t *idx8, int64_t N, int64_t Nv, int s, int nearest, float *w,
                                      void *stream)
{
    if (N < 0 || Nv < 0 || s < 1 || s >= (1 << 18)) return TP3D_E_BADARG;
    if (N == 0) return TP3D_OK;
    if (!pc || !idx8 || !w) return TP3D_E_BADARG;
    if (N >= 0x7fffffff / 8 || Nv >= 0x7fffffff) return TP3D_E_TOOBIG;
    hipLaunchKernelGGL(pv_trilinear_kernel, dim3((unsigned)((N + PV_BLOCK - 1) / PV_BLOCK)), dim3(PV_BLOCK), 0, (hipStream_t)stream,
                       pc, idx8, N, Nv, s, nearest, w);
    return check_launch();
}

TP3D_EXPORT size_t tp3d_pv_invert_workspace_bytes(int64_t N, int K)
{
    if (N <= 0 || K <= 0 || N >= 0x7fffffff / K) return 0;
    return carve_sort_workspace(nullptr, N * K, false, false).bytes;
}

TP3D_EXPORT int tp3d_pv_invert_i32(const int32_t *table, int64_t N, int K, int64_t Nv, int32_t *start, int32_t *order,
                                   void *workspace, size_t workspace_bytes, void *stream)
{
    if (N < 0 || (K != 1 && K != 8) || Nv < 0 || !start) return TP3D_E_BADARG;
    if (N >= 0x7fffffff / K || Nv >= 0x7fffffff) return TP3D_E_TOOBIG;
    hipStream_t s = (hipStream_t)stream;
    const int64_t slots = N * K;
    if (slots == 0) return zero_async(start, (size_t)(Nv + 1) * sizeof(int32_t), s);
    if (!table || !order || !workspace) return TP3D_E_BADARG;
    SortWorkspace w = carve_sort_workspace(workspace, slots, false, false);  // the values are sorted into `order`
    if (workspace_bytes < w.bytes) return TP3D_E_BADARG;
    const unsigned blocks = (unsigned)((slots + PV_BLOCK - 1) / PV_BLOCK);
    hipLaunchKernelGGL(pv_invert_keys_kernel, dim3(blocks), dim3(PV_BLOCK), 0, s, table, slots, Nv, w.keys_in, w.vals_in);
    if (int rc = check_launch()) return rc;
    if (int rc = sort_pairs_u64_u32(w.tmp, w.tmp_bytes, w.keys_in, w.keys_out, w.vals_in, reinterpret_cast<unsigned int *>(order),
                                    slots, sort_bits((unsigned __int128)Nv + 1), s))  // the keys are 0 .. Nv
        return rc;
    hipLaunchKernelGGL(pv_invert_start_kernel, dim3((unsigned)((Nv + 1 + PV_BLOCK - 1) / PV_BLOCK)), dim3(PV_BLOCK), 0, s, w.keys_out,
                       slots, Nv, start);
    return check_launch();
}

TP3D_EXPORT int tp3d_pv_gather_f32(const float *src, const int32_t *table, const float *w, const float *scale, int64_t N, int K,
                                   int64_t Nsrc, int C, float *out, void *stream)
{
    if (N < 0 || Nsrc < 0 || (K != 1 && K != 8) || C <= 0) return TP3D_E_BADARG;
    if (N == 0) return TP3D_OK;
    if (!out) return TP3D_E_BADARG;
    if (N >= 0x7fffffff / K || Nsrc >= 0x7fffffff) return TP3D_E_TOOBIG;
    hipStream_t s = (hipStream_t)stream;
    if (Nsrc == 0) return zero_async(out, (size_t)N * C * sizeof(float), s);
    if (!src || !table) return TP3D_E_BADARG;
    const bool vec = pv_vec_ok(C, src, out);
    const int tl = pv_team_log2(vec ? C / 4 : C);
    const unsigned blocks = (unsigned)((N + (PV_BLOCK >> tl) - 1) / (PV_BLOCK >> tl));
#define PV_GATHER(KK, VV)                                                                                                      \
    hipLaunchKernelGGL((pv_gather_kernel<KK, VV>), dim3(blocks), dim3(PV_BLOCK), 0, s, src, table, w, scale, N, Nsrc, C, tl, out)
    if (K == 8) {
        if (vec) PV_GATHER(8, true);
        else PV_GATHER(8, false);
    } else {
        if (vec) PV_GATHER(1, true);
        else PV_GATHER(1, false);
    }
#undef PV_GATHER
    return check_launch();
}

TP3D_EXPORT int tp3d_pv_runsum_f32(const float *src, const int32_t *start, const int32_t *order, const float *w, const float *scale,
                                   int64_t Nv, int K, int64_t Nsrc, int C, float *out, void *stream)
{
    if (Nv < 0 || Nsrc < 0 || (K != 1 && K != 8) || C <= 0) return TP3D_E_BADARG;
    if (Nv == 0) return TP3D_OK;
    if (!out) return TP3D_E_BADARG;
    if (Nsrc >= 0x7fffffff / K || Nv >= 0x7fffffff) return TP3D_E_TOOBIG;
    hipStream_t s = (hipStream_t)stream;
    if (Nsrc == 0) return zero_async(out, (size_t)Nv * C * sizeof(float), s);
    if (!src || !start || !order) return TP3D_E_BADARG;
    const int64_t slots = Nsrc * K;
    const int ks = K == 8 ? 3 : 0;
    const bool vec = pv_vec_ok(C, src, out);
    const int tl = pv_team_log2(vec ? C / 4 : C);
    const unsigned blocks = (unsigned)((Nv + (PV_BLOCK >> tl) - 1) / (PV_BLOCK >> tl));
    if (vec)
        hipLaunchKernelGGL(pv_runsum_kernel<true>, dim3(blocks), dim3(PV_BLOCK), 0, s, src, start, order, w, scale, Nv, slots, ks,
                           Nsrc, C, tl, out);
    else
        hipLaunchKernelGGL(pv_runsum_kernel<false>, dim3(blocks), dim3(PV_BLOCK), 0, s, src, start, order, w, scale, Nv, slots, ks,
                           Nsrc, C, tl, out);
    if (int rc = check_launch()) return rc;
    // at most slots / (PV_LONG_RUN + 1) rows have a long run; the workgroups stride over the rows and skip the others
    int64_t longest = slots / (PV_LONG_RUN + 1);
    if (longest > Nv) longest = Nv;
    if (longest > 1024) longest = 1024;
    if (longest == 0) return TP3D_OK;
    if (vec)
        hipLaunchKernelGGL(pv_runsum_long_kernel<true>, dim3((unsigned)longest), dim3(PV_BLOCK), 0, s, src, start, order, w, scale,
                           Nv, slots, ks, Nsrc, C, out);
    else
        hipLaunchKernelGGL(pv_runsum_long_kernel<false>, dim3((unsigned)longest), dim3(PV_BLOCK), 0, s, src, start, order, w, scale,
                           Nv, slots, ks, Nsrc, C, out);
    return check_launch();
}
