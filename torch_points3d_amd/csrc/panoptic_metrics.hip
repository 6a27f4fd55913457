// Panoptic evaluation on the device: the best ground-truth instance of every cluster, the sparse cluster overlaps, the
// greedy suppression over them and the true-positive walk of the instance AP.
// Integer counters only: no float atomics, bit-reproducible, nothing read back by the host, and never a (K, N), (K, K) or
// (K, G) tensor.  Contracts: include/tp3d_hip.h ("Panoptic metrics").
#include "inverse_table.h"
#include "sorted_keys.h"

namespace tp3d {
namespace {

constexpr int PM_WINDOW = TP3D_CLUSTER_BEST_WINDOW;  // columns of one LDS histogram
constexpr int PM_SMALL = 256;                        // clusters of up to this many members take one wave, larger a workgroup
constexpr int PM_BLOCK = 256;
constexpr int PM_SCAN_BLOCK = 1024;
constexpr unsigned long long PM_NO_KEY = ~0ull;      // fills the pair keys behind the last pair

// the better of two candidates of a "first maximum": the larger value, of equal values the lower column
template <typename V>
__device__ __forceinline__ bool comes_first(V v, long long col, V best, long long best_col)
{
    return v > best || (v == best && col >= 0 && (best_col < 0 || col < best_col));
}

template <typename V>
__device__ __forceinline__ void wave_first_max(V &v, long long &col, long long &inter)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const V ov = __shfl_xor(v, off);
        const long long oc = __shfl_xor(col, off);
        const long long oi = __shfl_xor(inter, off);
        if (comes_first(ov, oc, v, col)) {
            v = ov;
            col = oc;
            inter = oi;
        }
    }
}

// One workgroup of THREADS lanes per cluster (THREADS = 64: clusters of up to PM_SMALL members; PM_BLOCK: the others).
// The members are counted per column of the cluster's cloud in an LDS histogram of PM_WINDOW columns, window after
// window over [col_lo, col_hi); every lane then walks its columns of the window in ascending order, so a strictly
// larger value is the first maximum of the lane, and the lanes are merged with "lower column wins".
template <int THREADS>
__global__ void __launch_bounds__(THREADS)
best_instance_kernel(const int64_t *__restrict__ members, const int64_t *__restrict__ starts, int64_t M,
                     const int64_t *__restrict__ column, int64_t N, const int64_t *__restrict__ gt_size,
                     const int64_t *__restrict__ gt_class, int64_t G, const int64_t *__restrict__ cluster_class,
                     const int64_t *__restrict__ col_lo, const int64_t *__restrict__ col_hi, int64_t *__restrict__ inter_all,
                     int64_t *__restrict__ col_all, int64_t *__restrict__ inter_cls, int64_t *__restrict__ col_cls)
{
    constexpr int WAVES = THREADS / 64;
    __shared__ int s_hist[PM_WINDOW];
    __shared__ float s_v32[WAVES];
    __shared__ double s_v64[WAVES];
    __shared__ long long s_c[2][WAVES], s_i[2][WAVES];
    const int64_t k = blockIdx.x;
    const int tid = threadIdx.x;
    int64_t s0 = starts[k], s1 = starts[k + 1];
    if (s0 < 0) s0 = 0;
    if (s1 > M) s1 = M;
    const int64_t size = s1 > s0 ? s1 - s0 : 0;
    if ((size > PM_SMALL) != (THREADS != 64)) return;  // the other launch serves this cluster
    int64_t lo = col_lo[k], hi = col_hi[k];
    if (lo < 0) lo = 0;
    if (hi > G) hi = G;
    const int64_t ccls = cluster_class[k];
    const float fsize = (float)size;
    float b32 = 0.0f;
    double b64 = 0.0;
    long long c_all = -1, i_all = 0, c_cls = -1, i_cls = 0;
    for (int64_t w0 = lo; w0 < hi; w0 += PM_WINDOW) {
        const int wn = (int)min((int64_t)PM_WINDOW, hi - w0);
        for (int j = tid; j < wn; j += THREADS) s_hist[j] = 0;
        __syncthreads();
        for (int64_t e = s0 + tid; e < s1; e += THREADS) {
            const int64_t p = members[e];
            if (p < 0 || p >= N) continue;
            const int64_t c = column[p];
            if (c >= w0 && c < w0 + wn) atomicAdd(&s_hist[(int)(c - w0)], 1);
        }
        __syncthreads();
        for (int j = tid; j < wn; j += THREADS) {
            const int inter = s_hist[j];
            if (inter == 0) continue;
            const int64_t col = w0 + j;
            const int64_t gs = gt_size[col];
            const float fi = (float)inter;
            const float iou = fi / fmaxf((fsize + (float)gs) - fi, 1.0f);
            if (iou > b32) {
                b32 = iou;
                c_all = col;
                i_all = inter;
            }
            if (gt_class[col] == ccls) {
                const double d = (double)inter / (double)(size + gs - inter);
                if (d > b64) {
                    b64 = d;
                    c_cls = col;
                    i_cls = inter;
                }
            }
        }
        __syncthreads();  // the histogram is read before the next window clears it
    }
    wave_first_max(b32, c_all, i_all);
    wave_first_max(b64, c_cls, i_cls);
    if (WAVES > 1) {
        const int wave = tid >> 6;
        if ((tid & 63) == 0) {
            s_v32[wave] = b32;
            s_v64[wave] = b64;
            s_c[0][wave] = c_all;
            s_i[0][wave] = i_all;
            s_c[1][wave] = c_cls;
            s_i[1][wave] = i_cls;
        }
        __syncthreads();
        if (tid == 0)
            for (int w = 1; w < WAVES; ++w) {
                if (comes_first(s_v32[w], s_c[0][w], b32, c_all)) {
                    b32 = s_v32[w];
                    c_all = s_c[0][w];
                    i_all = s_i[0][w];
                }
                if (comes_first(s_v64[w], s_c[1][w], b64, c_cls)) {
                    b64 = s_v64[w];
                    c_cls = s_c[1][w];
                    i_cls = s_i[1][w];
                }
            }
    }
    if (tid == 0) {
        inter_all[k] = c_all >= 0 ? i_all : 0;
        col_all[k] = c_all;
        inter_cls[k] = c_cls >= 0 ? i_cls : 0;
        col_cls[k] = c_cls;
    }
}

// ---------------------------------------------------------------------------------------------- sparse overlaps
__global__ void __launch_bounds__(PM_BLOCK)
slot_key_kernel(const int64_t *__restrict__ members, int64_t M, unsigned long long *__restrict__ keys,
                unsigned int *__restrict__ vals)
{
    const int64_t e = (int64_t)blockIdx.x * PM_BLOCK + threadIdx.x;
    if (e >= M) return;
    keys[e] = (unsigned long long)members[e];
    vals[e] = (unsigned int)e;
}

__device__ __forceinline__ int64_t owner_of(const int64_t *__restrict__ owner, const unsigned int *__restrict__ slot, int64_t s,
                                            int64_t K)
{
    const int64_t c = owner[slot[s]];
    return c < 0 ? 0 : (c >= K ? K - 1 : c);
}

// The clusters of the run of sorted slot s (one point) other than its own, each once: slots of one point are sorted by
// slot, so by cluster, and a cluster that lists the point twice shows as neighbouring equal owners.  Calls f(cluster)
// in ascending order; returns at once for a slot that repeats the (point, cluster) of the slot in front of it.
template <typename F>
__device__ __forceinline__ void for_other_clusters(const unsigned long long *__restrict__ keys, const unsigned int *__restrict__ slot,
                                                   const int64_t *__restrict__ owner, int64_t M, int64_t K, int64_t s, int64_t c, F f)
{
    const unsigned long long p = keys[s];
    if (s > 0 && keys[s - 1] == p && owner_of(owner, slot, s - 1, K) == c) return;
    int64_t a = s;
    while (a > 0 && keys[a - 1] == p) --a;
    int64_t prev = -1;
    for (int64_t t = a; t < M && keys[t] == p; ++t) {
        const int64_t ct = owner_of(owner, slot, t, K);
        if (ct != prev && ct != c) f(ct);
        prev = ct;
    }
}

// cnt[s] = ordered pairs that sorted slot s leads; stats[0] += their number (64-bit integer atomics, one per wave)
__global__ void __launch_bounds__(PM_BLOCK)
pair_count_kernel(const unsigned long long *__restrict__ keys, const unsigned int *__restrict__ slot,
                  const int64_t *__restrict__ owner, int64_t M, int64_t K, int *__restrict__ cnt, int64_t *__restrict__ stats)
{
    const int64_t s = (int64_t)blockIdx.x * PM_BLOCK + threadIdx.x;
    int n = 0;
    if (s < M) {
        const int64_t c = owner_of(owner, slot, s, K);
        for_other_clusters(keys, slot, owner, M, K, s, c, [&](int64_t) { ++n; });
        cnt[s] = n;
    }
    long long sum = n;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
    if ((threadIdx.x & 63) == 0 && sum)
        __hip_atomic_fetch_add(reinterpret_cast<unsigned long long *>(stats), (unsigned long long)sum, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
}

// exclusive scan of cnt[0..M) into off[0..M) by one workgroup (block_scan_chunk of the inverse-table core)
__global__ void __launch_bounds__(PM_SCAN_BLOCK)
pair_scan_kernel(const int *__restrict__ cnt, int64_t M, int *__restrict__ off)
{
    __shared__ int s_w[PM_SCAN_BLOCK / 64];
    int64_t k0, k1;
    int run = block_scan_chunk<PM_SCAN_BLOCK>(cnt, M, s_w, k0, k1);
    for (int64_t k = k0; k < k1; ++k) {
        const int v = cnt[k];
        off[k] = run;
        run += v;
    }
}

// pair keys own * K + other at off[s] ..; a key that would land outside [0, cap) is dropped (the call is then flagged)
__global__ void __launch_bounds__(PM_BLOCK)
pair_emit_kernel(const unsigned long long *__restrict__ keys, const unsigned int *__restrict__ slot,
                 const int64_t *__restrict__ owner, int64_t M, int64_t K, const int *__restrict__ cnt, const int *__restrict__ off,
                 int64_t cap, unsigned long long *__restrict__ pair_keys)
{
    const int64_t s = (int64_t)blockIdx.x * PM_BLOCK + threadIdx.x;
    if (s >= M || cnt[s] == 0) return;
    const int64_t c = owner_of(owner, slot, s, K);
    int64_t o = off[s];
    for_other_clusters(keys, slot, owner, M, K, s, c, [&](int64_t ct) {
        if (o >= 0 && o < cap) pair_keys[o] = (unsigned long long)c * (unsigned long long)K + (unsigned long long)ct;
        ++o;
    });
}

// the last slot of every run of equal pair keys writes the run: its id is the entry, its length the shared points
__global__ void __launch_bounds__(PM_BLOCK)
overlap_entry_kernel(const unsigned long long *__restrict__ keys, const int *__restrict__ cid, int64_t cap, int64_t K,
                     int64_t *__restrict__ ov_other, int64_t *__restrict__ ov_inter)
{
    const int64_t i = (int64_t)blockIdx.x * PM_BLOCK + threadIdx.x;
    if (i >= cap) return;
    const unsigned long long key = keys[i];
    if (key == PM_NO_KEY || (i + 1 < cap && keys[i + 1] == key)) return;
    const int64_t first = lower_bound_u64(keys, cap, key);
    const int64_t p = cid[i];
    if (p < 0 || p >= cap) return;
    ov_other[p] = (int64_t)(key % (unsigned long long)K);
    ov_inter[p] = i - first + 1;
}

// ov_start[k] = entries in front of cluster k; stats[1] = entries, stats[2] = 1 when the pairs did not fit `cap`
__global__ void __launch_bounds__(PM_BLOCK)
overlap_start_kernel(const unsigned long long *__restrict__ keys, const int *__restrict__ cid, int64_t cap, int64_t K,
                     int64_t *__restrict__ ov_start, int64_t *__restrict__ stats)
{
    const int64_t k = (int64_t)blockIdx.x * PM_BLOCK + threadIdx.x;
    if (k > K) return;
    const bool over = stats[0] > cap;
    int64_t at = 0;
    if (!over && cap > 0) {
        const int64_t lb = lower_bound_u64(keys, cap, (unsigned long long)k * (unsigned long long)K);
        at = lb < cap ? cid[lb] : (int64_t)cid[cap - 1] + (keys[cap - 1] == PM_NO_KEY ? 0 : 1);
    }
    ov_start[k] = at;
    if (k == K) {
        stats[1] = at;
        stats[2] = over ? 1 : 0;
    }
}

// ---------------------------------------------------------------------------------------------- suppression
__device__ __forceinline__ bool suppresses(int64_t inter, int64_t ni, int64_t nj, float thr)
{
    const float fi = (float)inter;
    return fi / (((float)ni + (float)nj) - fi) > thr;
}

// keep := 1; hot[k] = 1 when cluster k has a neighbour it suppresses (the relation is symmetric: or is suppressed by)
__global__ void __launch_bounds__(PM_BLOCK)
nms_mark_kernel(const int64_t *__restrict__ starts, const int64_t *__restrict__ ov_start, const int64_t *__restrict__ ov_other,
                const int64_t *__restrict__ ov_inter, int64_t K, int64_t P, float thr, uint8_t *__restrict__ keep,
                uint8_t *__restrict__ hot)
{
    const int64_t k = (int64_t)blockIdx.x * PM_BLOCK + threadIdx.x;
    if (k >= K) return;
    keep[k] = 1;
    int64_t e0 = ov_start[k], e1 = ov_start[k + 1];
    if (e0 < 0) e0 = 0;
    if (e1 > P) e1 = P;
    const int64_t ni = starts[k + 1] - starts[k];
    uint8_t h = 0;
    for (int64_t e = e0; e < e1 && !h; ++e) {
        const int64_t j = ov_other[e];
        if (j >= 0 && j < K && suppresses(ov_inter[e], ni, starts[j + 1] - starts[j], thr)) h = 1;
    }
    hot[k] = h;
}

// One workgroup walks the visiting order PM_BLOCK positions at a time; only the hot clusters of a chunk enter the serial
// part, where a cluster that is still alive clears its neighbours, the lanes spread over its neighbour list.
__global__ void __launch_bounds__(PM_BLOCK)
nms_walk_kernel(const int64_t *__restrict__ order, const int64_t *__restrict__ starts, const int64_t *__restrict__ ov_start,
                const int64_t *__restrict__ ov_other, const int64_t *__restrict__ ov_inter, int64_t K, int64_t P, float thr,
                const uint8_t *__restrict__ hot, volatile uint8_t *keep)
{
    __shared__ long long s_idx[PM_BLOCK];
    __shared__ int s_wave[PM_BLOCK / 64];
    const int tid = threadIdx.x, wave = tid >> 6;
    for (int64_t q0 = 0; q0 < K; q0 += PM_BLOCK) {
        long long mine = -1;
        if (q0 + tid < K) {
            const int64_t i = order[q0 + tid];
            if (i >= 0 && i < K && hot[i]) mine = i;
        }
        // the hot clusters of the chunk, packed in visiting order
        const unsigned long long hot_lanes = __ballot(mine >= 0);
        if ((tid & 63) == 0) s_wave[wave] = __popcll(hot_lanes);
        __syncthreads();
        int base = 0, n = 0;
#pragma unroll
        for (int w = 0; w < PM_BLOCK / 64; ++w) {
            const int c = s_wave[w];
            base += w < wave ? c : 0;
            n += c;
        }
        if (mine >= 0) s_idx[base + lanes_below(hot_lanes)] = mine;
        __syncthreads();
        for (int t = 0; t < n; ++t) {
            const long long i = s_idx[t];
            if (keep[i]) {  // every lane reads the same byte: the branch is uniform
                int64_t e0 = ov_start[i], e1 = ov_start[i + 1];
                if (e0 < 0) e0 = 0;
                if (e1 > P) e1 = P;
                const int64_t ni = starts[i + 1] - starts[i];
                for (int64_t e = e0 + tid; e < e1; e += PM_BLOCK) {
                    const int64_t j = ov_other[e];
                    if (j >= 0 && j < K && j != i && suppresses(ov_inter[e], ni, starts[j + 1] - starts[j], thr)) keep[j] = 0;
                }
            }
            __syncthreads();  // the cleared flags are visible to the next visit
        }
        __syncthreads();  // s_idx is rewritten
    }
}

// ---------------------------------------------------------------------------------------------- instance AP
// The sibling of ap_match_kernel (detection.hip) for instances: position p of the grouped order leads a (cloud, class)
// group when position p - 1 belongs to another; the leader walks its group.  An instance belongs to one group only, so
// its `taken` flag has a single writer.  The IoU is formed here in float64 from the integers and compared with >=.
__global__ void __launch_bounds__(PM_BLOCK)
instance_ap_match_kernel(const int64_t *__restrict__ order, const int64_t *__restrict__ cls, const int64_t *__restrict__ cloud,
                         const uint8_t *__restrict__ valid, int64_t K, const int64_t *__restrict__ size,
                         const int64_t *__restrict__ inter_cls, const int64_t *__restrict__ col_cls,
                         const int64_t *__restrict__ gt_size, int64_t G, double thr, uint8_t *__restrict__ taken,
                         uint8_t *__restrict__ tp)
{
    const int64_t p = (int64_t)blockIdx.x * PM_BLOCK + threadIdx.x;
    if (p >= K) return;
    const int64_t d0 = order[p];
    if (d0 < 0 || d0 >= K) return;
    const int64_t c = cls[d0], sc = cloud[d0];
    if (p > 0) {
        const int64_t dp = order[p - 1];
        if (dp >= 0 && dp < K && cls[dp] == c && cloud[dp] == sc) return;
    }
    for (int64_t q = p; q < K; ++q) {
        const int64_t d = order[q];
        if (d < 0 || d >= K || cls[d] != c || cloud[d] != sc) break;
        uint8_t hit = 0;
        const int64_t j = col_cls[d];
        if (valid[d] && j >= 0 && j < G) {
            const int64_t inter = inter_cls[d];
            const double iou = (double)inter / (double)(size[d] + gt_size[j] - inter);
            if (iou >= thr && !taken[j]) {
                taken[j] = 1;
                hit = 1;
            }
        }
        tp[d] = hit;
    }
}

struct OverlapCountWorkspace {
    SortWorkspace sort;
    int *cnt, *off;
    size_t bytes;
};

OverlapCountWorkspace carve_count_workspace(void *ws, int64_t M)
{
    OverlapCountWorkspace w;
    w.sort = carve_sort_workspace(ws, M, true, false);
    char *p = static_cast<char *>(ws);
    size_t at = align_up(w.sort.bytes, 256);
    w.cnt = reinterpret_cast<int *>(p + at);
    at += align_up((size_t)M * 4, 256);
    w.off = reinterpret_cast<int *>(p + at);
    at += align_up((size_t)M * 4, 256);
    w.bytes = at;
    return w;
}

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + PM_BLOCK - 1) / PM_BLOCK); }

constexpr int64_t PM_MAX = 0x7fffffff;

}  // namespace
}  // namespace tp3d

using namespace tp3d;

TP3D_EXPORT int tp3d_cluster_best_window(void) { return TP3D_CLUSTER_BEST_WINDOW; }

TP3D_EXPORT int tp3d_cluster_best_instance(const int64_t *members, const int64_t *starts, int64_t M, int64_t K,
                                           const int64_t *column, int64_t N, const int64_t *gt_size, const int64_t *gt_class,
                                           int64_t G, const int64_t *cluster_class, const int64_t *col_lo, const int64_t *col_hi,
                                           int64_t *inter_all, int64_t *col_all, int64_t *inter_cls, int64_t *col_cls, void *stream)
{
    if (M < 0 || K < 0 || N < 0 || G < 0) return TP3D_E_BADARG;
    if (K == 0) return TP3D_OK;
    if (K > PM_MAX) return TP3D_E_TOOBIG;
    if (!starts || !cluster_class || !col_lo || !col_hi || !inter_all || !col_all || !inter_cls || !col_cls) return TP3D_E_BADARG;
    if ((M > 0 && !members) || (N > 0 && !column) || (G > 0 && (!gt_size || !gt_class))) return TP3D_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(best_instance_kernel<64>, dim3((unsigned)K), dim3(64), 0, s, members, starts, M, column, N, gt_size,
                       gt_class, G, cluster_class, col_lo, col_hi, inter_all, col_all, inter_cls, col_cls);
    if (int rc = check_launch()) return rc;
    hipLaunchKernelGGL(best_instance_kernel<PM_BLOCK>, dim3((unsigned)K), dim3(PM_BLOCK), 0, s, members, starts, M, column, N,
                       gt_size, gt_class, G, cluster_class, col_lo, col_hi, inter_all, col_all, inter_cls, col_cls);
    return check_launch();
}

TP3D_EXPORT size_t tp3d_cluster_overlap_count_workspace_bytes(int64_t M)
{
    if (M <= 0 || M > PM_MAX) return 0;
    return carve_count_workspace(nullptr, M).bytes;
}

TP3D_EXPORT size_t tp3d_cluster_overlap_emit_workspace_bytes(int64_t cap)
{
    if (cap <= 0 || cap > PM_MAX) return 0;
    return carve_sort_workspace(nullptr, cap, true, true).bytes;
}

TP3D_EXPORT int tp3d_cluster_overlap_count(const int64_t *members, const int64_t *member_cluster, int64_t M, int64_t K,
                                           int point_bits, int64_t *stats, void *workspace, size_t workspace_bytes, void *stream)
{
    if (M < 0 || K < 0 || point_bits < 1 || point_bits > 63 || !stats) return TP3D_E_BADARG;
    if (M > PM_MAX || K > PM_MAX) return TP3D_E_TOOBIG;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = zero_async(stats, 3 * sizeof(int64_t), s)) return rc;
    if (M == 0 || K == 0) return TP3D_OK;
    if (!members || !member_cluster || !workspace) return TP3D_E_BADARG;
    OverlapCountWorkspace w = carve_count_workspace(workspace, M);
    if (workspace_bytes < w.bytes) return TP3D_E_BADARG;
    hipLaunchKernelGGL(slot_key_kernel, dim3(blocks_for(M)), dim3(PM_BLOCK), 0, s, members, M, w.sort.keys_in, w.sort.vals_in);
    if (int rc = check_launch()) return rc;
    if (int rc = sort_pairs_u64_u32(w.sort.tmp, w.sort.tmp_bytes, w.sort.keys_in, w.sort.keys_out, w.sort.vals_in,
                                    w.sort.vals_out, M, (unsigned)point_bits, s))
        return rc;
    hipLaunchKernelGGL(pair_count_kernel, dim3(blocks_for(M)), dim3(PM_BLOCK), 0, s, w.sort.keys_out, w.sort.vals_out,
                       member_cluster, M, K, w.cnt, stats);
    return check_launch();
}

TP3D_EXPORT int tp3d_cluster_overlap_emit(const int64_t *member_cluster, int64_t M, int64_t K, int64_t cap, int64_t *ov_start,
                                          int64_t *ov_other, int64_t *ov_inter, int64_t *stats, void *count_workspace,
                                          size_t count_workspace_bytes, void *workspace, size_t workspace_bytes, void *stream)
{
    if (M < 0 || K < 0 || cap < 0 || !stats || !ov_start) return TP3D_E_BADARG;
    if (M > PM_MAX || K > PM_MAX || cap > PM_MAX) return TP3D_E_TOOBIG;
    hipStream_t s = (hipStream_t)stream;
    SortWorkspace w2;
    w2.keys_out = nullptr;
    w2.cid = nullptr;
    if (cap > 0 && M > 0 && K > 0) {
        if (!member_cluster || !ov_other || !ov_inter || !count_workspace || !workspace) return TP3D_E_BADARG;
        OverlapCountWorkspace w = carve_count_workspace(count_workspace, M);
        w2 = carve_sort_workspace(workspace, cap, true, true);
        if (count_workspace_bytes < w.bytes || workspace_bytes < w2.bytes) return TP3D_E_BADARG;
        hipLaunchKernelGGL(pair_scan_kernel, dim3(1), dim3(PM_SCAN_BLOCK), 0, s, w.cnt, M, w.off);
        if (int rc = check_launch()) return rc;
        if (int rc = hip_rc(hipMemsetAsync(w2.keys_in, 0xff, (size_t)cap * 8, s))) return rc;
        hipLaunchKernelGGL(pair_emit_kernel, dim3(blocks_for(M)), dim3(PM_BLOCK), 0, s, w.sort.keys_out, w.sort.vals_out,
                           member_cluster, M, K, w.cnt, w.off, cap, w2.keys_in);
        if (int rc = check_launch()) return rc;
        // the unused low bits of PM_NO_KEY are all ones, above the largest pair key K * K - 2
        const unsigned bits = sort_bits((unsigned __int128)K * (unsigned __int128)K);
        if (int rc = sort_pairs_u64_u32(w2.tmp, w2.tmp_bytes, w2.keys_in, w2.keys_out, w2.vals_in, w2.vals_out, cap, bits, s))
            return rc;
        if (int rc = run_ids(w2.keys_out, cap, w2, s)) return rc;
        hipLaunchKernelGGL(overlap_entry_kernel, dim3(blocks_for(cap)), dim3(PM_BLOCK), 0, s, w2.keys_out, w2.cid, cap, K,
                           ov_other, ov_inter);
        if (int rc = check_launch()) return rc;
    } else {
        cap = 0;
    }
    hipLaunchKernelGGL(overlap_start_kernel, dim3(blocks_for(K + 1)), dim3(PM_BLOCK), 0, s, w2.keys_out, w2.cid, cap, K, ov_start,
                       stats);
    return check_launch();
}

TP3D_EXPORT int tp3d_cluster_nms(const int64_t *order, const int64_t *starts, int64_t K, const int64_t *ov_start,
                                 const int64_t *ov_other, const int64_t *ov_inter, int64_t P, float threshold, uint8_t *hot,
                                 uint8_t *keep, void *stream)
{
    if (K < 0 || P < 0) return TP3D_E_BADARG;
    if (K == 0) return TP3D_OK;
    if (K > PM_MAX) return TP3D_E_TOOBIG;
    if (!order || !starts || !ov_start || !hot || !keep || (P > 0 && (!ov_other || !ov_inter))) return TP3D_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(nms_mark_kernel, dim3(blocks_for(K)), dim3(PM_BLOCK), 0, s, starts, ov_start, ov_other, ov_inter, K, P,
                       threshold, keep, hot);
    if (int rc = check_launch()) return rc;
    if (P == 0) return TP3D_OK;
    hipLaunchKernelGGL(nms_walk_kernel, dim3(1), dim3(PM_BLOCK), 0, s, order, starts, ov_start, ov_other, ov_inter, K, P,
                       threshold, hot, keep);
    return check_launch();
}

TP3D_EXPORT int tp3d_instance_ap_match(const int64_t *order, const int64_t *cls, const int64_t *cloud, const uint8_t *valid,
                                       int64_t K, const int64_t *size, const int64_t *inter_cls, const int64_t *col_cls,
                                       const int64_t *gt_size, int64_t G, double threshold, uint8_t *taken, uint8_t *tp,
                                       void *stream)
{
    if (K < 0 || G < 0) return TP3D_E_BADARG;
    if (K == 0) return TP3D_OK;
    if (K > PM_MAX) return TP3D_E_TOOBIG;
    if (!order || !cls || !cloud || !valid || !size || !inter_cls || !col_cls || !tp) return TP3D_E_BADARG;
    if (G > 0 && (!gt_size || !taken)) return TP3D_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = zero_async(taken, (size_t)G, s)) return rc;
    hipLaunchKernelGGL(instance_ap_match_kernel, dim3(blocks_for(K)), dim3(PM_BLOCK), 0, s, order, cls, cloud, valid, K, size,
                       inter_cls, col_cls, gt_size, G, threshold, taken, tp);
    return check_launch();
}
