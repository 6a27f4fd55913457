// Region growing of PointGroup on the device: the connected components of a radius graph
// (reference models/panoptic/pointgroup.py:98-121, torch_points_kernels.region_grow).
//
// Two points are joined when they carry the same label, sit in the same cloud, the label is not ignored and
// sqdist3(p_i, p_j) < r2, with r2 = radius * radius formed as the partial-dense ball query forms it: membership is the
// ball query's.  (a - b)^2 == (b - a)^2 exactly in fp32, so the test is symmetric and the graph undirected.
//
// Pipeline (sorted-key core + the block scan of the inverse-table core; memory proportional to N, one stream, no host
// read in between):
//   1. integer bounding box of the cells of the kept points (box8_reduce_to); cell edge 1.01 * radius, as grid.hip: a
//      pair inside the ball is at most one cell apart whatever the fp32 rounding of the cell coordinate;
//   2. key = label | cloud | cz+1 | cy+1 | cx+1 (12 | 10 | 14 | 14 | 14 bits), one stable radix sort, a cell-ordered
//      float4 copy of the points (x, y, z, point index as int bits).  What does not fit a field raises a flag in the
//      stats words and is left out; nothing wraps;
//   3. one wave per point: the 27 cells around it are nine x-runs whose keys are consecutive, so each run is one pair of
//      binary searches in the sorted keys (lanes 0..8 and 16..24 search the eighteen bounds at once).  Every hit is
//      counted (the row length of an uncapped ball query), every hit with a lower index is united with the point in a
//      min-root union-find: the larger root is hooked under the smaller by a compare-and-swap on the root, so the root
//      of a finished component is its lowest point index whatever the execution order -- the result is deterministic;
//   4. parent[i] = root(i) in a launch of its own;
//   5. a second stable sort of (label, root) with the point index as value: runs = components in (label, lowest member)
//      order, members ascending; run ids, run lengths, a one-workgroup scan of the kept runs, one scatter.
//
// Visibility: inside the hook kernel every access to parent[] is an agent-scope relaxed atomic (load, compare-and-swap
// or min) -- per-XCD L2s are not coherent and a CU's L1 is never refreshed by another CU's stores.  No fences, no
// payload hand-off, and no wave ever waits for another: rg_find only follows strictly decreasing ids, and a failed
// compare-and-swap means another thread has lowered that root, so the larger of the two ids strictly decreases with
// every round of rg_hook.
#include "inverse_table.h"
#include "sorted_keys.h"

namespace tp3d {

constexpr int RG_BLOCK = SK_BLOCK;          // 4 waves, one point per wave in the hook kernel
constexpr int RG_SCAN_BLOCK = 1024;         // the one workgroup that scans the runs
constexpr int RG_CELL_BITS = 14;
constexpr int RG_CELL_MAX = (1 << RG_CELL_BITS) - 3;  // largest cell coordinate relative to the box: c + 1 +- 1 fits
constexpr int RG_CLOUD_BITS = 10;
constexpr int RG_LABEL_MAX = 4094;          // 12 bits, 4095 is the key of a point that is left out
constexpr int RG_COORD_LIMIT = 1 << 24;
constexpr unsigned long long RG_DEAD = ~0ull;
constexpr int RG_ROOT_BITS = 31;
constexpr unsigned long long RG_DEAD2 = 1ull << (RG_ROOT_BITS + 12);  // above every (label, root) key
constexpr int RG_FLAG_LABEL = 1, RG_FLAG_CLOUD = 2, RG_FLAG_COORD = 4, RG_FLAG_CELLS = 8;

__device__ __forceinline__ int rg_cell(float p, float inv_cell)
{
    const float c = floorf(p * inv_cell);
    return (int)fminf(fmaxf(c, -(float)RG_COORD_LIMIT), (float)RG_COORD_LIMIT);
}

__device__ __forceinline__ bool rg_ignored(int64_t label, const int64_t *__restrict__ ignore, int n_ignore)
{
    bool ig = false;
    for (int k = 0; k < n_ignore; ++k) ig |= ignore[k] == label;
    return ig;
}

// flag bits of point i, or -1 when its label is ignored
__device__ __forceinline__ int rg_classify(int64_t label, int64_t cloud, const int64_t *__restrict__ ignore, int n_ignore)
{
    if (rg_ignored(label, ignore, n_ignore)) return -1;
    return ((label < 0 || label > RG_LABEL_MAX) ? RG_FLAG_LABEL : 0) |
           ((cloud < 0 || cloud >= (1 << RG_CLOUD_BITS)) ? RG_FLAG_CLOUD : 0);
}

// bounds = [min cx,cy,cz | max cx,cy,cz | unused | flags] over the kept points; a point whose cell coordinate is
// beyond the limit raises its flag and stays out of the box
__global__ __launch_bounds__(RG_BLOCK) void rg_bounds_kernel(const float *__restrict__ pos, const int64_t *__restrict__ labels,
                                                             const int64_t *__restrict__ batch, int64_t N,
                                                             const int64_t *__restrict__ ignore, int n_ignore,
                                                             float inv_cell, int *__restrict__ bounds)
{
    int mn[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff};
    int mx[3] = {(int)0x80000000, (int)0x80000000, (int)0x80000000};
    int bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * RG_BLOCK + threadIdx.x; i < N; i += (int64_t)gridDim.x * RG_BLOCK) {
        const int cls = rg_classify(labels[i], batch[i], ignore, n_ignore);
        if (cls < 0) continue;
        bad |= cls;
        if (cls) continue;
        int c[3];
        bool far = false;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            c[a] = rg_cell(pos[i * 3 + a], inv_cell);
            far |= c[a] <= -RG_COORD_LIMIT || c[a] >= RG_COORD_LIMIT;
        }
        if (far) {
            bad |= RG_FLAG_COORD;
            continue;
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            mn[a] = min(mn[a], c[a]);
            mx[a] = max(mx[a], c[a]);
        }
    }
    int v[8] = {mn[0], mn[1], mn[2], mx[0], mx[1], mx[2], (int)0x80000000, bad};
    box8_reduce_to(v, bounds);
}

// keys, vals = iota, parent[i] = i (-1 for a point that is left out); the flags go to stats[3]
__global__ __launch_bounds__(RG_BLOCK) void rg_key_kernel(const float *__restrict__ pos, const int64_t *__restrict__ labels,
                                                          const int64_t *__restrict__ batch, int64_t N,
                                                          const int64_t *__restrict__ ignore, int n_ignore, float inv_cell,
                                                          const int *__restrict__ bounds,
                                                          unsigned long long *__restrict__ keys,
                                                          unsigned int *__restrict__ vals, int *__restrict__ parent,
                                                          int *__restrict__ stats)
{
    const int64_t i = (int64_t)blockIdx.x * RG_BLOCK + threadIdx.x;
    if (i >= N) return;
    const int64_t label = labels[i], cloud = batch[i];
    const int cls = rg_classify(label, cloud, ignore, n_ignore);
    bool live = cls == 0;
    unsigned long long key = RG_DEAD;
    int wide = 0;
    if (live) {
        unsigned long long cell = 0;
#pragma unroll
        for (int a = 2; a >= 0; --a) {  // z slowest, x fastest: the x-neighbours of a cell have consecutive keys
            // (a coordinate beyond the limit raised its flag in the bounds pass and is left out here)
            const int c = rg_cell(pos[i * 3 + a], inv_cell);
            const int64_t rel = (int64_t)c - (int64_t)bounds[a];
            wide |= (rel < 0 || rel > RG_CELL_MAX || c <= -RG_COORD_LIMIT || c >= RG_COORD_LIMIT) ? 1 : 0;
            cell = (cell << RG_CELL_BITS) | (unsigned long long)(rel + 1);
        }
        live = !wide;  // a box of more than RG_CELL_MAX + 1 cells along an axis: flagged, never wrapped
        if (live)
            key = ((((unsigned long long)label << RG_CLOUD_BITS) | (unsigned long long)cloud) << (3 * RG_CELL_BITS)) | cell;
    }
    keys[i] = key;
    vals[i] = (unsigned int)i;
    parent[i] = live ? (int)i : -1;
    if (i == 0) {
        int f = bounds[7];
#pragma unroll
        for (int a = 0; a < 3; ++a)
            f |= (bounds[3 + a] >= bounds[a] && (int64_t)bounds[3 + a] - bounds[a] > RG_CELL_MAX) ? RG_FLAG_CELLS : 0;
        stats[3] = f;
    }
}

__global__ __launch_bounds__(RG_BLOCK) void rg_fill_kernel(const float *__restrict__ pos, const unsigned int *__restrict__ vals,
                                                           int64_t N, float4 *__restrict__ sorted_pt)
{
    const int64_t t = (int64_t)blockIdx.x * RG_BLOCK + threadIdx.x;
    if (t >= N) return;
    const int64_t p = vals[t];
    sorted_pt[t] = make_float4(pos[p * 3 + 0], pos[p * 3 + 1], pos[p * 3 + 2], __int_as_float((int)p));
}

__device__ __forceinline__ int rg_load(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// root of x; `first` = parent[x] as it was read.  parent[y] <= y always and < y below a root: the walk strictly descends.
__device__ __forceinline__ int rg_find(const int *parent, int x, int &first)
{
    int p = rg_load(parent + x);
    first = p;
    while (p != x) {
        x = p;
        p = rg_load(parent + x);
    }
    return x;
}

// unites the sets of a and b.  Only roots are ever hooked, and only under a smaller id, so a root is the lowest id of
// its set.  A failed compare-and-swap returns where another thread has hooked a: an id below a, from which the next
// round goes on, and b never grows -- max(a, b) strictly decreases per round.
__device__ __forceinline__ void rg_hook(int *parent, int a, int b)
{
    int unused;
    while (true) {
        a = rg_find(parent, a, unused);
        b = rg_find(parent, b, unused);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicCAS(parent + a, a, b);
        if (old == a) return;
        a = old;
    }
}

// One wave per sorted slot (the waves of a workgroup share a cell or neighbouring ones).  stats[0] = largest hit count.
__global__ __launch_bounds__(RG_BLOCK) void rg_hook_kernel(const unsigned long long *__restrict__ keys,
                                                           const float4 *__restrict__ sorted_pt, int N, float r2,
                                                           int *parent, int *stats)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t t64 = (int64_t)blockIdx.x * (RG_BLOCK / 64) + wave;
    if (t64 >= N) return;  // wave-uniform, no workgroup barrier in this kernel
    const int t = (int)t64;
    const unsigned long long key = keys[t];
    if (key == RG_DEAD) return;
    const float4 q = sorted_pt[t];
    const int i = __float_as_int(q.w);
    // lanes 0..8: first slot of the run of row (dz, dy), lanes 16..24: the slot behind it.  The fields hold c + 1, so
    // -1 / +1 per field neither borrows nor carries; + 2 on the x field may carry into y, which as a number is still
    // the bound behind every key of the row.
    int bound = 0;
    {
        const int r = lane & 15;
        if (r < 9 && lane < 32) {
            const long long dz = r / 3 - 1, dy = r % 3 - 1;
            const unsigned long long row = key + (unsigned long long)(dz * (1ll << (2 * RG_CELL_BITS)) + dy * (1ll << RG_CELL_BITS));
            bound = (int)lower_bound_u64(keys, N, lane < 16 ? row - 1 : row + 2);
        }
    }
    int cnt = 0;
#pragma unroll
    for (int rr = 0; rr < 9; ++rr) {
        const int j0 = __builtin_amdgcn_readlane(bound, rr), j1 = __builtin_amdgcn_readlane(bound, 16 + rr);
        for (int j = j0; j < j1; j += 64) {
            const int tt = j + lane;
            const bool valid = tt < j1;
            const float4 pt = sorted_pt[valid ? tt : j0];
            const float d = sqdist3(pt.x, pt.y, pt.z, q.x, q.y, q.z);
            const bool hit = valid && d < r2;
            cnt += __builtin_popcountll(__ballot(hit));
            const int id = __float_as_int(pt.w);
            // the graph is undirected: the edge (i, id) is also seen from id, so the higher end unites
            const bool link = hit && id < i;
            const unsigned long long links = __ballot(link);
            if (links == 0) continue;
            int first;
            const int r = rg_find(parent, link ? id : i, first);
            int m = r;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) m = min(m, __shfl_xor(m, off));
            // one lane per distinct root hooks it under the wave's lowest
            unsigned long long pending = __ballot(r != m);
            while (pending) {
                const int leader = __builtin_ctzll(pending);
                const int rl = __shfl(r, leader);
                if (lane == leader) rg_hook(parent, rl, m);
                pending &= ~__ballot(r == rl);
            }
            // a lane without a link walks from the point itself; when all 64 lanes hold one (64 lower-indexed
            // neighbours in one stretch of a run) none has, and the point is united here
            if (links == ~0ull && lane == 0) rg_hook(parent, i, m);
            // shorten the paths: m is now in the set of every lane's point and no larger than its root was; a root is
            // the lowest id of its set, so this never lowers a root's own entry
            if ((link || lane == 0) && first > m) atomicMin(parent + (link ? id : i), m);
        }
    }
    if (lane == 0 && cnt > rg_load(stats)) atomicMax(stats, cnt);
}

// A launch of its own: parent[] is final and read with plain loads.
__global__ __launch_bounds__(RG_BLOCK) void rg_flatten_kernel(const int *__restrict__ parent, const int64_t *__restrict__ labels,
                                                              int64_t N,
                                                              unsigned long long *__restrict__ keys,
                                                              unsigned int *__restrict__ vals)
{
    const int64_t i = (int64_t)blockIdx.x * RG_BLOCK + threadIdx.x;
    if (i >= N) return;
    int x = (int)i, p = parent[x];
    if (p < 0) x = -1;
    else
        while (p != x) {
            x = p;
            p = parent[x];
        }
    keys[i] = x < 0 ? RG_DEAD2 : (((unsigned long long)labels[i] << RG_ROOT_BITS) | (unsigned long long)x);
    vals[i] = (unsigned int)i;
}

// run_start[c] = first slot of run c; run_start[runs] = N; meta[0] = runs
__global__ __launch_bounds__(RG_BLOCK) void rg_runs_kernel(const int *__restrict__ cid, int64_t N, int *__restrict__ run_start,
                                                           int *__restrict__ meta)
{
    const int64_t t = (int64_t)blockIdx.x * RG_BLOCK + threadIdx.x;
    if (t >= N) return;
    const int c = cid[t];
    if (t == 0 || cid[t - 1] != c) run_start[c] = (int)t;
    if (t == N - 1) {
        run_start[c + 1] = (int)N;
        meta[0] = c + 1;
    }
}

// One workgroup: which runs stay, their new ids and the slots in front of them (block_scan_chunk of the inverse-table core).
__global__ __launch_bounds__(RG_SCAN_BLOCK) void rg_scan_kernel(const unsigned long long *__restrict__ keys,
                                                                const int *__restrict__ run_start, const int *__restrict__ meta,
                                                                const int64_t *__restrict__ batch, int64_t min_size,
                                                                int *__restrict__ cnt_k, int *__restrict__ cnt_m,
                                                                int *__restrict__ newid, int *__restrict__ outstart,
                                                                int64_t *__restrict__ starts, int64_t *__restrict__ cluster_label,
                                                                int64_t *__restrict__ cluster_cloud, int *__restrict__ stats)
{
    __shared__ int s_wave_k[RG_SCAN_BLOCK / 64], s_wave_m[RG_SCAN_BLOCK / 64];
    const int runs = meta[0];
    for (int r = threadIdx.x; r < runs; r += RG_SCAN_BLOCK) {
        const int len = run_start[r + 1] - run_start[r];
        const bool keep = keys[run_start[r]] != RG_DEAD2 && (int64_t)len >= min_size;
        cnt_k[r] = keep ? 1 : 0;
        cnt_m[r] = keep ? len : 0;
    }
    __syncthreads();
    int k0, k1;
    int run_k = block_scan_chunk<RG_SCAN_BLOCK>(cnt_k, runs, s_wave_k, k0, k1);
    int run_m = block_scan_chunk<RG_SCAN_BLOCK>(cnt_m, runs, s_wave_m, k0, k1);
    for (int r = k0; r < k1; ++r) {
        outstart[r] = run_m;
        if (cnt_k[r]) {
            const unsigned long long key = keys[run_start[r]];
            newid[r] = run_k;
            starts[run_k] = run_m;
            cluster_label[run_k] = (int64_t)(key >> RG_ROOT_BITS);
            cluster_cloud[run_k] = batch[key & ((1ull << RG_ROOT_BITS) - 1)];
            ++run_k;
            run_m += cnt_m[r];
        } else {
            newid[r] = -1;
        }
    }
    if (k0 < k1 && k1 == runs) {  // the thread that owns the last run
        starts[run_k] = run_m;
        stats[1] = run_k;
        stats[2] = run_m;
    }
}

__global__ __launch_bounds__(RG_BLOCK) void rg_members_kernel(const unsigned int *__restrict__ vals, const int *__restrict__ cid,
                                                              const int *__restrict__ run_start, const int *__restrict__ newid,
                                                              const int *__restrict__ outstart, int64_t N,
                                                              int64_t *__restrict__ members, int64_t *__restrict__ member_cluster)
{
    const int64_t t = (int64_t)blockIdx.x * RG_BLOCK + threadIdx.x;
    if (t >= N) return;
    const int c = cid[t], id = newid[c];
    if (id < 0) return;
    const int64_t o = (int64_t)outstart[c] + (t - run_start[c]);  // o < N: the kept runs are a subset of the slots
    members[o] = vals[t];
    member_cluster[o] = id;
}

// bounds[8] + meta | sort (N, values, run ids) | sorted_pt | parent | run_start (N + 1) | newid | outstart | cnt_k | cnt_m
struct RegionGrowWorkspace {
    int *bounds, *meta;
    SortWorkspace sort;
    float4 *sorted_pt;
    int *parent, *run_start, *newid, *outstart, *cnt_k, *cnt_m;
    size_t bytes;
};

static RegionGrowWorkspace carve_region_grow_workspace(void *ws, int64_t N)
{
    char *p = static_cast<char *>(ws);
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char *at = p + off;
        off += align_up(bytes, 256);
        return at;
    };
    RegionGrowWorkspace w;
    w.bounds = reinterpret_cast<int *>(take(16 * 4));
    w.meta = w.bounds + 8;
    w.sort = carve_sort_workspace(take(0), N, true, true);
    off += w.sort.bytes;
    w.sorted_pt = reinterpret_cast<float4 *>(take((size_t)N * 16));
    w.parent = reinterpret_cast<int *>(take((size_t)N * 4));
    w.run_start = reinterpret_cast<int *>(take((size_t)(N + 1) * 4));
    w.newid = reinterpret_cast<int *>(take((size_t)N * 4));
    w.outstart = reinterpret_cast<int *>(take((size_t)N * 4));
    w.cnt_k = reinterpret_cast<int *>(take((size_t)N * 4));
    w.cnt_m = reinterpret_cast<int *>(take((size_t)N * 4));
    w.bytes = off;
    return w;
}

}  // namespace tp3d

using namespace tp3d;

TP3D_EXPORT size_t tp3d_region_grow_workspace_bytes(int64_t N)
{
    if (N <= 0 || N >= 0x7fffffff) return 0;
    return carve_region_grow_workspace(nullptr, N).bytes;
}

TP3D_EXPORT int tp3d_region_grow_f32(const float *pos, const int64_t *labels, const int64_t *batch, int64_t N,
                                     const int64_t *ignore, int n_ignore, float radius, int64_t min_cluster_size,
                                     int64_t *members, int64_t *member_cluster, int64_t *starts, int64_t *cluster_label,
                                     int64_t *cluster_cloud, int32_t *stats, void *workspace, size_t workspace_bytes,
                                     void *stream)
{
    if (N <= 0 || N >= 0x7fffffff || !(radius > 0.0f) || n_ignore < 0 || (n_ignore > 0 && !ignore) || !pos || !labels ||
        !batch || !members || !member_cluster || !starts || !cluster_label || !cluster_cloud || !stats || !workspace)
        return TP3D_E_BADARG;
    const RegionGrowWorkspace w = carve_region_grow_workspace(workspace, N);
    if (workspace_bytes < w.bytes) return TP3D_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    const float inv_cell = 1.0f / (radius * 1.01f);
    const float r2 = radius * radius;  // as tp3d_ball_query_partial_dense_f32 forms it
    const unsigned blocks = (unsigned)((N + RG_BLOCK - 1) / RG_BLOCK);
    if (int rc = zero_async(stats, 8 * sizeof(int32_t), s)) return rc;
    hipLaunchKernelGGL(box_init_kernel, dim3(1), dim3(64), 0, s, w.bounds, 16);
    hipLaunchKernelGGL(rg_bounds_kernel, dim3(blocks > 2048 ? 2048 : blocks), dim3(RG_BLOCK), 0, s, pos, labels, batch, N,
                       ignore, n_ignore, inv_cell, w.bounds);
    hipLaunchKernelGGL(rg_key_kernel, dim3(blocks), dim3(RG_BLOCK), 0, s, pos, labels, batch, N, ignore, n_ignore, inv_cell,
                       w.bounds, w.sort.keys_in, w.sort.vals_in, w.parent, stats);
    if (int rc = check_launch()) return rc;
    if (int rc = sort_pairs_u64_u32(w.sort.tmp, w.sort.tmp_bytes, w.sort.keys_in, w.sort.keys_out, w.sort.vals_in,
                                    w.sort.vals_out, N, 64u, s))
        return rc;
    hipLaunchKernelGGL(rg_fill_kernel, dim3(blocks), dim3(RG_BLOCK), 0, s, pos, w.sort.vals_out, N, w.sorted_pt);
    const int64_t hook_blocks = (N + RG_BLOCK / 64 - 1) / (RG_BLOCK / 64);
    hipLaunchKernelGGL(rg_hook_kernel, dim3((unsigned)hook_blocks), dim3(RG_BLOCK), 0, s, w.sort.keys_out, w.sorted_pt, (int)N,
                       r2, w.parent, stats);
    hipLaunchKernelGGL(rg_flatten_kernel, dim3(blocks), dim3(RG_BLOCK), 0, s, w.parent, labels, N, w.sort.keys_in,
                       w.sort.vals_in);
    if (int rc = check_launch()) return rc;
    if (int rc = sort_pairs_u64_u32(w.sort.tmp, w.sort.tmp_bytes, w.sort.keys_in, w.sort.keys_out, w.sort.vals_in,
                                    w.sort.vals_out, N, (unsigned)(RG_ROOT_BITS + 13), s))
        return rc;
    if (int rc = run_ids(w.sort.keys_out, N, w.sort, s)) return rc;
    hipLaunchKernelGGL(rg_runs_kernel, dim3(blocks), dim3(RG_BLOCK), 0, s, w.sort.cid, N, w.run_start, w.meta);
    hipLaunchKernelGGL(rg_scan_kernel, dim3(1), dim3(RG_SCAN_BLOCK), 0, s, w.sort.keys_out, w.run_start, w.meta, batch,
                       min_cluster_size, w.cnt_k, w.cnt_m, w.newid, w.outstart, starts, cluster_label, cluster_cloud, stats);
    hipLaunchKernelGGL(rg_members_kernel, dim3(blocks), dim3(RG_BLOCK), 0, s, w.sort.vals_out, w.sort.cid, w.run_start,
                       w.newid, w.outstart, N, members, member_cluster);
    return check_launch();
}
