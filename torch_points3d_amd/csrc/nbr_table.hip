// Inverse of a neighbour table and what runs through it (no kernel points here): for every support point the slots
// (q, n) that reference it, in ascending slot order, so that a backward pass sums per point instead of scattering.  No
// float atomics: a global counting sort over the Nq*Mn slots (integer histogram -> scan -> fill -> per-point sort of
// its short run, which makes the summation order ascending in (q, n) whatever the timing).  Used by the KPConv
// backward passes (kpconv.hip, kpconv_deform.hip), the neighbour max-pool below and the flat scatter of rows.hip.
#include <algorithm>

#include "tp3d_common.h"

namespace tp3d {

constexpr int NBR_BLOCK = 256;  // 4 waves, one support point per wave in the gather kernels

// bin of slot s: the table entry itself, or -- for a batch of per-cloud tables flattened into one -- the entry clamped
// to its cloud's bins plus the cloud's offset
__device__ __forceinline__ int64_t slot_bin(const int64_t *__restrict__ nbr, int64_t s, int64_t L, int64_t nbins)
{
    const int64_t m = nbr[s];
    return L > 0 ? min(max(m, (int64_t)0), nbins - 1) + (s / L) * nbins : m;
}

__global__ void nbr_hist_kernel(const int64_t *__restrict__ nbr, int64_t slots, int64_t M, int *__restrict__ cnt,
                                int64_t L, int64_t nbins)
{
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < slots; s += (int64_t)gridDim.x * blockDim.x) {
        const int64_t m = slot_bin(nbr, s, L, nbins);
        if (m >= 0 && m < M) atomicAdd(&cnt[m], 1);
    }
}

// exclusive scan of cnt[0..M) into start[0..M] (one workgroup), cursor := start
__global__ __launch_bounds__(1024) void nbr_scan_kernel(const int *__restrict__ cnt, int64_t M, int *__restrict__ start,
                                                         int *__restrict__ cursor)
{
    __shared__ int s_w[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t per = (M + 1023) / 1024;
    const int64_t k0 = min((int64_t)tid * per, M), k1 = min(k0 + per, M);
    int sum = 0;
    for (int64_t k = k0; k < k1; ++k) sum += cnt[k];
    int incl = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int v = __shfl_up(incl, off);
        if (lane >= off) incl += v;
    }
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int w = 0; w < 16; ++w) {
            const int v = s_w[w];
            s_w[w] = run;
            run += v;
        }
    }
    __syncthreads();
    int run = s_w[wave] + incl - sum;
    for (int64_t k = k0; k < k1; ++k) {
        const int v = cnt[k];
        start[k] = run;
        cursor[k] = run;
        run += v;
    }
    if (k1 == M) start[M] = run;  // every thread whose range ends at M holds the grand total
}

__global__ void nbr_fill_kernel(const int64_t *__restrict__ nbr, int64_t slots, int64_t M, int *__restrict__ cursor,
                                int *__restrict__ order, int64_t L, int64_t nbins)
{
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < slots; s += (int64_t)gridDim.x * blockDim.x) {
        const int64_t m = slot_bin(nbr, s, L, nbins);
        if (m >= 0 && m < M) order[atomicAdd(&cursor[m], 1)] = (int)s;
    }
}

// canonical order inside every bin (ascending slot id): one lane per bin for bins of up to NBR_SMALL_BIN slots
// (insertion sort; the fill leaves them nearly sorted), a whole wave's bitonic network for larger ones -- a point that
// hundreds of slots reference (padded tails of dense ball queries) would otherwise be hundreds of dependent global
// round trips in one thread
constexpr int NBR_SMALL_BIN = 24;
// A bin of more than 1024 slots, sorted by one wave: 1024-slot runs through the bitonic network, then log2(runs) merge
// passes between `order` and `tmp` -- every lane merges an equal share of a run pair, its split found by bisection
// (merge path).  Slot ids are unique, so the result is the ascending order whatever the arrival order was.
// (one thread's insertion sort needed tens of seconds for a 52 800-slot bin)
__device__ void wave_merge_sort_bin(int *order, int *tmp, int n, int lane)
{
    for (int a = 0; a < n; a += 1024) wave_sort_bin<16>(order + a, min(1024, n - a), lane);
    int *src = order, *dst = tmp;
    for (int width = 1024; width < n; width <<= 1) {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        __builtin_amdgcn_wave_barrier();
        for (int lo = 0; lo < n; lo += 2 * width) {
            const int mid = min(lo + width, n), hi = min(lo + 2 * width, n);
            const int *A = src + lo, *B = src + mid;
            const int na = mid - lo, nb = hi - mid, total = hi - lo;
            const int per = (total + 63) / 64;
            const int o0 = min(lane * per, total), o1 = min(o0 + per, total);
            // i = how many of the first o0 outputs come from A: smallest i with A[i] > B[o0 - i - 1]
            int x = max(0, o0 - nb), y = min(o0, na);
            while (x < y) {
                const int i = (x + y) >> 1, j = o0 - i;
                if (j > 0 && A[i] < B[j - 1]) x = i + 1;
                else y = i;
            }
            int i = x, j = o0 - x;
            for (int o = o0; o < o1; ++o) {
                const bool from_a = j >= nb || (i < na && A[i] < B[j]);
                dst[lo + o] = from_a ? A[i++] : B[j++];
            }
        }
        int *t = src;
        src = dst;
        dst = t;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
    if (src != order)
        for (int e = lane; e < n; e += 64) order[e] = src[e];
}

__global__ __launch_bounds__(256) void nbr_sort_kernel(const int *__restrict__ start, int64_t M, int *order, int *tmp)
{
    const int lane = threadIdx.x & 63;
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int s0 = 0, s1 = 0;
    if (m < M) {
        s0 = start[m];
        s1 = start[m + 1];
    }
    const int n = s1 - s0;
    if (n <= NBR_SMALL_BIN || (n > 1024 && !tmp)) {
        for (int a = s0 + 1; a < s1; ++a) {
            const int v = order[a];
            int p = a;
            while (p > s0 && order[p - 1] > v) {
                order[p] = order[p - 1];
                --p;
            }
            order[p] = v;
        }
    }
    unsigned long long big = __ballot(n > NBR_SMALL_BIN && n <= 1024);
    while (big) {  // wave-uniform
        const int l = __builtin_ctzll(big);
        big &= big - 1;
        const int blo = __builtin_amdgcn_readlane(s0, l), bn = __builtin_amdgcn_readlane(n, l);
        if (bn <= 64) wave_sort_bin<1>(order + blo, bn, lane);
        else if (bn <= 128) wave_sort_bin<2>(order + blo, bn, lane);
        else if (bn <= 256) wave_sort_bin<4>(order + blo, bn, lane);
        else if (bn <= 512) wave_sort_bin<8>(order + blo, bn, lane);
        else wave_sort_bin<16>(order + blo, bn, lane);
    }
    if (tmp) {
        unsigned long long giant = __ballot(n > 1024);
        while (giant) {  // wave-uniform
            const int l = __builtin_ctzll(giant);
            giant &= giant - 1;
            const int blo = __builtin_amdgcn_readlane(s0, l), bn = __builtin_amdgcn_readlane(n, l);
            wave_merge_sort_bin(order + blo, tmp + blo, bn, lane);
        }
    }
}

// Inverse of an index table over any number of workgroups: for every bin m the slots that reference it, ascending
// (integer histogram -> scan -> fill -> per-bin insertion sort of its short run).  Entries outside [0, M) are skipped.
// cnt, cursor: M ints; start: M + 1 ints; order: `slots` ints.
int invert_table(const int64_t *idx, int64_t slots, int64_t M, int *cnt, int *start, int *cursor, int *order,
                 hipStream_t s, int64_t per_cloud_slots, int64_t per_cloud_bins, int *merge_tmp)
{
    if (int rc = zero_async(cnt, (size_t)M * 4, s)) return rc;
    const unsigned gs = (unsigned)std::min<int64_t>((slots + 255) / 256, 4096);
    hipLaunchKernelGGL(nbr_hist_kernel, dim3(gs), dim3(256), 0, s, idx, slots, M, cnt, per_cloud_slots, per_cloud_bins);
    hipLaunchKernelGGL(nbr_scan_kernel, dim3(1), dim3(1024), 0, s, cnt, M, start, cursor);
    hipLaunchKernelGGL(nbr_fill_kernel, dim3(gs), dim3(256), 0, s, idx, slots, M, cursor, order, per_cloud_slots,
                       per_cloud_bins);
    hipLaunchKernelGGL(nbr_sort_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, start, M, order, merge_tmp);
    return check_launch();
}

// workspace: tp3d_kpconv_bwd_workspace_bytes(M, slots)
int invert_neighbors(const int64_t *neighbors, int64_t slots, int64_t M, void *workspace, int **start_out,
                     int **order_out, hipStream_t s, bool ready)
{
    auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
    char *p = static_cast<char *>(workspace);
    int *cnt = reinterpret_cast<int *>(p);
    int *start = reinterpret_cast<int *>(p + up((size_t)M * 4));
    int *cursor = reinterpret_cast<int *>(p + up((size_t)M * 4) + up((size_t)(M + 1) * 4));
    int *order = reinterpret_cast<int *>(p + up((size_t)M * 4) + up((size_t)(M + 1) * 4) + up((size_t)M * 4));
    // second buffer of the run merge that sorts a bin of more than 1024 slots (a hub support point: many queries padding
    // onto one index, duplicated points); without it such a bin fell back to one lane's insertion sort -- tens of seconds
    int *merge_tmp = reinterpret_cast<int *>(p + up((size_t)M * 4) + up((size_t)(M + 1) * 4) + up((size_t)M * 4) +
                                             up((size_t)slots * 4));
    *start_out = start;
    *order_out = order;
    if (ready) return TP3D_OK;  // the caller kept the table of an earlier call on the same neighbours
    return invert_table(neighbors, slots, M, cnt, start, cursor, order, s, 0, 0, merge_tmp);
}

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

// d_x[m, :] = sum of the per-slot gradient rows g[q, n, :] that reference m, ascending slot (one wave per support point;
// second step of the rigid and the deformable KPConv backward)
__global__ __launch_bounds__(NBR_BLOCK) void kpconv_bwd_gather_kernel(const float *__restrict__ g,
                                                                      const int *__restrict__ start,
                                                                      const int *__restrict__ order, int64_t M, int Cin,
                                                                      float *__restrict__ d_x)
{
    const int lane = threadIdx.x & 63;
    const int64_t m = (int64_t)blockIdx.x * (NBR_BLOCK / 64) + (threadIdx.x >> 6);
    if (m >= M) return;  // wave-uniform; no workgroup barrier in this kernel
    const int s0 = start[m], s1 = start[m + 1];
    for (int c0 = 0; c0 < Cin; c0 += 64) {
        const int c = min(c0 + lane, Cin - 1);
        float acc = 0.0f;
        // the run's slot ids are fetched 64 at a time with one coalesced load and handed out by v_readlane, so the row
        // reads (four in flight) no longer wait for a dependent index load each; summed in slot order
        for (int j0 = s0; j0 < s1; j0 += 64) {
            const int cnt = min(64, s1 - j0);
            const int mine = lane < cnt ? order[j0 + lane] : 0;
            int t = 0;
            for (; t + 4 <= cnt; t += 4) {
                const int r0 = __builtin_amdgcn_readlane(mine, t), r1 = __builtin_amdgcn_readlane(mine, t + 1);
                const int r2 = __builtin_amdgcn_readlane(mine, t + 2), r3 = __builtin_amdgcn_readlane(mine, t + 3);
                const float v0 = g[(size_t)r0 * Cin + c], v1 = g[(size_t)r1 * Cin + c];
                const float v2 = g[(size_t)r2 * Cin + c], v3 = g[(size_t)r3 * Cin + c];
                acc = (((acc + v0) + v1) + v2) + v3;
            }
            for (; t < cnt; ++t) acc += g[(size_t)__builtin_amdgcn_readlane(mine, t) * Cin + c];
        }
        if (c0 + lane < Cin) d_x[(size_t)m * Cin + c0 + lane] = acc;
    }
}

// d_x[m, :] = sum of the per-slot rows g that reference m
int gather_slot_rows(const float *g, const int *start, const int *order, int64_t M, int Cin, float *d_x, hipStream_t s)
{
    hipLaunchKernelGGL(kpconv_bwd_gather_kernel, dim3((unsigned)((M + NBR_BLOCK / 64 - 1) / (NBR_BLOCK / 64))),
                       dim3(NBR_BLOCK), 0, s, g, start, order, M, Cin, d_x);
    return check_launch();
}

}  // namespace tp3d

TP3D_EXPORT size_t tp3d_kpconv_bwd_workspace_bytes(int64_t M, int64_t slots)
{
    if (M < 0 || slots < 0) return 0;
    auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
    return up((size_t)M * 4) + up((size_t)(M + 1) * 4) + up((size_t)M * 4) + 2 * up((size_t)slots * 4);  // + merge buffer
}

TP3D_EXPORT size_t tp3d_kpconv_grad_workspace_bytes(int64_t M, int64_t slots, int Cin)
{
    if (M < 0 || slots < 0 || Cin <= 0) return 0;
    return ((size_t)slots * Cin * 4 + 15) & ~(size_t)15;  // the per-slot gradient rows
}

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
