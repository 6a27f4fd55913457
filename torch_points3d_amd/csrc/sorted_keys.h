// What the sorted-key features share (voxel.hip: GridSampling3D clusters, sparseconv.hip: coordinate sets,
// pointvoxel.hip: table inversion, grid.hip: the sort-based grid build): 64-bit keys -> stable radix sort of
// (key, slot) -> boundary flags + inclusive scan -> consecutive run ids -> binary search in the sorted keys, with the
// scratch layout around it and the integer bounding-box reduction the key kernels start from.  sorted_keys.hip is the
// library's only user of rocPRIM.  Device functions are __forceinline__: every kernel keeps its own instruction stream.
#pragma once
#include "tp3d_common.h"

namespace tp3d {

constexpr int SK_BLOCK = 256;  // block size of the flag pass and of every kernel that calls box8_reduce_to

// The library's one radix-sort instantiation (u64 keys, u32 values, stable, over the low `bits` bits of the key).
size_t sort_pairs_tmp_bytes(int64_t n);
int sort_pairs_u64_u32(void *tmp, size_t tmp_bytes, const unsigned long long *keys_in, unsigned long long *keys_out,
                       const unsigned int *vals_in, unsigned int *vals_out, int64_t n, unsigned bits, hipStream_t s);

// bits the sort must cover for `total` distinct keys 0 .. total - 1: the least bits >= 1 with 2^bits >= total, at most 63
unsigned sort_bits(unsigned __int128 total);

// keys_in | keys_out | vals_in | [vals_out] | [flags | cid] | tmp, each rounded up to 256 bytes.  tmp holds the sort's
// scratch, or the larger of the sort's and the scan's when the run ids are wanted.
struct SortWorkspace {
    unsigned long long *keys_in, *keys_out;
    unsigned int *vals_in, *vals_out;  // vals_out null: the caller sorts the values into a buffer of its own
    int *flags, *cid;                  // null without run ids
    void *tmp;
    size_t tmp_bytes, bytes;
};
SortWorkspace carve_sort_workspace(void *ws, int64_t n, bool with_vals_out, bool with_run_ids);

// w.cid[i] = number of distinct keys in front of the run of sorted slot i (boundary flags + inclusive scan)
int run_ids(const unsigned long long *sorted_keys, int64_t n, const SortWorkspace &w, hipStream_t s);

// first slot with keys[slot] >= key (n when there is none)
__device__ __forceinline__ int64_t lower_bound_u64(const unsigned long long *__restrict__ keys, int64_t n,
                                                   unsigned long long key)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// p = [INT_MAX x3 | INT_MIN x4 | 0 ...]: the neutral elements of box8_reduce_to, zeros behind them (n <= 64, one block)
static __global__ void box_init_kernel(int *p, int n)
{
    const int t = threadIdx.x;
    if (t < n) p[t] = t < 3 ? 0x7fffffff : (t < 7 ? (int)0x80000000 : 0);
}

// v = [min x,y,z | max x,y,z | max batch | flag bits] of this thread -> out[0..7] over the whole grid: wave shuffles,
// one LDS round over the SK_BLOCK / 64 waves, then atomicMin (0-2), atomicMax (3-6), atomicOr (7).  Every thread of an
// SK_BLOCK-thread block calls it once.
__device__ __forceinline__ void box8_reduce_to(int v[8], int *__restrict__ out)
{
    __shared__ int s_red[8][SK_BLOCK / 64];
    auto combine = [](int k, int a, int b) { return k < 3 ? min(a, b) : (k < 7 ? max(a, b) : (a | b)); };
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v[k] = combine(k, v[k], __shfl_xor(v[k], off));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < 8; ++k) s_red[k][wave] = v[k];
    __syncthreads();
    if (threadIdx.x < 8) {
        const int k = threadIdx.x;
        int r = s_red[k][0];
        for (int w = 1; w < SK_BLOCK / 64; ++w) r = combine(k, r, s_red[k][w]);
        if (k < 3) atomicMin(&out[k], r);
        else if (k < 7) atomicMax(&out[k], r);
        else atomicOr(&out[k], r);
    }
}

}  // namespace tp3d
