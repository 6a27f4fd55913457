// The rocPRIM side of sorted_keys.h: the radix sort, the scan behind the run ids and the scratch they need.
#include <cstring>  // rocPRIM's texture iterator calls memset unqualified

#include <rocprim/rocprim.hpp>

#include "sorted_keys.h"

namespace tp3d {

size_t sort_pairs_tmp_bytes(int64_t n)
{
    size_t bytes = 0;
    (void)rocprim::radix_sort_pairs(nullptr, bytes, (const unsigned long long *)nullptr, (unsigned long long *)nullptr,
                                    (const unsigned int *)nullptr, (unsigned int *)nullptr, (size_t)n, 0u, 64u,
                                    (hipStream_t)0);
    return bytes;
}

int sort_pairs_u64_u32(void *tmp, size_t tmp_bytes, const unsigned long long *keys_in, unsigned long long *keys_out,
                       const unsigned int *vals_in, unsigned int *vals_out, int64_t n, unsigned bits, hipStream_t s)
{
    size_t tb = tmp_bytes;
    return hip_rc(rocprim::radix_sort_pairs(tmp, tb, keys_in, keys_out, vals_in, vals_out, (size_t)n, 0u, bits, s));
}

unsigned sort_bits(unsigned __int128 total)
{
    unsigned bits = 1;
    while (bits < 63 && ((unsigned __int128)1 << bits) < total) ++bits;
    return bits;
}

SortWorkspace carve_sort_workspace(void *ws, int64_t n, bool with_vals_out, bool with_run_ids)
{
    auto up = [](size_t v) { return align_up(v, 256); };
    char *p = static_cast<char *>(ws);
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char *at = p + off;
        off += up(bytes);
        return at;
    };
    SortWorkspace w;
    w.keys_in = reinterpret_cast<unsigned long long *>(take((size_t)n * 8));
    w.keys_out = reinterpret_cast<unsigned long long *>(take((size_t)n * 8));
    w.vals_in = reinterpret_cast<unsigned int *>(take((size_t)n * 4));
    w.vals_out = with_vals_out ? reinterpret_cast<unsigned int *>(take((size_t)n * 4)) : nullptr;
    w.flags = with_run_ids ? reinterpret_cast<int *>(take((size_t)n * 4)) : nullptr;
    w.cid = with_run_ids ? reinterpret_cast<int *>(take((size_t)n * 4)) : nullptr;
    w.tmp_bytes = sort_pairs_tmp_bytes(n);
    if (with_run_ids) {
        size_t scan_bytes = 0;
        (void)rocprim::inclusive_scan(nullptr, scan_bytes, (const int *)nullptr, (int *)nullptr, (size_t)n,
                                      rocprim::plus<int>(), (hipStream_t)0);
        if (scan_bytes > w.tmp_bytes) w.tmp_bytes = scan_bytes;
    }
    w.tmp = take(w.tmp_bytes + 256);
    w.bytes = off;
    return w;
}

__global__ __launch_bounds__(SK_BLOCK) void run_flag_kernel(const unsigned long long *__restrict__ keys, int64_t n,
                                                             int *__restrict__ flags)
{
    const int64_t i = (int64_t)blockIdx.x * SK_BLOCK + threadIdx.x;
    if (i >= n) return;
    flags[i] = (i > 0 && keys[i] != keys[i - 1]) ? 1 : 0;
}

int run_ids(const unsigned long long *sorted_keys, int64_t n, const SortWorkspace &w, hipStream_t s)
{
    hipLaunchKernelGGL(run_flag_kernel, dim3((unsigned)((n + SK_BLOCK - 1) / SK_BLOCK)), dim3(SK_BLOCK), 0, s, sorted_keys, n,
                       w.flags);
    if (int rc = check_launch()) return rc;
    size_t tb = w.tmp_bytes;
    return hip_rc(rocprim::inclusive_scan(w.tmp, tb, (const int *)w.flags, w.cid, (size_t)n, rocprim::plus<int>(), s));
}

}  // namespace tp3d
