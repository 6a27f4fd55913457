// Shared device/host helpers for libtp3d_hip.so (gfx950 only, wave = 64 lanes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tp3d_hip.h"

#define TP3D_EXPORT extern "C" __attribute__((visibility("default")))

namespace tp3d {

constexpr int kWave = 64;

void set_last_hip_error(hipError_t e);

// HIP status -> library status; a failure is kept for tp3d_last_error.
inline int hip_rc(hipError_t e)
{
    if (e == hipSuccess) return TP3D_OK;
    set_last_hip_error(e);
    return TP3D_E_LAUNCH;
}

// Checks the launch that was just enqueued; called by every entry point.
inline int check_launch() { return hip_rc(hipGetLastError()); }

// Kernels that need more than 64 KiB of dynamic LDS must opt in once per (function, device).
inline void allow_large_dynamic_lds(const void *func, int bytes, bool *done_per_device /*[64]*/)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    if (!done_per_device[dev]) {
        (void)hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        done_per_device[dev] = true;
    }
}
// The usual form, allow_large_dynamic_lds<&kernel>(bytes): the kernel is a template argument, so every kernel gets its
// own per-device `done` array (a function argument would share one array among all kernels of one signature).
template <auto kernel>
inline void allow_large_dynamic_lds(int bytes)
{
    static bool done[64] = {false};
    allow_large_dynamic_lds(reinterpret_cast<const void *>(kernel), bytes, done);
}

// v rounded up to a multiple of a (a power of two): workspace and LDS carves
constexpr size_t align_up(size_t v, size_t a) { return (v + a - 1) & ~(a - 1); }

// Zero-fills a device buffer on the stream (used by the scatter-add backward entry points).
inline int zero_async(void *ptr, size_t bytes, hipStream_t s)
{
    return bytes == 0 ? TP3D_OK : hip_rc(hipMemsetAsync(ptr, 0, bytes, s));
}

// Squared distance in the one evaluation order shared with oracle/tpk_ref_cpu.c.
// The translation units are built with -ffp-contract=off: no v_fma may be formed here.
__device__ __forceinline__ float sqdist3(float ax, float ay, float az, float bx, float by, float bz)
{
    float dx = ax - bx;
    float dy = ay - by;
    float dz = az - bz;
    return (dx * dx + dy * dy) + dz * dz;
}

// gemm_tn.hip: out[e] = sum over the row splits of partial[s][e], in ascending split order (reproducible)
// dbeta, dgamma (, c1, c2) from chunk partials [chunks][2][C] (rows.hip)
int bn_bwd_finalize_launch(const float *partial, int chunks, int C, float *dbeta, float *dgamma, const float *invstd, int64_t M,
                           int training, float *c1, float *c2, hipStream_t s);
int tn_reduce_splits(const float *partial, int splits, int64_t NK, float *out, hipStream_t s);

__device__ __forceinline__ int lane_id() { return threadIdx.x & (kWave - 1); }

// number of set bits of `mask` strictly below this lane
__device__ __forceinline__ int lanes_below(unsigned long long mask)
{
    return __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0));
}

// inclusive scan of v over the 64 lanes of the wave (Hillis-Steele on the cross-lane network, six steps)
template <typename T>
__device__ __forceinline__ T wave_inclusive_scan(T v)
{
    const int lane = lane_id();
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const T o = __shfl_up(v, off);
        if (lane >= off) v += o;
    }
    return v;
}

}  // namespace tp3d
