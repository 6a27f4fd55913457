// What the message-passing kernels share (pointconv.hip: PointConv and the segmented max, rsconv_mp.hip: RSConv): the
// launch shape and the device code of "a wave owns one run of a CSR edge list, or one piece of it, and its lanes walk
// the run's row-major elements".  A run is clamped to [0, E): no index derived from it leaves the (E, ld) matrices.
// Device functions are __forceinline__: every kernel keeps its own instruction stream.
#pragma once
#include "tp3d_common.h"

namespace tp3d {

constexpr int ER_BLOCK = 256;  // 4 waves, one query / segment (piece) each
constexpr int ER_WAVES = ER_BLOCK / kWave;

static inline bool grid_ok(int64_t waves) { return (waves + ER_WAVES - 1) / ER_WAVES <= INT32_MAX; }
static inline dim3 grid_of(int64_t waves) { return dim3((unsigned)((waves + ER_WAVES - 1) / ER_WAVES)); }

// pieces per run of the element-walking kernels: about 64 rows per wave, from the MEAN run length (the per-query runs
// of a capped finder: one piece; a cloud of the global pool: many)
static inline int64_t run_parts(int64_t S, int64_t E)
{
    const int64_t parts = (E / S + 63) / 64;
    return parts < 1 ? 1 : (parts > 1024 ? 1024 : parts);
}

// wave -> (item, sub) for count * per waves (per >= 1), sub the fast index; false past the end, and the caller
// returns.  The test is wave-uniform: callers that shuffle see whole waves.  It comes last so that the kernel keeps
// ONE branch for it (as an early return here it costs rsconv_msgmax_fwd_kernel a second one and 8 SGPRs).
__device__ __forceinline__ bool wave_item(int64_t count, int per, int64_t &item, int &sub)
{
    const int64_t w = (int64_t)blockIdx.x * ER_WAVES + threadIdx.x / kWave;
    item = w / per;
    sub = (int)(w - item * per);
    return w < count * per;
}

// the run [r0, r1) of item s (empty: r0 >= r1)
__device__ __forceinline__ void run_bounds(const int64_t *__restrict__ edge_start, int64_t s, int64_t E, int64_t &r0,
                                           int64_t &r1)
{
    r0 = edge_start[s];
    r1 = edge_start[s + 1];
    if (r0 < 0) r0 = 0;
    if (r1 > E) r1 = E;
}

// the piece [a, b) of the run of item s that wave `part` of `parts` owns (empty: a >= b)
__device__ __forceinline__ void run_piece(const int64_t *__restrict__ edge_start, int64_t s, int64_t E, int part,
                                          int parts, int64_t &a, int64_t &b)
{
    int64_t r0, r1;
    run_bounds(edge_start, s, E, r0, r1);
    a = b = 0;
    if (r0 >= r1) return;
    const int64_t per = (r1 - r0 + parts - 1) / parts;
    a = r0 + part * per;
    b = a + per < r1 ? a + per : r1;
}

// the lanes of a wave over the (b - a) * ld floats of the rows [a, b) of an (E, ld) matrix, 64 consecutive floats per
// step: value(row, column, offset of the element in the matrix)
template <class F>
__device__ __forceinline__ void walk_rows(int64_t a, int64_t b, int ld, F &&value)
{
    const int64_t n = (b - a) * ld;
    for (int64_t f = lane_id(); f < n; f += kWave) {
        const int64_t r = f / ld;
        value(a + r, (int)(f - r * ld), a * ld + f);
    }
}

// coordinate k of a point held in registers.  The values are passed, not selected in place: a conditional between
// the captures of a walker's lambda is a conditional between addresses, and keeps the closure in memory.
__device__ __forceinline__ float pick3(int k, float x, float y, float z) { return k == 0 ? x : (k == 1 ? y : z); }

}  // namespace tp3d
