// Batch building on the device (include/tp3d_hip.h, "Data transforms"): the region cut that replaces the reference's
// KDTree.query_radius / ball_query / crop masks, the mask compaction behind apply_mask, and ElasticDistortion's blur and
// trilinear warp.  Integer counters and plain stores only, no float atomics: repeats are bit-equal.
//
// Region cut = count (per tile, per region) -> one block scan (block_scan_chunk of inverse_table.h) -> emit (ballot +
// prefix inside the tile, so rows come out ascending).  Both passes evaluate the same predicate in double from the fp32
// inputs, differences first, then products, summed left to right; -ffp-contract=off keeps v_fma out of it, so a numpy
// float64 restatement is bit-equal.
#include "inverse_table.h"
#include "sorted_keys.h"

namespace tp3d {

constexpr int RC_BLOCK = 256;                // threads of the count and emit kernels
constexpr int RC_SUB = 4;                    // rows per thread: sub-chunk j holds rows tile * RC_TILE + j * RC_BLOCK + tid
constexpr int RC_TILE = RC_BLOCK * RC_SUB;   // rows per tile
constexpr int RC_WAVES = RC_BLOCK / kWave;
constexpr int RC_SCAN_BLOCK = 1024;

enum { RC_SPHERE = 0, RC_CYLINDER = 1, RC_BOX = 2, RC_ELLIPSOID = 3, RC_MASK = 4 };
enum { RC_EACH = 0, RC_KEEP = 1 };
enum { RC_CLOSED = 1, RC_SKIP_ZERO = 2, RC_ALIGN = 4 };

struct RegionArgs {
    const float *pos;
    int64_t N;
    const int64_t *seg;
    int64_t S;
    int kind, mode, flags;
    const float *centre, *param, *rot;
    const int64_t *scene;
    const uint8_t *mask;
    int64_t B, tiles;
};

// the rows [lo, hi) region b may hold: its scene's, or all of them; a scene outside [0, S) holds none
__device__ __forceinline__ void region_rows(const RegionArgs &a, int64_t b, int64_t &lo, int64_t &hi)
{
    lo = 0;
    hi = a.N;
    if (a.scene) {
        const int64_t s = a.scene[b];
        if (s < 0 || s >= a.S) {
            hi = 0;
            return;
        }
        lo = min(max(a.seg[s], (int64_t)0), a.N);
        hi = min(max(a.seg[s + 1], lo), a.N);
    }
}

// Is the point inside region b?  double throughout, one rounding per operation.
__device__ __forceinline__ bool region_holds(const RegionArgs &a, int64_t b, float px, float py, float pz)
{
    const float *c = a.centre + 3 * b, *p = a.param + 3 * b;
    const double dx = (double)px - (double)c[0];
    const double dy = (double)py - (double)c[1];
    const double dz = (double)pz - (double)c[2];
    const bool closed = a.flags & RC_CLOSED;
    const double planar = dx * dx + dy * dy;
    const double d2 = a.kind == RC_CYLINDER ? planar : planar + dz * dz;
    if ((a.flags & RC_SKIP_ZERO) && d2 == 0.0) return false;
    if (a.kind == RC_SPHERE || a.kind == RC_CYLINDER) {
        const double r2 = (double)p[0] * (double)p[0];
        return closed ? d2 <= r2 : d2 < r2;
    }
    double qx = dx, qy = dy, qz = dz;
    if (a.rot) {
        const float *R = a.rot + 9 * b;
        qx = ((double)R[0] * dx + (double)R[1] * dy) + (double)R[2] * dz;
        qy = ((double)R[3] * dx + (double)R[4] * dy) + (double)R[5] * dz;
        qz = ((double)R[6] * dx + (double)R[7] * dy) + (double)R[8] * dz;
    }
    const double h0 = (double)p[0], h1 = (double)p[1], h2 = (double)p[2];
    if (a.kind == RC_BOX) {
        return closed ? (fabs(qx) <= h0 && fabs(qy) <= h1 && fabs(qz) <= h2)
                      : (fabs(qx) < h0 && fabs(qy) < h1 && fabs(qz) < h2);
    }
    const double v = ((qx * qx) / (h0 * h0) + (qy * qy) / (h1 * h1)) + (qz * qz) / (h2 * h2);
    return closed ? v <= 1.0 : v < 1.0;
}

// Does `row` belong to the list the block writes?  each: inside region b (lo, hi: its rows).  keep: a non-zero mask
// byte, or inside none of the regions whose rows it is one of.
__device__ __forceinline__ bool row_selected(const RegionArgs &a, int64_t b, int64_t lo, int64_t hi, int64_t row)
{
    if (row >= a.N) return false;
    if (a.kind == RC_MASK) return a.mask[row] != 0;
    const float px = a.pos[3 * row], py = a.pos[3 * row + 1], pz = a.pos[3 * row + 2];
    if (a.mode == RC_EACH) return row >= lo && row < hi && region_holds(a, b, px, py, pz);
    for (int64_t r = 0; r < a.B; ++r) {
        int64_t rlo, rhi;
        region_rows(a, r, rlo, rhi);
        if (row >= rlo && row < rhi && region_holds(a, r, px, py, pz)) return false;
    }
    return true;
}

// block -> (region, tile); false when no row of the tile can be selected (nothing is read then)
__device__ __forceinline__ bool block_tile(const RegionArgs &a, int64_t &b, int64_t &tile, int64_t &lo, int64_t &hi)
{
    const int64_t id = blockIdx.x;
    b = a.mode == RC_EACH ? id / a.tiles : 0;
    tile = a.mode == RC_EACH ? id % a.tiles : id;
    lo = 0;
    hi = a.N;
    if (a.mode == RC_EACH && a.kind != RC_MASK) region_rows(a, b, lo, hi);
    const int64_t r0 = tile * RC_TILE;
    return r0 < hi && r0 + RC_TILE > lo;
}

__global__ __launch_bounds__(RC_BLOCK) void region_count_kernel(RegionArgs a, int *__restrict__ cnt)
{
    __shared__ int s_cnt[RC_WAVES];
    int64_t b, tile, lo, hi;
    if (!block_tile(a, b, tile, lo, hi)) {
        if (threadIdx.x == 0) cnt[blockIdx.x] = 0;
        return;
    }
    int mine = 0;
#pragma unroll
    for (int j = 0; j < RC_SUB; ++j)
        mine += row_selected(a, b, lo, hi, tile * RC_TILE + j * RC_BLOCK + threadIdx.x) ? 1 : 0;
    const int total = wave_inclusive_scan(mine);
    if (lane_id() == kWave - 1) s_cnt[threadIdx.x >> 6] = total;
    __syncthreads();
    if (threadIdx.x == 0) {
        int sum = 0;
#pragma unroll
        for (int w = 0; w < RC_WAVES; ++w) sum += s_cnt[w];
        cnt[blockIdx.x] = sum;
    }
}

// cnt[0 .. n) -> exclusive offsets in place; each: start[b] = the offset of region b's first tile, start[B] = the total;
// keep: start = [0, total].  status[0] = total, status[1] = 1 when it exceeds a given capacity (capacity < 0: none).
__global__ __launch_bounds__(RC_SCAN_BLOCK) void region_scan_kernel(int *__restrict__ cnt, int64_t n, int64_t tiles,
                                                                    int64_t B, int mode, int64_t capacity,
                                                                    int64_t *__restrict__ start,
                                                                    int64_t *__restrict__ status)
{
    __shared__ int s_wave[RC_SCAN_BLOCK / 64];
    int64_t k0, k1;
    int run = block_scan_chunk<RC_SCAN_BLOCK, int64_t>(cnt, n, s_wave, k0, k1);
    for (int64_t k = k0; k < k1; ++k) {
        const int c = cnt[k];
        cnt[k] = run;
        if (mode == RC_EACH && k % tiles == 0) start[k / tiles] = run;
        run += c;
    }
    if (threadIdx.x == RC_SCAN_BLOCK - 1) {  // the last chunk ends at n: run is the total
        if (mode == RC_KEEP) start[0] = 0;
        start[mode == RC_EACH ? B : 1] = run;
        status[0] = run;
        status[1] = (capacity >= 0 && run > capacity) ? 1 : 0;
    }
}

__global__ __launch_bounds__(RC_BLOCK) void region_emit_kernel(RegionArgs a, const int *__restrict__ offset,
                                                               int64_t capacity, int64_t *__restrict__ index,
                                                               int64_t *__restrict__ batch, float *__restrict__ pos_out)
{
    __shared__ int s_cnt[RC_SUB * RC_WAVES];
    int64_t b, tile, lo, hi;
    if (!block_tile(a, b, tile, lo, hi)) return;
    const int wave = threadIdx.x >> 6;
    bool sel[RC_SUB];
    int below[RC_SUB];
#pragma unroll
    for (int j = 0; j < RC_SUB; ++j) {
        sel[j] = row_selected(a, b, lo, hi, tile * RC_TILE + j * RC_BLOCK + threadIdx.x);
        const unsigned long long m = __ballot(sel[j]);
        below[j] = lanes_below(m);
        if (lane_id() == 0) s_cnt[j * RC_WAVES + wave] = __popcll(m);
    }
    __syncthreads();
    const int64_t base = offset[blockIdx.x];
    float cx = 0.f, cy = 0.f, cz = 0.f;
    if (pos_out && (a.flags & RC_ALIGN) && a.mode == RC_EACH && a.kind != RC_MASK) {
        cx = a.centre[3 * b];
        cy = a.centre[3 * b + 1];
        cz = a.kind == RC_CYLINDER ? 0.f : a.centre[3 * b + 2];
    }
    int front = 0;  // selected rows of the tile in the (sub-chunk, wave) pairs before this one
#pragma unroll
    for (int j = 0; j < RC_SUB; ++j) {
#pragma unroll
        for (int w = 0; w < RC_WAVES; ++w) {
            if (w == wave && sel[j]) {
                const int64_t dst = base + front + below[j];
                if (dst < capacity) {  // a total beyond the capacity is reported by status[1]; nothing is written past it
                    const int64_t row = tile * RC_TILE + j * RC_BLOCK + threadIdx.x;
                    index[dst] = row;
                    if (batch) batch[dst] = b;
                    if (pos_out) {
                        pos_out[3 * dst] = a.pos[3 * row] - cx;
                        pos_out[3 * dst + 1] = a.pos[3 * row + 1] - cy;
                        pos_out[3 * dst + 2] = a.pos[3 * row + 2] - cz;
                    }
                }
            }
            front += s_cnt[j * RC_WAVES + w];
        }
    }
}

// keep mode: seg_out[s] = the kept rows below seg[s] (index is ascending); all zero after an overflow
__global__ void region_seg_kernel(const int64_t *__restrict__ index, const int64_t *__restrict__ status, int64_t capacity,
                                  const int64_t *__restrict__ seg, int64_t S, int64_t *__restrict__ seg_out)
{
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s > S) return;
    const int64_t T = status[0];
    if (status[1] != 0 || T > capacity) {
        seg_out[s] = 0;
        return;
    }
    seg_out[s] = lower_bound_u64(reinterpret_cast<const unsigned long long *>(index), T, (unsigned long long)max(seg[s], (int64_t)0));
}

static int region_check(const float *pos, int64_t N, const int64_t *seg, int64_t S, int kind, int mode, const float *centre,
                        const float *param, const int64_t *scene, const uint8_t *mask, int64_t B, int64_t &tiles,
                        int64_t &blocks)
{
    if (N < 0 || S < 0 || B < 0 || kind < RC_SPHERE || kind > RC_MASK || (mode != RC_EACH && mode != RC_KEEP))
        return TP3D_E_BADARG;
    if (kind == RC_MASK) {
        if (mode != RC_KEEP || B != 0 || (N > 0 && !mask)) return TP3D_E_BADARG;
    } else if ((N > 0 && !pos) || (B > 0 && (!centre || !param)) || (scene && !seg)) {
        return TP3D_E_BADARG;
    }
    tiles = (N + RC_TILE - 1) / RC_TILE;
    blocks = mode == RC_EACH ? tiles * B : tiles;
    // the offsets are ints: every list together holds at most N * B rows (each) or N (keep)
    if (N > INT32_MAX || B > INT32_MAX || (mode == RC_EACH ? N * B : N) > INT32_MAX) return TP3D_E_TOOBIG;
    return TP3D_OK;
}

static RegionArgs region_args(const float *pos, int64_t N, const int64_t *seg, int64_t S, int kind, int mode, int flags,
                              const float *centre, const float *param, const float *rot, const int64_t *scene,
                              const uint8_t *mask, int64_t B, int64_t tiles)
{
    RegionArgs a;
    a.pos = pos, a.N = N, a.seg = seg, a.S = S, a.kind = kind, a.mode = mode, a.flags = flags;
    a.centre = centre, a.param = param, a.rot = rot, a.scene = scene, a.mask = mask, a.B = B, a.tiles = tiles;
    return a;
}

// ---------------------------------------------------------------------------------------------------- elastic distortion
constexpr int EL_BLOCK = 256;

// the cloud whose range [off[b], off[b + 1]) holds i (off ascending, off[0] = 0, i < off[B])
__device__ __forceinline__ int64_t range_of(const int64_t *__restrict__ off, int64_t B, int64_t i)
{
    int64_t lo = 0, hi = B;  // the last b with off[b] <= i
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (off[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

// one pass of the 3-tap box blur along `axis` with zero padding: the taps in ascending order, summed in double over the
// fp32 weight 1/3, rounded once to fp32 (scipy.ndimage.convolve on float32 input)
__global__ __launch_bounds__(EL_BLOCK) void elastic_blur_kernel(const float *__restrict__ in, float *__restrict__ out,
                                                                const int *__restrict__ dims,
                                                                const int64_t *__restrict__ goff, int64_t B,
                                                                int64_t total, int axis)
{
    const int64_t i = (int64_t)blockIdx.x * EL_BLOCK + threadIdx.x;
    if (i >= total) return;
    const int64_t b = range_of(goff, B, i);
    const int64_t e = i - goff[b];
    const int64_t d1 = dims[3 * b + 1], d2 = dims[3 * b + 2];
    const int64_t stride = axis == 0 ? d1 * d2 * 3 : (axis == 1 ? d2 * 3 : 3);
    const int64_t len = dims[3 * b + axis];
    const int64_t at = (e / stride) % len;
    const double w = (double)(1.0f / 3.0f);
    double sum = 0.0;
    sum += (at > 0 ? (double)in[i - stride] : 0.0) * w;
    sum += (double)in[i] * w;
    sum += (at + 1 < len ? (double)in[i + stride] : 0.0) * w;
    out[i] = (float)sum;
}

// value i of numpy.linspace(start, stop, n) as numpy forms it: i * step + start, the last one `stop` itself
__device__ __forceinline__ double axis_value(const double *ax, int n, int i) { return i == n - 1 ? ax[2] : (double)i * ax[1] + ax[0]; }

// out = fp32(pos + interp(pos) * magnitude): trilinear in double over the cloud's axes (axes[b][d] = start, step, stop),
// the eight corners in the order and with the weight products of scipy's RegularGridInterpolator; zero outside the axes
__global__ __launch_bounds__(EL_BLOCK) void elastic_apply_kernel(const float *__restrict__ pos, const int64_t *__restrict__ seg,
                                                                 int64_t B, int64_t N, const float *__restrict__ noise,
                                                                 const int *__restrict__ dims,
                                                                 const int64_t *__restrict__ goff,
                                                                 const double *__restrict__ axes, double magnitude,
                                                                 float *__restrict__ out)
{
    const int64_t row = (int64_t)blockIdx.x * EL_BLOCK + threadIdx.x;
    if (row >= N) return;
    const float p[3] = {pos[3 * row], pos[3 * row + 1], pos[3 * row + 2]};
    if (row < seg[0] || row >= seg[B]) {  // a row of no cloud is copied
        for (int d = 0; d < 3; ++d) out[3 * row + d] = p[d];
        return;
    }
    const int64_t b = range_of(seg, B, row);
    int idx[3];
    double y[3];
    bool inside = true;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double *ax = axes + (b * 3 + d) * 3;
        const int n = dims[3 * b + d];
        const double x = (double)p[d];
        if (n < 2 || !(x >= ax[0] && x <= ax[2])) inside = false;
        // the interval with grid[i] <= x < grid[i + 1], the last one closed
        int i = (int)fmax(fmin(floor((x - ax[0]) / ax[1]), (double)(n - 2)), 0.0);
        while (i > 0 && axis_value(ax, n, i) > x) --i;
        while (i < n - 2 && axis_value(ax, n, i + 1) <= x) ++i;
        idx[d] = i;
        const double g0 = axis_value(ax, n, i), g1 = axis_value(ax, n, i + 1);
        y[d] = (x - g0) / (g1 - g0);
    }
    double value[3] = {0.0, 0.0, 0.0};
    if (inside) {
        const int64_t d1 = dims[3 * b + 1], d2 = dims[3 * b + 2];
        const float *g = noise + goff[b];
#pragma unroll
        for (int h = 0; h < 8; ++h) {
            const int hx = h >> 2, hy = (h >> 1) & 1, hz = h & 1;
            double weight = 1.0;
            weight = weight * (hx ? y[0] : 1.0 - y[0]);
            weight = weight * (hy ? y[1] : 1.0 - y[1]);
            weight = weight * (hz ? y[2] : 1.0 - y[2]);
            const int64_t cell = ((int64_t)(idx[0] + hx) * d1 + (idx[1] + hy)) * d2 + (idx[2] + hz);
#pragma unroll
            for (int c = 0; c < 3; ++c) value[c] = value[c] + (double)g[3 * cell + c] * weight;
        }
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) out[3 * row + d] = (float)((double)p[d] + value[d] * magnitude);
}

}  // namespace tp3d

TP3D_EXPORT int tp3d_region_tile_rows(void) { return tp3d::RC_TILE; }

TP3D_EXPORT size_t tp3d_region_workspace_bytes(int64_t N, int64_t B, int mode)
{
    if (N < 0 || B < 0) return 0;
    const int64_t tiles = (N + tp3d::RC_TILE - 1) / tp3d::RC_TILE;
    return tp3d::align_up((size_t)(mode == tp3d::RC_EACH ? tiles * B : tiles) * sizeof(int), 256);
}

TP3D_EXPORT int tp3d_region_count_f32(const float *pos, int64_t N, const int64_t *seg, int64_t S, int kind, int mode, int flags,
                                      const float *centre, const float *param, const float *rot, const int64_t *scene,
                                      const uint8_t *mask, int64_t B, int64_t capacity, int64_t *start, int64_t *status,
                                      void *workspace, size_t workspace_bytes, void *stream)
{
    int64_t tiles, blocks;
    if (int rc = tp3d::region_check(pos, N, seg, S, kind, mode, centre, param, scene, mask, B, tiles, blocks)) return rc;
    if (!start || !status) return TP3D_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    const int64_t nstart = mode == tp3d::RC_EACH ? B + 1 : 2;
    if (blocks == 0) {  // no row or no region: empty lists
        if (int rc = tp3d::zero_async(start, (size_t)nstart * sizeof(int64_t), s)) return rc;
        return tp3d::zero_async(status, 2 * sizeof(int64_t), s);
    }
    if (!workspace || workspace_bytes < tp3d_region_workspace_bytes(N, B, mode)) return TP3D_E_BADARG;
    const tp3d::RegionArgs a = tp3d::region_args(pos, N, seg, S, kind, mode, flags, centre, param, rot, scene, mask, B, tiles);
    int *cnt = (int *)workspace;
    hipLaunchKernelGGL(tp3d::region_count_kernel, dim3((unsigned)blocks), dim3(tp3d::RC_BLOCK), 0, s, a, cnt);
    if (int rc = tp3d::check_launch()) return rc;
    hipLaunchKernelGGL(tp3d::region_scan_kernel, dim3(1), dim3(tp3d::RC_SCAN_BLOCK), 0, s, cnt, blocks, tiles, B, mode,
                       capacity, start, status);
    return tp3d::check_launch();
}

TP3D_EXPORT int tp3d_region_emit_f32(const float *pos, int64_t N, const int64_t *seg, int64_t S, int kind, int mode, int flags,
                                     const float *centre, const float *param, const float *rot, const int64_t *scene,
                                     const uint8_t *mask, int64_t B, int64_t capacity, const int64_t *status, int64_t *index,
                                     int64_t *batch, float *pos_out, int64_t *seg_out, const void *workspace,
                                     size_t workspace_bytes, void *stream)
{
    int64_t tiles, blocks;
    if (int rc = tp3d::region_check(pos, N, seg, S, kind, mode, centre, param, scene, mask, B, tiles, blocks)) return rc;
    if (capacity < 0 || !status || (capacity > 0 && !index)) return TP3D_E_BADARG;
    if (kind == tp3d::RC_MASK && pos_out) return TP3D_E_BADARG;  // a mask has no positions to copy
    if (mode == tp3d::RC_KEEP && seg_out && !seg) return TP3D_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    if (blocks > 0) {
        if (!workspace || workspace_bytes < tp3d_region_workspace_bytes(N, B, mode)) return TP3D_E_BADARG;
        const tp3d::RegionArgs a =
            tp3d::region_args(pos, N, seg, S, kind, mode, flags, centre, param, rot, scene, mask, B, tiles);
        hipLaunchKernelGGL(tp3d::region_emit_kernel, dim3((unsigned)blocks), dim3(tp3d::RC_BLOCK), 0, s, a,
                           (const int *)workspace, capacity, index, mode == tp3d::RC_EACH ? batch : nullptr, pos_out);
        if (int rc = tp3d::check_launch()) return rc;
    }
    if (mode == tp3d::RC_KEEP && seg_out) {
        hipLaunchKernelGGL(tp3d::region_seg_kernel, dim3((unsigned)(S / 256 + 1)), dim3(256), 0, s, index, status, capacity,
                           seg, S, seg_out);
        return tp3d::check_launch();
    }
    return TP3D_OK;
}

TP3D_EXPORT int tp3d_elastic_blur_f32(float *noise, float *tmp, const int32_t *dims, const int64_t *goff, int64_t B,
                                      int64_t total, int rounds, void *stream)
{
    if (B < 0 || total < 0 || rounds < 0) return TP3D_E_BADARG;
    if (B == 0 || total == 0 || rounds == 0) return TP3D_OK;
    if (!noise || !tmp || !dims || !goff) return TP3D_E_BADARG;
    const int64_t blocks = (total + tp3d::EL_BLOCK - 1) / tp3d::EL_BLOCK;
    if (blocks > INT32_MAX) return TP3D_E_TOOBIG;
    float *src = noise, *dst = tmp;
    for (int pass = 0; pass < 3 * rounds; ++pass) {
        hipLaunchKernelGGL(tp3d::elastic_blur_kernel, dim3((unsigned)blocks), dim3(tp3d::EL_BLOCK), 0, (hipStream_t)stream,
                           (const float *)src, dst, dims, goff, B, total, pass % 3);
        if (int rc = tp3d::check_launch()) return rc;
        float *t = src;
        src = dst;
        dst = t;
    }
    if (src != noise)  // an odd number of passes ends in tmp
        return tp3d::hip_rc(hipMemcpyAsync(noise, src, (size_t)total * sizeof(float), hipMemcpyDeviceToDevice,
                                           (hipStream_t)stream));
    return TP3D_OK;
}

TP3D_EXPORT int tp3d_elastic_apply_f32(const float *pos, const int64_t *seg, int64_t B, int64_t N, const float *noise,
                                       const int32_t *dims, const int64_t *goff, const double *axes, double magnitude,
                                       float *out, void *stream)
{
    if (B < 0 || N < 0) return TP3D_E_BADARG;
    if (N == 0) return TP3D_OK;
    if (B == 0 || !pos || !seg || !noise || !dims || !goff || !axes || !out) return TP3D_E_BADARG;
    const int64_t blocks = (N + tp3d::EL_BLOCK - 1) / tp3d::EL_BLOCK;
    if (blocks > INT32_MAX) return TP3D_E_TOOBIG;
    hipLaunchKernelGGL(tp3d::elastic_apply_kernel, dim3((unsigned)blocks), dim3(tp3d::EL_BLOCK), 0, (hipStream_t)stream, pos,
                       seg, B, N, noise, dims, goff, axes, magnitude, out);
    return tp3d::check_launch();
}
