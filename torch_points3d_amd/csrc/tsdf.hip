// TSDF fusion on the device (include/tp3d_hip.h, "TSDF fusion"): depth frames into a truncated signed distance volume,
// the surface cloud of a volume, and the unprojection of depth frames -- the reference's datasets/registration/fusion.py
// and utils.py, as restated in float64 numpy by torch_points3d_amd/tsdf.py.  That file is the definition; every rule
// below is evaluated in the same order with one rounding per operation (-ffp-contract=off keeps v_fma out), so the
// results are bit-equal to it.  One owner per voxel, plain vector stores, no atomics.
//
// The two compactions are count (per tile) -> one block scan (block_scan_chunk of inverse_table.h) -> emit (ballot +
// prefix inside the tile, rows ascending), the pieces of the region cut of transforms.hip over another predicate; the
// predicate is evaluated on the fly in both passes, nothing of volume size is written.
#include "inverse_table.h"

namespace tp3d {

constexpr int TS_BLOCK = 256;               // threads of every kernel here
constexpr int TS_SUB = 4;                   // rows per thread of the compactions
constexpr int TS_TILE = TS_BLOCK * TS_SUB;  // rows per tile: sub-chunk j holds rows tile * TS_TILE + j * TS_BLOCK + tid
constexpr int TS_WAVES = TS_BLOCK / kWave;
constexpr int TS_SCAN_BLOCK = 1024;
constexpr int TS_CONSTS = TP3D_TSDF_CONSTS;
constexpr int UP_CONSTS = TP3D_UNPROJECT_CONSTS;

// depth in metres of one pixel: raw 16-bit (divided by the scale, zeroed above the threshold: rgbd2fragment_fine's
// preprocessing, done in the load) or float64 metres as they are
__device__ __forceinline__ double depth_metres(const uint16_t *__restrict__ depth, int64_t at, double scale, double thresh)
{
    const double d = (double)depth[at] / scale;
    return d > thresh ? 0.0 : d;
}
__device__ __forceinline__ double depth_metres(const double *__restrict__ depth, int64_t at, double, double) { return depth[at]; }

// One thread per voxel, consecutive threads along z.  The F frames are applied in order to the voxel's two values in
// registers: one read and at most one write of each volume element.  consts[f] is read at a wave-uniform address.
template <typename DepthT>
__global__ __launch_bounds__(TS_BLOCK) void tsdf_integrate_kernel(float *__restrict__ tsdf, float *__restrict__ weight,
                                                                  int64_t N, int64_t dy, int64_t dz, float ox, float oy,
                                                                  float oz, float vs, double trunc,
                                                                  const DepthT *__restrict__ depth, int F, int H, int W,
                                                                  const double *__restrict__ consts, double depth_scale,
                                                                  double depth_thresh)
{
    const int64_t i = (int64_t)blockIdx.x * TS_BLOCK + threadIdx.x;
    if (i >= N) return;
    const int64_t iz = i % dz, iy = (i / dz) % dy, ix = i / (dz * dy);
    // two fp32 roundings per coordinate
    const double px = (double)(ox + vs * (float)ix);
    const double py = (double)(oy + vs * (float)iy);
    const double pz = (double)(oz + vs * (float)iz);
    float t = tsdf[i], w = weight[i];
    bool touched = false;
    const double fw = (double)W, fh = (double)H;
    const int64_t HW = (int64_t)H * W;
    for (int f = 0; f < F; ++f) {
        const double *c = consts + (int64_t)f * TS_CONSTS;
        const double cz = ((c[8] * px + c[9] * py) + c[10] * pz) + c[11];
        if (!(cz > 0.0)) continue;  // before any division
        const double cx = ((c[0] * px + c[1] * py) + c[2] * pz) + c[3];
        const double cy = ((c[4] * px + c[5] * py) + c[6] * pz) + c[7];
        const double u = rint(cx * c[12] / cz + c[14]);
        const double v = rint(cy * c[13] / cz + c[15]);
        if (!(u >= 0.0 && u < fw && v >= 0.0 && v < fh)) continue;  // in double, before the cast
        const double d = depth_metres(depth, f * HW + (int64_t)v * W + (int64_t)u, depth_scale, depth_thresh);
        if (!(d > 0.0)) continue;
        const double diff = d - cz;
        if (!(diff >= -trunc)) continue;
        const double q = diff / trunc;
        const double dist = q < 1.0 ? q : 1.0;
        const double obs = c[16];
        const float w_new = (float)((double)w + obs);
        const float prod = w * t;  // fp32 x fp32, rounded to fp32
        t = (float)(((double)prod + obs * dist) / (double)w_new);
        w = w_new;
        touched = true;
    }
    if (touched) {
        tsdf[i] = t;
        weight[i] = w;
    }
}

// ------------------------------------------------------------------------------------------------------------- compaction
// A predicate P selects rows of `lists` lists of `rows` rows each (the voxels of one volume; the pixels of F frames).
// block -> (list, tile).
struct SurfacePred {
    const float *tsdf, *weight;
    float tsdf_thresh, weight_thresh;
    __device__ __forceinline__ bool operator()(int64_t, int64_t row) const
    {
        return fabsf(tsdf[row]) < tsdf_thresh && weight[row] > weight_thresh;
    }
};

struct DepthPred {
    const uint16_t *depth;
    int64_t HW;
    double scale, max_depth;
    __device__ __forceinline__ double z(int64_t list, int64_t row) const { return (double)depth[list * HW + row] / scale; }
    __device__ __forceinline__ bool operator()(int64_t list, int64_t row) const
    {
        const double Z = z(list, row);
        return Z < max_depth && Z > 0.0;
    }
};

template <typename P>
__global__ __launch_bounds__(TS_BLOCK) void compact_count_kernel(P pred, int64_t rows, int64_t tiles, int *__restrict__ cnt)
{
    __shared__ int s_cnt[TS_WAVES];
    const int64_t list = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    int mine = 0;
#pragma unroll
    for (int j = 0; j < TS_SUB; ++j) {
        const int64_t row = tile * TS_TILE + j * TS_BLOCK + threadIdx.x;
        mine += (row < rows && pred(list, row)) ? 1 : 0;
    }
    const int total = wave_inclusive_scan(mine);
    if (lane_id() == kWave - 1) s_cnt[threadIdx.x >> 6] = total;
    __syncthreads();
    if (threadIdx.x == 0) {
        int sum = 0;
#pragma unroll
        for (int w = 0; w < TS_WAVES; ++w) sum += s_cnt[w];
        cnt[blockIdx.x] = sum;
    }
}

// cnt[0 .. n) -> exclusive offsets in place; start[l] = the offset of list l's first tile, start[lists] = the total
// (start null: not wanted); status = [total, total > capacity] (capacity < 0: no bound)
__global__ __launch_bounds__(TS_SCAN_BLOCK) void compact_scan_kernel(int *__restrict__ cnt, int64_t n, int64_t tiles,
                                                                     int64_t lists, int64_t capacity,
                                                                     int64_t *__restrict__ start,
                                                                     int64_t *__restrict__ status)
{
    __shared__ int s_wave[TS_SCAN_BLOCK / 64];
    int64_t k0, k1;
    int run = block_scan_chunk<TS_SCAN_BLOCK, int64_t>(cnt, n, s_wave, k0, k1);
    for (int64_t k = k0; k < k1; ++k) {
        const int c = cnt[k];
        cnt[k] = run;
        if (start && k % tiles == 0) start[k / tiles] = run;
        run += c;
    }
    if (threadIdx.x == TS_SCAN_BLOCK - 1) {  // the last chunk ends at n: run is the total
        if (start) start[lists] = run;
        status[0] = run;
        status[1] = (capacity >= 0 && run > capacity) ? 1 : 0;
    }
}

// E::emit(list, row, dst) writes one selected row to slot dst < capacity
template <typename P, typename E>
__global__ __launch_bounds__(TS_BLOCK) void compact_emit_kernel(P pred, E out, int64_t rows, int64_t tiles,
                                                                const int *__restrict__ offset, int64_t capacity)
{
    __shared__ int s_cnt[TS_SUB * TS_WAVES];
    const int64_t list = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int wave = threadIdx.x >> 6;
    bool sel[TS_SUB];
    int below[TS_SUB];
#pragma unroll
    for (int j = 0; j < TS_SUB; ++j) {
        const int64_t row = tile * TS_TILE + j * TS_BLOCK + threadIdx.x;
        sel[j] = row < rows && pred(list, row);
        const unsigned long long m = __ballot(sel[j]);
        below[j] = lanes_below(m);
        if (lane_id() == 0) s_cnt[j * TS_WAVES + wave] = __popcll(m);
    }
    __syncthreads();
    const int64_t base = offset[blockIdx.x];
    int front = 0;  // selected rows of the tile in the (sub-chunk, wave) pairs before this one
#pragma unroll
    for (int j = 0; j < TS_SUB; ++j) {
#pragma unroll
        for (int w = 0; w < TS_WAVES; ++w) {
            if (w == wave && sel[j]) {
                const int64_t dst = base + front + below[j];
                // a total beyond the capacity is reported by status[1]; nothing is written past it
                if (dst < capacity) out.emit(list, tile * TS_TILE + j * TS_BLOCK + threadIdx.x, dst);
            }
            front += s_cnt[j * TS_WAVES + w];
        }
    }
}

struct SurfaceEmit {
    int64_t dy, dz;
    double ox, oy, oz, vs;
    double *pos;
    int64_t *index;
    __device__ __forceinline__ void emit(int64_t, int64_t row, int64_t dst) const
    {
        const int64_t iz = row % dz, iy = (row / dz) % dy, ix = row / (dz * dy);
        if (pos) {
            pos[3 * dst] = (double)ix * vs + ox;
            pos[3 * dst + 1] = (double)iy * vs + oy;
            pos[3 * dst + 2] = (double)iz * vs + oz;
        }
        if (index) index[dst] = row;
    }
};

struct DepthEmit {
    DepthPred pred;
    int64_t W;
    const double *consts;
    double *pos;
    int64_t *pixel;
    __device__ __forceinline__ void emit(int64_t list, int64_t row, int64_t dst) const
    {
        if (pos) {
            const double *c = consts + list * UP_CONSTS;
            const double Z = pred.z(list, row);
            const double x = (double)(row % W), y = (double)(row / W);
            const double X = ((x + 0.5) - c[14]) * Z / c[12];
            const double Y = ((y + 0.5) - c[15]) * Z / c[13];
#pragma unroll
            for (int a = 0; a < 3; ++a) pos[3 * dst + a] = ((X * c[4 * a] + Y * c[4 * a + 1]) + Z * c[4 * a + 2]) + c[4 * a + 3];
        }
        if (pixel) pixel[dst] = list * pred.HW + row;
    }
};

// tiles and blocks of a compaction over `lists` lists of `rows` rows; the offsets are ints
static int compact_shape(int64_t lists, int64_t rows, int64_t &tiles, int64_t &blocks)
{
    if (lists < 0 || rows < 0) return TP3D_E_BADARG;
    if (rows > INT32_MAX || lists > INT32_MAX || lists * rows > INT32_MAX) return TP3D_E_TOOBIG;
    tiles = (rows + TS_TILE - 1) / TS_TILE;
    blocks = tiles * lists;
    return TP3D_OK;
}

static size_t compact_workspace_bytes(int64_t lists, int64_t rows)
{
    int64_t tiles, blocks;
    if (compact_shape(lists, rows, tiles, blocks) != TP3D_OK) return 0;
    return align_up((size_t)blocks * sizeof(int), 256);
}

template <typename P>
static int compact_count(const P &pred, int64_t lists, int64_t rows, int64_t capacity, int64_t *start, int64_t *status,
                         void *workspace, size_t workspace_bytes, hipStream_t s)
{
    int64_t tiles, blocks;
    if (int rc = compact_shape(lists, rows, tiles, blocks)) return rc;
    if (!status) return TP3D_E_BADARG;
    if (blocks == 0) {
        if (start)
            if (int rc = zero_async(start, (size_t)(lists + 1) * sizeof(int64_t), s)) return rc;
        return zero_async(status, 2 * sizeof(int64_t), s);
    }
    if (!workspace || workspace_bytes < compact_workspace_bytes(lists, rows)) return TP3D_E_BADARG;
    int *cnt = (int *)workspace;
    hipLaunchKernelGGL(compact_count_kernel<P>, dim3((unsigned)blocks), dim3(TS_BLOCK), 0, s, pred, rows, tiles, cnt);
    if (int rc = check_launch()) return rc;
    hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(TS_SCAN_BLOCK), 0, s, cnt, blocks, tiles, lists, capacity, start,
                       status);
    return check_launch();
}

template <typename P, typename E>
static int compact_emit(const P &pred, const E &out, int64_t lists, int64_t rows, int64_t capacity, const void *workspace,
                        size_t workspace_bytes, hipStream_t s)
{
    int64_t tiles, blocks;
    if (int rc = compact_shape(lists, rows, tiles, blocks)) return rc;
    if (capacity < 0) return TP3D_E_BADARG;
    if (blocks == 0 || capacity == 0) return TP3D_OK;
    if (!workspace || workspace_bytes < compact_workspace_bytes(lists, rows)) return TP3D_E_BADARG;
    hipLaunchKernelGGL((compact_emit_kernel<P, E>), dim3((unsigned)blocks), dim3(TS_BLOCK), 0, s, pred, out, rows, tiles,
                       (const int *)workspace, capacity);
    return check_launch();
}

}  // namespace tp3d

TP3D_EXPORT int tp3d_tsdf_tile_rows(void) { return tp3d::TS_TILE; }

TP3D_EXPORT int tp3d_tsdf_integrate(float *tsdf, float *weight, int64_t X, int64_t Y, int64_t Z, float ox, float oy, float oz,
                                    double voxel_size, double trunc, const void *depth, int depth_kind, int F, int H, int W,
                                    const double *consts, double depth_scale, double depth_thresh, void *stream)
{
    if (X < 0 || Y < 0 || Z < 0 || F < 0 || H < 0 || W < 0 || (depth_kind != 0 && depth_kind != 1)) return TP3D_E_BADARG;
    if (F > TP3D_TSDF_MAX_FRAMES) return TP3D_E_BADARG;
    if (!(trunc > 0.0) || !(depth_scale > 0.0)) return TP3D_E_BADARG;
    if (X > INT32_MAX || Y > INT32_MAX || Z > INT32_MAX) return TP3D_E_TOOBIG;
    if (X == 0 || Y == 0 || Z == 0 || F == 0) return TP3D_OK;
    if (Y * Z > INT32_MAX || (Y * Z) * X > (int64_t)INT32_MAX * tp3d::TS_BLOCK) return TP3D_E_TOOBIG;
    const int64_t N = X * Y * Z;
    if (H == 0 || W == 0) return TP3D_OK;  // frames without pixels see nothing
    if (!tsdf || !weight || !depth || !consts) return TP3D_E_BADARG;
    const int64_t blocks = (N + tp3d::TS_BLOCK - 1) / tp3d::TS_BLOCK;
    hipStream_t s = (hipStream_t)stream;
    const float vs = (float)voxel_size;
    if (depth_kind == 0)
        hipLaunchKernelGGL(tp3d::tsdf_integrate_kernel<uint16_t>, dim3((unsigned)blocks), dim3(tp3d::TS_BLOCK), 0, s, tsdf,
                           weight, N, Y, Z, ox, oy, oz, vs, trunc, (const uint16_t *)depth, F, H, W, consts, depth_scale,
                           depth_thresh);
    else
        hipLaunchKernelGGL(tp3d::tsdf_integrate_kernel<double>, dim3((unsigned)blocks), dim3(tp3d::TS_BLOCK), 0, s, tsdf,
                           weight, N, Y, Z, ox, oy, oz, vs, trunc, (const double *)depth, F, H, W, consts, depth_scale,
                           depth_thresh);
    return tp3d::check_launch();
}

TP3D_EXPORT size_t tp3d_tsdf_surface_workspace_bytes(int64_t N) { return tp3d::compact_workspace_bytes(1, N); }

TP3D_EXPORT int tp3d_tsdf_surface_count(const float *tsdf, const float *weight, int64_t N, float tsdf_thresh,
                                        float weight_thresh, int64_t capacity, int64_t *status, void *workspace,
                                        size_t workspace_bytes, void *stream)
{
    if (N > 0 && (!tsdf || !weight)) return TP3D_E_BADARG;
    const tp3d::SurfacePred pred = {tsdf, weight, tsdf_thresh, weight_thresh};
    return tp3d::compact_count(pred, 1, N, capacity, nullptr, status, workspace, workspace_bytes, (hipStream_t)stream);
}

TP3D_EXPORT int tp3d_tsdf_surface_emit(const float *tsdf, const float *weight, int64_t X, int64_t Y, int64_t Z, float ox,
                                       float oy, float oz, double voxel_size, float tsdf_thresh, float weight_thresh,
                                       int64_t capacity, double *pos, int64_t *index, const void *workspace,
                                       size_t workspace_bytes, void *stream)
{
    if (X < 0 || Y < 0 || Z < 0) return TP3D_E_BADARG;
    if (X > INT32_MAX || Y > INT32_MAX || Z > INT32_MAX || Y * Z > INT32_MAX || (Y * Z) * X > INT32_MAX) return TP3D_E_TOOBIG;
    const int64_t N = X * Y * Z;
    if (N > 0 && (!tsdf || !weight)) return TP3D_E_BADARG;
    const tp3d::SurfacePred pred = {tsdf, weight, tsdf_thresh, weight_thresh};
    const tp3d::SurfaceEmit out = {Y, Z, (double)ox, (double)oy, (double)oz, voxel_size, pos, index};
    return tp3d::compact_emit(pred, out, 1, N, capacity, workspace, workspace_bytes, (hipStream_t)stream);
}

TP3D_EXPORT size_t tp3d_depth_unproject_workspace_bytes(int64_t F, int64_t HW) { return tp3d::compact_workspace_bytes(F, HW); }

TP3D_EXPORT int tp3d_depth_unproject_count(const uint16_t *depth, int64_t F, int64_t H, int64_t W, double depth_scale,
                                           double max_depth, int64_t capacity, int64_t *start, int64_t *status,
                                           void *workspace, size_t workspace_bytes, void *stream)
{
    if (F < 0 || H < 0 || W < 0 || !(depth_scale > 0.0) || !start) return TP3D_E_BADARG;
    if (H > INT32_MAX || W > INT32_MAX) return TP3D_E_TOOBIG;
    if (F > 0 && H > 0 && W > 0 && !depth) return TP3D_E_BADARG;
    const tp3d::DepthPred pred = {depth, H * W, depth_scale, max_depth};
    return tp3d::compact_count(pred, F, H * W, capacity, start, status, workspace, workspace_bytes, (hipStream_t)stream);
}

TP3D_EXPORT int tp3d_depth_unproject_emit(const uint16_t *depth, int64_t F, int64_t H, int64_t W, const double *consts,
                                          double depth_scale, double max_depth, int64_t capacity, double *pos,
                                          int64_t *pixel, const void *workspace, size_t workspace_bytes, void *stream)
{
    if (F < 0 || H < 0 || W < 0 || !(depth_scale > 0.0)) return TP3D_E_BADARG;
    if (H > INT32_MAX || W > INT32_MAX) return TP3D_E_TOOBIG;
    if (F > 0 && H > 0 && W > 0 && (!depth || (pos && !consts))) return TP3D_E_BADARG;
    const tp3d::DepthPred pred = {depth, H * W, depth_scale, max_depth};
    const tp3d::DepthEmit out = {pred, W, consts, pos, pixel};
    return tp3d::compact_emit(pred, out, F, H * W, capacity, workspace, workspace_bytes, (hipStream_t)stream);
}
