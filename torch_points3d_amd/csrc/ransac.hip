// RANSAC over correspondences (utils/registration.py:141-163, open3d's registration_ransac_based_on_correspondence) and
// the weighted Kabsch refit, on the device.
//
// ransac_pose_kernel    one thread per hypothesis: the rigid pose of its n sampled pairs by Horn's closed form in double
//   (ransac_horn.h), rounded to 12 floats.  Computed ONCE per hypothesis: the Jacobi sweeps cost as much as scoring a few
//   hundred correspondences, so the score kernel reads the 48 bytes back instead of repeating them per split.
// ransac_score_kernel   one thread per hypothesis with its pose in 12 registers; the correspondences are the same for
//   every lane, so their addresses are wave-uniform and the loads are scalar loads that cost no vector or LDS issue slot
//   (a form that staged tiles of pairs in LDS and read them as broadcasts was 3-7 % slower).  fp32:
//   s_a = fma(R_a0, px, fma(R_a1, py, fma(R_a2, pz, t_a))), d_a = s_a - q_a, d2 = fma(dz, dz, fma(dy, dy, dx * dx)),
//   a hit when d2 < threshold^2.  N is split over blockIdx.y in whole tiles; the per-split counts go to an integer
//   table that ransac_count_kernel adds in split order.  Integers only: nothing depends on the execution order.
// ransac_select_kernel  one workgroup: the maximum of (count << 32) | (0xffffffff - h), i.e. the highest count and among
//   equal counts the LOWEST index; the winner's pose is formed again in double and written to the workspace.
// kabsch_accumulate_kernel / kabsch_solve_kernel   the shape of fgr_accumulate / fgr_solve (registration.hip): per-block
//   partial sums in double of the weight, the weighted sums of p and q and the 9 cross products, the weight being
//   weight[i] and / or the gate "within `threshold` of q under the pose of the workspace"; one wave adds the partials in
//   block order, centres them, runs Horn and writes the pose.  The inlier set is never compacted or read back.
#include "tp3d_common.h"
#include "ransac_horn.h"

namespace tp3d {

constexpr int RS_BLOCK = TP3D_RANSAC_HYP_BLOCK;  // hypotheses per workgroup, one per thread
constexpr int RS_TILE = TP3D_RANSAC_TILE;        // correspondences per tile: the unit N is split in
constexpr int RS_TARGET_BLOCKS = 1024;           // workgroups asked for (four per CU) before N stops being split further
constexpr int RS_MAX_SPLITS = 64;
constexpr int RS_MAX_N = 8;                      // largest sample size
constexpr int RS_SELECT_BLOCK = 1024;

constexpr int KB_BLOCK = 256;
constexpr int KB_MAX_BLOCKS = 128;
constexpr int KB_TERMS = 18;  // W, sum w p (3), sum w q (3), sum w p_a q_b (9), gated count, gated sum of d^2
// the head of the workspace, doubles: pose (12, row-major [R | t]), 12 has_pose, 13 best index, 14 best count,
// 15 gated count and 16 gated sum of d^2 of the last accumulate, 17 its weight sum
constexpr int RS_STATE = 32;

struct RsPlan {
    int xblocks, splits, per_split;
};

static RsPlan rs_plan(int64_t N, int64_t H)
{
    RsPlan p;
    p.xblocks = (int)((H + RS_BLOCK - 1) / RS_BLOCK);
    const int64_t tiles = (N + RS_TILE - 1) / RS_TILE;
    int64_t want = (RS_TARGET_BLOCKS + p.xblocks - 1) / (p.xblocks > 0 ? p.xblocks : 1);
    if (want > RS_MAX_SPLITS) want = RS_MAX_SPLITS;
    if (want > tiles) want = tiles;
    if (want < 1) want = 1;
    const int64_t tiles_per_split = (tiles + want - 1) / want;
    p.per_split = (int)((tiles_per_split > 0 ? tiles_per_split : 1) * RS_TILE);
    p.splits = (int)((N + p.per_split - 1) / p.per_split);
    if (p.splits < 1) p.splits = 1;
    return p;
}

static int kb_blocks(int64_t N)
{
    const int64_t nb = (N + KB_BLOCK - 1) / KB_BLOCK;
    return (int)(nb < 1 ? 1 : (nb > KB_MAX_BLOCKS ? KB_MAX_BLOCKS : nb));
}

static bool rs_served(int64_t N, int64_t H) { return N >= 3 && N < 0x7fffffff / 3 && H >= 0 && H <= ((int64_t)1 << 31); }

static size_t rs_partial_offset() { return (size_t)RS_STATE * sizeof(double); }
static size_t rs_poses_offset() { return rs_partial_offset() + (size_t)KB_MAX_BLOCKS * KB_TERMS * sizeof(double); }
static size_t rs_counts_offset(int64_t H) { return align_up(rs_poses_offset() + (size_t)H * 12 * sizeof(float), 16); }

// (the translation units are built with -fno-honor-nans: "finite" is read from the exponent bits)
__device__ __forceinline__ bool rs_finite(double v)
{
    return ((unsigned long long)__double_as_longlong(v) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

__device__ __forceinline__ bool rs_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// the pose of hypothesis h in double; false (and a pose of NaNs) if a sampled row lies outside [0, N) or the result is not finite
__device__ __forceinline__ bool rs_hypothesis(const float *__restrict__ xyz, const float *__restrict__ tgt, int64_t N,
                                              const int64_t *__restrict__ samples, int64_t h, int n, double (&pose)[12])
{
    double mp[3] = {0, 0, 0}, mq[3] = {0, 0, 0}, S[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    bool ok = true;
    for (int k = 0; k < n; ++k) {
        const int64_t i = samples[h * n + k];
        if (i < 0 || i >= N) {
            ok = false;
            continue;
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) mp[a] += (double)xyz[i * 3 + a], mq[a] += (double)tgt[i * 3 + a];
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) mp[a] /= (double)n, mq[a] /= (double)n;
    for (int k = 0; k < n && ok; ++k) {
        const int64_t i = samples[h * n + k];
        double p[3], q[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) p[a] = (double)xyz[i * 3 + a] - mp[a], q[a] = (double)tgt[i * 3 + a] - mq[a];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) S[a * 3 + b] += p[a] * q[b];
    }
    if (ok) {
        horn_pose(S, mp, mq, pose);
#pragma unroll
        for (int e = 0; e < 12; ++e) ok = ok && rs_finite(pose[e]);
    }
    if (!ok) {
#pragma unroll
        for (int e = 0; e < 12; ++e) pose[e] = __longlong_as_double(0x7ff8000000000000ll);
    }
    return ok;
}

__global__ __launch_bounds__(RS_BLOCK) void ransac_pose_kernel(const float *__restrict__ xyz, const float *__restrict__ tgt, int64_t N,
                                                               const int64_t *__restrict__ samples, int64_t H, int n,
                                                               float *__restrict__ poses)
{
    const int64_t h = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
    if (h >= H) return;
    double pose[12];
    rs_hypothesis(xyz, tgt, N, samples, h, n, pose);
#pragma unroll
    for (int e = 0; e < 12; ++e) poses[h * 12 + e] = (float)pose[e];
}

__device__ __forceinline__ int rs_hit(const float (&P)[12], float px, float py, float pz, float qx, float qy, float qz, float thr2)
{
    const float dx = fmaf(P[0], px, fmaf(P[1], py, fmaf(P[2], pz, P[3]))) - qx;
    const float dy = fmaf(P[4], px, fmaf(P[5], py, fmaf(P[6], pz, P[7]))) - qy;
    const float dz = fmaf(P[8], px, fmaf(P[9], py, fmaf(P[10], pz, P[11]))) - qz;
    return fmaf(dz, dz, fmaf(dy, dy, dx * dx)) < thr2 ? 1 : 0;
}

// grid (hypothesis blocks, splits of N); out: counts (one split) or the (splits, H) table
__global__ __launch_bounds__(RS_BLOCK) void ransac_score_kernel(const float *__restrict__ xyz, const float *__restrict__ tgt, int N,
                                                                const float *__restrict__ poses, int64_t H, float thr2,
                                                                int per_split, int vec, int32_t *__restrict__ out)
{
    const int64_t h = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
    const bool live = h < H;
    float P[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (live) {
#pragma unroll
        for (int e = 0; e < 12; ++e) P[e] = poses[h * 12 + e];
    }
    bool ok = true;
#pragma unroll
    for (int e = 0; e < 12; ++e) ok = ok && rs_finite(P[e]);
    const int lo = (int)blockIdx.y * per_split;
    const int hi = lo + per_split < N ? lo + per_split : N;
    int count = 0;
    // the index is the same in every lane: scalar loads, the coordinates sit in scalar registers.  Four
    // correspondences are 12 floats = three 16-byte loads per side (lo is a multiple of the tile, so with 16-byte
    // aligned clouds every group is aligned; `vec` says they are)
    int i = lo;
    if (vec) {
        const float4 *__restrict__ p4 = reinterpret_cast<const float4 *>(xyz + 3 * lo);
        const float4 *__restrict__ q4 = reinterpret_cast<const float4 *>(tgt + 3 * lo);
        const int groups = (hi - lo) >> 2;
#pragma unroll 2
        for (int g = 0; g < groups; ++g) {
            const float4 a = p4[3 * g], b = p4[3 * g + 1], c = p4[3 * g + 2];
            const float4 u = q4[3 * g], v = q4[3 * g + 1], w = q4[3 * g + 2];
            count += rs_hit(P, a.x, a.y, a.z, u.x, u.y, u.z, thr2);
            count += rs_hit(P, a.w, b.x, b.y, u.w, v.x, v.y, thr2);
            count += rs_hit(P, b.z, b.w, c.x, v.z, v.w, w.x, thr2);
            count += rs_hit(P, c.y, c.z, c.w, w.y, w.z, w.w, thr2);
        }
        i += groups * 4;
    }
    for (; i < hi; ++i)
        count += rs_hit(P, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], tgt[3 * i], tgt[3 * i + 1], tgt[3 * i + 2], thr2);
    if (live) out[(int64_t)blockIdx.y * H + h] = ok ? count : 0;
}

__global__ __launch_bounds__(RS_BLOCK) void ransac_count_kernel(const int32_t *__restrict__ partial, int splits, int64_t H,
                                                                int32_t *__restrict__ counts)
{
    const int64_t h = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
    if (h >= H) return;
    int v = 0;
    for (int s = 0; s < splits; ++s) v += partial[(int64_t)s * H + h];
    counts[h] = v;
}

__global__ __launch_bounds__(RS_SELECT_BLOCK) void ransac_select_kernel(const int32_t *__restrict__ counts, int64_t H,
                                                                        const float *__restrict__ xyz, const float *__restrict__ tgt,
                                                                        int64_t N, const int64_t *__restrict__ samples, int n,
                                                                        double *__restrict__ state)
{
    __shared__ unsigned long long s_key[RS_SELECT_BLOCK / kWave];
    unsigned long long key = 0;
    for (int64_t h = threadIdx.x; h < H; h += RS_SELECT_BLOCK) {
        const unsigned long long k = ((unsigned long long)(unsigned)counts[h] << 32) | (unsigned long long)(0xffffffffu - (unsigned)h);
        key = k > key ? k : key;
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)key, off), hi = __shfl_xor((unsigned)(key >> 32), off);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        key = o > key ? o : key;
    }
    if ((threadIdx.x & (kWave - 1)) == 0) s_key[threadIdx.x / kWave] = key;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < RS_SELECT_BLOCK / kWave; ++w) key = s_key[w] > key ? s_key[w] : key;
    const int64_t best = (int64_t)(0xffffffffu - (unsigned)(key & 0xffffffffull));
    double pose[12];
    const bool ok = rs_hypothesis(xyz, tgt, N, samples, best, n, pose);
#pragma unroll
    for (int e = 0; e < 12; ++e) state[e] = ok ? pose[e] : (e % 5 == 0 ? 1.0 : 0.0);
    state[12] = ok ? 1.0 : 0.0;
    state[13] = (double)best;
    state[14] = (double)(unsigned)(key >> 32);
    state[15] = state[16] = state[17] = 0.0;
}

// gate: only correspondences within `threshold` of their target under the workspace's pose weigh in (none without a pose)
__global__ __launch_bounds__(KB_BLOCK) void kabsch_accumulate_kernel(const float *__restrict__ xyz, const float *__restrict__ tgt,
                                                                     const float *__restrict__ weight, int64_t N,
                                                                     const double *__restrict__ state, int gate, double thr2,
                                                                     double *__restrict__ partial)
{
    __shared__ double s_red[KB_BLOCK / kWave][KB_TERMS];
    double T[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    bool has_pose = false;
    if (gate) {
        has_pose = state[12] != 0.0;
        if (has_pose) {
#pragma unroll
            for (int e = 0; e < 12; ++e) T[e] = state[e];
        }
    }
    double m[KB_TERMS];
#pragma unroll
    for (int e = 0; e < KB_TERMS; ++e) m[e] = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * KB_BLOCK + threadIdx.x; i < N; i += (int64_t)gridDim.x * KB_BLOCK) {
        const double p[3] = {(double)xyz[i * 3], (double)xyz[i * 3 + 1], (double)xyz[i * 3 + 2]};
        const double q[3] = {(double)tgt[i * 3], (double)tgt[i * 3 + 1], (double)tgt[i * 3 + 2]};
        double w = weight ? (double)weight[i] : 1.0;
        if (gate) {
            const double dx = (((T[0] * p[0] + T[1] * p[1]) + T[2] * p[2]) + T[3]) - q[0];
            const double dy = (((T[4] * p[0] + T[5] * p[1]) + T[6] * p[2]) + T[7]) - q[1];
            const double dz = (((T[8] * p[0] + T[9] * p[1]) + T[10] * p[2]) + T[11]) - q[2];
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            if (has_pose && d2 < thr2) {
                m[16] += 1.0;
                m[17] += d2;
            } else {
                w = 0.0;
            }
        }
        m[0] += w;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            m[1 + a] += w * p[a];
            m[4 + a] += w * q[a];
#pragma unroll
            for (int b = 0; b < 3; ++b) m[7 + a * 3 + b] += w * (p[a] * q[b]);
        }
    }
    // lanes of a wave in a fixed butterfly, then the waves in order
#pragma unroll
    for (int e = 0; e < KB_TERMS; ++e) {
        double v = m[e];
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
        m[e] = v;
    }
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    if (lane == 0) {
#pragma unroll
        for (int e = 0; e < KB_TERMS; ++e) s_red[wave][e] = m[e];
    }
    __syncthreads();
    if (threadIdx.x < KB_TERMS) {
        double v = s_red[0][threadIdx.x];
        for (int w = 1; w < KB_BLOCK / kWave; ++w) v += s_red[w][threadIdx.x];
        partial[(int64_t)blockIdx.x * KB_TERMS + threadIdx.x] = v;
    }
}

// update == 0: the pose stays; only the stats of the accumulate are recorded (and T written)
__global__ __launch_bounds__(kWave) void kabsch_solve_kernel(const double *__restrict__ partial, int blocks, double *__restrict__ state,
                                                             int gate, int update, float *__restrict__ T_out)
{
    __shared__ double s_sum[KB_TERMS];
    if (threadIdx.x < KB_TERMS) {
        double v = 0.0;
        for (int k = 0; k < blocks; ++k) v += partial[(int64_t)k * KB_TERMS + threadIdx.x];
        s_sum[threadIdx.x] = v;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double pose[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    bool has_pose = gate && state[12] != 0.0;  // (a solve without the gate starts afresh)
    if (has_pose)
        for (int e = 0; e < 12; ++e) pose[e] = state[e];
    const double W = s_sum[0];
    if (update && rs_finite(W) && W > 0.0 && (!gate || s_sum[16] >= 3.0)) {
        double mp[3], mq[3], S[9], fresh[12];
        for (int a = 0; a < 3; ++a) mp[a] = s_sum[1 + a] / W, mq[a] = s_sum[4 + a] / W;
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) S[a * 3 + b] = s_sum[7 + a * 3 + b] / W - mp[a] * mq[b];
        horn_pose(S, mp, mq, fresh);
        bool ok = true;
        for (int e = 0; e < 12; ++e) ok = ok && rs_finite(fresh[e]);
        if (ok) {
            for (int e = 0; e < 12; ++e) pose[e] = fresh[e];
            has_pose = true;
        }
    }
    for (int e = 0; e < 12; ++e) state[e] = pose[e];
    state[12] = has_pose ? 1.0 : 0.0;
    state[15] = s_sum[16];
    state[16] = s_sum[17];
    state[17] = W;
    if (T_out) {
        for (int e = 0; e < 12; ++e) T_out[e] = (float)pose[e];
        T_out[12] = T_out[13] = T_out[14] = 0.0f;
        T_out[15] = 1.0f;
    }
}

}  // namespace tp3d

using namespace tp3d;

TP3D_EXPORT size_t tp3d_ransac_workspace_bytes(int64_t N, int64_t H)
{
    if (!rs_served(N, H)) return 0;
    return rs_counts_offset(H) + (size_t)rs_plan(N, H).splits * (size_t)H * sizeof(int32_t);
}

TP3D_EXPORT int tp3d_ransac_splits(int64_t N, int64_t H) { return rs_served(N, H) && H > 0 ? rs_plan(N, H).splits : 0; }

// workspace: [state: 32 doubles][Kabsch partials: 128 x 18 doubles][poses: H x 12 floats][counts per split: splits x H int32]
TP3D_EXPORT int tp3d_ransac_score_f32(const float *xyz, const float *xyz_target, int64_t N, const int64_t *samples, int64_t H, int n,
                                      float threshold, float *poses, int32_t *counts, void *workspace, size_t workspace_bytes,
                                      void *stream)
{
    if (N < 3 || H < 1 || n < 3 || n > RS_MAX_N || !xyz || !xyz_target || !samples || !counts || !workspace) return TP3D_E_BADARG;
    if (!rs_served(N, H)) return TP3D_E_TOOBIG;
    if (workspace_bytes < tp3d_ransac_workspace_bytes(N, H)) return TP3D_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    char *ws = static_cast<char *>(workspace);
    if (!poses) poses = reinterpret_cast<float *>(ws + rs_poses_offset());
    const RsPlan p = rs_plan(N, H);
    hipLaunchKernelGGL(ransac_pose_kernel, dim3((unsigned)p.xblocks), dim3(RS_BLOCK), 0, s, xyz, xyz_target, N, samples, H, n, poses);
    if (int rc = check_launch()) return rc;
    int32_t *partial = reinterpret_cast<int32_t *>(ws + rs_counts_offset(H));
    const int vec = ((reinterpret_cast<uintptr_t>(xyz) | reinterpret_cast<uintptr_t>(xyz_target)) & 15) == 0;
    hipLaunchKernelGGL(ransac_score_kernel, dim3((unsigned)p.xblocks, (unsigned)p.splits), dim3(RS_BLOCK), 0, s, xyz,
                       xyz_target, (int)N, poses, H, threshold * threshold, p.per_split, vec, p.splits == 1 ? counts : partial);
    if (int rc = check_launch()) return rc;
    if (p.splits == 1) return TP3D_OK;
    hipLaunchKernelGGL(ransac_count_kernel, dim3((unsigned)p.xblocks), dim3(RS_BLOCK), 0, s, partial, p.splits, H, counts);
    return check_launch();
}

TP3D_EXPORT int tp3d_ransac_select(const float *xyz, const float *xyz_target, int64_t N, const int64_t *samples, int64_t H, int n,
                                   const int32_t *counts, void *workspace, size_t workspace_bytes, void *stream)
{
    if (N < 3 || H < 1 || n < 3 || n > RS_MAX_N || !xyz || !xyz_target || !samples || !counts || !workspace) return TP3D_E_BADARG;
    if (!rs_served(N, H)) return TP3D_E_TOOBIG;
    if (workspace_bytes < tp3d_ransac_workspace_bytes(N, H)) return TP3D_E_BADARG;
    hipLaunchKernelGGL(ransac_select_kernel, dim3(1), dim3(RS_SELECT_BLOCK), 0, (hipStream_t)stream, counts, H, xyz, xyz_target, N,
                       samples, n, static_cast<double *>(workspace));
    return check_launch();
}

TP3D_EXPORT int tp3d_kabsch_accumulate_f32(const float *xyz, const float *xyz_target, const float *weight, int64_t N, int gate,
                                           double threshold, void *workspace, size_t workspace_bytes, void *stream)
{
    if (N < 3 || !xyz || !xyz_target || !workspace) return TP3D_E_BADARG;
    if (!rs_served(N, 0)) return TP3D_E_TOOBIG;
    if (workspace_bytes < tp3d_ransac_workspace_bytes(N, 0)) return TP3D_E_BADARG;
    double *state = static_cast<double *>(workspace);
    hipLaunchKernelGGL(kabsch_accumulate_kernel, dim3((unsigned)kb_blocks(N)), dim3(KB_BLOCK), 0, (hipStream_t)stream, xyz, xyz_target,
                       weight, N, state, gate, threshold * threshold, state + RS_STATE);
    return check_launch();
}

TP3D_EXPORT int tp3d_kabsch_solve(int64_t N, int gate, int update, float *T, void *workspace, size_t workspace_bytes, void *stream)
{
    if (N < 3 || !workspace) return TP3D_E_BADARG;
    if (!rs_served(N, 0)) return TP3D_E_TOOBIG;
    if (workspace_bytes < tp3d_ransac_workspace_bytes(N, 0)) return TP3D_E_BADARG;
    double *state = static_cast<double *>(workspace);
    hipLaunchKernelGGL(kabsch_solve_kernel, dim3(1), dim3(kWave), 0, (hipStream_t)stream, state + RS_STATE, kb_blocks(N), state, gate,
                       update, T);
    return check_launch();
}
