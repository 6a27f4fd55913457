// Registration descriptors (torch_points3d/core/losses/metric_losses.py, utils/registration.py): the nearest row of b in
// feature space for every row of a, and the normal equations + pose update of Fast Global Registration.
//
// feature_nn   dist2[i] = min_j sum_c (a[i][c] - b[j][c])^2 over the allowed j, idx[i] the lowest such j.  The direct
//   difference form in fp32 (descriptors are unit vectors and the hard negatives are the small distances, where
//   |a|^2 + |b|^2 - 2ab cancels).  A workgroup of four waves owns 64 * RPT query rows, kept in registers (lane l of
//   EVERY wave holds rows l, l + 64, ...); b is streamed through LDS in chunks of FN_ROWS rows, wave w takes the rows
//   w, w + 4, ... of a chunk, and every lane of a wave reads the same LDS address (a broadcast, no bank conflict).  The sum
//   over the channels runs in four interleaved chains, c = 0, 4, 8, ... | 1, 5, ... | ..., each an fma chain in ascending c,
//   combined as (s0 + s1) + (s2 + s3); wider rows than the register tile are summed tile after tile in ascending order.
//   (distance bits << 32 | j) is a u64 whose unsigned order is (distance, index) order: d2 >= +0, and a NaN has larger
//   bits than +inf, so it never beats the "nothing" key (inf, 0xffffffff).  S is split over blockIdx.y; the per-split
//   minima go to the workspace and a second kernel takes their minimum and decodes it.  Integer minima only: the result
//   does not depend on the execution order and repeats are bit-equal.
//
// fgr   one iteration = fgr_accumulate_kernel (per-block partial sums of the 21 + 6 distinct entries of A^T A and A^T b of
//   get_matrix_system, in double, the (3N, 6) matrix is never stored) + fgr_solve_kernel (one wave: the partials added in
//   block order, a 6 x 6 solve by Gaussian elimination with partial pivoting, the Rodrigues matrix of get_trans, T_res <-
//   T T_res, mu halved on the reference's schedule).  The pose lives in device memory in double between the launches: the
//   host reads nothing back.
#include "tp3d_common.h"

namespace tp3d {

constexpr int FN_BLOCK = 256;
constexpr int FN_WAVES = FN_BLOCK / kWave;
constexpr int FN_ROWS = 64;                        // rows of b per LDS chunk
constexpr int FN_ROWS_PER_WAVE = FN_ROWS / FN_WAVES;
constexpr int FN_TARGET_BLOCKS = 1024;             // workgroups asked for before S stops being split further
constexpr unsigned long long FN_NONE = (0x7f800000ull << 32) | 0xffffffffull;

struct FnPlan {
    int ct, rpt;       // channels per register tile, query rows per lane
    bool multi;        // C > the widest register tile: the channel tiles are looped over
    int xblocks, splits;
    int64_t rows_per_split;
};

static FnPlan fn_plan(int64_t P, int64_t S, int C)
{
    FnPlan p;
    p.multi = C > 128;
    if (C <= 32) p.ct = 32, p.rpt = 2;
    else if (C <= 64) p.ct = 64, p.rpt = 2;
    else if (C <= 128) p.ct = 128, p.rpt = 1;
    else p.ct = 64, p.rpt = 1;
    const int tile = kWave * p.rpt;
    p.xblocks = (int)((P + tile - 1) / tile);
    const int64_t chunks = (S + FN_ROWS - 1) / FN_ROWS;
    int64_t want = FN_TARGET_BLOCKS / (p.xblocks > 0 ? p.xblocks : 1);
    if (want < 1) want = 1;
    if (want > chunks) want = chunks;
    if (want > 1024) want = 1024;
    if (want < 1) want = 1;
    const int64_t chunks_per_split = (chunks + want - 1) / want;
    p.rows_per_split = (chunks_per_split > 0 ? chunks_per_split : 1) * FN_ROWS;
    p.splits = (int)((S + p.rows_per_split - 1) / p.rows_per_split);
    if (p.splits < 1) p.splits = 1;
    return p;
}

// sum over one register tile of (a[c] - b[c])^2, four interleaved fma chains; brow: LDS, the same address in every lane
template <int CT>
__device__ __forceinline__ float fn_tile_dist(const float (&a)[CT], const float *brow)
{
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
#pragma unroll
    for (int c = 0; c < CT; c += 4) {
        const float4 bv = *reinterpret_cast<const float4 *>(brow + c);
        const float d0 = a[c] - bv.x, d1 = a[c + 1] - bv.y, d2 = a[c + 2] - bv.z, d3 = a[c + 3] - bv.w;
        s0 = __builtin_fmaf(d0, d0, s0);
        s1 = __builtin_fmaf(d1, d1, s1);
        s2 = __builtin_fmaf(d2, d2, s2);
        s3 = __builtin_fmaf(d3, d3, s3);
    }
    return (s0 + s1) + (s2 + s3);
}

template <int CT>
__device__ __forceinline__ void fn_load_a(float (&a)[CT], const float *__restrict__ arow, int c0, int C, bool live)
{
#pragma unroll
    for (int c = 0; c < CT; ++c) a[c] = (live && c0 + c < C) ? arow[c0 + c] : 0.0f;
}

// rows [j0, j0 + FN_ROWS) x channels [c0, c0 + CT) of b into s_b[FN_ROWS][CT], zeros outside [0, jend) x [0, C)
template <int CT>
__device__ __forceinline__ void fn_stage_b(float *s_b, const float *__restrict__ b, int64_t j0, int64_t jend, int c0, int C,
                                           bool vec)
{
    if (vec) {  // C % 4 == 0 and b 16-byte aligned: c0 and CT are multiples of 4, so a group of 4 is inside the row or outside
        for (int e = threadIdx.x; e < FN_ROWS * (CT / 4); e += FN_BLOCK) {
            const int r = e / (CT / 4), c = (e % (CT / 4)) * 4;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (j0 + r < jend && c0 + c < C) v = *reinterpret_cast<const float4 *>(b + (j0 + r) * C + c0 + c);
            *reinterpret_cast<float4 *>(s_b + r * CT + c) = v;
        }
    } else {
        for (int e = threadIdx.x; e < FN_ROWS * CT; e += FN_BLOCK) {
            const int r = e / CT, c = e % CT;
            s_b[e] = (j0 + r < jend && c0 + c < C) ? b[(j0 + r) * C + c0 + c] : 0.0f;
        }
    }
}

__device__ __forceinline__ unsigned long long fn_key(float d2, int64_t j, bool allowed)
{
    const unsigned long long k = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned long long)(unsigned)j;
    return allowed ? k : FN_NONE;
}

__device__ __forceinline__ unsigned long long fn_min(unsigned long long x, unsigned long long y) { return x < y ? x : y; }

template <int CT, int RPT, bool MULTI>
__global__ __launch_bounds__(FN_BLOCK) void feature_nn_kernel(const float *__restrict__ a, const float *__restrict__ b,
                                                               const float *__restrict__ pos_a, const float *__restrict__ pos_b,
                                                               int64_t P, int64_t S, int C, float min_dist,
                                                               int64_t rows_per_split, int vec,
                                                               unsigned long long *__restrict__ partial)
{
    __shared__ __attribute__((aligned(16))) float s_b[FN_ROWS * CT];
    __shared__ float s_pos[FN_ROWS * 3];
    __shared__ unsigned long long s_best[FN_WAVES][kWave * RPT];
    __shared__ float s_acc[MULTI ? FN_ROWS_PER_WAVE * RPT : 1][FN_BLOCK];  // MULTI: the distances of the chunk's rows so far
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const bool use_pos = pos_a != nullptr;
    const int64_t row0 = (int64_t)blockIdx.x * (kWave * RPT) + lane;
    const int64_t jbeg = (int64_t)blockIdx.y * rows_per_split;
    const int64_t jend = jbeg + rows_per_split < S ? jbeg + rows_per_split : S;

    float av[RPT][CT];
    float pa[RPT][3];
    bool live[RPT];
    unsigned long long best[RPT];
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        const int64_t row = row0 + (int64_t)r * kWave;
        live[r] = row < P;
        best[r] = FN_NONE;
        if (!MULTI) fn_load_a<CT>(av[r], a + (live[r] ? row : 0) * C, 0, C, live[r]);
#pragma unroll
        for (int d = 0; d < 3; ++d) pa[r][d] = (use_pos && live[r]) ? pos_a[row * 3 + d] : 0.0f;
    }

    // (distance, index) key of chunk row jj for query row r, or "nothing" when the positions rule the pair out
    auto key_of = [&](int r, int jj, int64_t j, float d2) {
        bool allowed = true;
        if (use_pos) {
            const float p2 = sqdist3(pa[r][0], pa[r][1], pa[r][2], s_pos[jj * 3], s_pos[jj * 3 + 1], s_pos[jj * 3 + 2]);
            allowed = sqrtf(p2 + 1e-7f) > min_dist;
        }
        return fn_key(d2, j, allowed);
    };
    for (int64_t j0 = jbeg; j0 < jend; j0 += FN_ROWS) {
        const int nrows = (int)(jend - j0 < FN_ROWS ? jend - j0 : FN_ROWS);
        for (int c0 = 0; c0 < (MULTI ? C : 1); c0 += CT) {
            __syncthreads();  // the previous tile has been read by every wave
            fn_stage_b<CT>(s_b, b, j0, jend, c0, C, vec != 0);
            if (use_pos && c0 == 0)
                for (int e = threadIdx.x; e < FN_ROWS * 3; e += FN_BLOCK) s_pos[e] = e / 3 < nrows ? pos_b[j0 * 3 + e] : 0.0f;
            if (MULTI) {
#pragma unroll
                for (int r = 0; r < RPT; ++r) fn_load_a<CT>(av[r], a + (live[r] ? row0 + (int64_t)r * kWave : 0) * C, c0, C, live[r]);
            }
            __syncthreads();
            // (not unrolled further: the compiler would hoist the LDS reads of every row and spill the query tile)
#pragma unroll 2
            for (int jj = wave; jj < nrows; jj += FN_WAVES) {
#pragma unroll
                for (int r = 0; r < RPT; ++r) {
                    const float t = fn_tile_dist<CT>(av[r], s_b + jj * CT);
                    if (MULTI) {  // the tiles of a row are added in ascending channel order; each slot has one owner lane
                        float *slot = &s_acc[(jj / FN_WAVES) * RPT + r][threadIdx.x];
                        *slot = c0 == 0 ? t : *slot + t;
                    } else {
                        best[r] = fn_min(best[r], key_of(r, jj, j0 + jj, t));
                    }
                }
            }
        }
        if (MULTI) {
            for (int jj = wave; jj < nrows; jj += FN_WAVES)
#pragma unroll
                for (int r = 0; r < RPT; ++r)
                    best[r] = fn_min(best[r], key_of(r, jj, j0 + jj, s_acc[(jj / FN_WAVES) * RPT + r][threadIdx.x]));
        }
    }
#pragma unroll
    for (int r = 0; r < RPT; ++r) s_best[wave][r * kWave + lane] = best[r];
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
            unsigned long long m = s_best[0][r * kWave + lane];
#pragma unroll
            for (int w = 1; w < FN_WAVES; ++w) m = fn_min(m, s_best[w][r * kWave + lane]);
            if (live[r]) partial[(int64_t)blockIdx.y * P + row0 + (int64_t)r * kWave] = m;
        }
    }
}

__global__ __launch_bounds__(FN_BLOCK) void feature_nn_reduce_kernel(const unsigned long long *__restrict__ partial, int64_t P,
                                                                      int splits, float *__restrict__ dist2,
                                                                      int64_t *__restrict__ idx)
{
    const int64_t i = (int64_t)blockIdx.x * FN_BLOCK + threadIdx.x;
    if (i >= P) return;
    unsigned long long m = FN_NONE;
    for (int s = 0; s < splits; ++s) m = fn_min(m, partial[(int64_t)s * P + i]);
    const unsigned lo = (unsigned)(m & 0xffffffffull);
    dist2[i] = __uint_as_float((unsigned)(m >> 32));
    idx[i] = lo == 0xffffffffu ? (int64_t)-1 : (int64_t)lo;
}

// ------------------------------------------------------------------------------------------- fast global registration
constexpr int FGR_BLOCK = 256;
constexpr int FGR_MAX_BLOCKS = 128;
constexpr int FGR_TERMS = 27;  // 21 upper entries of A^T A (row-major, b >= a) + 6 of A^T b
constexpr int FGR_STATE = 17;  // doubles: T_res (4 x 4, row-major), mu

static int fgr_blocks(int64_t N)
{
    const int64_t nb = (N + FGR_BLOCK - 1) / FGR_BLOCK;
    return (int)(nb < 1 ? 1 : (nb > FGR_MAX_BLOCKS ? FGR_MAX_BLOCKS : nb));
}

__device__ __forceinline__ bool fgr_finite(double v)
{
    return ((unsigned long long)__double_as_longlong(v) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

// state: T_res and mu of the previous iteration (iter == 0: identity; the weights are 1 and mu is not read)
__global__ __launch_bounds__(FGR_BLOCK) void fgr_accumulate_kernel(const float *__restrict__ xyz, const float *__restrict__ tgt,
                                                                    int64_t N, const double *__restrict__ state, int iter,
                                                                    double *__restrict__ partial)
{
    __shared__ double s_red[FGR_BLOCK / kWave][FGR_TERMS];
    double T[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    double mu = 1.0;
    if (iter > 0) {
#pragma unroll
        for (int e = 0; e < 12; ++e) T[e] = state[e];
        mu = state[16];
    }
    double m[FGR_TERMS];
#pragma unroll
    for (int e = 0; e < FGR_TERMS; ++e) m[e] = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * FGR_BLOCK + threadIdx.x; i < N; i += (int64_t)gridDim.x * FGR_BLOCK) {
        const double px = xyz[i * 3], py = xyz[i * 3 + 1], pz = xyz[i * 3 + 2];
        const double x = ((T[0] * px + T[1] * py) + T[2] * pz) + T[3];
        const double y = ((T[4] * px + T[5] * py) + T[6] * pz) + T[7];
        const double z = ((T[8] * px + T[9] * py) + T[10] * pz) + T[11];
        const double res[3] = {(double)tgt[i * 3] - x, (double)tgt[i * 3 + 1] - y, (double)tgt[i * 3 + 2] - z};
        double w = 1.0;
        if (iter > 0) w = mu / (mu + ((res[0] * res[0] + res[1] * res[1]) + res[2] * res[2]));
        const double w2 = w * w;  // the weight multiplies A and b alike
        // the three rows of get_matrix_system (without the weight): minus the cross-product matrix of s | identity
        const double rows[3][6] = {{0.0, z, -y, 1.0, 0.0, 0.0}, {-z, 0.0, x, 0.0, 1.0, 0.0}, {y, -x, 0.0, 0.0, 0.0, 1.0}};
        int e = 0;
#pragma unroll
        for (int p = 0; p < 6; ++p)
#pragma unroll
            for (int q = p; q < 6; ++q, ++e)
                m[e] += w2 * ((rows[0][p] * rows[0][q] + rows[1][p] * rows[1][q]) + rows[2][p] * rows[2][q]);
#pragma unroll
        for (int p = 0; p < 6; ++p) m[21 + p] += w2 * ((rows[0][p] * res[0] + rows[1][p] * res[1]) + rows[2][p] * res[2]);
    }
    // lanes of a wave in a fixed butterfly, then the waves in order
#pragma unroll
    for (int e = 0; e < FGR_TERMS; ++e) {
        double v = m[e];
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
        m[e] = v;
    }
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    if (lane == 0) {
#pragma unroll
        for (int e = 0; e < FGR_TERMS; ++e) s_red[wave][e] = m[e];
    }
    __syncthreads();
    if (threadIdx.x < FGR_TERMS) {
        double v = s_red[0][threadIdx.x];
        for (int w = 1; w < FGR_BLOCK / kWave; ++w) v += s_red[w][threadIdx.x];
        partial[(int64_t)blockIdx.x * FGR_TERMS + threadIdx.x] = v;
    }
}

__global__ __launch_bounds__(kWave) void fgr_solve_kernel(const double *__restrict__ partial, int blocks, double *__restrict__ state,
                                                           int iter, double mu_init, float *__restrict__ T_out)
{
    __shared__ double s_sum[FGR_TERMS];
    __shared__ double s_m[6][7];
    if (threadIdx.x < FGR_TERMS) {
        double v = 0.0;
        for (int k = 0; k < blocks; ++k) v += partial[(int64_t)k * FGR_TERMS + threadIdx.x];
        s_sum[threadIdx.x] = v;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double Tres[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    double mu = mu_init;
    if (iter > 0) {
        for (int e = 0; e < 16; ++e) Tres[e] = state[e];
        mu = state[16];
    }
    if (iter > 0 && iter % 5 == 0) mu *= 0.5;
    int e = 0;
    for (int p = 0; p < 6; ++p)
        for (int q = p; q < 6; ++q, ++e) s_m[p][q] = s_m[q][p] = s_sum[e];
    for (int p = 0; p < 6; ++p) s_m[p][6] = s_sum[21 + p];
    bool ok = true;
    for (int c = 0; c < 6 && ok; ++c) {
        int piv = c;
        double big = fabs(s_m[c][c]);
        for (int r = c + 1; r < 6; ++r) {
            const double v = fabs(s_m[r][c]);
            if (v > big) big = v, piv = r;
        }
        if (!(big > 0.0) || !fgr_finite(big)) {  // a pivot that is exactly 0 (or not a number): no update this iteration
            ok = false;
            break;
        }
        if (piv != c)
            for (int q = c; q < 7; ++q) {
                const double t = s_m[c][q];
                s_m[c][q] = s_m[piv][q];
                s_m[piv][q] = t;
            }
        for (int r = c + 1; r < 6; ++r) {
            const double f = s_m[r][c] / s_m[c][c];
            for (int q = c; q < 7; ++q) s_m[r][q] -= f * s_m[c][q];
        }
    }
    double x[6] = {0, 0, 0, 0, 0, 0};
    if (ok) {
        for (int r = 5; r >= 0; --r) {
            double v = s_m[r][6];
            for (int q = r + 1; q < 6; ++q) v -= s_m[r][q] * x[q];
            x[r] = v / s_m[r][r];
            ok = ok && fgr_finite(x[r]);
        }
    }
    if (ok) {
        // get_trans: Rodrigues matrix of the axis x[0:3] / theta and the angle theta (identity at theta == 0), t = x[3:6]
        const double theta = sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]);
        double k0 = x[0], k1 = x[1], k2 = x[2];
        if (theta > 0.0) k0 /= theta, k1 /= theta, k2 /= theta;
        const double K[3][3] = {{0.0, -k2, k1}, {k2, 0.0, -k0}, {-k1, k0, 0.0}};
        const double sn = sin(theta), cs = 1.0 - cos(theta);
        double T[16] = {1, 0, 0, x[3], 0, 1, 0, x[4], 0, 0, 1, x[5], 0, 0, 0, 1};
        for (int p = 0; p < 3; ++p)
            for (int q = 0; q < 3; ++q) {
                const double kk = (K[p][0] * K[0][q] + K[p][1] * K[1][q]) + K[p][2] * K[2][q];
                T[p * 4 + q] = ((p == q ? 1.0 : 0.0) + sn * K[p][q]) + cs * kk;
            }
        double out[16];
        for (int p = 0; p < 4; ++p)
            for (int q = 0; q < 4; ++q) {
                double v = 0.0;
                for (int k = 0; k < 4; ++k) v += T[p * 4 + k] * Tres[k * 4 + q];
                out[p * 4 + q] = v;
                ok = ok && fgr_finite(v);
            }
        if (ok)
            for (int k = 0; k < 16; ++k) Tres[k] = out[k];
    }
    for (int k = 0; k < 16; ++k) {
        state[k] = Tres[k];
        T_out[k] = (float)Tres[k];
    }
    state[16] = mu;
}

}  // namespace tp3d

using namespace tp3d;

TP3D_EXPORT size_t tp3d_feature_nn_workspace_bytes(int64_t P, int64_t S, int C)
{
    if (P <= 0 || S <= 0 || C <= 0 || P >= 0x7fffffff || S >= 0x7fffffff) return 0;
    return (size_t)fn_plan(P, S, C).splits * (size_t)P * sizeof(unsigned long long);
}

TP3D_EXPORT int tp3d_feature_nn_f32(const float *a, const float *b, const float *pos_a, const float *pos_b, int64_t P, int64_t S,
                                    int C, float min_dist, float *dist2, int64_t *idx, void *workspace, size_t workspace_bytes,
                                    void *stream)
{
    if (P < 0 || S < 0 || C <= 0 || ((pos_a == nullptr) != (pos_b == nullptr))) return TP3D_E_BADARG;
    if (P == 0) return TP3D_OK;
    if (!a || !dist2 || !idx) return TP3D_E_BADARG;
    if (P >= 0x7fffffff || S >= 0x7fffffff || (int64_t)C * (P > S ? P : S) >= ((int64_t)1 << 40)) return TP3D_E_TOOBIG;
    hipStream_t s = (hipStream_t)stream;
    const unsigned rblocks = (unsigned)((P + FN_BLOCK - 1) / FN_BLOCK);
    if (S == 0) {  // no candidate at all: the reduce kernel over zero splits writes (inf, -1)
        hipLaunchKernelGGL(feature_nn_reduce_kernel, dim3(rblocks), dim3(FN_BLOCK), 0, s, nullptr, P, 0, dist2, idx);
        return check_launch();
    }
    if (!b || !workspace) return TP3D_E_BADARG;
    const FnPlan p = fn_plan(P, S, C);
    if (workspace_bytes < (size_t)p.splits * (size_t)P * sizeof(unsigned long long)) return TP3D_E_BADARG;
    unsigned long long *partial = static_cast<unsigned long long *>(workspace);
    const int vec = (C & 3) == 0 && (reinterpret_cast<uintptr_t>(b) & 15) == 0;
    const dim3 grid((unsigned)p.xblocks, (unsigned)p.splits);
#define FN_LAUNCH(CT, RPT, MULTI)                                                                                               \
    hipLaunchKernelGGL((feature_nn_kernel<CT, RPT, MULTI>), grid, dim3(FN_BLOCK), 0, s, a, b, pos_a, pos_b, P, S, C, min_dist, \
                       p.rows_per_split, vec, partial)
    if (p.multi) FN_LAUNCH(64, 1, true);
    else if (p.ct == 32) FN_LAUNCH(32, 2, false);
    else if (p.ct == 64) FN_LAUNCH(64, 2, false);
    else FN_LAUNCH(128, 1, false);
#undef FN_LAUNCH
    if (int rc = check_launch()) return rc;
    hipLaunchKernelGGL(feature_nn_reduce_kernel, dim3(rblocks), dim3(FN_BLOCK), 0, s, partial, P, p.splits, dist2, idx);
    return check_launch();
}

TP3D_EXPORT size_t tp3d_fgr_workspace_bytes(int64_t N)
{
    if (N < 0 || N >= 0x7fffffff / 3) return 0;
    return ((size_t)fgr_blocks(N) * FGR_TERMS + FGR_STATE) * sizeof(double);
}

// workspace: [state: 17 doubles][partials: blocks x 27 doubles]
TP3D_EXPORT int tp3d_fgr_accumulate_f32(const float *xyz, const float *xyz_target, int64_t N, int iter, void *workspace,
                                        size_t workspace_bytes, void *stream)
{
    if (N < 0 || iter < 0 || !workspace) return TP3D_E_BADARG;
    if (N >= 0x7fffffff / 3) return TP3D_E_TOOBIG;
    if (N > 0 && (!xyz || !xyz_target)) return TP3D_E_BADARG;
    if (workspace_bytes < tp3d_fgr_workspace_bytes(N)) return TP3D_E_BADARG;
    double *state = static_cast<double *>(workspace);
    hipLaunchKernelGGL(fgr_accumulate_kernel, dim3((unsigned)fgr_blocks(N)), dim3(FGR_BLOCK), 0, (hipStream_t)stream, xyz, xyz_target,
                       N, state, iter, state + FGR_STATE);
    return check_launch();
}

TP3D_EXPORT int tp3d_fgr_solve(int64_t N, int iter, double mu_init, float *T, void *workspace, size_t workspace_bytes, void *stream)
{
    if (N < 0 || iter < 0 || !workspace || !T) return TP3D_E_BADARG;
    if (N >= 0x7fffffff / 3) return TP3D_E_TOOBIG;
    if (workspace_bytes < tp3d_fgr_workspace_bytes(N)) return TP3D_E_BADARG;
    double *state = static_cast<double *>(workspace);
    hipLaunchKernelGGL(fgr_solve_kernel, dim3(1), dim3(kWave), 0, (hipStream_t)stream, state + FGR_STATE, fgr_blocks(N), state, iter,
                       mu_init, T);
    return check_launch();
}
