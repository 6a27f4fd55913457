// FPFH on the device (include/tp3d_hip.h, "FPFH descriptors"): the hybrid radius / max_nn search, PCA normals, the SPFH
// bin counts and the weighted FPFH sum of open3d's estimate_normals + compute_fpfh_feature, as restated in float64 numpy
// by torch_points3d_amd/fpfh.py (the definition).  Integer counters, fixed summation orders and plain stores only, no
// float atomics: repeats are bit-equal.  Pair features, covariances and the FPFH sums are computed in double from the
// fp32 inputs with +, -, *, /, sqrt only; -ffp-contract=off keeps v_fma out of it, so the counts equal numpy's exactly.
//
// Search: one wave per query over the grid of grid.h built with the radius as the cell edge, so the ball lies inside the
// 27 cells around the query's cell for every max_nn.  Hits (d2 < r2, the membership of the ball query) are appended to a
// per-wave LDS buffer; when it would overflow it is cut at its max_nn-th smallest distance, found by fixing the bits of
// that distance from the top down with ballots over keys held in registers; the distance then bounds admission.  At the
// end the survivors are ranked by (d2, index) against each other and written straight to their slots.
#include "grid.h"

namespace tp3d {

constexpr int FS_BLOCK = 256;  // 4 waves, one query (search) or one point (SPFH) per wave
constexpr int FS_WAVES = FS_BLOCK / kWave;
constexpr int FS_CAP = 1024;                   // candidate slots per wave
constexpr int FS_PER_LANE = FS_CAP / kWave;
constexpr int FS_KMAX = TP3D_FPFH_MAX_NN;      // largest max_nn: the staging slots of an exact cut
constexpr int FPFH_BINS = 11;
constexpr int FPFH_DIM = 3 * FPFH_BINS;
constexpr int FN_BLOCK = 128;  // normals: one thread per point
constexpr int FN_MAX_SWEEPS = 16;

static_assert(FS_KMAX + kWave <= FS_CAP, "a compacted buffer must take one more batch of hits");

// (cos, sin) of the interior bin edges -pi + 2 pi e / 11, e = 1 .. 10: the literals of fpfh.py's EDGE_TABLE
#define TP3D_FPFH_EDGES                                                                                               \
    {-0.84125353283118109, -0.54064081745559778}, {-0.41541501300188632, -0.90963199535451844},                        \
        {0.14231483827328512, -0.98982144188093268}, {0.6548607339452851, -0.75574957435425827},                       \
        {0.95949297361449748, -0.2817325568414295}, {0.95949297361449748, 0.2817325568414295},                         \
        {0.6548607339452851, 0.75574957435425827}, {0.14231483827328512, 0.98982144188093268},                         \
        {-0.41541501300188616, 0.90963199535451855}, {-0.84125353283118132, 0.54064081745559744}
static const double FPFH_EDGE_HOST[10][2] = {TP3D_FPFH_EDGES};
__constant__ double FPFH_EDGE[10][2] = {TP3D_FPFH_EDGES};

__device__ __forceinline__ bool fs_pair_less(float da, int ia, float db, int ib)
{
    return da < db || (da == db && ia < ib);
}

__device__ __forceinline__ void fs_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// ------------------------------------------------------------------------------------------------------------------ search
__global__ __launch_bounds__(FS_BLOCK) void hybrid_search_kernel(
    const float *__restrict__ y, const int64_t *__restrict__ seg, const int64_t *__restrict__ batch_y, int64_t total_q,
    int num_clouds, float r2, int k, int G, const GridInfo *__restrict__ info, const int *__restrict__ cell_start,
    const float4 *__restrict__ sorted_pt, int *__restrict__ idx, float *__restrict__ dist2, int *__restrict__ count)
{
    __shared__ int s_id[FS_WAVES][FS_CAP];
    __shared__ float s_d[FS_WAVES][FS_CAP];
    __shared__ int s_si[FS_WAVES][FS_KMAX];
    __shared__ float s_sd[FS_WAVES][FS_KMAX];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t q = (int64_t)blockIdx.x * FS_WAVES + wave;
    if (q >= total_q) return;  // wave-uniform; the kernel has no workgroup barrier
    int *cid = s_id[wave];
    float *cd = s_d[wave];
    int *si = s_si[wave];
    float *sd = s_sd[wave];
    int *io = idx + q * k;
    float *dd = dist2 + q * k;
    const int64_t bq = batch_y[q];
    int64_t lo = 0;
    int L = 0;
    if (bq >= 0 && bq < num_clouds) {
        lo = seg[bq];
        L = (int)(seg[bq + 1] - seg[bq]);
    }
    int h = 0;  // candidates in the buffer (wave-uniform)
    float tau = 3.0e38f;  // once max_nn hits are known: an upper bound of the max_nn-th distance
    // The k-th smallest distance of the buffer (h >= k): the keys live in registers, 16 per lane, and the bit pattern of
    // the answer is fixed from the top bit down (distances are non-negative, so the patterns order like the values);
    // counts are ballots, no LDS traffic and no cross-lane moves inside the 31 rounds.
    auto kth_distance = [&]() {
        fs_wave_sync();
        unsigned key[FS_PER_LANE];
#pragma unroll
        for (int m = 0; m < FS_PER_LANE; ++m) {
            const int t = m * 64 + lane;
            key[m] = t < h ? __float_as_uint(cd[t]) : 0xffffffffu;
        }
        unsigned res = 0;
        for (int bit = 30; bit >= 0; --bit) {
            const unsigned trial = res | (1u << bit);
            int below = 0;
#pragma unroll
            for (int m = 0; m < FS_PER_LANE; ++m) below += __builtin_popcountll(__ballot(key[m] < trial));
            if (below < k) res = trial;  // fewer than k keys lie below `trial`: the k-th smallest is at least `trial`
        }
        return __uint_as_float(res);
    };
    // keep the pairs with d <= v, in place and in order (a pair moves towards the front only)
    auto squeeze = [&](float v) {
        int nh = 0;
        for (int t0 = 0; t0 < h; t0 += 64) {
            const int t = t0 + lane;
            const float d = t < h ? cd[t] : 0.0f;
            const int id = t < h ? cid[t] : 0;
            const bool keep = t < h && d <= v;
            const unsigned long long mask = __ballot(keep);
            fs_wave_sync();
            if (keep) {
                const int slot = nh + lanes_below(mask);
                cd[slot] = d;
                cid[slot] = id;
            }
            nh += __builtin_popcountll(mask);
            fs_wave_sync();
        }
        h = nh;
    };
    // Rank every pair of the buffer among all of them by (distance, index) -- the indices are distinct, so are the
    // ranks -- and put those of rank < k in their place: the output row (final), or the front of the buffer.  Four pairs
    // per lane share each broadcast read.
    auto place = [&](bool final) {
        fs_wave_sync();
        for (int g0 = 0; g0 < h; g0 += 4 * 64) {
            float d4[4];
            int i4[4], r4[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int t = g0 + m * 64 + lane;
                d4[m] = t < h ? cd[t] : 3.0e38f;
                i4[m] = t < h ? cid[t] : 0x7fffffff;
                r4[m] = 0;
            }
            for (int u = 0; u < h; ++u) {
                const float du = cd[u];
                const int iu = cid[u];
#pragma unroll
                for (int m = 0; m < 4; ++m) r4[m] += fs_pair_less(du, iu, d4[m], i4[m]) ? 1 : 0;
            }
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                if (g0 + m * 64 + lane < h && r4[m] < k) {
                    if (final) {
                        io[r4[m]] = (int)(lo + i4[m]);
                        dd[r4[m]] = d4[m];
                    } else {
                        sd[r4[m]] = d4[m];
                        si[r4[m]] = i4[m];
                    }
                }
            }
        }
        h = min(h, k);
        if (!final) {
            fs_wave_sync();
            for (int t = lane; t < h; t += 64) {
                cd[t] = sd[t];
                cid[t] = si[t];
            }
            fs_wave_sync();
        }
    };
    // the buffer is full: cut it at the k-th distance, which bounds admission from then on.  Pairs AT that distance all
    // stay (one of lower index may still arrive); should so many be equal that no room is won, the cut is made exact.
    auto compact = [&]() {
        tau = kth_distance();
        squeeze(tau);
        if (h + 64 > FS_CAP) place(false);
    };
    if (L > 0) {
        const float qx = y[q * 3 + 0], qy = y[q * 3 + 1], qz = y[q * 3 + 2];
        const GridInfo gi = info[bq];
        const int *cs = cell_start + (size_t)bq * ((size_t)G * G * G + 1);
        // unclamped cell of the query (clamped in float first: a far-away query must not overflow the conversion); cells
        // outside [-1, g] cannot touch the ball: the cell edge is at least 1.01 radius
        const float far = (float)(G + 8);
        const int cx = (int)floorf(fminf(fmaxf((qx - gi.minx) * gi.inv_cs, -4.0f), far));
        const int cy = (int)floorf(fminf(fmaxf((qy - gi.miny) * gi.inv_cs, -4.0f), far));
        const int cz = (int)floorf(fminf(fmaxf((qz - gi.minz) * gi.inv_cs, -4.0f), far));
        const int x0 = max(cx - 1, 0), x1 = min(cx + 1, gi.gx - 1);
        if (x0 <= x1) {
            // the nine (z, y) rows around the query are contiguous x-runs of the cell-ordered copy
            int j0v = 0, j1v = 0;
            if (lane < 9) {
                const int zz = cz + lane / 3 - 1, yy = cy + lane % 3 - 1;
                if (zz >= 0 && zz < gi.gz && yy >= 0 && yy < gi.gy) {
                    const int rowbase = (zz * gi.gy + yy) * gi.gx;
                    j0v = cs[rowbase + x0];
                    j1v = cs[rowbase + x1 + 1];
                }
            }
            for (int rr = 0; rr < 9; ++rr) {
                const int j0 = __shfl(j0v, rr), j1 = min(__shfl(j1v, rr), L);
                for (int j = j0; j < j1; j += 64) {
                    const int t = j + lane;
                    const bool valid = t < j1;
                    const float4 pt = sorted_pt[lo + (valid ? t : j0)];
                    const float d = sqdist3(pt.x, pt.y, pt.z, qx, qy, qz);
                    const int id = __float_as_int(pt.w);
                    bool hit = valid && d < r2 && d <= tau;
                    unsigned long long mask = __ballot(hit);
                    if (!mask) continue;
                    if (h + __builtin_popcountll(mask) > FS_CAP) {
                        compact();
                        hit = hit && d <= tau;
                        mask = __ballot(hit);
                        if (!mask) continue;
                    }
                    if (hit) {
                        const int slot = h + lanes_below(mask);
                        cd[slot] = d;
                        cid[slot] = id;
                    }
                    h += __builtin_popcountll(mask);
                }
            }
        }
    }
    if (h > k) squeeze(kth_distance());  // what is left beyond k lies AT the k-th distance: the ranks decide by index
    place(true);
    for (int s = h + lane; s < k; s += 64) {
        io[s] = -1;
        dd[s] = -1.0f;
    }
    if (lane == 0) count[q] = h;
}

// ----------------------------------------------------------------------------------------------------------------- normals
// one Jacobi rotation in the (P, Q) plane of a symmetric 3 x 3 matrix: A <- J^T A J, V <- V J (horn_rotate of
// ransac_horn.h for three rows)
template <int P, int Q>
__device__ __forceinline__ void fn_rotate(double (&A)[3][3], double (&V)[3][3])
{
    const double apq = A[P][Q];
    if (apq == 0.0) return;
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    A[P][P] -= t * apq;
    A[Q][Q] += t * apq;
    A[P][Q] = A[Q][P] = 0.0;
    constexpr int K = 3 - P - Q;
    const double akp = A[K][P], akq = A[K][Q];
    A[K][P] = A[P][K] = c * akp - s * akq;
    A[K][Q] = A[Q][K] = s * akp + c * akq;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double vp = V[r][P], vq = V[r][Q];
        V[r][P] = c * vp - s * vq;
        V[r][Q] = s * vp + c * vq;
    }
}

__global__ __launch_bounds__(FN_BLOCK) void fpfh_normals_kernel(const float *__restrict__ pos, const int *__restrict__ idx,
                                                                const int *__restrict__ count, int64_t N, int K,
                                                                const float *__restrict__ viewpoint,
                                                                float *__restrict__ normals)
{
    const int64_t i = (int64_t)blockIdx.x * FN_BLOCK + threadIdx.x;
    if (i >= N) return;
    const int k = min(max(count[i], 0), K);
    float *out = normals + 3 * i;
    if (k < 3) {
        out[0] = 0.0f;
        out[1] = 0.0f;
        out[2] = 1.0f;
        return;
    }
    const int *row = idx + i * K;
    double mx = 0.0, my = 0.0, mz = 0.0;
    for (int s = 0; s < k; ++s) {
        const int64_t j = min(max((int64_t)row[s], (int64_t)0), N - 1);
        mx += (double)pos[3 * j];
        my += (double)pos[3 * j + 1];
        mz += (double)pos[3 * j + 2];
    }
    const double kd = (double)k;
    mx = mx / kd;
    my = my / kd;
    mz = mz / kd;
    double A[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    for (int s = 0; s < k; ++s) {
        const int64_t j = min(max((int64_t)row[s], (int64_t)0), N - 1);
        const double dx = (double)pos[3 * j] - mx, dy = (double)pos[3 * j + 1] - my, dz = (double)pos[3 * j + 2] - mz;
        A[0][0] += dx * dx;
        A[0][1] += dx * dy;
        A[0][2] += dx * dz;
        A[1][1] += dy * dy;
        A[1][2] += dy * dz;
        A[2][2] += dz * dz;
    }
    A[0][0] = A[0][0] / kd;
    A[1][1] = A[1][1] / kd;
    A[2][2] = A[2][2] / kd;
    A[0][1] = A[1][0] = A[0][1] / kd;
    A[0][2] = A[2][0] = A[0][2] / kd;
    A[1][2] = A[2][1] = A[1][2] / kd;
    double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    for (int sweep = 0; sweep < FN_MAX_SWEEPS; ++sweep) {
        const double off = (A[0][1] * A[0][1] + A[0][2] * A[0][2]) + A[1][2] * A[1][2];
        const double diag = (A[0][0] * A[0][0] + A[1][1] * A[1][1]) + A[2][2] * A[2][2];
        if (!(off > 1e-36 * diag)) break;
        fn_rotate<0, 1>(A, V);
        fn_rotate<0, 2>(A, V);
        fn_rotate<1, 2>(A, V);
    }
    // the column of the smallest eigenvalue (the lowest index among equal ones)
    double lam = A[0][0];
    double nx = V[0][0], ny = V[1][0], nz = V[2][0];
#pragma unroll
    for (int m = 1; m < 3; ++m) {
        if (A[m][m] < lam) {
            lam = A[m][m];
            nx = V[0][m], ny = V[1][m], nz = V[2][m];
        }
    }
    const double norm = sqrt((nx * nx + ny * ny) + nz * nz);
    nx = nx / norm;
    ny = ny / norm;
    nz = nz / norm;
    bool flip;
    if (viewpoint) {
        const double dx = (double)viewpoint[3 * i] - (double)pos[3 * i];
        const double dy = (double)viewpoint[3 * i + 1] - (double)pos[3 * i + 1];
        const double dz = (double)viewpoint[3 * i + 2] - (double)pos[3 * i + 2];
        flip = (nx * dx + ny * dy) + nz * dz < 0.0;
    } else {
        double top = nx;
        if (fabs(ny) > fabs(top)) top = ny;
        if (fabs(nz) > fabs(top)) top = nz;
        flip = top < 0.0;
    }
    out[0] = (float)(flip ? -nx : nx);
    out[1] = (float)(flip ? -ny : ny);
    out[2] = (float)(flip ? -nz : nz);
}

// -------------------------------------------------------------------------------------------------------------------- SPFH
__device__ __forceinline__ int fpfh_value_bin(double f)
{
    const int b = (int)floor((11.0 * (f + 1.0)) * 0.5);
    return min(max(b, 0), FPFH_BINS - 1);
}

// floor(11 (angle + pi) / 2 pi) of the direction (c, s), clamped, without atan2: the number of interior edges the
// direction has passed (fpfh.py: angle_bin)
__device__ __forceinline__ int fpfh_angle_bin(double c, double s)
{
    if (c == 0.0 && s == 0.0) return 5;
    int b = 0;
#pragma unroll
    for (int e = 0; e < 10; ++e) {
        const double cross = FPFH_EDGE[e][0] * s - FPFH_EDGE[e][1] * c;
        if (e < 5) b += !(s < 0.0 && cross < 0.0) ? 1 : 0;
        else b += (s >= 0.0 && cross >= 0.0) ? 1 : 0;
    }
    return b;
}

// the three bins of the pair (p1, n1) -> (p2, n2)
__device__ __forceinline__ void fpfh_pair_bins(const double (&p1)[3], const double (&n1in)[3], const double (&p2)[3],
                                               const double (&n2in)[3], int &b0, int &b1, int &b2)
{
    b0 = b1 = b2 = 5;  // the features (0, 0, 0)
    double dx = p2[0] - p1[0], dy = p2[1] - p1[1], dz = p2[2] - p1[2];
    const double d = sqrt((dx * dx + dy * dy) + dz * dz);
    if (d == 0.0) return;
    const double a1 = ((n1in[0] * dx + n1in[1] * dy) + n1in[2] * dz) / d;
    const double a2 = ((n2in[0] * dx + n2in[1] * dy) + n2in[2] * dz) / d;
    const bool swap = fabs(a1) < fabs(a2);
    const double f2 = swap ? -a2 : a1;
    double n1[3], n2[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        n1[a] = swap ? n2in[a] : n1in[a];
        n2[a] = swap ? n1in[a] : n2in[a];
    }
    if (swap) {
        dx = -dx;
        dy = -dy;
        dz = -dz;
    }
    double vx = dy * n1[2] - dz * n1[1];
    double vy = dz * n1[0] - dx * n1[2];
    double vz = dx * n1[1] - dy * n1[0];
    const double vn = sqrt((vx * vx + vy * vy) + vz * vz);
    if (vn == 0.0) return;
    vx = vx / vn;
    vy = vy / vn;
    vz = vz / vn;
    const double wx = n1[1] * vz - n1[2] * vy;
    const double wy = n1[2] * vx - n1[0] * vz;
    const double wz = n1[0] * vy - n1[1] * vx;
    const double f1 = (vx * n2[0] + vy * n2[1]) + vz * n2[2];
    const double c = (n1[0] * n2[0] + n1[1] * n2[1]) + n1[2] * n2[2];
    const double s = (wx * n2[0] + wy * n2[1]) + wz * n2[2];
    b0 = fpfh_angle_bin(c, s);
    b1 = fpfh_value_bin(f1);
    b2 = fpfh_value_bin(f2);
}

__global__ __launch_bounds__(FS_BLOCK) void spfh_counts_kernel(const float *__restrict__ pos, const float *__restrict__ nrm,
                                                               const int *__restrict__ idx, const int *__restrict__ count,
                                                               int64_t N, int K, int *__restrict__ counts)
{
    __shared__ int s_cnt[FS_WAVES][FPFH_DIM];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * FS_WAVES + wave;
    const bool live = i < N;  // (no early return: the block meets at the barriers)
    if (lane < FPFH_DIM) s_cnt[wave][lane] = 0;
    __syncthreads();
    if (live) {
        const int k = min(max(count[i], 0), K);
        const double p1[3] = {(double)pos[3 * i], (double)pos[3 * i + 1], (double)pos[3 * i + 2]};
        const double n1[3] = {(double)nrm[3 * i], (double)nrm[3 * i + 1], (double)nrm[3 * i + 2]};
        for (int s = 1 + lane; s < k; s += 64) {
            const int64_t j = idx[i * K + s];
            if (j < 0 || j >= N) continue;
            const double p2[3] = {(double)pos[3 * j], (double)pos[3 * j + 1], (double)pos[3 * j + 2]};
            const double n2[3] = {(double)nrm[3 * j], (double)nrm[3 * j + 1], (double)nrm[3 * j + 2]};
            int b0, b1, b2;
            fpfh_pair_bins(p1, n1, p2, n2, b0, b1, b2);
            atomicAdd(&s_cnt[wave][b0], 1);  // LDS integer adds: order-free and exact
            atomicAdd(&s_cnt[wave][FPFH_BINS + b1], 1);
            atomicAdd(&s_cnt[wave][2 * FPFH_BINS + b2], 1);
        }
    }
    __syncthreads();
    if (live && lane < FPFH_DIM) counts[i * FPFH_DIM + lane] = s_cnt[wave][lane];
}

// -------------------------------------------------------------------------------------------------------------------- FPFH
// One thread per (output row, block of 11 bins): the thread walks the slots in order with the block's 11 sums and its
// normaliser in registers, so every sum has one association -- acc[b] over the slots, sum over (slot, bin) with the bin
// running fastest -- and no value crosses a lane.  (One wave per row with its lanes across the 33 bins, the normaliser
// gathered by eleven cross-lane moves per slot, was built first: bit-equal and 4.2 times slower, 6.9 against 1.65 ms at
// 10^5 rows x 255 slots.)
constexpr int FB_BLOCK = 192;  // 64 rows of three blocks
__global__ __launch_bounds__(FB_BLOCK) void fpfh_rows_kernel(const float *__restrict__ pos, const int *__restrict__ idx,
                                                             const int *__restrict__ count, const int *__restrict__ counts,
                                                             const int64_t *__restrict__ rows, int64_t R, int64_t N, int K,
                                                             double *__restrict__ out64, float *__restrict__ out32)
{
    const int64_t t = (int64_t)blockIdx.x * FB_BLOCK + threadIdx.x;
    const int64_t r = t / 3;
    const int blk = (int)(t - 3 * r);
    if (r >= R) return;
    const int64_t i = rows ? rows[r] : r;
    double acc[FPFH_BINS], own[FPFH_BINS];
    double sum = 0.0;
#pragma unroll
    for (int b = 0; b < FPFH_BINS; ++b) acc[b] = own[b] = 0.0;
    if (i >= 0 && i < N) {
        const int k = min(max(count[i], 0), K);
        const double px = (double)pos[3 * i], py = (double)pos[3 * i + 1], pz = (double)pos[3 * i + 2];
        const int *row = idx + i * K;
        for (int s = 1; s < k; ++s) {
            const int64_t j = row[s];
            if (j < 0 || j >= N) continue;
            const double dx = (double)pos[3 * j] - px, dy = (double)pos[3 * j + 1] - py, dz = (double)pos[3 * j + 2] - pz;
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            if (d2 == 0.0) continue;
            const int kj = count[j];
            const double inc = kj > 1 ? 100.0 / (double)(kj - 1) : 0.0;
            const int *cj = counts + j * FPFH_DIM + blk * FPFH_BINS;
#pragma unroll
            for (int b = 0; b < FPFH_BINS; ++b) {
                const double term = ((double)cj[b] * inc) / d2;
                acc[b] += term;
                sum += term;
            }
        }
        const int ki = count[i];
        const double inc = ki > 1 ? 100.0 / (double)(ki - 1) : 0.0;
#pragma unroll
        for (int b = 0; b < FPFH_BINS; ++b) own[b] = (double)counts[i * FPFH_DIM + blk * FPFH_BINS + b] * inc;
    }
#pragma unroll
    for (int b = 0; b < FPFH_BINS; ++b) {
        const double res = (sum != 0.0 ? (acc[b] * 100.0) / sum : 0.0) + own[b];
        const int64_t o = r * FPFH_DIM + blk * FPFH_BINS + b;
        if (out64) out64[o] = res;
        if (out32) out32[o] = (float)res;
    }
}

}  // namespace tp3d

using namespace tp3d;

TP3D_EXPORT int tp3d_fpfh_edge_table(double *table)
{
    if (!table) return TP3D_E_BADARG;
    for (int e = 0; e < 10; ++e) {
        table[2 * e] = FPFH_EDGE_HOST[e][0];
        table[2 * e + 1] = FPFH_EDGE_HOST[e][1];
    }
    return TP3D_OK;
}

TP3D_EXPORT size_t tp3d_hybrid_search_workspace_bytes(int num_clouds, int64_t rows, int max_cloud_points)
{
    if (num_clouds <= 0 || rows < 0 || max_cloud_points <= 0) return 0;
    const GridPlan plan = grid_plan(max_cloud_points);
    if (plan.G < 2) return 0;
    return carve_grid_workspace(nullptr, num_clouds, rows, plan).bytes;
}

TP3D_EXPORT int tp3d_hybrid_search_f32(const float *x, const float *y, const int64_t *batch_y, const int64_t *seg_x,
                                       int num_clouds, int max_cloud_points, int64_t M, int64_t Nq, float radius,
                                       int max_nn, int32_t *idx, float *dist2, int32_t *count, void *workspace,
                                       size_t workspace_bytes, void *stream)
{
    if (M < 0 || Nq < 0 || max_nn <= 0 || max_nn > FS_KMAX || num_clouds <= 0 || max_cloud_points < 0 || !(radius > 0.0f))
        return TP3D_E_BADARG;
    if (M > 0x7fffffff) return TP3D_E_TOOBIG;
    if (Nq == 0) return TP3D_OK;
    if (!y || !batch_y || !seg_x || !idx || !dist2 || !count || !workspace) return TP3D_E_BADARG;
    if (M > 0 && !x) return TP3D_E_BADARG;
    if (max_cloud_points == 0) max_cloud_points = 1;  // every cloud empty: the kernel only writes the padding
    hipStream_t s = (hipStream_t)stream;
    const GridPlan plan = grid_plan(max_cloud_points);
    if (plan.G < 2) return TP3D_E_TOOBIG;
    GridWorkspace w = carve_grid_workspace(workspace, num_clouds, M, plan);
    if (workspace_bytes < w.bytes) return TP3D_E_BADARG;
    if (int rc = grid_build(x, seg_x, num_clouds, M, 0, max_cloud_points, radius, 2.0f, plan, w, s)) return rc;
    const int64_t blocks = (Nq + FS_WAVES - 1) / FS_WAVES;
    if (blocks > 0x7fffffff) return TP3D_E_TOOBIG;
    hipLaunchKernelGGL(hybrid_search_kernel, dim3((unsigned)blocks), dim3(FS_BLOCK), 0, s, y, seg_x, batch_y, Nq, num_clouds,
                       radius * radius, max_nn, plan.G, w.info, w.cell_start, w.sorted_pt, idx, dist2, count);
    return check_launch();
}

TP3D_EXPORT int tp3d_fpfh_normals_f32(const float *pos, const int32_t *idx, const int32_t *count, int64_t N, int max_nn,
                                      const float *viewpoint, float *normals, void *stream)
{
    if (N < 0 || max_nn <= 0) return TP3D_E_BADARG;
    if (N == 0) return TP3D_OK;
    if (!pos || !idx || !count || !normals) return TP3D_E_BADARG;
    const int64_t blocks = (N + FN_BLOCK - 1) / FN_BLOCK;
    if (blocks > 0x7fffffff) return TP3D_E_TOOBIG;
    hipLaunchKernelGGL(fpfh_normals_kernel, dim3((unsigned)blocks), dim3(FN_BLOCK), 0, (hipStream_t)stream, pos, idx, count,
                       N, max_nn, viewpoint, normals);
    return check_launch();
}

TP3D_EXPORT int tp3d_spfh_counts_f32(const float *pos, const float *normals, const int32_t *idx, const int32_t *count,
                                     int64_t N, int max_nn, int32_t *counts, void *stream)
{
    if (N < 0 || max_nn <= 0) return TP3D_E_BADARG;
    if (N == 0) return TP3D_OK;
    if (!pos || !normals || !idx || !count || !counts) return TP3D_E_BADARG;
    const int64_t blocks = (N + FS_WAVES - 1) / FS_WAVES;
    if (blocks > 0x7fffffff) return TP3D_E_TOOBIG;
    hipLaunchKernelGGL(spfh_counts_kernel, dim3((unsigned)blocks), dim3(FS_BLOCK), 0, (hipStream_t)stream, pos, normals, idx,
                       count, N, max_nn, counts);
    return check_launch();
}

TP3D_EXPORT int tp3d_fpfh_f32(const float *pos, const int32_t *idx, const int32_t *count, const int32_t *counts,
                              const int64_t *rows, int64_t R, int64_t N, int max_nn, double *out64, float *out32,
                              void *stream)
{
    if (N < 0 || R < 0 || max_nn <= 0) return TP3D_E_BADARG;
    if (R == 0) return TP3D_OK;
    if (!pos || !idx || !count || !counts || (!out64 && !out32)) return TP3D_E_BADARG;
    const int64_t blocks = (3 * R + FB_BLOCK - 1) / FB_BLOCK;
    if (blocks > 0x7fffffff) return TP3D_E_TOOBIG;
    hipLaunchKernelGGL(fpfh_rows_kernel, dim3((unsigned)blocks), dim3(FB_BLOCK), 0,
                       (hipStream_t)stream, pos, idx, count, counts, rows, R, N, max_nn, out64, out32);
    return check_launch();
}
