// Sparse voxel convolution (the SparseConv3d family of torch_points3d/modules/SparseConv3d over torchsparse):
// coordinate sets, kernel maps, one gather-GEMM for the four products and the weight gradient.
//
// A coordinate set is (keys, rows, meta): `keys` the sorted 64-bit keys of its voxels, `rows[slot]` the row of the
// tensor that owns the key in that slot, `meta` 16 ints on the device: [min x,y,z | max x,y,z | max batch | bad flags |
// row count].  key = ((batch * EX + x - minx) * EY + y - miny) * EZ + z - minz with the extents of the set's own
// bounding box, so keys ascend in (batch, x, y, z) -- the row order of a stride-2 output set.
//
// A kernel map is two int32 tables built here by binary search: forward (Nout, K) = input row at coord(o) + offset_k,
// inverse (Nin, K) = output row o with coord(o) + offset_k == coord(i); -1 where absent.  Offsets: odd k {-(k/2)..k/2} * ts
// (k = 3 or 5), k = 2 {0,1} * ts per axis, x slowest, z fastest.  Every product is y[r] = sum_k x[table[r][k]] . W[k]: gathered rows and
// the W[k] tile are staged in LDS, contracted with v_mfma_f32_16x16x4_f32, accumulators stay in registers across k;
// nothing of size N*K*C is written to memory.  The gather also range-checks every index against the source row count.
// No float atomics: forward, dX and dW are bit-reproducible.
#include "sorted_keys.h"

namespace tp3d {

constexpr int SP_BLOCK = SK_BLOCK;
constexpr int SP_COORD_LIMIT = 1 << 18;  // |coord| below this at tensor stride 1
constexpr int SP_BATCH_LIMIT = 1 << 9;   // batch below this (tp3d_sparse_set_build_i32)
constexpr int SP_CLOUD_LIMIT_MAX = 1 << 24;  // largest bound tp3d_sparse_set_build_clouds_i32 takes
constexpr int SP_META = 16;
constexpr int SP_KMAX = 125;  // offsets of the widest kernel served (5^3)
constexpr int SP_BAD_RANGE = 1, SP_BAD_DUP = 2, SP_BAD_SPAN = 4;

typedef float sp_f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int sp_floor_to(int c, int m)
{
    // floor(c / m) * m for m > 0 (C++ '/' truncates)
    int q = c / m;
    if (c % m != 0 && c < 0) --q;
    return q * m;
}

// The one coordinate rule (sparseconv.py check_coords_host): a voxel of tensor stride ts covers [c, c + ts) per
// axis and is accepted when that interval holds a coordinate of (-2^18, 2^18).  At ts = 1 that is |c| < 2^18; a coarser
// set may hold -2^18 itself, the floor of -(2^18 - 1), so the floor of an accepted voxel is accepted at the coarser stride.
__device__ __forceinline__ bool sp_coord_ok(int c, int ts) { return c < SP_COORD_LIMIT && c > -SP_COORD_LIMIT - ts + 1; }

// bounding box of the (floored) coordinates + the range flag
__global__ __launch_bounds__(SP_BLOCK) void sp_bounds_kernel(const int *__restrict__ coords, int64_t N, int ts, int down,
                                                              int cloud_limit, int *__restrict__ meta)
{
    int v[8] = {0x7fffffff, 0x7fffffff, 0x7fffffff, (int)0x80000000, (int)0x80000000, (int)0x80000000, (int)0x80000000, 0};
    for (int64_t i = (int64_t)blockIdx.x * SP_BLOCK + threadIdx.x; i < N; i += (int64_t)gridDim.x * SP_BLOCK) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            int c = coords[i * 4 + a];
            if (!sp_coord_ok(c, ts)) {
                v[7] |= SP_BAD_RANGE;
                c = 0;
            }
            if (down > 0) c = sp_floor_to(c, down);
            v[a] = min(v[a], c);
            v[3 + a] = max(v[3 + a], c);
        }
        int b = coords[i * 4 + 3];
        if (b < 0 || b >= cloud_limit) {
            v[7] |= SP_BAD_RANGE;
            b = 0;
        }
        v[6] = max(v[6], b);
    }
    box8_reduce_to(v, meta);
}

// key of (x, y, z, b) in the set described by meta; false when the voxel lies outside the set's bounding box
__device__ __forceinline__ bool sp_key(const int *__restrict__ meta, int x, int y, int z, int b, unsigned long long *key)
{
    const int minx = meta[0], miny = meta[1], minz = meta[2];
    const int maxx = meta[3], maxy = meta[4], maxz = meta[5], maxb = meta[6];
    if (x < minx || x > maxx || y < miny || y > maxy || z < minz || z > maxz || b < 0 || b > maxb) return false;
    const unsigned long long ex = (unsigned long long)((int64_t)maxx - minx + 1);
    const unsigned long long ey = (unsigned long long)((int64_t)maxy - miny + 1);
    const unsigned long long ez = (unsigned long long)((int64_t)maxz - minz + 1);
    *key = (((unsigned long long)b * ex + (unsigned long long)(x - minx)) * ey + (unsigned long long)(y - miny)) * ez +
           (unsigned long long)(z - minz);
    return true;
}

__global__ __launch_bounds__(SP_BLOCK) void sp_key_kernel(const int *__restrict__ coords, int64_t N, int ts, int down,
                                                           int cloud_limit, int *__restrict__ meta,
                                                           unsigned long long *__restrict__ keys,
                                                           unsigned int *__restrict__ vals)
{
    const int64_t i = (int64_t)blockIdx.x * SP_BLOCK + threadIdx.x;
    if (i == 0) {
        // extents <= 2^19 each, batches <= cloud_limit <= 2^24: the product passes 2^63 for a box no real scene has (2^9
        // clouds) or for many clouds over a wide box (4e18 / 2^24 clouds = a cube of 6 000 cells) -- flag it
        const double total = ((double)meta[3] - meta[0] + 1.0) * ((double)meta[4] - meta[1] + 1.0) *
                             ((double)meta[5] - meta[2] + 1.0) * ((double)meta[6] + 1.0);
        if (total >= 4.0e18) atomicOr(&meta[7], SP_BAD_SPAN);
    }
    if (i >= N) return;
    int c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        c[a] = coords[i * 4 + a];
        if (!sp_coord_ok(c[a], ts)) c[a] = 0;  // (flagged by the bounds pass)
        if (down > 0) c[a] = sp_floor_to(c[a], down);
    }
    int b = coords[i * 4 + 3];
    if (b < 0 || b >= cloud_limit) b = 0;
    unsigned long long key = 0;
    (void)sp_key(meta, c[0], c[1], c[2], b, &key);
    keys[i] = key;
    vals[i] = (unsigned int)i;
}

// input set: rows of the sorted slots, duplicate flag (adjacent equal keys)
__global__ __launch_bounds__(SP_BLOCK) void sp_input_finish_kernel(const unsigned long long *__restrict__ keys,
                                                                    const unsigned int *__restrict__ vals, int64_t N,
                                                                    int *__restrict__ rows, int *__restrict__ meta)
{
    const int64_t i = (int64_t)blockIdx.x * SP_BLOCK + threadIdx.x;
    if (i >= N) return;
    rows[i] = (int)vals[i];
    if (i > 0 && keys[i] == keys[i - 1]) atomicOr(&meta[7], SP_BAD_DUP);
    if (i == 0) meta[8] = (int)N;
}

// stride-2 set: the first slot of every run of equal keys writes the voxel (keys ascend = (batch, x, y, z) order)
__global__ __launch_bounds__(SP_BLOCK) void sp_compact_kernel(const unsigned long long *__restrict__ keys,
                                                               const unsigned int *__restrict__ vals,
                                                               const int *__restrict__ cid, const int *__restrict__ coords,
                                                               int64_t N, int ts, int down,
                                                               unsigned long long *__restrict__ keys_out,
                                                               int *__restrict__ rows_out, int *__restrict__ coords_out,
                                                               int *__restrict__ meta)
{
    const int64_t i = (int64_t)blockIdx.x * SP_BLOCK + threadIdx.x;
    if (i >= N) return;
    const int c = cid[i];
    if (i == 0 || cid[i - 1] != c) {
        const int64_t p = vals[i];
        keys_out[c] = keys[i];
        rows_out[c] = c;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            int v = coords[p * 4 + a];
            if (!sp_coord_ok(v, ts)) v = 0;
            coords_out[(int64_t)c * 4 + a] = sp_floor_to(v, down);
        }
        coords_out[(int64_t)c * 4 + 3] = coords[p * 4 + 3];
    }
    if (i == N - 1) meta[8] = c + 1;
}

// table[q][k] = row of the set's voxel at coord(q) + sign * offset_k * step, or -1
__global__ __launch_bounds__(SP_BLOCK) void sp_kmap_kernel(const int *__restrict__ qcoords, int64_t Nq, int ksize, int step,
                                                            int sign, const unsigned long long *__restrict__ keys,
                                                            const int *__restrict__ rows, const int *__restrict__ meta,
                                                            int64_t Ns, int *__restrict__ table)
{
    const int K = ksize * ksize * ksize;
    const int64_t t = (int64_t)blockIdx.x * SP_BLOCK + threadIdx.x;
    if (t >= Nq * K) return;
    const int64_t q = t / K;
    const int k = (int)(t - q * K);
    const int lo_off = (ksize & 1) ? -(ksize / 2) : 0;
    const int ox = (k / (ksize * ksize) + lo_off) * step * sign;
    const int oy = ((k / ksize) % ksize + lo_off) * step * sign;
    const int oz = (k % ksize + lo_off) * step * sign;
    unsigned long long key;
    int found = -1;
    if (sp_key(meta, qcoords[q * 4 + 0] + ox, qcoords[q * 4 + 1] + oy, qcoords[q * 4 + 2] + oz, qcoords[q * 4 + 3], &key)) {
        const int64_t lo = lower_bound_u64(keys, Ns, key);
        if (lo < Ns && keys[lo] == key) {
            const int r = rows[lo];
            found = (r >= 0 && r < Ns) ? r : -1;
        }
    }
    table[t] = found;
}

// stride 1: inverse[i][k] = forward[i][K - 1 - k] (coord(o) + off_k == coord(i)  <=>  o = row at coord(i) - off_k, and the
// offsets of an odd kernel mirror under k -> K - 1 - k)
__global__ __launch_bounds__(SP_BLOCK) void sp_mirror_kernel(const int *__restrict__ fwd, int64_t N, int K, int *__restrict__ inv)
{
    const int64_t t = (int64_t)blockIdx.x * SP_BLOCK + threadIdx.x;
    if (t >= N * K) return;
    const int64_t q = t / K;
    const int k = (int)(t - q * K);
    inv[t] = fwd[q * K + (K - 1 - k)];
}

// ------------------------------------------------------------------------------------------------------- gather-GEMM
constexpr int SP_TM = 64;   // output rows per workgroup (16 per wave)
constexpr int SP_TN = 64;   // output columns per workgroup
constexpr int SP_KC = 32;   // input channels per LDS stage
constexpr int SP_XLD = SP_KC + 1;
constexpr int SP_WLD = SP_TN + 16;

// y[r][co] = sum_k sum_ci x[table[r][k]][ci] * W[k * wk + ci * wci + co * wco]
__global__ __launch_bounds__(SP_BLOCK) void sp_conv_mfma_kernel(const float *__restrict__ x, const int *__restrict__ table,
                                                                 const float *__restrict__ W, int64_t Nout, int64_t Nsrc, int K,
                                                                 int Cin, int Cout, int64_t wk, int wci, int wco,
                                                                 float *__restrict__ y)
{
    __shared__ float s_x[SP_TM * SP_XLD];
    __shared__ float s_w[SP_KC * SP_WLD];
    __shared__ int s_idx[SP_TM];
    __shared__ int s_any[SP_BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * SP_TM;
    const int c0 = blockIdx.y * SP_TN;
    sp_f32x4 acc[SP_TN / 16];
#pragma unroll
    for (int b = 0; b < SP_TN / 16; ++b) acc[b] = (sp_f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    const bool vec = (Cin & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;  // float4 rows
    for (int k = 0; k < K; ++k) {
        // this offset's source rows of the tile; skip it when no row has one (most offsets on a surface)
        int idx = -1;
        if (tid < SP_TM) {
            const int64_t r = r0 + tid;
            if (r < Nout) idx = table[r * K + k];
            if (idx < 0 || idx >= Nsrc) idx = -1;
            s_idx[tid] = idx;
        }
        const unsigned long long any = __ballot(idx >= 0);
        if (lane == 0) s_any[wave] = any != 0ull;
        __syncthreads();
        const bool has = (s_any[0] | s_any[1] | s_any[2] | s_any[3]) != 0;  // (workgroup-uniform)
        if (has) {
            for (int ci0 = 0; ci0 < Cin; ci0 += SP_KC) {
                // gathered rows -> s_x[row][ci - ci0]
                if (vec) {
                    for (int e = tid; e < SP_TM * (SP_KC / 4); e += SP_BLOCK) {
                        const int row = e / (SP_KC / 4), c4 = (e % (SP_KC / 4)) * 4;
                        const int src = s_idx[row];
                        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                        if (src >= 0 && ci0 + c4 < Cin) v = *reinterpret_cast<const float4 *>(x + (int64_t)src * Cin + ci0 + c4);
                        float *d = s_x + row * SP_XLD + c4;
                        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
                    }
                } else {
                    for (int e = tid; e < SP_TM * SP_KC; e += SP_BLOCK) {
                        const int row = e / SP_KC, c = e % SP_KC;
                        const int src = s_idx[row];
                        s_x[row * SP_XLD + c] = (src >= 0 && ci0 + c < Cin) ? x[(int64_t)src * Cin + ci0 + c] : 0.0f;
                    }
                }
                // W[k] tile -> s_w[ci - ci0][co - c0]; the fastest thread index follows the unit stride
                if (wco == 1) {
                    for (int e = tid; e < SP_KC * SP_TN; e += SP_BLOCK) {
                        const int ci = e / SP_TN, co = e % SP_TN;
                        s_w[ci * SP_WLD + co] = (ci0 + ci < Cin && c0 + co < Cout)
                                                    ? W[k * wk + (int64_t)(ci0 + ci) * wci + (int64_t)(c0 + co) * wco] : 0.0f;
                    }
                } else {
                    for (int e = tid; e < SP_KC * SP_TN; e += SP_BLOCK) {
                        const int co = e / SP_KC, ci = e % SP_KC;
                        s_w[ci * SP_WLD + co] = (ci0 + ci < Cin && c0 + co < Cout)
                                                    ? W[k * wk + (int64_t)(ci0 + ci) * wci + (int64_t)(c0 + co) * wco] : 0.0f;
                    }
                }
                __syncthreads();
                const float *xa = s_x + (16 * wave + (lane & 15)) * SP_XLD + (lane >> 4);
                const float *wb = s_w + (lane >> 4) * SP_WLD + (lane & 15);
#pragma unroll
                for (int kk = 0; kk < SP_KC; kk += 4) {
                    const float a = xa[kk];
#pragma unroll
                    for (int b = 0; b < SP_TN / 16; ++b)
                        acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wb[kk * SP_WLD + 16 * b], acc[b], 0, 0, 0);
                }
                __syncthreads();
            }
        } else {
            __syncthreads();  // s_idx / s_any are rewritten by the next offset
        }
    }
    // D[row = 4 (lane >> 4) + j][col = lane & 15]
#pragma unroll
    for (int b = 0; b < SP_TN / 16; ++b) {
        const int co = c0 + 16 * b + (lane & 15);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t r = r0 + 16 * wave + 4 * (lane >> 4) + j;
            if (r < Nout && co < Cout) y[r * Cout + co] = acc[b][j];
        }
    }
}

// narrow route (Cin <= 4, the first layer): one thread per output element, plain FMA
__global__ __launch_bounds__(SP_BLOCK) void sp_conv_narrow_kernel(const float *__restrict__ x, const int *__restrict__ table,
                                                                   const float *__restrict__ W, int64_t Nout, int64_t Nsrc,
                                                                   int K, int Cin, int Cout, int64_t wk, int wci, int wco,
                                                                   float *__restrict__ y)
{
    const int64_t t = (int64_t)blockIdx.x * SP_BLOCK + threadIdx.x;
    if (t >= Nout * Cout) return;
    const int64_t r = t / Cout;
    const int co = (int)(t - r * Cout);
    float acc = 0.0f;
    for (int k = 0; k < K; ++k) {
        const int idx = table[r * K + k];
        if (idx < 0 || idx >= Nsrc) continue;
        const float *xr = x + (int64_t)idx * Cin;
        const float *w = W + k * wk + (int64_t)co * wco;
        for (int ci = 0; ci < Cin; ++ci) acc = __builtin_fmaf(xr[ci], w[(int64_t)ci * wci], acc);
    }
    y[t] = acc;
}

// ----------------------------------------------------------------------------------------------------- weight gradient
constexpr int SP_WG_ROWS = 1024;  // least rows per chunk
constexpr int SP_WG_MAX_CHUNKS = 32;
constexpr int SP_WG_STEP = 32;  // rows per LDS stage
constexpr int SP_GLD = 64 + 16;

inline int64_t sp_wgrad_chunk_rows(int64_t N)
{
    int64_t rows = (N + SP_WG_MAX_CHUNKS - 1) / SP_WG_MAX_CHUNKS;
    rows = (rows + SP_WG_STEP - 1) / SP_WG_STEP * SP_WG_STEP;
    return rows < SP_WG_ROWS ? SP_WG_ROWS : rows;
}

// out[chunk][k][ci][co] = sum over the chunk's rows r (ascending) of x[table[r][k]][ci] * dy[r][co]
// grid: (chunks, K, Cin tiles * Cout tiles); a wave owns 16 ci x 64 co
__global__ __launch_bounds__(SP_BLOCK) void sp_wgrad_kernel(const float *__restrict__ x, const float *__restrict__ dy,
                                                             const int *__restrict__ table, int64_t N, int64_t Nsrc, int K,
                                                             int Cin, int Cout, int64_t chunk_rows, float *__restrict__ out)
{
    __shared__ float s_x[SP_WG_STEP * SP_GLD];
    __shared__ float s_g[SP_WG_STEP * SP_GLD];
    __shared__ int s_idx[SP_WG_STEP];
    __shared__ int s_any;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = blockIdx.y;
    const int co_tiles = (Cout + 63) / 64;
    const int ci0 = (blockIdx.z / co_tiles) * 64, co0 = (blockIdx.z % co_tiles) * 64;
    const int64_t rb = (int64_t)blockIdx.x * chunk_rows;
    const int64_t re = min(N, rb + chunk_rows);
    sp_f32x4 acc[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[b] = (sp_f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    for (int64_t r0 = rb; r0 < re; r0 += SP_WG_STEP) {
        if (tid < 64) {
            int idx = -1;
            if (tid < SP_WG_STEP && r0 + tid < re) idx = table[(r0 + tid) * K + k];
            if (idx < 0 || idx >= Nsrc) idx = -1;
            if (tid < SP_WG_STEP) s_idx[tid] = idx;
            const unsigned long long any = __ballot(idx >= 0);
            if (tid == 0) s_any = any != 0ull;
        }
        __syncthreads();
        if (s_any) {  // (workgroup-uniform) rows without this offset contribute nothing
            for (int e = tid; e < SP_WG_STEP * 64; e += SP_BLOCK) {
                const int row = e >> 6, c = e & 63;
                const int src = s_idx[row];
                s_x[row * SP_GLD + c] = (src >= 0 && ci0 + c < Cin) ? x[(int64_t)src * Cin + ci0 + c] : 0.0f;
                s_g[row * SP_GLD + c] = (src >= 0 && co0 + c < Cout) ? dy[(r0 + row) * Cout + co0 + c] : 0.0f;
            }
            __syncthreads();
            // A[row = ci][kk = r] = s_x[r][ci], B[kk = r][col = co] = s_g[r][co]
            const float *xa = s_x + (lane >> 4) * SP_GLD + 16 * wave + (lane & 15);
            const float *gb = s_g + (lane >> 4) * SP_GLD + (lane & 15);
#pragma unroll
            for (int kk = 0; kk < SP_WG_STEP; kk += 4) {
                const float a = xa[kk * SP_GLD];
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, gb[kk * SP_GLD + 16 * b], acc[b], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    float *o = out + ((int64_t)blockIdx.x * K + k) * (int64_t)Cin * Cout;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int co = co0 + 16 * b + (lane & 15);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ci = ci0 + 16 * wave + 4 * (lane >> 4) + j;
            if (ci < Cin && co < Cout) o[(int64_t)ci * Cout + co] = acc[b][j];
        }
    }
}

// ------------------------------------------------------------------------- wide first layer (Cin <= 4, 27 < K <= 125)
// A 5^3 kernel on a scanned surface finds a small part of its 125 offsets.  A wave reads a row's table entries with two
// coalesced loads, compacts the present ones (ascending k) into its own LDS list with a ballot and loops over the hits only.
constexpr int SPW_HITS = 128;            // hit slots per row (K <= 125)
constexpr int SPW_CT = 32;               // channels per pass: the lanes of a half-wave
constexpr int SPW_MAX_CIN = 4;
constexpr int SPW_LDS_MAX = 160 * 1024;  // LDS of a CU
constexpr int SPW_FWD_ROWS = 2 * (SP_BLOCK / 64);  // rows per workgroup step: two per wave
constexpr int SPW_FWD_MAX_BLOCKS = 512;
constexpr int SPW_WG_ROWS = 128;         // least rows per weight-gradient chunk
constexpr int SPW_WG_MAX_CHUNKS = 256;
constexpr int SPW_WG_MAX_WAVES = 4;

// the wave's own LDS writes have landed (each wave owns its hit lists and accumulators)
__device__ __forceinline__ void sp_wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// hk[0..n), hi[0..n) = the offsets k (ascending) of row r with a source row in [0, Nsrc), and those rows; returns n
// (wave-uniform).  r < 0: no row.
__device__ __forceinline__ int spw_compact_row(const int *__restrict__ table, int64_t r, int K, int64_t Nsrc, int lane, int *hk,
                                               int *hi)
{
    int t0 = -1, t1 = -1;
    if (r >= 0) {
        const int *row = table + r * K;
        if (lane < K) t0 = row[lane];
        if (lane + 64 < K) t1 = row[lane + 64];
    }
    if (t0 < 0 || t0 >= Nsrc) t0 = -1;
    if (t1 < 0 || t1 >= Nsrc) t1 = -1;
    const unsigned long long m0 = __ballot(t0 >= 0), m1 = __ballot(t1 >= 0);
    const int n0 = __popcll(m0);
    if (t0 >= 0) {
        const int p = lanes_below(m0);
        hk[p] = lane;
        hi[p] = t0;
    }
    if (t1 >= 0) {
        const int p = n0 + lanes_below(m1);
        hk[p] = lane + 64;
        hi[p] = t1;
    }
    return n0 + __popcll(m1);
}

// y[r][co] = sum over the present k (ascending), ci (ascending) of x[table[r][k]][ci] * W[k][ci][co].  W is staged in LDS
// once per workgroup; a half-wave owns a row, its lanes are 32 output channels (wider layers take further passes).
__global__ __launch_bounds__(SP_BLOCK) void sp_conv_wide_kernel(const float *__restrict__ x, const int *__restrict__ table,
                                                                 const float *__restrict__ W, int64_t Nout, int64_t Nsrc, int K,
                                                                 int Cin, int Cout, float *__restrict__ y)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, c = lane & 31;
    const int KCC = K * Cin * Cout;
    float *s_w = reinterpret_cast<float *>(smem);
    int *s_hit = reinterpret_cast<int *>(s_w + KCC) + wave * 4 * SPW_HITS;  // [row of the wave][k | source row][slot]
    for (int e = tid; e < KCC; e += SP_BLOCK) s_w[e] = W[e];
    __syncthreads();
    for (int64_t base = (int64_t)blockIdx.x * SPW_FWD_ROWS; base < Nout; base += (int64_t)gridDim.x * SPW_FWD_ROWS) {
        const int64_t r0 = base + 2 * wave;
        const int n0 = spw_compact_row(table, r0 < Nout ? r0 : -1, K, Nsrc, lane, s_hit, s_hit + SPW_HITS);
        const int n1 = spw_compact_row(table, r0 + 1 < Nout ? r0 + 1 : -1, K, Nsrc, lane, s_hit + 2 * SPW_HITS, s_hit + 3 * SPW_HITS);
        sp_wave_lds_sync();
        const int64_t r = r0 + half;
        const int n = half ? n1 : n0;
        const int *hk = s_hit + 2 * half * SPW_HITS, *hi = hk + SPW_HITS;
        for (int co = c; co < Cout; co += SPW_CT) {
            float acc = 0.0f;
            for (int h = 0; h < n; ++h) {
                const float *xr = x + (int64_t)hi[h] * Cin;
                const float *w = s_w + hk[h] * Cin * Cout + co;
                for (int ci = 0; ci < Cin; ++ci) acc = __builtin_fmaf(xr[ci], w[ci * Cout], acc);
            }
            if (r < Nout) y[r * Cout + co] = acc;
        }
        sp_wave_lds_sync();  // the next step rewrites the hit lists
    }
}

inline int64_t spw_wgrad_chunk_rows(int64_t N)
{
    int64_t rows = (N + SPW_WG_MAX_CHUNKS - 1) / SPW_WG_MAX_CHUNKS;
    rows = (rows + 7) / 8 * 8;
    return rows < SPW_WG_ROWS ? SPW_WG_ROWS : rows;
}

// waves per workgroup of the wide weight gradient: each owns K * Cin * Cout accumulators and one hit list in LDS; 0 when
// not even one fits
inline int spw_wgrad_waves(int K, int Cin, int Cout)
{
    const int64_t per_wave = (int64_t)K * Cin * Cout * 4 + 2 * SPW_HITS * 4;
    const int64_t waves = SPW_LDS_MAX / per_wave;
    return (int)(waves > SPW_WG_MAX_WAVES ? SPW_WG_MAX_WAVES : waves);
}

// out[chunk][k][ci][co] = sum over the chunk's rows of x[table[r][k]][ci] * dy[r][co].  One workgroup per chunk; a wave
// takes a contiguous run of the chunk's rows in ascending order and adds into its own accumulators in LDS: lanes are 32
// output channels x two hit slots, so a step updates two different k and no two lanes share an address.  The waves'
// accumulators are then summed in wave order.  Every dy row and table row is read once; no atomics.
__global__ __launch_bounds__(64 * SPW_WG_MAX_WAVES) void sp_wgrad_wide_kernel(const float *__restrict__ x, const float *__restrict__ dy, const int *__restrict__ table,
                                     int64_t N, int64_t Nsrc, int K, int Cin, int Cout, int64_t chunk_rows,
                                     float *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, slot = lane >> 5, c = lane & 31;
    const int waves = blockDim.x >> 6;
    const int KCC = K * Cin * Cout;
    float *s_acc = reinterpret_cast<float *>(smem);
    float *acc = s_acc + (int64_t)wave * KCC;
    int *hk = reinterpret_cast<int *>(s_acc + (int64_t)waves * KCC) + wave * 2 * SPW_HITS, *hi = hk + SPW_HITS;
    for (int e = lane; e < KCC; e += 64) acc[e] = 0.0f;
    const int64_t rb = (int64_t)blockIdx.x * chunk_rows;
    const int64_t re = min(N, rb + chunk_rows);
    const int64_t per = (re - rb + waves - 1) / waves;
    const int64_t wb = rb + wave * per, we = min(re, wb + per);
    sp_wave_lds_sync();
    for (int64_t r = wb; r < we; ++r) {
        const int n = spw_compact_row(table, r, K, Nsrc, lane, hk, hi);
        sp_wave_lds_sync();
        for (int co = c; co < Cout; co += SPW_CT) {
            const float g = dy[r * Cout + co];
            for (int h = slot; h < n; h += 2) {
                const float *xr = x + (int64_t)hi[h] * Cin;
                float *a = acc + hk[h] * Cin * Cout + co;
                for (int ci = 0; ci < Cin; ++ci) a[ci * Cout] = __builtin_fmaf(xr[ci], g, a[ci * Cout]);
            }
        }
        sp_wave_lds_sync();  // the next row rewrites the hit list and may update the same accumulators from other lanes
    }
    __syncthreads();
    float *o = out + (int64_t)blockIdx.x * KCC;
    for (int e = tid; e < KCC; e += blockDim.x) {
        float t = s_acc[e];
        for (int w = 1; w < waves; ++w) t += s_acc[(int64_t)w * KCC + e];
        o[e] = t;
    }
}

// the sort covers the bits the key can have: the host knows the hard limits only (3 * 19 + 9 bits, or + 24 with a cloud
// bound of its own, would pass 64; the span flag rejects such a box), so 63
constexpr unsigned SP_KEY_BITS = 63;

}  // namespace tp3d

using namespace tp3d;

TP3D_EXPORT size_t tp3d_sparse_workspace_bytes(int64_t N)
{
    if (N <= 0 || N >= 0x7fffffff) return 0;
    return carve_sort_workspace(nullptr, N, true, true).bytes;
}

TP3D_EXPORT int tp3d_sparse_set_build_clouds_i32(const int32_t *coords, int64_t N, int ts, int down, int cloud_limit,
                                                 int64_t *keys_out, int32_t *rows_out, int32_t *coords_out, int32_t *meta,
                                                 void *workspace, size_t workspace_bytes, void *stream)
{
    if (cloud_limit < 1 || cloud_limit > SP_CLOUD_LIMIT_MAX) return TP3D_E_BADARG;
    if (N <= 0 || N >= 0x7fffffff || ts < 1 || ts >= SP_COORD_LIMIT || down < 0 || down >= SP_COORD_LIMIT || !coords || !keys_out || !rows_out || !meta ||
        !workspace || (down > 0 && !coords_out))
        return TP3D_E_BADARG;
    SortWorkspace w = carve_sort_workspace(workspace, N, true, true);
    if (workspace_bytes < w.bytes) return TP3D_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    const unsigned blocks = (unsigned)((N + SP_BLOCK - 1) / SP_BLOCK);
    hipLaunchKernelGGL(box_init_kernel, dim3(1), dim3(64), 0, s, meta, SP_META);
    if (int rc = check_launch()) return rc;
    hipLaunchKernelGGL(sp_bounds_kernel, dim3(blocks > 1024 ? 1024 : blocks), dim3(SP_BLOCK), 0, s, coords, N, ts, down,
                       cloud_limit, meta);
    if (int rc = check_launch()) return rc;
    hipLaunchKernelGGL(sp_key_kernel, dim3(blocks), dim3(SP_BLOCK), 0, s, coords, N, ts, down, cloud_limit, meta, w.keys_in,
                       w.vals_in);
    if (int rc = check_launch()) return rc;
    unsigned long long *sorted = down > 0 ? w.keys_out : reinterpret_cast<unsigned long long *>(keys_out);
    if (int rc = sort_pairs_u64_u32(w.tmp, w.tmp_bytes, w.keys_in, sorted, w.vals_in, w.vals_out, N, SP_KEY_BITS, s)) return rc;
    if (down == 0) {
        hipLaunchKernelGGL(sp_input_finish_kernel, dim3(blocks), dim3(SP_BLOCK), 0, s, sorted, w.vals_out, N, rows_out, meta);
        return check_launch();
    }
    if (int rc = run_ids(sorted, N, w, s)) return rc;
    hipLaunchKernelGGL(sp_compact_kernel, dim3(blocks), dim3(SP_BLOCK), 0, s, sorted, w.vals_out, w.cid, coords, N, ts, down,
                       reinterpret_cast<unsigned long long *>(keys_out), rows_out, coords_out, meta);
    return check_launch();
}

TP3D_EXPORT int tp3d_sparse_set_build_i32(const int32_t *coords, int64_t N, int ts, int down, int64_t *keys_out,
                                          int32_t *rows_out, int32_t *coords_out, int32_t *meta, void *workspace,
                                          size_t workspace_bytes, void *stream)
{
    return tp3d_sparse_set_build_clouds_i32(coords, N, ts, down, SP_BATCH_LIMIT, keys_out, rows_out, coords_out, meta, workspace,
                                            workspace_bytes, stream);
}

TP3D_EXPORT int tp3d_sparse_cloud_limit_max(void) { return SP_CLOUD_LIMIT_MAX; }

TP3D_EXPORT int tp3d_sparse_kmap_i32(const int32_t *qcoords, int64_t Nq, int ksize, int step, int sign, const int64_t *keys,
                                     const int32_t *rows, const int32_t *meta, int64_t Ns, int32_t *table, void *stream)
{
    if (Nq <= 0 || Ns <= 0 || ksize < 1 || ksize > 5 || ksize == 4 || step <= 0 || step >= SP_COORD_LIMIT || (sign != 1 && sign != -1) ||
        !qcoords || !keys || !rows || !meta || !table)
        return TP3D_E_BADARG;
    const int K = ksize * ksize * ksize;
    const int64_t blocks = (Nq * K + SP_BLOCK - 1) / SP_BLOCK;
    if (blocks > 0x7fffffff || Nq >= 0x7fffffff || Ns >= 0x7fffffff) return TP3D_E_TOOBIG;
    hipLaunchKernelGGL(sp_kmap_kernel, dim3((unsigned)blocks), dim3(SP_BLOCK), 0, (hipStream_t)stream, qcoords, Nq, ksize, step,
                       sign, reinterpret_cast<const unsigned long long *>(keys), rows, meta, Ns, table);
    return check_launch();
}

TP3D_EXPORT int tp3d_sparse_kmap_mirror_i32(const int32_t *forward, int64_t N, int K, int32_t *inverse, void *stream)
{
    if (N <= 0 || K <= 0 || (K & 1) == 0 || !forward || !inverse) return TP3D_E_BADARG;
    const int64_t blocks = (N * K + SP_BLOCK - 1) / SP_BLOCK;
    if (blocks > 0x7fffffff) return TP3D_E_TOOBIG;
    hipLaunchKernelGGL(sp_mirror_kernel, dim3((unsigned)blocks), dim3(SP_BLOCK), 0, (hipStream_t)stream, forward, N, K, inverse);
    return check_launch();
}

TP3D_EXPORT int tp3d_sparse_conv_f32(const float *x, const int32_t *table, const float *W, int64_t Nout, int64_t Nsrc, int K,
                                     int Cin, int Cout, int w_transposed, float *y, void *stream)
{
    if (Nout < 0 || Nsrc < 0 || K <= 0 || K > SP_KMAX || Cin <= 0 || Cout <= 0) return TP3D_E_BADARG;
    if (Nout == 0) return TP3D_OK;
    if (!table || !W || !y || (Nsrc > 0 && !x)) return TP3D_E_BADARG;
    if (Nout >= 0x7fffffff || Nsrc >= 0x7fffffff) return TP3D_E_TOOBIG;
    // W (K, Cin, Cout), or with w_transposed the layer's (K, Cout, Cin) read as its transpose per offset
    const int64_t wk = (int64_t)Cin * Cout;
    const int wci = w_transposed ? 1 : Cout, wco = w_transposed ? Cin : 1;
    hipStream_t s = (hipStream_t)stream;
    if (Cin <= 4) {
        const int64_t blocks = (Nout * Cout + SP_BLOCK - 1) / SP_BLOCK;
        if (blocks > 0x7fffffff) return TP3D_E_TOOBIG;
        hipLaunchKernelGGL(sp_conv_narrow_kernel, dim3((unsigned)blocks), dim3(SP_BLOCK), 0, s, x, table, W, Nout, Nsrc, K, Cin,
                           Cout, wk, wci, wco, y);
        return check_launch();
    }
    const int64_t row_tiles = (Nout + SP_TM - 1) / SP_TM;
    const int col_tiles = (Cout + SP_TN - 1) / SP_TN;
    if (col_tiles > 65535) return TP3D_E_TOOBIG;
    hipLaunchKernelGGL(sp_conv_mfma_kernel, dim3((unsigned)row_tiles, (unsigned)col_tiles), dim3(SP_BLOCK), 0, s, x, table, W, Nout,
                       Nsrc, K, Cin, Cout, wk, wci, wco, y);
    return check_launch();
}

TP3D_EXPORT int tp3d_sparse_wgrad_chunks(int64_t N, int K, int Cin, int Cout)
{
    if (N <= 0 || K <= 0 || Cin <= 0 || Cout <= 0) return 0;
    const int64_t rows = sp_wgrad_chunk_rows(N);
    return (int)((N + rows - 1) / rows);
}

TP3D_EXPORT size_t tp3d_sparse_wgrad_workspace_floats(int64_t N, int K, int Cin, int Cout)
{
    const int chunks = tp3d_sparse_wgrad_chunks(N, K, Cin, Cout);
    return chunks <= 1 ? 0 : (size_t)chunks * K * Cin * Cout;
}

TP3D_EXPORT int tp3d_sparse_wgrad_f32(const float *x, const float *dy, const int32_t *table, int64_t N, int64_t Nsrc, int K,
                                      int Cin, int Cout, float *dW, float *workspace, size_t workspace_floats, void *stream)
{
    if (N < 0 || Nsrc < 0 || K <= 0 || K > SP_KMAX || Cin <= 0 || Cout <= 0 || !dW) return TP3D_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    const int64_t NK = (int64_t)K * Cin * Cout;
    if (N == 0 || Nsrc == 0) return zero_async(dW, (size_t)NK * sizeof(float), s);
    if (!x || !dy || !table) return TP3D_E_BADARG;
    if (N >= 0x7fffffff || Nsrc >= 0x7fffffff) return TP3D_E_TOOBIG;
    const int chunks = tp3d_sparse_wgrad_chunks(N, K, Cin, Cout);
    const int64_t tiles = (int64_t)((Cin + 63) / 64) * ((Cout + 63) / 64);
    if (tiles > 65535) return TP3D_E_TOOBIG;
    float *out = dW;
    if (chunks > 1) {
        if (!workspace || workspace_floats < tp3d_sparse_wgrad_workspace_floats(N, K, Cin, Cout)) return TP3D_E_BADARG;
        out = workspace;
    }
    hipLaunchKernelGGL(sp_wgrad_kernel, dim3((unsigned)chunks, (unsigned)K, (unsigned)tiles), dim3(SP_BLOCK), 0, s, x, dy, table,
                       N, Nsrc, K, Cin, Cout, sp_wgrad_chunk_rows(N), out);
    if (int rc = check_launch()) return rc;
    if (chunks > 1) return tn_reduce_splits(workspace, chunks, NK, dW, s);
    return TP3D_OK;
}

// ---- wide first layer: Cin <= 4, 27 < K <= 125 ----
static size_t spw_fwd_lds(int K, int Cin, int Cout) { return (size_t)K * Cin * Cout * 4 + (size_t)(SP_BLOCK / 64) * 4 * SPW_HITS * 4; }

static bool spw_shape_ok(int K, int Cin, int Cout)
{
    return K > 27 && K <= SP_KMAX && Cin > 0 && Cin <= SPW_MAX_CIN && Cout > 0 && Cout <= 65536;
}

TP3D_EXPORT int tp3d_sparse_conv_wide_serves(int K, int Cin, int Cout)
{
    return spw_shape_ok(K, Cin, Cout) && spw_fwd_lds(K, Cin, Cout) <= (size_t)SPW_LDS_MAX;
}

TP3D_EXPORT int tp3d_sparse_conv_wide_f32(const float *x, const int32_t *table, const float *W, int64_t Nout, int64_t Nsrc, int K,
                                          int Cin, int Cout, float *y, void *stream)
{
    if (Nout < 0 || Nsrc < 0 || !tp3d_sparse_conv_wide_serves(K, Cin, Cout)) return TP3D_E_BADARG;
    if (Nout == 0) return TP3D_OK;
    if (!table || !W || !y || (Nsrc > 0 && !x)) return TP3D_E_BADARG;
    if (Nout >= 0x7fffffff || Nsrc >= 0x7fffffff) return TP3D_E_TOOBIG;
    int64_t blocks = (Nout + SPW_FWD_ROWS - 1) / SPW_FWD_ROWS;
    if (blocks > SPW_FWD_MAX_BLOCKS) blocks = SPW_FWD_MAX_BLOCKS;
    const size_t lds = spw_fwd_lds(K, Cin, Cout);
    allow_large_dynamic_lds<&sp_conv_wide_kernel>(SPW_LDS_MAX);
    hipLaunchKernelGGL(sp_conv_wide_kernel, dim3((unsigned)blocks), dim3(SP_BLOCK), lds, (hipStream_t)stream, x, table, W, Nout,
                       Nsrc, K, Cin, Cout, y);
    return check_launch();
}

TP3D_EXPORT int tp3d_sparse_wgrad_wide_chunks(int64_t N, int K, int Cin, int Cout)
{
    if (N <= 0 || N >= 0x7fffffff || !spw_shape_ok(K, Cin, Cout) || spw_wgrad_waves(K, Cin, Cout) < 1) return 0;
    const int64_t rows = spw_wgrad_chunk_rows(N);
    return (int)((N + rows - 1) / rows);
}

TP3D_EXPORT size_t tp3d_sparse_wgrad_wide_workspace_floats(int64_t N, int K, int Cin, int Cout)
{
    const int chunks = tp3d_sparse_wgrad_wide_chunks(N, K, Cin, Cout);
    return chunks <= 1 ? 0 : (size_t)chunks * K * Cin * Cout;
}

TP3D_EXPORT int tp3d_sparse_wgrad_wide_f32(const float *x, const float *dy, const int32_t *table, int64_t N, int64_t Nsrc, int K,
                                           int Cin, int Cout, float *dW, float *workspace, size_t workspace_floats, void *stream)
{
    if (N < 0 || Nsrc < 0 || !spw_shape_ok(K, Cin, Cout) || !dW) return TP3D_E_BADARG;
    const int waves = spw_wgrad_waves(K, Cin, Cout);
    if (waves < 1) return TP3D_E_BADARG;  // the accumulators of one wave do not fit the LDS: the generic kernel serves it
    hipStream_t s = (hipStream_t)stream;
    const int64_t NK = (int64_t)K * Cin * Cout;
    if (N == 0 || Nsrc == 0) return zero_async(dW, (size_t)NK * sizeof(float), s);
    if (!x || !dy || !table) return TP3D_E_BADARG;
    if (N >= 0x7fffffff || Nsrc >= 0x7fffffff) return TP3D_E_TOOBIG;
    const int chunks = tp3d_sparse_wgrad_wide_chunks(N, K, Cin, Cout);
    float *out = dW;
    if (chunks > 1) {
        if (!workspace || workspace_floats < (size_t)chunks * NK) return TP3D_E_BADARG;
        out = workspace;
    }
    const size_t lds = (size_t)waves * ((size_t)NK * 4 + 2 * SPW_HITS * 4);
    allow_large_dynamic_lds<&sp_wgrad_wide_kernel>(SPW_LDS_MAX);
    hipLaunchKernelGGL(sp_wgrad_wide_kernel, dim3((unsigned)chunks), dim3(64 * waves), lds, s, x, dy, table, N, Nsrc, K, Cin, Cout,
                       spw_wgrad_chunk_rows(N), out);
    if (int rc = check_launch()) return rc;
    if (chunks > 1) return tn_reduce_splits(workspace, chunks, NK, dW, s);
    return TP3D_OK;
}
