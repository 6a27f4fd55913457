// Message-passing PointNet++ (PointConv over a radius neighbourhood of varying size, per-cloud global pool):
// neighbour table -> edge list, edge rows, segmented max forward / backward.
//
// Reference contract: torch_points3d/modules/pointnet2/message_passing.py:9-31 (SAModule: torch_geometric `radius`
// + `PointConv`), core/base_conv/message_passing.py:132-151 (GlobalBaseModule: `global_max_pool`).
//
// All four are streams over (edges, ld) rows: a wave owns one query / segment, its lanes walk the row-major
// elements of that query's edges, so every store (and the feature loads of one support row) is contiguous.
// The launch shape, the run bounds and the element walk are edge_run.h's.
#include "edge_run.h"

namespace tp3d {

// ---- table -> edges ---------------------------------------------------------------------------------------------
// counts[i + 1] = number of slots >= 0 in row i of the -1 padded table (one wave per row, 64 slots per step)
__global__ __launch_bounds__(ER_BLOCK) void table_count_kernel(const int64_t *__restrict__ table, int64_t Nq, int W,
                                                                int64_t *__restrict__ edge_start)
{
    const int64_t i = (int64_t)blockIdx.x * ER_WAVES + threadIdx.x / kWave;
    if (i >= Nq) return;
    const int lane = lane_id();
    int n = 0;
    for (int s0 = 0; s0 < W; s0 += kWave) {
        const int s = s0 + lane;
        const bool hit = s < W && table[i * W + s] >= 0;
        n += __popcll(__ballot(hit));
    }
    if (lane == 0) edge_start[i + 1] = n;
    if (i == 0 && lane == 0) edge_start[0] = 0;
}

// in-place inclusive scan of v[1 .. n] by ONE workgroup (v[0] = 0 stays): tiles of 4 * 1024 values, a carry between
// the tiles.  n is the number of queries of a batch (10^5): a few dozen tiles.
constexpr int SCAN_BLOCK = 1024;
__global__ __launch_bounds__(SCAN_BLOCK) void scan_kernel(int64_t *__restrict__ v, int64_t n)
{
    __shared__ int64_t s_wave[SCAN_BLOCK / kWave];
    __shared__ int64_t s_carry;
    const int t = threadIdx.x, lane = t & (kWave - 1), wave = t / kWave;
    if (t == 0) s_carry = 0;
    __syncthreads();
    for (int64_t base = 1; base <= n; base += 4 * SCAN_BLOCK) {
        int64_t a[4];
        int64_t sum = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t j = base + (int64_t)t * 4 + k;
            a[k] = j <= n ? v[j] : 0;
            sum += a[k];
            a[k] = sum;  // inclusive inside the thread
        }
        const int64_t inc = wave_inclusive_scan(sum);  // of the thread sums inside the wave
        if (lane == kWave - 1) s_wave[wave] = inc;
        __syncthreads();
        int64_t before = s_carry;
        for (int w = 0; w < wave; ++w) before += s_wave[w];
        before += inc - sum;  // everything in front of this thread's four values
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t j = base + (int64_t)t * 4 + k;
            if (j <= n) v[j] = before + a[k];
        }
        __syncthreads();
        if (t == SCAN_BLOCK - 1) s_carry = before + sum;
        __syncthreads();
    }
}

// col[edge_start[i] + rank] = table[i, s] for the slots >= 0 of row i, in slot order
__global__ __launch_bounds__(ER_BLOCK) void table_fill_kernel(const int64_t *__restrict__ table, int64_t Nq, int W,
                                                               const int64_t *__restrict__ edge_start, int64_t E,
                                                               int64_t *__restrict__ col)
{
    const int64_t i = (int64_t)blockIdx.x * ER_WAVES + threadIdx.x / kWave;
    if (i >= Nq) return;
    const int lane = lane_id();
    int64_t at = edge_start[i];
    for (int s0 = 0; s0 < W; s0 += kWave) {
        const int s = s0 + lane;
        const int64_t j = s < W ? table[i * W + s] : -1;
        const unsigned long long mask = __ballot(j >= 0);
        const int64_t e = at + lanes_below(mask);
        if (j >= 0 && e < E) col[e] = j;
        at += __popcll(mask);
    }
}

// ---- edge rows --------------------------------------------------------------------------------------------------
// out[e, :] = [ x[col[e], 0:C] | pos_s[col[e]] - pos_q[i] | 0 .. ] for the edges e of query i (one piece per query)
__global__ __launch_bounds__(ER_BLOCK) void pointconv_rows_kernel(const float *__restrict__ x,
                                                                   const float *__restrict__ pos_s,
                                                                   const float *__restrict__ pos_q,
                                                                   const int64_t *__restrict__ edge_start,
                                                                   const int64_t *__restrict__ col, int64_t Nq,
                                                                   int64_t M, int64_t E, int C, int ld,
                                                                   float *__restrict__ out)
{
    int64_t i, e0, e1;
    int one;
    if (!wave_item(Nq, 1, i, one)) return;
    run_bounds(edge_start, i, E, e0, e1);
    if (e0 >= e1) return;
    const float qx = pos_q[i * 3 + 0], qy = pos_q[i * 3 + 1], qz = pos_q[i * 3 + 2];
    walk_rows(e0, e1, ld, [&](int64_t e, int c, int64_t at) {
        const int64_t j = col[e];
        float v = 0.0f;
        if (j >= 0 && j < M) {
            if (c < C) v = x[j * C + c];
            else if (c < C + 3) v = pos_s[j * 3 + (c - C)] - pick3(c - C, qx, qy, qz);
        }
        out[at] = v;
    });
}

// ---- segmented max ----------------------------------------------------------------------------------------------
// one wave per (segment, 64 channels): rows in ascending order, strict '>' keeps the first maximum
__global__ __launch_bounds__(ER_BLOCK) void segment_max_fwd_kernel(const float *__restrict__ rows,
                                                                    const int64_t *__restrict__ seg, int64_t S,
                                                                    int64_t E, int C, int ld, int chunks,
                                                                    float *__restrict__ out,
                                                                    int64_t *__restrict__ argmax)
{
    int64_t s, r0, r1;
    int chunk;
    if (!wave_item(S, chunks, s, chunk)) return;
    const int c = chunk * kWave + lane_id();
    if (c >= C) return;
    run_bounds(seg, s, E, r0, r1);
    float best = 0.0f;
    int64_t arg = -1;
    if (r0 < r1) {
        best = rows[r0 * ld + c];
        arg = r0;
        for (int64_t r = r0 + 1; r < r1; ++r) {
            const float v = rows[r * ld + c];
            if (v > best) {
                best = v;
                arg = r;
            }
        }
    }
    out[s * C + c] = best;
    argmax[s * C + c] = arg;
}

// d_rows[r, c] = dout[s, c] where r is the winning row of (s, c), else 0 (padding columns 0): every row belongs to
// one segment, so the rows are written, not accumulated.  A segment is cut into `parts` pieces of rows, a wave each.
__global__ __launch_bounds__(ER_BLOCK) void segment_max_bwd_kernel(const float *__restrict__ dout,
                                                                    const int64_t *__restrict__ argmax,
                                                                    const int64_t *__restrict__ seg, int64_t S,
                                                                    int64_t E, int C, int ld, int parts,
                                                                    float *__restrict__ d_rows)
{
    int64_t s, a, b;
    int part;
    if (!wave_item(S, parts, s, part)) return;
    run_piece(seg, s, E, part, parts, a, b);
    walk_rows(a, b, ld, [&](int64_t r, int c, int64_t at) {
        float v = 0.0f;
        if (c < C && argmax[s * C + c] == r) v = dout[s * C + c];
        d_rows[at] = v;
    });
}

}  // namespace tp3d

TP3D_EXPORT int tp3d_table_edge_start_i64(const int64_t *table, int64_t Nq, int max_num, int64_t *edge_start,
                                          void *stream)
{
    using namespace tp3d;
    if (Nq < 0 || max_num < 0 || !edge_start) return TP3D_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    if (Nq == 0) return zero_async(edge_start, sizeof(int64_t), s);
    if (!table && max_num > 0) return TP3D_E_BADARG;
    if (!grid_ok(Nq)) return TP3D_E_TOOBIG;
    hipLaunchKernelGGL(table_count_kernel, grid_of(Nq), dim3(ER_BLOCK), 0, s, table, Nq, max_num, edge_start);
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(SCAN_BLOCK), 0, s, edge_start, Nq);
    return check_launch();
}

TP3D_EXPORT int tp3d_table_edge_col_i64(const int64_t *table, const int64_t *edge_start, int64_t Nq, int max_num,
                                        int64_t E, int64_t *col, void *stream)
{
    using namespace tp3d;
    if (Nq < 0 || max_num < 0 || E < 0) return TP3D_E_BADARG;
    if (Nq == 0 || E == 0 || max_num == 0) return TP3D_OK;
    if (!table || !edge_start || !col) return TP3D_E_BADARG;
    if (!grid_ok(Nq)) return TP3D_E_TOOBIG;
    hipLaunchKernelGGL(table_fill_kernel, grid_of(Nq), dim3(ER_BLOCK), 0, (hipStream_t)stream, table, Nq, max_num,
                       edge_start, E, col);
    return check_launch();
}

TP3D_EXPORT int tp3d_pointconv_rows_f32(const float *x, const float *pos_s, const float *pos_q,
                                        const int64_t *edge_start, const int64_t *col, int64_t Nq, int64_t M,
                                        int64_t E, int C, int ld, float *out, void *stream)
{
    using namespace tp3d;
    if (Nq < 0 || M < 0 || E < 0 || C < 0 || ld < C + 3) return TP3D_E_BADARG;
    if (Nq == 0 || E == 0) return TP3D_OK;
    if (!pos_s || !pos_q || !edge_start || !col || !out || (C > 0 && !x)) return TP3D_E_BADARG;
    if (!grid_ok(Nq)) return TP3D_E_TOOBIG;
    hipLaunchKernelGGL(pointconv_rows_kernel, grid_of(Nq), dim3(ER_BLOCK), 0, (hipStream_t)stream, x, pos_s, pos_q,
                       edge_start, col, Nq, M, E, C, ld, out);
    return check_launch();
}

TP3D_EXPORT int tp3d_segment_max_fwd_f32(const float *rows, const int64_t *seg, int64_t S, int64_t E, int C, int ld,
                                         float *out, int64_t *argmax, void *stream)
{
    using namespace tp3d;
    if (S < 0 || E < 0 || C < 0 || ld < C) return TP3D_E_BADARG;
    if (S == 0 || C == 0) return TP3D_OK;
    if (!seg || !out || !argmax || (E > 0 && !rows)) return TP3D_E_BADARG;
    const int chunks = (C + kWave - 1) / kWave;
    if (!grid_ok(S * chunks)) return TP3D_E_TOOBIG;
    hipLaunchKernelGGL(segment_max_fwd_kernel, grid_of(S * chunks), dim3(ER_BLOCK), 0, (hipStream_t)stream, rows, seg,
                       S, E, C, ld, chunks, out, argmax);
    return check_launch();
}

TP3D_EXPORT int tp3d_segment_max_bwd_f32(const float *dout, const int64_t *argmax, const int64_t *seg, int64_t S,
                                         int64_t E, int C, int ld, float *d_rows, void *stream)
{
    using namespace tp3d;
    if (S < 0 || E < 0 || C < 0 || ld < C) return TP3D_E_BADARG;
    if (S == 0 || E == 0 || ld == 0) return TP3D_OK;
    if (!dout || !argmax || !seg || !d_rows) return TP3D_E_BADARG;
    const int64_t parts = run_parts(S, E);
    if (!grid_ok(S * parts)) return TP3D_E_TOOBIG;
    hipLaunchKernelGGL(segment_max_bwd_kernel, grid_of(S * parts), dim3(ER_BLOCK), 0, (hipStream_t)stream, dout,
                       argmax, seg, S, E, C, ld, (int)parts, d_rows);
    return check_launch();
}
