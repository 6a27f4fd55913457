// Message-passing RSConv (Relation-Shape convolution over a radius neighbourhood of varying size):
// relation rows, and the fused "gather x weight -> max" aggregation with its backward.
//
// Reference contract: torch_points3d/modules/RSConv/message_passing.py:30-50 (Convolution.message / update):
//   h_ij = [ |p_i - p_j|, p_i - p_j, p_i, p_j ],  M_ij = local_nn(h_ij),  out_i = max_j M_ij * x_j.
// local_nn has BatchNorm over ALL edges, so M (E, C) has to exist in memory; the gathered features x[col], the
// product and the rows the max reads do not: msgmax reads w and x and writes (Nq, C) only.
//
// Launch shapes (edge_run.h: blocks of 256 = 4 waves, a wave owns one query or one piece of its run):
//   * relation rows / msgmax backward: walk_rows over the (run, ld) floats of the query's edge run, so every store
//     is contiguous.  A run longer than 64 edges is cut into `parts` pieces of a wave each (the finder's cap is 64:
//     one piece; the entry points take any CSR).
//   * msgmax forward: one wave per (query, chunk of 64 channels).  A chunk of cw <= 64 channels puts G = 64 / cw
//     edges side by side in the wave (lane = edge_in_step * cw + channel): C = 3 walks 21 edges per step instead of
//     one, C >= 33 one edge per step with the lane as the channel, loads of one edge row contiguous.  Four steps are
//     loaded before they are compared (the loads of col, w and x of a step depend on nothing before them).  Every
//     lane keeps the first maximum of its own edges (ascending, strict '>'); the G lanes of a channel are then
//     folded by a shuffle tree under "larger value, or equal value and lower edge": the first maximum of the run, the
//     rule of tp3d_segment_max_fwd_f32.  One multiply per element and nothing to contract it with: bit-equal to
//     segment_max(w * x[col]).
//
// Backward route for dx: the EXISTING one.  The backward kernel writes d_w (dense, every element once) and, when x
// wants a gradient, the sparse edge rows g[e, c] = d_out[i, c] * w[e, c] at the winners (0 elsewhere) next to it in
// the same pass; tp3d_rows_scatter_bwd_f32 (inverse table + ordered gather-sum, no atomics) sums them per support
// row, as _PointConvRows.backward does.  It is deterministic and already tested at hub supports; the price is one
// (E, ld) matrix written and read once.  The alternative -- walking an inverse (support -> edges) list per support
// row and reading arg / d_out / w through it, which keeps the edge rows out of memory -- needs the same inversion
// and turns the contiguous row reads into one (query, channel) probe of `arg` per (edge, channel); it was not built.
// No floating-point atomics anywhere.
#include "edge_run.h"

namespace tp3d {

constexpr int RS_LD_MIN = 10;

// out[e, :] = [ |d|, d = pos_q[i] - pos_s[col[e]], pos_q[i], pos_s[col[e]], 0 .. ] for the edges e of query i
__global__ __launch_bounds__(ER_BLOCK) void rsconv_relation_rows_kernel(const float *__restrict__ pos_s,
                                                                         const float *__restrict__ pos_q,
                                                                         const int64_t *__restrict__ edge_start,
                                                                         const int64_t *__restrict__ col, int64_t Nq,
                                                                         int64_t M, int64_t E, int ld, int parts,
                                                                         float *__restrict__ out)
{
    int64_t i, a, b;
    int part;
    if (!wave_item(Nq, parts, i, part)) return;
    run_piece(edge_start, i, E, part, parts, a, b);
    if (a >= b) return;
    const float q[3] = {pos_q[i * 3 + 0], pos_q[i * 3 + 1], pos_q[i * 3 + 2]};
    walk_rows(a, b, ld, [&](int64_t e, int c, int64_t at) {
        const int64_t j = col[e];
        float v = 0.0f;
        if (j >= 0 && j < M && c < RS_LD_MIN) {
            if (c == 0) {
                v = sqrtf(sqdist3(q[0], q[1], q[2], pos_s[j * 3 + 0], pos_s[j * 3 + 1], pos_s[j * 3 + 2]));
            } else {
                const int k = (c - 1) % 3;
                const float qv = pick3(k, q[0], q[1], q[2]);
                v = c <= 3 ? qv - pos_s[j * 3 + k] : (c <= 6 ? qv : pos_s[j * 3 + k]);
            }
        }
        out[at] = v;
    });
}

// one product of edge e, channel c (a col outside [0, M) counts as a zero feature row)
__device__ __forceinline__ float msg_of(const float *__restrict__ w, int ldw, const float *__restrict__ x, int ldx,
                                        int64_t M, int64_t e, int64_t j, int c)
{
    const float xv = (j >= 0 && j < M) ? x[j * ldx + c] : 0.0f;
    return w[e * ldw + c] * xv;
}

__global__ __launch_bounds__(ER_BLOCK) void rsconv_msgmax_fwd_kernel(const float *__restrict__ w, int ldw,
                                                                      const float *__restrict__ x, int ldx,
                                                                      const int64_t *__restrict__ col,
                                                                      const int64_t *__restrict__ edge_start,
                                                                      int64_t Nq, int64_t M, int64_t E, int C, int chunks,
                                                                      float *__restrict__ out, int64_t *__restrict__ arg)
{
    int64_t i, e0, e1;
    int chunk;
    if (!wave_item(Nq, chunks, i, chunk)) return;  // wave-uniform: the shuffles below see whole waves
    const int c0 = chunk * kWave;
    const int cw = C - c0 < kWave ? C - c0 : kWave;  // channels of this chunk, >= 1
    const int G = kWave / cw;                        // edges side by side
    const int lane = lane_id();
    const int g = lane / cw;
    const int c = c0 + (lane - g * cw);
    const bool live = g < G;
    run_bounds(edge_start, i, E, e0, e1);
    float best = 0.0f;
    int64_t at = -1;
    if (live) {
        int64_t e = e0 + g;
        for (; e + 3 * (int64_t)G < e1; e += 4 * (int64_t)G) {
            int64_t j[4];
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) j[u] = col[e + u * G];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = msg_of(w, ldw, x, ldx, M, e + u * G, j[u], c);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (at < 0 || v[u] > best) {
                    best = v[u];
                    at = e + u * G;
                }
            }
        }
        for (; e < e1; e += G) {
            const float v = msg_of(w, ldw, x, ldx, M, e, col[e], c);
            if (at < 0 || v > best) {
                best = v;
                at = e;
            }
        }
    }
    // fold the G lanes of a channel: lane (g, c) takes lane (g + off, c)
    int top = 1;
    while (top < G) top <<= 1;
    for (int off = top >> 1; off >= 1; off >>= 1) {
        const int src = lane + off * cw;
        const float ov = __shfl(best, src & (kWave - 1));
        const int64_t oa = __shfl(at, src & (kWave - 1));
        if (live && g < off && g + off < G && oa >= 0 && (at < 0 || ov > best || (ov == best && oa < at))) {
            best = ov;
            at = oa;
        }
    }
    if (live && g == 0) {
        out[i * C + c] = at < 0 ? 0.0f : best;
        arg[i * C + c] = at;
    }
}

// d_w[e, c] = d_out[i, c] * x[col[e], c] and g_x[e, c] = d_out[i, c] * w[e, c] where e == arg[i, c], else 0 (padding
// columns 0); both (E, ldw), every element written once by the wave that owns the piece of the run.  g_x may be null.
__global__ __launch_bounds__(ER_BLOCK) void rsconv_msgmax_bwd_kernel(const float *__restrict__ dout,
                                                                      const int64_t *__restrict__ arg,
                                                                      const float *__restrict__ w, int ldw,
                                                                      const float *__restrict__ x, int ldx,
                                                                      const int64_t *__restrict__ col,
                                                                      const int64_t *__restrict__ edge_start,
                                                                      int64_t Nq, int64_t M, int64_t E, int C, int parts,
                                                                      float *__restrict__ d_w, float *__restrict__ g_x)
{
    int64_t i, a, b;
    int part;
    if (!wave_item(Nq, parts, i, part)) return;
    run_piece(edge_start, i, E, part, parts, a, b);
    walk_rows(a, b, ldw, [&](int64_t e, int c, int64_t at) {
        float dw = 0.0f, gx = 0.0f;
        if (c < C && arg[i * C + c] == e) {
            const float g = dout[i * C + c];
            const int64_t j = col[e];
            dw = g * ((j >= 0 && j < M) ? x[j * ldx + c] : 0.0f);
            gx = g * w[e * ldw + c];
        }
        d_w[at] = dw;
        if (g_x) g_x[at] = gx;
    });
}

}  // namespace tp3d

TP3D_EXPORT int tp3d_rsconv_relation_rows_f32(const float *pos_s, const float *pos_q, const int64_t *edge_start,
                                              const int64_t *col, int64_t Nq, int64_t M, int64_t E, int ld, float *out,
                                              void *stream)
{
    using namespace tp3d;
    if (Nq < 0 || M < 0 || E < 0 || ld < RS_LD_MIN) return TP3D_E_BADARG;
    if (Nq == 0 || E == 0) return TP3D_OK;
    if (!pos_s || !pos_q || !edge_start || !col || !out) return TP3D_E_BADARG;
    const int64_t parts = run_parts(Nq, E);
    if (!grid_ok(Nq * parts)) return TP3D_E_TOOBIG;
    hipLaunchKernelGGL(rsconv_relation_rows_kernel, grid_of(Nq * parts), dim3(ER_BLOCK), 0, (hipStream_t)stream, pos_s,
                       pos_q, edge_start, col, Nq, M, E, ld, (int)parts, out);
    return check_launch();
}

TP3D_EXPORT int tp3d_rsconv_msgmax_fwd_f32(const float *w, int ldw, const float *x, int ldx, const int64_t *col,
                                           const int64_t *edge_start, int64_t Nq, int64_t M, int64_t E, int C, float *out,
                                           int64_t *arg, void *stream)
{
    using namespace tp3d;
    if (Nq < 0 || M < 0 || E < 0 || C < 0 || ldw < C || ldx < C) return TP3D_E_BADARG;
    if (Nq == 0 || C == 0) return TP3D_OK;
    if (!edge_start || !out || !arg || (E > 0 && (!w || !x || !col))) return TP3D_E_BADARG;
    const int chunks = (C + kWave - 1) / kWave;
    if (!grid_ok(Nq * chunks)) return TP3D_E_TOOBIG;
    hipLaunchKernelGGL(rsconv_msgmax_fwd_kernel, grid_of(Nq * chunks), dim3(ER_BLOCK), 0, (hipStream_t)stream, w, ldw, x,
                       ldx, col, edge_start, Nq, M, E, C, chunks, out, arg);
    return check_launch();
}

TP3D_EXPORT int tp3d_rsconv_msgmax_bwd_f32(const float *dout, const int64_t *arg, const float *w, int ldw, const float *x,
                                           int ldx, const int64_t *col, const int64_t *edge_start, int64_t Nq, int64_t M,
                                           int64_t E, int C, float *d_w, float *g_x, void *stream)
{
    using namespace tp3d;
    if (Nq < 0 || M < 0 || E < 0 || C < 0 || ldw < C || ldx < C) return TP3D_E_BADARG;
    if (Nq == 0 || E == 0 || ldw == 0) return TP3D_OK;
    if (!dout || !arg || !w || !x || !col || !edge_start || !d_w) return TP3D_E_BADARG;
    const int64_t parts = run_parts(Nq, E);
    if (!grid_ok(Nq * parts)) return TP3D_E_TOOBIG;
    hipLaunchKernelGGL(rsconv_msgmax_bwd_kernel, grid_of(Nq * parts), dim3(ER_BLOCK), 0, (hipStream_t)stream, dout, arg, w,
                       ldw, x, ldx, col, edge_start, Nq, M, E, C, (int)parts, d_w, g_x);
    return check_launch();
}
