// Segmentation metrics on the device: confusion counts, ShapeNet part intersection / union counts, vote accumulation.
// Streaming passes with integer counters only: no float atomics, bit-reproducible, nothing read back by the host.
// Contracts: include/tp3d_hip.h ("Segmentation metrics").
#include "tp3d_common.h"

namespace tp3d {

constexpr int SM_BLOCK = 256;             // one lane per row of a tile
constexpr int SM_TILE = SM_BLOCK;         // rows staged per step
constexpr int SM_CW = 32;                 // columns staged per step
constexpr int SM_LDT = SM_CW + 1;         // odd row stride of the staged tile: lane r reads bank (33 r + c) % 64
constexpr int SM_MAX_BLOCKS = 1024;       // grid-stride over the tiles: 4 workgroups per CU
constexpr int SM_LDS_MAX_C = TP3D_CONFUSION_LDS_MAX_CLASSES;
constexpr int SM_PARTS = TP3D_PART_IOU_MAX_PARTS;
static_assert(SM_PARTS <= SM_CW, "a category is staged in one column step");

// Row argmax of a staged tile.  src[r] (LDS, written by the caller, barrier included) is the scores row of tile row r
// or -1 for a row that takes no part; columns [col_lo, col_lo + width) are staged SM_CW at a time with coalesced
// loads (consecutive lanes read consecutive columns of a row, then the next row), then lane r walks its own row in
// LDS.  The running maximum starts from the first column and only a strictly larger value replaces it: the lowest
// column holding the maximum wins, as numpy's argmax.  Returns the column offset inside the range.
__device__ __forceinline__ int tile_argmax(const float *__restrict__ scores, int ld, const int64_t *src, int rows, int col_lo,
                                           int width, float *tile)
{
    const int tid = threadIdx.x;
    float best = 0.0f;
    int arg = 0;
    for (int c0 = 0; c0 < width; c0 += SM_CW) {
        const int cw = min(SM_CW, width - c0);
        if (c0) __syncthreads();  // the previous step's reads are done
        for (int e = tid; e < rows * cw; e += SM_BLOCK) {
            const int r = e / cw;
            const int c = e - r * cw;
            const int64_t s = src[r];
            if (s >= 0) tile[r * SM_LDT + c] = scores[s * ld + col_lo + c0 + c];
        }
        __syncthreads();
        if (tid < rows && src[tid] >= 0) {
            const float *row = tile + tid * SM_LDT;
            int c = 0;
            if (c0 == 0) {
                best = row[0];
                c = 1;
            }
            for (; c < cw; ++c) {
                const float v = row[c];
                if (v > best) {
                    best = v;
                    arg = c0 + c;
                }
            }
        }
    }
    return arg;
}

__device__ __forceinline__ void add_i64(int64_t *p, int64_t v)
{
    __hip_atomic_fetch_add(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
}

// cm[label * C + prediction] += 1 per counted row, cm[C * C] += 1 per invalid row.  LDS_ROUTE: the workgroup counts in
// C * C int32 LDS cells (dynamic LDS) over all its tiles and flushes the non-zero ones once.
template <bool LDS_ROUTE>
__global__ __launch_bounds__(SM_BLOCK) void confusion_kernel(const float *__restrict__ scores, int64_t n_score_rows, int ld,
                                                             const int64_t *__restrict__ pred,
                                                             const int64_t *__restrict__ labels,
                                                             const int64_t *__restrict__ row_index, int64_t N, int C,
                                                             int col_lo, int col_hi, int64_t ignore_label, int64_t *cm)
{
    __shared__ float tile[SM_TILE * SM_LDT];
    __shared__ int64_t src[SM_TILE];
    __shared__ int invalid;
    extern __shared__ int cells[];
    const int tid = threadIdx.x;
    if (LDS_ROUTE)
        for (int e = tid; e < C * C; e += SM_BLOCK) cells[e] = 0;
    if (tid == 0) invalid = 0;
    const int64_t tiles = (N + SM_TILE - 1) / SM_TILE;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t i = t * SM_TILE + tid;
        const int rows = (int)min((int64_t)SM_TILE, N - t * SM_TILE);
        int64_t label = 0, s = -1;
        bool bad = false;
        __syncthreads();  // the zeroing above / the previous tile's reads of src
        if (tid < rows) {
            label = labels[i];
            if (label != ignore_label) {
                s = row_index ? row_index[i] : i;
                if (!(row_index && s == -1)) {
                    if (label < 0 || label >= C) bad = true;
                    if (pred) {
                        s = pred[i];
                        if (s < 0 || s >= C) bad = true;
                    } else if (s < 0 || s >= n_score_rows) {
                        bad = true;
                    }
                }
                if (bad) s = -1;
            }
        }
        int p;
        if (pred) {
            p = (int)s;
        } else {
            src[tid] = s;
            __syncthreads();
            p = col_lo + tile_argmax(scores, ld, src, rows, col_lo, col_hi - col_lo, tile);
        }
        if (bad) atomicAdd(&invalid, 1);
        if (s >= 0) {
            const int cell = (int)label * C + p;
            if (LDS_ROUTE)
                atomicAdd(&cells[cell], 1);
            else
                add_i64(cm + cell, 1);
        }
    }
    __syncthreads();
    if (LDS_ROUTE)
        for (int e = tid; e < C * C; e += SM_BLOCK) {
            const int v = cells[e];
            if (v) add_i64(cm + e, v);
        }
    if (tid == 0 && invalid) add_i64(cm + (int64_t)C * C, invalid);
}

// One workgroup per cloud: (intersection, union) per part of the cloud's category, the category being that of the
// cloud's FIRST label.  cat_lo[b] = first label of the category, -1 for an empty cloud, -2 where the first label, the
// tables or the offsets are unusable (nothing is counted then).
__global__ __launch_bounds__(SM_BLOCK) void part_iou_kernel(const float *__restrict__ scores, int ld,
                                                            const int64_t *__restrict__ labels,
                                                            const int64_t *__restrict__ seg, int64_t N, int C,
                                                            const int32_t *__restrict__ part_lo,
                                                            const int32_t *__restrict__ part_hi, int32_t *counts,
                                                            int32_t *cat_lo)
{
    __shared__ float tile[SM_TILE * SM_LDT];
    __shared__ int64_t src[SM_TILE];
    __shared__ int cells[SM_PARTS * 2];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    if (tid < SM_PARTS * 2) cells[tid] = 0;
    const int64_t s0 = seg[b], s1 = seg[b + 1];
    int lo = -1, hi = -1;
    if (s0 < 0 || s1 < s0 || s1 > N) {
        lo = -2;
    } else if (s1 > s0) {
        const int64_t first = labels[s0];
        if (first < 0 || first >= C) {
            lo = -2;
        } else {
            lo = part_lo[first];
            hi = part_hi[first];
            if (lo < 0 || hi <= lo || hi > C || hi - lo > SM_PARTS) lo = -2;
        }
    }
    if (lo >= 0) {
        for (int64_t r0 = s0; r0 < s1; r0 += SM_TILE) {
            const int rows = (int)min((int64_t)SM_TILE, s1 - r0);
            __syncthreads();
            src[tid] = tid < rows ? r0 + tid : -1;
            __syncthreads();
            const int p = tile_argmax(scores, ld, src, rows, lo, hi - lo, tile);  // prediction - lo
            if (tid < rows) {
                const int64_t l = labels[r0 + tid] - lo;  // a label outside the category matches no part
                if (l == p) {
                    atomicAdd(&cells[2 * p], 1);
                    atomicAdd(&cells[2 * p + 1], 1);
                } else {
                    atomicAdd(&cells[2 * p + 1], 1);
                    if (l >= 0 && l < hi - lo) atomicAdd(&cells[2 * (int)l + 1], 1);
                }
            }
        }
    }
    __syncthreads();
    if (tid < SM_PARTS * 2) counts[b * (SM_PARTS * 2) + tid] = cells[tid];
    if (tid == 0) cat_lo[b] = lo;
}

// Pass 1 of vote_add: the highest row of every target, as max over (epoch << 32 | row) words.  A word left by an
// earlier call carries a smaller epoch, so it loses against any row of this call: no clear between calls.
__global__ __launch_bounds__(SM_BLOCK) void vote_claim_kernel(const int64_t *__restrict__ ids, int64_t n, int64_t T,
                                                              int64_t epoch, int64_t *ws, int64_t *errors)
{
    const int64_t i = (int64_t)blockIdx.x * SM_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int64_t id = ids[i];
    if (id < 0 || id >= T) {
        add_i64(errors, 1);
        return;
    }
    __hip_atomic_fetch_max(reinterpret_cast<unsigned long long *>(ws) + id, (unsigned long long)((epoch << 32) | i),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Pass 2: the winning row of a target adds itself with plain loads and stores (one writer per target).
__global__ __launch_bounds__(SM_BLOCK) void vote_apply_kernel(const float *__restrict__ out, int ld,
                                                              const int64_t *__restrict__ ids, int64_t n, int C, int64_t T,
                                                              int64_t epoch, const int64_t *__restrict__ ws, float *votes,
                                                              int32_t *counts)
{
    const int64_t e = (int64_t)blockIdx.x * SM_BLOCK + threadIdx.x;
    if (e >= n * C) return;
    const int64_t i = e / C;
    const int c = (int)(e - i * C);
    const int64_t id = ids[i];
    if (id < 0 || id >= T || ws[id] != ((epoch << 32) | i)) return;
    votes[id * C + c] += out[i * ld + c];
    if (c == 0) counts[id] += 1;
}

}  // namespace tp3d

TP3D_EXPORT int tp3d_confusion_tile_rows(void) { return tp3d::SM_TILE; }
TP3D_EXPORT int tp3d_confusion_lds_max_classes(void) { return tp3d::SM_LDS_MAX_C; }
TP3D_EXPORT int tp3d_part_iou_max_parts(void) { return tp3d::SM_PARTS; }

TP3D_EXPORT int tp3d_confusion_count_f32(const float *scores, int64_t n_score_rows, int ld, const int64_t *pred,
                                         const int64_t *labels, const int64_t *row_index, int64_t N, int C, int col_lo,
                                         int col_hi, int64_t ignore_label, int64_t *cm, void *stream)
{
    if (N < 0 || C <= 0 || C > 32768 || n_score_rows < 0) return TP3D_E_BADARG;
    if (pred) {
        if (scores || row_index) return TP3D_E_BADARG;
    } else if (col_lo < 0 || col_hi <= col_lo || col_hi > C || ld < col_hi) {
        return TP3D_E_BADARG;
    }
    if (N == 0) return TP3D_OK;
    if (!labels || !cm || (!pred && !scores && n_score_rows > 0)) return TP3D_E_BADARG;
    if (N > ((int64_t)1 << 40)) return TP3D_E_TOOBIG;  // int32 LDS cells: at most N / 1024 + 256 rows per workgroup
    const int64_t tiles = (N + tp3d::SM_TILE - 1) / tp3d::SM_TILE;
    const unsigned blocks = (unsigned)(tiles < tp3d::SM_MAX_BLOCKS ? tiles : tp3d::SM_MAX_BLOCKS);
    if (C <= tp3d::SM_LDS_MAX_C)
        hipLaunchKernelGGL(tp3d::confusion_kernel<true>, dim3(blocks), dim3(tp3d::SM_BLOCK), (size_t)C * C * sizeof(int),
                           (hipStream_t)stream, scores, n_score_rows, ld, pred, labels, row_index, N, C, col_lo, col_hi,
                           ignore_label, cm);
    else
        hipLaunchKernelGGL(tp3d::confusion_kernel<false>, dim3(blocks), dim3(tp3d::SM_BLOCK), 0, (hipStream_t)stream, scores,
                           n_score_rows, ld, pred, labels, row_index, N, C, col_lo, col_hi, ignore_label, cm);
    return tp3d::check_launch();
}

TP3D_EXPORT int tp3d_part_iou_counts_f32(const float *scores, int ld, const int64_t *labels, const int64_t *seg, int64_t N,
                                         int64_t B, int C, const int32_t *part_lo, const int32_t *part_hi, int max_parts,
                                         int32_t *counts, int32_t *cat_lo, void *stream)
{
    if (N < 0 || B < 0 || C <= 0 || ld < C || max_parts <= 0) return TP3D_E_BADARG;
    if (max_parts > tp3d::SM_PARTS || N > INT32_MAX || B > INT32_MAX) return TP3D_E_TOOBIG;
    if (B == 0) return TP3D_OK;
    if (!seg || !part_lo || !part_hi || !counts || !cat_lo || (N > 0 && (!scores || !labels))) return TP3D_E_BADARG;
    hipLaunchKernelGGL(tp3d::part_iou_kernel, dim3((unsigned)B), dim3(tp3d::SM_BLOCK), 0, (hipStream_t)stream, scores, ld,
                       labels, seg, N, C, part_lo, part_hi, counts, cat_lo);
    return tp3d::check_launch();
}

TP3D_EXPORT int tp3d_vote_add_f32(const float *out, int ld, const int64_t *ids, int64_t n, int C, int64_t T, int64_t epoch,
                                  float *votes, int32_t *counts, int64_t *workspace, int64_t *errors, void *stream)
{
    if (n < 0 || C <= 0 || ld < C || T < 0 || epoch <= 0 || epoch > INT32_MAX) return TP3D_E_BADARG;
    if (n == 0) return TP3D_OK;
    if (!out || !ids || !errors || (T > 0 && (!votes || !counts || !workspace))) return TP3D_E_BADARG;
    const int64_t blocks1 = (n + tp3d::SM_BLOCK - 1) / tp3d::SM_BLOCK;
    const int64_t blocks2 = (n * C + tp3d::SM_BLOCK - 1) / tp3d::SM_BLOCK;
    if (n > INT32_MAX || blocks2 > INT32_MAX) return TP3D_E_TOOBIG;  // the row is the low half of the claim word
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(tp3d::vote_claim_kernel, dim3((unsigned)blocks1), dim3(tp3d::SM_BLOCK), 0, s, ids, n, T, epoch,
                       workspace, errors);
    if (int rc = tp3d::check_launch()) return rc;
    hipLaunchKernelGGL(tp3d::vote_apply_kernel, dim3((unsigned)blocks2), dim3(tp3d::SM_BLOCK), 0, s, out, ld, ids, n, C, T,
                       epoch, workspace, votes, counts);
    return tp3d::check_launch();
}
