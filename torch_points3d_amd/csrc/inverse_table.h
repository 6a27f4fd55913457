// The inverse-table core: for every destination of an index table the slots that name it, in ascending slot order, so
// that a backward pass sums one run per destination instead of scattering -- no float atomics, a fixed summation order,
// bit-reproducible.  Two inverters build the table (inverse_table.hip): csr_transpose, one workgroup per cloud with the
// tables in LDS, and invert_table, a counting sort over any number of workgroups.  run_sum.hip sums through it.
// This header owns what the two inverters and the grid build (grid.hip) share -- the block scan of a histogram, the
// sorts of a bin, the workspace layouts -- with the standing edge_run.h has for the message-passing kernels:
// __forceinline__ device functions, every kernel keeps its own instruction stream.
#pragma once
#include "tp3d_common.h"

namespace tp3d {

// Exclusive scan of a histogram cnt[0..n) by one workgroup of BLOCK threads, cut where its users agree: thread tid owns
// the serial chunk [k0, k1), sums it, the wave scans the sums, and after one barrier every thread adds the totals of the
// waves in front of it (no serial pass by thread 0: one barrier fewer).  Returns the number of slots in the bins before
// k0; the caller walks its chunk and writes what it needs (in place, start + cursor, cell starts).  s_wave: BLOCK / 64
// ints of LDS.  Ends without a barrier.
template <int BLOCK, typename IdxT>
__device__ __forceinline__ int block_scan_chunk(const int *cnt, IdxT n, int *s_wave, IdxT &k0, IdxT &k1)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const IdxT per = (n + BLOCK - 1) / BLOCK;
    k0 = min((IdxT)tid * per, n);
    k1 = min(k0 + per, n);
    int sum = 0;
    for (IdxT k = k0; k < k1; ++k) sum += cnt[k];
    const int incl = wave_inclusive_scan(sum);
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int run = incl - sum;
#pragma unroll
    for (int w = 0; w < BLOCK / 64; ++w) run += (w < wave) ? s_wave[w] : 0;  // the waves in front
    return run;
}

// Bins of up to this many slots are insertion-sorted by one thread (the fills leave them nearly sorted); larger ones go
// to a whole wave.
constexpr int SMALL_BIN = 24;
template <typename OrdT>
__device__ __forceinline__ void sort_small_bin(OrdT *ord, int lo, int hi)
{
    for (int a = lo + 1; a < hi; ++a) {
        const OrdT v = ord[a];
        int p = a;
        while (p > lo && ord[p - 1] > v) {
            ord[p] = ord[p - 1];
            --p;
        }
        ord[p] = v;
    }
}

// Bitonic sort of one bin (n <= 64 * NU slot ids) by one wave: element i lives in lane i & 63, register i >> 6.
template <int NU, typename OrdT>
__device__ __forceinline__ void wave_sort_bin(OrdT *__restrict__ bin, int n, int lane)
{
    int e[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) e[u] = (lane + 64 * u < n) ? (int)bin[lane + 64 * u] : 0x7fffffff;
#pragma unroll
    for (int size = 2; size <= 64 * NU; size <<= 1) {
#pragma unroll
        for (int stride = size >> 1; stride >= 1; stride >>= 1) {
            if (stride >= 64) {  // partner in the same lane, another register
#pragma unroll
                for (int u = 0; u < NU; ++u) {
                    const int pu = u ^ (stride >> 6);
                    if (pu > u) {
                        const bool up = (((u << 6) | lane) & size) == 0;
                        const int a = e[u], b = e[pu];
                        const bool swap = up ? a > b : a < b;
                        e[u] = swap ? b : a;
                        e[pu] = swap ? a : b;
                    }
                }
            } else {
#pragma unroll
                for (int u = 0; u < NU; ++u) {
                    const int other = __shfl_xor(e[u], stride);
                    const bool up = (((u << 6) | lane) & size) == 0;
                    const bool lower = (lane & stride) == 0;
                    e[u] = (lower == up) ? min(e[u], other) : max(e[u], other);
                }
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();  // (the loads above all happened before the first exchange)
#pragma unroll
    for (int u = 0; u < NU; ++u)
        if (lane + 64 * u < n) bin[lane + 64 * u] = (OrdT)e[u];
}

// a bin of up to 1024 slots by one wave.  OrdT: uint16_t in LDS (L <= 65536), int otherwise.
template <typename OrdT>
__device__ __forceinline__ void wave_sort_any(OrdT *bin, int n, int lane)
{
    if (n <= 64) wave_sort_bin<1>(bin, n, lane);
    else if (n <= 128) wave_sort_bin<2>(bin, n, lane);
    else if (n <= 256) wave_sort_bin<4>(bin, n, lane);
    else if (n <= 512) wave_sort_bin<8>(bin, n, lane);
    else wave_sort_bin<16>(bin, n, lane);
}

constexpr int CSR_LDS_BYTES = 144 * 1024;  // LDS budget of the in-LDS inverter and of the channel-major gather-sum

// Workspace of the scatter-add backward entry points (all offsets 16-byte aligned).
struct ScatterWorkspace {
    int *start;      // B*(nbins+1)
    int *order;      // B*L
    int *scratch;    // B*L (only touched when a cloud's tables do not fit LDS)
    float *wsorted;  // B*L or null
    int *merge_tmp;  // B*L: second buffer of the run merge that sorts bins of more than 1024 slots (flat inversion)
    int *hubs;       // 1 + B*nbins: count, then the ids b*nbins + k of the destinations with long runs (run_sum.hip)
    size_t bytes;
};
ScatterWorkspace carve_scatter_workspace(void *ws, int B, int L, int nbins, bool with_weights);

// Workspace of invert_neighbors, tp3d_kpconv_bwd_workspace_bytes(M, slots): cnt | start | cursor | order | merge_tmp
struct InverseWorkspace {
    int *cnt;        // M
    int *start;      // M + 1
    int *cursor;     // M
    int *order;      // slots
    int *merge_tmp;  // slots: second buffer of the run merge that sorts a bin of more than 1024 slots (a hub support
                     // point: many queries padding onto one index, duplicated points); without it such a bin fell back
                     // to one lane's insertion sort -- tens of seconds
    size_t bytes;
};
InverseWorkspace carve_inverse_workspace(void *ws, int64_t M, int64_t slots);

// One workgroup per cloud (up to four for large in-LDS tables).  start: B*(nbins+1) ints, order: B*L ints (slot / div),
// wsorted: B*L floats or null, scratch_ord: B*L ints, only touched when the tables do not fit LDS.
int csr_transpose(const int64_t *idx, int B, int L, int nbins, int div, const float *weight, int *start, int *order,
                  float *wsorted, int *scratch_ord, hipStream_t s);
// does that transpose fit LDS?
bool csr_fits_lds(int L, int nbins);
// Multi-workgroup inverse of an index table (cnt, cursor: M ints; start: M + 1; order: slots).
// per_cloud_slots > 0: idx is (clouds, per_cloud_slots) with values clamped to [0, per_cloud_bins); bin = cloud *
// per_cloud_bins + value, M = clouds * per_cloud_bins (one flat table over the batch).
int invert_table(const int64_t *idx, int64_t slots, int64_t M, int *cnt, int *start, int *cursor, int *order,
                 hipStream_t s, int64_t per_cloud_slots = 0, int64_t per_cloud_bins = 0, int *merge_tmp = nullptr);
// Which of the two the row scatter (tp3d_rows_scatter_*) takes: one flat table over the batch through invert_table?
bool scatter_goes_flat(int B, int L, int nbins);
// The inverted neighbour table inside a tp3d_kpconv_bwd_workspace_bytes(M, slots) buffer (built unless `ready`).
int invert_neighbors(const int64_t *neighbors, int64_t slots, int64_t M, void *workspace, int **start_out,
                     int **order_out, hipStream_t s, bool ready = false);

// run_sum.hip: out[b,c,k] = sum over the run of k of (w *) rows[b,c,order[j]] (channel-major), and the per-support-point
// sum of per-slot gradient rows (ascending slot order)
int gather_sum(const float *rows, const int *start, const int *order, const float *wsorted, int B, int C, int nbins,
               int Lrow, int Lslots, float *out, hipStream_t s);
int gather_slot_rows(const float *g, const int *start, const int *order, int64_t M, int Cin, float *d_x, hipStream_t s);
// run_sum.hip: the hub list of a table (destinations with runs long enough for a whole workgroup): hubs[0] = their
// number, hubs[1..] = their ids b * nbins + k; enqueued at the end of tp3d_rows_scatter_invert
int find_hubs(const int *start, int B, int nbins, bool flat, int *hubs, hipStream_t s);

}  // namespace tp3d
