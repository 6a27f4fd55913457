// The two inverters of an index table (inverse_table.h) and the entry points that choose between them.
//
// Given idx (B, L) with values in [0, nbins), produce per cloud
//     start (nbins+1) : start[k]..start[k+1] = the slots l with idx[l] == k
//     order (L)       : those slots, bin by bin, ASCENDING slot id inside a bin
// so that a backward pass becomes one gather-sum per destination element: no float atomics, and the
// summation order is fixed => bitwise reproducible (the oracle accumulates in the same ascending order).
//
// csr_transpose: one workgroup per cloud, everything in LDS: histogram with LDS integer atomics, block scan, unordered
// atomic fill, then every bin's (short) segment is insertion-sorted by slot id, which erases the only
// timing-dependent part.  Clouds whose tables do not fit LDS use the same algorithm on caller scratch in HBM.
// Used by the two scatter-add backward ops (grouping_operation and three_interpolate) and the row scatter below.
//
// invert_table: the same counting sort over any number of workgroups and the Nq*Mn slots of a whole neighbour table
// (integer histogram -> scan -> fill -> per-point sort of its short run, which makes the summation order ascending in
// (q, n) whatever the timing).  Used by the KPConv backward passes (kpconv.hip, kpconv_deform.hip), PosPool, the
// neighbour max-pool (nbr_maxpool.hip) and the flat form of the row scatter.
//
// A bin of more than 1024 slots is sorted differently by the two: the LDS kernel fills window by window behind barriers,
// so such a bin already is a sequence of sorted-by-window segments and sorting each segment sorts the bin; the
// multi-workgroup fill has no such order, so its wave merges 1024-slot runs through a second buffer (merge_tmp).
#include <algorithm>

#include "inverse_table.h"

namespace tp3d {

constexpr int CSR_BLOCK = 1024;
constexpr int CSR_RANK_SLOTS = 16;  // slots per lane when a wave ranks a large bin (bins up to 1024 slots)

template <typename OrdT, bool IN_LDS>
__global__ __launch_bounds__(CSR_BLOCK) void csr_transpose_kernel(const int64_t *__restrict__ idx, int L, int nbins,
                                                                   int div, const float *__restrict__ weight,
                                                                   int *__restrict__ start, int *__restrict__ order,
                                                                   float *__restrict__ wsorted,
                                                                   int *__restrict__ scratch_ord)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int s_wave[32];  // 128 B: keeps the dynamic region 16-byte aligned
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const int64_t *ib = idx + (size_t)b * L;
    int *g_start = start + (size_t)b * (nbins + 1);
    int *g_order = order + (size_t)b * L;
    // gridDim.y workgroups share a cloud (in-LDS tables only): each builds the full histogram (cheap) but fills, sorts
    // and writes only its contiguous range of bins -- the per-bin sorts are what the pass spends its time on
    const int part = blockIdx.y, parts = gridDim.y;
    const int k_lo = (int)((int64_t)nbins * part / parts), k_hi = (int)((int64_t)nbins * (part + 1) / parts);

    int *cnt;   // nbins ints: histogram -> bin start -> bin end
    OrdT *ord;  // L slot ids
    if (IN_LDS) {
        cnt = reinterpret_cast<int *>(smem);
        ord = reinterpret_cast<OrdT *>(smem + align_up((size_t)nbins * 4, 16));
    } else {
        cnt = g_start;  // reuse the output array (entry nbins is written at the end)
        ord = reinterpret_cast<OrdT *>(scratch_ord + (size_t)b * L);
    }

    for (int k = tid; k < nbins; k += CSR_BLOCK) cnt[k] = 0;
    __syncthreads();
    // Both slot passes were chains of (global index load -> LDS atomic), one 1024-slot window per iteration: ~2 us of
    // L2 latency each, 2 x L/1024 times, with one workgroup per cloud.  The indices of PER windows are now fetched
    // together into registers (and kept for the second pass when the cloud has at most PER windows), so the windows
    // themselves only touch LDS.  The fill pass still walks the windows in order with a barrier between them: a bin
    // must receive its slots in (nearly) ascending order or the insertion sort below degenerates (the padded tail of
    // a dense ball query repeats one index up to nsample times).
    constexpr int PER = 32;
    int vals[PER];
    const bool keep = L <= PER * CSR_BLOCK;
    for (int base = 0; base < L; base += PER * CSR_BLOCK) {
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int s = base + u * CSR_BLOCK + tid;
            vals[u] = s < L ? min(max((int)ib[s], 0), nbins - 1) : -1;
        }
#pragma unroll
        for (int u = 0; u < PER; ++u)
            if (vals[u] >= 0) atomicAdd(&cnt[vals[u]], 1);
    }
    __syncthreads();
    {  // histogram -> bin starts, in place: cnt[k] = #slots in bins < k
        int k0, k1;
        int run = block_scan_chunk<CSR_BLOCK>(cnt, nbins, s_wave, k0, k1);
        for (int k = k0; k < k1; ++k) {
            const int v = cnt[k];
            cnt[k] = run;
            run += v;
        }
    }
    __syncthreads();
    const int j_lo = k_lo < nbins ? cnt[k_lo] : L;  // first slot position of this workgroup's bins (read before the fill)
    __syncthreads();
    for (int base = 0; base < L; base += PER * CSR_BLOCK) {
        if (!keep) {
#pragma unroll
            for (int u = 0; u < PER; ++u) {
                const int s = base + u * CSR_BLOCK + tid;
                vals[u] = s < L ? min(max((int)ib[s], 0), nbins - 1) : -1;
            }
        }
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            if (base + u * CSR_BLOCK < L) {  // workgroup-uniform: the barrier is reached by every thread
                if (vals[u] >= k_lo && vals[u] < k_hi) {
                    const int pos = atomicAdd(&cnt[vals[u]], 1);  // cnt[k] ends as the END of bin k (own bins)
                    ord[pos] = (OrdT)(base + u * CSR_BLOCK + tid);
                }
                __syncthreads();
            }
        }
    }
    __syncthreads();
    // canonical order inside every bin: ascending slot id.  Small bins: one thread each, insertion sort (arrival order
    // is nearly sorted).  Large bins -- a point referenced by many slots: the padded tail of a dense ball query repeats
    // its first hit up to nsample times per query, an interpolation table references each coarse point ~100 times --
    // would serialise hundreds of dependent LDS steps in one thread (measured: 78 of 95 us for SA2's table), so a whole
    // wave sorts such a bin instead: its slots sit in registers (up to 16 per lane) and go through a bitonic network
    // (in-lane exchanges for strides >= 64, wave shuffles below).
    for (int k = k_lo + tid; k < k_hi; k += CSR_BLOCK) {
        const int lo = k == k_lo ? j_lo : cnt[k - 1], hi = cnt[k];
        if (hi - lo <= SMALL_BIN) sort_small_bin(ord, lo, hi);  // larger ones: sorted by a wave below
    }
    {
        const int lane = tid & 63, wave = tid >> 6;
        for (int k0 = k_lo + wave * 64; k0 < k_hi; k0 += (CSR_BLOCK / 64) * 64) {
            const int k = k0 + lane;
            int lo = 0, hi = 0;
            if (k < k_hi) {
                lo = k == k_lo ? j_lo : cnt[k - 1];
                hi = cnt[k];
            }
            unsigned long long big = __ballot(hi - lo > SMALL_BIN);
            while (big) {
                const int l = __builtin_ctzll(big);
                big &= big - 1;
                const int blo = __builtin_amdgcn_readlane(lo, l), bhi = __builtin_amdgcn_readlane(hi, l);
                if (bhi - blo <= 64 * CSR_RANK_SLOTS) {
                    wave_sort_any(ord + blo, bhi - blo, lane);
                    continue;
                }
                // A bin of more than 1024 slots (the first hit of many padded dense-ball queries): the fill pass above
                // walked the slots one 1024-slot window at a time with a barrier in between, so the bin is a sequence
                // of per-window segments that are already in window order -- sorting each segment (<= 1024 slots, found
                // by bisection on slot / 1024) sorts the bin.  One thread's insertion sort took 2.5 ms here.
                int a = blo;
                while (a < bhi) {
                    const int w = (int)ord[a] / CSR_BLOCK;
                    int x = a + 1, y = bhi;  // first position in (a, bhi] whose window differs
                    while (x < y) {
                        const int mid = (x + y) >> 1;
                        if ((int)ord[mid] / CSR_BLOCK == w) x = mid + 1;
                        else y = mid;
                    }
                    if (x - a > 1) wave_sort_any(ord + a, x - a, lane);
                    a = x;
                }
            }
        }
    }
    __syncthreads();
    const int j_hi = k_hi > k_lo ? cnt[k_hi - 1] : j_lo;
    for (int j = j_lo + tid; j < j_hi; j += CSR_BLOCK) {
        const int s = (int)ord[j];
        if (wsorted) wsorted[(size_t)b * L + j] = weight[(size_t)b * L + s];
        g_order[j] = s / div;
    }
    if (IN_LDS) {
        for (int k = k_lo + tid; k < k_hi; k += CSR_BLOCK) g_start[k] = k == k_lo ? j_lo : cnt[k - 1];
        if (tid == 0 && part == parts - 1) g_start[nbins] = L;
    } else {
        // cnt aliases g_start and holds bin ENDS: shift by one bin (every thread reads before anyone writes)
        const int per = (nbins + CSR_BLOCK - 1) / CSR_BLOCK;
        const int lo = min(tid * per, nbins), hi = min(lo + per, nbins);
        int prev = lo ? cnt[lo - 1] : 0;
        __syncthreads();
        for (int k = lo; k < hi; ++k) {
            int e = cnt[k];
            g_start[k] = prev;
            prev = e;
        }
        if (tid == 0) g_start[nbins] = L;
    }
}

size_t csr_lds_bytes(int L, int nbins) { return align_up((size_t)nbins * 4, 16) + (size_t)L * 2; }

bool csr_fits_lds(int L, int nbins) { return L <= 65536 && csr_lds_bytes(L, nbins) <= (size_t)CSR_LDS_BYTES; }

// Enqueue the transpose (buffers: inverse_table.h).
int csr_transpose(const int64_t *idx, int B, int L, int nbins, int div, const float *weight, int *start, int *order,
                  float *wsorted, int *scratch_ord, hipStream_t s)
{
    if (csr_fits_lds(L, nbins)) {
        allow_large_dynamic_lds<&csr_transpose_kernel<uint16_t, true>>(CSR_LDS_BYTES);
        // few clouds with large tables leave most of the chip idle: up to four workgroups per cloud, each a bin range
        int parts = 1;
        while (parts < 4 && B * parts * 2 <= 256 && nbins >= parts * 2 * 64 && L >= 8192) parts *= 2;
        hipLaunchKernelGGL((csr_transpose_kernel<uint16_t, true>), dim3(B, parts), dim3(CSR_BLOCK), csr_lds_bytes(L, nbins),
                           s, idx, L, nbins, div, weight, start, order, wsorted, scratch_ord);
    } else {
        hipLaunchKernelGGL((csr_transpose_kernel<int, false>), dim3(B), dim3(CSR_BLOCK), 0, s, idx, L, nbins, div,
                           weight, start, order, wsorted, scratch_ord);
    }
    return check_launch();
}

// ---------------------------------------------------------------------------------------------------
// The multi-workgroup inverter.

// bin of slot s: the table entry itself, or -- for a batch of per-cloud tables flattened into one -- the entry clamped
// to its cloud's bins plus the cloud's offset
__device__ __forceinline__ int64_t slot_bin(const int64_t *__restrict__ nbr, int64_t s, int64_t L, int64_t nbins)
{
    const int64_t m = nbr[s];
    return L > 0 ? min(max(m, (int64_t)0), nbins - 1) + (s / L) * nbins : m;
}

__global__ void nbr_hist_kernel(const int64_t *__restrict__ nbr, int64_t slots, int64_t M, int *__restrict__ cnt,
                                int64_t L, int64_t nbins)
{
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < slots; s += (int64_t)gridDim.x * blockDim.x) {
        const int64_t m = slot_bin(nbr, s, L, nbins);
        if (m >= 0 && m < M) atomicAdd(&cnt[m], 1);
    }
}

// exclusive scan of cnt[0..M) into start[0..M] (one workgroup), cursor := start
__global__ __launch_bounds__(1024) void nbr_scan_kernel(const int *__restrict__ cnt, int64_t M, int *__restrict__ start,
                                                         int *__restrict__ cursor)
{
    __shared__ int s_w[16];
    int64_t k0, k1;
    int run = block_scan_chunk<1024>(cnt, M, s_w, k0, k1);
    for (int64_t k = k0; k < k1; ++k) {
        const int v = cnt[k];
        start[k] = run;
        cursor[k] = run;
        run += v;
    }
    if (k1 == M) start[M] = run;  // every thread whose range ends at M holds the grand total
}

__global__ void nbr_fill_kernel(const int64_t *__restrict__ nbr, int64_t slots, int64_t M, int *__restrict__ cursor,
                                int *__restrict__ order, int64_t L, int64_t nbins)
{
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < slots; s += (int64_t)gridDim.x * blockDim.x) {
        const int64_t m = slot_bin(nbr, s, L, nbins);
        if (m >= 0 && m < M) order[atomicAdd(&cursor[m], 1)] = (int)s;
    }
}

// canonical order inside every bin (ascending slot id): one lane per bin for bins of up to SMALL_BIN slots
// (insertion sort; the fill leaves them nearly sorted), a whole wave's bitonic network for larger ones -- a point that
// hundreds of slots reference (padded tails of dense ball queries) would otherwise be hundreds of dependent global
// round trips in one thread
// A bin of more than 1024 slots, sorted by one wave: 1024-slot runs through the bitonic network, then log2(runs) merge
// passes between `order` and `tmp` -- every lane merges an equal share of a run pair, its split found by bisection
// (merge path).  Slot ids are unique, so the result is the ascending order whatever the arrival order was.
// (one thread's insertion sort needed tens of seconds for a 52 800-slot bin)
__device__ void wave_merge_sort_bin(int *order, int *tmp, int n, int lane)
{
    for (int a = 0; a < n; a += 1024) wave_sort_bin<16>(order + a, min(1024, n - a), lane);
    int *src = order, *dst = tmp;
    for (int width = 1024; width < n; width <<= 1) {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        __builtin_amdgcn_wave_barrier();
        for (int lo = 0; lo < n; lo += 2 * width) {
            const int mid = min(lo + width, n), hi = min(lo + 2 * width, n);
            const int *A = src + lo, *B = src + mid;
            const int na = mid - lo, nb = hi - mid, total = hi - lo;
            const int per = (total + 63) / 64;
            const int o0 = min(lane * per, total), o1 = min(o0 + per, total);
            // i = how many of the first o0 outputs come from A: smallest i with A[i] > B[o0 - i - 1]
            int x = max(0, o0 - nb), y = min(o0, na);
            while (x < y) {
                const int i = (x + y) >> 1, j = o0 - i;
                if (j > 0 && A[i] < B[j - 1]) x = i + 1;
                else y = i;
            }
            int i = x, j = o0 - x;
            for (int o = o0; o < o1; ++o) {
                const bool from_a = j >= nb || (i < na && A[i] < B[j]);
                dst[lo + o] = from_a ? A[i++] : B[j++];
            }
        }
        int *t = src;
        src = dst;
        dst = t;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
    if (src != order)
        for (int e = lane; e < n; e += 64) order[e] = src[e];
}

__global__ __launch_bounds__(256) void nbr_sort_kernel(const int *__restrict__ start, int64_t M, int *order, int *tmp)
{
    const int lane = threadIdx.x & 63;
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int s0 = 0, s1 = 0;
    if (m < M) {
        s0 = start[m];
        s1 = start[m + 1];
    }
    const int n = s1 - s0;
    if (n <= SMALL_BIN || (n > 1024 && !tmp)) sort_small_bin(order, s0, s1);
    unsigned long long big = __ballot(n > SMALL_BIN && n <= 1024);
    while (big) {  // wave-uniform
        const int l = __builtin_ctzll(big);
        big &= big - 1;
        const int blo = __builtin_amdgcn_readlane(s0, l), bn = __builtin_amdgcn_readlane(n, l);
        wave_sort_any(order + blo, bn, lane);
    }
    if (tmp) {
        unsigned long long giant = __ballot(n > 1024);
        while (giant) {  // wave-uniform
            const int l = __builtin_ctzll(giant);
            giant &= giant - 1;
            const int blo = __builtin_amdgcn_readlane(s0, l), bn = __builtin_amdgcn_readlane(n, l);
            wave_merge_sort_bin(order + blo, tmp + blo, bn, lane);
        }
    }
}

// Inverse of an index table over any number of workgroups: for every bin m the slots that reference it, ascending
// (integer histogram -> scan -> fill -> per-bin insertion sort of its short run).  Entries outside [0, M) are skipped.
// cnt, cursor: M ints; start: M + 1 ints; order: `slots` ints.
int invert_table(const int64_t *idx, int64_t slots, int64_t M, int *cnt, int *start, int *cursor, int *order,
                 hipStream_t s, int64_t per_cloud_slots, int64_t per_cloud_bins, int *merge_tmp)
{
    if (int rc = zero_async(cnt, (size_t)M * 4, s)) return rc;
    const unsigned gs = (unsigned)std::min<int64_t>((slots + 255) / 256, 4096);
    hipLaunchKernelGGL(nbr_hist_kernel, dim3(gs), dim3(256), 0, s, idx, slots, M, cnt, per_cloud_slots, per_cloud_bins);
    hipLaunchKernelGGL(nbr_scan_kernel, dim3(1), dim3(1024), 0, s, cnt, M, start, cursor);
    hipLaunchKernelGGL(nbr_fill_kernel, dim3(gs), dim3(256), 0, s, idx, slots, M, cursor, order, per_cloud_slots,
                       per_cloud_bins);
    hipLaunchKernelGGL(nbr_sort_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, start, M, order, merge_tmp);
    return check_launch();
}

// The next n 4-byte entries of a workspace that is handed out front to back (every piece 16-byte aligned).
template <typename T>
static T *carve(void *ws, size_t &off, size_t n)
{
    T *piece = reinterpret_cast<T *>(static_cast<char *>(ws) + off);
    off += align_up(n * 4, 16);
    return piece;
}

InverseWorkspace carve_inverse_workspace(void *ws, int64_t M, int64_t slots)
{
    InverseWorkspace w;
    w.bytes = 0;
    w.cnt = carve<int>(ws, w.bytes, (size_t)M);
    w.start = carve<int>(ws, w.bytes, (size_t)M + 1);
    w.cursor = carve<int>(ws, w.bytes, (size_t)M);
    w.order = carve<int>(ws, w.bytes, (size_t)slots);
    w.merge_tmp = carve<int>(ws, w.bytes, (size_t)slots);
    return w;
}

// workspace: tp3d_kpconv_bwd_workspace_bytes(M, slots)
int invert_neighbors(const int64_t *neighbors, int64_t slots, int64_t M, void *workspace, int **start_out,
                     int **order_out, hipStream_t s, bool ready)
{
    const InverseWorkspace w = carve_inverse_workspace(workspace, M, slots);
    *start_out = w.start;
    *order_out = w.order;
    if (ready) return TP3D_OK;  // the caller kept the table of an earlier call on the same neighbours
    return invert_table(neighbors, slots, M, w.cnt, w.start, w.cursor, w.order, s, 0, 0, w.merge_tmp);
}

// Workspace carve shared by the two backward entry points (all offsets 16-byte aligned).
ScatterWorkspace carve_scatter_workspace(void *ws, int B, int L, int nbins, bool with_weights)
{
    ScatterWorkspace w;
    w.bytes = 0;
    w.start = carve<int>(ws, w.bytes, (size_t)B * (nbins + 1));
    w.order = carve<int>(ws, w.bytes, (size_t)B * L);
    w.scratch = carve<int>(ws, w.bytes, (size_t)B * L);
    w.wsorted = with_weights ? carve<float>(ws, w.bytes, (size_t)B * L) : nullptr;
    w.merge_tmp = carve<int>(ws, w.bytes, (size_t)B * L);
    w.hubs = carve<int>(ws, w.bytes, (size_t)B * nbins + 1);
    return w;
}

// order[j] (slot id) -> row id (slot / div); wsorted[j] = weight[slot]; only the first start[nbins] entries are real
__global__ void slots_to_rows_kernel(int *__restrict__ order, const float *__restrict__ weight, int div, int L,
                                     const int *__restrict__ start, int nbins, float *__restrict__ wsorted)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= L || j >= start[nbins]) return;
    const int slot = order[j];
    if (wsorted) wsorted[j] = weight[slot];
    order[j] = slot / div;
}

bool scatter_goes_flat(int B, int L, int nbins)
{
    return L >= 2 * nbins && (int64_t)B * L < 0x7fffffff && (int64_t)B * nbins < 0x3fffffff &&
           ((B == 1 && L >= 16384) || !csr_fits_lds(L, nbins));
}

}  // namespace tp3d

using namespace tp3d;

TP3D_EXPORT size_t tp3d_scatter_workspace_bytes(int B, int L, int nbins, int with_weights)
{
    if (B < 0 || L < 0 || nbins < 0) return 0;
    return carve_scatter_workspace(nullptr, B, L, nbins, with_weights != 0).bytes;
}

TP3D_EXPORT size_t tp3d_kpconv_bwd_workspace_bytes(int64_t M, int64_t slots)
{
    if (M < 0 || slots < 0) return 0;
    return carve_inverse_workspace(nullptr, M, slots).bytes;
}

TP3D_EXPORT size_t tp3d_kpconv_grad_workspace_bytes(int64_t M, int64_t slots, int Cin)
{
    if (M < 0 || slots < 0 || Cin <= 0) return 0;
    return align_up((size_t)slots * Cin * 4, 16);  // the per-slot gradient rows
}

// plan[0..8] = byte offsets of start, order, scratch, wsorted (-1 without weights), merge_tmp in the workspace, its
// size in bytes, 1 when the table is inverted flat over the whole batch, ints of `scratch` that path uses, byte offset
// of the hub list (1 + B*nbins ints)
TP3D_EXPORT int tp3d_scatter_plan(int B, int L, int nbins, int with_weights, int64_t *plan)
{
    if (B <= 0 || L <= 0 || nbins <= 0 || !plan) return TP3D_E_BADARG;
    const ScatterWorkspace w = carve_scatter_workspace(nullptr, B, L, nbins, with_weights != 0);
    plan[0] = (char *)w.start - (char *)nullptr;
    plan[1] = (char *)w.order - (char *)nullptr;
    plan[2] = (char *)w.scratch - (char *)nullptr;
    plan[3] = w.wsorted ? (char *)w.wsorted - (char *)nullptr : -1;
    plan[4] = (char *)w.merge_tmp - (char *)nullptr;
    plan[5] = (int64_t)w.bytes;
    plan[6] = scatter_goes_flat(B, L, nbins) ? 1 : 0;
    plan[7] = plan[6] ? 2 * (int64_t)B * nbins : 0;  // invert_table: histogram + cursors
    plan[8] = (char *)w.hubs - (char *)nullptr;
    return TP3D_OK;
}

// The inverted neighbour table ("which slots point at support point k") depends on idx / weight only -- geometry, not
// features: tp3d_rows_scatter_invert builds it into `workspace`, tp3d_rows_scatter_apply_f32 consumes a table built
// earlier for the same (idx, weight, B, L, div, nbins) -- e.g. one step ahead on another stream, beside the sampling
// and the searches -- and tp3d_rows_scatter_bwd_f32 does both.
TP3D_EXPORT int tp3d_rows_scatter_invert(const int64_t *idx, const float *weight, int B, int L, int div, int nbins,
                                         void *workspace, size_t workspace_bytes, void *stream)
{
    if (B < 0 || L < 0 || div <= 0 || nbins <= 0) return TP3D_E_BADARG;
    if (B == 0 || L == 0) return TP3D_OK;
    if (!idx || !workspace || B > 65535) return TP3D_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    ScatterWorkspace w = carve_scatter_workspace(workspace, B, L, nbins, weight != nullptr);
    if (workspace_bytes < w.bytes) return TP3D_E_BADARG;
    // One large cloud (partial-dense decoders), or clouds whose tables do not fit one workgroup's LDS (multi-scale
    // grouping: 512 x 128 slots per cloud): invert ONE flat table over the whole device instead of one table per
    // workgroup (scratch holds the histogram and the cursors), then turn slot ids into row ids and line the weights up.
    // (measured on the 49 152-slot decoder tables, which fit LDS: flat 523 us vs per-cloud 354 us, so off by default)
    const bool flat = scatter_goes_flat(B, L, nbins);
    if (flat) {
        const int64_t slots = (int64_t)B * L, bins = (int64_t)B * nbins;
        if (int rc = invert_table(idx, slots, bins, w.scratch, w.start, w.scratch + bins, w.order, s, L, nbins, w.merge_tmp))
            return rc;
        hipLaunchKernelGGL(slots_to_rows_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, s, w.order, weight, div,
                           (int)slots, w.start, (int)bins, w.wsorted);
        if (int rc = check_launch()) return rc;
    } else if (int rc = csr_transpose(idx, B, L, nbins, div, weight, w.start, w.order, w.wsorted, w.scratch, s)) {
        return rc;
    }
    // the destinations whose runs are long enough to be summed by a whole workgroup (rows_gather_hub_kernel)
    return find_hubs(w.start, B, nbins, flat, w.hubs, s);
}
