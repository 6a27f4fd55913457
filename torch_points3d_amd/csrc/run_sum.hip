// Summing through an inverted table (inverse_table.h): every destination adds the rows of its run in ascending slot
// order -- the gather that replaces the scatter-add of a backward pass, without float atomics and bit-reproducibly.
// Row-major ("rows") form: one wave per destination, lanes over channels (grouped-MLP backward of group_concat /
// interp_concat, the per-slot gradient rows of the KPConv backward passes).  Channel-major form: gather_sum_kernel, for
// grouping_operation and three_interpolate on (B, C, L) tensors.
#include <type_traits>

#include "inverse_table.h"

namespace tp3d {

constexpr int RW_BLOCK = 256;  // 4 waves, one destination per wave

__device__ __forceinline__ float rl_f(float x, int lane)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), lane));
}

// grad_x_cl[b,k,:] = sum over slots l (ascending) with idx[b,l]==k of grad_rows[(b,l), col0 + :]   (CSR gather)
// one wave per destination point, lanes over channels: every read is a contiguous row segment.  NP = channel slots per
// lane (c = lane + 64 p): a row of up to 64 NP channels is fetched in one traversal of the run, so 4 NP independent
// loads are in flight per lane (two traversals of 64 channels each ran the 128-channel decoder tables at 1.6 TB/s).
//
// acc[p] += sum over the slots [lo, hi) of the run, in slot order, of (weight *) row[c[p]]
template <int NP>
__device__ __forceinline__ void gather_run(const float *__restrict__ base, const int *__restrict__ od,
                                           const float *__restrict__ ws, int lo, int hi, int ld, const int (&c)[NP],
                                           float (&acc)[NP], int lane)
{
    // the run's (row, weight) pairs are fetched 64 at a time with one coalesced load, then broadcast lane by
    // lane (v_readlane), so independent row reads are in flight instead of a dependent index->row chain
    for (int j0 = lo; j0 < hi; j0 += 64) {
        const int cnt = min(64, hi - j0);
        const int my_r = (lane < cnt) ? od[j0 + lane] : 0;
        const float my_w = (ws && lane < cnt) ? ws[j0 + lane] : 1.0f;
        int t = 0;
        // U rows per step, all their loads issued before the first add (latency per step counts on a long run)
        auto take = [&](auto utag) {
            constexpr int U = decltype(utag)::value;
            int r[U];
            float wv[U], v[U][NP];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                r[u] = __builtin_amdgcn_readlane(my_r, t + u);
                wv[u] = ws ? rl_f(my_w, t + u) : 1.0f;
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int p = 0; p < NP; ++p) v[u][p] = base[(size_t)r[u] * ld + c[p]];
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int p = 0; p < NP; ++p) acc[p] = acc[p] + (ws ? wv[u] * v[u][p] : v[u][p]);  // slot order
            t += U;
        };
        while (t + 8 <= cnt) take(std::integral_constant<int, 8>());
        if (t + 4 <= cnt) take(std::integral_constant<int, 4>());
        // tail of 1..3 rows (most runs of a grouping table are that short): requested together, summed in order
        const int rem = cnt - t;
        if (rem > 0) {
            const int r0 = __builtin_amdgcn_readlane(my_r, t);
            const int r1 = __builtin_amdgcn_readlane(my_r, min(t + 1, cnt - 1));
            const int r2 = __builtin_amdgcn_readlane(my_r, min(t + 2, cnt - 1));
            const float w0 = ws ? rl_f(my_w, t) : 1.0f, w1 = ws ? rl_f(my_w, min(t + 1, cnt - 1)) : 1.0f,
                        w2 = ws ? rl_f(my_w, min(t + 2, cnt - 1)) : 1.0f;
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const float v0 = base[(size_t)r0 * ld + c[p]], v1 = base[(size_t)r1 * ld + c[p]],
                            v2 = base[(size_t)r2 * ld + c[p]];
                acc[p] = acc[p] + (ws ? w0 * v0 : v0);
                if (rem > 1) acc[p] = acc[p] + (ws ? w1 * v1 : v1);
                if (rem > 2) acc[p] = acc[p] + (ws ? w2 * v2 : v2);
            }
        }
    }
}

// Runs longer than HUB_MIN slots are left to rows_gather_hub_kernel (hub_min > 0): the first hit of a padded ball query
// collects every padding slot of every ball it opens -- 1295 slots on a 128-centre, 128-slot table over 512 points --
// and one wave walking that run alone held the whole launch (0.65 ms where a table of the same size without hubs takes
// 0.14 ms).
constexpr int HUB_MIN = 128;
constexpr int HUB_BLOCK = 1024;

template <int NP>
__global__ __launch_bounds__(RW_BLOCK) void rows_gather_sum_kernel(const float *__restrict__ grad_rows,
                                                                    const int *__restrict__ start,
                                                                    const int *__restrict__ order,
                                                                    const float *__restrict__ wsorted, int nbins,
                                                                    int L, int rows_per_cloud, int ld, int col0,
                                                                    int C, float *__restrict__ out, int flat, int hub_min)
{
    const int lane = threadIdx.x & 63;
    const int64_t dest = (int64_t)blockIdx.x * (RW_BLOCK / 64) + (threadIdx.x >> 6);  // destination point k
    const int b = blockIdx.y;
    if (dest >= nbins) return;
    // flat: one table over the whole batch (bins b*nbins + k, entries are batch-wide row ids); else one per cloud
    const int *st = flat ? start + (size_t)b * nbins : start + (size_t)b * (nbins + 1);
    const int *od = flat ? order : order + (size_t)b * L;
    const float *ws = wsorted ? (flat ? wsorted : wsorted + (size_t)b * L) : nullptr;
    const int lo = st[dest], hi = st[dest + 1];
    if (hub_min > 0 && hi - lo > hub_min) return;  // a hub: rows_gather_hub_kernel
    const float *base = grad_rows + (flat ? (size_t)0 : (size_t)b * rows_per_cloud * ld) + col0;
    for (int c0 = 0; c0 < C; c0 += 64 * NP) {
        int c[NP];
        float acc[NP];
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            c[p] = min(c0 + p * 64 + lane, C - 1);
            acc[p] = 0.0f;
        }
        gather_run<NP>(base, od, ws, lo, hi, ld, c, acc, lane);
#pragma unroll
        for (int p = 0; p < NP; ++p)
            if (c0 + p * 64 + lane < C) out[((size_t)b * nbins + dest) * C + c0 + p * 64 + lane] = acc[p];
    }
}

// hubs[0] = number of destinations with more than HUB_MIN slots, hubs[1..] = their ids b * nbins + k (any order)
__global__ __launch_bounds__(256) void find_hubs_kernel(const int *__restrict__ start, int B, int nbins, int flat,
                                                        int *__restrict__ hubs)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)B * nbins) return;
    const int b = (int)(e / nbins), k = (int)(e - (int64_t)b * nbins);
    const int *st = flat ? start + (size_t)b * nbins : start + (size_t)b * (nbins + 1);
    if (st[k + 1] - st[k] > HUB_MIN) hubs[1 + atomicAdd(&hubs[0], 1)] = (int)e;
}

// One workgroup of 16 waves per hub: the run is cut into 16 contiguous pieces, one per wave (each summed in slot order),
// and the pieces are added in piece order -- a fixed association, so the result is reproducible run to run.
template <int NP>
__global__ __launch_bounds__(HUB_BLOCK) void rows_gather_hub_kernel(const float *__restrict__ grad_rows,
                                                                     const int *__restrict__ start,
                                                                     const int *__restrict__ order,
                                                                     const float *__restrict__ wsorted,
                                                                     const int *__restrict__ hubs, int nbins, int L,
                                                                     int rows_per_cloud, int ld, int col0, int C,
                                                                     float *__restrict__ out, int flat)
{
    constexpr int NW = HUB_BLOCK / 64;
    __shared__ float part[NW][64 * NP];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int count = hubs[0];
    for (int h = blockIdx.x; h < count; h += gridDim.x) {
        const int e = hubs[1 + h];
        const int b = e / nbins, dest = e - b * nbins;
        const int *st = flat ? start + (size_t)b * nbins : start + (size_t)b * (nbins + 1);
        const int *od = flat ? order : order + (size_t)b * L;
        const float *ws = wsorted ? (flat ? wsorted : wsorted + (size_t)b * L) : nullptr;
        const int lo = st[dest], hi = st[dest + 1];
        const int per = ((hi - lo + NW - 1) / NW + 7) & ~7;  // slots per wave, a multiple of the 8-row step
        const int wlo = min(lo + wave * per, hi), whi = min(wlo + per, hi);
        const float *base = grad_rows + (flat ? (size_t)0 : (size_t)b * rows_per_cloud * ld) + col0;
        for (int c0 = 0; c0 < C; c0 += 64 * NP) {
            int c[NP];
            float acc[NP];
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                c[p] = min(c0 + p * 64 + lane, C - 1);
                acc[p] = 0.0f;
            }
            gather_run<NP>(base, od, ws, wlo, whi, ld, c, acc, lane);
#pragma unroll
            for (int p = 0; p < NP; ++p) part[wave][p * 64 + lane] = acc[p];
            __syncthreads();
            for (int x = threadIdx.x; x < 64 * NP; x += HUB_BLOCK) {
                float sum = part[0][x];
                for (int w = 1; w < NW; ++w) sum = sum + part[w][x];
                const int cc = c0 + x;  // x = p * 64 + lane
                if (cc < C) out[((size_t)b * nbins + dest) * C + cc] = sum;
            }
            __syncthreads();
        }
    }
}

// f(NP as an integral_constant) for rows of C channels: NP = channel slots per lane of the two row kernels
template <typename F>
static void with_np(int C, F f)
{
    if (C > 128) f(std::integral_constant<int, 4>());
    else if (C > 64) f(std::integral_constant<int, 2>());
    else f(std::integral_constant<int, 1>());
}

int find_hubs(const int *start, int B, int nbins, bool flat, int *hubs, hipStream_t s)
{
    if (int rc = zero_async(hubs, sizeof(int), s)) return rc;
    hipLaunchKernelGGL(find_hubs_kernel, dim3((unsigned)(((int64_t)B * nbins + 255) / 256)), dim3(256), 0, s, start, B, nbins,
                       flat ? 1 : 0, hubs);
    return check_launch();
}

// d_x[m, :] = sum of the per-slot gradient rows g[slot, :] that reference support point m, ascending slot (second step of
// the rigid and the deformable KPConv backward): the row gather over one flat table whose `order` holds slot ids, which
// are the row ids of g.  hub_min = 0: every run is summed sequentially by its wave, hubs included.
int gather_slot_rows(const float *g, const int *start, const int *order, int64_t M, int Cin, float *d_x, hipStream_t s)
{
    const dim3 grid((unsigned)((M + RW_BLOCK / 64 - 1) / (RW_BLOCK / 64)));
    with_np(Cin, [&](auto np) {
        hipLaunchKernelGGL(rows_gather_sum_kernel<decltype(np)::value>, grid, dim3(RW_BLOCK), 0, s, g, start, order, nullptr,
                           (int)M, 0, 0, Cin, 0, Cin, d_x, 1, 0);
    });
    return check_launch();
}

// ---------------------------------------------------------------------------------------------------
// Gather-sum over the transposed table: out[b,c,k] = sum_{j in [start[k], start[k+1])} w[j] * rows[b,c,order[j]]
// CC channel rows are staged in LDS (coalesced read of grad_out, each byte fetched once); every lane owns a
// destination k, reads its (order, weight) run once and accumulates CC channels from LDS.
constexpr int GS_BLOCK = 512;
constexpr int GS_HUB_MIN = 128;   // longer runs are summed by the whole workgroup
constexpr int GS_HUB_CAP = 1024;  // hubs listed per (cloud, channel group); further ones are walked by their lane

template <int CC, bool WEIGHTED, bool IN_LDS>
__global__ __launch_bounds__(GS_BLOCK) void gather_sum_kernel(const float *__restrict__ rows,
                                                               const int *__restrict__ start,
                                                               const int *__restrict__ order,
                                                               const float *__restrict__ wsorted, int C, int nbins,
                                                               int Lrow, int Lslots, float *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *srow = reinterpret_cast<float *>(smem);
    const int b = blockIdx.y;
    const int c0 = blockIdx.x * CC;
    const int tid = threadIdx.x;
    const float *gbase = rows + ((size_t)b * C + c0) * Lrow;
    const int nc = min(CC, C - c0);
    if (IN_LDS) {
        const int total = nc * Lrow;
        if ((Lrow & 3) == 0) {
            const float4 *g4 = reinterpret_cast<const float4 *>(gbase);
            float4 *s4 = reinterpret_cast<float4 *>(srow);
            for (int e = tid; e < total / 4; e += GS_BLOCK) s4[e] = g4[e];
        } else {
            for (int e = tid; e < total; e += GS_BLOCK) srow[e] = gbase[e];
        }
        __syncthreads();
    }
    const float *src = IN_LDS ? srow : gbase;
    const int *st = start + (size_t)b * (nbins + 1);
    const int *od = order + (size_t)b * Lslots;
    const float *ws = WEIGHTED ? wsorted + (size_t)b * Lslots : nullptr;
    // Destinations with more than GS_HUB_MIN slots (the shared first hit of padded ball queries collects hundreds to
    // thousands) are not walked by one lane while its workgroup waits: they are listed and then summed by the whole
    // workgroup, every wave a contiguous piece of the run, every lane a stride of the piece, the partial sums added in a
    // fixed order (lanes by butterfly, then pieces in order): reproducible run to run; shorter runs keep the oracle's
    // sequential order bit for bit.  (128 centres x 128 slots over 512 points, 128 channels: 1.5 ms -> see DESIGN.md.)
    __shared__ int s_nhub;
    __shared__ int s_hub[GS_HUB_CAP];
    __shared__ float s_part[GS_BLOCK / 64][CC];
    if (tid == 0) s_nhub = 0;
    __syncthreads();
    for (int k = tid; k < nbins; k += GS_BLOCK) {
        const int lo = st[k], hi = st[k + 1];
        if (hi - lo > GS_HUB_MIN) {
            const int pos = atomicAdd(&s_nhub, 1);
            if (pos < GS_HUB_CAP) {
                s_hub[pos] = k;
                continue;
            }  // (list full: this lane walks it after all)
        }
        float acc[CC];
#pragma unroll
        for (int cc = 0; cc < CC; ++cc) acc[cc] = 0.0f;
        for (int j = lo; j < hi; ++j) {
            const int r = od[j];
            const float w = WEIGHTED ? ws[j] : 1.0f;
#pragma unroll
            for (int cc = 0; cc < CC; ++cc) {
                if (cc < nc) {
                    const float v = src[(size_t)cc * Lrow + r];
                    acc[cc] = acc[cc] + (WEIGHTED ? w * v : v);  // mul then add, never fused (oracle order)
                }
            }
        }
#pragma unroll
        for (int cc = 0; cc < CC; ++cc)
            if (cc < nc) out[((size_t)b * C + c0 + cc) * nbins + k] = acc[cc];
    }
    __syncthreads();
    const int nhub = min(s_nhub, GS_HUB_CAP);
    const int lane = tid & 63, wave = tid >> 6;
    constexpr int NW = GS_BLOCK / 64;
    for (int h = 0; h < nhub; ++h) {
        const int k = s_hub[h];
        const int lo = st[k], hi = st[k + 1];
        const int per = (hi - lo + NW - 1) / NW;
        const int plo = min(lo + wave * per, hi), phi = min(plo + per, hi);
        float acc[CC];
#pragma unroll
        for (int cc = 0; cc < CC; ++cc) acc[cc] = 0.0f;
        for (int j = plo + lane; j < phi; j += 64) {
            const int r = od[j];
            const float w = WEIGHTED ? ws[j] : 1.0f;
#pragma unroll
            for (int cc = 0; cc < CC; ++cc)
                if (cc < nc) {
                    const float v = src[(size_t)cc * Lrow + r];
                    acc[cc] = acc[cc] + (WEIGHTED ? w * v : v);
                }
        }
#pragma unroll
        for (int cc = 0; cc < CC; ++cc)
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) acc[cc] = acc[cc] + __shfl_xor(acc[cc], off);
        if (lane == 0)
#pragma unroll
            for (int cc = 0; cc < CC; ++cc) s_part[wave][cc] = acc[cc];
        __syncthreads();
        if (tid < nc) {
            float sum = s_part[0][tid];
            for (int w = 1; w < NW; ++w) sum = sum + s_part[w][tid];
            out[((size_t)b * C + c0 + tid) * nbins + k] = sum;
        }
        __syncthreads();
    }
}

template <int CC, bool WEIGHTED, bool IN_LDS>
static void launch_gather(const float *rows, const int *start, const int *order, const float *wsorted, int B, int C,
                          int nbins, int Lrow, int Lslots, float *out, hipStream_t s)
{
    const size_t lds = IN_LDS ? (size_t)CC * Lrow * sizeof(float) : 0;
    if (lds > 64 * 1024)
        allow_large_dynamic_lds<&gather_sum_kernel<CC, WEIGHTED, IN_LDS>>(CSR_LDS_BYTES);
    dim3 grid((C + CC - 1) / CC, B);
    hipLaunchKernelGGL((gather_sum_kernel<CC, WEIGHTED, IN_LDS>), grid, dim3(GS_BLOCK), lds, s, rows, start, order,
                       wsorted, C, nbins, Lrow, Lslots, out);
}

template <bool WEIGHTED>
static int gather_sum_t(const float *rows, const int *start, const int *order, const float *wsorted, int B, int C,
                        int nbins, int Lrow, int Lslots, float *out, hipStream_t s)
{
    const size_t row_bytes = (size_t)Lrow * sizeof(float);
    if (4 * row_bytes <= (size_t)CSR_LDS_BYTES && C >= 4)
        launch_gather<4, WEIGHTED, true>(rows, start, order, wsorted, B, C, nbins, Lrow, Lslots, out, s);
    else if (2 * row_bytes <= (size_t)CSR_LDS_BYTES && C >= 2)
        launch_gather<2, WEIGHTED, true>(rows, start, order, wsorted, B, C, nbins, Lrow, Lslots, out, s);
    else if (row_bytes <= (size_t)CSR_LDS_BYTES)
        launch_gather<1, WEIGHTED, true>(rows, start, order, wsorted, B, C, nbins, Lrow, Lslots, out, s);
    else
        launch_gather<4, WEIGHTED, false>(rows, start, order, wsorted, B, C, nbins, Lrow, Lslots, out, s);
    return check_launch();
}

int gather_sum(const float *rows, const int *start, const int *order, const float *wsorted, int B, int C, int nbins,
               int Lrow, int Lslots, float *out, hipStream_t s)
{
    return wsorted ? gather_sum_t<true>(rows, start, order, wsorted, B, C, nbins, Lrow, Lslots, out, s)
                   : gather_sum_t<false>(rows, start, order, wsorted, B, C, nbins, Lrow, Lslots, out, s);
}

}  // namespace tp3d

using namespace tp3d;

TP3D_EXPORT int tp3d_rows_scatter_apply_f32(const float *grad_rows, int B, int L, int div, int nbins, int ld, int col0,
                                            int C, int with_weights, float *grad_x_cl, void *table, size_t table_bytes,
                                            void *stream)
{
    // grad_rows: (B, L/div rows, ld); slot l of cloud b refers to row l/div; destinations: (B, nbins, C)
    if (B < 0 || L < 0 || div <= 0 || nbins <= 0 || ld <= 0 || col0 < 0 || C < 0 || col0 + C > ld) return TP3D_E_BADARG;
    if (B == 0 || C == 0) return TP3D_OK;
    if (!grad_x_cl) return TP3D_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    if (L == 0) return zero_async(grad_x_cl, (size_t)B * nbins * C * sizeof(float), s);
    if (!grad_rows || !table || B > 65535) return TP3D_E_BADARG;
    ScatterWorkspace w = carve_scatter_workspace(table, B, L, nbins, with_weights != 0);
    if (table_bytes < w.bytes) return TP3D_E_BADARG;
    const bool flat = scatter_goes_flat(B, L, nbins);
    dim3 grid((nbins + RW_BLOCK / 64 - 1) / (RW_BLOCK / 64), B);
    const dim3 hub_grid(256);  // the hub count lives on the device: a fixed grid strides over the list (usually a few dozen)
    const int fl = flat ? 1 : 0;
    with_np(C, [&](auto np) {
        constexpr int NP = decltype(np)::value;
        hipLaunchKernelGGL(rows_gather_sum_kernel<NP>, grid, dim3(RW_BLOCK), 0, s, grad_rows, w.start, w.order, w.wsorted,
                           nbins, L, L / div, ld, col0, C, grad_x_cl, fl, HUB_MIN);
        hipLaunchKernelGGL(rows_gather_hub_kernel<NP>, hub_grid, dim3(HUB_BLOCK), 0, s, grad_rows, w.start, w.order, w.wsorted,
                           w.hubs, nbins, L, L / div, ld, col0, C, grad_x_cl, fl);
    });
    return check_launch();
}

TP3D_EXPORT int tp3d_rows_scatter_bwd_f32(const float *grad_rows, const int64_t *idx, const float *weight, int B,
                                          int L, int div, int nbins, int ld, int col0, int C, float *grad_x_cl,
                                          void *workspace, size_t workspace_bytes, void *stream)
{
    if (B < 0 || L < 0 || div <= 0 || nbins <= 0 || ld <= 0 || col0 < 0 || C < 0 || col0 + C > ld) return TP3D_E_BADARG;
    if (B == 0 || C == 0) return TP3D_OK;
    if (!grad_x_cl) return TP3D_E_BADARG;
    if (L == 0) return zero_async(grad_x_cl, (size_t)B * nbins * C * sizeof(float), (hipStream_t)stream);
    if (!grad_rows || !idx || !workspace || B > 65535) return TP3D_E_BADARG;
    if (int rc = tp3d_rows_scatter_invert(idx, weight, B, L, div, nbins, workspace, workspace_bytes, stream)) return rc;
    return tp3d_rows_scatter_apply_f32(grad_rows, B, L, div, nbins, ld, col0, C, weight != nullptr, grad_x_cl, workspace,
                                       workspace_bytes, stream);
}
