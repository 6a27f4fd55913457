// Stand-alone sweep of the host-side launch plans of the rows GEMM and the weight-gradient GEMM
// (torch_points3d_amd/csrc/gemm_plans.h) under the host sanitizers -- no device, no Python:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//         -I torch_points3d_amd/csrc tests/guard/few_row_plans_main.cpp -o few_row_plans && ./few_row_plans
// For both settings of the few-row tile rule and the ROWS x CHANNELS grid of tests/test_plans_cpu.py it walks every
// workgroup of a 64 x 64 rows launch through the kernel's own index arithmetic (tile origin inside the padded matrix,
// statistics chunk inside the buffer the caller was told to allocate) and every weight-gradient plan through its tile
// and split bounds.  Exit status 0 and "ok" on success.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "gemm_plans.h"

using namespace tp3d;

static int failures = 0;
#define CHECK(cond, ...)                                                                                             \
    do {                                                                                                             \
        if (!(cond)) {                                                                                               \
            if (++failures <= 20) {                                                                                  \
                fprintf(stderr, "%s:%d: %s failed: ", __FILE__, __LINE__, #cond);                                    \
                fprintf(stderr, __VA_ARGS__);                                                                        \
                fprintf(stderr, "\n");                                                                               \
            }                                                                                                        \
        }                                                                                                            \
    } while (0)

static std::vector<int64_t> rows()
{
    std::vector<int64_t> r = {1, 2, 3, 31, 32, 33, 63, 64, 65, 120, 127, 128, 129, 255, 256, 257, 480, 512, 1000, 1023, 1024,
                              1025, 2048, 2100, 3840, 4095, 4096, 4097, 8191, 8192, 11520, 16384, 65535, 65536, 65537, 130047,
                              130048, 130049, 130176, 130177, 130944, 131071, 131072, 131073, 262144, 524288, 1048575, 1048576,
                              1048577, 2097152, 4194304};
    const int ks[] = {1016, 1017, 1020, 1023, 1024, 1025};
    for (int k : ks)
        for (int d = -1; d <= 1; ++d) r.push_back(128 * (int64_t)k + d);
    return r;
}
static const int CHANNELS[] = {1, 3, 4, 6, 8, 10, 13, 16, 20, 24, 32, 48, 50, 64, 96, 128, 131, 132, 192, 196, 256, 259, 260,
                               320, 323, 384, 512, 515, 516, 1024, 1280, 1536};

// the statistics floats tp3d_gemm_rows_stat_floats reports (gemm_rows.hip)
static int64_t stat_floats(const RowsPlan &p, int N)
{
    const int64_t by_block = p.wave_rows * p.row_blocks;
    return (p.chunks > by_block ? p.chunks : by_block) * 4 * (int64_t)N;
}

static void sweep_rows(int64_t M, int N, int K)
{
    for (int split = 0; split < 2; ++split) {
        g_few_row_tiles = 0;
        const RowsPlan p0 = rows_plan(M, N, K, split != 0);
        CHECK(!rows_small_plan(p0).routed, "M=%lld N=%d K=%d", (long long)M, N, K);
        g_few_row_tiles = 1;
        const RowsPlan p = rows_plan(M, N, K, split != 0);
        CHECK(p.chunks == p0.chunks && p.items == p0.items && p.ksplit == p0.ksplit && p.wide == p0.wide, "M=%lld N=%d K=%d",
              (long long)M, N, K);
        const RowsSmallPlan s = rows_small_plan(p);
        CHECK(s.routed == (p.wide && p.ksplit == 1 && p.items <= 256), "M=%lld N=%d K=%d", (long long)M, N, K);
        if (!s.routed) continue;
        CHECK(s.blocks == 4 * p.items && s.blocks <= GR_GRID && s.items == s.blocks && !p.per_workgroup, "M=%lld N=%d",
              (long long)M, N);
        const int64_t floats = stat_floats(p, N);
        std::vector<char> seen((size_t)(p.row_blocks * 2 * p.tiles_n * 2), 0);  // every 64 x 64 part of the matrix once
        const int per = 32 * p.tiles_n;
        for (int64_t wg = 0; wg < s.blocks; ++wg) {  // gemm_rows_small_kernel's decode
            const int rem = (int)(wg % per);
            const int64_t rb = wg / per * 8 + (rem & 7);
            if (rb * GR_BM >= M) continue;
            const int half = (rem >> 3) & 1, n0 = (rem >> 4) * 64;
            CHECK(rb < p.row_blocks && n0 < p.tiles_n * 128, "M=%lld N=%d wg=%lld", (long long)M, N, (long long)wg);
            const size_t part = (size_t)((rb * 2 + half) * (p.tiles_n * 2) + n0 / 64);
            CHECK(part < seen.size() && !seen[part], "M=%lld N=%d wg=%lld", (long long)M, N, (long long)wg);
            if (part < seen.size()) seen[part] = 1;
            // last float of the chunk this workgroup writes: rows 0..3 of chunk (rb, half), columns below N
            const int64_t last = ((rb * 2 + half) * 4 + 3) * N + (N - 1);
            CHECK(rb * 2 + half < p.chunks && last < floats, "M=%lld N=%d wg=%lld", (long long)M, N, (long long)wg);
        }
        for (size_t i = 0; i < seen.size(); ++i) CHECK(seen[i], "M=%lld N=%d part %zu not covered", (long long)M, N, i);
    }
}

static void sweep_tn(int64_t M, int N, int K)
{
    g_few_row_tiles = 0;
    const TnPlan a = plan_tn(M, N, K);
    g_few_row_tiles = 1;
    const TnPlan b = plan_tn(M, N, K);
    CHECK(a.splits == b.splits && a.rows_per_split == b.rows_per_split && a.gn == b.gn, "M=%lld N=%d K=%d", (long long)M, N, K);
    const TnPlan *both[2] = {&a, &b};
    for (const TnPlan *p : both) {
        const int staged = (p->wm * p->wn) % 3 == 0 ? 16 : 64 / (p->wm * p->wn);
        CHECK(p->splits >= 1 && p->splits <= 512 && p->rows_per_split % 64 == 0 && p->rows_per_split % staged == 0, "M=%lld N=%d K=%d",
              (long long)M, N, K);
        CHECK((int64_t)(p->splits - 1) * p->rows_per_split < M && (int64_t)p->splits * p->rows_per_split >= M, "M=%lld N=%d K=%d",
              (long long)M, N, K);
        CHECK(p->tn == 32 * p->gn * p->wm && p->tk == 32 * (4 / p->gn) * p->wn, "M=%lld N=%d K=%d", (long long)M, N, K);
        CHECK((int64_t)p->tiles_n * p->tn >= N && (int64_t)(p->tiles_n - 1) * p->tn < N, "M=%lld N=%d K=%d", (long long)M, N, K);
        CHECK((int64_t)p->tiles_k * p->tk >= K && (int64_t)(p->tiles_k - 1) * p->tk < K, "M=%lld N=%d K=%d", (long long)M, N, K);
    }
    const int64_t wa = (int64_t)a.tiles_n * a.tiles_k * a.splits, wb = (int64_t)b.tiles_n * b.tiles_k * b.splits;
    if (a.gn == 1 || a.wn == 3 || wa >= TN_FILL) {
        CHECK(b.wm == a.wm && b.wn == a.wn, "M=%lld N=%d K=%d", (long long)M, N, K);
    } else {
        CHECK(b.wm <= a.wm && b.wn <= a.wn && b.wn != 3 && wb >= wa, "M=%lld N=%d K=%d", (long long)M, N, K);
    }
}

int main()
{
    long plans = 0;
    for (int64_t M : rows())
        for (int N : CHANNELS) {
            const int ks[] = {0, 4, 32, 256, 260, 1024, 1280, 1536};
            for (int K : ks) sweep_rows(M, N, K), ++plans;
            for (int K : CHANNELS)
                if ((int64_t)N * K <= 1024 * 1280) sweep_tn(M, N, K), ++plans;
        }
    g_few_row_tiles = 1;
    if (failures) {
        fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    printf("ok: %ld plans\n", plans);
    return 0;
}
