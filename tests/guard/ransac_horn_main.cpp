// csrc/ransac_horn.h compiled without a device, as a program of its own (tests/test_ransac_cpu.py runs it, under the host
// sanitizers where there are any):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I torch_points3d_amd/csrc tests/guard/ransac_horn_main.cpp \
//       -o ransac_horn && ./ransac_horn
// For samples of 3, 4 and 8 pairs -- rigid copies, noisy copies, planar clouds, planar clouds against their mirror image,
// repeated points, one point -- the pose must be a proper rotation (orthonormal to 1e-12, det = +1), must leave a sum of
// squared residuals below 1e-18 where an exact fit exists, and must never be worse in the least-squares sense than the
// pose the data were made with or than the best translation alone.
#include <stdint.h>
#include <stdio.h>

#include "ransac_horn.h"

static uint64_t g_state = 0x9e3779b97f4a7c15ull;

static double uniform()  // [-1, 1)
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_state >> 11) / (double)(1ull << 52) - 1.0;
}

static int g_failed = 0;

#define CHECK(cond, ...)                       \
    do {                                       \
        if (!(cond)) {                         \
            if (g_failed < 10) {               \
                printf("FAILED %s: ", #cond);  \
                printf(__VA_ARGS__);           \
                printf("\n");                  \
            }                                  \
            ++g_failed;                        \
        }                                      \
    } while (0)

static void rotation_of(double ax, double ay, double az, double angle, double (&R)[9])
{
    const double n = sqrt(ax * ax + ay * ay + az * az);
    const double x = ax / n, y = ay / n, z = az / n, c = cos(angle), s = sin(angle), v = 1.0 - c;
    const double r[9] = {c + x * x * v, x * y * v - z * s, x * z * v + y * s, y * x * v + z * s, c + y * y * v,
                         y * z * v - x * s, z * x * v - y * s, z * y * v + x * s, c + z * z * v};
    for (int e = 0; e < 9; ++e) R[e] = r[e];
}

// sum |R p + t - q|^2 over the pairs
static double residual(const double (&pose)[12], const double (*p)[3], const double (*q)[3], int n)
{
    double sum = 0.0;
    for (int i = 0; i < n; ++i)
        for (int a = 0; a < 3; ++a) {
            const double d = pose[a * 4] * p[i][0] + pose[a * 4 + 1] * p[i][1] + pose[a * 4 + 2] * p[i][2] + pose[a * 4 + 3] - q[i][a];
            sum += d * d;
        }
    return sum;
}

static void solve(const double (*p)[3], const double (*q)[3], int n, double (&pose)[12])
{
    double mp[3] = {0, 0, 0}, mq[3] = {0, 0, 0}, S[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < n; ++i)
        for (int a = 0; a < 3; ++a) mp[a] += p[i][a] / n, mq[a] += q[i][a] / n;
    for (int i = 0; i < n; ++i)
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) S[a * 3 + b] += (p[i][a] - mp[a]) * (q[i][b] - mq[b]);
    tp3d::horn_pose(S, mp, mq, pose);
}

int main()
{
    const int sizes[3] = {3, 4, 8};
    int cases = 0;
    for (int trial = 0; trial < 6000; ++trial) {
        const int n = sizes[trial % 3], kind = (trial / 3) % 6;
        double p[8][3], q[8][3], R[9], t[3] = {uniform() * 3, uniform() * 3, uniform() * 3};
        rotation_of(uniform(), uniform(), uniform() + 1.5, uniform() * 3.1, R);
        for (int i = 0; i < n; ++i) {
            for (int a = 0; a < 3; ++a) p[i][a] = uniform();
            if (kind == 2 || kind == 3) p[i][2] = 0.25;         // planar
            if (kind == 4 && i > 0 && i % 2 == 1)               // repeated points (a draw with replacement)
                for (int a = 0; a < 3; ++a) p[i][a] = p[i - 1][a];
            if (kind == 5)                                      // one point, n times
                for (int a = 0; a < 3; ++a) p[i][a] = p[0][a];
        }
        for (int i = 0; i < n; ++i) {
            const double m[3] = {kind == 3 ? -p[i][0] : p[i][0], p[i][1], p[i][2]};  // kind 3: the mirror image
            for (int a = 0; a < 3; ++a) {
                q[i][a] = R[a * 3] * m[0] + R[a * 3 + 1] * m[1] + R[a * 3 + 2] * m[2] + t[a];
                if (kind == 1) q[i][a] += 0.05 * uniform();     // noisy
            }
        }
        double pose[12];
        solve(p, q, n, pose);
        ++cases;
        double worst = 0.0;
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) {
                double dot = 0.0;
                for (int k = 0; k < 3; ++k) dot += pose[a * 4 + k] * pose[b * 4 + k];
                worst = fmax(worst, fabs(dot - (a == b ? 1.0 : 0.0)));
            }
        const double det = pose[0] * (pose[5] * pose[10] - pose[6] * pose[9]) - pose[1] * (pose[4] * pose[10] - pose[6] * pose[8]) +
                           pose[2] * (pose[4] * pose[9] - pose[5] * pose[8]);
        CHECK(worst < 1e-12 && fabs(det - 1.0) < 1e-12, "trial %d kind %d n %d: |R R^T - I| %.3g, det %.17g", trial, kind, n, worst, det);
        const double got = residual(pose, p, q, n);
        if (kind == 0 || kind == 2 || kind == 3)  // an exact fit exists (for the mirrored plane: the half turn about an in-plane axis)
            CHECK(got < 1e-18, "trial %d kind %d n %d: residual %.3g of an exact fit", trial, kind, n, got);
        if (kind != 3) {  // never worse than the pose the data were made with, nor than the best translation alone
            double truth[12], plain[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
            for (int a = 0; a < 3; ++a) {
                for (int b = 0; b < 3; ++b) truth[a * 4 + b] = R[a * 3 + b];
                truth[a * 4 + 3] = t[a];
            }
            CHECK(got <= residual(truth, p, q, n) + 1e-12, "trial %d kind %d n %d: %.3g worse than the true pose", trial, kind, n, got);
            double mp[3] = {0, 0, 0}, mq[3] = {0, 0, 0};
            for (int i = 0; i < n; ++i)
                for (int a = 0; a < 3; ++a) mp[a] += p[i][a] / n, mq[a] += q[i][a] / n;
            for (int a = 0; a < 3; ++a) plain[a * 4 + 3] = mq[a] - mp[a];
            CHECK(got <= residual(plain, p, q, n) + 1e-12, "trial %d kind %d n %d: %.3g worse than a translation", trial, kind, n, got);
        }
        if (kind == 5) CHECK(got < 1e-24, "trial %d: one point is not mapped onto its image (%.3g)", trial, got);
    }
    // a matrix of zeros: the identity rotation
    const double zero[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    double R0[9];
    tp3d::horn_rotation(zero, R0);
    for (int e = 0; e < 9; ++e) CHECK(R0[e] == (e % 4 == 0 ? 1.0 : 0.0), "zeros: R[%d] = %.17g", e, R0[e]);
    if (g_failed) {
        printf("%d checks failed\n", g_failed);
        return 1;
    }
    printf("ok: %d poses\n", cases);
    return 0;
}
