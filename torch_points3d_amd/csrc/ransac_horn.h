// Horn's closed-form absolute orientation in double (Horn 1987, "Closed-form solution of absolute orientation using unit
// quaternions"): the rotation that maps centred sources p onto centred targets q in the least-squares sense, from their
// cross-covariance S[a * 3 + b] = sum w p_a q_b.  The unit eigenvector of the largest eigenvalue of the symmetric 4 x 4
// matrix N(S) is the quaternion (w, x, y, z) of that rotation; it is found by cyclic Jacobi sweeps with every index a
// compile-time constant (one thread per problem, everything in registers).  The result is a proper rotation by
// construction: this equals Kabsch with the determinant correction, without a 3 x 3 SVD.
//
// Plain C++: the device kernels of ransac.hip and a host program compile the same text.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define TP3D_HD __host__ __device__ __forceinline__
#else
#define TP3D_HD inline
#endif

namespace tp3d {

constexpr int HORN_MAX_SWEEPS = 16;  // cyclic Jacobi on a 4 x 4 matrix converges quadratically: 6-8 sweeps in practice

// one Jacobi rotation in the (P, Q) plane: A <- J^T A J (A symmetric, both triangles kept), V <- V J
template <int P, int Q>
TP3D_HD void horn_rotate(double (&A)[4][4], double (&V)[4][4])
{
    const double apq = A[P][Q];
    if (apq == 0.0) return;
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    // the smaller root of t^2 + 2 t theta - 1 = 0; |theta| = inf (apq negligible) gives t = 0
    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    A[P][P] -= t * apq;
    A[Q][Q] += t * apq;
    A[P][Q] = A[Q][P] = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k != P && k != Q) {
            const double akp = A[k][P], akq = A[k][Q];
            A[k][P] = A[P][k] = c * akp - s * akq;
            A[k][Q] = A[Q][k] = s * akp + c * akq;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double vkp = V[k][P], vkq = V[k][Q];
        V[k][P] = c * vkp - s * vkq;
        V[k][Q] = s * vkp + c * vkq;
    }
}

// R (row-major 3 x 3) from the cross-covariance S (row-major 3 x 3, S[a * 3 + b] = sum p_a q_b of the centred pairs)
TP3D_HD void horn_rotation(const double (&S)[9], double (&R)[9])
{
    double A[4][4], V[4][4];
    A[0][0] = (S[0] + S[4]) + S[8];
    A[1][1] = (S[0] - S[4]) - S[8];
    A[2][2] = (S[4] - S[0]) - S[8];
    A[3][3] = (S[8] - S[0]) - S[4];
    A[0][1] = A[1][0] = S[5] - S[7];
    A[0][2] = A[2][0] = S[6] - S[2];
    A[0][3] = A[3][0] = S[1] - S[3];
    A[1][2] = A[2][1] = S[1] + S[3];
    A[1][3] = A[3][1] = S[6] + S[2];
    A[2][3] = A[3][2] = S[5] + S[7];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) V[r][c] = r == c ? 1.0 : 0.0;
    for (int sweep = 0; sweep < HORN_MAX_SWEEPS; ++sweep) {
        const double off = ((A[0][1] * A[0][1] + A[0][2] * A[0][2]) + (A[0][3] * A[0][3] + A[1][2] * A[1][2])) +
                           (A[1][3] * A[1][3] + A[2][3] * A[2][3]);
        const double diag = (A[0][0] * A[0][0] + A[1][1] * A[1][1]) + (A[2][2] * A[2][2] + A[3][3] * A[3][3]);
        if (!(off > 1e-36 * diag)) break;  // (also ends a matrix of zeros, and one that is not a number)
        horn_rotate<0, 1>(A, V);
        horn_rotate<0, 2>(A, V);
        horn_rotate<0, 3>(A, V);
        horn_rotate<1, 2>(A, V);
        horn_rotate<1, 3>(A, V);
        horn_rotate<2, 3>(A, V);
    }
    // the column of the largest eigenvalue (the lowest index among equal ones)
    double best = A[0][0];
    double w = V[0][0], x = V[1][0], y = V[2][0], z = V[3][0];
#pragma unroll
    for (int m = 1; m < 4; ++m) {
        if (A[m][m] > best) {
            best = A[m][m];
            w = V[0][m], x = V[1][m], y = V[2][m], z = V[3][m];
        }
    }
    const double inv = 1.0 / sqrt((w * w + x * x) + (y * y + z * z));
    w *= inv, x *= inv, y *= inv, z *= inv;
    R[0] = (w * w + x * x) - (y * y + z * z);
    R[1] = 2.0 * (x * y - w * z);
    R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z);
    R[4] = (w * w - x * x) + (y * y - z * z);
    R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y);
    R[7] = 2.0 * (y * z + w * x);
    R[8] = (w * w - x * x) - (y * y - z * z);
}

// pose[12] = row-major [R | t] with t = mq - R mp, from the means and the centred cross-covariance
TP3D_HD void horn_pose(const double (&S)[9], const double (&mp)[3], const double (&mq)[3], double (&pose)[12])
{
    double R[9];
    horn_rotation(S, R);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        pose[r * 4 + 0] = R[r * 3 + 0];
        pose[r * 4 + 1] = R[r * 3 + 1];
        pose[r * 4 + 2] = R[r * 3 + 2];
        pose[r * 4 + 3] = mq[r] - ((R[r * 3 + 0] * mp[0] + R[r * 3 + 1] * mp[1]) + R[r * 3 + 2] * mp[2]);
    }
}

}  // namespace tp3d
