// rigid_solve.h -- from the 16 folded float64 sums of a weighted point pairing to the rigid motion (R, t): what rigid_fit.hip
// (targets p + flow) and icp.hip (targets the matched points) share.  Header only, device
// only.  The arithmetic is part of both interfaces (include/hpl_bcl.h); the library builds with -ffp-contract=off, so the
// bits do not depend on which file includes it.
#pragma once
#include "cloud_common.h"

#include <math.h>

namespace hpl {

constexpr int RIGID_SUMS = 16;                       // W, Sp[3], Sq[3], Spq[9]
constexpr int RIGID_SWEEPS = 12;

// The unit quaternion (w, x, y, z) of the proper rotation that maximises tr(R H), H = sum u (p - mp)(q - mq)^T (Horn 1987).
__device__ inline void horn_quaternion(const double *H, double *quat) {
    const double Sxx = H[0], Sxy = H[1], Sxz = H[2], Syx = H[3], Syy = H[4], Syz = H[5], Szx = H[6], Szy = H[7], Szz = H[8];
    double A[4][4] = {{(Sxx + Syy) + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                      {Syz - Szy, (Sxx - Syy) - Szz, Sxy + Syx, Szx + Sxz},
                      {Szx - Sxz, Sxy + Syx, (Syy - Sxx) - Szz, Syz + Szy},
                      {Sxy - Syx, Szx + Sxz, Syz + Szy, (Szz - Sxx) - Syy}};
    double V[4][4];
    jacobi_eigen(A, V, RIGID_SWEEPS);
    int best = 0;                                // the largest eigenvalue; ties go to the smaller index
    double most = A[0][0];
#pragma unroll
    for (int i = 1; i < 4; ++i) {
        best = A[i][i] > most ? i : best;
        most = A[i][i] > most ? A[i][i] : most;
    }
    double n2 = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        quat[k] = best == 0 ? V[k][0] : best == 1 ? V[k][1] : best == 2 ? V[k][2] : V[k][3];
        n2 += quat[k] * quat[k];
    }
    const double inv = (quat[0] < 0.0 ? -1.0 : 1.0) / sqrt(n2);
#pragma unroll
    for (int k = 0; k < 4; ++k) quat[k] *= inv;
}

// tot[16]: W = tot[0] > 0, sum u dp, sum u dq, sum u dp dq^T about the pivot piv -> R[0 .. 8] row-major, R[9 .. 11] = t, the
// rotation angle in degrees and |t|.
__device__ inline void rigid_from_sums(const double *tot, const double *piv, double *R, double &angle, double &tn) {
    const double W = tot[0];
    double mp[3], mq[3], H[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) { mp[i] = tot[1 + i] / W; mq[i] = tot[4 + i] / W; }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) H[3 * i + j] = tot[7 + 3 * i + j] - W * mp[i] * mq[j];
    double q[4];
    horn_quaternion(H, q);
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - w * z);       R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z);       R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y);       R[7] = 2.0 * (y * z + w * x);       R[8] = 1.0 - 2.0 * (x * x + y * y);
    // t = mq - R mp with mp = piv + mp', mq = piv + mq'
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double rp = (R[3 * i] * (piv[0] + mp[0]) + R[3 * i + 1] * (piv[1] + mp[1])) + R[3 * i + 2] * (piv[2] + mp[2]);
        R[9 + i] = (piv[i] + mq[i]) - rp;
    }
    angle = 2.0 * atan2(sqrt((x * x + y * y) + z * z), fabs(w)) * (180.0 / 3.14159265358979323846);
    tn = sqrt((R[9] * R[9] + R[10] * R[10]) + R[11] * R[11]);
}

}  // namespace hpl
