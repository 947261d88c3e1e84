// vh_solve_6x6.hpp -- the 6x6 symmetric solve that the camera trackers (vh_icp.hip) and the scene registration
// (vh_align.hip) share: written once, so that both take the same step from the same system, bit for bit.
#pragma once

#include "vh_device.hpp"

namespace vhd {

// The 6x6 symmetric system solved through its eigen-decomposition (cyclic Jacobi, double precision):
// x = V diag(1/l_i) V^T b with eigenvalues below 6 eps * l_max (and exact zeros) dropped, which is what Eigen's JacobiSVD::solve returns
// for a symmetric positive semi-definite matrix.  A is destroyed; returns the condition number l_max / l_min.
VHD float icp_solve_6x6(double (&A)[6][6], const double (&b)[6], double (&xs)[6])
{
    // cyclic Jacobi on A (symmetric): A -> diag, V accumulates the rotations
    double V[6][6];
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < 6; j++) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 30; sweep++) {
        double off = 0.0, diag = 0.0;
        for (int i = 0; i < 6; i++) {
            diag += A[i][i] * A[i][i];
            for (int j = i + 1; j < 6; j++) off += A[i][j] * A[i][j];
        }
        if (off <= 1e-26 * diag) break; // eigenvalues to ~1e-13 relative: far below what the float results can show
        for (int p = 0; p < 5; p++)
            for (int q = p + 1; q < 6; q++) {
                if (fabs(A[p][q]) < 1e-300) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
                const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
                for (int k = 0; k < 6; k++) { // columns p, q
                    const double akp = A[k][p], akq = A[k][q];
                    A[k][p] = c * akp - s * akq;
                    A[k][q] = s * akp + c * akq;
                }
                for (int k = 0; k < 6; k++) { // rows p, q
                    const double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = c * apk - s * aqk;
                    A[q][k] = s * apk + c * aqk;
                }
                for (int k = 0; k < 6; k++) {
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq;
                    V[k][q] = s * vkp + c * vkq;
                }
            }
    }
    double lmax = 0.0, lmin = 1e300;
    for (int i = 0; i < 6; i++) { const double l = fabs(A[i][i]); lmax = l > lmax ? l : lmax; lmin = l < lmin ? l : lmin; }
    for (int k = 0; k < 6; k++) xs[k] = 0.0;
    for (int i = 0; i < 6; i++) {
        const double l = fabs(A[i][i]);
        // JacobiSVD::rank() (SVD/JacobiSVD.h:683-691, threshold() :733-738): a singular value counts unless it is exactly
        // zero or strictly below diagSize * epsilon * s_0; one sitting on the threshold is kept
        if (l == 0.0 || l < 6.0 * 1.1920928955078125e-7 * lmax) continue;
        double proj = 0.0;
        for (int k = 0; k < 6; k++) proj += V[k][i] * b[k];
        proj /= A[i][i];
        for (int k = 0; k < 6; k++) xs[k] += V[k][i] * proj;
    }
    return (float)(lmax / lmin);
}

} // namespace vhd
