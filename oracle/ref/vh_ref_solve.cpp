/*
 * vh_ref_solve.cpp -- the 6x6 solve step of both trackers through the Eigen the reference vendors
 * (DepthSensingCUDA/Include/Eigen, an include path at build time: nothing of it is copied), in the float32 types and with
 * the calls the reference's host code makes: Matrix<float, 6, 6>::isZero(), JacobiSVD(ComputeFullU | ComputeFullV)
 * .solve(), .singularValues(), .rank(), and AngleAxisf(R).angle().  TEST INFRASTRUCTURE ONLY; tests/icp_reference.py, the
 * float64 restatement of these rules, is held to it.
 */
#include <Eigen/Dense>

typedef Eigen::Matrix<float, 6, 6> Matrix6x6f;
typedef Eigen::Matrix<float, 6, 1> Vector6f;

extern "C" {

/* terms: the 21 upper-triangle ATA entries row by row, then the 6 ATb entries (a wave row's order).  x: SVD.solve(ATb);
 * *cond = evs[0] / evs[5] of the singular values, in float as the reference divides them; *zero = ATA.isZero(), after
 * which the reference does not solve (x = 0, *cond = 0, rank 0 then); returns SVD.rank(). */
int vhr_icp_solve(const float terms[30], float x[6], float* cond, int* zero)
{
    Matrix6x6f ATA;
    Vector6f ATb;
    int k = 0;
    for (int r = 0; r < 6; r++) {
        for (int c = r; c < 6; c++, k++) ATA(r, c) = ATA(c, r) = terms[k];
        ATb(r) = terms[21 + r];
    }
    *zero = ATA.isZero() ? 1 : 0;
    if (*zero) { /* the reference reports lost tracking here and never decomposes such a matrix */
        for (int i = 0; i < 6; i++) x[i] = 0.0f;
        *cond = 0.0f;
        return 0;
    }
    Eigen::JacobiSVD<Matrix6x6f> SVD(ATA, Eigen::ComputeFullU | Eigen::ComputeFullV);
    Vector6f sol = SVD.solve(ATb);
    Vector6f evs = SVD.singularValues();
    for (int i = 0; i < 6; i++) x[i] = sol[i];
    *cond = evs[0] / evs[5];
    return (int)SVD.rank();
}

/* AngleAxisf(R).angle() of a row-major 3x3 */
float vhr_rotation_angle(const float R[9])
{
    Eigen::Matrix3f m;
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) m(r, c) = R[3 * r + c];
    Eigen::AngleAxisf aa(m);
    return aa.angle();
}

} /* extern "C" */
