// emat_dev.h -- per-lane essential-matrix geometry for the score, select and scale kernels (gfx950): the Sampson distance and
// its Jacobian, [t]x R, the decomposition of E and the cheirality test.  The 5-point solver itself is emat_lds.h.
// Device statement of EssentialMatrixSolver's arithmetic (lib/models/matching/pose_solver.py:29-61;
// cv.findEssentialMat / cv.recoverPose restated from the published algorithms, see emat.hip).
// Same FP contract as geom_dev.h (binary64, + - * / sqrt only, no FMA contraction, fixed order).
#pragma once
#include "solver_dev.h"

namespace mfr {

// pose_solver.py:39-43 in the dtype K arrives in: numpy float32 arithmetic for a float32 K, float64 (keypoints widened) for the Map-free
// loader's float64 K; the threshold mean likewise.  K0 row b0 / K1 row b1 (the rig solver has one K0 per sample, one K1 per frame).
// thr^2 with thr = PIX_THRESHOLD / mean(fx0, fy1, fy0, fx1) (:43, Q8)
MFR_DEV double emat_thr2(const void *K0, int b0, const void *K1, int b1, int k_dtype, double pix_thr)
{
    double thr;
    if (k_dtype == MFR_K_F32) {
        const float *k0 = (const float *)K0 + 9 * (size_t)b0, *k1 = (const float *)K1 + 9 * (size_t)b1;
        const float m = (((k0[0] + k1[4]) + k0[4]) + k1[0]) / 4.0f;       // np.mean([fx0, fy1, fy0, fx1]) in f32
        thr = pix_thr / (double)m;
    } else {
        const double *k0 = (const double *)K0 + 9 * (size_t)b0, *k1 = (const double *)K1 + 9 * (size_t)b1;
        const double m = (((k0[0] + k1[4]) + k0[4]) + k1[0]) / 4.0;
        thr = pix_thr / m;
    }
    return thr * thr;
}
// one correspondence p0 <-> p1 (pixels) K-normalised (:39-40): x = {x0, y0, x1, y1}
MFR_DEV void emat_normalize(const float *p0, const float *p1, const void *K0, int b0, const void *K1, int b1, int k_dtype, double x[4])
{
    if (k_dtype == MFR_K_F32) {
        const float *k0 = (const float *)K0 + 9 * (size_t)b0, *k1 = (const float *)K1 + 9 * (size_t)b1;
        x[0] = (double)((p0[0] - k0[2]) / k0[0]); x[1] = (double)((p0[1] - k0[5]) / k0[4]);
        x[2] = (double)((p1[0] - k1[2]) / k1[0]); x[3] = (double)((p1[1] - k1[5]) / k1[4]);
    } else {
        const double *k0 = (const double *)K0 + 9 * (size_t)b0, *k1 = (const double *)K1 + 9 * (size_t)b1;
        x[0] = ((double)p0[0] - k0[2]) / k0[0]; x[1] = ((double)p0[1] - k0[5]) / k0[4];
        x[2] = ((double)p1[0] - k1[2]) / k1[0]; x[3] = ((double)p1[1] - k1[5]) / k1[4];
    }
}

MFR_DEV double sampson2(const double *E, double a, double b, double c, double d)
{
    const double Ex0 = (E[0] * a + E[1] * b) + E[2], Ex1 = (E[3] * a + E[4] * b) + E[5], Ex2 = (E[6] * a + E[7] * b) + E[8];
    const double Et0 = (E[0] * c + E[3] * d) + E[6], Et1 = (E[1] * c + E[4] * d) + E[7];
    const double num = (c * Ex0 + d * Ex1) + Ex2;
    const double den = ((Ex0 * Ex0 + Ex1 * Ex1) + Et0 * Et0) + Et1 * Et1;
    return (num * num) / den;
}

// the Sampson residual r = num / sqrt(den) of one correspondence (a, b) <-> (c, d) under E = [t]x R, and its Jacobian J[6] with respect
// to a right rotation update (J[0..2]) and a translation update (J[3..5]); r * r = sampson2(E, a, b, c, d) up to rounding
MFR_DEV void sampson_jac(const double *E, const double *R, const double *t, double a, double b, double c, double d, double J[6], double &r)
{
    const double Ex0 = (E[0] * a + E[1] * b) + E[2], Ex1 = (E[3] * a + E[4] * b) + E[5], Ex2 = (E[6] * a + E[7] * b) + E[8];
    const double Et0 = (E[0] * c + E[3] * d) + E[6], Et1 = (E[1] * c + E[4] * d) + E[7];
    const double num = (c * Ex0 + d * Ex1) + Ex2;
    const double den = ((Ex0 * Ex0 + Ex1 * Ex1) + Et0 * Et0) + Et1 * Et1;
    const double wgt = 1.0 / sqrt(den);
    const double q[3] = { c, d, 1.0 }, p[3] = { a, b, 1.0 };
    const double txq[3] = { t[1] * q[2] - t[2] * q[1], t[2] * q[0] - t[0] * q[2], t[0] * q[1] - t[1] * q[0] };
    const double u[3] = { -((R[0] * txq[0] + R[3] * txq[1]) + R[6] * txq[2]),
                          -((R[1] * txq[0] + R[4] * txq[1]) + R[7] * txq[2]),
                          -((R[2] * txq[0] + R[5] * txq[1]) + R[8] * txq[2]) };
    const double Rp[3] = { (R[0] * p[0] + R[1] * p[1]) + R[2] * p[2], (R[3] * p[0] + R[4] * p[1]) + R[5] * p[2],
                           (R[6] * p[0] + R[7] * p[1]) + R[8] * p[2] };
    J[0] = (p[1] * u[2] - p[2] * u[1]) * wgt; J[1] = (p[2] * u[0] - p[0] * u[2]) * wgt; J[2] = (p[0] * u[1] - p[1] * u[0]) * wgt;
    J[3] = (Rp[1] * q[2] - Rp[2] * q[1]) * wgt; J[4] = (Rp[2] * q[0] - Rp[0] * q[2]) * wgt; J[5] = (Rp[0] * q[1] - Rp[1] * q[0]) * wgt;
    r = num * wgt;
}

MFR_DEV void skew_mul(const double *t, const double *R, double *E)
{
    for (int j = 0; j < 3; ++j) {
        E[j]     = t[1] * R[6 + j] - t[2] * R[3 + j];
        E[3 + j] = t[2] * R[j]     - t[0] * R[6 + j];
        E[6 + j] = t[0] * R[3 + j] - t[1] * R[j];
    }
}

// Horn 1990 closed-form decomposition (stands in for the SVD inside cv::recoverPose)
MFR_DEV int emat_decompose(const double *E, double *Ra, double *Rb, double *tu)
{
    double EEt[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            EEt[3 * i + j] = (E[3 * i] * E[3 * j] + E[3 * i + 1] * E[3 * j + 1]) + E[3 * i + 2] * E[3 * j + 2];
    const double htr = 0.5 * ((EEt[0] + EEt[4]) + EEt[8]);
    double bb[9];
    for (int i = 0; i < 9; ++i) bb[i] = -EEt[i];
    bb[0] = bb[0] + htr; bb[4] = bb[4] + htr; bb[8] = bb[8] + htr;
    // column k of bb with the largest diagonal entry -- by selects, not by an index into the local array (a run-time index puts bb in scratch)
    int k = 0;
    double dk = bb[0];
    if (bb[4] > dk) { k = 1; dk = bb[4]; }
    if (bb[8] > dk) { k = 2; dk = bb[8]; }
    if (!(dk > 0.0)) return -1;
    const double s = sqrt(dk);
    const double c0 = k == 0 ? bb[0] : k == 1 ? bb[1] : bb[2], c1 = k == 0 ? bb[3] : k == 1 ? bb[4] : bb[5], c2 = k == 0 ? bb[6] : k == 1 ? bb[7] : bb[8];
    const double b[3] = { c0 / s, c1 / s, c2 / s };
    double C[9];
    C[0] = E[4] * E[8] - E[5] * E[7]; C[1] = -(E[3] * E[8] - E[5] * E[6]); C[2] = E[3] * E[7] - E[4] * E[6];
    C[3] = -(E[1] * E[8] - E[2] * E[7]); C[4] = E[0] * E[8] - E[2] * E[6]; C[5] = -(E[0] * E[7] - E[1] * E[6]);
    C[6] = E[1] * E[5] - E[2] * E[4]; C[7] = -(E[0] * E[5] - E[2] * E[3]); C[8] = E[0] * E[4] - E[1] * E[3];
    double bE[9];
    skew_mul(b, E, bE);
    const double b2 = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2];
    for (int i = 0; i < 9; ++i) { Ra[i] = (C[i] - bE[i]) / b2; Rb[i] = (C[i] + bE[i]) / b2; }
    const double nb = sqrt(b2);
    tu[0] = b[0] / nb; tu[1] = b[1] / nb; tu[2] = b[2] / nb;
    return 0;
}

// closest-point depths along both rays > 0 (cheirality vote of cv::recoverPose)
MFR_DEV bool cheirality(const double *R, const double *t, double a, double b, double c, double d)
{
    const double p[3] = { (R[0] * a + R[1] * b) + R[2], (R[3] * a + R[4] * b) + R[5], (R[6] * a + R[7] * b) + R[8] };
    const double q[3] = { c, d, 1.0 };
    const double pp = (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2], qq = (q[0] * q[0] + q[1] * q[1]) + q[2] * q[2];
    const double pq = (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2];
    const double pt = (p[0] * t[0] + p[1] * t[1]) + p[2] * t[2], qt = (q[0] * t[0] + q[1] * t[1]) + q[2] * t[2];
    const double det = pp * qq - pq * pq;
    if (!(det > 1e-18 * pp * qq)) return false;
    const double l0 = (pq * qt - qq * pt) / det;
    const double l1 = (pp * qt - pq * pt) / det;
    return (l0 > 0.0) && (l1 > 0.0);
}

}  // namespace mfr
