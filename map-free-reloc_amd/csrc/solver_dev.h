// solver_dev.h -- the pieces the f64 pose solvers share above the per-lane geometry of geom_dev.h: the 4x4 Jacobi eigen-solve and Horn's
// Kabsch on it, the replay of OpenCV's RANSAC loop over precomputed counts, the 6-parameter Levenberg-Marquardt pieces, the depth lift
// of one keypoint.  ONE definition each: the solvers equal the CPU oracle bit for bit.  FP contract of geom_dev.h.
#pragma once
#include "geom_dev.h"

namespace mfr {

// ---------------------------------------------------------------- symmetric 4x4 eigenproblem
// cyclic Jacobi, SWEEPS sweeps over the 6 off-diagonal entries; on return the diagonal of A holds the eigenvalues and the COLUMNS of V
// the eigenvectors.  A rotation whose angle underflows (theta^2 = inf) is the identity; NaN input gives NaN output after the same work.
// Unrolled: every index into A and V is static, so both stay in registers.
template <int SWEEPS>
MFR_DEV void jacobi4(double A[4][4], double V[4][4])
{
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) V[i][j] = (i == j) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < SWEEPS; ++sweep) {
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                const double apq = A[p][q];
                if (apq == 0.0) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
                const double at = theta < 0.0 ? -theta : theta;
                double t = 1.0 / (at + sqrt(theta * theta + 1.0));
                if (theta < 0.0) t = -t;
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const double akp = A[k][p], akq = A[k][q];
                    A[k][p] = c * akp - s * akq; A[k][q] = s * akp + c * akq;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = c * apk - s * aqk; A[q][k] = s * apk + c * aqk;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq;
                }
            }
    }
}
// column of the largest (want_max) or smallest eigenvalue, first index on ties (np.argmax / the last row of vh); selected by compares
template <int SWEEPS>
MFR_DEV void jacobi4_pick(double A[4][4], bool want_max, double v[4])
{
    double V[4][4];
    jacobi4<SWEEPS>(A, V);
    int best = 0;
#pragma unroll
    for (int i = 1; i < 4; ++i)
        if (want_max ? (A[i][i] > A[best][best]) : (A[i][i] < A[best][best])) best = i;
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = (best == 0) ? V[k][0] : (best == 1) ? V[k][1] : (best == 2) ? V[k][2] : V[k][3];
}

// Horn's closed-form absolute orientation q = R p + t from the 16 moments s = {n, sum p, sum q, sum p q^T}: the rotation is the unit
// quaternion of the largest eigenvalue of N (10 Jacobi sweeps, the column divided by its norm).  Twin: the oracle's kabsch_from_moments.
MFR_DEV_NOINLINE void kabsch_from_moments(const double *s, double *R, double *t)
{
    const double n = s[0], pc[3] = { s[1] / n, s[2] / n, s[3] / n }, qc[3] = { s[4] / n, s[5] / n, s[6] / n };
    double S[3][3];
    for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) S[a][b] = s[7 + 3 * a + b] - n * pc[a] * qc[b];
    double N[4][4];
    N[0][0] = (S[0][0] + S[1][1]) + S[2][2];
    N[0][1] = S[1][2] - S[2][1]; N[0][2] = S[2][0] - S[0][2]; N[0][3] = S[0][1] - S[1][0];
    N[1][1] = (S[0][0] - S[1][1]) - S[2][2]; N[1][2] = S[0][1] + S[1][0]; N[1][3] = S[2][0] + S[0][2];
    N[2][2] = (-S[0][0] + S[1][1]) - S[2][2]; N[2][3] = S[1][2] + S[2][1];
    N[3][3] = (-S[0][0] - S[1][1]) + S[2][2];
    for (int i = 0; i < 4; ++i) for (int j = 0; j < i; ++j) N[i][j] = N[j][i];
    double v[4];
    jacobi4_pick<10>(N, true, v);
    const double nn = sqrt(((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) + v[3] * v[3]);
    const double w = v[0] / nn, x = v[1] / nn, y = v[2] / nn, z = v[3] / nn;
    R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - w * z);       R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z);       R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y);       R[7] = 2.0 * (y * z + w * x);       R[8] = 1.0 - 2.0 * (x * x + y * y);
    for (int i = 0; i < 3; ++i) t[i] = qc[i] - ((R[3 * i] * pc[0] + R[3 * i + 1] * pc[1]) + R[3 * i + 2] * pc[2]);
}

// ---------------------------------------------------------------- RANSAC replay over precomputed counts
// What RANSACPointSetRegistrator::run's sequential loop does with cnt[0 .. max_iters): iteration `it` becomes the best model when cnt[it]
// beats every earlier count and model_points - 1, and then lowers the iteration cap (update_num_iters); the loop ends at the cap.  One
// wavefront, every lane in step (all results wave-uniform): per chunk of 64 counts a prefix-max scan marks the records of the running
// maximum, which are then taken in order while they lie below the cap.  Returns the loop's exit index (iterations run); `best` is the
// winning count (model_points - 1 if none), `bit` its iteration (-1 if none).
MFR_DEV int ransac_replay_counts(const int32_t *__restrict__ cnt, int max_iters, int n, double conf, int model_points, int &best, int &bit)
{
    const int lane = lane_id();
    int niters = max_iters, carry = model_points - 1;
    bool stop = false;
    best = model_points - 1; bit = -1;
    for (int c0 = 0; c0 < max_iters && !stop && c0 < niters; c0 += 64) {
        const int it = c0 + lane;
        const int v = (it < max_iters) ? cnt[it] : -1;
        int incl = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_up(incl, off, 64);
            if (lane >= off && o > incl) incl = o;
        }
        int excl = __shfl_up(incl, 1, 64);
        if (lane == 0 || excl < carry) excl = carry;
        unsigned long long rec = __ballot(v > excl);
        while (rec) {
            const int l = __ffsll((long long)rec) - 1;
            rec &= rec - 1;
            const int itr = c0 + l;
            if (itr >= niters) { stop = true; break; }
            best = __shfl(v, l, 64);
            bit = itr;
            niters = update_num_iters(conf, (double)(n - best) / (double)n, model_points, niters);
        }
        const int last = __shfl(incl, 63, 64);
        if (last > carry) carry = last;
    }
    return (bit + 1 > niters) ? bit + 1 : niters;
}

// ---------------------------------------------------------------- 6-parameter Levenberg-Marquardt pieces
// The normal equations travel as 27 sums: the 21 entries of the upper triangle of J^T J row by row, then the 6 of J^T r.  Each solver
// keeps its own loop (gauge term, renormalisation, exit tolerance and reduction width differ) and calls these.
// one residual row: acc += w J J^T, w J r (the weight multiplies J[rr] first)
MFR_DEV void lm6_accumulate(double acc[27], const double J[6], double r, double w = 1.0)
{
    int q = 0;
#pragma unroll
    for (int rr = 0; rr < 6; ++rr) {
        const double wj = w * J[rr];
#pragma unroll
        for (int cc = rr; cc < 6; ++cc, ++q) acc[q] = acc[q] + wj * J[cc];
    }
#pragma unroll
    for (int rr = 0; rr < 6; ++rr, ++q) acc[q] = acc[q] + (w * J[rr]) * r;
}
// the reduced sums as the symmetric H and the right-hand side g = -J^T r of H dl = g
MFR_DEV void lm6_unpack(const double acc[27], double H[36], double g[6])
{
    int qq = 0;
    for (int rr = 0; rr < 6; ++rr)
        for (int cc = rr; cc < 6; ++cc, ++qq) { H[6 * rr + cc] = acc[qq]; H[6 * cc + rr] = acc[qq]; }
    for (int rr = 0; rr < 6; ++rr, ++qq) g[rr] = -acc[qq];
}
MFR_DEV double lm6_max_abs(const double dl[6])
{
    double mx = 0.0;
    for (int k = 0; k < 6; ++k) { const double a = dl[k] < 0.0 ? -dl[k] : dl[k]; if (a > mx) mx = a; }
    return mx;
}
// Marquardt's damping H_ii += lambda H_ii; reject() and accept() move lambda and return whether the iteration ends
struct LmDamping {
    double lambda = 1e-3;
    __device__ __forceinline__ void damp(double H[36]) const
    {
        for (int rr = 0; rr < 6; ++rr) H[6 * rr + rr] = H[6 * rr + rr] + lambda * H[6 * rr + rr];
    }
    __device__ __forceinline__ bool reject()                   // no step, or a step that did not lower the cost
    {
        lambda = lambda * 10.0;
        return lambda > 1e12;
    }
    __device__ __forceinline__ bool accept(double dec, double tol)      // the cost fell by dec
    {
        lambda = lambda * 0.1;
        if (lambda < 1e-12) lambda = 1e-12;
        return dec <= tol;
    }
};

// ---------------------------------------------------------------- depth lift of one keypoint
// np.int32 truncation of (px, py), depth gather, valid if inside the map and above dmin, X = depth * inv(K) [u, v, 1]
// (pose_solver.py:186-206 with dmin = depth.min(), quirk Q6; :138-151 with dmin = 0).  No branch: a keypoint outside the map reads
// pixel 0 and is invalid, so the gathers of a correspondence's two views are in flight together.  X means nothing unless valid.
MFR_DEV bool lift_point(float px, float py, const float *__restrict__ depth, int H, int W, float dmin, const double Ki[4], double X[3])
{
    int u = 0, v = 0;
    const bool inu = pix_trunc(px, W, u), inv = pix_trunc(py, H, v), inside = inu && inv;
    const float d = depth[inside ? v * W + u : 0];
    backproject(u, v, d, Ki, X);
    return inside && d > dmin;
}

}  // namespace mfr
