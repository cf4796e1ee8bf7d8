// pnp_dev.h -- what the single-camera PnP solver (pnp.hip) and the rig solver (pnp_rig.hip) share above solver_dev.h: the depth-lift
// kernel and the Levenberg-Marquardt refinement of a pose (R, t) on the reprojection error over an inlier list.  ONE definition each.
//
// pnp_lift_kernel: `rows_per_ref` consecutive rows share one reference view (depth map, its minimum, K0): 1 for pairs, T for a rig's
// window frames.
//
// pnp_lm: what differs between the two solvers is where the point R X + t is seen from, which is the `Cam` parameter:
//     cam.kd(j, Kd)      {fx, fy, cx, cy} of the camera that observed point j
//     cam.to_cam(j, Y)   Y = R X + t (the model's frame) -> the observing camera's frame, in place
//     cam.jac(j, G)      the 3 x 6 derivative of Y by the six pose parameters -> that of the transformed point, in place
// PnpOneCamera does nothing in to_cam / jac, so pnp.hip's arithmetic is the sequence of operations it always was (the CPU oracle's
// mfr_ref_pnp_lm, bit for bit).  Wave-parallel with the deterministic wave64 reduction order of wave_sum.  FP contract of geom_dev.h.
#pragma once
#include "solver_dev.h"

// ------------------------------------------------------------------------------------------
// one workgroup per row; order-preserving compaction of the valid correspondences
static __global__ void __launch_bounds__(256) pnp_lift_kernel(
    const float *__restrict__ pts0, const float *__restrict__ pts1, const int32_t *__restrict__ n_corr, int maxN,
    const float *__restrict__ depth0, const float *__restrict__ partial_min, int H, int W,
    const void *__restrict__ K0, int k_dtype, int rows_per_ref, double *__restrict__ xyz, double *__restrict__ obs,
    int32_t *__restrict__ src_idx, int32_t *__restrict__ n_valid)
{
    const int b = blockIdx.x, tid = threadIdx.x, ref = b / rows_per_ref;
    int n = n_corr[b];
    if (n > maxN) n = maxN;
    __shared__ mfr::Compact256 cs;
    const float dmin = mfr::depth_min_fold(partial_min, ref);
    double Ki[4];
    mfr::kinv(K0, k_dtype, ref, Ki);
    const float *p0 = pts0 + (size_t)b * maxN * 2, *p1 = pts1 + (size_t)b * maxN * 2;
    const float *dm = depth0 + (size_t)ref * H * W;
    double *oxyz = xyz + (size_t)b * maxN * 3, *oobs = obs + (size_t)b * maxN * 2;
    int32_t *osrc = src_idx + (size_t)b * maxN;
    int total = 0;
    for (int start = 0; start < n; start += 256) {
        const int i = start + tid;
        double X[3];
        const bool valid = i < n && mfr::lift_point(p0[2 * i], p0[2 * i + 1], dm, H, W, dmin, Ki, X);   // :186-206 (Q1, Q6), :6-17
        const int m = mfr::compact256_slot(cs, valid, total);
        if (valid) {
            oxyz[3 * m] = X[0]; oxyz[3 * m + 1] = X[1]; oxyz[3 * m + 2] = X[2];
            oobs[2 * m] = (double)p1[2 * i]; oobs[2 * m + 1] = (double)p1[2 * i + 1];
            osrc[m] = i;
        }
    }
    if (tid == 0) n_valid[b] = total;
}

namespace mfr {

// ------------------------------------------------------------------------------------------
// the model IS the camera pose: one K for every point
struct PnpOneCamera {
    const double *Kd;
    __device__ __forceinline__ void kd(int, double out[4]) const { out[0] = Kd[0]; out[1] = Kd[1]; out[2] = Kd[2]; out[3] = Kd[3]; }
    __device__ __forceinline__ void to_cam(int, double *) const {}
    __device__ __forceinline__ void jac(int, double (*)[6]) const {}
};

template <class Cam>
MFR_DEV double pnp_cost(const double *X, const double *O, const int32_t *idx, int n, const Cam &cam, const double *R, const double *t)
{
    double acc = 0.0;
    for (int i = lane_id(); i < n; i += 64) {
        const int j = idx[i];
        double Kd[4], Y[3];
        cam.kd(j, Kd);
        rot_apply(R, t, X + 3 * (size_t)j, Y);
        cam.to_cam(j, Y);
        acc = acc + cam_err2(Y, O + 2 * (size_t)j, Kd);
    }
    return wave_sum(acc);
}

// Stands in for the EPnP refit inside cv::solvePnPRansac and for cv.solvePnPGeneric(ITERATIVE) (pose_solver.py:216-220).
// X, O are indexed by the entries of idx.  -1 when the starting cost is not finite.
template <class Cam>
MFR_DEV_NOINLINE int pnp_lm(const double *X, const double *O, const int32_t *idx, int n_idx, const Cam &cam, int max_iter, double *R, double *t)
{
    LmDamping lm;
    double cost = pnp_cost(X, O, idx, n_idx, cam, R, t);
    if (!(cost == cost) || !(cost < 1e300)) return -1;
    for (int it = 0; it < max_iter; ++it) {
        double acc[27];
#pragma unroll
        for (int q = 0; q < 27; ++q) acc[q] = 0.0;
        for (int i = lane_id(); i < n_idx; i += 64) {
            const int j = idx[i];
            const double *P = X + 3 * (size_t)j, *x = O + 2 * (size_t)j;
            double Kd[4], Y[3];
            cam.kd(j, Kd);
            rot_apply(R, t, P, Y);
            cam.to_cam(j, Y);
            const double iz = (Y[2] != 0.0) ? 1.0 / Y[2] : 1.0;
            const double xn = Y[0] * iz, yn = Y[1] * iz;
            const double ru = (Kd[0] * xn + Kd[2]) - x[0];
            const double rv = (Kd[1] * yn + Kd[3]) - x[1];
            const double a0[3] = { 0.0, -P[2], P[1] }, a1[3] = { P[2], 0.0, -P[0] }, a2[3] = { -P[1], P[0], 0.0 };
            double G[3][6];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                G[r][0] = (R[3 * r] * a0[0] + R[3 * r + 1] * a0[1]) + R[3 * r + 2] * a0[2];
                G[r][1] = (R[3 * r] * a1[0] + R[3 * r + 1] * a1[1]) + R[3 * r + 2] * a1[2];
                G[r][2] = (R[3 * r] * a2[0] + R[3 * r + 1] * a2[1]) + R[3 * r + 2] * a2[2];
                G[r][3] = (r == 0) ? 1.0 : 0.0; G[r][4] = (r == 1) ? 1.0 : 0.0; G[r][5] = (r == 2) ? 1.0 : 0.0;
            }
            cam.jac(j, G);
            const double pu0 = Kd[0] * iz, pu2 = -(Kd[0] * xn) * iz;
            const double pv1 = Kd[1] * iz, pv2 = -(Kd[1] * yn) * iz;
            double Ju[6], Jv[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                Ju[k] = pu0 * G[0][k] + pu2 * G[2][k];
                Jv[k] = pv1 * G[1][k] + pv2 * G[2][k];
            }
            int q = 0;
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int c = r; c < 6; ++c, ++q) acc[q] = acc[q] + (Ju[r] * Ju[c] + Jv[r] * Jv[c]);
#pragma unroll
            for (int r = 0; r < 6; ++r, ++q) acc[q] = acc[q] + (Ju[r] * ru + Jv[r] * rv);
        }
#pragma unroll
        for (int q = 0; q < 27; ++q) acc[q] = wave_sum(acc[q]);
        double Hm[36], g[6], dlt[6];
        lm6_unpack(acc, Hm, g);
        lm.damp(Hm);
        if (chol_solve6(Hm, g, dlt)) {
            if (lm.reject()) break;
            continue;
        }
        double Rn[9], tn[3];
        quat_right_update(R, dlt, Rn);
        tn[0] = t[0] + dlt[3]; tn[1] = t[1] + dlt[4]; tn[2] = t[2] + dlt[5];
        const double cn = pnp_cost(X, O, idx, n_idx, cam, Rn, tn);
        if (cn < cost) {
            for (int k = 0; k < 9; ++k) R[k] = Rn[k];
            for (int k = 0; k < 3; ++k) t[k] = tn[k];
            const bool done = lm.accept(cost - cn, 1e-14 * cost);
            cost = cn;
            if (done) break;
        } else if (lm.reject()) break;
        if (lm6_max_abs(dlt) < 1e-13) break;
    }
    return 0;
}

}  // namespace mfr
