// rig_dev.h -- what the rig solvers (pnp_rig.hip, the rig entry point of procrustes.hip) share: the rig row A = {R_A row-major, t_A}
// (A_j maps coordinates in the LAST window frame's camera to coordinates in frame j's camera) applied to a model and to a point, and
// the dimension check of their C-ABI.  ONE definition each: the numpy mirrors restate these operation orders.  FP contract of geom_dev.h.
#pragma once
#include "geom_dev.h"

#define MFR_RIG_MAX_T 16

namespace mfr {

// (R, t) reference -> last frame, seen from frame j: Rc = R_A R, tc = R_A t + t_A.  A = {R_A row-major, t_A}.
MFR_DEV void rig_compose(const double *A, const double *R, const double *t, double *Rc, double *tc)
{
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) Rc[3 * i + c] = (A[3 * i] * R[c] + A[3 * i + 1] * R[3 + c]) + A[3 * i + 2] * R[6 + c];
    rot_apply(A, A + 9, t, tc);
}
// (R', t') reference -> frame j carried to the last frame: R = R_A^T R', t = R_A^T (t' - t_A)
MFR_DEV void rig_to_last(const double *A, const double *Rp, const double *tp, double *R, double *t)
{
    const double d[3] = { tp[0] - A[9], tp[1] - A[10], tp[2] - A[11] };
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int c = 0; c < 3; ++c) R[3 * i + c] = (A[i] * Rp[c] + A[3 + i] * Rp[3 + c]) + A[6 + i] * Rp[6 + c];
        t[i] = (A[i] * d[0] + A[3 + i] * d[1]) + A[6 + i] * d[2];
    }
}
// a point Q in frame j's camera carried into the last frame's camera: Q' = R_A^T (Q - t_A), the translation part of rig_to_last.
// With the identity row Q' = Q exactly.
MFR_DEV void rig_point_to_last(const double *A, const double *Q, double *Ql)
{
    const double d[3] = { Q[0] - A[9], Q[1] - A[10], Q[2] - A[11] };
#pragma unroll
    for (int i = 0; i < 3; ++i) Ql[i] = (A[i] * d[0] + A[3 + i] * d[1]) + A[6 + i] * d[2];
}

}  // namespace mfr

// B T maxN must index as int (the pooled index j maxN + i and the rows do)
static inline bool rig_dims_ok(int B, int T, int maxN)
{
    return B > 0 && T >= 1 && T <= MFR_RIG_MAX_T && maxN > 0 && (long long)B * T * maxN <= 0x7fffffffLL / 3;
}
