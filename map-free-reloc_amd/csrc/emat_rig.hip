// emat_rig.hip -- essential-matrix pose for a calibrated camera RIG on gfx950 (MI355X): one METRIC pose for T query frames, no depth.
//
// POSE_SOLVER 'RigEssentialMatrix' of the multi-frame model.  A rig with known metric baselines makes the scale of an essential-matrix
// solution observable (Clipp et al. 2008: five points in one camera, the other cameras fix the scale).  Upstream has no such solver; the
// yardsticks are the numpy mirror tests/rig_emat_ref.py and, with T = 1, the single-frame solver bit for bit.
//
// Stage 1 (emat.hip, unchanged): mfr_emat_solve_batch over the B T rows (frame j of sample b = row b T + j, RANSAC key pair_id T + j):
// per frame (R'_j, unit u_j, inlier count, inlier mask, status), all on the device.
// Stage 2 (this file), per sample, deterministic, no random numbers.  Rig row A_j = (R_Aj, t_Aj): last frame's camera -> frame j's; the
// model is (R, t) reference -> LAST frame, frame j sees it as (R_Aj R, R_Aj t + t_Aj) (rig_dev.h).
//   T = 1            the frame's (R', u), count, mask and status pass through bit for bit (no rig, no scale: the unit translation)
//   usable frames    those whose stage-1 status is OK.  T > 1 and fewer than two: MFR_ST_NO_MODEL -- or, when no frame is usable and all
//                    failed the same way, that status -- NaN pose, 0 inliers
//   erig_hyp_kernel  every unordered pair (j < k) of usable frames in combinations order, for each the rotation of j then of k:
//                    hypothesis h = 2 pair + {0, 1}, at most T (T - 1) = 240.  R_h = R_Am^T R'_m; t_h = the least-squares solution of
//                    u_f x (R_Af t + t_Af) = 0 over f in {j, k}: M t = -c with M = sum R_Af^T P_f R_Af, c = sum R_Af^T P_f t_Af,
//                    P_f = I - u_f u_f^T, solved by cofactors.  M has the eigenvalues 2, 1 + cos, 1 - cos of the angle between the two
//                    translation directions seen from the last frame: det M = 2 sin^2.  The hypothesis is SKIPPED (score -1) when
//                    det M <= ER_DET_REL (tr M / 3)^3 with ER_DET_REL = 1e-6 -- directions within about 1e-3 rad of parallel, where a
//                    bearing error of a five-point solution (1e-3 rad at best) moves the intersection by more than its distance -- and
//                    when (R_Af t + t_Af) . u_f <= 0 for either frame (the intersection lies behind a frame's bearing)
//   erig_score_kernel  one wavefront per hypothesis over ALL frames' correspondences (non-usable frames too, as rig PnP counts every
//                    frame), points K-normalised (emat_dev.h: emat_prep_kernel's arithmetic, per frame, in K's dtype) and staged in LDS per
//                    frame tile of 1024; per frame E_k = [t_k / |t_k|]x R_k of the composed model, a frame with |t_k| < ER_T_FLOOR = 1e-12
//                    contributes nothing; a point counts when sampson2 < thr2_k and cheirality holds.  The pooled count wins, the first
//                    maximum on a tie
//   erig_select_kernel  pooled inlier list in (frame, index) order; with 6 or more inliers Levenberg-Marquardt over the six pose parameters
//                    on the signed Sampson residuals, each through its frame's composed (R_k, t_k), sampson_jac chained through rig_compose
//                    (rotation: the same right update; translation: J_t R_Ak).  The translation is NOT renormalised and there is no gauge
//                    term: the known t_Ak make all six parameters observable.  Damping and schedule: the COUNT-score polish of emat.hip
//                    (LmDamping, at most 20 iterations, accept tolerance 1e-14 cost, step exit 1e-13).  Sums: lane l adds the pooled
//                    inliers l, l + 64, ... in order, then the wavefront butterfly.  Re-score under the refined model: n_inliers and the
//                    [B T, maxN] mask are that pooled set.  A non-finite pose or |t| > 1000 gives MFR_ST_DEGENERATE.
//
// This TU is compiled with -ffp-contract=off (see geom_dev.h for the FP contract).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mfr_hip.h"
#include "zero_fill.h"
#include "emat_dev.h"
#include "rig_dev.h"

using namespace mfr;

#define ER_HYP_WG 16                                      // hypotheses per workgroup of erig_score_kernel: 4 wavefronts, 4 each
#define ER_TILE 1024
#define ER_MAX_HYP (MFR_RIG_MAX_T * (MFR_RIG_MAX_T - 1))  // 240
#define ER_DET_REL 1e-6
#define ER_T_FLOOR 1e-12

// bit j set: frame j of the sample is usable
MFR_DEV unsigned erig_usable(const int32_t *st1, int T)
{
    unsigned um = 0;
    for (int j = 0; j < T; ++j)
        if (st1[j] == MFR_ST_OK) um |= 1u << j;
    return um;
}

// hypothesis of the frame pair (fa < fb), rotation of fa (which = 0) or fb (1); 0 when skipped (header)
MFR_DEV int erig_hypothesis(const double *rig, const double *R1, const double *t1, int fa, int fb, int which, double *R, double *t)
{
    const int m = which ? fb : fa;
    const double zero[3] = { 0.0, 0.0, 0.0 };
    double unused[3];
    rig_to_last(rig + 12 * m, R1 + 9 * m, zero, R, unused);
    double M[9], c[3];
    for (int k = 0; k < 9; ++k) M[k] = 0.0;
    for (int k = 0; k < 3; ++k) c[k] = 0.0;
    for (int s = 0; s < 2; ++s) {
        const int f = s ? fb : fa;
        const double *A = rig + 12 * f, *u = t1 + 3 * f;
        double P[9], PA[9], Pt[3];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) P[3 * i + j] = ((i == j) ? 1.0 : 0.0) - u[i] * u[j];
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) PA[3 * i + j] = (P[3 * i] * A[j] + P[3 * i + 1] * A[3 + j]) + P[3 * i + 2] * A[6 + j];
            Pt[i] = (P[3 * i] * A[9] + P[3 * i + 1] * A[10]) + P[3 * i + 2] * A[11];
        }
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) M[3 * i + j] = M[3 * i + j] + ((A[i] * PA[j] + A[3 + i] * PA[3 + j]) + A[6 + i] * PA[6 + j]);
            c[i] = c[i] + ((A[i] * Pt[0] + A[3 + i] * Pt[1]) + A[6 + i] * Pt[2]);
        }
    }
    const double C0 = M[4] * M[8] - M[5] * M[7], C1 = M[5] * M[6] - M[3] * M[8], C2 = M[3] * M[7] - M[4] * M[6];
    const double det = (M[0] * C0 + M[1] * C1) + M[2] * C2;
    const double tr3 = ((M[0] + M[4]) + M[8]) / 3.0;
    if (!(det > ER_DET_REL * ((tr3 * tr3) * tr3))) return 0;
    const double inv[9] = { C0, M[2] * M[7] - M[1] * M[8], M[1] * M[5] - M[2] * M[4],
                            C1, M[0] * M[8] - M[2] * M[6], M[2] * M[3] - M[0] * M[5],
                            C2, M[1] * M[6] - M[0] * M[7], M[0] * M[4] - M[1] * M[3] };
    const double b0 = -c[0], b1 = -c[1], b2 = -c[2];
    for (int i = 0; i < 3; ++i) t[i] = ((inv[3 * i] * b0 + inv[3 * i + 1] * b1) + inv[3 * i + 2] * b2) / det;
    for (int s = 0; s < 2; ++s) {
        const int f = s ? fb : fa;
        const double *A = rig + 12 * f;
        double y[3];
        rot_apply(A, A + 9, t, y);
        if (!(dot3(y, t1 + 3 * f) > 0.0)) return 0;
    }
    return 1;
}

// grid (B), one thread per hypothesis: models [B, NH, 12], counts [B, NH] = 0 (to be scored) or -1 (skipped / no such pair); NH = T (T - 1)
__global__ void __launch_bounds__(256) erig_hyp_kernel(const double *__restrict__ R1, const double *__restrict__ t1,
                                                       const int32_t *__restrict__ st1, int T, const double *__restrict__ rig,
                                                       double *__restrict__ models, int32_t *__restrict__ counts)
{
    const int b = blockIdx.x, h = threadIdx.x, NH = T * (T - 1);
    if (h >= NH) return;
    const size_t row0 = (size_t)b * T;
    const unsigned um = erig_usable(st1 + row0, T);
    int fa = -1, fb = -1, pair = 0;
    for (int j = 0; j < T; ++j)
        for (int k = j + 1; k < T; ++k)
            if (((um >> j) & 1u) && ((um >> k) & 1u)) {
                if (pair == (h >> 1)) { fa = j; fb = k; }
                ++pair;
            }
    double R[9], t[3];
    int ok = 0;
    if (fa >= 0) ok = erig_hypothesis(rig + row0 * 12, R1 + row0 * 9, t1 + row0 * 3, fa, fb, h & 1, R, t);
    counts[(size_t)b * NH + h] = ok ? 0 : -1;
    if (ok) {
        double *o = models + ((size_t)b * NH + h) * 12;
        for (int k = 0; k < 9; ++k) o[k] = R[k];
        for (int k = 0; k < 3; ++k) o[9 + k] = t[k];
    }
}

// the model seen from a frame, ready to score: E = [tc / |tc|]x Rc; false when |tc| < ER_T_FLOOR
MFR_DEV bool erig_frame_model(const double *A, const double *R, const double *t, double *E, double *Rc, double *tn)
{
    double tc[3];
    rig_compose(A, R, t, Rc, tc);
    const double nt = sqrt(dot3(tc, tc));
    if (!(nt >= ER_T_FLOOR)) return false;
    tn[0] = tc[0] / nt; tn[1] = tc[1] / nt; tn[2] = tc[2] / nt;
    skew_mul(tn, Rc, E);
    return true;
}
MFR_DEV int erig_n(const int32_t *n_corr, size_t row, int maxN)
{
    const int n = n_corr[row];
    return n < 0 ? 0 : (n > maxN ? maxN : n);
}

// grid (ceil(NH / 16), B), 256 threads
__global__ void __launch_bounds__(256) erig_score_kernel(
    const float *__restrict__ pts0, const float *__restrict__ pts1, const int32_t *__restrict__ n_corr, int T, int maxN,
    const void *__restrict__ K0, const void *__restrict__ K1, int k_dtype, double pix_thr, const double *__restrict__ rig,
    const double *__restrict__ models, int32_t *__restrict__ counts)
{
    __shared__ double model[12][ER_HYP_WG], comp[21][ER_HYP_WG];
    __shared__ double pa[ER_TILE], pb[ER_TILE], pc[ER_TILE], pd[ER_TILE];
    __shared__ int okh[ER_HYP_WG], okf[ER_HYP_WG], cnt[ER_HYP_WG];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, NH = T * (T - 1);
    const int h = blockIdx.x * ER_HYP_WG + tid;                  // tid < ER_HYP_WG: this thread's hypothesis
    if (tid < ER_HYP_WG) {
        const int ok = (h < NH) && counts[(size_t)b * NH + h] >= 0;
        okh[tid] = ok; okf[tid] = 0; cnt[tid] = 0;
        if (ok)
            for (int k = 0; k < 12; ++k) model[k][tid] = models[((size_t)b * NH + h) * 12 + k];
    }
    __syncthreads();
    int any = 0;
    for (int k = 0; k < ER_HYP_WG; ++k) any |= okh[k];
    if (!any) return;                                            // uniform over the workgroup
    for (int j = 0; j < T; ++j) {
        const size_t row = (size_t)b * T + j;
        const int n = erig_n(n_corr, row, maxN);
        if (n == 0) continue;                                    // uniform
        const double thr2 = emat_thr2(K0, b, K1, (int)row, k_dtype, pix_thr);
        for (int base = 0; base < n; base += ER_TILE) {
            const int tn = min(ER_TILE, n - base);
            __syncthreads();
            for (int i = tid; i < tn; i += 256) {
                const size_t o = (row * maxN + base + i) * 2;
                double x[4];
                emat_normalize(pts0 + o, pts1 + o, K0, b, K1, (int)row, k_dtype, x);
                pa[i] = x[0]; pb[i] = x[1]; pc[i] = x[2]; pd[i] = x[3];
            }
            if (base == 0 && tid < ER_HYP_WG && okh[tid]) {      // okh[tid] was written by this thread
                double R[9], t[3], E[9], Rc[9], tu[3];
                for (int k = 0; k < 9; ++k) R[k] = model[k][tid];
                for (int k = 0; k < 3; ++k) t[k] = model[9 + k][tid];
                const bool ok = erig_frame_model(rig + row * 12, R, t, E, Rc, tu);
                okf[tid] = ok ? 1 : 0;
                if (ok) {
                    for (int k = 0; k < 9; ++k) { comp[k][tid] = E[k]; comp[9 + k][tid] = Rc[k]; }
                    for (int k = 0; k < 3; ++k) comp[18 + k][tid] = tu[k];
                }
            }
            __syncthreads();
            for (int hi = wid; hi < ER_HYP_WG; hi += 4) {
                if (!okh[hi] || !okf[hi]) continue;              // wave-uniform
                double E[9], Rc[9], tu[3];
#pragma unroll
                for (int k = 0; k < 9; ++k) { E[k] = comp[k][hi]; Rc[k] = comp[9 + k][hi]; }
#pragma unroll
                for (int k = 0; k < 3; ++k) tu[k] = comp[18 + k][hi];
                int c = 0;
                for (int i0 = 0; i0 < tn; i0 += 64) {
                    const int i = i0 + lane;
                    bool in = false;
                    if (i < tn) in = sampson2(E, pa[i], pb[i], pc[i], pd[i]) < thr2 && cheirality(Rc, tu, pa[i], pb[i], pc[i], pd[i]);
                    c += __popcll(__ballot(in));
                }
                if (lane == 0) cnt[hi] += c;
            }
        }
    }
    __syncthreads();
    if (tid < ER_HYP_WG && okh[tid]) counts[(size_t)b * NH + h] = cnt[tid];
}

// what erig_select_kernel knows about its sample
struct ErigSample {
    const float *pts0, *pts1; const int32_t *n_corr; const void *K0, *K1; const double *rig; int k_dtype, b, T, maxN;
    __device__ __forceinline__ size_t row(int j) const { return (size_t)b * T + j; }
    __device__ __forceinline__ void point(int j, int i, double x[4]) const
    {
        const size_t o = (row(j) * maxN + i) * 2;
        emat_normalize(pts0 + o, pts1 + o, K0, b, K1, (int)row(j), k_dtype, x);
    }
};

// sum of squared Sampson residuals of the pooled inliers idx[0 .. m): lane partials in list order, then the butterfly
MFR_DEV double erig_cost(const ErigSample &s, const int32_t *idx, int m, const double *R, const double *t)
{
    double acc = 0.0;
    for (int q = lane_id(); q < m; q += 64) {
        const int p = idx[q], j = p / s.maxN, i = p - j * s.maxN;
        double Rc[9], tc[3], E[9], x[4];
        rig_compose(s.rig + s.row(j) * 12, R, t, Rc, tc);
        skew_mul(tc, Rc, E);
        s.point(j, i, x);
        acc = acc + sampson2(E, x[0], x[1], x[2], x[3]);
    }
    return wave_sum(acc);
}

// Levenberg-Marquardt over (R, t) (header); -1 when the starting cost is not finite (R, t untouched)
MFR_DEV int erig_lm(const ErigSample &s, const int32_t *idx, int m, int max_iter, double *R, double *t)
{
    LmDamping lm;
    double cost = erig_cost(s, idx, m, R, t);
    if (!(cost == cost) || !(cost < 1e300)) return -1;
    for (int it = 0; it < max_iter; ++it) {
        double acc[27];
#pragma unroll
        for (int q = 0; q < 27; ++q) acc[q] = 0.0;
        for (int q = lane_id(); q < m; q += 64) {
            const int p = idx[q], j = p / s.maxN, i = p - j * s.maxN;
            const double *A = s.rig + s.row(j) * 12;
            double Rc[9], tc[3], E[9], x[4], Jk[6], J[6], r;
            rig_compose(A, R, t, Rc, tc);
            skew_mul(tc, Rc, E);
            s.point(j, i, x);
            sampson_jac(E, Rc, tc, x[0], x[1], x[2], x[3], Jk, r);
            J[0] = Jk[0]; J[1] = Jk[1]; J[2] = Jk[2];
#pragma unroll
            for (int c = 0; c < 3; ++c) J[3 + c] = (Jk[3] * A[c] + Jk[4] * A[3 + c]) + Jk[5] * A[6 + c];
            lm6_accumulate(acc, J, r);
        }
#pragma unroll
        for (int q = 0; q < 27; ++q) acc[q] = wave_sum(acc[q]);
        double H[36], g[6], dl[6];
        lm6_unpack(acc, H, g);
        lm.damp(H);
        if (chol_solve6(H, g, dl)) {
            if (lm.reject()) break;
            continue;
        }
        double Rn[9], tn[3];
        quat_right_update(R, dl, Rn);
        tn[0] = t[0] + dl[3]; tn[1] = t[1] + dl[4]; tn[2] = t[2] + dl[5];
        const double cn = erig_cost(s, idx, m, Rn, tn);
        if (cn < cost) {
            for (int k = 0; k < 9; ++k) R[k] = Rn[k];
            for (int k = 0; k < 3; ++k) t[k] = tn[k];
            const bool done = lm.accept(cost - cn, 1e-14 * cost);
            cost = cn;
            if (done) break;
        } else if (lm.reject()) break;
        if (lm6_max_abs(dl) < 1e-13) break;
    }
    return 0;
}

// one wavefront per sample
__global__ void __launch_bounds__(64) erig_select_kernel(
    const float *__restrict__ pts0, const float *__restrict__ pts1, const int32_t *__restrict__ n_corr, int T, int maxN,
    const void *__restrict__ K0, const void *__restrict__ K1, int k_dtype, double pix_thr, const double *__restrict__ rig,
    const double *__restrict__ R1, const double *__restrict__ t1, const int32_t *__restrict__ ninl1, const int32_t *__restrict__ st1,
    const uint8_t *__restrict__ mask1, const double *__restrict__ models, const int32_t *__restrict__ counts,
    int32_t *__restrict__ idx_ws, double *__restrict__ Rout, double *__restrict__ tout, int32_t *__restrict__ n_inliers,
    int32_t *__restrict__ status, uint8_t *__restrict__ mask_out, int32_t *__restrict__ best_hyp)
{
    const int b = blockIdx.x, lane = threadIdx.x, NH = T * (T - 1);
    const size_t pool = (size_t)T * maxN, row0 = (size_t)b * T;
    uint8_t *mo = mask_out ? mask_out + (size_t)b * pool : nullptr;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    if (T == 1) {                                              // no rig: stage 1's result is the answer
        if (mo)
            for (int i = lane; i < maxN; i += 64) mo[i] = mask1[row0 * maxN + i];
        if (lane == 0) {
            for (int k = 0; k < 9; ++k) Rout[9 * b + k] = R1[9 * row0 + k];
            for (int k = 0; k < 3; ++k) tout[3 * b + k] = t1[3 * row0 + k];
            n_inliers[b] = ninl1[row0]; status[b] = st1[row0];
            if (best_hyp) best_hyp[b] = -1;
        }
        return;
    }
    const ErigSample s = { pts0, pts1, n_corr, K0, K1, rig, k_dtype, b, T, maxN };
    int32_t *idx = idx_ws + (size_t)b * pool;
    const unsigned um = erig_usable(st1 + row0, T);
    int st = MFR_ST_OK;
    if (__popc(um) < 2) {
        bool same = true;
        for (int j = 1; j < T; ++j) same = same && st1[row0 + j] == st1[row0];
        st = (um == 0 && same) ? st1[row0] : MFR_ST_NO_MODEL;
    }
    int bh = -1, bestc = -1, m = 0, cntf = 0;
    double R[9], t[3];
    if (st == MFR_ST_OK) {
        for (int h = 0; h < NH; ++h) {
            const int c = counts[(size_t)b * NH + h];
            if (c > bestc) { bestc = c; bh = h; }
        }
        if (bh < 0) st = MFR_ST_NO_MODEL;
    }
    if (st == MFR_ST_OK) {
        const double *src = models + ((size_t)b * NH + bh) * 12;
        for (int k = 0; k < 9; ++k) R[k] = src[k];
        for (int k = 0; k < 3; ++k) t[k] = src[9 + k];
    }
    // pass 0: the pooled inlier list of the best hypothesis; pass 1: the count and mask of the refined model
    for (int pass = 0; pass < 2 && st == MFR_ST_OK; ++pass) {
        for (int j = 0; j < T; ++j) {
            const int n = erig_n(n_corr, s.row(j), maxN);
            double E[9], Rc[9], tu[3];
            const bool okf = n > 0 && erig_frame_model(rig + s.row(j) * 12, R, t, E, Rc, tu);
            const double thr2 = emat_thr2(K0, b, K1, (int)s.row(j), k_dtype, pix_thr);
            for (int i0 = 0; i0 < n; i0 += 64) {
                const int i = i0 + lane;
                bool in = false;
                if (okf && i < n) {
                    double x[4];
                    s.point(j, i, x);
                    in = sampson2(E, x[0], x[1], x[2], x[3]) < thr2 && cheirality(Rc, tu, x[0], x[1], x[2], x[3]);
                }
                if (pass == 0) wave_compact_append(in, j * maxN + i, idx, m);
                else {
                    cntf += __popcll(__ballot(in));
                    if (mo && i < n) mo[(size_t)j * maxN + i] = in ? 1 : 0;
                }
            }
            if (pass == 1 && mo)
                for (int i = n + lane; i < maxN; i += 64) mo[(size_t)j * maxN + i] = 0;
        }
        if (pass == 0) {
            __threadfence();                                   // idx[] written by other lanes of this wave is read below
            if (m >= 6) erig_lm(s, idx, m, 20, R, t);
            bool bad = false;
            for (int k = 0; k < 9; ++k) bad |= !isfinite(R[k]);
            for (int k = 0; k < 3; ++k) bad |= !isfinite(t[k]);
            if (bad || sqrt(dot3(t, t)) > 1000.0) st = MFR_ST_DEGENERATE;
        }
    }
    if (st != MFR_ST_OK && mo)
        for (size_t i = lane; i < pool; i += 64) mo[i] = 0;
    if (lane == 0) {
        for (int k = 0; k < 9; ++k) Rout[9 * b + k] = (st == MFR_ST_OK) ? R[k] : qnan;
        for (int k = 0; k < 3; ++k) tout[3 * b + k] = (st == MFR_ST_OK) ? t[k] : qnan;
        n_inliers[b] = (st == MFR_ST_OK) ? cntf : 0;
        status[b] = st;
        if (best_hyp) best_hyp[b] = bh;
    }
}

// rows of stage 1 from a sample's one K0 and pair id: K0 row b T + j = K0[b], key = pair_id T + j (the rig PnP path's keys)
__global__ void erig_rows_kernel(const void *K0, int k_dtype, const int64_t *pair_ids, int B, int T, void *K0_rows, int64_t *pid_rows)
{
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= B * T) return;
    const int b = row / T, j = row - b * T;
    pid_rows[row] = (int64_t)((uint64_t)pair_ids[b] * (uint64_t)T + (uint64_t)j);
    for (int k = 0; k < 9; ++k) {
        if (k_dtype == MFR_K_F32) ((float *)K0_rows)[9 * (size_t)row + k] = ((const float *)K0)[9 * (size_t)b + k];
        else ((double *)K0_rows)[9 * (size_t)row + k] = ((const double *)K0)[9 * (size_t)b + k];
    }
}

// ------------------------------------------------------------------------------------------
// C-ABI
struct ErigWs { double *models; int32_t *counts, *idx; size_t total; };
static ErigWs erig_ws(void *base, int B, int T, int maxN)
{
    WsCarver c(base);
    ErigWs w;
    const size_t b = (size_t)B, nh = (size_t)(T > 1 ? T * (T - 1) : 1);
    w.models = c.take<double>(12 * b * nh);
    w.counts = c.take<int32_t>(b * nh);
    w.idx = c.take<int32_t>(b * T * maxN);
    w.total = c.off;
    return w;
}
struct ErigBatchWs { double *K0r; int64_t *pid; double *R1, *t1; int32_t *ninl1, *st1; uint8_t *mask1; char *stage1, *stage2; size_t n1, n2, total; };
static ErigBatchWs erig_batch_ws(void *base, int B, int T, int maxN, int max_iters)
{
    WsCarver c(base);
    ErigBatchWs w;
    const size_t rows = (size_t)B * T;
    w.K0r = c.take<double>(9 * rows);
    w.pid = c.take<int64_t>(rows);
    w.R1 = c.take<double>(9 * rows);
    w.t1 = c.take<double>(3 * rows);
    w.ninl1 = c.take<int32_t>(rows);
    w.st1 = c.take<int32_t>(rows);
    w.mask1 = c.take<uint8_t>(rows * maxN);
    w.n1 = mfr_emat_workspace_bytes((int)rows, maxN, max_iters);
    w.n2 = erig_ws(nullptr, B, T, maxN).total;
    w.stage1 = c.take<char>(w.n1);
    w.stage2 = c.take<char>(w.n2);
    w.total = c.off;
    return w;
}

extern "C" {

size_t mfr_rig_emat_workspace_bytes(int B, int T, int maxN)
{
    if (!rig_dims_ok(B, T, maxN)) return 0;
    return erig_ws(nullptr, B, T, maxN).total;
}

int mfr_rig_emat_solve(const float *pts0, const float *pts1, const int32_t *n_corr, int B, int T, int maxN,
                       const void *K0, const void *K1, int k_dtype, const double *rig, double pix_thr,
                       const double *R1, const double *t1, const int32_t *n_inliers1, const int32_t *status1, const uint8_t *mask1,
                       void *workspace, size_t workspace_bytes, double *R, double *t, int32_t *n_inliers, int32_t *status,
                       uint8_t *inlier_mask, int32_t *hyp_counts, int32_t *best_hyp, void *stream)
{
    if (!pts0 || !pts1 || !n_corr || !K0 || !K1 || !rig || !R1 || !t1 || !n_inliers1 || !status1 || !mask1 || !workspace || !R || !t ||
        !n_inliers || !status || !rig_dims_ok(B, T, maxN) || !(pix_thr > 0.0) || !k_dtype_ok(k_dtype)) return MFR_E_ARG;
    const ErigWs w = erig_ws(workspace, B, T, maxN);
    if (workspace_bytes < w.total) return MFR_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int NH = T * (T - 1);
    if (T > 1) {
        hipLaunchKernelGGL(erig_hyp_kernel, dim3(B), dim3(256), 0, s, R1, t1, status1, T, rig, w.models, w.counts);
        CHECK_LAUNCH();
        hipLaunchKernelGGL(erig_score_kernel, dim3((NH + ER_HYP_WG - 1) / ER_HYP_WG, B), dim3(256), 0, s, pts0, pts1, n_corr, T, maxN, K0,
                           K1, k_dtype, pix_thr, rig, w.models, w.counts);
        CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(erig_select_kernel, dim3(B), dim3(64), 0, s, pts0, pts1, n_corr, T, maxN, K0, K1, k_dtype, pix_thr, rig, R1, t1,
                       n_inliers1, status1, mask1, w.models, w.counts, w.idx, R, t, n_inliers, status, inlier_mask, best_hyp);
    CHECK_LAUNCH();
    if (hyp_counts && T > 1)
        if (hipMemcpyAsync(hyp_counts, w.counts, sizeof(int32_t) * (size_t)B * NH, hipMemcpyDeviceToDevice, s) != hipSuccess)
            return MFR_E_LAUNCH;
    return 0;
}

size_t mfr_rig_emat_batch_workspace_bytes(int B, int T, int maxN, int max_iters)
{
    if (!rig_dims_ok(B, T, maxN)) return 0;
    if (max_iters < 1) max_iters = 1;
    return erig_batch_ws(nullptr, B, T, maxN, max_iters).total;
}

int mfr_rig_emat_solve_batch(const float *pts0, const float *pts1, const int32_t *n_corr, int B, int T, int maxN,
                             const void *K0, const void *K1, int k_dtype, const double *rig, double pix_thr, double confidence,
                             int max_iters, uint64_t seed, const int64_t *pair_ids, int score_method, const double *magsac_lut, int lut_m,
                             double max_thr_ratio, void *workspace, size_t workspace_bytes, double *R, double *t, int32_t *n_inliers,
                             int32_t *status, uint8_t *inlier_mask, int32_t *hyp_counts, int32_t *best_hyp, void *stream)
{
    if (!pts0 || !pts1 || !n_corr || !K0 || !K1 || !rig || !pair_ids || !workspace || !R || !t || !n_inliers || !status ||
        !rig_dims_ok(B, T, maxN) || !(pix_thr > 0.0) || !k_dtype_ok(k_dtype)) return MFR_E_ARG;
    if (max_iters < 1) max_iters = 1;
    const ErigBatchWs w = erig_batch_ws(workspace, B, T, maxN, max_iters);
    if (workspace_bytes < w.total) return MFR_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int rows = B * T;
    hipLaunchKernelGGL(erig_rows_kernel, dim3((rows + 63) / 64), dim3(64), 0, s, K0, k_dtype, pair_ids, B, T, (void *)w.K0r, w.pid);
    CHECK_LAUNCH();
    int rc = mfr_emat_solve_batch(pts0, pts1, n_corr, rows, maxN, w.K0r, K1, k_dtype, pix_thr, confidence, max_iters, seed, w.pid, score_method,
                                  magsac_lut, lut_m, max_thr_ratio, w.stage1, w.n1, w.R1, w.t1, w.ninl1, w.st1, w.mask1, nullptr, nullptr,
                                  nullptr, nullptr, nullptr, stream);
    if (rc) return rc;
    return mfr_rig_emat_solve(pts0, pts1, n_corr, B, T, maxN, K0, K1, k_dtype, rig, pix_thr, w.R1, w.t1, w.ninl1, w.st1, w.mask1, w.stage2,
                              w.n2, R, t, n_inliers, status, inlier_mask, hyp_counts, best_hyp, stream);
}

}  // extern "C"
