// abs_pose.hip -- absolute query pose from the relative poses to several database images on gfx950: the fusion step of the 7Scenes
// benchmark (lib/utils/localize.py), batched over queries.
//
//   abs_pose_pair_kernel    one THREAD per (database, query) pair: RelaPosePair.__init__ / AbsPose (:896-964) -- the mat2quat -> quat2mat
//                           round trip of the predicted rotation, x_te, abs_q_pred, abs_c_pred, the two rows the pair adds to the
//                           triangulation system, and t_opt = -r^T t with its norm.  32 doubles per pair in the workspace.
//   abs_pose_ransac_kernel  mode 1, one WAVEFRONT per query: ransac(pair_type='relapose') (:471-635).  Lanes over the C(k,2) minimal
//                           samples (64 at a time, combinations order): estimate_model + find_inliers per lane.  Then the sequential part,
//                           kept: the lowest lane with >= 2 inliers and strictly more than the best so far wins (ballot + ffs), runs
//                           local_optimisation with lanes over its 2 + lo_iters candidates, and its result suppresses the later lanes.
//   abs_pose_median_kernel  mode 0, one THREAD per query: cal_abs_pose_err_metric (:352-421) -- Weiszfeld geometric median of the
//                           abs_c_pred (capped at AP_WEISZFELD_CAP iterations) and the chordal L2 mean of the rotations.
//
// Inlier sets are 64-bit masks (k <= 64 neighbours in mode 1), models are always fitted over a set in ascending pair index.
// The three eigenproblems (mat2quat, the triangulation's null vector as the smallest eigenvector of A^T A, the chordal mean) are a cyclic
// Jacobi on a symmetric 4x4 with a fixed number of sweeps.  Every loop is bounded by k, 64, lo_iters or a constant.
// The random subsets of local_optimisation come from Philox keyed by (seed, query, LO call, iteration) -- the reference shuffles with
// numpy's unseeded global generator.  f64 VALU only, compiled with -ffp-contract=off (FP contract in geom_dev.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mfr_hip.h"
#include "solver_dev.h"

using namespace mfr;

#define AP_PW 32                 // doubles per pair in the workspace
#define AP_A 0                   // [2][4] rows of the triangulation system: x_te[r] * p[2,:] - p[r,:]
#define AP_Q 8                   // abs_q_pred (wxyz)
#define AP_C 12                  // abs_c_pred
#define AP_RTR 15                // r_train (row major)
#define AP_CTR 24                // c_train
#define AP_TOPT 27               // t_opt = -r^T t
#define AP_NOPT 30               // |t_opt|
#define AP_SWEEPS 12
#define AP_WAVES 4               // queries per workgroup (mode 1)

// ---------------------------------------------------------------- quaternions
// transforms3d.quaternions.quat2mat: divides by the squared norm, identity below eps
MFR_DEV void quat2mat(const double q[4], double R[9])
{
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double Nq = ((w * w + x * x) + y * y) + z * z;
    if (Nq < 2.220446049250313e-16) {
        R[0] = 1.0; R[1] = 0.0; R[2] = 0.0; R[3] = 0.0; R[4] = 1.0; R[5] = 0.0; R[6] = 0.0; R[7] = 0.0; R[8] = 1.0;
        return;
    }
    const double s = 2.0 / Nq;
    const double X = x * s, Y = y * s, Z = z * s;
    const double wX = w * X, wY = w * Y, wZ = w * Z, xX = x * X, xY = x * Y, xZ = x * Z, yY = y * Y, yZ = y * Z, zZ = z * Z;
    R[0] = 1.0 - (yY + zZ); R[1] = xY - wZ;         R[2] = xZ + wY;
    R[3] = xY + wZ;         R[4] = 1.0 - (xX + zZ); R[5] = yZ - wX;
    R[6] = xZ - wY;         R[7] = yZ + wX;         R[8] = 1.0 - (xX + yY);
}
// transforms3d.quaternions.mat2quat: the largest eigenvector of the symmetric K / 3 (built from its lower triangle), w >= 0
MFR_DEV void mat2quat(const double M[9], double q[4])
{
    const double Qxx = M[0], Qyx = M[1], Qzx = M[2], Qxy = M[3], Qyy = M[4], Qzy = M[5], Qxz = M[6], Qyz = M[7], Qzz = M[8];
    double K[4][4];
    K[0][0] = ((Qxx - Qyy) - Qzz) / 3.0;
    K[1][0] = (Qyx + Qxy) / 3.0; K[1][1] = ((Qyy - Qxx) - Qzz) / 3.0;
    K[2][0] = (Qzx + Qxz) / 3.0; K[2][1] = (Qzy + Qyz) / 3.0; K[2][2] = ((Qzz - Qxx) - Qyy) / 3.0;
    K[3][0] = (Qyz - Qzy) / 3.0; K[3][1] = (Qzx - Qxz) / 3.0; K[3][2] = (Qxy - Qyx) / 3.0; K[3][3] = ((Qxx + Qyy) + Qzz) / 3.0;
    K[0][1] = K[1][0]; K[0][2] = K[2][0]; K[0][3] = K[3][0]; K[1][2] = K[2][1]; K[1][3] = K[3][1]; K[2][3] = K[3][2];
    double v[4];
    jacobi4_pick<AP_SWEEPS>(K, true, v);
    q[0] = v[3]; q[1] = v[0]; q[2] = v[1]; q[3] = v[2];
    if (q[0] < 0.0) { q[0] = -q[0]; q[1] = -q[1]; q[2] = -q[2]; q[3] = -q[3]; }
}

// ---------------------------------------------------------------- per pair
__global__ void __launch_bounds__(64) abs_pose_pair_kernel(
    const double *__restrict__ train_q, const double *__restrict__ train_c, const double *__restrict__ pred_R,
    const double *__restrict__ pred_t, int P, double *__restrict__ pw)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    double qp[4], r[9], rtr[9], qt[4], Rin[9];
    for (int k = 0; k < 9; ++k) Rin[k] = pred_R[9 * (size_t)i + k];
    mat2quat(Rin, qp);                                   // benchmark/sevenscenes.py:59
    quat2mat(qp, r);                                     // RelaPose.__init__
    for (int k = 0; k < 4; ++k) qt[k] = train_q[4 * (size_t)i + k];
    quat2mat(qt, rtr);                                   // AbsPose.__init__
    const double t[3] = { pred_t[3 * (size_t)i], pred_t[3 * (size_t)i + 1], pred_t[3 * (size_t)i + 2] };
    const double ct[3] = { train_c[3 * (size_t)i], train_c[3 * (size_t)i + 1], train_c[3 * (size_t)i + 2] };
    double *o = pw + (size_t)i * AP_PW;
    double topt[3];                                      // -r^T t: x_te before the division (:959), t_opt of find_inliers (:705)
    for (int a = 0; a < 3; ++a) topt[a] = -((r[a] * t[0] + r[3 + a] * t[1]) + r[6 + a] * t[2]);
    const double z = (topt[2] != 0.0) ? topt[2] : 1.0;
    const double xte[2] = { topt[0] / z, topt[1] / z };
    double tt[3];                                        // AbsPose.t = -r c
    for (int a = 0; a < 3; ++a) tt[a] = -((rtr[3 * a] * ct[0] + rtr[3 * a + 1] * ct[1]) + rtr[3 * a + 2] * ct[2]);
    for (int rr = 0; rr < 2; ++rr) {                     // triangulate_multi_views rows (:798-799)
        for (int a = 0; a < 3; ++a) o[AP_A + 4 * rr + a] = xte[rr] * rtr[6 + a] - rtr[3 * rr + a];
        o[AP_A + 4 * rr + 3] = xte[rr] * tt[2] - tt[rr];
    }
    double ar[9], aq[4];                                 // abs_r_pred = r . r_train (:961)
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) ar[3 * a + b] = (r[3 * a] * rtr[b] + r[3 * a + 1] * rtr[3 + b]) + r[3 * a + 2] * rtr[6 + b];
    mat2quat(ar, aq);
    for (int k = 0; k < 4; ++k) o[AP_Q + k] = aq[k];
    for (int a = 0; a < 3; ++a)                          // abs_c_pred = c_train - r_train^T r^T t (:963)
        o[AP_C + a] = ct[a] + ((rtr[a] * topt[0] + rtr[3 + a] * topt[1]) + rtr[6 + a] * topt[2]);
    for (int k = 0; k < 9; ++k) o[AP_RTR + k] = rtr[k];
    for (int a = 0; a < 3; ++a) { o[AP_CTR + a] = ct[a]; o[AP_TOPT + a] = topt[a]; }
    o[AP_NOPT] = sqrt((topt[0] * topt[0] + topt[1] * topt[1]) + topt[2] * topt[2]);
    o[31] = 0.0;
}

// ---------------------------------------------------------------- mode 1
struct ApHyp { double c[3]; double q[4]; };

// estimate_model (:734-756) over the pairs of `mask`, ascending: null vector of the stacked rows, mean of the abs_q_pred
MFR_DEV void ap_estimate(const double *__restrict__ pw, int k, uint64_t mask, ApHyp &h)
{
    double M[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) M[a][b] = 0.0;
    double qs[4] = { 0.0, 0.0, 0.0, 0.0 };
    int n = 0;
    for (int i = 0; i < k; ++i) {
        if (!((mask >> i) & 1ull)) continue;
        const double *p = pw + (size_t)i * AP_PW;
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
            double row[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) row[a] = p[AP_A + 4 * rr + a];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = a; b < 4; ++b) M[a][b] = M[a][b] + row[a] * row[b];
        }
#pragma unroll
        for (int a = 0; a < 4; ++a) qs[a] = qs[a] + p[AP_Q + a];
        ++n;
    }
#pragma unroll
    for (int a = 1; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < a; ++b) M[a][b] = M[b][a];
    double X[4];
    jacobi4_pick<AP_SWEEPS>(M, false, X);
    h.c[0] = X[0] / X[3]; h.c[1] = X[1] / X[3]; h.c[2] = X[2] / X[3];
    const double dn = (double)n;
#pragma unroll
    for (int a = 0; a < 4; ++a) h.q[a] = qs[a] / dn;
}

// find_inliers (:667-731) of a hypothesised centre.  A zero t_est is error 0; a zero t_opt or an infinite t_est is the reference's
// RuntimeWarning route (the error stays inf: no inlier); a NaN angle is error 0 (cal_vec_angle_error :31)
MFR_DEV uint64_t ap_inliers(const double *__restrict__ pw, int k, const double c[3], double thr)
{
    uint64_t m = 0;
    for (int i = 0; i < k; ++i) {
        const double *p = pw + (size_t)i * AP_PW;
        const double d[3] = { c[0] - p[AP_CTR], c[1] - p[AP_CTR + 1], c[2] - p[AP_CTR + 2] };
        double te[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) te[a] = (p[AP_RTR + 3 * a] * d[0] + p[AP_RTR + 3 * a + 1] * d[1]) + p[AP_RTR + 3 * a + 2] * d[2];
        const double ne = sqrt((te[0] * te[0] + te[1] * te[1]) + te[2] * te[2]);
        const double no = p[AP_NOPT];
        double err;
        if (ne == 0.0) err = 0.0;
        else if (no == 0.0 || ne == __longlong_as_double(0x7ff0000000000000LL)) continue;
        else {
            double dd = ((p[AP_TOPT] / no) * (te[0] / ne) + (p[AP_TOPT + 1] / no) * (te[1] / ne)) + (p[AP_TOPT + 2] / no) * (te[2] / ne);
            dd = __builtin_rint(dd * 1e4) / 1e4;
            if (dd < -1.0) dd = -1.0;
            if (dd > 1.0) dd = 1.0;
            err = acos(dd) * (180.0 / 3.141592653589793);
            if (!(err == err)) err = 0.0;
        }
        if (err < thr) m |= 1ull << i;
    }
    return m;
}

MFR_DEV void ap_bcast(ApHyp &h, int src)
{
#pragma unroll
    for (int a = 0; a < 3; ++a) h.c[a] = __shfl(h.c[a], src, 64);
#pragma unroll
    for (int a = 0; a < 4; ++a) h.q[a] = __shfl(h.q[a], src, 64);
}

// the `it`-th subset of local optimisation call `call` of query `qid`: nsub (<= 14) distinct members of `base` (nb of them)
MFR_DEV uint64_t ap_subset(uint64_t seed, uint32_t qid, uint32_t call, uint32_t it, uint64_t base, int nb, int nsub)
{
    uint64_t rem = base, sub = 0;
    uint32_t w[4] = { 0u, 0u, 0u, 0u };
    for (int j = 0; j < nsub; ++j) {
        if ((j & 3) == 0) philox4x32_10(it, call * 4u + (uint32_t)(j >> 2), qid, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), w);
        const int jj = j & 3;
        const uint32_t wj = (jj == 0) ? w[0] : (jj == 1) ? w[1] : (jj == 2) ? w[2] : w[3];      // selected by compares: w stays in registers
        int r = (int)__umulhi(wj, (uint32_t)(nb - j));
        for (int bit = 0; bit < 64; ++bit) {
            if (!((rem >> bit) & 1ull)) continue;
            if (r == 0) { sub |= 1ull << bit; rem &= ~(1ull << bit); break; }
            --r;
        }
    }
    return sub;
}

__global__ void __launch_bounds__(64 * AP_WAVES) abs_pose_ransac_kernel(
    const double *__restrict__ pw_all, const double *__restrict__ train_q, const double *__restrict__ train_c,
    const int32_t *__restrict__ offsets, int Q, int P, double thr, double thr_mult, int lo_iters, uint64_t seed,
    double *__restrict__ abs_q, double *__restrict__ abs_c, int32_t *__restrict__ inlier_mask, int32_t *__restrict__ status)
{
    const int lane = lane_id(), qi = blockIdx.x * AP_WAVES + (int)(threadIdx.x >> 6);
    if (qi >= Q) return;                                                // whole wavefronts leave; no workgroup barrier below
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    const int p0 = offsets[qi], k = offsets[qi + 1] - p0;
    if (p0 < 0 || k <= 0 || k > MFR_AP_MAX_PAIRS || (long long)p0 + k > (long long)P) {
        const bool ranged = p0 >= 0 && k > 0 && (long long)p0 + k <= (long long)P;
        if (lane < 4) abs_q[4 * (size_t)qi + lane] = qnan;
        if (lane < 3) abs_c[3 * (size_t)qi + lane] = qnan;
        if (lane == 0) status[qi] = (k == 0 && p0 >= 0 && p0 <= P) ? MFR_AP_NO_PAIRS : ranged ? MFR_AP_TOO_MANY : MFR_AP_BAD_OFFSETS;
        if (ranged)
            for (int i = lane; i < k; i += 64) inlier_mask[p0 + i] = 0;
        return;
    }
    const double *pw = pw_all + (size_t)p0 * AP_PW;
    const int H = k * (k - 1) / 2;
    const double thr_lo = thr_mult * thr;
    ApHyp best;
    for (int a = 0; a < 3; ++a) best.c[a] = qnan;
    for (int a = 0; a < 4; ++a) best.q[a] = qnan;
    uint64_t best_mask = 0;
    int best_n = 0;
    uint32_t lo_call = 0;
    bool have = false;
    for (int base = 0; base < H; base += 64) {
        const int h = base + lane;
        const bool valid = h < H;
        ApHyp hy;
        for (int a = 0; a < 3; ++a) hy.c[a] = qnan;
        for (int a = 0; a < 4; ++a) hy.q[a] = qnan;
        uint64_t hm = 0;
        int hn = -1;
        if (valid) {
            int a = 0, rem = h;                                         // itertools.combinations(range(k), 2), h-th
            for (; a < k - 1; ++a) { if (rem < k - 1 - a) break; rem -= k - 1 - a; }
            const int b = a + 1 + rem;
            ap_estimate(pw, k, (1ull << a) | (1ull << b), hy);
            hm = ap_inliers(pw, k, hy.c, thr);
            hn = __popcll(hm);
        }
        int from = 0;
        for (int step = 0; step < 64; ++step) {                         // every pass raises best_n: at most k of them
            const unsigned long long bal = __ballot(valid && lane >= from && hn >= 2 && hn > best_n);
            if (!bal) break;
            const int src = __ffsll((long long)bal) - 1;
            best = hy; ap_bcast(best, src);
            best_mask = __shfl((unsigned long long)hm, src, 64);
            best_n = __popcll(best_mask);
            have = true;
            // local_optimisation (:638-664): candidates [best, refit at thr_mult * thr, lo_iters random subsets of its inliers]
            const uint64_t m_mult = ap_inliers(pw, k, best.c, thr_lo);
            ApHyp pm;
            ap_estimate(pw, k, m_mult, pm);
            const uint64_t m_base = ap_inliers(pw, k, pm.c, thr);
            const int nb = __popcll(m_base), nsub = min(14, nb / 2);
            const int ncand = 2 + (nsub > 2 ? lo_iters : 0);
            ApHyp cand = (lane == 0) ? best : pm;
            if (lane >= 2 && lane < ncand) ap_estimate(pw, k, ap_subset(seed, (uint32_t)qi, lo_call, (uint32_t)(lane - 2), m_base, nb, nsub), cand);
            uint64_t cm = 0;
            if (lane < ncand) cm = ap_inliers(pw, k, cand.c, thr);
            float bc = (lane < ncand) ? (float)__popcll(cm) : -1.f;
            int bi = lane;
            wave_argmax(bc, bi);                                        // first strict maximum of the candidate list
            if ((int)bc > best_n) {
                best = cand; ap_bcast(best, bi);
                best_mask = __shfl((unsigned long long)cm, bi, 64);
                best_n = (int)bc;
            }
            ++lo_call;
            from = src + 1;
        }
    }
    int st = MFR_AP_OK;
    if (!have) {                                                        // :541-550: the first pair's database pose
        st = MFR_AP_APPROXIMATED;
        for (int a = 0; a < 4; ++a) best.q[a] = train_q[4 * (size_t)p0 + a];
        for (int a = 0; a < 3; ++a) best.c[a] = train_c[3 * (size_t)p0 + a];
        best_mask = 1ull;
    }
    if (lane == 0) {
        for (int a = 0; a < 4; ++a) abs_q[4 * (size_t)qi + a] = best.q[a];
        for (int a = 0; a < 3; ++a) abs_c[3 * (size_t)qi + a] = best.c[a];
        status[qi] = st;
    }
    if (lane < k) inlier_mask[p0 + lane] = (int32_t)((best_mask >> lane) & 1ull);
}

// ---------------------------------------------------------------- mode 0
__global__ void __launch_bounds__(64) abs_pose_median_kernel(
    const double *__restrict__ pw_all, const int32_t *__restrict__ offsets, int Q, int P,
    double *__restrict__ abs_q, double *__restrict__ abs_c, int32_t *__restrict__ inlier_mask, int32_t *__restrict__ status)
{
    const int qi = blockIdx.x * blockDim.x + threadIdx.x;
    if (qi >= Q) return;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    const int p0 = offsets[qi], k = offsets[qi + 1] - p0;
    if (p0 < 0 || k <= 0 || (long long)p0 + k > (long long)P) {
        for (int a = 0; a < 4; ++a) abs_q[4 * (size_t)qi + a] = qnan;
        for (int a = 0; a < 3; ++a) abs_c[3 * (size_t)qi + a] = qnan;
        status[qi] = (k == 0 && p0 >= 0 && p0 <= P) ? MFR_AP_NO_PAIRS : MFR_AP_BAD_OFFSETS;
        return;
    }
    const double *pw = pw_all + (size_t)p0 * AP_PW;
    const double dk = (double)k;
    // geometric_median (:228-254)
    double y[3] = { 0.0, 0.0, 0.0 };
    for (int i = 0; i < k; ++i)
        for (int a = 0; a < 3; ++a) y[a] = y[a] + pw[(size_t)i * AP_PW + AP_C + a];
    for (int a = 0; a < 3; ++a) y[a] = y[a] / dk;
    int st = MFR_AP_OK | MFR_AP_ITER_CAP;
    for (int it = 0; it < MFR_AP_WEISZFELD_CAP; ++it) {
        double Dinvs = 0.0;
        int nz = 0;
        for (int i = 0; i < k; ++i) {
            const double *x = pw + (size_t)i * AP_PW + AP_C;
            const double e0 = x[0] - y[0], e1 = x[1] - y[1], e2 = x[2] - y[2];
            const double D = sqrt((e0 * e0 + e1 * e1) + e2 * e2);
            if (D != 0.0) Dinvs = Dinvs + 1.0 / D; else ++nz;
        }
        if (nz == k) { st = MFR_AP_OK; break; }                          // every point on y: y is returned
        double T[3] = { 0.0, 0.0, 0.0 };
        for (int i = 0; i < k; ++i) {
            const double *x = pw + (size_t)i * AP_PW + AP_C;
            const double e0 = x[0] - y[0], e1 = x[1] - y[1], e2 = x[2] - y[2];
            const double D = sqrt((e0 * e0 + e1 * e1) + e2 * e2);
            if (D != 0.0) {
                const double W = (1.0 / D) / Dinvs;
                for (int a = 0; a < 3; ++a) T[a] = T[a] + W * x[a];
            }
        }
        double y1[3];
        if (nz == 0) { for (int a = 0; a < 3; ++a) y1[a] = T[a]; }
        else {
            const double R0 = (T[0] - y[0]) * Dinvs, R1 = (T[1] - y[1]) * Dinvs, R2 = (T[2] - y[2]) * Dinvs;
            const double r = sqrt((R0 * R0 + R1 * R1) + R2 * R2);
            const double rinv = (r == 0.0) ? 0.0 : (double)nz / r;
            const double wa = (1.0 - rinv > 0.0) ? 1.0 - rinv : 0.0, wb = (rinv < 1.0) ? rinv : 1.0;
            for (int a = 0; a < 3; ++a) y1[a] = wa * T[a] + wb * y[a];
        }
        const double s0 = y[0] - y1[0], s1 = y[1] - y1[1], s2 = y[2] - y1[2];
        const double step = sqrt((s0 * s0 + s1 * s1) + s2 * s2);
        for (int a = 0; a < 3; ++a) y[a] = y1[a];
        if (step < 1e-5) { st = MFR_AP_OK; break; }
    }
    // Rotation.from_matrix(quat2mat(q_i)).mean() (:396-398): largest eigenvector of sum q q^T over the unit quaternions
    double M[4][4];
    for (int a = 0; a < 4; ++a)
        for (int b = 0; b < 4; ++b) M[a][b] = 0.0;
    for (int i = 0; i < k; ++i) {
        const double *q = pw + (size_t)i * AP_PW + AP_Q;
        const double nn = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
        const double u[4] = { q[0] / nn, q[1] / nn, q[2] / nn, q[3] / nn };
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = a; b < 4; ++b) M[a][b] = M[a][b] + u[a] * u[b];
    }
#pragma unroll
    for (int a = 1; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < a; ++b) M[a][b] = M[b][a];
    double v[4], Rm[9], qo[4];
    jacobi4_pick<AP_SWEEPS>(M, true, v);
    quat2mat(v, Rm);                                                    // .as_matrix(), then mat2quat (:397-398)
    mat2quat(Rm, qo);
    for (int a = 0; a < 4; ++a) abs_q[4 * (size_t)qi + a] = qo[a];
    for (int a = 0; a < 3; ++a) abs_c[3 * (size_t)qi + a] = y[a];
    for (int i = 0; i < k; ++i) inlier_mask[p0 + i] = 1;
    status[qi] = st;
}

// the subsets of ap_subset as 64-bit masks, for the test that pins them to the host restatement: out[(q * calls + c) * iters + it]
__global__ void abs_pose_subset_test_kernel(uint64_t seed, const uint64_t *__restrict__ base, int n, int calls, int iters, int nsub,
                                            uint64_t *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * calls * iters) return;
    const int it = i % iters, c = (i / iters) % calls, q = i / (iters * calls);
    const int nb = __popcll(base[q]);
    out[i] = (nsub <= nb) ? ap_subset(seed, (uint32_t)q, (uint32_t)c, (uint32_t)it, base[q], nb, nsub) : 0ull;
}

extern "C" {

int mfr_test_abs_pose_subset(uint64_t seed, const uint64_t *base, int n, int calls, int iters, int nsub, uint64_t *out, void *stream)
{
    if (!base || !out || n <= 0 || calls <= 0 || calls > MFR_AP_MAX_PAIRS || iters <= 0 || iters > MFR_AP_MAX_LO_ITERS || nsub < 1 || nsub > 14 ||
        (long long)n * calls * iters > 0x7fffffffLL) return MFR_E_ARG;
    const int total = n * calls * iters;
    hipLaunchKernelGGL(abs_pose_subset_test_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, seed, base, n, calls, iters, nsub, out);
    CHECK_LAUNCH();
    return 0;
}

size_t mfr_abs_pose_workspace_bytes(int P)
{
    if (P <= 0) return 0;
    return align_up(sizeof(double) * (size_t)P * AP_PW, 256);
}

int mfr_abs_pose_fuse(const double *train_q, const double *train_c, const double *pred_R, const double *pred_t, int P,
                      const int32_t *offsets, int Q, int mode, double thr_deg, double thr_mult, int lo_iters, uint64_t seed,
                      void *workspace, size_t workspace_bytes,
                      double *abs_q, double *abs_c, int32_t *inlier_mask, int32_t *status, void *stream)
{
    if (!offsets || !abs_q || !abs_c || !status || Q <= 0 || P < 0 || (mode != 0 && mode != 1) || lo_iters < 0 ||
        lo_iters > MFR_AP_MAX_LO_ITERS || !(thr_mult >= 1.0) || !(thr_deg == thr_deg)) return MFR_E_ARG;
    if (P > 0 && (!train_q || !train_c || !pred_R || !pred_t || !workspace || !inlier_mask)) return MFR_E_ARG;
    if (workspace_bytes < mfr_abs_pose_workspace_bytes(P)) return MFR_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    double *pw = (double *)workspace;
    if (P > 0) {
        hipLaunchKernelGGL(abs_pose_pair_kernel, dim3((P + 63) / 64), dim3(64), 0, s, train_q, train_c, pred_R, pred_t, P, pw);
        CHECK_LAUNCH();
    }
    if (mode == 1)
        hipLaunchKernelGGL(abs_pose_ransac_kernel, dim3((Q + AP_WAVES - 1) / AP_WAVES), dim3(64 * AP_WAVES), 0, s, pw, train_q, train_c,
                           offsets, Q, P, thr_deg, thr_mult, lo_iters, seed, abs_q, abs_c, inlier_mask, status);
    else
        hipLaunchKernelGGL(abs_pose_median_kernel, dim3((Q + 63) / 64), dim3(64), 0, s, pw, offsets, Q, P, abs_q, abs_c, inlier_mask, status);
    CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
