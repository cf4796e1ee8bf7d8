// procrustes.hip -- 3-D/3-D Procrustes path of the relative-pose solver on gfx950 (MI355X).
//
// Replaces ProcrustesSolver.estimate_pose (lib/models/matching/pose_solver.py:238-320, REFINE False as
// in config/matching/mapfree/sg_procrustes_dptkitti.yaml) for a batch of pairs:
//   proc_lift_kernel    np.int32 both views (:248-249), depth gather (:256-258), valid vs each map's
//                       minimum (:261, Q6), back-project both (:273-274), ordered compaction
//   proc_hyp_kernel     o3d registration_ransac_based_on_correspondence (:286-287): lane per 3-point
//                       Kabsch (Horn quaternion + fixed-sweep Jacobi), wavefront per hypothesis
//                       scoring (count + squared-error sum in wave64 order)
//   proc_select_kernel  replay of Open3D's best-model rule (fitness, then inlier RMSE) and its
//                       confidence-based exit, final re-fit on the inliers, inliers = int(fitness*N)
// Open3D 0.17 is not available offline: restated from the published algorithm, parity unpinned vs
// Open3D (see oracle/mfr_oracle_procrustes.c for the substitutions).  -ffp-contract=off.
//
// Rig entry point (mfr_rig_procrustes_solve_batch; POSE_SOLVER 'RigProcrustes' of the multi-frame model): ONE pose, reference view ->
// LAST window frame, from the 3-D/3-D correspondences of all T window frames of a sample.  Upstream has no such solver; the yardsticks
// are the numpy mirror tests/rig_procrustes_ref.py and, with T = 1 and the identity rig, the single-frame entry point bit for bit.
//   proc_rig_lift_kernel   frame by frame what proc_lift_kernel does (depth0 against its minimum, taken once per sample; query map j
//                          against its own minimum), then Q' = R_Aj^T (Q - t_Aj) carries the query point into the last frame's camera
//                          (rig_dev.h, rig_to_last's operation order); valid rows of all frames are compacted into ONE pooled list in
//                          (frame, index) order, N = sum of n_valid[j]
//   proc_hyp_kernel, proc_select_kernel   unchanged, on the pooled (P, Q') with maxN = T maxN: hypothesis `it` is
//                          sample_distinct<3>(seed, pair_id, it, N) -- the key is pair_id itself, pooled sampling has no frame draw
//   proc_rig_mask_kernel   the inliers of the re-fitted model (the set n_inliers counts), scattered to ORIGINAL correspondence indices
// Status: all correspondences of a sample count together: fewer than 3 -> MFR_ST_TOO_FEW, fewer than 3 valid -> MFR_ST_BAD_DEPTH.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mfr_hip.h"
#include "solver_dev.h"
#include "rig_dev.h"
#include "zero_fill.h"

using namespace mfr;
#define PR_TILE 512

MFR_DEV double dist2(const double *R, const double *t, double p0, double p1, double p2, double q0, double q1, double q2)
{
    const double d0 = (((R[0] * p0 + R[1] * p1) + R[2] * p2) + t[0]) - q0;
    const double d1 = (((R[3] * p0 + R[4] * p1) + R[5] * p2) + t[1]) - q1;
    const double d2 = (((R[6] * p0 + R[7] * p1) + R[8] * p2) + t[2]) - q2;
    return (d0 * d0 + d1 * d1) + d2 * d2;
}

MFR_DEV void sample3_model(const double *P, const double *Q, int n, uint64_t seed, uint64_t pair_id, int it, double *R, double *t)
{
    int s[3];
    if (n == 3) { s[0] = 0; s[1] = 1; s[2] = 2; } else sample_distinct<3>(seed, pair_id, (uint32_t)it, n, s);
    double m[16];
    for (int k = 0; k < 16; ++k) m[k] = 0.0;
    for (int j = 0; j < 3; ++j) {
        const double *p = P + 3 * (size_t)s[j], *q = Q + 3 * (size_t)s[j];
        m[0] = m[0] + 1.0;
        for (int a = 0; a < 3; ++a) { m[1 + a] = m[1 + a] + p[a]; m[4 + a] = m[4 + a] + q[a]; }
        for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) m[7 + 3 * a + b] = m[7 + 3 * a + b] + p[a] * q[b];
    }
    kabsch_from_moments(m, R, t);
}

__global__ void __launch_bounds__(256) proc_lift_kernel(
    const float *__restrict__ pts0, const float *__restrict__ pts1, const int32_t *__restrict__ n_corr, int maxN,
    const float *__restrict__ depth0, const float *__restrict__ depth1, const float *__restrict__ pmin0,
    const float *__restrict__ pmin1, int H, int W, const void *__restrict__ K0, const void *__restrict__ K1, int k_dtype,
    double *__restrict__ P, double *__restrict__ Q, int32_t *__restrict__ n_valid)
{
    const int b = blockIdx.x, tid = threadIdx.x;
    int n = n_corr[b];
    if (n > maxN) n = maxN;
    __shared__ Compact256 cs;
    const float m0 = depth_min_fold(pmin0, b), m1 = depth_min_fold(pmin1, b);
    double Ki0[4], Ki1[4];
    kinv(K0, k_dtype, b, Ki0); kinv(K1, k_dtype, b, Ki1);
    const float *p0 = pts0 + (size_t)b * maxN * 2, *p1 = pts1 + (size_t)b * maxN * 2;
    const float *d0m = depth0 + (size_t)b * H * W, *d1m = depth1 + (size_t)b * H * W;
    double *oP = P + (size_t)b * maxN * 3, *oQ = Q + (size_t)b * maxN * 3;
    int total = 0;
    for (int start = 0; start < n; start += 256) {
        const int i = start + tid;
        double a[3], c[3];
        bool valid = false;
        if (i < n) {
            const bool v0 = lift_point(p0[2 * i], p0[2 * i + 1], d0m, H, W, m0, Ki0, a);
            const bool v1 = lift_point(p1[2 * i], p1[2 * i + 1], d1m, H, W, m1, Ki1, c);
            valid = v0 && v1;
        }
        const int m = compact256_slot(cs, valid, total);
        if (valid) {
            oP[3 * m] = a[0]; oP[3 * m + 1] = a[1]; oP[3 * m + 2] = a[2];
            oQ[3 * m] = c[0]; oQ[3 * m + 1] = c[1]; oQ[3 * m + 2] = c[2];
        }
    }
    if (tid == 0) n_valid[b] = total;
}

// grid (ceil(iters/256), B)
__global__ void __launch_bounds__(256) proc_hyp_kernel(
    const double *__restrict__ P, const double *__restrict__ Q, const int32_t *__restrict__ n_valid, int maxN,
    int max_iters, double thr2, uint64_t seed, const int64_t *__restrict__ pair_ids,
    int32_t *__restrict__ counts, double *__restrict__ err2)
{
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double *model = (double *)smem_raw;                      // [12][256]
    double *tp = model + 12 * 256;                           // SoA tile: 6 x PR_TILE
    int *cnt = (int *)(tp + 6 * PR_TILE);                    // [256]
    double *esum = (double *)(cnt + 256);                    // [256]
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int n = n_valid[b];
    const int it = blockIdx.x * 256 + tid;
    if (n < 3) {
        if (it < max_iters) { counts[(size_t)b * max_iters + it] = -1; err2[(size_t)b * max_iters + it] = 0.0; }
        return;
    }
    const double *Pb = P + (size_t)b * maxN * 3, *Qb = Q + (size_t)b * maxN * 3;
    {
        double R[9], t[3];
        if (it < max_iters) sample3_model(Pb, Qb, n, seed, (uint64_t)pair_ids[b], it, R, t);
        else { for (int k = 0; k < 9; ++k) R[k] = 0.0; for (int k = 0; k < 3; ++k) t[k] = 0.0; }
        for (int k = 0; k < 9; ++k) model[k * 256 + tid] = R[k];
        for (int k = 0; k < 3; ++k) model[(9 + k) * 256 + tid] = t[k];
        cnt[tid] = 0; esum[tid] = 0.0;
    }
    // error sums: wave64 order inside each 512-point tile, tile sums added in tile order (the oracle's order)
    for (int base = 0; base < n; base += PR_TILE) {
        const int tn = min(PR_TILE, n - base);
        __syncthreads();
        for (int i = tid; i < tn; i += 256) {
            const double *p = Pb + 3 * (size_t)(base + i), *q = Qb + 3 * (size_t)(base + i);
            tp[i] = p[0]; tp[PR_TILE + i] = p[1]; tp[2 * PR_TILE + i] = p[2];
            tp[3 * PR_TILE + i] = q[0]; tp[4 * PR_TILE + i] = q[1]; tp[5 * PR_TILE + i] = q[2];
        }
        __syncthreads();
        for (int h = 0; h < 64; ++h) {
            const int hi = wid * 64 + h;
            if (blockIdx.x * 256 + hi >= max_iters) break;
            double R[9], t[3];
#pragma unroll
            for (int k = 0; k < 9; ++k) R[k] = model[k * 256 + hi];
#pragma unroll
            for (int k = 0; k < 3; ++k) t[k] = model[(9 + k) * 256 + hi];
            int c = 0;
            double e = 0.0;                                   // this lane's partial over points i with (i & 63) == lane
            for (int i0 = 0; i0 < tn; i0 += 64) {
                const int i = i0 + lane;
                bool in = false;
                double d = 0.0;
                if (i < tn) {
                    d = dist2(R, t, tp[i], tp[PR_TILE + i], tp[2 * PR_TILE + i], tp[3 * PR_TILE + i], tp[4 * PR_TILE + i], tp[5 * PR_TILE + i]);
                    in = d < thr2;
                }
                if (in) e = e + d;
                c += __popcll(__ballot(in));
            }
            const double ts = wave_sum(e);
            if (lane == 0) { cnt[hi] += c; esum[hi] = esum[hi] + ts; }
        }
    }
    __syncthreads();
    if (it < max_iters) { counts[(size_t)b * max_iters + it] = cnt[tid]; err2[(size_t)b * max_iters + it] = esum[tid]; }
}

// one wavefront per pair
__global__ void __launch_bounds__(64) proc_select_kernel(
    const double *__restrict__ P, const double *__restrict__ Q, const int32_t *__restrict__ n_valid,
    const int32_t *__restrict__ n_corr, int maxN, int max_iters, double thr2, double conf, uint64_t seed,
    const int64_t *__restrict__ pair_ids, const int32_t *__restrict__ counts, const double *__restrict__ err2,
    int32_t *__restrict__ idx_ws, double *__restrict__ Rout, double *__restrict__ tout, int32_t *__restrict__ n_inliers,
    int32_t *__restrict__ status, int32_t *__restrict__ best_iter, int32_t *__restrict__ iters_run)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    const int n = n_valid[b];
    const double *Pb = P + (size_t)b * maxN * 3, *Qb = Q + (size_t)b * maxN * 3;
    int32_t *idx = idx_ws + (size_t)b * maxN;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    int st = MFR_ST_OK;
    if (n_corr[b] < 3) st = MFR_ST_TOO_FEW;                                 // :252-253
    else if (n < 3) st = MFR_ST_BAD_DEPTH;                                  // :262-263
    double R[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 }, t[3] = { 0, 0, 0 };
    int bit = -1, bcnt = 0, run = 0, cntf = 0;
    if (st == MFR_ST_OK) {
        // sequential replay of Open3D's loop (every lane runs it redundantly on broadcast loads)
        const int32_t *cn = counts + (size_t)b * max_iters;
        const double *er = err2 + (size_t)b * max_iters;
        double berr = 0.0;
        int est_k = max_iters, it = 0;
        const double lnum = det_log(1.0 - conf);
        for (it = 0; it < est_k; ++it) {
            const int c = cn[it];
            const double e = er[it];
            bool better = false;
            if (c > bcnt) better = true;
            else if (c == bcnt && c > 0 && e < berr) better = true;
            if (better) {
                bcnt = c; berr = e; bit = it;
                const double ratio = (double)c / (double)n, r3 = (ratio * ratio) * ratio;
                int k;
                if (r3 >= 1.0) k = 0;
                else {
                    const double kd = lnum / det_log(1.0 - r3);
                    k = (kd < (double)est_k) ? (int)__builtin_ceil(kd) : est_k;
                }
                if (k < est_k) est_k = k;
            }
        }
        run = it;
        if (bit >= 0) {
            sample3_model(Pb, Qb, n, seed, (uint64_t)pair_ids[b], bit, R, t);
            int m = 0;
            for (int i0 = 0; i0 < n; i0 += 64) {
                const int i = i0 + lane;
                const bool in = (i < n) && (dist2(R, t, Pb[3 * (size_t)i], Pb[3 * (size_t)i + 1], Pb[3 * (size_t)i + 2],
                                                  Qb[3 * (size_t)i], Qb[3 * (size_t)i + 1], Qb[3 * (size_t)i + 2]) < thr2);
                wave_compact_append(in, i, idx, m);
            }
            __threadfence();
            double acc[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) acc[k] = 0.0;
            for (int q = lane; q < m; q += 64) {
                const int i = idx[q];
                const double *p = Pb + 3 * (size_t)i, *qq = Qb + 3 * (size_t)i;
                acc[0] = acc[0] + 1.0;
#pragma unroll
                for (int c = 0; c < 3; ++c) { acc[1 + c] = acc[1 + c] + p[c]; acc[4 + c] = acc[4 + c] + qq[c]; }
#pragma unroll
                for (int c = 0; c < 3; ++c)
#pragma unroll
                    for (int d = 0; d < 3; ++d) acc[7 + 3 * c + d] = acc[7 + 3 * c + d] + p[c] * qq[d];
            }
#pragma unroll
            for (int k = 0; k < 16; ++k) acc[k] = wave_sum(acc[k]);
            if (m >= 3) kabsch_from_moments(acc, R, t);
            for (int i0 = 0; i0 < n; i0 += 64) {
                const int i = i0 + lane;
                const bool in = (i < n) && (dist2(R, t, Pb[3 * (size_t)i], Pb[3 * (size_t)i + 1], Pb[3 * (size_t)i + 2],
                                                  Qb[3 * (size_t)i], Qb[3 * (size_t)i + 1], Qb[3 * (size_t)i + 2]) < thr2);
                cntf += __popcll(__ballot(in));
            }
        }
    }
    if (lane == 0) {
        for (int k = 0; k < 9; ++k) Rout[9 * b + k] = (st == MFR_ST_OK) ? R[k] : qnan;
        for (int k = 0; k < 3; ++k) tout[3 * b + k] = (st == MFR_ST_OK) ? t[k] : qnan;
        n_inliers[b] = (st == MFR_ST_OK) ? cntf : 0;
        status[b] = st;
        if (best_iter) best_iter[b] = bit;
        if (iters_run) iters_run[b] = run;
    }
}

// one workgroup per SAMPLE: its T frames in order, one running compaction count.  Rows b T + j of pts0 / pts1 / n_corr / K1 / depth1 / pmin1;
// depth0 / pmin0 / K0 per sample.  P, Q, src are [B, T maxN]; src = j maxN + i, the pooled ORIGINAL index of a pooled valid point.
__global__ void __launch_bounds__(256) proc_rig_lift_kernel(
    const float *__restrict__ pts0, const float *__restrict__ pts1, const int32_t *__restrict__ n_corr, int T, int maxN,
    const float *__restrict__ depth0, const float *__restrict__ depth1, const float *__restrict__ pmin0,
    const float *__restrict__ pmin1, int H, int W, const void *__restrict__ K0, const void *__restrict__ K1, int k_dtype,
    const double *__restrict__ rig, double *__restrict__ P, double *__restrict__ Q, int32_t *__restrict__ src,
    int32_t *__restrict__ n_valid, int32_t *__restrict__ n_pool, int32_t *__restrict__ n_corr_pool)
{
    const int b = blockIdx.x, tid = threadIdx.x;
    __shared__ Compact256 cs;
    const size_t pool = (size_t)T * maxN;
    const float m0 = depth_min_fold(pmin0, b);
    double Ki0[4];
    kinv(K0, k_dtype, b, Ki0);
    const float *d0m = depth0 + (size_t)b * H * W;
    double *oP = P + (size_t)b * pool * 3, *oQ = Q + (size_t)b * pool * 3;
    int32_t *os = src + (size_t)b * pool;
    int total = 0;
    long long nc = 0;
    for (int j = 0; j < T; ++j) {
        const size_t row = (size_t)b * T + j;
        int n = n_corr[row];
        if (n > 0) nc += n;
        if (n > maxN) n = maxN;
        const float m1 = depth_min_fold(pmin1, (int)row);
        double Ki1[4];
        kinv(K1, k_dtype, (int)row, Ki1);
        const double *A = rig + row * 12;
        const float *p0 = pts0 + row * maxN * 2, *p1 = pts1 + row * maxN * 2;
        const float *d1m = depth1 + row * H * W;
        const int before = total;
        for (int start = 0; start < n; start += 256) {
            const int i = start + tid;
            double a[3], c[3];
            bool valid = false;
            if (i < n) {
                const bool v0 = lift_point(p0[2 * i], p0[2 * i + 1], d0m, H, W, m0, Ki0, a);
                const bool v1 = lift_point(p1[2 * i], p1[2 * i + 1], d1m, H, W, m1, Ki1, c);
                valid = v0 && v1;
            }
            const int m = compact256_slot(cs, valid, total);
            if (valid) {
                double cl[3];
                rig_point_to_last(A, c, cl);
                oP[3 * m] = a[0]; oP[3 * m + 1] = a[1]; oP[3 * m + 2] = a[2];
                oQ[3 * m] = cl[0]; oQ[3 * m + 1] = cl[1]; oQ[3 * m + 2] = cl[2];
                os[m] = j * maxN + i;
            }
        }
        if (tid == 0) n_valid[row] = total - before;
    }
    if (tid == 0) { n_pool[b] = total; n_corr_pool[b] = (nc > 0x7fffffffLL) ? 0x7fffffff : (int)nc; }
}

// grid (ceil(T maxN / 256), B): the pooled points within max_corr_dist under the pose proc_select_kernel wrote -- the set its final count
// is the size of -- marked at their ORIGINAL index.  mask_out [B, T maxN] was zeroed by the caller; a sample without a model marks nothing.
__global__ void __launch_bounds__(256) proc_rig_mask_kernel(
    const double *__restrict__ P, const double *__restrict__ Q, const int32_t *__restrict__ src, const int32_t *__restrict__ n_pool,
    int pool, double thr2, const double *__restrict__ R, const double *__restrict__ t, const int32_t *__restrict__ n_inliers,
    const int32_t *__restrict__ status, uint8_t *__restrict__ mask_out)
{
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (status[b] != MFR_ST_OK || n_inliers[b] <= 0 || i >= n_pool[b]) return;
    const double *p = P + ((size_t)b * pool + i) * 3, *q = Q + ((size_t)b * pool + i) * 3;
    if (dist2(R + 9 * b, t + 3 * b, p[0], p[1], p[2], q[0], q[1], q[2]) < thr2) mask_out[(size_t)b * pool + src[(size_t)b * pool + i]] = 1;
}

struct PrWs { float *pm0, *pm1; double *P, *Q; int32_t *nvalid, *counts; double *err2; int32_t *idx; size_t total; };
static PrWs pr_ws(void *base, int B, int maxN, int iters)
{
    WsCarver c(base);
    PrWs w;
    const size_t b = (size_t)B;
    w.pm0 = c.take<float>(MFR_NSEG * b);
    w.pm1 = c.take<float>(MFR_NSEG * b);
    w.P = c.take<double>(3 * b * maxN);
    w.Q = c.take<double>(3 * b * maxN);
    w.nvalid = c.take<int32_t>(b);
    w.counts = c.take<int32_t>(b * iters);
    w.err2 = c.take<double>(b * iters);
    w.idx = c.take<int32_t>(b * maxN);
    w.total = c.off;
    return w;
}

static size_t proc_hyp_smem_bytes(void)
{
    return (size_t)(12 * 256 + 6 * PR_TILE) * sizeof(double) + 256 * sizeof(int) + 256 * sizeof(double);
}

extern "C" {

size_t mfr_procrustes_workspace_bytes(int B, int maxN, int max_iters)
{
    if (B <= 0 || maxN <= 0) return 0;
    if (max_iters < 1) max_iters = 1;
    return pr_ws(nullptr, B, maxN, max_iters).total;
}

int mfr_procrustes_solve_batch(const float *pts0, const float *pts1, const int32_t *n_corr, int B, int maxN,
                               const float *depth0, const float *depth1, int H, int W, const void *K0, const void *K1, int k_dtype,
                               double max_corr_dist, double confidence, int max_iters, uint64_t seed, const int64_t *pair_ids,
                               void *workspace, size_t workspace_bytes, double *R, double *t, int32_t *n_inliers,
                               int32_t *status, int32_t *best_iter, int32_t *iters_run, int32_t *counts_out, void *stream)
{
    if (!pts0 || !pts1 || !n_corr || !depth0 || !depth1 || !K0 || !K1 || !pair_ids || !workspace || !R || !t || !n_inliers ||
        !status || B <= 0 || maxN <= 0 || H <= 0 || W <= 0 || !(max_corr_dist > 0.0) || !k_dtype_ok(k_dtype)) return MFR_E_ARG;
    if (max_iters < 1) max_iters = 1;
    const PrWs w = pr_ws(workspace, B, maxN, max_iters);
    if (workspace_bytes < w.total) return MFR_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    float *pm0 = w.pm0, *pm1 = w.pm1;
    double *P = w.P, *Q = w.Q, *err2 = w.err2;
    int32_t *nvalid = w.nvalid, *counts = w.counts, *idx = w.idx;
    int rc = mfr_depth_min(depth0, B, H, W, pm0, stream);
    if (rc) return rc;
    rc = mfr_depth_min(depth1, B, H, W, pm1, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(proc_lift_kernel, dim3(B), dim3(256), 0, s, pts0, pts1, n_corr, maxN, depth0, depth1, pm0, pm1, H, W, K0,
                       K1, k_dtype, P, Q, nvalid);
    CHECK_LAUNCH();
    const double thr2 = max_corr_dist * max_corr_dist;
    hipLaunchKernelGGL(proc_hyp_kernel, dim3((max_iters + 255) / 256, B), dim3(256), proc_hyp_smem_bytes(), s, P, Q, nvalid, maxN,
                       max_iters, thr2, seed, pair_ids, counts, err2);
    CHECK_LAUNCH();
    hipLaunchKernelGGL(proc_select_kernel, dim3(B), dim3(64), 0, s, P, Q, nvalid, n_corr, maxN, max_iters, thr2, confidence, seed,
                       pair_ids, counts, err2, idx, R, t, n_inliers, status, best_iter, iters_run);
    CHECK_LAUNCH();
    if (counts_out)
        if (hipMemcpyAsync(counts_out, counts, sizeof(int32_t) * (size_t)B * max_iters, hipMemcpyDeviceToDevice, s) != hipSuccess)
            return MFR_E_LAUNCH;
    return 0;
}

// workspace of mfr_rig_procrustes_solve_batch; pool = T maxN
struct PrRigWs { float *pm0, *pm1; double *P, *Q; int32_t *src, *nvalid, *npool, *ncpool, *counts; double *err2; int32_t *idx; size_t total; };
static PrRigWs pr_rig_ws(void *base, int B, int T, int maxN, int iters)
{
    WsCarver c(base);
    PrRigWs w;
    const size_t b = (size_t)B, rows = b * T;
    w.pm0 = c.take<float>(MFR_NSEG * b);
    w.pm1 = c.take<float>(MFR_NSEG * rows);
    w.P = c.take<double>(3 * rows * maxN);
    w.Q = c.take<double>(3 * rows * maxN);
    w.src = c.take<int32_t>(rows * maxN);
    w.nvalid = c.take<int32_t>(rows);
    w.npool = c.take<int32_t>(b);
    w.ncpool = c.take<int32_t>(b);
    w.counts = c.take<int32_t>(b * iters);
    w.err2 = c.take<double>(b * iters);
    w.idx = c.take<int32_t>(rows * maxN);
    w.total = c.off;
    return w;
}

size_t mfr_rig_procrustes_workspace_bytes(int B, int T, int maxN, int max_iters)
{
    if (!rig_dims_ok(B, T, maxN)) return 0;
    if (max_iters < 1) max_iters = 1;
    return pr_rig_ws(nullptr, B, T, maxN, max_iters).total;
}

int mfr_rig_procrustes_solve_batch(const float *pts0, const float *pts1, const int32_t *n_corr, int B, int T, int maxN,
                                   const float *depth0, const float *depth1, int H, int W, const void *K0, const void *K1, int k_dtype,
                                   const double *rig, double max_corr_dist, double confidence, int max_iters, uint64_t seed,
                                   const int64_t *pair_ids, void *workspace, size_t workspace_bytes, double *R, double *t,
                                   int32_t *n_inliers, int32_t *status, uint8_t *inlier_mask, int32_t *n_valid, int32_t *best_iter,
                                   int32_t *iters_run, int32_t *counts_out, void *stream)
{
    if (!pts0 || !pts1 || !n_corr || !depth0 || !depth1 || !K0 || !K1 || !rig || !pair_ids || !workspace || !R || !t || !n_inliers ||
        !status || !rig_dims_ok(B, T, maxN) || H <= 0 || W <= 0 || !(max_corr_dist > 0.0) || !k_dtype_ok(k_dtype)) return MFR_E_ARG;
    if (max_iters < 1) max_iters = 1;
    const PrRigWs w = pr_rig_ws(workspace, B, T, maxN, max_iters);
    if (workspace_bytes < w.total) return MFR_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int rows = B * T, pool = T * maxN;
    int32_t *nvalid = n_valid ? n_valid : w.nvalid;
    int rc = mfr_depth_min(depth0, B, H, W, w.pm0, stream);
    if (rc) return rc;
    rc = mfr_depth_min(depth1, rows, H, W, w.pm1, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(proc_rig_lift_kernel, dim3(B), dim3(256), 0, s, pts0, pts1, n_corr, T, maxN, depth0, depth1, w.pm0, w.pm1, H, W,
                       K0, K1, k_dtype, rig, w.P, w.Q, w.src, nvalid, w.npool, w.ncpool);
    CHECK_LAUNCH();
    // the single-frame RANSAC on the pooled list: rows of T maxN points
    const double thr2 = max_corr_dist * max_corr_dist;
    hipLaunchKernelGGL(proc_hyp_kernel, dim3((max_iters + 255) / 256, B), dim3(256), proc_hyp_smem_bytes(), s, w.P, w.Q, w.npool, pool,
                       max_iters, thr2, seed, pair_ids, w.counts, w.err2);
    CHECK_LAUNCH();
    hipLaunchKernelGGL(proc_select_kernel, dim3(B), dim3(64), 0, s, w.P, w.Q, w.npool, w.ncpool, pool, max_iters, thr2, confidence, seed,
                       pair_ids, w.counts, w.err2, w.idx, R, t, n_inliers, status, best_iter, iters_run);
    CHECK_LAUNCH();
    if (inlier_mask) {
        if (mfr_zero_async(inlier_mask, (size_t)rows * maxN, s) != hipSuccess) return MFR_E_LAUNCH;
        hipLaunchKernelGGL(proc_rig_mask_kernel, dim3((pool + 255) / 256, B), dim3(256), 0, s, w.P, w.Q, w.src, w.npool, pool, thr2, R, t,
                           n_inliers, status, inlier_mask);
        CHECK_LAUNCH();
    }
    if (counts_out)
        if (hipMemcpyAsync(counts_out, w.counts, sizeof(int32_t) * (size_t)B * max_iters, hipMemcpyDeviceToDevice, s) != hipSuccess)
            return MFR_E_LAUNCH;
    return 0;
}

}  // extern "C"
