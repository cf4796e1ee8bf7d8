// pnp.hip -- PnP path of the relative-pose solver on gfx950 (MI355X).
//
// Replaces PnPSolver.estimate_pose (lib/models/matching/pose_solver.py:184-235) for a BATCH of
// image pairs, device-resident end to end:
//
//   depth_min_kernel      depth_0.min()                                   (:196, quirk Q6)
//   pnp_lift_kernel       (pnp_dev.h) np.int32(pts0) -> depth gather -> valid -> backproject_3d  (:186-206, :6-17)
//   pnp_hyp_score_kernel  cv.solvePnPRansac(P3P) hypotheses + inlier counts (:209-213)
//   pnp_select_kernel     RANSAC best-model replay (adaptive iteration cap), inlier set,
//                         non-minimal refit + ITERATIVE refinement (:216-220), |t|>1000 (:223-225)
//
// RANSAC mapping: hypothesis `it` of pair b is a pure function of (seed, pair_id[b], it)
// (Philox counters), so all max_iters hypotheses are evaluated concurrently -- one LANE per
// minimal solve, then one WAVEFRONT per hypothesis for scoring (lanes stride over the points,
// 64-bit __ballot + popcount gives the inlier count).  OpenCV's sequential early-termination
// rule is then replayed exactly as a prefix-max scan over the counts, so the selected model and
// its inlier set are identical to the sequential CPU loop.
//
// This TU is compiled with -ffp-contract=off (see geom_dev.h for the FP contract).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mfr_hip.h"
#include "zero_fill.h"
#include "solver_dev.h"
#include "pnp_dev.h"

using namespace mfr;

// pnp_hyp_score_kernel: hypotheses per workgroup / threads per workgroup.  Round 5: 256 / 256 -> 64 / 256 -- a wavefront scored the 64 hypotheses its own
// lanes had solved, one after the other (500 wavefronts on 1024 SIMDs at 1000 iterations x 32 pairs); now wavefront 0 solves a workgroup's 64
// hypotheses and all four wavefronts score 16 each.  A hypothesis' count does not depend on the grouping.
#define HYP_BLOCK 64
#define HYP_THREADS 256
#define PT_TILE 768          // points staged in LDS per tile (24 KB models + 30 KB points < 64 KB)

// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) depth_min_kernel(const float *__restrict__ depth, int HW,
                                                        float *__restrict__ partial)
{
    const int b = blockIdx.y, s = blockIdx.x;
    const int seg = (HW + MFR_NSEG - 1) / MFR_NSEG;
    const int lo = s * seg, hi = min(HW, lo + seg);
    const float *d = depth + (size_t)b * HW;
    float m = INFINITY;
    for (int i = lo + (int)threadIdx.x; i < hi; i += 256) {
        const float v = d[i];
        if (v < m) m = v;
    }
    m = wave_min(m);
    __shared__ float sm[4];
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        float r = sm[0];
        for (int w = 1; w < 4; ++w) if (sm[w] < r) r = sm[w];
        partial[b * MFR_NSEG + s] = r;
    }
}

// ------------------------------------------------------------------------------------------
// grid (ceil(iters/256), B).  Phase 1: one lane per hypothesis (sample + P3P + 4th-point
// disambiguation) -> model in LDS.  Phase 2: one wavefront per hypothesis, lanes stride over the
// LDS-staged points, ballot/popcount inlier counting.
__global__ void __launch_bounds__(HYP_THREADS) pnp_hyp_score_kernel(
    const double *__restrict__ xyz, const double *__restrict__ obs, const int32_t *__restrict__ n_valid,
    int maxN, const void *__restrict__ K1, int k_dtype, int max_iters, double thr2, uint64_t seed,
    const int64_t *__restrict__ pair_ids, int32_t *__restrict__ counts)
{
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int n = n_valid[b];
    const int it = blockIdx.x * HYP_BLOCK + tid;                 // tid < HYP_BLOCK: this thread's hypothesis
    int32_t *cnt_out = counts + (size_t)b * max_iters;
    if (n <= 4) {                      // n < 4: no RANSAC; n == 4: handled by the select kernel
        if (tid < HYP_BLOCK && it < max_iters) cnt_out[it] = -1;
        return;
    }
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double *model = (double *)smem_raw;                       // [12][HYP_BLOCK] (transposed: conflict-free)
    double *px = model + 12 * HYP_BLOCK;                      // SoA point tile
    double *py = px + PT_TILE, *pz = py + PT_TILE, *pu = pz + PT_TILE, *pv = pu + PT_TILE;
    int *mvalid = (int *)(pv + PT_TILE);                      // [HYP_BLOCK]
    int *cnt = mvalid + HYP_BLOCK;                            // [HYP_BLOCK]

    const double *X = xyz + (size_t)b * maxN * 3, *O = obs + (size_t)b * maxN * 2;
    double Kd[4];
    kparams(K1, k_dtype, b, Kd);

    if (tid < HYP_BLOCK) {   // phase 1 (wavefront 0)
        double R[9], t[3];
        int ok = 0;
        if (it < max_iters) {
            int s[4];
            sample_distinct<4>(seed, (uint64_t)pair_ids[b], (uint32_t)it, n, s);
            ok = pnp_hypothesis(X, O, s, Kd, R, t);
        }
        mvalid[tid] = ok;
        cnt[tid] = 0;
        if (ok) {
#pragma unroll
            for (int k = 0; k < 9; ++k) model[k * HYP_BLOCK + tid] = R[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) model[(9 + k) * HYP_BLOCK + tid] = t[k];
        }
    }
    // phase 2
    for (int base = 0; base < n; base += PT_TILE) {
        const int tn = min(PT_TILE, n - base);
        __syncthreads();
        for (int i = tid; i < tn; i += HYP_THREADS) {
            const double *p = X + 3 * (size_t)(base + i);
            const double *o = O + 2 * (size_t)(base + i);
            px[i] = p[0]; py[i] = p[1]; pz[i] = p[2]; pu[i] = o[0]; pv[i] = o[1];
        }
        __syncthreads();
        for (int hi = wid; hi < HYP_BLOCK; hi += HYP_THREADS / 64) {
            if (!mvalid[hi]) continue;                         // wave-uniform
            double R[9], t[3];
#pragma unroll
            for (int k = 0; k < 9; ++k) R[k] = model[k * HYP_BLOCK + hi];
#pragma unroll
            for (int k = 0; k < 3; ++k) t[k] = model[(9 + k) * HYP_BLOCK + hi];
            int c = 0;
            for (int i0 = 0; i0 < tn; i0 += 64) {
                const int i = i0 + lane;
                bool in = false;
                if (i < tn) {
                    const double P[3] = { px[i], py[i], pz[i] };
                    const double x2[2] = { pu[i], pv[i] };
                    in = reproj_err2(R, t, P, x2, Kd) <= thr2;
                }
                c += __popcll(__ballot(in));
            }
            if (lane == 0) cnt[hi] += c;
        }
    }
    __syncthreads();
    if (tid < HYP_BLOCK && it < max_iters) cnt_out[it] = mvalid[tid] ? cnt[tid] : 0;
}

// ------------------------------------------------------------------------------------------
// the LM refinement (pnp_lm) lives in pnp_dev.h, shared with pnp_rig.hip; here the model is the camera pose (PnpOneCamera)

// ------------------------------------------------------------------------------------------
// one wavefront per pair: replay of RANSACPointSetRegistrator::run's best-model / adaptive
// iteration-cap logic over the precomputed counts, inlier set, refit + refinement, checks.
__global__ void __launch_bounds__(64) pnp_select_kernel(
    const double *__restrict__ xyz, const double *__restrict__ obs, const int32_t *__restrict__ n_valid,
    const int32_t *__restrict__ pre_status, int maxN, const void *__restrict__ K1, int k_dtype, int max_iters,
    double thr2, double conf, uint64_t seed, const int64_t *__restrict__ pair_ids,
    const int32_t *__restrict__ counts, int32_t *__restrict__ inl_idx,
    double *__restrict__ Rout, double *__restrict__ tout, int32_t *__restrict__ n_inliers,
    int32_t *__restrict__ status, uint8_t *__restrict__ mask_valid, int32_t *__restrict__ best_iter,
    int32_t *__restrict__ iters_run)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    const int n = n_valid[b];
    const double *X = xyz + (size_t)b * maxN * 3, *O = obs + (size_t)b * maxN * 2;
    double Kd[4];
    kparams(K1, k_dtype, b, Kd);
    int32_t *idx = inl_idx + (size_t)b * maxN;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);

    int st = pre_status ? pre_status[b] : MFR_ST_OK;
    if (st == MFR_ST_OK && n < 4) st = MFR_ST_TOO_FEW;
    int bit = -1, best = 3, run = 0, m = 0;
    double R[9], t[3];
    if (mask_valid)
        for (int i = lane; i < maxN; i += 64) mask_valid[(size_t)b * maxN + i] = 0;

    if (st == MFR_ST_OK) {
        if (n == 4) {
            const int s[4] = { 0, 1, 2, 3 };
            if (pnp_hypothesis(X, O, s, Kd, R, t)) { bit = 0; best = 4; run = 1; } else st = MFR_ST_NO_MODEL;
        } else {
            run = ransac_replay_counts(counts + (size_t)b * max_iters, max_iters, n, conf, 4, best, bit);
            if (bit < 0) st = MFR_ST_NO_MODEL;
            else {
                int s[4];
                sample_distinct<4>(seed, (uint64_t)pair_ids[b], (uint32_t)bit, n, s);
                if (!pnp_hypothesis(X, O, s, Kd, R, t)) st = MFR_ST_NO_MODEL;   // cannot happen (count > 3)
            }
        }
    }
    if (st == MFR_ST_OK) {
        // inlier list of the best model (ascending index order)
        for (int i0 = 0; i0 < n; i0 += 64) {
            const int i = i0 + lane;
            bool in = false;
            if (i < n) in = (n == 4) ? true : (reproj_err2(R, t, X + 3 * (size_t)i, O + 2 * (size_t)i, Kd) <= thr2);
            wave_compact_append(in, i, idx, m);
            if (mask_valid && i < n) mask_valid[(size_t)b * maxN + i] = in ? 1 : 0;
        }
        __threadfence();          // idx[] written by other lanes of this wave is read below
        if (n > 4) {
            const PnpOneCamera cam = { Kd };
            if (pnp_lm(X, O, idx, m, cam, 20, R, t)) st = MFR_ST_NO_MODEL;
            if (st == MFR_ST_OK && m >= 6)
                if (pnp_lm(X, O, idx, m, cam, 20, R, t)) st = MFR_ST_NO_MODEL;   // pose_solver.py:216-220
        }
    }
    if (st == MFR_ST_OK) {
        bool bad = !is_rotation(R);                                             // OK needs a finite rotation ...
        for (int k = 0; k < 3; ++k) bad |= !isfinite(t[k]);                    // ... and a finite translation
        if (bad) st = MFR_ST_NO_MODEL;
    }
    if (st == MFR_ST_OK) {
        const double tn = sqrt(dot3(t, t));
        if (tn > 1000.0) st = MFR_ST_DEGENERATE;                                 // pose_solver.py:223-225
    }
    if (st != MFR_ST_OK && mask_valid)                       // a failed pair has no inliers (each lane clears what it wrote above)
        for (int i = lane; i < n; i += 64) mask_valid[(size_t)b * maxN + i] = 0;
    if (lane == 0) {
        for (int k = 0; k < 9; ++k) Rout[9 * b + k] = (st == MFR_ST_OK) ? R[k] : qnan;
        for (int k = 0; k < 3; ++k) tout[3 * b + k] = (st == MFR_ST_OK) ? t[k] : qnan;
        n_inliers[b] = (st == MFR_ST_OK) ? m : 0;
        status[b] = st;
        if (best_iter) best_iter[b] = bit;
        if (iters_run) iters_run[b] = run;
    }
}

// pre-status: too-few / bad-depth decided from counts (pose_solver.py:188-189,197-198)
__global__ void pnp_prestatus_kernel(const int32_t *n_corr, const int32_t *n_valid, int B, int32_t *pre)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int st = MFR_ST_OK;
    if (n_corr[b] < 4) st = MFR_ST_TOO_FEW;
    else if (n_valid[b] < 4) st = MFR_ST_BAD_DEPTH;
    pre[b] = st;
}

// scatter the inlier mask over lifted points back to original correspondence indices
__global__ void pnp_mask_scatter_kernel(const uint8_t *mask_valid, const int32_t *src_idx, const int32_t *n_valid,
                                        const int32_t *status, int maxN, uint8_t *mask_out)
{
    const int b = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= maxN) return;
    // mask_out was zeroed by the caller-side memset node
    if (status[b] == MFR_ST_OK && i < n_valid[b] && mask_valid[(size_t)b * maxN + i])
        mask_out[(size_t)b * maxN + src_idx[(size_t)b * maxN + i]] = 1;
}

// ------------------------------------------------------------------------------------------
// test hooks
__global__ void f64_ops_kernel(const double *a, const double *b, const double *c, int n, double *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[3 * i] = a[i] / b[i];
    out[3 * i + 1] = sqrt(a[i] < 0 ? -a[i] : a[i]);
    out[3 * i + 2] = a[i] * b[i] + c[i];
}
template <int K>
__global__ void sample_kernel(uint64_t seed, const int64_t *pair_ids, int iters, int n, int32_t *out)
{
    const int b = blockIdx.y;
    const int it = blockIdx.x * blockDim.x + threadIdx.x;
    if (it >= iters) return;
    int s[K];
    sample_distinct<K>(seed, (uint64_t)pair_ids[b], (uint32_t)it, n, s);
    for (int k = 0; k < K; ++k) out[((size_t)b * iters + it) * K + k] = s[k];
}

// one wavefront per row of counts: ransac_replay_counts alone (n points per row, confidence conf)
__global__ void __launch_bounds__(64) replay_counts_kernel(const int32_t *counts, int max_iters, int n, double conf, int model_points,
                                                           int32_t *out)
{
    int best, bit;
    const int run = ransac_replay_counts(counts + (size_t)blockIdx.x * max_iters, max_iters, n, conf, model_points, best, bit);
    if (threadIdx.x == 0) { out[3 * blockIdx.x] = best; out[3 * blockIdx.x + 1] = bit; out[3 * blockIdx.x + 2] = run; }
}

// ------------------------------------------------------------------------------------------
// C-ABI
extern "C" {

int mfr_abi_version(void) { return MFR_ABI_VERSION; }
const char *mfr_target_arch(void) { return "gfx950"; }

int mfr_test_f64_ops(const double *a, const double *b, const double *c, int n, double *out3, void *stream)
{
    if (!a || !b || !c || !out3 || n < 0) return MFR_E_ARG;
    if (n == 0) return 0;
    hipLaunchKernelGGL(f64_ops_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, a, b, c, n, out3);
    CHECK_LAUNCH();
    return 0;
}

int mfr_test_sample(uint64_t seed, const int64_t *pair_ids, int B, int iters, int n, int k, int32_t *out, void *stream)
{
    if (!pair_ids || !out || B <= 0 || iters <= 0 || n < k || (k != 4 && k != 5)) return MFR_E_ARG;
    dim3 grid((iters + 255) / 256, B);
    if (k == 4) hipLaunchKernelGGL(sample_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, seed, pair_ids, iters, n, out);
    else hipLaunchKernelGGL(sample_kernel<5>, grid, dim3(256), 0, (hipStream_t)stream, seed, pair_ids, iters, n, out);
    CHECK_LAUNCH();
    return 0;
}

// test hook of the shared count replay, kept out of the public header: counts [B,max_iters] -> out [B,3] = (best, bit, run)
int mfr_test_replay_counts(const int32_t *counts, int B, int max_iters, int n, double conf, int model_points, int32_t *out, void *stream)
{
    if (!counts || !out || B <= 0 || max_iters <= 0 || n < model_points || (model_points != 4 && model_points != 5)) return MFR_E_ARG;
    hipLaunchKernelGGL(replay_counts_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, counts, max_iters, n, conf, model_points, out);
    CHECK_LAUNCH();
    return 0;
}

int mfr_depth_min(const float *depth, int B, int H, int W, float *partial_min, void *stream)
{
    if (!depth || !partial_min || B <= 0 || H <= 0 || W <= 0) return MFR_E_ARG;
    hipLaunchKernelGGL(depth_min_kernel, dim3(MFR_NSEG, B), dim3(256), 0, (hipStream_t)stream, depth, H * W, partial_min);
    CHECK_LAUNCH();
    return 0;
}

int mfr_pnp_lift(const float *pts0, const float *pts1, const int32_t *n_corr, int B, int maxN,
                 const float *depth0, const float *partial_min, int H, int W, const void *K0, int k_dtype,
                 double *xyz, double *obs, int32_t *src_idx, int32_t *n_valid, void *stream)
{
    if (!pts0 || !pts1 || !n_corr || !depth0 || !partial_min || !K0 || !xyz || !obs || !src_idx || !n_valid ||
        B <= 0 || maxN <= 0 || H <= 0 || W <= 0 || !k_dtype_ok(k_dtype)) return MFR_E_ARG;
    hipLaunchKernelGGL(pnp_lift_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, pts0, pts1, n_corr, maxN,
                       depth0, partial_min, H, W, K0, k_dtype, 1, xyz, obs, src_idx, n_valid);
    CHECK_LAUNCH();
    return 0;
}

static size_t hyp_smem_bytes(void)
{
    return (size_t)(12 * HYP_BLOCK + 5 * PT_TILE) * sizeof(double) + 2 * HYP_BLOCK * sizeof(int);
}

static int launch_ransac(const double *xyz, const double *obs, const int32_t *n_valid, const int32_t *pre_status,
                         int B, int maxN, const void *K1, int k_dtype, int max_iters, double thr, double conf, uint64_t seed,
                         const int64_t *pair_ids, int32_t *counts, int32_t *inl_idx, double *R, double *t,
                         int32_t *n_inliers, int32_t *status, uint8_t *mask_valid, int32_t *best_iter,
                         int32_t *iters_run, hipStream_t s)
{
    const double thr2 = thr * thr;
    hipLaunchKernelGGL(pnp_hyp_score_kernel, dim3((max_iters + HYP_BLOCK - 1) / HYP_BLOCK, B), dim3(HYP_THREADS),
                       hyp_smem_bytes(), s, xyz, obs, n_valid, maxN, K1, k_dtype, max_iters, thr2, seed, pair_ids, counts);
    CHECK_LAUNCH();
    hipLaunchKernelGGL(pnp_select_kernel, dim3(B), dim3(64), 0, s, xyz, obs, n_valid, pre_status, maxN, K1, k_dtype, max_iters,
                       thr2, conf, seed, pair_ids, counts, inl_idx, R, t, n_inliers, status, mask_valid, best_iter,
                       iters_run);
    CHECK_LAUNCH();
    return 0;
}

int mfr_pnp_ransac(const double *xyz, const double *obs, const int32_t *n_valid, int B, int maxN,
                   const void *K1, int k_dtype, int max_iters, double reproj_thr, double confidence,
                   uint64_t seed, const int64_t *pair_ids, int32_t *counts, int32_t *inl_idx,
                   double *R, double *t, int32_t *n_inliers, int32_t *status, uint8_t *mask_valid,
                   int32_t *best_iter, int32_t *iters_run, void *stream)
{
    if (!xyz || !obs || !n_valid || !K1 || !pair_ids || !counts || !inl_idx || !R || !t || !n_inliers || !status ||
        B <= 0 || maxN <= 0 || !k_dtype_ok(k_dtype)) return MFR_E_ARG;
    if (max_iters < 1) max_iters = 1;
    return launch_ransac(xyz, obs, n_valid, nullptr, B, maxN, K1, k_dtype, max_iters, reproj_thr, confidence, seed, pair_ids,
                         counts, inl_idx, R, t, n_inliers, status, mask_valid, best_iter, iters_run, (hipStream_t)stream);
}

// workspace of mfr_pnp_solve_batch
struct PnpWs { float *partial; double *xyz, *obs; int32_t *src, *nvalid, *pre, *counts, *inl; uint8_t *maskv; size_t total; };
static PnpWs pnp_ws(void *base, int B, int maxN, int max_iters)
{
    WsCarver c(base);
    PnpWs w;
    const size_t b = (size_t)B;
    w.partial = c.take<float>(MFR_NSEG * b);
    w.xyz = c.take<double>(3 * b * maxN);
    w.obs = c.take<double>(2 * b * maxN);
    w.src = c.take<int32_t>(b * maxN);
    w.nvalid = c.take<int32_t>(b);
    w.pre = c.take<int32_t>(b);
    w.counts = c.take<int32_t>(b * max_iters);
    w.inl = c.take<int32_t>(b * maxN);
    w.maskv = c.take<uint8_t>(b * maxN);
    w.total = c.off;
    return w;
}

size_t mfr_pnp_workspace_bytes(int B, int maxN, int max_iters)
{
    if (B <= 0 || maxN <= 0) return 0;
    if (max_iters < 1) max_iters = 1;
    return pnp_ws(nullptr, B, maxN, max_iters).total;
}

int mfr_pnp_solve_batch(const float *pts0, const float *pts1, const int32_t *n_corr, int B, int maxN,
                        const float *depth0, int H, int W, const void *K0, const void *K1, int k_dtype,
                        int max_iters, double reproj_thr, double confidence, uint64_t seed, const int64_t *pair_ids,
                        void *workspace, size_t workspace_bytes,
                        double *R, double *t, int32_t *n_inliers, int32_t *status, uint8_t *inlier_mask, void *stream)
{
    if (!pts0 || !pts1 || !n_corr || !depth0 || !K0 || !K1 || !pair_ids || !workspace || !R || !t || !n_inliers ||
        !status || B <= 0 || maxN <= 0 || H <= 0 || W <= 0 || !k_dtype_ok(k_dtype)) return MFR_E_ARG;
    if (max_iters < 1) max_iters = 1;
    const PnpWs w = pnp_ws(workspace, B, maxN, max_iters);
    if (workspace_bytes < w.total) return MFR_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;

    int rc = mfr_depth_min(depth0, B, H, W, w.partial, stream);
    if (rc) return rc;
    rc = mfr_pnp_lift(pts0, pts1, n_corr, B, maxN, depth0, w.partial, H, W, K0, k_dtype, w.xyz, w.obs, w.src, w.nvalid, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(pnp_prestatus_kernel, dim3((B + 63) / 64), dim3(64), 0, s, n_corr, w.nvalid, B, w.pre);
    CHECK_LAUNCH();
    rc = launch_ransac(w.xyz, w.obs, w.nvalid, w.pre, B, maxN, K1, k_dtype, max_iters, reproj_thr, confidence, seed, pair_ids, w.counts,
                       w.inl, R, t, n_inliers, status, inlier_mask ? w.maskv : nullptr, nullptr, nullptr, s);
    if (rc) return rc;
    if (inlier_mask) {
        if (mfr_zero_async(inlier_mask, (size_t)B * maxN, s) != hipSuccess) return MFR_E_LAUNCH;
        hipLaunchKernelGGL(pnp_mask_scatter_kernel, dim3((maxN + 255) / 256, B), dim3(256), 0, s, w.maskv, w.src, w.nvalid,
                           status, maxN, inlier_mask);
        CHECK_LAUNCH();
    }
    return 0;
}

}  // extern "C"
