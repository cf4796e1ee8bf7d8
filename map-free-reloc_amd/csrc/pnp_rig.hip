// pnp_rig.hip -- PnP RANSAC for a calibrated camera RIG on gfx950 (MI355X): one pose for T query frames.
//
// The Map-free multi-frame track hands over a window of T query frames together with the device-tracking poses of the scene
// (datasets.MapFreeSceneMultiFrame: `rig_T`).  Those make the window a rig: A_j = (R_Aj, t_Aj) maps coordinates in the LAST frame's
// camera to coordinates in frame j's camera.  The model is (R, t) from the reference view to the last frame; a reference point X is seen
// in frame j at  R_Aj (R X + t) + t_Aj,  projected with K_j.  Upstream has no such solver (it regresses against the last frame alone);
// the yardstick is the numpy mirror tests/rig_pnp_ref.py, and with T = 1 and the identity rig this solver IS pnp.hip, bit for bit.
//
//   pnp_lift_kernel           (pnp_dev.h) every window frame's correspondences against the ONE reference depth map
//   rig_hyp_score_kernel      hypothesis = a frame drawn among the eligible ones + P3P on four of its points, carried to the last frame;
//                             its count is the sum of the inlier counts over all frames
//   rig_select_kernel         replay of the adaptive iteration cap over the pooled counts, pooled inlier list, LM over the six pose
//                             parameters with every residual going through its frame's (A_j, K_j), finite / |t| > 1000 checks
//
// Hypothesis `it` of sample b is a pure function of (seed, pair_id, it):
//   - frame j is eligible when n_valid[b T + j] >= 5;
//   - one eligible frame: it is taken and no random word is consumed; more: the e-th eligible frame in frame order with
//     e = umulhi(w, n_eligible), w = word 0 of Philox4x32-10 at counter (it, RIG_FRAME_CTR, lo(pair_id T), hi(pair_id T)) under the seed
//     as key.  sample_distinct uses counter word 1 = 0 and 1 only, so the frame draw shares no block with a point draw;
//   - the four points are sample_distinct<4>(seed, pair_id T + j, it, n_j); pnp_hypothesis with K_j gives (R', t') reference -> j;
//   - the model is R = R_Aj^T R', t = R_Aj^T (t' - t_Aj).
//
// Layout: row b T + j of xyz / obs / n_valid / K1 is frame j of sample b ([B T, maxN] rows as mfr_pnp_lift writes them); rig [B,T,12]
// f64 = R_Aj row-major, then t_Aj.  The pooled index of point i of frame j is j maxN + i (ascending = (frame, index) order).
//
// This TU is compiled with -ffp-contract=off (see geom_dev.h for the FP contract).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mfr_hip.h"
#include "zero_fill.h"
#include "solver_dev.h"
#include "pnp_dev.h"
#include "rig_dev.h"

using namespace mfr;

#define HYP_BLOCK 64         // hypotheses per workgroup: solved by wavefront 0, scored by all four (as pnp_hyp_score_kernel)
#define HYP_THREADS 256
#define PT_TILE 768          // points of ONE frame staged in LDS per tile (6 KB models + 6 KB composed + 30 KB points < 64 KB)
#define RIG_FRAME_CTR 0x80000000u

// ------------------------------------------------------------------------------------------
// rig_compose / rig_to_last: rig_dev.h

// what both kernels know about sample b
struct RigSample {
    const double *X, *O;          // row b T of xyz / obs: pooled indexing
    const int32_t *nv;            // n_valid + b T
    const double *rig;            // [T,12]
    const void *K1; int k_dtype, row0, T, maxN;
    __device__ __forceinline__ int n(int j) const { const int v = nv[j]; return v < 0 ? 0 : (v > maxN ? maxN : v); }
    __device__ __forceinline__ void kd(int j, double Kd[4]) const { kparams(K1, k_dtype, row0 + j, Kd); }
    __device__ __forceinline__ const double *A(int j) const { return rig + 12 * j; }
};
MFR_DEV RigSample rig_sample(const double *xyz, const double *obs, const int32_t *n_valid, const double *rig, const void *K1,
                             int k_dtype, int b, int T, int maxN)
{
    RigSample s;
    s.X = xyz + (size_t)b * T * maxN * 3; s.O = obs + (size_t)b * T * maxN * 2;
    s.nv = n_valid + (size_t)b * T; s.rig = rig + (size_t)b * T * 12;
    s.K1 = K1; s.k_dtype = k_dtype; s.row0 = b * T; s.T = T; s.maxN = maxN;
    return s;
}
// frames with n_valid >= min_pts: their number, `first` the lowest (T if none)
MFR_DEV int rig_count_frames(const RigSample &s, int min_pts, int &first)
{
    int ne = 0;
    first = s.T;
    for (int j = 0; j < s.T; ++j)
        if (s.n(j) >= min_pts) { if (ne == 0) first = j; ++ne; }
    return ne;
}
// the minimal solve in frame j on sample points smp[4], carried to the last frame
MFR_DEV int rig_solve_in_frame(const RigSample &s, int j, const int *smp, double *R, double *t)
{
    double Kd[4], Rp[9], tp[3];
    s.kd(j, Kd);
    if (!pnp_hypothesis(s.X + 3 * (size_t)j * s.maxN, s.O + 2 * (size_t)j * s.maxN, smp, Kd, Rp, tp)) return 0;
    rig_to_last(s.A(j), Rp, tp, R, t);
    return 1;
}
// hypothesis `it` (header); ne >= 1 eligible frames
MFR_DEV int rig_hypothesis(const RigSample &s, int ne, uint64_t seed, uint64_t pair_id, uint32_t it, double *R, double *t)
{
    const uint64_t id0 = pair_id * (uint64_t)s.T;
    int e = 0;
    if (ne > 1) {
        uint32_t w[4];
        philox4x32_10(it, RIG_FRAME_CTR, (uint32_t)id0, (uint32_t)(id0 >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), w);
        e = (int)__umulhi(w[0], (uint32_t)ne);
    }
    int j = 0;
    for (int k = 0, seen = 0; k < s.T; ++k)
        if (s.n(k) >= 5) { if (seen == e) j = k; ++seen; }
    int smp[4];
    sample_distinct<4>(seed, id0 + (uint64_t)j, it, s.n(j), smp);
    return rig_solve_in_frame(s, j, smp, R, t);
}

// ------------------------------------------------------------------------------------------
// grid (ceil(iters / 64), B).  Phase 1: one lane of wavefront 0 per hypothesis -> model in LDS.  Phase 2: frame by frame, tile by tile;
// when a frame's first tile is staged wavefront 0 also composes the 12 numbers of every hypothesis for that frame; then one wavefront
// per hypothesis, lanes stride over the LDS-staged points, ballot/popcount inlier counting.
__global__ void __launch_bounds__(HYP_THREADS) rig_hyp_score_kernel(
    const double *__restrict__ xyz, const double *__restrict__ obs, const int32_t *__restrict__ n_valid,
    int T, int maxN, const void *__restrict__ K1, int k_dtype, const double *__restrict__ rig, int max_iters, double thr2,
    uint64_t seed, const int64_t *__restrict__ pair_ids, int32_t *__restrict__ counts)
{
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const RigSample s = rig_sample(xyz, obs, n_valid, rig, K1, k_dtype, b, T, maxN);
    const int it = blockIdx.x * HYP_BLOCK + tid;                 // tid < HYP_BLOCK: this thread's hypothesis
    int32_t *cnt_out = counts + (size_t)b * max_iters;
    int first;
    const int ne = rig_count_frames(s, 5, first);
    if (ne == 0) {                     // no frame to sample from: the select kernel handles what is left
        if (tid < HYP_BLOCK && it < max_iters) cnt_out[it] = -1;
        return;
    }
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double *model = (double *)smem_raw;                       // [12][HYP_BLOCK] (transposed: conflict-free)
    double *comp = model + 12 * HYP_BLOCK;                    // [12][HYP_BLOCK] the model seen from the current frame
    double *px = comp + 12 * HYP_BLOCK;                       // SoA point tile
    double *py = px + PT_TILE, *pz = py + PT_TILE, *pu = pz + PT_TILE, *pv = pu + PT_TILE;
    int *mvalid = (int *)(pv + PT_TILE);                      // [HYP_BLOCK]
    int *cnt = mvalid + HYP_BLOCK;                            // [HYP_BLOCK]

    if (tid < HYP_BLOCK) {   // phase 1 (wavefront 0)
        double R[9], t[3];
        int ok = 0;
        if (it < max_iters) ok = rig_hypothesis(s, ne, seed, (uint64_t)pair_ids[b], (uint32_t)it, R, t);
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
    for (int j = 0; j < T; ++j) {
        const int n = s.n(j);
        const double *X = s.X + 3 * (size_t)j * maxN, *O = s.O + 2 * (size_t)j * maxN;
        double Kd[4];
        s.kd(j, Kd);
        for (int base = 0; base < n; base += PT_TILE) {
            const int tn = min(PT_TILE, n - base);
            __syncthreads();
            for (int i = tid; i < tn; i += HYP_THREADS) {
                const double *p = X + 3 * (size_t)(base + i);
                const double *o = O + 2 * (size_t)(base + i);
                px[i] = p[0]; py[i] = p[1]; pz[i] = p[2]; pu[i] = o[0]; pv[i] = o[1];
            }
            if (base == 0 && tid < HYP_BLOCK && mvalid[tid]) {     // mvalid[tid] was written by this thread
                double R[9], t[3], Rc[9], tc[3];
#pragma unroll
                for (int k = 0; k < 9; ++k) R[k] = model[k * HYP_BLOCK + tid];
#pragma unroll
                for (int k = 0; k < 3; ++k) t[k] = model[(9 + k) * HYP_BLOCK + tid];
                rig_compose(s.A(j), R, t, Rc, tc);
#pragma unroll
                for (int k = 0; k < 9; ++k) comp[k * HYP_BLOCK + tid] = Rc[k];
#pragma unroll
                for (int k = 0; k < 3; ++k) comp[(9 + k) * HYP_BLOCK + tid] = tc[k];
            }
            __syncthreads();
            for (int hi = wid; hi < HYP_BLOCK; hi += HYP_THREADS / 64) {
                if (!mvalid[hi]) continue;                         // wave-uniform
                double R[9], t[3];
#pragma unroll
                for (int k = 0; k < 9; ++k) R[k] = comp[k * HYP_BLOCK + hi];
#pragma unroll
                for (int k = 0; k < 3; ++k) t[k] = comp[(9 + k) * HYP_BLOCK + hi];
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
    }
    __syncthreads();
    if (tid < HYP_BLOCK && it < max_iters) cnt_out[it] = mvalid[tid] ? cnt[tid] : 0;
}

// ------------------------------------------------------------------------------------------
// the rig as pnp_lm's camera: pooled index p -> frame p / maxN
struct PnpRigCamera {
    RigSample s;
    __device__ __forceinline__ void kd(int p, double out[4]) const { s.kd(p / s.maxN, out); }
    __device__ __forceinline__ void to_cam(int p, double *Y) const
    {
        const double *A = s.A(p / s.maxN);
        double Yc[3];
        rot_apply(A, A + 9, Y, Yc);
        Y[0] = Yc[0]; Y[1] = Yc[1]; Y[2] = Yc[2];
    }
    __device__ __forceinline__ void jac(int p, double (*G)[6]) const
    {
        const double *A = s.A(p / s.maxN);
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const double g0 = G[0][k], g1 = G[1][k], g2 = G[2][k];
#pragma unroll
            for (int r = 0; r < 3; ++r) G[r][k] = (A[3 * r] * g0 + A[3 * r + 1] * g1) + A[3 * r + 2] * g2;
        }
    }
};

// one wavefront per sample
__global__ void __launch_bounds__(64) rig_select_kernel(
    const double *__restrict__ xyz, const double *__restrict__ obs, const int32_t *__restrict__ n_valid,
    const int32_t *__restrict__ pre_status, int T, int maxN, const void *__restrict__ K1, int k_dtype,
    const double *__restrict__ rig, int max_iters, double thr2, double conf, uint64_t seed, const int64_t *__restrict__ pair_ids,
    const int32_t *__restrict__ counts, int32_t *__restrict__ inl_idx,
    double *__restrict__ Rout, double *__restrict__ tout, int32_t *__restrict__ n_inliers,
    int32_t *__restrict__ status, uint8_t *__restrict__ mask_valid, int32_t *__restrict__ best_iter,
    int32_t *__restrict__ iters_run)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    const RigSample s = rig_sample(xyz, obs, n_valid, rig, K1, k_dtype, b, T, maxN);
    const size_t pool = (size_t)T * maxN;
    int32_t *idx = inl_idx + (size_t)b * pool;
    uint8_t *mask = mask_valid ? mask_valid + (size_t)b * pool : nullptr;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);

    int N = 0;
    for (int j = 0; j < T; ++j) N += s.n(j);
    int first4, first5;
    const int n4 = rig_count_frames(s, 4, first4), ne = rig_count_frames(s, 5, first5);
    int st = pre_status ? pre_status[b] : MFR_ST_OK;
    if (st == MFR_ST_OK && n4 == 0) st = MFR_ST_TOO_FEW;
    int bit = -1, best = 3, run = 0, m = 0;
    int fixed = -1;                    // the frame of the fixed sample {0,1,2,3}: its four points are inliers as in pnp_select_kernel
    double R[9], t[3];
    if (mask)                          // lane i % 64 owns point i of every frame, here and below
        for (int j = 0; j < T; ++j)
            for (int i = lane; i < maxN; i += 64) mask[(size_t)j * maxN + i] = 0;

    if (st == MFR_ST_OK) {
        if (ne == 0) {
            const int smp[4] = { 0, 1, 2, 3 };
            fixed = first4;
            if (rig_solve_in_frame(s, fixed, smp, R, t)) { bit = 0; best = 4; run = 1; } else st = MFR_ST_NO_MODEL;
        } else {
            run = ransac_replay_counts(counts + (size_t)b * max_iters, max_iters, N, conf, 4, best, bit);
            if (bit < 0) st = MFR_ST_NO_MODEL;
            else if (!rig_hypothesis(s, ne, seed, (uint64_t)pair_ids[b], (uint32_t)bit, R, t)) st = MFR_ST_NO_MODEL;   // cannot happen (count > 3)
        }
    }
    if (st == MFR_ST_OK) {
        // pooled inlier list of the best model (ascending (frame, index) order)
        for (int j = 0; j < T; ++j) {
            const int n = s.n(j);
            if (n == 0) continue;
            double Kd[4], Rc[9], tc[3];
            s.kd(j, Kd);
            rig_compose(s.A(j), R, t, Rc, tc);
            const double *X = s.X + 3 * (size_t)j * maxN, *O = s.O + 2 * (size_t)j * maxN;
            for (int i0 = 0; i0 < n; i0 += 64) {
                const int i = i0 + lane;
                bool in = false;
                if (i < n) in = (j == fixed) ? true : (reproj_err2(Rc, tc, X + 3 * (size_t)i, O + 2 * (size_t)i, Kd) <= thr2);
                wave_compact_append(in, j * maxN + i, idx, m);
                if (mask && i < n) mask[(size_t)j * maxN + i] = in ? 1 : 0;
            }
        }
        __threadfence();          // idx[] written by other lanes of this wave is read below
        if (N > 4) {
            const PnpRigCamera cam = { s };
            if (pnp_lm(s.X, s.O, idx, m, cam, 20, R, t)) st = MFR_ST_NO_MODEL;
            if (st == MFR_ST_OK && m >= 6)
                if (pnp_lm(s.X, s.O, idx, m, cam, 20, R, t)) st = MFR_ST_NO_MODEL;
        }
    }
    if (st == MFR_ST_OK) {
        bool bad = !is_rotation(R);
        for (int k = 0; k < 3; ++k) bad |= !isfinite(t[k]);
        if (bad) st = MFR_ST_NO_MODEL;
    }
    if (st == MFR_ST_OK) {
        const double tn = sqrt(dot3(t, t));
        if (tn > 1000.0) st = MFR_ST_DEGENERATE;
    }
    if (st != MFR_ST_OK && mask)                             // a failed sample has no inliers (each lane clears what it wrote above)
        for (int j = 0; j < T; ++j)
            for (int i = lane; i < s.n(j); i += 64) mask[(size_t)j * maxN + i] = 0;
    if (lane == 0) {
        for (int k = 0; k < 9; ++k) Rout[9 * b + k] = (st == MFR_ST_OK) ? R[k] : qnan;
        for (int k = 0; k < 3; ++k) tout[3 * b + k] = (st == MFR_ST_OK) ? t[k] : qnan;
        n_inliers[b] = (st == MFR_ST_OK) ? m : 0;
        status[b] = st;
        if (best_iter) best_iter[b] = bit;
        if (iters_run) iters_run[b] = run;
    }
}

// pre-status of a sample from its frames' counts: no frame with 4 correspondences -> TOO_FEW, else none with 4 valid depths -> BAD_DEPTH
__global__ void rig_prestatus_kernel(const int32_t *n_corr, const int32_t *n_valid, int B, int T, int32_t *pre)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    bool corr4 = false, valid4 = false;
    for (int j = 0; j < T; ++j) {
        corr4 |= n_corr[(size_t)b * T + j] >= 4;
        valid4 |= n_valid[(size_t)b * T + j] >= 4;
    }
    pre[b] = !corr4 ? MFR_ST_TOO_FEW : !valid4 ? MFR_ST_BAD_DEPTH : MFR_ST_OK;
}

// scatter the inlier mask over lifted points back to original correspondence indices; row = b T + j
__global__ void rig_mask_scatter_kernel(const uint8_t *mask_valid, const int32_t *src_idx, const int32_t *n_valid,
                                        const int32_t *status, int T, int maxN, uint8_t *mask_out)
{
    const int row = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= maxN) return;
    // mask_out was zeroed by the caller-side zero fill
    if (status[row / T] == MFR_ST_OK && i < n_valid[row] && mask_valid[(size_t)row * maxN + i])
        mask_out[(size_t)row * maxN + src_idx[(size_t)row * maxN + i]] = 1;
}

// ------------------------------------------------------------------------------------------
// C-ABI
extern "C" {

static size_t rig_hyp_smem_bytes(void)
{
    return (size_t)(24 * HYP_BLOCK + 5 * PT_TILE) * sizeof(double) + 2 * HYP_BLOCK * sizeof(int);
}

static int rig_launch_ransac(const double *xyz, const double *obs, const int32_t *n_valid, const int32_t *pre_status,
                             int B, int T, int maxN, const void *K1, int k_dtype, const double *rig, int max_iters, double thr,
                             double conf, uint64_t seed, const int64_t *pair_ids, int32_t *counts, int32_t *inl_idx, double *R,
                             double *t, int32_t *n_inliers, int32_t *status, uint8_t *mask_valid, int32_t *best_iter,
                             int32_t *iters_run, hipStream_t s)
{
    const double thr2 = thr * thr;
    hipLaunchKernelGGL(rig_hyp_score_kernel, dim3((max_iters + HYP_BLOCK - 1) / HYP_BLOCK, B), dim3(HYP_THREADS),
                       rig_hyp_smem_bytes(), s, xyz, obs, n_valid, T, maxN, K1, k_dtype, rig, max_iters, thr2, seed, pair_ids, counts);
    CHECK_LAUNCH();
    hipLaunchKernelGGL(rig_select_kernel, dim3(B), dim3(64), 0, s, xyz, obs, n_valid, pre_status, T, maxN, K1, k_dtype, rig,
                       max_iters, thr2, conf, seed, pair_ids, counts, inl_idx, R, t, n_inliers, status, mask_valid, best_iter,
                       iters_run);
    CHECK_LAUNCH();
    return 0;
}

int mfr_rig_pnp_ransac(const double *xyz, const double *obs, const int32_t *n_valid, int B, int T, int maxN,
                       const void *K1, int k_dtype, const double *rig, int max_iters, double reproj_thr, double confidence,
                       uint64_t seed, const int64_t *pair_ids, int32_t *counts, int32_t *inl_idx,
                       double *R, double *t, int32_t *n_inliers, int32_t *status, uint8_t *mask_valid,
                       int32_t *best_iter, int32_t *iters_run, void *stream)
{
    if (!xyz || !obs || !n_valid || !K1 || !rig || !pair_ids || !counts || !inl_idx || !R || !t || !n_inliers || !status ||
        !rig_dims_ok(B, T, maxN) || !k_dtype_ok(k_dtype)) return MFR_E_ARG;
    if (max_iters < 1) max_iters = 1;
    return rig_launch_ransac(xyz, obs, n_valid, nullptr, B, T, maxN, K1, k_dtype, rig, max_iters, reproj_thr, confidence, seed,
                             pair_ids, counts, inl_idx, R, t, n_inliers, status, mask_valid, best_iter, iters_run, (hipStream_t)stream);
}

// workspace of mfr_rig_pnp_solve_batch
struct RigWs { float *partial; double *xyz, *obs; int32_t *src, *nvalid, *pre, *counts, *inl; uint8_t *maskv; size_t total; };
static RigWs rig_ws(void *base, int B, int T, int maxN, int max_iters)
{
    WsCarver c(base);
    RigWs w;
    const size_t b = (size_t)B, rows = b * T;
    w.partial = c.take<float>(MFR_NSEG * b);
    w.xyz = c.take<double>(3 * rows * maxN);
    w.obs = c.take<double>(2 * rows * maxN);
    w.src = c.take<int32_t>(rows * maxN);
    w.nvalid = c.take<int32_t>(rows);
    w.pre = c.take<int32_t>(b);
    w.counts = c.take<int32_t>(b * max_iters);
    w.inl = c.take<int32_t>(rows * maxN);
    w.maskv = c.take<uint8_t>(rows * maxN);
    w.total = c.off;
    return w;
}

size_t mfr_rig_pnp_workspace_bytes(int B, int T, int maxN, int max_iters)
{
    if (!rig_dims_ok(B, T, maxN)) return 0;
    if (max_iters < 1) max_iters = 1;
    return rig_ws(nullptr, B, T, maxN, max_iters).total;
}

int mfr_rig_pnp_solve_batch(const float *pts0, const float *pts1, const int32_t *n_corr, int B, int T, int maxN,
                            const float *depth0, int H, int W, const void *K0, const void *K1, int k_dtype, const double *rig,
                            int max_iters, double reproj_thr, double confidence, uint64_t seed, const int64_t *pair_ids,
                            void *workspace, size_t workspace_bytes,
                            double *R, double *t, int32_t *n_inliers, int32_t *status, uint8_t *inlier_mask, void *stream)
{
    if (!pts0 || !pts1 || !n_corr || !depth0 || !K0 || !K1 || !rig || !pair_ids || !workspace || !R || !t || !n_inliers ||
        !status || !rig_dims_ok(B, T, maxN) || H <= 0 || W <= 0 || !k_dtype_ok(k_dtype)) return MFR_E_ARG;
    if (max_iters < 1) max_iters = 1;
    const RigWs w = rig_ws(workspace, B, T, maxN, max_iters);
    if (workspace_bytes < w.total) return MFR_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int rows = B * T;

    int rc = mfr_depth_min(depth0, B, H, W, w.partial, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(pnp_lift_kernel, dim3(rows), dim3(256), 0, s, pts0, pts1, n_corr, maxN, depth0, w.partial, H, W, K0, k_dtype,
                       T, w.xyz, w.obs, w.src, w.nvalid);
    CHECK_LAUNCH();
    hipLaunchKernelGGL(rig_prestatus_kernel, dim3((B + 63) / 64), dim3(64), 0, s, n_corr, w.nvalid, B, T, w.pre);
    CHECK_LAUNCH();
    rc = rig_launch_ransac(w.xyz, w.obs, w.nvalid, w.pre, B, T, maxN, K1, k_dtype, rig, max_iters, reproj_thr, confidence, seed,
                           pair_ids, w.counts, w.inl, R, t, n_inliers, status, inlier_mask ? w.maskv : nullptr, nullptr, nullptr, s);
    if (rc) return rc;
    if (inlier_mask) {
        if (mfr_zero_async(inlier_mask, (size_t)rows * maxN, s) != hipSuccess) return MFR_E_LAUNCH;
        hipLaunchKernelGGL(rig_mask_scatter_kernel, dim3((maxN + 255) / 256, rows), dim3(256), 0, s, w.maskv, w.src, w.nvalid,
                           status, T, maxN, inlier_mask);
        CHECK_LAUNCH();
    }
    return 0;
}

}  // extern "C"
