/*
 * include/mfr_hip.h -- C-ABI of libmfr_hip.so, the MI355X (gfx950) drop-in for the
 * feature-matching + scale-from-depth relative-pose hot path of
 * nianticlabs/map-free-reloc.
 *
 * Conventions:
 *   - extern "C", plain pointers and sizes; no torch types.  All data pointers are
 *     DEVICE pointers unless the parameter name ends in _host.
 *   - the caller allocates every buffer (including the workspace, whose size is
 *     returned by the matching *_workspace_bytes query); the library keeps no
 *     per-call state and is re-entrant per stream.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).
 *   - return value: 0 = launched OK, <0 = argument / launch error (MFR_E_*).
 *     Per-pair failures are VALUES, like the reference's NaN-pose convention
 *     (pose_solver.py:30-33,188-189,197-198,230-233): status[b] != 0 and R,t filled
 *     with NaN, n_inliers = 0.  A failing pair never aborts the batch.
 *   - batches: leading dim B = image pairs; correspondences are fixed-stride
 *     [B, maxN, 2] float32 with a count n_corr[B] (the device-side twin of the
 *     NaN-padded [Npairs, maxN, 4] npz wire format, utils.py:59-69).
 *   - images are H x W row-major float32.  Intrinsics K are [B,3,3] row-major with zero skew and
 *     bottom row [0,0,1], handed over IN THE DTYPE THE `data` DICT HOLDS THEM, tagged by `k_dtype`
 *     (one tag for K0 and K1):
 *       MFR_K_F64  float64 -- the Map-free loader's flow: correct_intrinsic_scale multiplies a
 *                  float64 np.eye(3) into K (lib/datasets/utils.py:117-130; always called,
 *                  lib/datasets/mapfree.py:50-52, config/mapfree.yaml:7-8), so np.linalg.inv(K)
 *                  (pose_solver.py:16), the K-normalisation (:39-40) and the threshold mean (:43)
 *                  are float64 arithmetic in the reference, and so they are here;
 *       MFR_K_F32  float32 -- resize=None datasets (K stays as parsed): the same three steps are
 *                  float32 arithmetic and only their results are promoted (quirk Q5).
 *     Both flows are pinned bit-for-bit against the reference's own Python
 *     (tests/golden/ref_k64.npz, ref_backproject.npz, ref_pnp_lift.npz, ref_emat_metric.npz).
 *
 * Every entry point names the reference interface it replaces (file:line under
 * the upstream repository).
 */
#ifndef MFR_HIP_H
#define MFR_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MFR_ABI_VERSION 6   /* 6 (round 6): mfr_conv3x3_direct_f16x2*, later (additive) the SIFT detector mfr_sift_*, the JPEG decoder mfr_jpeg_*, the depth PNG decoder mfr_png_depth_*, mfr_resize_gray_bilinear (the device image resize), mfr_conv3x3s2_direct_f16x2, mfr_mlp_ln_*, mfr_loftr_ot_match (LoFTR's optimal-transport coarse matching), mfr_abs_pose_fuse (7Scenes: absolute pose from relative poses), mfr_rig_pnp_* (one pose for a rig of query frames); 5 (round 6): mfr_f16x2_guard_bind (the f16x2 range guard); 2: intrinsics as (const void *K, int k_dtype) instead of const float *; 3: mfr_emat_solve_batch takes the
                             * model-quality method (MAGSAC++ / count) and its table; 4 (round 5): the f16x2 entry points (mfr_gemm_f16x2*,
                             * mfr_wino_f16x2_*, mfr_conv3x3_wino_f16x2, mfr_conv_igemm_f16x2), mfr_sg_attention_variant renumbered (0 f16x2,
                             * 1 exact fp32, 2 bf16x3), the measurement-only entry points (mfr_conv3x3_wino_bf16x3_variant,
                             * mfr_wino_bf16x3_profile, the GEMM ablation flags) removed */

/* intrinsics dtype tags */
#define MFR_K_F32 0
#define MFR_K_F64 1

/* library-level error codes (negative) */
#define MFR_E_ARG      (-1)
#define MFR_E_LAUNCH   (-2)
#define MFR_E_WORKSPACE (-3)

/* per-pair status values (same as oracle/mfr_oracle.h) */
#define MFR_ST_OK          0
#define MFR_ST_TOO_FEW     1   /* fewer correspondences than the solver minimum (Q9) */
#define MFR_ST_BAD_DEPTH   2   /* too few correspondences with valid depth          */
#define MFR_ST_NO_MODEL    3   /* RANSAC produced no model / refinement failed      */
#define MFR_ST_DEGENERATE  4   /* |t| > 1000 (pose_solver.py:223-225)               */

int mfr_abi_version(void);

/* ---- f16x2 range guard (round 6).  The reference's networks are plain fp32 (etc/feature_matching_baselines/matchers.py:50,105 call fp32 PyTorch
 *      modules: no input-range precondition); the f16x2 kernels (mfr_gemm_f16x2*, mfr_conv_igemm_f16x2, mfr_conv3x3_wino_f16x2, mfr_sp_conv1ab_f16x2,
 *      mfr_sg_attention variant 0) represent an activation as two f16 terms and need |x| <= 65504 (Winograd: |x| < 16376).  After
 *      mfr_f16x2_guard_bind(flag) every such launch issued by THIS host thread ORs 1 into *flag (a device int the caller owns and clears) when one of
 *      its fp32 accumulators is NaN / +-inf before the activation -- which is the case for every output that an out-of-range (or non-finite) input
 *      element contributes to (csrc/guard.h).  flag = NULL unbinds (the default: no test).  The bound pointer is the ONE piece of state the library
 *      keeps (thread-local); it is read when a launch is issued, so a captured HIP graph keeps the pointer it was captured with.
 *      Host side: pipeline.py folds the flag into the per-pair status (MFR_ST_RANGE) and re-runs such a batch in the exact bf16x3 arithmetic. ---- */
int mfr_f16x2_guard_bind(int *device_flag);
#define MFR_ST_RANGE 7         /* host-side status (pipeline.py): the f16x2 range guard fired for this batch; no pose unless re-run in bf16x3 */
/* name of the gfx target the kernels were compiled for ("gfx950") */
const char *mfr_target_arch(void);

/* ---- numerics self-test hook: out[i] = {a/b, sqrt(a), a*b+c (unfused)} in f64, used by
 *      tests to prove the host/device IEEE contract the bit-exact parity relies on ---- */
int mfr_test_f64_ops(const double *a, const double *b, const double *c, int n, double *out3, void *stream);
/* raw RNG / sampler exposure for parity tests (oracle: mfr_ref_sample_distinct) */
int mfr_test_sample(uint64_t seed, const int64_t *pair_ids, int B, int iters, int n, int k, int32_t *out, void *stream);

/* ------------------------------------------------------------------------------------------
 * PnP path:  PnPSolver.estimate_pose, lib/models/matching/pose_solver.py:184-235
 *   int-truncate pts0 (:186) -> depth gather (:192-193) -> valid = d > depth.min() (:196, Q6)
 *   -> backproject_3d with K0 (:206, :6-17) -> cv.solvePnPRansac(P3P, iters, thr, conf) (:209-213)
 *   -> refit + cv.solvePnPGeneric(ITERATIVE) when >= 6 inliers (:216-220) -> |t| > 1000 reject.
 * Outputs: R [B,9] f64 row-major, t [B,3] f64, n_inliers [B] i32 (= len(inliers), the
 * submission confidence, model.py:37), status [B] i32, inlier_mask [B,maxN] u8 indexed by
 * the ORIGINAL correspondence index (may be NULL).
 * RNG: Philox4x32-10 keyed by (seed, pair_ids[b], iteration) -- the reference has no seed
 * knob (OpenCV fixed RNG); results are bit-reproducible for fixed (seed, pair_id).
 * ------------------------------------------------------------------------------------------ */
size_t mfr_pnp_workspace_bytes(int B, int maxN, int max_iters);
int mfr_pnp_solve_batch(const float *pts0, const float *pts1, const int32_t *n_corr, int B, int maxN,
                        const float *depth0, int H, int W,
                        const void *K0, const void *K1, int k_dtype,
                        int max_iters, double reproj_thr, double confidence,
                        uint64_t seed, const int64_t *pair_ids,
                        void *workspace, size_t workspace_bytes,
                        double *R, double *t, int32_t *n_inliers, int32_t *status, uint8_t *inlier_mask,
                        void *stream);

/* stage-level entry points of the PnP path (same arithmetic, exposed for parity tests and
 * for callers that already hold lifted 3-D points).  xyz [B,maxN,3] f64, obs [B,maxN,2] f64,
 * src_idx [B,maxN] i32, n_valid [B] i32. */
int mfr_depth_min(const float *depth, int B, int H, int W, float *partial_min /*[B,16]*/, void *stream);
int mfr_pnp_lift(const float *pts0, const float *pts1, const int32_t *n_corr, int B, int maxN,
                 const float *depth0, const float *partial_min, int H, int W, const void *K0, int k_dtype,
                 double *xyz, double *obs, int32_t *src_idx, int32_t *n_valid, void *stream);
int mfr_pnp_ransac(const double *xyz, const double *obs, const int32_t *n_valid, int B, int maxN,
                   const void *K1, int k_dtype, int max_iters, double reproj_thr, double confidence,
                   uint64_t seed, const int64_t *pair_ids,
                   int32_t *counts /*[B,max_iters] workspace*/, int32_t *inl_idx /*[B,maxN] workspace*/,
                   double *R, double *t, int32_t *n_inliers, int32_t *status,
                   uint8_t *mask_valid /*[B,maxN] over lifted points, may be NULL*/,
                   int32_t *best_iter /*[B] may be NULL*/, int32_t *iters_run /*[B] may be NULL*/,
                   void *stream);

/* ------------------------------------------------------------------------------------------
 * Rig PnP path (additive; csrc/pnp_rig.hip): ONE pose for a window of T query frames, the Map-free multi-frame track
 * (config/mapfree_multi.yaml, DATASET.QUERY_FRAME_COUNT; lib/datasets/mapfree.py:285 reads the device-tracking poses that make
 * the window a calibrated rig).  Upstream has no such solver (RegressionMultiFrameModel regresses against the last frame).
 *   Model: (R, t) reference -> LAST window frame.  Frame j sees a reference point X at R_Aj (R X + t) + t_Aj, projected with K_j;
 *   rig [B,T,12] f64 = R_Aj row-major then t_Aj (A_j: last frame's camera -> frame j's camera; the last row is the identity).
 *   Rows: frame j of sample b is row b*T + j of pts0 / pts1 / n_corr / xyz / obs / n_valid / K1 ([B*T,3,3]); depth0 [B,H,W] and
 *   K0 [B,3,3] belong to the one reference view of a sample.  1 <= T <= 16.
 *   Hypothesis `it` of sample b: a frame with n_valid >= 5 (the only one, or drawn uniformly: word 0 of Philox4x32-10 at counter
 *   (it, 0x80000000, lo, hi of pair_id*T), key seed -- sample_distinct uses counter word 1 in {0, 1}), four of its points by
 *   sample_distinct<4>(seed, pair_id*T + j, it, n_j), P3P with K_j, carried to the last frame; its count is summed over ALL frames.
 *   Then as the PnP path: replay of the adaptive iteration cap (N = sum of n_valid), pooled inlier list in (frame, index) order,
 *   LM over the six pose parameters (the same two calls), finite / |t| > 1000 checks.  n_inliers = the pooled RANSAC count.
 *   Status: no frame with n_corr >= 4 -> MFR_ST_TOO_FEW; else none with n_valid >= 4 -> MFR_ST_BAD_DEPTH; else no frame with
 *   n_valid >= 5: the one model is the fixed sample {0,1,2,3} of the first frame with n_valid == 4 (those four are inliers, the
 *   other frames' points are scored; LM only if N > 4).
 *   With T = 1 and the identity rig every output equals mfr_pnp_ransac / mfr_pnp_solve_batch bit for bit.
 * mask_valid / inlier_mask are [B*T,maxN] (lifted points / ORIGINAL correspondence index), counts [B,max_iters],
 * inl_idx [B*T,maxN] workspace.  Bad arguments (T < 1, T > 16, NULL pointers, workspace too small) return MFR_E_* and launch nothing.
 * ------------------------------------------------------------------------------------------ */
size_t mfr_rig_pnp_workspace_bytes(int B, int T, int maxN, int max_iters);
int mfr_rig_pnp_ransac(const double *xyz, const double *obs, const int32_t *n_valid, int B, int T, int maxN,
                       const void *K1, int k_dtype, const double *rig, int max_iters, double reproj_thr, double confidence,
                       uint64_t seed, const int64_t *pair_ids,
                       int32_t *counts /*[B,max_iters] workspace*/, int32_t *inl_idx /*[B*T,maxN] workspace*/,
                       double *R, double *t, int32_t *n_inliers, int32_t *status,
                       uint8_t *mask_valid /*[B*T,maxN] over lifted points, may be NULL*/,
                       int32_t *best_iter /*[B] may be NULL*/, int32_t *iters_run /*[B] may be NULL*/,
                       void *stream);
int mfr_rig_pnp_solve_batch(const float *pts0, const float *pts1, const int32_t *n_corr, int B, int T, int maxN,
                            const float *depth0, int H, int W,
                            const void *K0, const void *K1, int k_dtype, const double *rig,
                            int max_iters, double reproj_thr, double confidence,
                            uint64_t seed, const int64_t *pair_ids,
                            void *workspace, size_t workspace_bytes,
                            double *R, double *t, int32_t *n_inliers, int32_t *status, uint8_t *inlier_mask /*may be NULL*/,
                            void *stream);

/* ------------------------------------------------------------------------------------------
 * Metric scale from depth: EssentialMatrixMetricSolver.estimate_pose, pose_solver.py:137-172
 *   mask == 1 inliers (:137) -> int-truncate both views (:138-139) -> depth gather (:140-141)
 *   -> valid = d0 > 0 & d1 > 0 (:144) -> back-project (:150-151) -> xyz0 <- R xyz0 (:154)
 *   -> scale_i = (xyz1_i - xyz0_i) . t (:157) -> exhaustive 1-D RANSAC, first strict max
 *   (:160-166, Q2) -> t_metric = best_scale * t (:169).
 * R [B,9], t [B,3] f64 inputs (unit translation); outputs t_metric [B,3] f64 (NaN on failure),
 * best_scale [B] f64, n_inliers [B] i32 (scale-consensus count = submission confidence),
 * status [B] (in_status != 0 is passed through: "inliers == 0 -> return", :131-132;
 * no valid depth -> MFR_ST_BAD_DEPTH, :145-149).
 * emat_mask [B,maxN] u8 may be NULL (= all correspondences).
 * ------------------------------------------------------------------------------------------ */
size_t mfr_scale_workspace_bytes(int B, int maxN);
int mfr_scale_from_depth_batch(const float *pts0, const float *pts1, const uint8_t *emat_mask,
                               const int32_t *n_corr, int B, int maxN,
                               const float *depth0, const float *depth1, int H, int W,
                               const void *K0, const void *K1, int k_dtype,
                               const double *R, const double *t,
                               const int32_t *in_status /* [B] status of the E-mat stage, may be NULL */,
                               double scale_thr,
                               void *workspace, size_t workspace_bytes,
                               double *t_metric, double *best_scale, int32_t *n_inliers, int32_t *status,
                               void *stream);

/* ------------------------------------------------------------------------------------------
 * Absolute pose of a query from its relative poses to several database images (7Scenes): lib/utils/localize.py
 *   per pair (RelaPosePair :942-964, AbsPose :896-918): q = mat2quat(R), r = quat2mat(q), x_te, abs_q_pred, abs_c_pred
 *   mode 0  cal_abs_pose_err_metric (:352-421): Weiszfeld geometric median of abs_c_pred (stop |y - y1| < 1e-5, at most
 *           MFR_AP_WEISZFELD_CAP iterations: then the current iterate, status | MFR_AP_ITER_CAP) + chordal mean rotation
 *   mode 1  ransac(pair_type='relapose') (:471-635): every pair of neighbours in combinations order, triangulation +
 *           raw quaternion mean, find_inliers at thr_deg, local_optimisation at thr_mult * thr_deg with lo_iters random
 *           subsets (Philox keyed by seed, query, LO call, iteration); no winner -> the first pair's database pose,
 *           MFR_AP_APPROXIMATED, inlier mask {0}.  At most MFR_AP_MAX_PAIRS neighbours per query (else MFR_AP_TOO_MANY).
 * All pointers are device memory.  train_q [P,4] wxyz, train_c [P,3], pred_R [P,9], pred_t [P,3] f64 (the caller drops pairs
 * without a finite pose); pairs of query i are offsets[i] .. offsets[i+1] (offsets [Q+1] i32, ascending, last <= P).
 * thr_mult >= 1 (else MFR_E_ARG): the local optimisation refits over the inliers at thr_mult * thr_deg, a superset of the >= 2 inliers
 * at thr_deg, so that set is never empty (the reference raises on an empty one).  0 <= lo_iters <= MFR_AP_MAX_LO_ITERS.
 * Outputs abs_q [Q,4] wxyz (mode 1: the unnormalised mean), abs_c [Q,3] (NaN without pairs), inlier_mask [P] i32, status [Q].
 * ------------------------------------------------------------------------------------------ */
#define MFR_AP_OK            0
#define MFR_AP_APPROXIMATED  1
#define MFR_AP_NO_PAIRS      2
#define MFR_AP_TOO_MANY      3
#define MFR_AP_BAD_OFFSETS   4
#define MFR_AP_ITER_CAP      16   /* bit, mode 0 */
#define MFR_AP_MAX_PAIRS     64
#define MFR_AP_MAX_LO_ITERS  62
#define MFR_AP_WEISZFELD_CAP 256
size_t mfr_abs_pose_workspace_bytes(int P);
int mfr_abs_pose_fuse(const double *train_q, const double *train_c, const double *pred_R, const double *pred_t, int P,
                      const int32_t *offsets, int Q, int mode, double thr_deg, double thr_mult, int lo_iters, uint64_t seed,
                      void *workspace, size_t workspace_bytes,
                      double *abs_q, double *abs_c, int32_t *inlier_mask, int32_t *status, void *stream);
/* test hook: the local optimisation's random subsets as bit masks, out[(q * calls + c) * iters + it] = the nsub (<= 14) members drawn from
 * the set bits of base[q] for (seed, query q, LO call c, iteration it); 0 where base[q] holds fewer than nsub.  Device pointers. */
int mfr_test_abs_pose_subset(uint64_t seed, const uint64_t *base, int n, int calls, int iters, int nsub, uint64_t *out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Essential-matrix path: EssentialMatrixSolver.estimate_pose, lib/models/matching/pose_solver.py:29-61
 *   K-normalise in K's dtype (:39-40) -> thr = pix_thr / mean(fx0, fy1, fy0, fx1) (:43, Q8)
 *   -> cv.findEssentialMat(USAC_MAGSAC, prob) (:46-48): 5-point RANSAC, max_iters (OpenCV default 1000; the reference does
 *      not override it), adaptive iteration cap driven by the number of points under thr, and -- score_method
 *      MFR_EMAT_SCORE_MAGSAC, the method the reference names -- MAGSAC++ model quality (sigma-marginalised loss, 4 degrees of
 *      freedom, k = 3.64, k sigma_max = max_thr_ratio * thr; smallest total loss wins) with sigma-consensus++ local optimisation
 *      (IRLS with the MAGSAC++ weights on (R, unit t): every new best model from iteration 100 on, and the winner at the end).
 *      MFR_EMAT_SCORE_COUNT: inlier count at thr + one LM polish of (R, t) (rounds 1-3; kept for A/B).
 *   -> cv.recoverPose per E (:56-60): 4 decompositions, cheirality vote.
 * magsac_lut: DEVICE copy of the table mfr_magsac_lut (host) fills, 2 * (lut_m + 1) doubles, lut_m <= 2048 (ignored for COUNT).
 * Outputs: R [B,9] (orthonormal to rounding), t [B,3] UNIT translation f64 (NaN on failure), n_inliers [B] = number of
 * cheirality-passing inliers (the `n` recoverPose returns), inlier_mask [B,maxN] u8 = those
 * inliers (what self.mask aliases after the loop, Q7; feed it to mfr_scale_from_depth_batch),
 * status [B].  best_iter / iters_run / counts_out [B,max_iters] / losses_out [B,max_iters] (MAGSAC) / lo_runs [B] (number of
 * local optimisations) are optional diagnostics (NULL ok).
 * ------------------------------------------------------------------------------------------ */
#define MFR_EMAT_SCORE_MAGSAC 0
#define MFR_EMAT_SCORE_COUNT  1
#define MFR_MAGSAC_LUT_M 2048
int mfr_magsac_lut(double *lut_host /* [2 * (M + 1)] */, int M);
size_t mfr_emat_workspace_bytes(int B, int maxN, int max_iters);
int mfr_emat_solve_batch(const float *pts0, const float *pts1, const int32_t *n_corr, int B, int maxN,
                         const void *K0, const void *K1, int k_dtype, double pix_thr, double confidence, int max_iters,
                         uint64_t seed, const int64_t *pair_ids, int score_method, const double *magsac_lut, int lut_m,
                         double max_thr_ratio, void *workspace, size_t workspace_bytes,
                         double *R, double *t, int32_t *n_inliers, int32_t *status, uint8_t *inlier_mask,
                         int32_t *best_iter, int32_t *iters_run, int32_t *counts_out, double *losses_out, int32_t *lo_runs,
                         void *stream);

/* ------------------------------------------------------------------------------------------
 * Rig essential-matrix path (additive; csrc/emat_rig.hip): ONE METRIC pose for a window of T query frames without any depth map,
 * POSE_SOLVER 'RigEssentialMatrix' of the multi-frame model.  The rig's known metric baselines make the scale observable (Clipp et
 * al. 2008).  Upstream has no such solver.  Model, rig rows and row layout as the rig PnP path: (R, t) reference -> LAST window frame;
 * rig [B,T,12] f64; frame j of sample b is row b*T + j of pts0 / pts1 / n_corr / K1 ([B*T,3,3]) and of stage 1's outputs; K0 [B,3,3]
 * belongs to the one reference view of a sample.  1 <= T <= 16.
 *   Stage 1 = mfr_emat_solve_batch over the B*T rows (K0 repeated per row, RANSAC key pair_id*T + j): R1 [B*T,9], t1 [B*T,3] unit,
 *   n_inliers1, status1 [B*T], mask1 [B*T,maxN], device memory.
 *   Stage 2 = mfr_rig_emat_solve, deterministic.  T = 1: stage 1's row passes through bit for bit (unit translation).  Usable frames:
 *   status1 OK; T > 1 and fewer than two -> MFR_ST_NO_MODEL (or the frames' common failure status when none is usable), NaN pose, 0
 *   inliers.  Hypothesis h = 2*pair + {0, 1} over the unordered pairs (j < k) of usable frames in combinations order (rotation of j,
 *   then of k): R_h = R_Am^T R1_m, t_h = least-squares intersection of the two frames' translation directions, u_f x (R_Af t + t_Af) = 0
 *   (3x3 normal equations M t = -c by cofactors).  Skipped (count -1): det M <= 1e-6 (tr M / 3)^3 (directions within ~1e-3 rad of
 *   parallel, e.g. zero baseline), or (R_Af t + t_Af) . u_f <= 0 for either frame.  Score: over ALL frames' correspondences, per frame
 *   E_k = [t_k/|t_k|]x R_k of the composed model (|t_k| < 1e-12: the frame contributes nothing), a point counts when its squared Sampson
 *   distance < thr2_k (the single-frame path's threshold and K-normalisation, per frame, in K's dtype) and cheirality holds; the largest
 *   pooled count wins, the first on a tie; none scored -> MFR_ST_NO_MODEL.  Refine: with >= 6 pooled inliers Levenberg-Marquardt over the
 *   six pose parameters on the signed Sampson residuals (each through its frame's rig row; translation not renormalised; the schedule of
 *   the single-frame COUNT-score polish), then re-score: n_inliers and inlier_mask [B*T,maxN] are that pooled set.  Non-finite pose or
 *   |t| > 1000 -> MFR_ST_DEGENERATE.
 * mfr_rig_emat_solve_batch runs both stages from raw correspondences, no host synchronisation between them (arguments of
 * mfr_emat_solve_batch).  hyp_counts [B, T*(T-1)] (T > 1) and best_hyp [B] (-1: none / T = 1) are optional diagnostics (NULL ok), as
 * is inlier_mask.  Bad arguments (T < 1, T > 16, NULL pointers, workspace too small) return MFR_E_* and launch nothing.
 * ------------------------------------------------------------------------------------------ */
size_t mfr_rig_emat_workspace_bytes(int B, int T, int maxN);
int mfr_rig_emat_solve(const float *pts0, const float *pts1, const int32_t *n_corr, int B, int T, int maxN,
                       const void *K0, const void *K1, int k_dtype, const double *rig, double pix_thr,
                       const double *R1, const double *t1, const int32_t *n_inliers1, const int32_t *status1, const uint8_t *mask1,
                       void *workspace, size_t workspace_bytes,
                       double *R, double *t, int32_t *n_inliers, int32_t *status, uint8_t *inlier_mask /*may be NULL*/,
                       int32_t *hyp_counts, int32_t *best_hyp, void *stream);
size_t mfr_rig_emat_batch_workspace_bytes(int B, int T, int maxN, int max_iters);
int mfr_rig_emat_solve_batch(const float *pts0, const float *pts1, const int32_t *n_corr, int B, int T, int maxN,
                             const void *K0, const void *K1, int k_dtype, const double *rig, double pix_thr, double confidence,
                             int max_iters, uint64_t seed, const int64_t *pair_ids, int score_method, const double *magsac_lut, int lut_m,
                             double max_thr_ratio, void *workspace, size_t workspace_bytes,
                             double *R, double *t, int32_t *n_inliers, int32_t *status, uint8_t *inlier_mask /*may be NULL*/,
                             int32_t *hyp_counts, int32_t *best_hyp, void *stream);

/* ------------------------------------------------------------------------------------------
 * Procrustes path: ProcrustesSolver.estimate_pose, lib/models/matching/pose_solver.py:238-320 with
 * PROCRUSTES.REFINE False (config/matching/mapfree/sg_procrustes_dptkitti.yaml; the optional ICP
 * refinement is mfr_procrustes_icp_refine below).  int-truncate both views (:248-249) -> depth gather (:256-258) -> valid vs each map's
 * minimum (:261, Q6) -> back-project both (:273-274) -> o3d registration_ransac_based_on_correspondence
 * (3-point Kabsch RANSAC, max_corr_dist, confidence 0.999, best = fitness then RMSE, final re-fit)
 * (:286-287) -> inliers = int(fitness * N) (:288).  max_iters caps Open3D's 100000.
 * No model found -> identity pose with 0 inliers and status OK (Open3D's default result), as upstream.
 * ------------------------------------------------------------------------------------------ */
size_t mfr_procrustes_workspace_bytes(int B, int maxN, int max_iters);
int mfr_procrustes_solve_batch(const float *pts0, const float *pts1, const int32_t *n_corr, int B, int maxN,
                               const float *depth0, const float *depth1, int H, int W, const void *K0, const void *K1, int k_dtype,
                               double max_corr_dist, double confidence, int max_iters, uint64_t seed, const int64_t *pair_ids,
                               void *workspace, size_t workspace_bytes, double *R, double *t, int32_t *n_inliers,
                               int32_t *status, int32_t *best_iter, int32_t *iters_run, int32_t *counts_out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Rig Procrustes path (additive; the rig entry point of csrc/procrustes.hip): ONE pose for a window of T query frames from 3-D/3-D
 * correspondences, POSE_SOLVER 'RigProcrustes' of the multi-frame model.  Where the rig PnP path reads the reference view's depth map
 * alone, this one reads all T + 1 maps.  Upstream has no such solver.
 *   Model: (R, t) reference -> LAST window frame, as the rig PnP path; rig [B,T,12] f64 = R_Aj row-major then t_Aj
 *   (A_j: last frame's camera -> frame j's camera; the last row is the identity).
 *   Rows: frame j of sample b is row b*T + j of pts0 / pts1 / n_corr / K1 ([B*T,3,3]) / depth1 ([B*T,H,W]) / n_valid; depth0 [B,H,W]
 *   and K0 [B,3,3] belong to the one reference view of a sample.  1 <= T <= 16.
 *   Lift: as the Procrustes path per frame -- the reference pixel through depth0 / K0, the frame-j pixel through depth1[j] / K1[j], each
 *   map compared against its own minimum (depth0's taken once per sample) -- then Q' = R_Aj^T (Q - t_Aj) carries the query point into
 *   the last frame's camera.  Valid rows are compacted into ONE pooled list in (frame, index) order, N = sum of n_valid[j].
 *   Solve: the Procrustes path's RANSAC on the pooled (P, Q'), the same kernels: hypothesis `it` is the Kabsch fit of
 *   sample_distinct<3>(seed, pair_id, it, N) (the key is pair_id itself: pooled sampling has no frame draw), best = count then squared
 *   error sum, confidence exit, final re-fit.  n_inliers = the pooled count after the re-fit.
 *   Status: all correspondences of a sample count together: fewer than 3 -> MFR_ST_TOO_FEW, fewer than 3 valid -> MFR_ST_BAD_DEPTH
 *   (NaN pose); no model -> the identity pose with 0 inliers and status OK, as the Procrustes path.
 *   With T = 1 and the identity rig every output equals mfr_procrustes_solve_batch bit for bit.
 * inlier_mask [B*T,maxN] u8 over ORIGINAL correspondence indices (the points n_inliers counts), n_valid [B*T], best_iter / iters_run
 * [B], counts_out [B,max_iters] are optional (NULL ok).  Bad arguments (T < 1, T > 16, NULL pointers, workspace too small) return
 * MFR_E_* and launch nothing.
 * ------------------------------------------------------------------------------------------ */
size_t mfr_rig_procrustes_workspace_bytes(int B, int T, int maxN, int max_iters);
int mfr_rig_procrustes_solve_batch(const float *pts0, const float *pts1, const int32_t *n_corr, int B, int T, int maxN,
                                   const float *depth0, const float *depth1, int H, int W,
                                   const void *K0, const void *K1, int k_dtype, const double *rig,
                                   double max_corr_dist, double confidence, int max_iters, uint64_t seed, const int64_t *pair_ids,
                                   void *workspace, size_t workspace_bytes,
                                   double *R, double *t, int32_t *n_inliers, int32_t *status, uint8_t *inlier_mask /*may be NULL*/,
                                   int32_t *n_valid, int32_t *best_iter, int32_t *iters_run, int32_t *counts_out, void *stream);

/* ------------------------------------------------------------------------------------------
 * SuperPoint post-processing.  Reference call site: SuperGlue_matcher.match,
 * etc/feature_matching_baselines/matchers.py:93-120 (hyper-parameters :65-71); the network itself
 * is the un-vendored magicleap submodule (.gitmodules:4-6), restated per SURVEY.md Appendix A.2.
 *   mfr_sp_scoremap            softmax-65, drop dustbin, 8x8 pixel shuffle: logits [B,65,Hc,Wc]
 *                              (NCHW) -> scores [B,8Hc,8Wc]
 *   mfr_sp_nms_candidates      simple_nms(radius 4, 2 rounds) + keypoint threshold + border
 *                              removal; appends survivors to cand [B,cand_cap] (u64 key = score
 *                              bits << 32 | ~raster index) and counts them; nms_out [B,H,W] optional
 *   mfr_sp_select_topk         top-K (K <= 1024) by (score desc, raster index asc); raster order
 *                              when <= K candidates -> kpts [B,K,2] (x,y), kscores [B,K], n_kpts [B]
 *   mfr_sp_sample_descriptors  dense descriptors [B,Hc,Wc,256] (NHWC, un-normalised) -> per-cell L2,
 *                              bilinear grid_sample(align_corners=True), L2 -> desc [B,K,256]
 * ------------------------------------------------------------------------------------------ */
int mfr_sp_scoremap(const float *logits, int B, int Hc, int Wc, float *scores, void *stream);
int mfr_sp_nms_candidates(const float *scores, int B, int H, int W, int nms_radius, float threshold, int border,
                          float *nms_out, uint64_t *cand, int cand_cap, int32_t *cand_count, void *stream);
/*   mfr_sp_nms_candidates_variant  0 = the streaming kernel (a wavefront walks down a strip of an image, no workgroup barrier), 1 = the tile kernel
 *                              (one workgroup per 64 x 32 tile in LDS); the same dense output and the same candidate set, list order arbitrary in both.
 *   mfr_sp_nms_stream_geometry the streaming kernel's useful columns per strip and output rows per segment (for tests on the seams) */
int mfr_sp_nms_candidates_variant(const float *scores, int B, int H, int W, int nms_radius, float threshold, int border,
                                  float *nms_out, uint64_t *cand, int cand_cap, int32_t *cand_count, int variant, void *stream);
int mfr_sp_nms_stream_geometry(int *useful_cols, int *segment_rows);
int mfr_sp_select_topk(const uint64_t *cand, int cand_cap, const int32_t *cand_count, int B, int W, int K,
                       float *kpts, float *kscores, int32_t *n_kpts, void *stream);
int mfr_sp_sample_descriptors(const float *dense_nhwc, int B, int Hc, int Wc, const float *kpts,
                              const int32_t *n_kpts, int K, float *desc, void *stream);
/*   mfr_sp_sample_descriptors_ld  the same with desc rows `ldd` >= 256 floats apart (a multiple of 4): into a wider buffer, e.g. the left half of
 *                              SuperGlue's [x | a] rows; the floats beyond a row's 256 are not touched */
int mfr_sp_sample_descriptors_ld(const float *dense_nhwc, int B, int Hc, int Wc, const float *kpts,
                                 const int32_t *n_kpts, int K, float *desc, int ldd, void *stream);

/* ------------------------------------------------------------------------------------------
 * SuperGlue kernels (same call site; upstream algorithm per SURVEY.md Appendix A.3).
 *   mfr_sg_attention       softmax(q k^T / 8) v, `heads` heads x 64, fp32 in / fp32 out, scores never materialised.
 *                          Both contractions run on the 16-bit matrix cores at fp32 accuracy by operand splitting (csrc/attention.hip).
 *                          mfr_sg_attention_variant: 0 = f16x2 (round 5, what mfr_sg_attention runs; csrc/split_f16.h: every operand as two f16
 *                          terms, main + correction accumulators, three partial products; precondition |q|, |k|, |v| <= 65504),
 *                          2 = bf16x3 (rounds 3-4: exact 3-way bf16 split, six partial products; the same pipelined kernel body as 0, with
 *                          another arithmetic), 1 = the exact-fp32 matrix-core kernel of
 *                          rounds 1-2 (v_mfma_f32_32x32x2_f32), kept for A/B and tests; error vs fp64 of all three = the fp32 class
 *                          (tests/test_gpu_nets_parity.py).  q,k,v [B2,N,ld] (head h = channels
 *                          [64h, 64h+64) from each base pointer), out [B2,N,ldo]; keys/queries
 *                          >= n_tok[image] are masked; cross != 0 -> image b reads K/V of image b^1.
 *   mfr_sg_sinkhorn_match  log_optimal_transport(S, bin_score, iters) without materialising the
 *                          dustbin-augmented matrix + mutual arg-max + exp(score) > match_thr +
 *                          ordered compaction (matchers.py:111-116) into pts0/pts1 [B,maxN,2],
 *                          n_corr [B] -- the layout mfr_pnp_solve_batch consumes.
 *                          S [B,ldS,ldS] = mdesc0^T mdesc1 / 16, n0/n1 [B] true keypoint counts,
 *                          kpts0/kpts1 [B,K,2]; also matches0 [B,ldS] (-1 = none), mscores0 [B,ldS].
 *                          mfr_sg_sinkhorn_match_variant: 0 = one sweep over S per iteration (round 4, default when ldS % 4 == 0 and
 *                          ldS <= 1024), 1 = a row pass and a column pass per iteration (rounds 1-3); the same bits either way.
 *                          Any ldS > 0 with n0, n1 <= ldS <= K.  S needs 4-byte alignment only: an S that is not 16-byte aligned is read
 *                          with 4-byte loads by the two-pass kernels, and every output has the bits an aligned copy gives.
 *                          The scores of the valid n0 x n1 block must be finite.  If a pair's block holds a NaN or +inf, the first
 *                          iteration (iters >= 1) turns its potentials into NaN and no row has an arg-max: that pair returns no matches
 *                          (n_corr 0, matches0 all -1, mscores0 and pts0 / pts1 all zero) and nothing is read out of bounds; the other
 *                          pairs of the launch are unaffected.  (-inf is not a masking value: its result is not defined.)
 * ------------------------------------------------------------------------------------------ */
/*   mfr_gemm_f16x2 / mfr_gemm_bf16x3   the transformers' linear layers, y [M, ldy] (+)= act(x [M, ldx] W [N, K]^T + bias), fp32 in / fp32 out, on
 *                          the 16-bit matrix cores at fp32 accuracy by operand splitting (csrc/gemm_split.hip; rounds 1-2 called the library's fp32
 *                          GEMM here).  f16x2 (round 5, what nets/linear.py runs; csrc/split_f16.h): activations as two f16 terms, the weight
 *                          pre-scaled per output feature and packed as three f16 terms, three partial products, fp32 accumulate;
 *                          precondition |x| <= 65504.  bf16x3 (rounds 3-4): exact 3-way bf16 split of both operands, six partial products.
 *                          W is split and packed once per weight set (mfr_gemm_*_pack, size from mfr_gemm_*_pack_bytes; 0 if K % 32 != 0;
 *                          the two packed formats are not interchangeable).  flags: 1 = ReLU, 2 = accumulate into y (y += x W^T + bias).
 *                          x 16-byte aligned, ldx % 4 == 0; bias may be NULL.  Kernel selection for the bitwise-agreement test (every
 *                          kernel sums each output element in the same order): + 4 one tile per workgroup (round 3), + 8 persistent
 *                          workgroups with register-staged W; none = persistent, W by LDS-DMA (K % 64 == 0; other K run as + 8). */
size_t mfr_gemm_f16x2_pack_bytes(int N, int K);
int mfr_gemm_f16x2_pack(const float *w, int N, int K, void *packed, void *stream);
int mfr_gemm_f16x2(const float *x, int ldx, const void *packed_w, const float *bias, float *y, int ldy, int M, int N, int K, int flags, void *stream);
/*   mfr_gemm_f16x2_batched   nbatch products of one shape in one launch, y_b [M, ldy] = x_b [M, ldx] w_b [N, K]^T * out_mul: the matchers' score /
 *                          similarity matrices (SuperGlue's S = mdesc0 mdesc1^T / 16, models/superglue.py:278-279 of the submodule; LoFTR's
 *                          feat_c0 feat_c1^T / C, coarse_matching.py:104-106), which rounds 1-4 left to the library's batched fp32 GEMM.  The second
 *                          operand of each product is packed per launch into caller scratch (mfr_gemm_f16x2_pack_batched: nbatch blobs of
 *                          mfr_gemm_f16x2_pack_bytes(N, K) each, consecutive; row stride ldw and batch stride in elements), with out_mul -- a power
 *                          of two, so exact -- folded into the per-row scale; batch strides of x and y in elements (x's a multiple of 4). */
int mfr_gemm_f16x2_pack_batched(const float *w, int ldw, int nbatch, long long w_batch_stride, int N, int K, float out_mul, void *packed, void *stream);
int mfr_gemm_f16x2_batched(const float *x, int ldx, long long x_batch_stride, const void *packed_w, const float *bias, float *y, int ldy, long long y_batch_stride,
                           int nbatch, int M, int N, int K, int flags, void *stream);
/*   mfr_conv_igemm_f16x2   implicit-GEMM convolution on NCHW images in the f16x2 arithmetic (csrc/gemm_split.hip): the strided / 1x1 / 7x7
 *                          convolutions of the matcher backbones (LoFTR's conv1, the stride-2 3x3 and 1x1 of layer2.0 / layer3.0, the FPN's 1x1
 *                          lateral and output convolutions; rounds 1-4: MIOpen / hipBLASLt).  y [B,Cout,Ho,Wo] = act(conv(x [B,Cin,H,W], w, stride,
 *                          pad) + bias), Ho = (H + 2 pad - KH) / stride + 1; relu != 0: ReLU; bias may be NULL.  packed_w = mfr_gemm_f16x2_pack of
 *                          the [Cout, K] matrix with K = mfr_conv_igemm_k(Cin, KH, KW) and k = (dy KW + dx) * Cpad + ci, Cpad = Cin rounded up to 32
 *                          (zero columns for ci >= Cin); Cin == 1: k = dy KW + dx, zero columns up to K. */
int mfr_conv_igemm_k(int Cin, int KH, int KW);
int mfr_conv_igemm_f16x2(const float *x, const void *packed_w, const float *bias, float *y, int B, int Cin, int H, int W, int Cout, int KH, int KW,
                         int stride, int pad, int relu, void *stream);
/*   mfr_conv_igemm_f16x2_pad   the same kernel behind an ASYMMETRIC zero padding: pad_lo rows / columns before the image, pad_hi after it (both axes), Ho =
 *                          (H + pad_lo + pad_hi - KH) / stride + 1.  TF-"SAME" padding of DPT-Hybrid's BiT stem (`transformers` WeightStandardizedConv2d with
 *                          padding="same": DynamicPad2d) on even sizes: (2, 3) for the 7x7 / 2 stem, (0, 1) for the 3x3 / 2 bottleneck convolutions.
 *                          pad_lo == pad_hi is mfr_conv_igemm_f16x2 bit for bit. */
int mfr_conv_igemm_f16x2_pad(const float *x, const void *packed_w, const float *bias, float *y, int B, int Cin, int H, int W, int Cout, int KH, int KW,
                             int stride, int pad_lo, int pad_hi, int relu, void *stream);
/*   mfr_conv_igemm_f16x2_upadd (round 6): the same convolution (no activation) + the FPN merge of LoFTR's backbone in one pass,
 *                          y = conv(x) + bias + F.interpolate(lo, scale_factor=2, mode='bilinear', align_corners=True) with lo [B,Cout,Hl,Wl], Ho = 2 Hl,
 *                          Wo = 2 Wl (upstream ResNetFPN_8_2.forward: x2_out = layer2_outconv(x2) + x3_out_2x, x1_out likewise; call site matchers.py:50);
 *                          the up-sampling arithmetic is mfr_upsample2x_add's. */
int mfr_conv_igemm_f16x2_upadd(const float *x, const void *packed_w, const float *bias, const float *lo, int Hl, int Wl, float *y, int B, int Cin, int H, int W,
                               int Cout, int KH, int KW, int stride, int pad, void *stream);
/*   mfr_gemm_f16x2_ln / mfr_gemm_bf16x3_ln (round 6): y = [y +] LayerNorm_N(x W^T + bias) * gamma + beta for N = 128 (one feature block) and K % 64 == 0:
 *                          the linear layer with the LayerNorm that follows it in upstream LoFTREncoderLayer.forward (`message = self.norm1(self.merge(...))`,
 *                          `message = self.norm2(self.mlp(...)); return x + message`; call site matchers.py:50) in ONE launch, for the fine-level encoder
 *                          (d_model 128) whose tensors (2.4 M rows) make every pass HBM-bound.  accumulate != 0: y += (the residual, in place).
 *                          Two-pass statistics (mean, then centred squares), biased variance, rsqrt(var + eps): the arithmetic of mfr_layernorm. */
int mfr_gemm_f16x2_ln(const float *x, int ldx, const void *packed_w, const float *bias, const float *gamma, const float *beta, float eps, float *y, int ldy,
                      int M, int N, int K, int accumulate, void *stream);
int mfr_gemm_bf16x3_ln(const float *x, int ldx, const void *packed_w, const float *bias, const float *gamma, const float *beta, float eps, float *y, int ldy,
                       int M, int N, int K, int accumulate, void *stream);
/*   mfr_gemm_f16x2_windows / mfr_gemm_bf16x3_windows (round 6): upstream FinePreprocess.forward (F.unfold(feat_f, 5x5, stride 4, padding 2) -> rows at the
 *                          matches -> merge_feat; call site matchers.py:50) as ONE product: y [nwin win^2, N] = window tokens W^T (+ bias) (+ window_bias
 *                          [nwin, N] broadcast over a window's tokens), the tokens read from the NHWC fine map feat [Bimg,Hf,Wf,C] in place: window w =
 *                          the win x win pixels around cell cell_ids[w] (centre ((cell / wc) stride, (cell % wc) stride)) of image img_ids[w], zero
 *                          outside the map (zero_row: C zeros the caller provides).  C = K a multiple of 64.  Replaces mfr_loftr_gather_windows + the
 *                          window tensor + mfr_gemm_* + a broadcast add. */
int mfr_gemm_f16x2_windows(const float *feat, int Bimg, int Hf, int Wf, int C, const int32_t *img_ids, const int32_t *cell_ids, int nwin, int wc, int stride, int win,
                           const float *zero_row, const void *packed_w, const float *bias, const float *window_bias, float *y, int ldy, int N, void *stream);
int mfr_gemm_bf16x3_windows(const float *feat, int Bimg, int Hf, int Wf, int C, const int32_t *img_ids, const int32_t *cell_ids, int nwin, int wc, int stride, int win,
                            const float *zero_row, const void *packed_w, const float *bias, const float *window_bias, float *y, int ldy, int N, void *stream);
/*   mfr_mlp_ln_f16x2 / mfr_mlp_ln_bf16x3 (round 6): y = [y +] LayerNorm_128( relu(x W1^T + b1) W2^T + b2 ) * gamma + beta in ONE launch: the MLP + norm2 +
 *                          residual of upstream LoFTREncoderLayer.forward at d_model 128 (`message = self.mlp(cat[x, message])`, `self.norm2`, `x + message`;
 *                          call site matchers.py:50).  x [M, K1] (K1 % 64 == 0; the fine level: 256 = [x | message]); W1 [256, K1] and W2 [128, 256] packed by
 *                          mfr_gemm_*_pack; the 256 hidden activations of a 128-row tile never leave the chip.  accumulate != 0: y += (in place residual). */
int mfr_mlp_ln_f16x2(const float *x, int ldx, int K1, const void *packed_w1, const float *b1, const void *packed_w2, const float *b2, const float *gamma, const float *beta,
                     float eps, float *y, int ldy, int M, int accumulate, void *stream);
int mfr_mlp_ln_bf16x3(const float *x, int ldx, int K1, const void *packed_w1, const float *b1, const void *packed_w2, const float *b2, const float *gamma, const float *beta,
                      float eps, float *y, int ldy, int M, int accumulate, void *stream);
size_t mfr_gemm_bf16x3_pack_bytes(int N, int K);
int mfr_gemm_bf16x3_pack(const float *w, int N, int K, void *packed, void *stream);
int mfr_gemm_bf16x3(const float *x, int ldx, const void *packed_w, const float *bias, float *y, int ldy, int M, int N, int K, int flags, void *stream);
int mfr_sg_attention(const float *q, const float *k, const float *v, int ld, int B2, int N, int heads,
                     const int32_t *n_tok, int cross, float *out, int ldo, void *stream);
int mfr_sg_attention_variant(const float *q, const float *k, const float *v, int ld, int B2, int N, int heads,
                             const int32_t *n_tok, int cross, float *out, int ldo, int variant, void *stream);
size_t mfr_sg_match_workspace_bytes(int B, int ldS);
int mfr_sg_sinkhorn_match(const float *S, int B, int ldS, const int32_t *n0, const int32_t *n1,
                          float bin_score, int iters, float match_thr,
                          const float *kpts0, const float *kpts1, int K,
                          void *workspace, size_t workspace_bytes,
                          int32_t *matches0, float *mscores0, float *pts0, float *pts1, int maxN, int32_t *n_corr,
                          void *stream);
int mfr_sg_sinkhorn_match_variant(const float *S, int B, int ldS, const int32_t *n0, const int32_t *n1,
                                  float bin_score, int iters, float match_thr,
                                  const float *kpts0, const float *kpts1, int K,
                                  void *workspace, size_t workspace_bytes,
                                  int32_t *matches0, float *mscores0, float *pts0, float *pts1, int maxN, int32_t *n_corr,
                                  int variant, void *stream);
/*   mfr_sg_sinkhorn_match_strided  the same, reading the matcher's interleaved [2B] tensors in place: `n_stride` elements between two pairs' counts
 *                          in n0 / n1, `kpts_stride` floats between two pairs' [K, 2] keypoints in kpts0 / kpts1 (contiguous: 1 and 2 K).  Like the
 *                          entry points above it writes zeros to the rows >= n_corr of pts0 / pts1, so the caller need not clear them. */
int mfr_sg_sinkhorn_match_strided(const float *S, int B, int ldS, const int32_t *n0, const int32_t *n1, long long n_stride,
                                  float bin_score, int iters, float match_thr,
                                  const float *kpts0, const float *kpts1, int K, long long kpts_stride,
                                  void *workspace, size_t workspace_bytes,
                                  int32_t *matches0, float *mscores0, float *pts0, float *pts1, int maxN, int32_t *n_corr,
                                  int variant, void *stream);
/*   mfr_sg_kenc_in         SuperGlue's keypoint-encoder input in one launch: kn = (kpts - (W, H) / 2) * fp32(1 / (0.7 max(W, H))) and layer 0 (w [32, 3], BatchNorm
 *                          folded), h = relu((kn_x w0 + kn_y w1) + (score w2 + b)), every operation rounded on its own; kpts [rows, 2], scores [rows] ->
 *                          out [rows, 32] (csrc/elementwise.hip) */
int mfr_sg_kenc_in(const float *kpts, const float *scores, const float *w, const float *bias, long long rows, int H, int W, float *out, void *stream);

/* ------------------------------------------------------------------------------------------
 * LightGlue kernels (csrc/lightglue.hip): the SuperPoint matcher of LightGlue (ICCV 2023) without adaptive depth / width.  The reference has
 * no LightGlue call site; the stage takes SuperGlue_matcher's place (etc/feature_matching_baselines/matchers.py:62-120) and the network is
 * restated from the paper with the parameter names of the `transformers` LightGlue module.  Linear layers: mfr_gemm_*; attention:
 * mfr_sg_attention (scale 1/8, cross = 1 for the flipped pair); similarity S: mfr_gemm_f16x2_batched under SPLIT f16x2, the framework's batched fp32
 * product (torch.bmm) under bf16x3, as for SuperGlue's scores.  All fp32, kernels only, bit-reproducible.
 *   mfr_lg_rotary_table   cs [M, 64] = (cos | sin)(Wr p) for M normalised keypoints p [M, 2] and the projector Wr [32, 2]: once per batch
 *   mfr_lg_rotary_apply   q, k [M, 256] (row stride ld, 4 heads x 64) rotated in place: (x_2i, x_2i+1) <- (x_2i c_i - x_2i+1 s_i, x_2i+1 c_i + x_2i s_i),
 *                         the same 32 angles for every head (the interleaved pairing; NOT the half-split convention)
 *   mfr_lg_ln_gelu        x [M, 512] (row stride ld) <- GELU_erf(LayerNorm_512(x) * gamma + beta) in place: the MLP's hidden row between fc1 and fc2 as a
 *                         pass of its own (the A/B partner of mfr_gemm_*_ln_gelu, which does it in fc1's epilogue)
 *   mfr_lg_assign         double softmax + matchability + match extraction on S [B, N0, ldS] (ldS >= N1), z0 [B, N0], z1 [B, N1], counts n0, n1 [B]:
 *                         score_ij = 2 S_ij - lse_j S_i. - lse_i S_.j + logsigmoid(z0_i) + logsigmoid(z1_j) over the valid n0 x n1 block (never
 *                         written; S is swept twice); matches0 [B, N0] / matches1 [B, N1] i32 (-1 = none): the mutual arg-max (lowest index on a
 *                         tie) whose exp(score) > threshold; mscores0 / mscores1: exp(score) at the mutual arg-max, 0 elsewhere.  n0 == 0 or
 *                         n1 == 0: all -1 / 0, S is not read.  Optional (all NULL or none): kpts0, kpts1 [B, K, 2] -> pts0, pts1 [B, maxN, 2], the
 *                         matched keypoints in ascending i, and n_corr [B] (the layout of mfr_sg_sinkhorn_match).
 * ------------------------------------------------------------------------------------------ */
/*   mfr_gemm_f16x2_ln_gelu / mfr_gemm_bf16x3_ln_gelu (csrc/gemm_split.hip): y = GELU_erf(LayerNorm_512(x W^T + bias) * gamma + beta) for N = 512 in ONE launch: fc1 of
 *                         LightGlue's MLP with the LayerNorm and the GELU in the epilogue.  A workgroup keeps the four 128-feature accumulator blocks of a
 *                         128-row tile on chip, so the pre-norm hidden row is never written; W packed by mfr_gemm_*_pack, K % 32 == 0.  Two-pass statistics,
 *                         biased variance, rsqrt(var + eps): the arithmetic of mfr_layernorm.  f16x2: the range guard tests the accumulators. */
int mfr_gemm_f16x2_ln_gelu(const float *x, int ldx, const void *packed_w, const float *bias, const float *gamma, const float *beta, float eps, float *y, int ldy,
                           int M, int N, int K, void *stream);
int mfr_gemm_bf16x3_ln_gelu(const float *x, int ldx, const void *packed_w, const float *bias, const float *gamma, const float *beta, float eps, float *y, int ldy,
                            int M, int N, int K, void *stream);
int mfr_lg_rotary_table(const float *kpts_norm, const float *wr, int M, float *cs, void *stream);
int mfr_lg_rotary_apply(float *q, float *k, int ld, int M, const float *cs, void *stream);
int mfr_lg_ln_gelu(float *x, int ld, int M, const float *gamma, const float *beta, float eps, void *stream);
size_t mfr_lg_assign_workspace_bytes(int B, int N0, int N1);
int mfr_lg_assign(const float *S, int B, int N0, int N1, int ldS, const float *z0, const float *z1, const int32_t *n0, const int32_t *n1,
                  float threshold, const float *kpts0, const float *kpts1, int K, void *workspace, size_t workspace_bytes,
                  int32_t *matches0, int32_t *matches1, float *mscores0, float *mscores1, float *pts0, float *pts1, int maxN, int32_t *n_corr,
                  void *stream);

/* ------------------------------------------------------------------------------------------
 * LoFTR kernels.  Reference call site: LoFTR_matcher.match, etc/feature_matching_baselines/
 * matchers.py:24-59 (LoFTR(default_cfg), *_ot.ckpt strict=False :16-18); network = un-vendored
 * zju3dv/LoFTR submodule (.gitmodules:1-3), restated per SURVEY.md Appendix A.4.
 *   mfr_loftr_linear_attention   LinearAttention of the coarse transformer (heads x 32, elu+1 feature
 *                                map, eps 1e-6): out = phi(Q) (phi(K)^T V/L) / (phi(Q).sum phi(K)) * L.
 *                                q [B,L,ldq], k,v [B,L,ld], out [B,L,ldo]; head h = channels [32h,32h+32)
 *   mfr_loftr_fine_attention     the same LinearAttention for the fine transformer: d_model 128 (8 heads x 16), L = 25
 *                                tokens per 5x5 window, Bw windows; one wavefront per window, no workspace.
 *                                q [Bw,25,ldq], k,v [Bw,25,ld], out [Bw,25,ldo]; L, D, heads must be 25, 128, 8
 *   mfr_loftr_coarse_match       CoarseMatching(dual_softmax) + get_coarse_match: S [B,L0,L1] =
 *                                (f0/sqrt C)(f1/sqrt C)^T; conf = softmax_i(S/T) * softmax_j(S/T);
 *                                conf > thr, border removal, mutual max -> i_ids, j_ids [B,L0] i32
 *                                (ascending i), mconf [B,L0], n_match [B]
 *   mfr_loftr_ot_match           CoarseMatching(sinkhorn) + get_coarse_match, the matcher the `*_ot.ckpt` weights of matchers.py:16-18
 *                                were trained with (upstream src/loftr/utils/coarse_matching.py, MATCH_TYPE 'sinkhorn', SKH_ITERS 3):
 *                                log-domain Sinkhorn on [[S, a], [a, a]] (a = coarse_matching.bin_score), conf = exp(Z)[:m, :n];
 *                                same outputs as mfr_loftr_coarse_match
 *   mfr_loftr_gather_windows     FinePreprocess unfold(win, stride, pad win/2) restricted to the
 *                                matched cells: feat [Bimg,Hf,Wf,C] NHWC -> out [M, win*win, C]
 *   mfr_loftr_fine_match         FineMatching: centre-feature correlation, softmax, spatial expectation,
 *                                sub-pixel update of the view-1 keypoints
 * ------------------------------------------------------------------------------------------ */
size_t mfr_loftr_linear_attention_workspace_bytes(int B, int L, int heads);
int mfr_loftr_linear_attention(const float *q, int ldq, const float *k, const float *v, int ld, int B, int L, int heads,
                               void *workspace, size_t workspace_bytes, float *out, int ldo, void *stream);
int mfr_loftr_fine_attention(const float *q, int ldq, const float *k, const float *v, int ld, int Bw, int L, int D, int heads,
                             float *out, int ldo, void *stream);
size_t mfr_loftr_coarse_match_workspace_bytes(int B, int L0, int L1);
int mfr_loftr_coarse_match(const float *S, int B, int h0, int w0, int h1, int w1, float temperature, float thr, int border,
                           void *workspace, size_t workspace_bytes, int32_t *i_ids, int32_t *j_ids, float *mconf,
                           int32_t *n_match, void *stream);
/* variant 0 (what mfr_loftr_coarse_match runs): S is swept twice (tiled kernels produce row AND column quantities in the same
 * sweep); variant 1: the four-sweep row / column kernels of round 1.  Same arithmetic per element; the partial logsumexps are
 * folded in a different (fixed) order. */
int mfr_loftr_coarse_match_variant(const float *S, int B, int h0, int w0, int h1, int w1, float temperature, float thr, int border,
                                   void *workspace, size_t workspace_bytes, int32_t *i_ids, int32_t *j_ids, float *mconf,
                                   int32_t *n_match, int variant, void *stream);
/* Optimal-transport coarse matching.  S [B, h0*w0, h1*w1] as for mfr_loftr_coarse_match (no temperature), read-only; the dustbin row / column
 * (the constant bin_score) are never materialised.  iters >= 1 Sinkhorn iterations (upstream 3).  variant 0: iters + 1 sweeps over S (per
 * iteration one sweep forms u_i from a complete row and adds S_ij + u_i to per-column partial logsumexps, folded in a fixed order; rows of up to
 * 8192 columns, longer rows run variant 1's kernels); variant 1: a row and a column kernel per iteration (2 iters + 1 sweeps; A/B, cross-check).
 * Both are bit-reproducible (no float atomics).  u_out [B, h0*w0 + 1] / v_out [B, h1*w1 + 1]: the final potentials incl. the dustbin entry
 * (log assignment = S_ij + u_i + v_j + log(m + n)), each may be NULL.  i_ids / j_ids / mconf [B, h0*w0], n_match [B]: ascending i, lowest j on a
 * tie, entries at index >= n_match unspecified. */
size_t mfr_loftr_ot_match_workspace_bytes(int B, int L0, int L1);
int mfr_loftr_ot_match(const float *S, int B, int h0, int w0, int h1, int w1, float bin_score, int iters, float thr, int border,
                       void *workspace, size_t workspace_bytes, int32_t *i_ids, int32_t *j_ids, float *mconf, int32_t *n_match,
                       float *u_out, float *v_out, int variant, void *stream);
int mfr_loftr_gather_windows(const float *feat, int Bimg, int Hf, int Wf, int C, const int32_t *img_ids,
                             const int32_t *cell_ids, int M, int wc, int stride, int win, float *out, void *stream);
/* FineMatching (the last step of LoFTR_matcher.match, matchers.py:50-55 -> mkpts1_f): per matched window, similarity of view 0's centre
 * feature against the W*W fine features of view 1 (/ sqrt C), softmax, spatial expectation over linspace(-1, 1, W)^2, and
 * pts1[lin_idx[m]] = k1[lin_idx[m]] + expectation * out_scale (out_scale = (W / 2) * image-to-fine-map scale).
 * g0, g1 [M, W*W, ld] f32 (first C columns), lin_idx [M] i32 slots into the [B * L0, 2] tensors k1 / pts1; expec [M, 2] optional
 * (the normalised expectation; pts1 / lin_idx / k1 may be NULL when only expec is wanted).  W*W <= 64. */
int mfr_loftr_fine_match(const float *g0, const float *g1, int ld, int C, int M, int W, float out_scale, const int32_t *lin_idx,
                         const float *k1, float *pts1, float *expec, void *stream);

/* ------------------------------------------------------------------------------------------
 * Fused conv epilogues of the SuperPoint encoder (NCHW f32; same call site as above): the MIOpen
 * convolutions run without bias and these finish the layer in one pass.
 *   mfr_bias_relu_nchw        x <- relu(x + bias[c]) in place, x [B,C,HW]
 *   mfr_bias_pool2_relu_nchw  y = relu(max_pool2x2(x) + bias[c]), x [B,C,H,W] -> y [B,C,H/2,W/2]
 * Bit-identical to conv -> +bias -> ReLU -> max_pool2d(2,2) (monotone rounding).
 *   mfr_conv3x3_c1_relu       SuperPoint conv1a fused: y = relu(conv3x3(x [B,1,H,W], w [64,1,3,3], pad 1) + bias),
 *                             y [B,64,H,W]; W % 4 == 0 (HBM-write-bound first layer, one pass)
 */
int mfr_conv3x3_c1_relu(const float *x, const float *w, const float *bias, int B, int H, int W, int out_channels,
                        float *y, void *stream);
int mfr_bias_relu_nchw(float *x, const float *bias, int B, int C, int HW, void *stream);
/* 1x1 convolution with few output channels (SuperPoint's detector head convPb 256 -> 65, same call site): y [B,Cout,HW] = w [Cout,Cin] x [B,Cin,HW]
 * + bias, one ascending fused-multiply-add chain per output: a pixel's result does not depend on the batch size.  Cin <= 512. */
int mfr_conv1x1_nchw(const float *x, const float *w, const float *bias, int B, int Cin, int Cout, int HW, float *y, void *stream);
/*   mfr_nchw_to_rows       x [B, C, HW] (+ add [C, HW], may be NULL) -> out[img'][p][c] with row stride ldo and image stride out_img_stride
 *                          (floats): the token-major operand of the linear layers, written in place of torch's permute().contiguous();
 *                          deinterleave != 0: image 2 k + s of a pair-interleaved batch goes to slot s * (B / 2) + k. */
int mfr_nchw_to_rows(const float *x, const float *add, int B, int C, int HW, int deinterleave, float *out, long long out_img_stride, int ldo, void *stream);
/*   mfr_nchw_to_rows_gather  the same transposition with the source image of every output slot taken from a table: out[j][p][c] = x[idx[j]][c][p]
 *                          (+ add[c][p]), j < n_out, x [n_src, C, HW].  `idx` is a HOST array; it travels to the device as a kernel argument (64 slots per
 *                          launch, more slots = more launches), so the call adds no copy and no synchronisation.  Every index must lie in [0, n_src):
 *                          otherwise MFR_E_ARG and nothing is launched.  (LoFTR's side-major token buffer filled from cached reference views.) */
int mfr_nchw_to_rows_gather(const float *x, const float *add, int n_src, int C, int HW, const int32_t *idx, int n_out, float *out, long long out_img_stride,
                            int ldo, void *stream);
int mfr_bias_pool2_relu_nchw(const float *x, const float *bias, int B, int C, int H, int W, float *y, void *stream);

/* ------------------------------------------------------------------------------------------
 * ProcrustesSolver's optional whole-cloud ICP refinement (PROCRUSTES.REFINE, lib/models/matching/pose_solver.py:290-319;
 * config/matching/scannet/ *_icp.yaml): o3d registration_icp(point-to-point, max distance, init = RANSAC transform,
 * ICPConvergenceCriteria(rel_fitness, rel_rmse, max_iter)) restated (csrc/procrustes_icp.hip); R, t are in/out, pairs whose
 * `status` (may be NULL) is not MFR_ST_OK are left untouched with 0 inliers; n_inliers = int(fitness * |target cloud|) (:319).
 */
size_t mfr_procrustes_icp_workspace_bytes(int B, int H, int W);
int mfr_procrustes_icp_refine(const float *depth0, const float *depth1, int B, int H, int W, const void *K0, const void *K1, int k_dtype,
                              double max_corr_dist, double rel_fitness, double rel_rmse, int max_iter, const int32_t *status,
                              void *workspace, size_t workspace_bytes, double *R, double *t, int32_t *n_inliers, double *fitness,
                              double *rmse, int32_t *iters, void *stream);

/* ------------------------------------------------------------------------------------------
 * LoFTR transformer / FPN glue, fused (csrc/loftr_fused.hip).  Reference call site: LoFTR_matcher.match
 * (etc/feature_matching_baselines/matchers.py:24-59) -> upstream LoFTREncoderLayer / ResNetFPN_8_2 (un-vendored).
 *   mfr_layernorm       torch.nn.LayerNorm(C) over rows of x (row stride ldx floats), C in {128, 256}, + optional residual
 *                       (row stride ldr; may alias out): out[r] = residual[r] + (x[r] - mean) * rstd * gamma + beta, row stride
 *                       ldo.  Strides let norm1 write into the right half of the MLP's [x | message] operand (no cat) and
 *                       norm2 + residual update x in place.  All pointers 16-byte aligned, strides multiples of 4.
 *   mfr_upsample2x_add  y [planes,2H,2W] += F.interpolate(lo [planes,H,W], scale_factor=2, bilinear, align_corners=True)
 */
int mfr_layernorm(const float *x, int ldx, const float *gamma, const float *beta, const float *residual, int ldr, long long rows, int C,
                  float eps, float *out, int ldo, void *stream);
int mfr_upsample2x_add(const float *lo, float *y, int planes, int H, int W, void *stream);
/*   mfr_upsample_bilinear  out [planes,Ho,Wo] = F.interpolate(in [planes,H,W], size=(Ho,Wo), bilinear, align_corners=True) with
 *                       torch's arithmetic; dtype 0 = float32, 1 = bfloat16 storage (f32 arithmetic).  Reference call site: the
 *                       regression encoder's `upconv` (lib/models/regression/encoder/resunet.py:30-38, used at :121-126). */
int mfr_upsample_bilinear(const void *in, void *out, int planes, int H, int W, int Ho, int Wo, int dtype, void *stream);
/*   mfr_conv_gemm_bf16    the 3x3 decoder convolutions of the regression encoder (`conv` inside upconv4 / iconv4 / upconv3 / iconv3,
 *                       lib/models/regression/encoder/resunet.py:16-38, 112-128; bf16 autocast of train.py:20-70) as implicit GEMMs on
 *                       the bf16 matrix cores (csrc/conv_gemm_bf16.hip): forward, d/d input and d/d weight are ONE kernel,
 *                           C[i, j] = sum_k A[i, k] B[j, k]      bf16 operands, fp32 accumulate,
 *                       whose k axis is cut into segments of Lk elements (Lk % 32 == 0); chunk c of 32 elements, in segment s = 32 c / Lk,
 *                       is read at A + zA[z] + i * sA + segA[s] + (32 c mod Lk) and at B + zB[z] + j * sB + segB[s] + (32 c mod Lk)
 *                       (all offsets and strides in ELEMENTS, multiples of 8; segA / segB hold one entry MORE than there are segments).
 *                       Slice z of the grid works on chunks [zk[z], min(zk[z] + nkc_z, nkc_total)) and writes C + zC[z] (element
 *                       offset), row stride ldc; out_dtype 0 = float32, 1 = bfloat16 (round to nearest even); bias [N] f32 (added
 *                       before rounding) or NULL; zA / zB / zC / zk may be NULL (= 0).  Rows i >= M / j >= N of a tile are neither read
 *                       nor written.  How a convolution maps onto it: map-free-reloc_amd/regression/conv_bf16.py. */
int mfr_conv_gemm_bf16(const void *A, long long sA, const long long *segA, const void *B, long long sB, const long long *segB,
                       int Lk, int nkc_total, int nkc_z, const float *bias, void *C, long long ldc, int out_dtype,
                       int M, int N, int nz, const long long *zA, const long long *zB, const long long *zC, const int *zk, void *stream);
/*   operand images of those products (memory-bound, every element written incl. the zero halo; x_dtype 0 = float32, 1 = bfloat16):
 *   mfr_conv_pack_nhwc_halo  x [B,C,H,W] -> out = guard_rows * C zeros | [B, H+2, Wp, C] bf16 | guard_rows * C zeros   (C % 8 == 0); Wp = W+2: a
 *                            zero column on either side of a row; Wp = W+1: one zero column in front of every row, shared with the row before
 *   mfr_conv_pack_cm_halo    x [BC,H,W] -> ncopies images, each  slack zeros | [BC][L] bf16 | slack zeros,  rows of Wq >= W+2 positions
 *                            (Wq % 8 == 0, L >= (H+2) Wq, L % 8 == 0, slack % 8 == 0); copy k holds the haloed image shifted by
 *                            first_shift + k positions along its rows (the kx tap shift of the d/d weight product) */
int mfr_conv_pack_nhwc_halo(const void *x, int x_dtype, int B, int C, int H, int W, int Wp, void *out, int guard_rows, void *stream);
int mfr_conv_pack_cm_halo(const void *x, int x_dtype, long long BC, int H, int W, int Wq, long long L, int ncopies, int first_shift, long long slack,
                          void *out, void *stream);
/*   mfr_conv_unpack_nchw    haloed NHWC result [B, H+2, Wp, N] bf16 (what the forward / d input product writes) -> y [B, N, H, W] bf16 */
int mfr_conv_unpack_nchw(const void *haloed, int B, int N, int H, int W, int Wp, void *y, void *stream);

/* ------------------------------------------------------------------------------------------
 * Differentiable batched Kabsch rotation of the regression heads (csrc/kabsch.hip, csrc/kabsch_math.h).  Reference: `procrustes`,
 * lib/utils/solver.py:4-37 (torch.svd + reflection fix), called from lib/models/regression/head.py:55-163.  No host
 * synchronisation (torch.linalg.svd reads the solver's status back), so the training step can be captured as a HIP graph.
 *   mfr_kabsch_fwd   H [B,3,3] = A_c^T B_c -> R [B,3,3], the proper rotation with B_c ~ A_c R^T (Horn quaternion + Jacobi)
 *   mfr_kabsch_bwd   gR = dL/dR -> gH = dL/dH (closed form through the polar factor, see kabsch.hip)
 * ------------------------------------------------------------------------------------------ */
int mfr_kabsch_fwd(const float *H, int B, float *R, void *stream);
int mfr_kabsch_bwd(const float *H, const float *gR, int B, float *gH, void *stream);

/* ------------------------------------------------------------------------------------------
 * SIFT-descriptor correspondence leg.  Reference call sites:
 * SIFTMatching.get_correspondences (lib/models/matching/feature_matching.py:75-118) and
 * SIFT_matcher.match (etc/feature_matching_baselines/matchers.py:135-188), everything AFTER
 * cv.SIFT.detectAndCompute (keypoint detection/description stays with the caller):
 *   mfr_rootsift          root_sift (feature_matching.py:68-74): out = sqrt(desc / (rowsum + 1e-7f)),
 *                         desc/out [n_rows,128] f32 (out may alias desc), norm2 [n_rows] = |out row|^2.
 *                         Bit-identical to the reference's numpy (same summation order).
 *   mfr_desc_ratio_match  replaces cv.FlannBasedMatcher(kd-tree).knnMatch(des0, des1, k=2) + Lowe's
 *                         ratio loop (:86-101): EXACT 2-NN (squared L2, ties -> lower train index) of
 *                         every query row, then keep i where sqrt(d1) < ratio * sqrt(d2) (binary64
 *                         compare, as the Python loop does), in query order.
 *                         des0 [B,N0,128], des1 [B,N1,128] (rootSIFT), norm0 [B,N0], norm1 [B,N1],
 *                         kp0 [B,N0,2], kp1 [B,N1,2] pixel (x,y); n0,n1 [B] valid rows per pair.
 *                         Out: nn_idx [B,N0] i32, nn_d2 [B,N0,2] f32 (best, second), pts0/pts1
 *                         [B,maxN,2] + n_corr [B] in the layout the solver entry points take.
 *                         Pairs with n1 < 2 yield no correspondences.
 * ------------------------------------------------------------------------------------------ */
int mfr_rootsift(const float *desc, int n_rows, float *out, float *norm2, void *stream);
int mfr_desc_ratio_match(const float *des0, const float *des1, const float *norm0, const float *norm1,
                         const float *kp0, const float *kp1, int B, int N0, int N1,
                         const int32_t *n0, const int32_t *n1, double ratio,
                         int32_t *nn_idx, float *nn_d2, float *pts0, float *pts1, int maxN, int32_t *n_corr,
                         void *stream);

/* ------------------------------------------------------------------------------------------
 * SIFT keypoint detection + description (csrc/sift.hip): OpenCV 4.8 SIFT_create(nfeatures) with default parameters
 * (3 layers, contrast 0.04, edge 10, sigma 1.6, doubled input), restated step by step in sift_ops.py's docstring.
 * Reference call sites: SIFT_create(cfg.SIFT.NUM_FEATURES).detectAndCompute (lib/models/matching/feature_matching.py:58,82-83)
 * and SIFT_create(2048) (etc/feature_matching_baselines/matchers.py:146-147).  Added to ABI v6 without a version bump
 * (purely additive).
 *   mfr_sift_workspace_bytes  workspace of mfr_sift_detect for B images of H x W (H, W >= 8) and a candidate capacity
 *                             (<= 0: the default, 16384 refined extrema per image); 0 for unsupported arguments
 *   mfr_sift_level_offset     byte offset of Gaussian level `level` (0..5) of octave `octave` inside that workspace (the
 *                             level is [B, Ho, Wo] f32, sizes written to *_host); -1 when the level does not exist
 *   mfr_sift_blur_taps        host: the f32 taps c[0..16] (c[0] centre, c[i] at distance i) and radius of the blur that
 *                             produces level `level` (level 0: the blur of the doubled base image)
 *   mfr_sift_detect           gray [B,H,W] u8 -> per image the keypoints OpenCV's detectAndCompute keeps, in ascending
 *                             (x, y, size desc, angle, response desc, octave desc) order: kpts [B,Nmax,2] (x, y) in
 *                             input pixels, desc [B,Nmax,128] (whole numbers 0..255 as f32), size/angle/response
 *                             [B,Nmax] f32, octave [B,Nmax] i32 (OpenCV's packed word), n [B] rows written (rows >= n
 *                             are not touched), status [B] bit set (0 = complete):
 */
#define MFR_SIFT_ST_CAND_OVERFLOW 1   /* more refined extrema than the candidate capacity: the excess was dropped */
#define MFR_SIFT_ST_KPT_OVERFLOW  2   /* more oriented keypoints than 16384 before selection: the excess was dropped */
#define MFR_SIFT_ST_OUT_OVERFLOW  4   /* the selected set (ties included) has more than Nmax rows: n = Nmax */
size_t mfr_sift_workspace_bytes(int B, int H, int W, int cand_cap);
long long mfr_sift_level_offset(int B, int H, int W, int octave, int level, int *Ho_host, int *Wo_host);
int mfr_sift_blur_taps(int level, float *taps_host, int *radius_host);
int mfr_sift_detect(const uint8_t *gray, int B, int H, int W, int nfeatures, int Nmax, int cand_cap, void *workspace,
                    size_t workspace_bytes, float *kpts, float *desc, float *size, float *angle, float *response,
                    int32_t *octave, int32_t *n, int32_t *status, void *stream);

/* ------------------------------------------------------------------------------------------
 * Baseline JPEG decode (csrc/jpeg.hip): sequential, Huffman-coded, 8-bit files -> the loaders' gray plane, bit for bit
 * datasets.read_gray_plane(path, None) (PIL's RGB decode: libjpeg-turbo JDCT_ISLOW + fancy upsampling, then luma_u8, / 255f).
 * Call site: the batched loaders of predict_fused with HIP.JPEG_DECODE 'device' (datasets.PairBatchLoader / DevicePrefetcher,
 * jpeg_ops.JpegDecoder).  The host half is csrc/host_decode.c mfr_host_jpeg_parse (libmfr_host.so), which writes one
 * mfr_jpeg_header and one record per file (include/mfr_jpeg.h).  Added to ABI v6 without a version bump (purely additive).
 *   mfr_jpeg_workspace_bytes  workspace of mfr_jpeg_decode for n images of H x W whose records are at most max_record_bytes,
 *                             at subsequence length subseq_bits (0 = the default); 0 for unsupported arguments
 *   mfr_jpeg_decode           headers [n] (device), records (device, offsets [n+1] i64 bytes, each a multiple of 16) ->
 *                             gray [n,1,H,W] f32 (may be NULL when rgb is given), rgb [n,H,W,3] u8 (may be NULL), status [n] (0 ok; a parse code of the
 *                             header passed through, its image untouched; MFR_JPEG_E_* bits from the device: that image's
 *                             planes are undefined), rounds [n] (may be NULL: the entropy stage's fixed-point rounds, a debug
 *                             counter).  subseq_bits: test-only subsequence length in bits (0 = default, >= 16 otherwise).
 */
size_t mfr_jpeg_workspace_bytes(int n, int H, int W, long long max_record_bytes, int subseq_bits);
int mfr_jpeg_decode(const void *headers, const uint8_t *records, const long long *offsets, int n, int H, int W,
                    long long max_record_bytes, float *gray, uint8_t *rgb, int32_t *status, int32_t *rounds, void *workspace,
                    size_t workspace_bytes, int subseq_bits, void *stream);

/* ------------------------------------------------------------------------------------------
 * 16-bit gray (millimetre depth) PNG decode (csrc/png.hip): non-interlaced colour type 0 / bit depth 16 files -> the loaders'
 * depth plane, bit for bit datasets.read_depth_plane(path): float32(uint16 / 1000.0).  Call site: the batched loaders of
 * predict_fused with HIP.DEPTH_DECODE 'device' (datasets.PairBatchLoader / DevicePrefetcher, png_ops.DepthPngDecoder).  The host
 * half is csrc/host_decode.c mfr_host_png_parse (libmfr_host.so), which writes one mfr_png_header and one record (the joined IDAT
 * payloads) per file (include/mfr_png.h).  Added to ABI v6 without a version bump (purely additive).
 *   mfr_png_depth_workspace_bytes  scratch of mfr_png_depth_decode for n images of H x W (the filtered scanlines, H (1 + 2 W) bytes
 *                                per image, 256-aligned); 0 for unsupported arguments (H or W above 65535, H (1 + 2 W) >= 2^31)
 *   mfr_png_depth_decode         headers [n] (device), records (device, offsets [n+1] i64 bytes, each a multiple of 16; record i
 *                                lies in [offsets[i], offsets[i+1]) and ends with >= 8 bytes after its stream) -> out [n,H,W] f32,
 *                                status [n] (0 ok; a parse code of the header passed through; MFR_PNG_E_* from the device).  A row
 *                                whose status is not 0 keeps its out plane untouched.  One wavefront per image: inflate (RFC 1950 /
 *                                1951: stored, fixed and dynamic blocks), size and Adler-32 check, filters 0-4, big-endian sample
 *                                / 1000.0 in f64 rounded to f32.  No input makes it read or write out of bounds or loop forever.
 */
size_t mfr_png_depth_workspace_bytes(int n, int H, int W);
int mfr_png_depth_decode(const void *headers, const uint8_t *records, const long long *offsets, int n, int H, int W,
                         long long max_record_bytes, void *scratch, size_t scratch_bytes, float *out, int32_t *status, void *stream);

/* ------------------------------------------------------------------------------------------
 * Gray plane of decoded RGB images at another size (csrc/resize.hip): rgb [n,H,W,3] u8 (mfr_jpeg_decode's) -> out [n,1,h,w] f32,
 * bit for bit datasets.gray_plane(rgb, (w, h)): luma (19595 R + 38470 G + 7471 B + 2^15) >> 16, that byte as f32, OpenCV-style
 * INTER_LINEAR of the float plane (source coordinate (x + 0.5) * n_in / n_out - 0.5, taps clamped at the edges, no antialiasing)
 * as top = a00 (1 - fx) + a01 fx, bot = a10 (1 - fx) + a11 fx, out = top (1 - fy) + bot fy with every product and sum rounded to
 * f32, then / 255f.  Call site: jpeg_ops.JpegDecoder.decode(resize=) and the device JPEG route of the batched loaders for datasets
 * whose files are not at the network size (ScanNet: 1296 x 968 -> 640 x 480).  Added to ABI v6 without a version bump (additive).
 *   y0, y1 [h] i32, fy [h] f32, x0, x1 [w] i32, fx [w] f32 (device): the tap tables, computed by the caller in float64 with the
 *     expression of datasets.resize_bilinear_f32 (jpeg_ops.resize_taps); indices are clamped to the image again on the device
 *   status [n] i32 (device, may be NULL): a row whose status is not 0 is left untouched
 * Any H, W, h, w >= 1, either direction, separate factors per axis; the same size reproduces byte / 255.
 */
int mfr_resize_gray_bilinear(const uint8_t *rgb, int n, int H, int W, const int32_t *status,
                             const int32_t *y0, const int32_t *y1, const float *fy,
                             const int32_t *x0, const int32_t *x1, const float *fx,
                             int h, int w, float *out, void *stream);

/* ------------------------------------------------------------------------------------------
 * 3x3 / stride 1 / pad 1 convolutions of the SuperPoint encoder (conv1b..conv4b, convPa, convDa; same
 * call site as the SuperPoint kernels above) as a fused Winograd F(2x2,3x3) kernel on the fp32 matrix
 * cores, with +bias, ReLU and the optional 2x2 max-pool in the output transform (csrc/winograd_conv.hip).
 *   mfr_wino_filter_bytes      size of the packed transformed filter (16*Cin*ceil32(Cout) floats); 0 if unsupported
 *   mfr_wino_filter_transform  w [Cout,Cin,3,3] f32 -> upk (G g G^T, packed in MFMA operand order); once per weight set
 *   mfr_conv3x3_wino           x [B,Cin,H,W] -> y [B,Cout,H,W] (pool=0) or [B,Cout,H/2,W/2] (pool=1; = max_pool2d(2,2)
 *                              of the activation); y = act(conv(x) + bias + residual): bias, residual ([B,Cout,H,W],
 *                              pool=0 only) may be NULL; act 0 none, 1 ReLU, 2 LeakyReLU(0.01).  Cin % 4 == 0; any Cout
 *                              (padded to a multiple of 32 inside the packed filter).  Also serves the stride-1 3x3
 *                              convolutions of LoFTR's ResNet-FPN backbone (BatchNorm folded into w / bias).
 * f32 Winograd arithmetic: agrees with a direct f32 convolution to ~1e-6 relative (not bit-identical).
 * ------------------------------------------------------------------------------------------ */
/* The same layer (same arguments, same epilogue) on the 16-bit matrix cores at fp32 accuracy by operand splitting (csrc/winograd_split.hip):
 * U = G g G^T and V = B^T d B are formed in fp32 as above.  f16x2 (round 5, what nets/conv.py runs; csrc/split_f16.h): V as two f16 terms,
 * U pre-scaled per output channel and packed as three f16 terms, three partial products; precondition |activation| < 16376.
 * bf16x3 (rounds 3-4): every operand split exactly into three bf16 terms, six partial products.  fp32 accumulate either way; error vs fp64 =
 * that of the exact-fp32 matrix instruction (profiles/r05_f16x2_probe.jsonl, r03_bf16x3_probe.jsonl).  Any Cin, Cout (padded to multiples
 * of 16 / 64 inside the packed filter; the two packed formats are not interchangeable).
 *   mfr_wino_*_filter_bytes      size of the packed, split filter (ceil(Cout/64) * ceil(Cin/16) * 96 KiB; f16x2: + the channel scales)
 *   mfr_wino_*_filter_transform  w [Cout,Cin,3,3] f32 -> upk; once per weight set
 *   mfr_conv3x3_wino_*           as mfr_conv3x3_wino */
size_t mfr_wino_f16x2_filter_bytes(int Cin, int Cout);
int mfr_wino_f16x2_filter_transform(const float *w, int Cin, int Cout, void *upk, void *stream);
int mfr_conv3x3_wino_f16x2(const float *x, const void *upk, const float *bias, const float *residual, int B, int Cin, int Cout,
                           int H, int W, int act, int pool, float *y, void *stream);
/* The same layer once more (same arguments, same epilogue, f16x2 arithmetic) as a DIRECT implicit GEMM (round 6, csrc/conv_direct.hip): the halo tile
 * of 16 input channels is split ONCE into LDS in operand form and the nine taps are shifted reads of it; a 4-wavefront workgroup (two per CU) computes 16 x 32 pixels x 64
 * channels (Cout <= 64) or 8 x 32 pixels x 128 channels.  2.25x Winograd's matrix instructions at ~2 other instructions per MFMA instead of 10-18: 1.0-1.3x
 * the Winograd kernel on every layer of the two backbones (profiles/r06_ab_direct_conv_halo.json), the default of nets/conv.py for SPLIT = f16x2.  Precondition |activation| <= 65504 (guarded: mfr_f16x2_guard_bind).
 *   mfr_conv3x3_direct_f16x2_filter_bytes   size of the packed filter: ceil(Cout/64) * ceil(Cin/16) * 54 KiB + the channel scales
 *   mfr_conv3x3_direct_f16x2_filter_pack    w [Cout,Cin,3,3] f32 -> packed; once per weight set
 *   mfr_conv3x3_direct_f16x2                as mfr_conv3x3_wino */
size_t mfr_conv3x3_direct_f16x2_filter_bytes(int Cin, int Cout);
int mfr_conv3x3_direct_f16x2_filter_pack(const float *w, int Cin, int Cout, void *packed, void *stream);
int mfr_conv3x3_direct_f16x2(const float *x, const void *packed, const float *bias, const float *residual, int B, int Cin, int Cout,
                             int H, int W, int act, int pool, float *y, void *stream);
/*   mfr_conv3x3_direct_f16x2_rows           the same layer with TOKEN-MAJOR output: yrows [B H W, ldy], channel c of pixel p at yrows[p ldy + c] (ldy >= Cout, both multiples
 *                                           of 4) -- what the 1x1 / linear layer behind the convolution reads (SuperPoint convDa -> convDb, models/superpoint.py; LoFTR
 *                                           layer1_outconv2 -> FinePreprocess' unfold, matchers.py:50): replaces the NCHW store + mfr_nchw_to_rows.  No residual, no pool. */
int mfr_conv3x3_direct_f16x2_rows(const float *x, const void *packed, const float *bias, int B, int Cin, int Cout, int H, int W, int act, float *yrows, int ldy, void *stream);
/*   mfr_conv3x3_direct_f16x2_tiled          both of the above with the PIXEL TILING chosen by the caller (A/B tool, tests; the entries above pass 0): tile_mode 0 = auto (the
 *                                           table in dc_conv), 1 = the 2-D tile (8 rows x 32 columns), 2 = the LINEAR tile: 256 consecutive units of the image as one padded
 *                                           linear space of pitch `pitch` >= W + 1 (0 = W + 1; <= 159), which computes ceil(H pitch / 256) * 256 positions per image instead
 *                                           of ceil(W / 32) * 32 * ceil(H / 8) * 8.  Same K loop, same products in the same order: bitwise the same output.  Mode 2 exists
 *                                           for Cout > 64, no pool; MFR_E_ARG otherwise.  ldrows > 0: token-major output as _rows (then no residual, no pool), 0: NCHW. */
int mfr_conv3x3_direct_f16x2_tiled(const float *x, const void *packed, const float *bias, const float *residual, int B, int Cin, int Cout, int H, int W,
                                   int act, int pool, float *y, int ldrows, int tile_mode, int pitch, void *stream);
/*   mfr_conv3x3s2_direct_f16x2              the STRIDE-2 3x3 / pad 1 layer (LoFTR's layer2.0 / layer3.0 conv1, `nn.Conv2d(k=3, s=2, p=1)` + folded BatchNorm + ReLU;
 *                                           un-vendored loftr/backbone/resnet_fpn.py, call site matchers.py:50) through the same kernel: the (2 TR + 1) x 65 patch is staged
 *                                           with its columns de-interleaved by parity, so every tap is again 32 consecutive LDS units; same packed filter as the
 *                                           stride-1 entry.  y [B,Cout,(H-1)/2+1,(W-1)/2+1]; act as above; no residual, no pool.  Rounds 1-5: mfr_conv_igemm_f16x2. */
int mfr_conv3x3s2_direct_f16x2(const float *x, const void *packed, const float *bias, int B, int Cin, int Cout, int H, int W, int act, float *y, void *stream);
/*   mfr_sp_conv1ab_f16x2         SuperPoint's first two layers in ONE kernel (round 5): y [B,64,H/2,W/2] = max_pool2(relu(conv1b(relu(conv1a(gray))))) for
 *                                gray [B,1,H,W]; w1a [64,1,3,3] / b1a [64] as they are, upk1b = mfr_wino_f16x2_filter_transform of conv1b's [64,64,3,3].
 *                                Bit-identical to mfr_conv3x3_c1_relu followed by mfr_conv3x3_wino_f16x2(..., act 1, pool 1): the 64-channel
 *                                intermediate (6.4 GB per 64 images) never exists in memory. */
int mfr_sp_conv1ab_f16x2(const float *gray, const float *w1a, const float *b1a, const void *upk1b, const float *bias1b, int B, int H, int W, float *y, void *stream);
size_t mfr_wino_bf16x3_filter_bytes(int Cin, int Cout);
int mfr_wino_bf16x3_filter_transform(const float *w, int Cin, int Cout, void *upk, void *stream);
int mfr_conv3x3_wino_bf16x3(const float *x, const void *upk, const float *bias, const float *residual, int B, int Cin, int Cout,
                            int H, int W, int act, int pool, float *y, void *stream);
size_t mfr_wino_filter_bytes(int Cin, int Cout);
int mfr_wino_filter_transform(const float *w, int Cin, int Cout, float *upk, void *stream);
int mfr_conv3x3_wino(const float *x, const float *upk, const float *bias, const float *residual, int B, int Cin, int Cout,
                     int H, int W, int act, int pool, float *y, void *stream);
/* the same convolution through a named kernel variant: 0 default, 1 classic, 2 software-pipelined K loop (bit-identical to 1),
 * 3 = 2 with the instruction placement left to the compiler, 4 shared-transform (two cout slices split every patch transform; bias
 * folded into an accumulator: f32-roundoff differences) -- for A/B timing (tools/tune_wino.py) and parity tests; other values: MFR_E_ARG */
int mfr_conv3x3_wino_variant(const float *x, const float *upk, const float *bias, const float *residual, int B, int Cin, int Cout,
                             int H, int W, int act, int pool, int variant, float *y, void *stream);

/* ------------------------------------------------------------------------------------------
 * Relative-pose-regression aggregator (csrc/corr_warp.hip).  Reference call sites:
 * CorrelationVolumeWarping.forward (lib/models/regression/aggregator.py:42-116) and
 * CorrelationVolumeWarpingQKV.forward (aggregator.py:134-191), and autograd's backward through them in
 * RegressionModel.training_step (lib/models/regression/model.py:87-97):
 *     cvolume = softmax(q^T k, dim=2);  warped = v cvolume^T;  pos = grid cvolume^T;  max = max_j cvolume
 * computed flash-style: the [B, N, N] volume never exists in memory, forward or backward.
 *   mfr_corr_warp_fwd   q, k [B,Dq,N] (Dq 16 or 32), v [B,32,N], grid [2,N] or NULL -> warped [B,32,N], pos [B,2,N]
 *                       (NULL iff grid NULL), max_score [B,N]; row_max / row_sum [B,N] are the softmax statistics
 *                       (max of log2(e)*score, and the sum of exp) the backward needs.
 *   mfr_corr_warp_bwd   d_warped [B,32,N], d_pos [B,2,N] or NULL, d_max [B,N] or NULL, delta [B,N] =
 *                       sum_c d_warped*warped + sum d_pos*pos + d_max*max_score  ->  dq, dk [B,Dq,N], dv [B,32,N].
 *                       One owner per output element (two kernels), no atomics: deterministic.
 * fp32 on the exact-fp32 matrix cores; agrees with the materialised fp32 computation to f32 round-off.
 * ------------------------------------------------------------------------------------------ */
int mfr_corr_warp_fwd(const float *q, const float *k, const float *v, const float *grid, int B, int Dq, int N,
                      float *warped, float *pos, float *max_score, float *row_max, float *row_sum, void *stream);
int mfr_corr_warp_bwd(const float *q, const float *k, const float *v, const float *grid, int B, int Dq, int N,
                      const float *d_warped, const float *d_pos, const float *d_max, const float *delta,
                      const float *row_max, const float *row_sum, float *dq, float *dk, float *dv, void *stream);

/* ------------------------------------------------------------------------------------------
 * DPT-Hybrid monocular depth (Ranftl et al., "Vision Transformers for Dense Prediction", ICCV 2021), the kernels BETWEEN its matrix products
 * (csrc/dpt.hip).  The architecture of record is `transformers.DPTForDepthEstimation` with is_hybrid=True (BiT ResNet-50 stem, ViT-Base,
 * reassemble / fusion neck, depth head); the products are mfr_gemm_*, mfr_conv_igemm_f16x2, mfr_conv3x3_direct_f16x2 and mfr_sg_attention.
 * fp32 storage and arithmetic.  Every argument check returns MFR_E_ARG before any launch; all pointers are device memory.
 *   mfr_dpt_prep          img: dtype 0 = u8 [B,H,W,3] (value / 255), 1 = f32 [B,3,H,W] in [0, 1]  ->  out [B,3,Hn,Wn] =
 *                         (F.interpolate(img, (Hn, Wn), 'bilinear', align_corners=False) - 0.5) / 0.5 with torch's arithmetic (source index
 *                         scale (dst + 0.5) - 0.5 clamped at 0, scale = in / out in f32).  Hn, Wn multiples of 32.
 *   mfr_dpt_groupnorm     y = GroupNorm(G, C)(x) [+ residual] [ReLU] over x [B,C,HW] (NCHW): BiT's BitGroupNormActivation, and with `residual` the
 *                         bottleneck's tail relu(norm3(.) + shortcut).  Two-pass statistics, biased variance, rsqrt(var + eps).  y may alias x or residual.
 *   mfr_dpt_maxpool3s2    3x3 / stride 2 max-pool of x [planes,H,W] padded with ZEROS by (pad_top, pad_bottom, pad_left, pad_right), each in 0..2 (BiT pads with
 *                         0, then pools: the padding takes part in the maximum).  TF-"SAME" is (0, 1) on an even axis and (1, 1) on an odd one.
 *                         y [planes,(H + pt + pb - 3) / 2 + 1,(W + pl + pr - 3) / 2 + 1].
 *   mfr_dpt_layernorm     mfr_layernorm for any C that is a multiple of 64 (<= 1024): out[r] = [residual[r] +] LayerNorm(x[r]) gamma + beta, row strides
 *                         ldx / ldr / ldo >= C; out may alias x or residual.  One wavefront per row, the row kept in registers.
 *   mfr_dpt_bias_gelu     x [rows,N] (row stride ld; N, ld multiples of 4, 16-byte aligned) <- GELU_erf(x + bias) in place (bias may be NULL)
 *   mfr_dpt_add_relu      s = a (+ b, may be NULL) over n floats (n % 4 == 0, 16-byte aligned): sum <- s (may be NULL), relu_out <- max(s, 0).  The fusion layer's
 *                         `hidden + residual_layer1(residual)` together with the pre-activation ReLU of the residual unit that reads the sum (no ReLU pass of its own).
 *   mfr_dpt_tokens        x [B,C,HW] (the patch projection's NCHW output) -> out [B,1 + HW,C] rows (row stride ldo, images (1 + HW) ldo apart):
 *                         out[b][0] = cls + pos[0];  out[b][1 + p][c] = x[b][c][p] + pos[1 + p][c]  (pos [1 + HW,C]: resized to this grid by the caller)
 *   mfr_dpt_tokens_inverse  out [B,C,HW] (NCHW) from rows: out[b][c][p] = act(rows[b img_stride + (skip + p) ld + c] + bias_img[b][c]); bias_img [B,C] or NULL
 *                         (the readout projection's cls half, W_b cls + b, one vector per image), gelu 0 | 1; skip = 1 drops the cls row
 *   mfr_dpt_shuffle       ConvTranspose2d(C, C, kernel = stride = s), s in {2, 4}, after its GEMM g [B H W, C s^2] (row stride ld, column (co s + i) s + j):
 *                         out [B,C,H s,W s], out[b][co][h s + i][w s + j] = g[(b H + h) W + w][(co s + i) s + j] + bias[co]
 *   mfr_dpt_head_tail     f [B,C,Hh,Wh] (C <= 64: the head's ReLU(conv3x3 . -> 32) output), w [C], bias: p = ReLU(w . f + bias); invert: p <- 1 / max(scale p + shift, 1e-8);
 *                         metres [B,Ho,Wo] = F.interpolate(p, (Ho, Wo), 'bilinear', align_corners=False); mm (u16 [B,Ho,Wo] or NULL) = the exact product
 *                         1000 metres rounded half to even, clamped to 0..65535 (NaN -> 0).  One pass over the full-resolution map.
 * Row-table twins of the two ends, for a consumer whose images are scattered rows of a larger batch (the fused route's interleaved pairs, nets/dpt.py
 * FusedDepthStage).  Added to ABI v6 without a version bump (purely additive); the tables are DEVICE memory and every entry is range-checked on the device:
 *   mfr_dpt_prep_rows     img u8 [N,H,W,3], rows i32 [m]: out[j] [3,Hn,Wn] = mfr_dpt_prep(dtype 0) of img[rows[j]], the same bits.  rows[j] outside [0, N): nothing is
 *                         read, out[j] is zeros and bit 0 of *status is set (an atomic OR; the caller clears the word).
 *   mfr_dpt_head_tail_rows  f [B,C,Hh,Wh], src / dst i32 [d]: plane dst[k] of metres [D,Ho,Wo] (and of mm, u16 or NULL) = mfr_dpt_head_tail of f[src[k]], the same
 *                         bits; one feature image may feed several planes, the dst entries must be distinct, planes not listed are not touched.  quantize 1: the
 *                         metres written are float32(mm / 1000.0) with the division in double (the value a reader of the 16-bit PNG holding mm gets).  dst[k]
 *                         outside [0, D): nothing is written; src[k] outside [0, B): the plane is zeros; either sets bit 0 of *status.
 * ------------------------------------------------------------------------------------------ */
int mfr_dpt_prep(const void *img, int dtype, int B, int H, int W, float *out, int Hn, int Wn, void *stream);
int mfr_dpt_groupnorm(const float *x, const float *gamma, const float *beta, const float *residual, int B, int C, int HW, int G, float eps, int relu,
                      float *y, void *stream);
int mfr_dpt_maxpool3s2(const float *x, int planes, int H, int W, int pad_top, int pad_bottom, int pad_left, int pad_right, float *y, void *stream);
int mfr_dpt_layernorm(const float *x, int ldx, const float *gamma, const float *beta, const float *residual, int ldr, long long rows, int C, float eps,
                      float *out, int ldo, void *stream);
int mfr_dpt_bias_gelu(float *x, int ld, long long rows, int N, const float *bias, void *stream);
int mfr_dpt_add_relu(const float *a, const float *b, long long n, float *sum, float *relu_out, void *stream);
int mfr_dpt_tokens(const float *x, const float *cls, const float *pos, int B, int C, int HW, float *out, int ldo, void *stream);
int mfr_dpt_tokens_inverse(const float *rows, int ld, long long img_stride, int skip, const float *bias_img, int gelu, int B, int C, int HW, float *out,
                           void *stream);
int mfr_dpt_shuffle(const float *g, int ld, const float *bias, int B, int C, int H, int W, int s, float *out, void *stream);
int mfr_dpt_head_tail(const float *f, const float *w, float bias, int B, int C, int Hh, int Wh, int invert, float scale, float shift, int Ho, int Wo,
                      float *metres, uint16_t *mm, void *stream);
int mfr_dpt_prep_rows(const uint8_t *img, int N, const int *rows, int m, int H, int W, float *out, int Hn, int Wn, int *status, void *stream);
int mfr_dpt_head_tail_rows(const float *f, const float *w, float bias, int B, int C, int Hh, int Wh, int invert, float scale, float shift, int Ho, int Wo,
                           const int *src, const int *dst, int d, float *metres, uint16_t *mm, int D, int quantize, int *status, void *stream);

/* ------------------------------------------------------------------------------------------
 * EfficientLoFTR (Wang et al., "Efficient LoFTR: Semi-Dense Local Feature Matching with Sparse-Like Speed", CVPR 2024), the kernels the
 * convolution / GEMM / coarse-matching entry points above do not cover (csrc/eloftr.hip; network: nets/eloftr.py).  The architecture of record is
 * `transformers.EfficientLoFTRForKeypointMatching` with the default configuration: hidden size 256, 8 heads x 32, 4 x 4 aggregation, 8 x 8 / 10 x 10
 * fine windows of 64 channels split 56 | 8.  fp32 storage and arithmetic.  Every argument check returns MFR_E_ARG before any launch; all pointers
 * are device memory.
 *   mfr_eloftr_stem_s2        y [B,Cout,H/2,W/2] = relu(conv3x3(x [B,1,H,W], w [Cout,1,3,3], stride 2, pad 1) + bias): the folded first RepVGG block
 *                             (mfr_conv3x3_c1_relu is stride 1).  H, W even, Cout <= 64.
 *   mfr_eloftr_aggregate      token rows x (token p of image i at x + i img_stride + p ldx, 256 channels, grid hc x wc, both multiples of 4) ->
 *                             q_out [nimg, hc/4 * wc/4, 256] = LayerNorm(depthwise 4x4 / stride 4 convolution, wq [256,1,4,4], no bias) and
 *                             kv_out (same shape) = LayerNorm(4x4 / stride 4 max-pool): ONE LayerNorm (gamma, beta, eps) for both, the 16 tokens of a
 *                             cell read once.  Either output may be NULL (cross attention takes q and k / v from different images).
 *   mfr_eloftr_rotary         rotary encoding in place on rows of q (and k, may be NULL) [rows, 256], row stride ld, row r at position r % La:
 *                             cos_sin [La, 256] = cos [128] | sin [128]; the pair (2 i, 2 i + 1) turns by angle i (the module's interleaved
 *                             rotate_half on the whole vector, before the split into heads).
 *   mfr_eloftr_attention      out = softmax(q k^T / sqrt(32)) v per head, heads x 32 contiguous channels, q [nb, Lq, .] (row stride ldq), k, v
 *                             [nb, Lk, .] (row stride ldkv), out row stride ldo: the short-sequence kernel (a wavefront owns 64 queries, key tiles of
 *                             a head in LDS); strides multiples of 4, pointers 16-byte aligned.
 *   mfr_eloftr_upsample4_rows dst rows of the 4 ha x 4 wa token grid (row stride ldx, image stride img_stride) = F.interpolate(msg [nimg, ha wa, 256]
 *                             as a map, scale_factor=4, bilinear, align_corners=False): the right half of the MLP's [x | message] operand.
 *   mfr_eloftr_upsample2x     out [planes,2H,2W] = (add, may be NULL) + F.interpolate(in [planes,H,W], scale_factor=2, bilinear, align_corners=False)
 *   mfr_eloftr_leaky_relu     x [rows, N] (row stride ld; N, ld multiples of 4) <- leaky_relu(x, slope) in place
 *   mfr_eloftr_rows_to_nchw   out [nimg, C, HW] = scale * token rows x (as for _aggregate), C % 32 == 0: the transformer's output as the map the fine
 *                             pyramid convolves, with the module's 1 / sqrt(hidden) in the same pass.
 *   mfr_eloftr_gather_windows out [B maxN, win^2, 64]: slot b maxN + s (s < min(n[b], maxN); other slots untouched) = the win x win window of image
 *                             img_ids[b] whose origin is the corner of cell cell_ids[b ld_cells + s] (grid width wc, cell_px pixels) minus pad, in the
 *                             FULL-resolution frame 2 Hh x 2 Wh, zeros outside it (unfold's padding).  feat_half [nimg, Hh, Wh, 64] is the HALF
 *                             resolution NHWC map: the pyramid's last x2 bilinear up-sampling is evaluated per window pixel, the full-resolution map
 *                             is never written.  (win, pad) = (8, 0) for image 0, (10, 1) for image 1.
 *   mfr_eloftr_fine_match     the two-stage refinement per slot, one wavefront each: stage 1 = correlation of the first 56 channels (both / sqrt 56),
 *                             softmax over rows x softmax over columns of the 64 x 100 matrix, interior 8 x 8, arg-max (lowest index on ties),
 *                             offsets grid - 4 + 0.5; stage 2 = last 8 channels (window 1 / sqrt 8), the 3 x 3 values of the padded 10 x 10 grid at
 *                             the UNPADDED winner index + {-1, 0, 1} (-1 wraps to 9, as in the module), softmax(. / 10), expectation added to pts1.
 *                             pts0 / pts1 [B maxN, 2] pixels of the padded frame; stage1_arg [B maxN] (may be NULL) the flat arg-max index.
 *   mfr_eloftr_compact        per pair, the first min(n[b], maxN) slots in order with both end points inside the unpadded frame (x < W, y < H) ->
 *                             out0 / out1 [B, maxN, 2], out_conf [B, maxN] (from conf [B, ld_conf]) zero-filled behind n_out[b].
 * ------------------------------------------------------------------------------------------ */
int mfr_eloftr_stem_s2(const float *x, const float *w, const float *bias, int B, int H, int W, int out_channels, float *y, void *stream);
int mfr_eloftr_aggregate(const float *x, int ldx, long long img_stride, int nimg, int hc, int wc, const float *wq, const float *gamma, const float *beta, float eps,
                         float *q_out, float *kv_out, void *stream);
int mfr_eloftr_rotary(float *q, float *k, int ld, const float *cos_sin, long long rows, int La, void *stream);
int mfr_eloftr_attention(const float *q, int ldq, const float *k, const float *v, int ldkv, int nb, int Lq, int Lk, int heads, float *out, int ldo, void *stream);
int mfr_eloftr_upsample4_rows(const float *msg, int ldm, int nimg, int ha, int wa, float *dst, int ldx, long long img_stride, void *stream);
int mfr_eloftr_upsample2x(const float *in, const float *add, float *out, int planes, int H, int W, void *stream);
int mfr_eloftr_leaky_relu(float *x, int ld, long long rows, int N, float slope, void *stream);
int mfr_eloftr_rows_to_nchw(const float *x, int ldx, long long img_stride, int nimg, int C, int HW, float scale, float *out, void *stream);
int mfr_eloftr_gather_windows(const float *feat_half, int nimg, int Hh, int Wh, int C, const int32_t *img_ids, const int32_t *cell_ids, long long ld_cells,
                              const int32_t *n, int B, int maxN, int wc, int cell_px, int win, int pad, float *out, void *stream);
int mfr_eloftr_fine_match(const float *win0, const float *win1, const int32_t *cell_i, const int32_t *cell_j, long long ld_cells, const int32_t *n, int B, int maxN,
                          int wc, int cell_px, float *pts0, float *pts1, int32_t *stage1_arg, void *stream);
int mfr_eloftr_compact(const float *pts0, const float *pts1, const float *conf, long long ld_conf, const int32_t *n, int B, int maxN, int W, int H, float *out0,
                       float *out1, float *out_conf, int32_t *n_out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Depth Anything V2 (Yang et al., NeurIPS 2024: a DINOv2 ViT behind a DPT head), the kernels the DPT-Hybrid entry points above do not cover
 * (csrc/depth_anything.hip; network: nets/depth_anything.py).  The architecture of record is `transformers.DepthAnythingForDepthEstimation` on a
 * Dinov2 backbone.  Purely additive (no ABI version bump).  fp32 storage and arithmetic.  Every argument check returns MFR_E_ARG before any launch;
 * all pointers are device memory.
 *   mfr_da_patch_rows      img: dtype 0 = u8 [B,H,W,3] (value / 255), 1 = f32 [B,3,H,W] in [0, 1]  ->  rows [B gh gw, ldk]: row (b gh + y) gw + x holds the
 *                          14 x 14 patch (y, x) of (F.interpolate(img, (14 gh, 14 gw), 'bilinear', align_corners=False) - mean[c]) / std[c] (torch's arithmetic,
 *                          as mfr_dpt_prep) at column (c 14 + i) 14 + j, columns 588 .. ldk - 1 zero: the layout in which the 14 x 14 / stride 14 patch
 *                          convolution's weight reshaped to [h, 588] is a linear layer's.  ldk >= 588, a multiple of 4; rows 16-byte aligned.  The
 *                          normalised full-resolution image is never written.
 *   mfr_da_patch_rows_tab  the row-table twin (semantics of mfr_dpt_prep_rows): img u8 [N,H,W,3], tab i32 [m]: the gh gw rows of output image j = those of
 *                          mfr_da_patch_rows(dtype 0) on img[tab[j]], the same bits.  tab[j] outside [0, N): nothing is read, the image's rows are zeros
 *                          and bit 0 of *status is set (an atomic OR; the caller clears the word).
 *   mfr_da_tokens          x [B HW, ldx] (the embedding product's output) -> out [B,1 + HW,C] rows (row stride ldo, images (1 + HW) ldo apart):
 *                          out[b][0] = cls + pos[0];  out[b][1 + p] = x[b HW + p] + pos[1 + p]  (pos [1 + HW,C]: resized to this grid by the caller).
 *                          C, ldx, ldo multiples of 4, pointers 16-byte aligned.
 *   mfr_da_head_tail       mfr_dpt_head_tail with Depth Anything's last activation: p = max_depth sigmoid(w . f + bias) (metric 1) or ReLU(w . f + bias)
 *                          (metric 0: the relative checkpoints); the resize, the millimetres and their rounding are mfr_dpt_head_tail's (one device function).
 *   mfr_da_head_tail_rows  its row-table twin: mfr_dpt_head_tail_rows's src / dst / quantize / status semantics, the same bits as the plain entry.
 * ------------------------------------------------------------------------------------------ */
int mfr_da_patch_rows(const void *img, int dtype, int B, int H, int W, int gh, int gw, float mean0, float mean1, float mean2, float std0, float std1, float std2,
                      float *rows, int ldk, void *stream);
int mfr_da_patch_rows_tab(const uint8_t *img, int N, const int *tab, int m, int H, int W, int gh, int gw, float mean0, float mean1, float mean2, float std0,
                          float std1, float std2, float *rows, int ldk, int *status, void *stream);
int mfr_da_tokens(const float *x, int ldx, const float *cls, const float *pos, int B, int C, int HW, float *out, int ldo, void *stream);
int mfr_da_head_tail(const float *f, const float *w, float bias, int B, int C, int Hh, int Wh, int metric, float max_depth, int Ho, int Wo, float *metres,
                     uint16_t *mm, void *stream);
int mfr_da_head_tail_rows(const float *f, const float *w, float bias, int B, int C, int Hh, int Wh, int metric, float max_depth, int Ho, int Wo, const int *src,
                          const int *dst, int d, float *metres, uint16_t *mm, int D, int quantize, int *status, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MFR_HIP_H */
