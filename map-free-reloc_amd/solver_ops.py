"""Batched, device-resident pose-solver ops: thin torch<->C-ABI glue over csrc/pnp.hip,
csrc/scale.hip, csrc/emat.hip (include/mfr_hip.h).  All tensors live on the GPU; torch only
provides memory and the stream.

Reference leg being replaced: lib/models/matching/pose_solver.py (PnPSolver :175-235,
EssentialMatrixSolver :20-61, EssentialMatrixMetricSolver :115-172).
"""
import torch

from . import _lib

# values of include/mfr_hip.h, stated here once for the package
ST_OK, ST_TOO_FEW, ST_BAD_DEPTH, ST_NO_MODEL, ST_DEGENERATE = range(5)      # MFR_ST_*
K_F32, K_F64 = 0, 1                                                         # MFR_K_F32 / MFR_K_F64
NSEG = 16                                                                   # partial minima per image of mfr_depth_min


def _chk(t, dtype, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise _lib.MfrLibraryError(f"{name} must be a CUDA(HIP) tensor: the HIP path has no CPU fallback")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    return t.contiguous()


def _chk_K(K0, K1=None):
    """Intrinsics go to the library in the dtype the `data` dict holds them: float64 from the Map-free loader
    (lib/datasets/utils.py:117-130 multiplies a float64 eye(3) into K), float32 from resize=None datasets.  -> (K0, K1, tag);
    a mixed pair is promoted to float64, as numpy would promote the reference's arithmetic."""
    Ks = [K for K in (K0, K1) if K is not None]
    for K in Ks:
        if not (isinstance(K, torch.Tensor) and K.is_cuda):
            raise _lib.MfrLibraryError("K must be a CUDA(HIP) tensor: the HIP path has no CPU fallback")
        if K.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"K: expected float32 or float64, got {K.dtype}")
    dt = torch.float64 if any(K.dtype == torch.float64 for K in Ks) else torch.float32
    out = [None if K is None else K.to(dt).contiguous() for K in (K0, K1)]
    return out[0], out[1], (K_F64 if dt == torch.float64 else K_F32)


def _chk_corr(pts0, pts1, n_corr):
    """the correspondence triple every solver takes -> (pts0, pts1, n_corr, B, maxN, device)"""
    pts0 = _chk(pts0, torch.float32, "pts0"); pts1 = _chk(pts1, torch.float32, "pts1")
    n_corr = _chk(n_corr, torch.int32, "n_corr")
    B, maxN, _ = pts0.shape
    return pts0, pts1, n_corr, B, maxN, pts0.device


def _pose_out(B, dev):
    """R [B,3,3] f64, t [B,3] f64, n_inliers [B] i32, status [B] i32"""
    return (torch.empty(B, 3, 3, dtype=torch.float64, device=dev), torch.empty(B, 3, dtype=torch.float64, device=dev),
            torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev))


def _i32(dev, *shape):
    return torch.empty(*shape, dtype=torch.int32, device=dev)


class _Workspace:
    """what the batched ops share: a grow-only scratch buffer, replaced when the device changes"""
    _buf = None

    def _ws(self, nbytes, dev):
        if self._buf is None or self._buf.numel() < nbytes or self._buf.device != dev:
            self._buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)
        return self._buf


def depth_min_partials(depth):
    """[B,H,W] f32 -> [B,16] partial minima (pose_solver.py:196 depth_0.min())."""
    _lib.load(require_gpu=True)
    depth = _chk(depth, torch.float32, "depth")
    B, H, W = depth.shape
    out = torch.empty(B, NSEG, dtype=torch.float32, device=depth.device)
    _lib.call("mfr_depth_min", depth, B, H, W, out)
    return out


def pnp_lift(pts0, pts1, n_corr, depth0, K0):
    """pose_solver.py:186-206: returns xyz [B,maxN,3] f64, obs [B,maxN,2] f64, src_idx, n_valid."""
    _lib.load(require_gpu=True)
    pts0, pts1, n_corr, B, maxN, dev = _chk_corr(pts0, pts1, n_corr)
    depth0 = _chk(depth0, torch.float32, "depth0")
    K0, _, kdt = _chk_K(K0)
    _, H, W = depth0.shape
    part = depth_min_partials(depth0)
    xyz = torch.zeros(B, maxN, 3, dtype=torch.float64, device=dev)
    obs = torch.zeros(B, maxN, 2, dtype=torch.float64, device=dev)
    src = torch.zeros(B, maxN, dtype=torch.int32, device=dev)
    nv = torch.zeros(B, dtype=torch.int32, device=dev)
    _lib.call("mfr_pnp_lift", pts0, pts1, n_corr, B, maxN, depth0, part, H, W, K0, kdt, xyz, obs, src, nv)
    return xyz, obs, src, nv


def pnp_ransac(xyz, obs, n_valid, K1, pair_ids, max_iters=1000, thr=3.0, conf=0.9999, seed=0):
    """cv.solvePnPRansac(P3P) + refit + ITERATIVE refinement restatement (pose_solver.py:209-235)
    on already lifted points.  Returns dict(R, t, n_inliers, status, mask, best_iter, iters_run, counts)."""
    _lib.load(require_gpu=True)
    xyz = _chk(xyz, torch.float64, "xyz"); obs = _chk(obs, torch.float64, "obs")
    n_valid = _chk(n_valid, torch.int32, "n_valid"); K1, _, kdt = _chk_K(K1)
    pair_ids = _chk(pair_ids, torch.int64, "pair_ids")
    B, maxN, _ = xyz.shape
    dev = xyz.device
    max_iters = max(int(max_iters), 1)
    counts, inl = _i32(dev, B, max_iters), _i32(dev, B, maxN)
    R, t, ni, st = _pose_out(B, dev)
    mask = torch.empty(B, maxN, dtype=torch.uint8, device=dev)
    bi, ir = _i32(dev, B), _i32(dev, B)
    _lib.call("mfr_pnp_ransac", xyz, obs, n_valid, B, maxN, K1, kdt, max_iters, float(thr), float(conf), int(seed), pair_ids,
              counts, inl, R, t, ni, st, mask, bi, ir)
    return dict(R=R, t=t, n_inliers=ni, status=st, mask=mask, best_iter=bi, iters_run=ir, counts=counts)


class PnPBatchSolver(_Workspace):
    """PnPSolver.estimate_pose (pose_solver.py:184-235) for a batch of pairs, one C-ABI call."""

    def __init__(self, max_iters=1000, reproj_thr=3.0, confidence=0.9999, seed=0):
        self.max_iters = max(int(max_iters), 1)
        self.reproj_thr = float(reproj_thr)
        self.confidence = float(confidence)
        self.seed = int(seed)

    def __call__(self, pts0, pts1, n_corr, depth0, K0, K1, pair_ids, want_mask=False):
        lib = _lib.load(require_gpu=True)
        pts0, pts1, n_corr, B, maxN, dev = _chk_corr(pts0, pts1, n_corr)
        depth0 = _chk(depth0, torch.float32, "depth0")
        K0, K1, kdt = _chk_K(K0, K1)
        pair_ids = _chk(pair_ids, torch.int64, "pair_ids")
        _, H, W = depth0.shape
        ws = self._ws(lib.mfr_pnp_workspace_bytes(B, maxN, self.max_iters), dev)
        R, t, ni, st = _pose_out(B, dev)
        mask = torch.empty(B, maxN, dtype=torch.uint8, device=dev) if want_mask else None
        _lib.call("mfr_pnp_solve_batch", pts0, pts1, n_corr, B, maxN, depth0, H, W, K0, K1, kdt, self.max_iters, self.reproj_thr,
                  self.confidence, self.seed, pair_ids, ws, ws.numel(), R, t, ni, st, mask)
        out = dict(R=R, t=t, n_inliers=ni, status=st)
        if want_mask:
            out["mask"] = mask
        return out


RIG_MAX_T = 16      # frames per rig the library takes (include/mfr_hip.h)


def rig_rows(rig_T):
    """[B,T,4,4] rigid transforms (last frame's camera -> frame j's camera) -> the library's [B,T,12] f64 rows: R row-major, then t"""
    rig_T = _chk(rig_T, torch.float64, "rig_T")
    if rig_T.dim() != 4 or rig_T.shape[-2:] != (4, 4):
        raise ValueError(f"rig_T: expected [B,T,4,4], got {tuple(rig_T.shape)}")
    return torch.cat([rig_T[..., :3, :3].reshape(*rig_T.shape[:2], 9), rig_T[..., :3, 3]], dim=-1).contiguous()


def rig_pnp_ransac(xyz, obs, n_valid, K1, rig, pair_ids, max_iters=1000, thr=3.0, conf=0.9999, seed=0):
    """The rig solver on already lifted rows (csrc/pnp_rig.hip): xyz [B,T,maxN,3], obs [B,T,maxN,2], n_valid [B,T], K1 [B,T,3,3],
    rig [B,T,12] f64 (rig_rows).  Returns dict(R, t, n_inliers, status, mask [B,T,maxN], best_iter, iters_run, counts)."""
    _lib.load(require_gpu=True)
    xyz = _chk(xyz, torch.float64, "xyz"); obs = _chk(obs, torch.float64, "obs")
    n_valid = _chk(n_valid, torch.int32, "n_valid"); K1, _, kdt = _chk_K(K1)
    rig = _chk(rig, torch.float64, "rig"); pair_ids = _chk(pair_ids, torch.int64, "pair_ids")
    B, T, maxN, _ = xyz.shape
    if tuple(rig.shape) != (B, T, 12) or tuple(K1.shape) != (B, T, 3, 3) or tuple(n_valid.shape) != (B, T):
        raise ValueError("rig_pnp_ransac: rig [B,T,12], K1 [B,T,3,3] and n_valid [B,T] must match xyz [B,T,maxN,3]")
    dev = xyz.device
    max_iters = max(int(max_iters), 1)
    counts, inl = _i32(dev, B, max_iters), _i32(dev, B, T, maxN)
    R, t, ni, st = _pose_out(B, dev)
    mask = torch.empty(B, T, maxN, dtype=torch.uint8, device=dev)
    bi, ir = _i32(dev, B), _i32(dev, B)
    _lib.call("mfr_rig_pnp_ransac", xyz, obs, n_valid, B, T, maxN, K1, kdt, rig, max_iters, float(thr), float(conf), int(seed), pair_ids,
              counts, inl, R, t, ni, st, mask, bi, ir)
    return dict(R=R, t=t, n_inliers=ni, status=st, mask=mask, best_iter=bi, iters_run=ir, counts=counts)


class RigPnPBatchSolver(_Workspace):
    """One pose (reference -> LAST window frame) for a rig of T query frames per sample, one C-ABI call (csrc/pnp_rig.hip).
    pts0 / pts1 [B,T,maxN,2] f32, n_corr [B,T] i32, depth0 [B,H,W], K0 [B,3,3], K1_multi [B,T,3,3], rig_T [B,T,4,4] f64
    (A_j: last frame's camera -> frame j's camera), pair_ids [B].  The mask is [B,T,maxN] over ORIGINAL correspondence indices."""

    def __init__(self, max_iters=1000, reproj_thr=3.0, confidence=0.9999, seed=0):
        self.max_iters = max(int(max_iters), 1)
        self.reproj_thr = float(reproj_thr)
        self.confidence = float(confidence)
        self.seed = int(seed)

    def __call__(self, pts0, pts1, n_corr, depth0, K0, K1_multi, rig_T, pair_ids, want_mask=False):
        lib = _lib.load(require_gpu=True)
        pts0 = _chk(pts0, torch.float32, "pts0"); pts1 = _chk(pts1, torch.float32, "pts1")
        n_corr = _chk(n_corr, torch.int32, "n_corr")
        if pts0.dim() != 4 or pts0.shape != pts1.shape or pts0.shape[-1] != 2:
            raise ValueError(f"pts0 / pts1: expected [B,T,maxN,2], got {tuple(pts0.shape)} / {tuple(pts1.shape)}")
        B, T, maxN, _ = pts0.shape
        if not 1 <= T <= RIG_MAX_T:
            raise ValueError(f"a rig holds 1..{RIG_MAX_T} frames, got T = {T}")
        dev = pts0.device
        depth0 = _chk(depth0, torch.float32, "depth0")
        K0, K1, kdt = _chk_K(K0, K1_multi)
        rig = rig_rows(rig_T)
        pair_ids = _chk(pair_ids, torch.int64, "pair_ids")
        if (tuple(n_corr.shape) != (B, T) or tuple(K1.shape) != (B, T, 3, 3) or tuple(rig.shape) != (B, T, 12)
                or depth0.dim() != 3 or depth0.shape[0] != B or tuple(K0.shape) != (B, 3, 3) or tuple(pair_ids.shape) != (B,)):
            raise ValueError("RigPnPBatchSolver: n_corr [B,T], K1_multi [B,T,3,3], rig_T [B,T,4,4], depth0 [B,H,W], K0 [B,3,3], "
                             "pair_ids [B] must match pts0 [B,T,maxN,2]")
        _, H, W = depth0.shape
        ws = self._ws(lib.mfr_rig_pnp_workspace_bytes(B, T, maxN, self.max_iters), dev)
        R, t, ni, st = _pose_out(B, dev)
        mask = torch.empty(B, T, maxN, dtype=torch.uint8, device=dev) if want_mask else None
        _lib.call("mfr_rig_pnp_solve_batch", pts0, pts1, n_corr, B, T, maxN, depth0, H, W, K0, K1, kdt, rig, self.max_iters, self.reproj_thr,
                  self.confidence, self.seed, pair_ids, ws, ws.numel(), R, t, ni, st, mask)
        out = dict(R=R, t=t, n_inliers=ni, status=st)
        if want_mask:
            out["mask"] = mask
        return out


EMAT_SCORE = {"magsac": 0, "count": 1}      # MFR_EMAT_SCORE_* of include/mfr_hip.h
MAGSAC_LUT_M = 2048


def magsac_lut_host(M=MAGSAC_LUT_M):
    """[M + 1, 2] float64 (normalised MAGSAC++ loss, IRLS weight) over r^2 / cut in [0, 1]: mfr_magsac_lut (host code of the library)"""
    import numpy as np
    t = np.zeros((M + 1, 2), dtype=np.float64)
    _lib.call("mfr_magsac_lut", t.ctypes.data, M)
    return t


class EssentialBatchSolver(_Workspace):
    """EssentialMatrixSolver.estimate_pose (pose_solver.py:29-61) for a batch of pairs.  score 'magsac' (default) = what the
    reference asks OpenCV for (cv.USAC_MAGSAC, :46-48): MAGSAC++ model quality + sigma-consensus++; 'count' = inlier count + LM
    polish (rounds 1-3, kept for A/B)."""

    def __init__(self, pix_thr=2.0, confidence=0.9999, seed=0, max_iters=1000, score="magsac", max_thr_ratio=1.0):
        if score not in EMAT_SCORE:
            raise ValueError(f"EssentialBatchSolver: unknown score {score!r}; known: {sorted(EMAT_SCORE)}")
        if not max_thr_ratio >= 1.0:
            raise ValueError("EssentialBatchSolver: max_thr_ratio must be >= 1")
        self.pix_thr, self.confidence = float(pix_thr), float(confidence)
        self.seed, self.max_iters = int(seed), max(int(max_iters), 1)
        self.score, self.max_thr_ratio = EMAT_SCORE[score], float(max_thr_ratio)
        self._lut = None

    def _table(self, dev):
        if self._lut is None or self._lut.device != dev:
            self._lut = torch.from_numpy(magsac_lut_host()).to(dev)
        return self._lut

    def __call__(self, pts0, pts1, n_corr, K0, K1, pair_ids, diagnostics=False):
        lib = _lib.load(require_gpu=True)
        pts0, pts1, n_corr, B, maxN, dev = _chk_corr(pts0, pts1, n_corr)
        K0, K1, kdt = _chk_K(K0, K1)
        pair_ids = _chk(pair_ids, torch.int64, "pair_ids")
        ws = self._ws(lib.mfr_emat_workspace_bytes(B, maxN, self.max_iters), dev)
        lut = self._table(dev) if self.score == 0 else None
        R, t, ni, st = _pose_out(B, dev)
        mask = torch.empty(B, maxN, dtype=torch.uint8, device=dev)
        bi = ir = cnt = los = lo = None
        if diagnostics:
            bi, ir, lo, cnt = _i32(dev, B), _i32(dev, B), _i32(dev, B), _i32(dev, B, self.max_iters)
            los = torch.zeros(B, self.max_iters, dtype=torch.float64, device=dev)
        _lib.call("mfr_emat_solve_batch", pts0, pts1, n_corr, B, maxN, K0, K1, kdt, self.pix_thr, self.confidence, self.max_iters, self.seed,
                  pair_ids, self.score, lut, MAGSAC_LUT_M, self.max_thr_ratio, ws, ws.numel(), R, t, ni, st, mask, bi, ir, cnt, los, lo)
        out = dict(R=R, t=t, n_inliers=ni, status=st, mask=mask)
        if diagnostics:
            out.update(best_iter=bi, iters_run=ir, counts=cnt, losses=los, lo_runs=lo)
        return out


class ProcrustesBatchSolver(_Workspace):
    """ProcrustesSolver.estimate_pose (pose_solver.py:238-320, REFINE False) for a batch of pairs."""

    def __init__(self, max_corr_dist=0.05, confidence=0.999, seed=0, max_iters=4096):
        self.max_corr_dist, self.confidence = float(max_corr_dist), float(confidence)
        self.seed, self.max_iters = int(seed), max(int(max_iters), 1)

    def __call__(self, pts0, pts1, n_corr, depth0, depth1, K0, K1, pair_ids, diagnostics=False):
        lib = _lib.load(require_gpu=True)
        pts0, pts1, n_corr, B, maxN, dev = _chk_corr(pts0, pts1, n_corr)
        depth0 = _chk(depth0, torch.float32, "depth0"); depth1 = _chk(depth1, torch.float32, "depth1")
        K0, K1, kdt = _chk_K(K0, K1)
        pair_ids = _chk(pair_ids, torch.int64, "pair_ids")
        _, H, W = depth0.shape
        ws = self._ws(lib.mfr_procrustes_workspace_bytes(B, maxN, self.max_iters), dev)
        R, t, ni, st = _pose_out(B, dev)
        bi = ir = cnt = None
        if diagnostics:
            bi, ir, cnt = _i32(dev, B), _i32(dev, B), _i32(dev, B, self.max_iters)
        _lib.call("mfr_procrustes_solve_batch", pts0, pts1, n_corr, B, maxN, depth0, depth1, H, W, K0, K1, kdt, self.max_corr_dist,
                  self.confidence, self.max_iters, self.seed, pair_ids, ws, ws.numel(), R, t, ni, st, bi, ir, cnt)
        out = dict(R=R, t=t, n_inliers=ni, status=st)
        if diagnostics:
            out.update(best_iter=bi, iters_run=ir, counts=cnt)
        return out


class RigProcrustesBatchSolver(_Workspace):
    """One pose (reference -> LAST window frame) for a rig of T query frames per sample from 3-D/3-D correspondences over all T + 1 depth
    maps, one C-ABI call (the rig entry point of csrc/procrustes.hip).  pts0 / pts1 [B,T,maxN,2] f32, n_corr [B,T] i32, depth0 [B,H,W],
    depth1 [B,T,H,W], K0 [B,3,3], K1_multi [B,T,3,3], rig_T [B,T,4,4] f64 (A_j: last frame's camera -> frame j's camera), pair_ids [B].
    The mask is [B,T,maxN] over ORIGINAL correspondence indices; diagnostics adds n_valid [B,T], best_iter, iters_run, counts."""

    def __init__(self, max_corr_dist=0.05, confidence=0.999, seed=0, max_iters=4096):
        self.max_corr_dist, self.confidence = float(max_corr_dist), float(confidence)
        self.seed, self.max_iters = int(seed), max(int(max_iters), 1)

    def __call__(self, pts0, pts1, n_corr, depth0, depth1, K0, K1_multi, rig_T, pair_ids, want_mask=False, diagnostics=False):
        lib = _lib.load(require_gpu=True)
        pts0 = _chk(pts0, torch.float32, "pts0"); pts1 = _chk(pts1, torch.float32, "pts1")
        n_corr = _chk(n_corr, torch.int32, "n_corr")
        if pts0.dim() != 4 or pts0.shape != pts1.shape or pts0.shape[-1] != 2:
            raise ValueError(f"pts0 / pts1: expected [B,T,maxN,2], got {tuple(pts0.shape)} / {tuple(pts1.shape)}")
        B, T, maxN, _ = pts0.shape
        if not 1 <= T <= RIG_MAX_T:
            raise ValueError(f"a rig holds 1..{RIG_MAX_T} frames, got T = {T}")
        dev = pts0.device
        depth0 = _chk(depth0, torch.float32, "depth0"); depth1 = _chk(depth1, torch.float32, "depth1")
        K0, K1, kdt = _chk_K(K0, K1_multi)
        rig = rig_rows(rig_T)
        pair_ids = _chk(pair_ids, torch.int64, "pair_ids")
        if (tuple(n_corr.shape) != (B, T) or tuple(K1.shape) != (B, T, 3, 3) or tuple(rig.shape) != (B, T, 12)
                or depth0.dim() != 3 or depth0.shape[0] != B or tuple(depth1.shape) != (B, T) + tuple(depth0.shape[1:])
                or tuple(K0.shape) != (B, 3, 3) or tuple(pair_ids.shape) != (B,)):
            raise ValueError("RigProcrustesBatchSolver: n_corr [B,T], K1_multi [B,T,3,3], rig_T [B,T,4,4], depth0 [B,H,W], depth1 [B,T,H,W], "
                             "K0 [B,3,3], pair_ids [B] must match pts0 [B,T,maxN,2]")
        _, H, W = depth0.shape
        ws = self._ws(lib.mfr_rig_procrustes_workspace_bytes(B, T, maxN, self.max_iters), dev)
        R, t, ni, st = _pose_out(B, dev)
        mask = torch.empty(B, T, maxN, dtype=torch.uint8, device=dev) if want_mask else None
        nv = bi = ir = cnt = None
        if diagnostics:
            nv, bi, ir, cnt = _i32(dev, B, T), _i32(dev, B), _i32(dev, B), _i32(dev, B, self.max_iters)
        _lib.call("mfr_rig_procrustes_solve_batch", pts0, pts1, n_corr, B, T, maxN, depth0, depth1, H, W, K0, K1, kdt, rig,
                  self.max_corr_dist, self.confidence, self.max_iters, self.seed, pair_ids, ws, ws.numel(), R, t, ni, st, mask, nv, bi, ir, cnt)
        out = dict(R=R, t=t, n_inliers=ni, status=st)
        if want_mask:
            out["mask"] = mask
        if diagnostics:
            out.update(n_valid=nv, best_iter=bi, iters_run=ir, counts=cnt)
        return out


def _chk_rig(pts0, pts1, n_corr, K0, K1_multi, rig_T, who):
    """the rig solvers' common arguments -> (pts0, pts1, n_corr, K0, K1, k tag, rig rows, B, T, maxN, device)"""
    pts0 = _chk(pts0, torch.float32, "pts0"); pts1 = _chk(pts1, torch.float32, "pts1")
    n_corr = _chk(n_corr, torch.int32, "n_corr")
    if pts0.dim() != 4 or pts0.shape != pts1.shape or pts0.shape[-1] != 2:
        raise ValueError(f"pts0 / pts1: expected [B,T,maxN,2], got {tuple(pts0.shape)} / {tuple(pts1.shape)}")
    B, T, maxN, _ = pts0.shape
    if not 1 <= T <= RIG_MAX_T:
        raise ValueError(f"a rig holds 1..{RIG_MAX_T} frames, got T = {T}")
    K0, K1, kdt = _chk_K(K0, K1_multi)
    rig = rig_rows(rig_T)
    if tuple(n_corr.shape) != (B, T) or tuple(K1.shape) != (B, T, 3, 3) or tuple(rig.shape) != (B, T, 12) or tuple(K0.shape) != (B, 3, 3):
        raise ValueError(f"{who}: n_corr [B,T], K1_multi [B,T,3,3], rig_T [B,T,4,4], K0 [B,3,3] must match pts0 [B,T,maxN,2]")
    return pts0, pts1, n_corr, K0, K1, kdt, rig, B, T, maxN, pts0.device


def rig_emat_stage1(solver, pts0, pts1, n_corr, K0, K1_multi, pair_ids):
    """Stage 1 of the essential-matrix rig solver: `solver` (an EssentialBatchSolver) over the B*T rows, K0 repeated per row, RANSAC key
    pair_id*T + j.  pts0 / pts1 [B,T,maxN,2] -> dict(R [B,T,3,3], t [B,T,3] unit, n_inliers, status [B,T], mask [B,T,maxN])"""
    B, T, maxN, _ = pts0.shape
    rows = lambda x: x.reshape((B * T,) + tuple(x.shape[2:])).contiguous()
    pid = (pair_ids.reshape(B, 1) * T + torch.arange(T, dtype=torch.int64, device=pair_ids.device)).reshape(-1)
    o = solver(rows(pts0), rows(pts1), rows(n_corr), K0.repeat_interleave(T, dim=0).contiguous(), rows(K1_multi), pid)
    return {k: o[k].reshape((B, T) + tuple(o[k].shape[1:])) for k in ("R", "t", "n_inliers", "status", "mask")}


def rig_emat_stage2(pts0, pts1, n_corr, K0, K1_multi, rig_T, stage1, pix_thr=2.0, want_mask=False, diagnostics=False):
    """Stage 2 of the essential-matrix rig solver (csrc/emat_rig.hip) on stage 1's device outputs: the rig-level hypotheses, pooled score,
    refinement.  -> dict(R, t, n_inliers, status [, mask [B,T,maxN]] [, hyp_counts [B,T(T-1)], best_hyp [B]])"""
    lib = _lib.load(require_gpu=True)
    pts0, pts1, n_corr, K0, K1, kdt, rig, B, T, maxN, dev = _chk_rig(pts0, pts1, n_corr, K0, K1_multi, rig_T, "rig_emat_stage2")
    R1 = _chk(stage1["R"], torch.float64, "stage1 R"); t1 = _chk(stage1["t"], torch.float64, "stage1 t")
    n1 = _chk(stage1["n_inliers"], torch.int32, "stage1 n_inliers"); s1 = _chk(stage1["status"], torch.int32, "stage1 status")
    m1 = _chk(stage1["mask"], torch.uint8, "stage1 mask")
    if R1.numel() != B * T * 9 or t1.numel() != B * T * 3 or n1.numel() != B * T or s1.numel() != B * T or m1.numel() != B * T * maxN:
        raise ValueError("rig_emat_stage2: stage 1's outputs must hold one row per frame of pts0 [B,T,maxN,2]")
    ws = torch.empty(max(int(lib.mfr_rig_emat_workspace_bytes(B, T, maxN)), 256), dtype=torch.uint8, device=dev)
    R, t, ni, st = _pose_out(B, dev)
    mask = torch.empty(B, T, maxN, dtype=torch.uint8, device=dev) if want_mask else None
    hc = bh = None
    if diagnostics:
        hc, bh = torch.full((B, max(T * (T - 1), 1)), -1, dtype=torch.int32, device=dev), _i32(dev, B)
    _lib.call("mfr_rig_emat_solve", pts0, pts1, n_corr, B, T, maxN, K0, K1, kdt, rig, float(pix_thr), R1, t1, n1, s1, m1, ws, ws.numel(),
              R, t, ni, st, mask, hc, bh)
    out = dict(R=R, t=t, n_inliers=ni, status=st)
    if want_mask:
        out["mask"] = mask
    if diagnostics:
        out.update(hyp_counts=hc, best_hyp=bh)
    return out


class RigEssentialBatchSolver(_Workspace):
    """One METRIC pose (reference -> LAST window frame) for a rig of T query frames per sample without any depth map: the single-frame
    essential-matrix solver per frame, then the rig's baselines fix rotation, scale and inlier set (csrc/emat_rig.hip), one C-ABI call, no
    host synchronisation between the stages.  pts0 / pts1 [B,T,maxN,2] f32, n_corr [B,T] i32, K0 [B,3,3], K1_multi [B,T,3,3], rig_T
    [B,T,4,4] f64, pair_ids [B].  With T = 1 the result is EssentialBatchSolver's (unit translation).  Options as EssentialBatchSolver."""

    def __init__(self, pix_thr=2.0, confidence=0.9999, seed=0, max_iters=1000, score="magsac", max_thr_ratio=1.0):
        self.stage1 = EssentialBatchSolver(pix_thr, confidence, seed, max_iters, score, max_thr_ratio)

    def __call__(self, pts0, pts1, n_corr, K0, K1_multi, rig_T, pair_ids, want_mask=False, diagnostics=False):
        lib = _lib.load(require_gpu=True)
        s1 = self.stage1
        pts0, pts1, n_corr, K0, K1, kdt, rig, B, T, maxN, dev = _chk_rig(pts0, pts1, n_corr, K0, K1_multi, rig_T, "RigEssentialBatchSolver")
        pair_ids = _chk(pair_ids, torch.int64, "pair_ids")
        if tuple(pair_ids.shape) != (B,):
            raise ValueError("RigEssentialBatchSolver: pair_ids [B] must match pts0 [B,T,maxN,2]")
        ws = self._ws(lib.mfr_rig_emat_batch_workspace_bytes(B, T, maxN, s1.max_iters), dev)
        lut = s1._table(dev) if s1.score == 0 else None
        R, t, ni, st = _pose_out(B, dev)
        mask = torch.empty(B, T, maxN, dtype=torch.uint8, device=dev) if want_mask else None
        hc = bh = None
        if diagnostics:
            hc, bh = torch.full((B, max(T * (T - 1), 1)), -1, dtype=torch.int32, device=dev), _i32(dev, B)
        _lib.call("mfr_rig_emat_solve_batch", pts0, pts1, n_corr, B, T, maxN, K0, K1, kdt, rig, s1.pix_thr, s1.confidence, s1.max_iters, s1.seed,
                  pair_ids, s1.score, lut, MAGSAC_LUT_M, s1.max_thr_ratio, ws, ws.numel(), R, t, ni, st, mask, hc, bh)
        out = dict(R=R, t=t, n_inliers=ni, status=st)
        if want_mask:
            out["mask"] = mask
        if diagnostics:
            out.update(hyp_counts=hc, best_hyp=bh)
        return out


class ProcrustesIcpRefine(_Workspace):
    """PROCRUSTES.REFINE (pose_solver.py:290-319): whole-cloud point-to-point ICP from the RANSAC transform, for a batch of
    pairs (csrc/procrustes_icp.hip).  R [B,3,3], t [B,3] f64 are refined IN PLACE; returns n_inliers / fitness / rmse / iters."""

    def __init__(self, max_corr_dist=0.05, rel_fitness=1e-4, rel_rmse=1e-4, max_iter=30):
        self.max_corr_dist, self.rel_fitness, self.rel_rmse = float(max_corr_dist), float(rel_fitness), float(rel_rmse)
        self.max_iter = int(max_iter)

    def __call__(self, depth0, depth1, K0, K1, R, t, status=None):
        lib = _lib.load(require_gpu=True)
        depth0 = _chk(depth0, torch.float32, "depth0"); depth1 = _chk(depth1, torch.float32, "depth1")
        K0, K1, kdt = _chk_K(K0, K1)
        R = _chk(R, torch.float64, "R"); t = _chk(t, torch.float64, "t")
        if status is not None:
            status = _chk(status, torch.int32, "status")
        B, H, W = depth0.shape
        dev = depth0.device
        ws = self._ws(lib.mfr_procrustes_icp_workspace_bytes(B, H, W), dev)
        ni, it = _i32(dev, B), _i32(dev, B)
        fit = torch.empty(B, dtype=torch.float64, device=dev); rm = torch.empty(B, dtype=torch.float64, device=dev)
        _lib.call("mfr_procrustes_icp_refine", depth0, depth1, B, H, W, K0, K1, kdt, self.max_corr_dist, self.rel_fitness, self.rel_rmse,
                  self.max_iter, status, ws, ws.numel(), R, t, ni, fit, rm, it)
        return dict(R=R, t=t, n_inliers=ni, fitness=fit, rmse=rm, iters=it)


class ScaleFromDepthBatch(_Workspace):
    """EssentialMatrixMetricSolver's own part (pose_solver.py:137-172) for a batch of pairs."""

    def __init__(self, scale_thr=0.1):
        self.scale_thr = float(scale_thr)

    def __call__(self, pts0, pts1, emat_mask, n_corr, depth0, depth1, K0, K1, R, t, in_status=None):
        lib = _lib.load(require_gpu=True)
        pts0, pts1, n_corr, B, maxN, dev = _chk_corr(pts0, pts1, n_corr)
        depth0 = _chk(depth0, torch.float32, "depth0"); depth1 = _chk(depth1, torch.float32, "depth1")
        K0, K1, kdt = _chk_K(K0, K1)
        R = _chk(R, torch.float64, "R"); t = _chk(t, torch.float64, "t")
        if emat_mask is not None:
            emat_mask = _chk(emat_mask, torch.uint8, "emat_mask")
        if in_status is not None:
            in_status = _chk(in_status, torch.int32, "in_status")
        _, H, W = depth0.shape
        ws = self._ws(lib.mfr_scale_workspace_bytes(B, maxN), dev)
        tm = torch.empty(B, 3, dtype=torch.float64, device=dev)
        bs = torch.empty(B, dtype=torch.float64, device=dev)
        ni, st = _i32(dev, B), _i32(dev, B)
        _lib.call("mfr_scale_from_depth_batch", pts0, pts1, emat_mask, n_corr, B, maxN, depth0, depth1, H, W, K0, K1, kdt, R, t, in_status,
                  self.scale_thr, ws, ws.numel(), tm, bs, ni, st)
        return dict(t_metric=tm, best_scale=bs, n_inliers=ni, status=st)


def test_f64_ops(a, b, c):
    _lib.load(require_gpu=True)
    a = _chk(a, torch.float64, "a"); b = _chk(b, torch.float64, "b"); c = _chk(c, torch.float64, "c")
    out = torch.empty(a.numel(), 3, dtype=torch.float64, device=a.device)
    _lib.call("mfr_test_f64_ops", a, b, c, a.numel(), out)
    return out


def test_sample(seed, pair_ids, iters, n, k):
    _lib.load(require_gpu=True)
    pair_ids = _chk(pair_ids, torch.int64, "pair_ids")
    B = pair_ids.numel()
    out = torch.empty(B, iters, k, dtype=torch.int32, device=pair_ids.device)
    _lib.call("mfr_test_sample", int(seed), pair_ids, B, iters, n, k, out)
    return out


def test_replay_counts(counts, n, conf, model_points):
    """ransac_replay_counts (csrc/solver_dev.h) alone: counts [B,max_iters] i32 -> [B,3] i32 (best, bit, run).  A test hook the public
    header does not declare, so _lib binds no signature for it: every argument is converted here (int status returned, ctypes' default)."""
    import ctypes as C
    lib = _lib.load(require_gpu=True)
    counts = _chk(counts, torch.int32, "counts")
    B, max_iters = counts.shape
    out = _i32(counts.device, B, 3)
    vp = C.c_void_p
    _lib.check(lib.mfr_test_replay_counts(vp(_lib.ptr(counts)), C.c_int(B), C.c_int(max_iters), C.c_int(int(n)), C.c_double(conf),
                                          C.c_int(int(model_points)), vp(_lib.ptr(out)), vp(_lib.stream_ptr())), "mfr_test_replay_counts")
    return out
