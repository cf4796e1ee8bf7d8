"""numpy mirror of the rig entry point of csrc/procrustes.hip (the test yardstick of mfr_rig_procrustes_solve_batch): Procrustes RANSAC for a
calibrated rig of T query frames.  Upstream has no such solver; with T = 1 and the identity rig the device solver equals
mfr_procrustes_solve_batch bit for bit (tests/test_gpu_rig_solvers.py), which the oracle pins.

Built on the oracle's procrustes_lift (one frame at a time: depth0 against its minimum, the frame's own map against its own) and
procrustes_ransac (the C twin of proc_hyp_kernel / proc_select_kernel: the same sampler, wave64-ordered error sums per 512-point tile,
best-model rule, confidence exit and re-fit), run on the pooled list.  The mirror owns
  - which correspondences are valid (the lift returns the compacted points only) -- checked against the lift's count;
  - Q' = R_A^T (Q - t_A) in rig_point_to_last's operation order: IEEE float64, one rounding per numpy ufunc, as the device without fma
    contraction;
  - the pooling in (frame, index) order, the status of a sample (all correspondences count together), and the inlier masks of the
    re-fitted model, scattered to original correspondence indices.
`margin` is the smallest |d^2 - max_dist^2| over the pooled points under the returned model, so that a test can require its inputs to be clear
of the boundary."""
import numpy as np

from oracle import oracle_lib as O

OK, TOO_FEW, BAD_DEPTH, NO_MODEL, DEGENERATE = range(5)


def rig_rows(rig_T):
    """[T,4,4] -> [T,12]: R_A row-major, then t_A (solver_ops.rig_rows)"""
    rig_T = np.asarray(rig_T, np.float64)
    return np.concatenate([rig_T[:, :3, :3].reshape(-1, 9), rig_T[:, :3, 3]], 1)


def point_to_last(A, Q):
    """rows of Q [n,3] in frame j's camera -> the last frame's camera (rig_dev.h rig_point_to_last)"""
    A = [float(v) for v in A]
    Q = np.asarray(Q, np.float64).reshape(-1, 3)
    d0, d1, d2 = Q[:, 0] - A[9], Q[:, 1] - A[10], Q[:, 2] - A[11]
    return np.stack([(A[i] * d0 + A[3 + i] * d1) + A[6 + i] * d2 for i in range(3)], 1)


def valid_rows(pts0, pts1, depth0, depth1):
    """indices of the correspondences proc_lift keeps: both pixels inside their map (np.int32 truncation) and above the map's minimum"""
    p0, p1 = np.asarray(pts0, np.float32).reshape(-1, 2), np.asarray(pts1, np.float32).reshape(-1, 2)
    H, W = depth0.shape
    keep = np.ones(len(p0), bool)
    for p, d in ((p0, np.asarray(depth0, np.float32)), (p1, np.asarray(depth1, np.float32))):
        inside = (p[:, 0] > -1.0) & (p[:, 0] < W) & (p[:, 1] > -1.0) & (p[:, 1] < H)
        u, v = np.where(inside, p[:, 0], 0).astype(np.int32), np.where(inside, p[:, 1], 0).astype(np.int32)
        keep &= inside & (d[v, u] > d.min())
    return np.flatnonzero(keep)


def dist2(R, t, P, Q):
    """dist2 of procrustes.hip over the rows of P, Q [n,3]"""
    R = [float(v) for v in np.asarray(R).reshape(9)]; t = [float(v) for v in np.asarray(t).reshape(3)]
    d = [(((R[3 * i] * P[:, 0] + R[3 * i + 1] * P[:, 1]) + R[3 * i + 2] * P[:, 2]) + t[i]) - Q[:, i] for i in range(3)]
    return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def lift(pts0, pts1, depth0, depth1, K0, K1, rig_T):
    """-> pooled P [N,3], Q' [N,3], frame [N], src [N] (original index within the frame), n_valid (list of T)"""
    T = len(pts0)
    rig = rig_rows(rig_T)
    Ps, Qs, fr, src, nv = [], [], [], [], []
    for j in range(T):
        if len(pts0[j]) == 0:
            nv.append(0)
            continue
        P, Q = O.procrustes_lift(pts0[j], pts1[j], depth0, depth1[j], K0, K1[j])
        idx = valid_rows(pts0[j], pts1[j], depth0, depth1[j])
        assert len(idx) == len(P)
        Ps.append(P); Qs.append(point_to_last(rig[j], Q)); fr.append(np.full(len(P), j)); src.append(idx); nv.append(len(P))
    cat = lambda a, w: np.concatenate(a) if a else np.zeros((0,) + w)
    return cat(Ps, (3,)), cat(Qs, (3,)), cat(fr, ()).astype(int), cat(src, ()).astype(int), nv


def rig_procrustes_solve(pts0, pts1, depth0, depth1, K0, K1, rig_T, max_dist=0.05, conf=0.999, max_iters=4096, seed=0, pair_id=0):
    """pts0 / pts1: lists of T float32 arrays [n_j,2]; depth0 [H,W], depth1 [T,H,W]; K1 [T,3,3]; rig_T [T,4,4].
    -> dict(status, R, t, n_inl, masks_orig (list of T bool arrays over original indices), n_valid, best_iter, iters_run, counts, margin, P, Q)"""
    T = len(pts0)
    P, Q, fr, src, nv = lift(pts0, pts1, depth0, depth1, K0, K1, rig_T)
    out = dict(status=OK, R=np.full((3, 3), np.nan), t=np.full(3, np.nan), n_inl=0, masks_orig=[np.zeros(len(p), bool) for p in pts0],
               n_valid=nv, best_iter=-1, iters_run=0, counts=np.full(max(int(max_iters), 1), -1, np.int32), margin=np.inf, P=P, Q=Q)
    if sum(len(p) for p in pts0) < 3:
        out["status"] = TOO_FEW
    elif len(P) < 3:
        out["status"] = BAD_DEPTH
    if out["status"] != OK:
        return out
    r = O.procrustes_ransac(P, Q, max_dist, conf, max_iters, seed, pair_id, want_counts=True)
    assert r["status"] == OK
    out.update(R=r["R"], t=r["t"], n_inl=r["n_inl"], best_iter=r["best_iter"], iters_run=r["iters_run"], counts=r["counts"])
    if r["best_iter"] >= 0:
        d = dist2(r["R"], r["t"], P, Q)
        thr2 = max_dist * max_dist
        inl = d < thr2
        assert int(inl.sum()) == r["n_inl"]
        out["margin"] = float(np.abs(d - thr2).min())
        for j in range(T):
            out["masks_orig"][j][src[(fr == j) & inl]] = True
    return out
