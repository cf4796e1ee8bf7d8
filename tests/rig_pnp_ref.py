"""numpy mirror of csrc/pnp_rig.hip (the test yardstick of mfr_rig_pnp_ransac / mfr_rig_pnp_solve_batch): PnP RANSAC for a calibrated rig of
T query frames.  Upstream has no such solver, so there is nothing else to compare against; with T = 1 and the identity rig the device
solver equals mfr_pnp_ransac bit for bit (tests/test_gpu_rig_pnp.py), which the oracle pins.

Built on the oracle's p3p, sample_distinct, philox, update_num_iters and pnp_lift.  The mirror owns
  - the frame draw (word 0 of Philox at counter (it, 0x80000000, lo, hi of pair_id * T), e = (w * n_eligible) >> 32);
  - the composition of (R, t) with a frame's (R_A, t_A) and the pooled scoring: IEEE float64, + - * / only, in the device's operation order
    (numpy's elementwise ufuncs do one rounding per operation, as the device does without fma contraction), so counts and inlier masks are
    equal as integers unless a point sits within rounding of the threshold;
  - the replay of OpenCV's adaptive iteration cap and the Levenberg-Marquardt refinement (the device's sums run over a wavefront butterfly,
    the mirror's in numpy order: poses agree to rounding, not to the bit).
`margin` in the result is the smallest |err^2 - thr^2| the selected model met, so that a test can require its inputs to be clear of the boundary."""
import numpy as np

from oracle import oracle_lib as O

OK, TOO_FEW, BAD_DEPTH, NO_MODEL, DEGENERATE = range(5)
FRAME_CTR = 0x80000000


def rig_rows(rig_T):
    """[T,4,4] -> [T,12]: R_A row-major, then t_A (solver_ops.rig_rows)"""
    rig_T = np.asarray(rig_T, np.float64)
    return np.concatenate([rig_T[:, :3, :3].reshape(-1, 9), rig_T[:, :3, 3]], 1)


def kd_of(K):
    K = np.asarray(K, np.float64).reshape(3, 3)
    return [float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])]


def compose(A, R, t):
    """Rc = R_A R, tc = R_A t + t_A (rig_compose): Python floats, one rounding per operation"""
    A = [float(v) for v in A]; R = [float(v) for v in np.asarray(R).reshape(9)]; t = [float(v) for v in np.asarray(t).reshape(3)]
    Rc = [(A[3 * i] * R[c] + A[3 * i + 1] * R[3 + c]) + A[3 * i + 2] * R[6 + c] for i in range(3) for c in range(3)]
    tc = [((A[3 * i] * t[0] + A[3 * i + 1] * t[1]) + A[3 * i + 2] * t[2]) + A[9 + i] for i in range(3)]
    return Rc, tc


def to_last(A, Rp, tp):
    """R = R_A^T R', t = R_A^T (t' - t_A) (rig_to_last)"""
    A = [float(v) for v in A]; Rp = [float(v) for v in np.asarray(Rp).reshape(9)]; tp = [float(v) for v in np.asarray(tp).reshape(3)]
    d = [tp[0] - A[9], tp[1] - A[10], tp[2] - A[11]]
    R = [(A[i] * Rp[c] + A[3 + i] * Rp[3 + c]) + A[6 + i] * Rp[6 + c] for i in range(3) for c in range(3)]
    t = [(A[i] * d[0] + A[3 + i] * d[1]) + A[6 + i] * d[2] for i in range(3)]
    return R, t


def err2(R, t, X, x, Kd):
    """reproj_err2 of geom_dev.h over the rows of X [n,3], x [n,2]"""
    X = np.asarray(X, np.float64).reshape(-1, 3); x = np.asarray(x, np.float64).reshape(-1, 2)
    Y0 = ((R[0] * X[:, 0] + R[1] * X[:, 1]) + R[2] * X[:, 2]) + t[0]
    Y1 = ((R[3] * X[:, 0] + R[4] * X[:, 1]) + R[5] * X[:, 2]) + t[1]
    Y2 = ((R[6] * X[:, 0] + R[7] * X[:, 1]) + R[8] * X[:, 2]) + t[2]
    with np.errstate(all="ignore"):
        iz = np.where(Y2 != 0.0, 1.0 / np.where(Y2 != 0.0, Y2, 1.0), 1.0)
        du = (Kd[0] * (Y0 * iz) + Kd[2]) - x[:, 0]
        dv = (Kd[1] * (Y1 * iz) + Kd[3]) - x[:, 1]
        return du * du + dv * dv


def pnp_hypothesis(xyz, obs, s, Kd):
    """geom_dev.h pnp_hypothesis: P3P on samples 0..2, the solution with the smallest error on sample 3 -> (R [9], t [3]) or None"""
    X = np.asarray(xyz, np.float64)[list(s[:3])]
    f = np.zeros((3, 3))
    for k in range(3):
        o = obs[s[k]]
        bx, by = (float(o[0]) - Kd[2]) / Kd[0], (float(o[1]) - Kd[3]) / Kd[1]
        nn = float(np.sqrt((bx * bx + by * by) + 1.0))
        f[k] = [bx / nn, by / nn, 1.0 / nn]
    Rs, ts = O.p3p(X, f)
    best, beste = None, 0.0
    for i in range(len(Rs)):
        e = float(err2(Rs[i].reshape(9), ts[i], xyz[s[3]], obs[s[3]], Kd)[0])
        if not e == e:
            continue
        if best is None or e < beste:
            best, beste = i, e
    if best is None:
        return None
    return [float(v) for v in Rs[best].reshape(9)], [float(v) for v in ts[best]]


def draw_frame(seed, pair_id, T, it, eligible):
    """the frame hypothesis `it` samples from; no random word when only one frame is eligible"""
    if len(eligible) == 1:
        return eligible[0]
    id0 = (int(pair_id) * T) & 0xFFFFFFFFFFFFFFFF
    w = O.philox([it, FRAME_CTR, id0 & 0xFFFFFFFF, id0 >> 32], seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return eligible[(int(w[0]) * len(eligible)) >> 32]


def hypothesis(xyz, obs, Kds, rig, seed, pair_id, it, eligible):
    T = len(xyz)
    j = draw_frame(seed, pair_id, T, it, eligible)
    s = O.sample_distinct(seed, (int(pair_id) * T + j) & 0xFFFFFFFFFFFFFFFF, it, len(xyz[j]), 4)
    h = pnp_hypothesis(xyz[j], obs[j], s, Kds[j])
    return None if h is None else to_last(rig[j], *h)


def score(xyz, obs, Kds, rig, R, t, thr2, fixed=-1):
    """per-frame inlier masks of the model (R, t) and the smallest |err^2 - thr^2|; frame `fixed`: all of its points are inliers"""
    masks, margin = [], np.inf
    for j in range(len(xyz)):
        if len(xyz[j]) == 0:
            masks.append(np.zeros(0, bool))
            continue
        if j == fixed:
            masks.append(np.ones(len(xyz[j]), bool))
            continue
        Rc, tc = compose(rig[j], R, t)
        e = err2(Rc, tc, xyz[j], obs[j], Kds[j])
        masks.append(e <= thr2)
        fin = np.abs(e[np.isfinite(e)] - thr2)
        if len(fin):
            margin = min(margin, float(fin.min()))
    return masks, margin


# ---------------------------------------------------------------- Levenberg-Marquardt (pnp_dev.h pnp_lm with the rig as the camera)
def _quat_right_update(R, dw):
    hx, hy, hz = 0.5 * dw[0], 0.5 * dw[1], 0.5 * dw[2]
    nn = np.sqrt(((hx * hx + hy * hy) + hz * hz) + 1.0)
    w, x, y, z = 1.0 / nn, hx / nn, hy / nn, hz / nn
    Q = np.array([[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
                  [2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)],
                  [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]])
    return R @ Q


def _residuals(P, x, RA, tA, Kp, R, t, jac=False):
    """P [m,3], x [m,2], per-point RA [m,3,3], tA [m,3], Kp [m,4] -> cost (, J^T J, J^T r)"""
    Yl = P @ R.T + t
    Y = np.einsum("mij,mj->mi", RA, Yl) + tA
    with np.errstate(all="ignore"):
        iz = np.where(Y[:, 2] != 0.0, 1.0 / np.where(Y[:, 2] != 0.0, Y[:, 2], 1.0), 1.0)
        xn, yn = Y[:, 0] * iz, Y[:, 1] * iz
        ru = (Kp[:, 0] * xn + Kp[:, 2]) - x[:, 0]
        rv = (Kp[:, 1] * yn + Kp[:, 3]) - x[:, 1]
        cost = float(np.sum(ru * ru + rv * rv))
    if not jac:
        return cost
    m = len(P)
    skew = np.zeros((m, 3, 3))
    skew[:, 0, 1], skew[:, 0, 2] = -P[:, 2], P[:, 1]
    skew[:, 1, 0], skew[:, 1, 2] = P[:, 2], -P[:, 0]
    skew[:, 2, 0], skew[:, 2, 1] = -P[:, 1], P[:, 0]
    G = np.concatenate([-(R @ skew), np.tile(np.eye(3), (m, 1, 1))], 2)        # d(R Q(dw) P + t + dt): [R [a0 a1 a2] | I], a_k as in pnp_lm
    G = np.einsum("mij,mjk->mik", RA, G)
    Ju = (Kp[:, 0] * iz)[:, None] * G[:, 0] + (-(Kp[:, 0] * xn) * iz)[:, None] * G[:, 2]
    Jv = (Kp[:, 1] * iz)[:, None] * G[:, 1] + (-(Kp[:, 1] * yn) * iz)[:, None] * G[:, 2]
    Hm = Ju.T @ Ju + Jv.T @ Jv
    g = -(Ju.T @ ru + Jv.T @ rv)
    return cost, Hm, g


def lm(P, x, RA, tA, Kp, R, t, max_iter=20):
    """-> (rc, R, t): rc = -1 when the starting cost is not finite"""
    R, t = np.array(R, np.float64).reshape(3, 3), np.array(t, np.float64).reshape(3)
    lam = 1e-3
    cost = _residuals(P, x, RA, tA, Kp, R, t)
    if not (cost == cost) or not (cost < 1e300):
        return -1, R, t
    for _ in range(max_iter):
        _, Hm, g = _residuals(P, x, RA, tA, Kp, R, t, jac=True)
        Hm = Hm + lam * np.diag(np.diag(Hm))
        try:
            with np.errstate(all="ignore"):
                if not np.isfinite(Hm).all():
                    raise np.linalg.LinAlgError
                L = np.linalg.cholesky(Hm)
                dl = np.linalg.solve(L.T, np.linalg.solve(L, g))
        except np.linalg.LinAlgError:
            lam *= 10.0
            if lam > 1e12:
                break
            continue
        Rn, tn = _quat_right_update(R, dl[:3]), t + dl[3:]
        cn = _residuals(P, x, RA, tA, Kp, Rn, tn)
        if cn < cost:
            R, t = Rn, tn
            lam = max(lam * 0.1, 1e-12)
            done = (cost - cn) <= 1e-14 * cost
            cost = cn
            if done:
                break
        else:
            lam *= 10.0
            if lam > 1e12:
                break
        if np.abs(dl).max() < 1e-13:
            break
    return 0, R, t


def _is_rotation(R):
    if not np.isfinite(R).all():
        return False
    return bool((np.abs(R.T @ R - np.eye(3)) <= 1e-12).all() and np.linalg.det(R) > 0.0)


# ---------------------------------------------------------------- the solver on lifted rows
def rig_pnp_ransac(xyz, obs, K1, rig, max_iters=1000, thr=3.0, conf=0.9999, seed=0, pair_id=0, all_counts=True, pre_status=OK):
    """xyz / obs: lists of T arrays [n_j,3] / [n_j,2] (lifted points of frame j), K1 [T,3,3], rig [T,12].
    all_counts=False stops scoring where the sequential loop would (the replay's cap): enough for the pose, not for comparing counts.
    -> dict(status, R, t, n_inl, masks (list of T bool arrays), best_iter, iters_run, counts, margin)"""
    T = len(xyz)
    xyz = [np.asarray(a, np.float64).reshape(-1, 3) for a in xyz]; obs = [np.asarray(a, np.float64).reshape(-1, 2) for a in obs]
    rig = np.asarray(rig, np.float64).reshape(T, 12)
    Kds = [kd_of(K1[j]) for j in range(T)]
    ns = [len(a) for a in xyz]
    N, thr2 = sum(ns), thr * thr
    max_iters = max(int(max_iters), 1)
    out = dict(status=pre_status, R=np.full((3, 3), np.nan), t=np.full(3, np.nan), n_inl=0, masks=[np.zeros(n, bool) for n in ns],
               best_iter=-1, iters_run=0, counts=np.full(max_iters, -1, np.int32), margin=np.inf)
    if out["status"] == OK and not any(n >= 4 for n in ns):
        out["status"] = TOO_FEW
    if out["status"] != OK:
        return out
    eligible = [j for j in range(T) if ns[j] >= 5]
    fixed, model = -1, None
    if not eligible:
        fixed = next(j for j in range(T) if ns[j] >= 4)
        h = pnp_hypothesis(xyz[fixed], obs[fixed], [0, 1, 2, 3], Kds[fixed])
        if h is not None:
            model = to_last(rig[fixed], *h)
            out["best_iter"], out["iters_run"] = 0, 1
    else:
        counts = out["counts"]
        niters, best, bit, it = max_iters, 3, -1, 0
        while it < (max_iters if all_counts else niters):
            h = hypothesis(xyz, obs, Kds, rig, seed, pair_id, it, eligible)
            c = 0 if h is None else int(sum(m.sum() for m in score(xyz, obs, Kds, rig, h[0], h[1], thr2)[0]))
            counts[it] = c
            if it < niters and c > best:
                best, bit = c, it
                niters = O.update_num_iters(conf, (N - best) / N, 4, niters)
            it += 1
        out["best_iter"], out["iters_run"] = bit, max(niters, bit + 1)
        if bit >= 0:
            model = hypothesis(xyz, obs, Kds, rig, seed, pair_id, bit, eligible)
    if model is None:
        out["status"] = NO_MODEL
        return out
    masks, out["margin"] = score(xyz, obs, Kds, rig, model[0], model[1], thr2, fixed)
    R, t = np.array(model[0]).reshape(3, 3), np.array(model[1])
    m = int(sum(k.sum() for k in masks))
    if N > 4:
        sel = [np.flatnonzero(k) for k in masks]
        P = np.concatenate([xyz[j][sel[j]] for j in range(T)]); x = np.concatenate([obs[j][sel[j]] for j in range(T)])
        fr = np.concatenate([np.full(len(sel[j]), j) for j in range(T)]).astype(int)
        RA, tA, Kp = rig[fr, :9].reshape(-1, 3, 3), rig[fr, 9:], np.array(Kds)[fr]
        rc, R, t = lm(P, x, RA, tA, Kp, R, t)
        if rc == 0 and m >= 6:
            rc, R, t = lm(P, x, RA, tA, Kp, R, t)
        if rc:
            out["status"] = NO_MODEL
            return out
    if not _is_rotation(R) or not np.isfinite(t).all():
        out["status"] = NO_MODEL
    elif np.sqrt(t @ t) > 1000.0:
        out["status"] = DEGENERATE
    if out["status"] == OK:
        out.update(R=R, t=t, n_inl=m, masks=masks)
    return out


def rig_pnp_solve(pts0, pts1, depth0, K0, K1, rig_T, **kw):
    """from raw correspondences (lists of T float32 arrays [n_j,2]): lift every frame against the ONE reference depth map, pre-status,
    RANSAC, masks scattered to the original correspondence indices.  kw as rig_pnp_ransac."""
    T = len(pts0)
    lifted = [O.pnp_lift(np.asarray(pts0[j], np.float32).reshape(-1, 2), np.asarray(pts1[j], np.float32).reshape(-1, 2), depth0, K0)
              if len(pts0[j]) else (np.zeros((0, 3)), np.zeros((0, 2)), np.zeros(0, np.int32)) for j in range(T)]
    pre = OK
    if not any(len(p) >= 4 for p in pts0):
        pre = TOO_FEW
    elif not any(len(l[0]) >= 4 for l in lifted):
        pre = BAD_DEPTH
    r = rig_pnp_ransac([l[0] for l in lifted], [l[1] for l in lifted], K1, rig_rows(rig_T), pre_status=pre, **kw)
    full = []
    for j in range(T):
        mk = np.zeros(len(pts0[j]), bool)
        mk[lifted[j][2][r["masks"][j]]] = True
        full.append(mk)
    r["masks_orig"], r["n_valid"] = full, [len(l[0]) for l in lifted]
    return r
