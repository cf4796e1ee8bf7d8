"""numpy mirror of csrc/emat_rig.hip, stage 2 of the essential-matrix rig solver (the test yardstick of mfr_rig_emat_solve): from the
per-frame results of the single-frame E-matrix solver (R'_j, unit u_j, status) and the rig to ONE metric pose, reference -> last frame.
Upstream has no such solver.  Stage 1 is not mirrored here: the tests feed the mirror the device's own stage-1 outputs (the single-frame
solver is pinned to the oracle by tests/test_gpu_emat_parity.py).

The mirror restates, in IEEE float64 with one rounding per operation and the device's operation order (Python floats for the 3 x 3 algebra,
numpy ufuncs over the points), everything a count or a tie depends on: the hypotheses (rotation carried to the last frame, the 3 x 3 normal
equations by cofactors, the two skip tests -- det M <= 1e-6 (tr M / 3)^3, bearing behind a frame), the composition with a frame's rig row,
E = [t/|t|]x R, the K-normalisation and threshold in K's dtype, the squared Sampson distance and the cheirality test.  So the per-hypothesis
counts and the best index are equal as integers.  The Levenberg-Marquardt refinement follows the device's schedule with numpy's summation
order: poses agree to rounding, the final inlier set exactly unless a point sits within rounding of its threshold.
`margin` is the smallest |sampson2 / thr2 - 1| over all points under the returned model (relative: thr2 is about 2e-4 in normalised units)."""
import numpy as np

import rig_pnp_ref as RP

OK, TOO_FEW, BAD_DEPTH, NO_MODEL, DEGENERATE = range(5)
DET_REL, T_FLOOR = 1e-6, 1e-12


def normalize(pts0, pts1, K0, K1):
    """[n,2] float32 pixels -> x [n,4] float64 (x0, y0, x1, y1), in K's dtype (emat_dev.h emat_normalize); a mixed pair is float64"""
    p0, p1 = np.asarray(pts0, np.float32).reshape(-1, 2), np.asarray(pts1, np.float32).reshape(-1, 2)
    if K0.dtype == np.float32 and K1.dtype == np.float32:
        c = [(p0[:, 0] - K0[0, 2]) / K0[0, 0], (p0[:, 1] - K0[1, 2]) / K0[1, 1], (p1[:, 0] - K1[0, 2]) / K1[0, 0], (p1[:, 1] - K1[1, 2]) / K1[1, 1]]
        assert all(v.dtype == np.float32 for v in c)
    else:
        K0, K1 = K0.astype(np.float64), K1.astype(np.float64)
        p0, p1 = p0.astype(np.float64), p1.astype(np.float64)
        c = [(p0[:, 0] - K0[0, 2]) / K0[0, 0], (p0[:, 1] - K0[1, 2]) / K0[1, 1], (p1[:, 0] - K1[0, 2]) / K1[0, 0], (p1[:, 1] - K1[1, 2]) / K1[1, 1]]
    return np.stack(c, 1).astype(np.float64)


def thr2_of(K0, K1, pix_thr):
    if K0.dtype == np.float32 and K1.dtype == np.float32:
        m = (((K0[0, 0] + K1[1, 1]) + K0[1, 1]) + K1[0, 0]) / np.float32(4.0)
        thr = pix_thr / float(m)
    else:
        m = (((float(K0[0, 0]) + float(K1[1, 1])) + float(K0[1, 1])) + float(K1[0, 0])) / 4.0
        thr = pix_thr / m
    return thr * thr


def skew_mul(t, R):
    E = [0.0] * 9
    for j in range(3):
        E[j] = t[1] * R[6 + j] - t[2] * R[3 + j]
        E[3 + j] = t[2] * R[j] - t[0] * R[6 + j]
        E[6 + j] = t[0] * R[3 + j] - t[1] * R[j]
    return E


def sampson2(E, x):
    a, b, c, d = x[:, 0], x[:, 1], x[:, 2], x[:, 3]
    Ex0, Ex1, Ex2 = (E[0] * a + E[1] * b) + E[2], (E[3] * a + E[4] * b) + E[5], (E[6] * a + E[7] * b) + E[8]
    Et0, Et1 = (E[0] * c + E[3] * d) + E[6], (E[1] * c + E[4] * d) + E[7]
    num = (c * Ex0 + d * Ex1) + Ex2
    den = ((Ex0 * Ex0 + Ex1 * Ex1) + Et0 * Et0) + Et1 * Et1
    with np.errstate(all="ignore"):
        return (num * num) / den


def cheirality(R, t, x):
    a, b, c, d = x[:, 0], x[:, 1], x[:, 2], x[:, 3]
    p = [(R[0] * a + R[1] * b) + R[2], (R[3] * a + R[4] * b) + R[5], (R[6] * a + R[7] * b) + R[8]]
    q = [c, d, np.ones_like(c)]
    pp, qq = (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2], (q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]
    pq = (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2]
    pt, qt = (p[0] * t[0] + p[1] * t[1]) + p[2] * t[2], (q[0] * t[0] + q[1] * t[1]) + q[2] * t[2]
    det = pp * qq - pq * pq
    with np.errstate(all="ignore"):
        ok = det > 1e-18 * pp * qq
        l0, l1 = (pq * qt - qq * pt) / det, (pp * qt - pq * pt) / det
        return ok & (l0 > 0.0) & (l1 > 0.0)


def hypothesis(rig, R1, t1, fa, fb, which):
    """erig_hypothesis -> (R [9], t [3]) or None when skipped"""
    m = fb if which else fa
    R, _ = RP.to_last(rig[m], R1[m], [0.0, 0.0, 0.0])
    M, c = [0.0] * 9, [0.0] * 3
    for f in (fa, fb):
        A, u = [float(v) for v in rig[f]], [float(v) for v in np.asarray(t1[f]).reshape(3)]
        P = [(1.0 if i == j else 0.0) - u[i] * u[j] for i in range(3) for j in range(3)]
        PA = [(P[3 * i] * A[j] + P[3 * i + 1] * A[3 + j]) + P[3 * i + 2] * A[6 + j] for i in range(3) for j in range(3)]
        Pt = [(P[3 * i] * A[9] + P[3 * i + 1] * A[10]) + P[3 * i + 2] * A[11] for i in range(3)]
        for i in range(3):
            for j in range(3):
                M[3 * i + j] = M[3 * i + j] + ((A[i] * PA[j] + A[3 + i] * PA[3 + j]) + A[6 + i] * PA[6 + j])
            c[i] = c[i] + ((A[i] * Pt[0] + A[3 + i] * Pt[1]) + A[6 + i] * Pt[2])
    C0, C1, C2 = M[4] * M[8] - M[5] * M[7], M[5] * M[6] - M[3] * M[8], M[3] * M[7] - M[4] * M[6]
    det = (M[0] * C0 + M[1] * C1) + M[2] * C2
    tr3 = ((M[0] + M[4]) + M[8]) / 3.0
    if not det > DET_REL * ((tr3 * tr3) * tr3):
        return None
    inv = [C0, M[2] * M[7] - M[1] * M[8], M[1] * M[5] - M[2] * M[4],
           C1, M[0] * M[8] - M[2] * M[6], M[2] * M[3] - M[0] * M[5],
           C2, M[1] * M[6] - M[0] * M[7], M[0] * M[4] - M[1] * M[3]]
    b = [-c[0], -c[1], -c[2]]
    t = [((inv[3 * i] * b[0] + inv[3 * i + 1] * b[1]) + inv[3 * i + 2] * b[2]) / det for i in range(3)]
    for f in (fa, fb):
        A, u = [float(v) for v in rig[f]], [float(v) for v in np.asarray(t1[f]).reshape(3)]
        y = [((A[3 * i] * t[0] + A[3 * i + 1] * t[1]) + A[3 * i + 2] * t[2]) + A[9 + i] for i in range(3)]
        if not (y[0] * u[0] + y[1] * u[1]) + y[2] * u[2] > 0.0:
            return None
    return R, t


def frame_model(A, R, t):
    """erig_frame_model -> (E, Rc, tn) or None"""
    Rc, tc = RP.compose(A, R, t)
    nt = float(np.sqrt((tc[0] * tc[0] + tc[1] * tc[1]) + tc[2] * tc[2]))
    if not nt >= T_FLOOR:
        return None
    tn = [tc[0] / nt, tc[1] / nt, tc[2] / nt]
    return skew_mul(tn, Rc), Rc, tn


def score(xs, thr2s, rig, R, t):
    """per-frame inlier masks of the model and the smallest |sampson2 / thr2 - 1|"""
    masks, margin = [], np.inf
    for j, x in enumerate(xs):
        fm = frame_model(rig[j], R, t) if len(x) else None
        if fm is None:
            masks.append(np.zeros(len(x), bool))
            continue
        s2 = sampson2(fm[0], x)
        masks.append((s2 < thr2s[j]) & cheirality(fm[1], fm[2], x))
        fin = np.abs(s2[np.isfinite(s2)] / thr2s[j] - 1.0)
        if len(fin):
            margin = min(margin, float(fin.min()))
    return masks, margin


# ---------------------------------------------------------------- Levenberg-Marquardt (erig_lm)
def _lm_terms(x, RA, tA, R, t, jac=False):
    """x [m,4], per-point rig rows RA [m,3,3], tA [m,3] -> cost (, J^T J, -J^T r)"""
    Rc = np.einsum("mij,jk->mik", RA, R)
    tc = RA @ t + tA
    E = np.cross(tc[:, :, None], Rc, axisa=1, axisb=1, axisc=1)                  # [t]x R, column by column
    p = np.concatenate([x[:, :2], np.ones((len(x), 1))], 1); q = np.concatenate([x[:, 2:], np.ones((len(x), 1))], 1)
    Ex = np.einsum("mij,mj->mi", E, p); Etq = np.einsum("mji,mj->mi", E, q)
    num = np.einsum("mi,mi->m", q, Ex)
    den = Ex[:, 0] ** 2 + Ex[:, 1] ** 2 + Etq[:, 0] ** 2 + Etq[:, 1] ** 2
    with np.errstate(all="ignore"):
        w = 1.0 / np.sqrt(den)
        r = num * w
        cost = float(np.sum(num * num / den))
    if not jac:
        return cost
    txq = np.cross(tc, q)
    u = -np.einsum("mji,mj->mi", Rc, txq)
    Rp = np.einsum("mij,mj->mi", Rc, p)
    Jr = np.cross(p, u) * w[:, None]
    Jt = np.einsum("mr,mrc->mc", np.cross(Rp, q) * w[:, None], RA)
    J = np.concatenate([Jr, Jt], 1)
    return cost, J.T @ J, -(J.T @ r)


def lm(x, RA, tA, R, t, max_iter=20):
    R, t = np.array(R, np.float64).reshape(3, 3), np.array(t, np.float64).reshape(3)
    lam = 1e-3
    cost = _lm_terms(x, RA, tA, R, t)
    if not (cost == cost) or not (cost < 1e300):
        return R, t
    for _ in range(max_iter):
        _, H, g = _lm_terms(x, RA, tA, R, t, jac=True)
        H = H + lam * np.diag(np.diag(H))
        try:
            with np.errstate(all="ignore"):
                if not np.isfinite(H).all():
                    raise np.linalg.LinAlgError
                L = np.linalg.cholesky(H)
                dl = np.linalg.solve(L.T, np.linalg.solve(L, g))
        except np.linalg.LinAlgError:
            lam *= 10.0
            if lam > 1e12:
                break
            continue
        Rn, tn = RP._quat_right_update(R, dl[:3]), t + dl[3:]
        cn = _lm_terms(x, RA, tA, Rn, tn)
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
    return R, t


# ---------------------------------------------------------------- stage 2
def rig_emat_stage2(pts0, pts1, K0, K1, rig_T, R1, t1, n1, st1, mask1, pix_thr=2.0):
    """pts0 / pts1: lists of T float32 arrays [n_j,2]; K0 [3,3], K1 [T,3,3]; rig_T [T,4,4]; stage 1 per frame: R1 [T,3,3], t1 [T,3], n1 [T],
    st1 [T], mask1: list of T bool arrays.  -> dict(status, R, t, n_inl, masks, hyp_counts [T (T - 1)], best_hyp, margin)"""
    T = len(pts0)
    rig = RP.rig_rows(rig_T)
    K0, K1 = np.asarray(K0), np.asarray(K1)
    NH = T * (T - 1)
    out = dict(status=OK, R=np.full((3, 3), np.nan), t=np.full(3, np.nan), n_inl=0, masks=[np.zeros(len(p), bool) for p in pts0],
               hyp_counts=np.full(max(NH, 1), -1, np.int32), best_hyp=-1, margin=np.inf)
    if T == 1:
        out.update(status=int(st1[0]), R=np.array(R1[0], np.float64).reshape(3, 3), t=np.array(t1[0], np.float64).reshape(3), n_inl=int(n1[0]),
                   masks=[np.asarray(mask1[0], bool)])
        return out
    usable = [j for j in range(T) if int(st1[j]) == OK]
    if len(usable) < 2:
        out["status"] = int(st1[0]) if (not usable and len(set(int(s) for s in st1)) == 1) else NO_MODEL
        return out
    xs = [normalize(pts0[j], pts1[j], K0, K1[j]) for j in range(T)]
    thr2s = [thr2_of(K0, K1[j], pix_thr) for j in range(T)]
    R1 = [np.asarray(R1[j], np.float64).reshape(9) for j in range(T)]
    models, h = {}, 0
    for a in range(len(usable)):
        for b in range(a + 1, len(usable)):
            for which in (0, 1):
                hyp = hypothesis(rig, R1, t1, usable[a], usable[b], which)
                if hyp is not None:
                    models[h] = hyp
                    out["hyp_counts"][h] = int(sum(m.sum() for m in score(xs, thr2s, rig, *hyp)[0]))
                h += 1
    if not models:
        out["status"] = NO_MODEL
        return out
    bh = int(np.argmax(out["hyp_counts"]))                                      # the first maximum
    out["best_hyp"] = bh
    R, t = models[bh]
    masks, _ = score(xs, thr2s, rig, R, t)
    R, t = np.array(R).reshape(3, 3), np.array(t)
    if sum(int(m.sum()) for m in masks) >= 6:
        fr = np.concatenate([np.full(int(masks[j].sum()), j) for j in range(T)]).astype(int)
        x = np.concatenate([xs[j][masks[j]] for j in range(T)])
        R, t = lm(x, rig[fr, :9].reshape(-1, 3, 3), rig[fr, 9:], R, t)
    if not (np.isfinite(R).all() and np.isfinite(t).all()) or np.sqrt(t @ t) > 1000.0:
        out["status"] = DEGENERATE
        return out
    masks, out["margin"] = score(xs, thr2s, rig, [float(v) for v in R.reshape(9)], [float(v) for v in t])
    out.update(R=R, t=t, n_inl=int(sum(m.sum() for m in masks)), masks=masks)
    return out
