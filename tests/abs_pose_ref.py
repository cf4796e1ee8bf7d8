"""numpy restatement of csrc/abs_pose.hip (the test mirror of mfr_abs_pose_fuse): lib/utils/localize.py's pose fusion, query by query, with
the device's conventions -- inlier sets are fitted in ascending pair index, the triangulation's null vector is the smallest eigenvector of
A^T A, the LO subsets come from Philox keyed by (seed, query, LO call, iteration).  Pinned to the reference's own run by
tests/golden/ref_sevenscenes.npz (tests/test_abs_pose_ref.py)."""
import itertools

import numpy as np

OK, APPROXIMATED, NO_PAIRS, TOO_MANY, BAD_OFFSETS, ITER_CAP = 0, 1, 2, 3, 4, 16
MAX_PAIRS, WEISZFELD_CAP = 64, 256
EPS = np.finfo(np.float64).eps
TRACE = None        # tools/gen_sevenscenes_golden.py sets a dict(cos=[], cond=[], steps=[], draws=[]) to measure the fixture's margins


def quat2mat(q):
    """transforms3d.quaternions.quat2mat"""
    w, x, y, z = q
    Nq = w * w + x * x + y * y + z * z
    if Nq < EPS:
        return np.eye(3)
    s = 2.0 / Nq
    X, Y, Z = x * s, y * s, z * s
    wX, wY, wZ, xX, xY, xZ, yY, yZ, zZ = w * X, w * Y, w * Z, x * X, x * Y, x * Z, y * Y, y * Z, z * Z
    return np.array([[1.0 - (yY + zZ), xY - wZ, xZ + wY], [xY + wZ, 1.0 - (xX + zZ), yZ - wX], [xZ - wY, yZ + wX, 1.0 - (xX + yY)]])


def mat2quat(M):
    """transforms3d.quaternions.mat2quat"""
    Qxx, Qyx, Qzx, Qxy, Qyy, Qzy, Qxz, Qyz, Qzz = np.asarray(M, np.float64).flat
    K = np.array([[Qxx - Qyy - Qzz, 0, 0, 0], [Qyx + Qxy, Qyy - Qxx - Qzz, 0, 0], [Qzx + Qxz, Qzy + Qyz, Qzz - Qxx - Qyy, 0],
                  [Qyz - Qzy, Qzx - Qxz, Qxy - Qyx, Qxx + Qyy + Qzz]]) / 3.0
    if not np.isfinite(K).all():
        return np.full(4, np.nan)
    vals, vecs = np.linalg.eigh(K)
    q = vecs[[3, 0, 1, 2], np.argmax(vals)]
    if q[0] < 0:
        q = -q
    return q


def philox4x32_10(ctr, key):
    c = [int(v) & 0xFFFFFFFF for v in ctr]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k0) & 0xFFFFFFFF, p1 & 0xFFFFFFFF, ((p0 >> 32) ^ c[3] ^ k1) & 0xFFFFFFFF, p0 & 0xFFFFFFFF]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c


def lo_subset(seed, qid, call, it, base, nsub):
    """abs_pose.hip ap_subset: nsub distinct members of the ascending list `base`, as a sorted list"""
    rem, sub, nb = list(base), [], len(base)
    if TRACE is not None:
        TRACE['draws'].append((qid, call, it))
    for j in range(nsub):
        if j % 4 == 0:
            w = philox4x32_10((it, call * 4 + j // 4, qid, 0), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
        r = (w[j % 4] * (nb - j)) >> 32
        sub.append(rem.pop(r))
    return sorted(sub)


class Pair:
    """RelaPosePair.__init__ (:942-964) with AbsPose (:896-918) of the database image, float64"""

    def __init__(self, train_q, train_c, R, t):
        self.train_q, self.train_c = np.asarray(train_q, np.float64), np.asarray(train_c, np.float64)
        t = np.asarray(t, np.float64)
        self.q = mat2quat(np.asarray(R, np.float64).reshape(3, 3))
        self.r = quat2mat(self.q)
        self.rtr = quat2mat(self.train_q)
        self.p = np.hstack([self.rtr, (-self.rtr.dot(self.train_c))[:, None]])
        self.t_opt = -self.r.T.dot(t)
        self.x_te = self.t_opt[:2] / (self.t_opt[2] if self.t_opt[2] != 0 else 1)
        self.abs_q = mat2quat(self.r.dot(self.rtr))
        self.abs_c = self.train_c + self.rtr.T.dot(self.t_opt)
        self.rows = np.stack([self.x_te[0] * self.p[2] - self.p[0], self.x_te[1] * self.p[2] - self.p[1]])


def estimate(pairs, idx):
    """estimate_model (:734-756): -> (c, unnormalised mean q)"""
    idx = sorted(idx)
    A = np.concatenate([pairs[i].rows for i in idx], 0)
    q = np.sum([pairs[i].abs_q for i in idx], 0) / len(idx)
    M = A.T @ A
    if not np.isfinite(M).all():
        return np.full(3, np.nan), q
    if TRACE is not None:
        sv = np.linalg.svd(A, compute_uv=False)
        TRACE['cond'].append(sv[0] ** 2 / (sv[2] ** 2 - sv[3] ** 2))
    vals, vecs = np.linalg.eigh(M)
    X = vecs[:, np.argmin(vals)]
    with np.errstate(all='ignore'):
        return X[:3] / X[3], q


def angle_cos(c, pr):
    """the rounded cosine find_inliers thresholds, or 'zero' / 'raise' for the two special routes"""
    te = pr.rtr.dot(c - pr.train_c)
    ne, no = np.sqrt(te.dot(te)), np.sqrt(pr.t_opt.dot(pr.t_opt))
    if ne == 0.0:
        return 'zero', None
    if no == 0.0 or np.isinf(ne):
        return 'raise', None
    d = float(np.sum((pr.t_opt / no) * (te / ne)))
    return 'cos', d


def find_inliers(pairs, c, thr):
    out = []
    with np.errstate(all='ignore'):
        for i, pr in enumerate(pairs):
            kind, d = angle_cos(c, pr)
            if kind == 'zero':
                err = 0.0
            elif kind == 'raise':
                continue
            else:
                if TRACE is not None:
                    TRACE['cos'].append((d, thr))
                err = np.degrees(np.arccos(np.clip(np.rint(d * 1e4) / 1e4, -1, 1)))
                if np.isnan(err):
                    err = 0.0
            if err < thr:
                out.append(i)
    return out


def ransac_query(pairs, thr, thr_mult=1.414, lo_iters=10, seed=0, qid=0):
    """-> (status, q [4], c [3], inlier list)"""
    k = len(pairs)
    if k == 0:
        return NO_PAIRS, np.full(4, np.nan), np.full(3, np.nan), []
    if k > MAX_PAIRS:
        return TOO_MANY, np.full(4, np.nan), np.full(3, np.nan), []
    best, best_in, call = None, [], 0
    for pair in itertools.combinations(range(k), 2):
        c, q = estimate(pairs, pair)
        inl = find_inliers(pairs, c, thr)
        if len(inl) >= 2 and len(inl) > len(best_in):
            best, best_in = (c, q), inl
            m_mult = find_inliers(pairs, c, thr_mult * thr)
            pm = estimate(pairs, m_mult)
            base = find_inliers(pairs, pm[0], thr)
            cands = [best, pm]
            nsub = min(14, len(base) // 2)
            if nsub > 2:
                cands += [estimate(pairs, lo_subset(seed, qid, call, it, base, nsub)) for it in range(lo_iters)]
            loc, loc_in = None, []
            for cand in cands:
                ci = find_inliers(pairs, cand[0], thr)
                if len(ci) > len(loc_in):
                    loc, loc_in = cand, ci
            if len(loc_in) > len(best_in):
                best, best_in = loc, loc_in
            call += 1
    if best is None:
        return APPROXIMATED, pairs[0].train_q.copy(), pairs[0].train_c.copy(), [0]
    return OK, best[1], best[0], best_in


def median_query(pairs):
    """cal_abs_pose_err_metric's pose (:386, :396-398) -> (status, q, c)"""
    k = len(pairs)
    if k == 0:
        return NO_PAIRS, np.full(4, np.nan), np.full(3, np.nan)
    X = np.stack([p.abs_c for p in pairs])
    y = np.sum(X, 0) / k
    st = OK | ITER_CAP
    with np.errstate(all='ignore'):
        for _ in range(WEISZFELD_CAP):
            D = np.sqrt(((X - y) ** 2).sum(1))
            nz = D != 0
            if not nz.any():
                st = OK
                break
            Dinv = 1 / D[nz]
            Dinvs = Dinv.sum()
            T = ((Dinv / Dinvs)[:, None] * X[nz]).sum(0)
            nzero = k - int(nz.sum())
            if nzero == 0:
                y1 = T
            else:
                R = (T - y) * Dinvs
                r = np.sqrt(R.dot(R))
                rinv = 0 if r == 0 else nzero / r
                y1 = max(0, 1 - rinv) * T + min(1, rinv) * y
            step = np.sqrt(((y - y1) ** 2).sum())
            if TRACE is not None:
                TRACE['steps'].append(step)
            y = y1
            if step < 1e-5:
                st = OK
                break
        U = np.stack([p.abs_q / np.sqrt(p.abs_q.dot(p.abs_q)) for p in pairs])
        M = U.T @ U
        if not np.isfinite(M).all():
            return st, np.full(4, np.nan), y
        vals, vecs = np.linalg.eigh(M)
        q = mat2quat(quat2mat(vecs[:, np.argmax(vals)]))
    return st, q, y


def fuse(train_q, train_c, pred_R, pred_t, offsets, mode, thr_deg=15.0, thr_mult=1.414, lo_iters=10, seed=0):
    """mfr_abs_pose_fuse on the host: -> dict abs_q [Q,4], abs_c [Q,3], inlier_mask [P] int32, status [Q] int32"""
    offsets = np.asarray(offsets, np.int64)
    Q, P = len(offsets) - 1, len(train_q)
    abs_q, abs_c = np.full((Q, 4), np.nan), np.full((Q, 3), np.nan)
    mask, status = np.zeros(P, np.int32), np.zeros(Q, np.int32)
    for qi in range(Q):
        a, b = offsets[qi], offsets[qi + 1]
        pairs = [Pair(train_q[i], train_c[i], pred_R[i], pred_t[i]) for i in range(a, b)]
        if mode == 1:
            status[qi], abs_q[qi], abs_c[qi], inl = ransac_query(pairs, thr_deg, thr_mult, lo_iters, seed, qi)
            mask[a + np.asarray(inl, np.int64)] = 1
        else:
            status[qi], abs_q[qi], abs_c[qi] = median_query(pairs)
            mask[a:b] = 1
    return dict(abs_q=abs_q, abs_c=abs_c, inlier_mask=mask, status=status)
