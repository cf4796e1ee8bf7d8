"""Hard two-view scenes for the pose solvers (test helper, not a test module).

`synth.make_pair` draws general-position points 1-10 m deep, rotations <= 30 deg and baselines of 0.2-2 m, with every keypoint
strictly inside the image and every value finite.  Map-free pairs are often harder: orbits around an object (rotations up to
180 deg), walls and floors, tiny baselines, repeated matches, sub-pixel keypoints on the image border, depth maps with holes,
constant patches or non-finite values.  `catalogue()` builds one case per such geometry; `make_batch()` stacks cases into the
dict `synth.make_batch` returns (pts0/pts1/n_corr/depth0/depth1/K0/K1/pair_ids/R_gt/t_gt), so the existing comparison code
runs on them unchanged.

Every case is deterministic and carries a stable pair id.  Keypoints of image 0 of the scene points sit on integer pixels and
depth0 holds their exact depth there, so a lifted point is the scene point itself; image-1 keypoints are sub-pixel projections
plus noise, with depth1 holding the true depth at their truncated pixel.  `expect` names the known answers the geometry
defines: 'pnp' / 'procrustes' (R and t recoverable), 'rot_only' (pure rotation: the direction of t is undefined for the
Essential matrix), 'emat' (the Essential matrix is well defined)."""
import numpy as np

H, W = 240, 320
F = 300.0


def _K(fx=F, fy=F, cx=W / 2 - 0.5, cy=H / 2 - 0.5):
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], dtype=np.float32)


def _rot(axis, deg):
    ax = np.asarray(axis, np.float64)
    ax = ax / np.linalg.norm(ax)
    a = np.deg2rad(deg)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx


def _background(rng):
    """depth map of the scene behind the points: 5 m +- 0.5 m, with a small hole (0 = no depth, as the dataset's PNGs hold)"""
    d = (5.0 + rng.uniform(-0.5, 0.5, (H, W))).astype(np.float32)
    d[100:104, 150:156] = 0.0
    return d


def _case(name, pid, ui, vi, z, R, t, rng, K0=None, K1=None, noise=0.3, outl=0.0, expect=()):
    """scene points given as integer pixels (ui, vi) of image 0 and their depth z -> case dict (only points seen by both views)"""
    K0 = _K() if K0 is None else K0
    K1 = _K() if K1 is None else K1
    ui, vi, z = np.asarray(ui, np.float64), np.asarray(vi, np.float64), np.asarray(z, np.float32).astype(np.float64)
    K0d, K1d = K0.astype(np.float64), K1.astype(np.float64)
    X0 = np.stack([(ui - K0d[0, 2]) / K0d[0, 0] * z, (vi - K0d[1, 2]) / K0d[1, 1] * z, z], 1)
    X1 = X0 @ R.T + t
    with np.errstate(divide="ignore", invalid="ignore"):
        u1 = K1d[0, 0] * X1[:, 0] / X1[:, 2] + K1d[0, 2]
        v1 = K1d[1, 1] * X1[:, 1] / X1[:, 2] + K1d[1, 2]
    u1 = u1 + rng.normal(size=len(u1)) * noise
    v1 = v1 + rng.normal(size=len(v1)) * noise
    ok = (X1[:, 2] > 0.3) & (u1 > 1) & (u1 < W - 2) & (v1 > 1) & (v1 < H - 2)
    ui, vi, z, X1, u1, v1 = ui[ok], vi[ok], z[ok], X1[ok], u1[ok], v1[ok]
    n = len(ui)
    pts0 = np.stack([ui, vi], 1).astype(np.float32)
    pts1 = np.stack([u1, v1], 1).astype(np.float32)
    inl = np.ones(n, bool)
    no = int(round(outl * n))
    if no:
        oi = rng.permutation(n)[:no]
        pts1[oi] = np.stack([rng.uniform(1, W - 2, no), rng.uniform(1, H - 2, no)], 1).astype(np.float32)
        inl[oi] = False
    depth0, depth1 = _background(rng), _background(rng)
    depth0[vi.astype(int), ui.astype(int)] = z.astype(np.float32)
    p1i = pts1.astype(np.int32)
    depth1[p1i[inl, 1], p1i[inl, 0]] = X1[inl, 2].astype(np.float32)
    return dict(name=name, pair_id=pid, pts0=pts0, pts1=pts1, depth0=depth0, depth1=depth1, K0=K0, K1=K1,
                R_gt=np.asarray(R, np.float64), t_gt=np.asarray(t, np.float64), inlier_gt=inl, expect=set(expect))


def _pixels(rng, n, u_lo=4, u_hi=W - 5, v_lo=4, v_hi=H - 5):
    """n distinct integer pixels"""
    flat = rng.choice((u_hi - u_lo) * (v_hi - v_lo), size=n, replace=False)
    return u_lo + flat % (u_hi - u_lo), v_lo + flat // (u_hi - u_lo)


def _general(name, pid, n=160, R=None, t=None, outl=0.3, K0=None, K1=None, expect=("pnp", "procrustes", "emat")):
    rng = np.random.default_rng(pid)
    R = _rot([0.2, 1.0, 0.1], 12.0) if R is None else R
    t = np.array([0.4, -0.05, 0.1]) if t is None else np.asarray(t, np.float64)
    ui, vi = _pixels(rng, 3 * n)
    z = rng.uniform(1.5, 6.0, 3 * n)
    c = _case(name, pid, ui, vi, z, R, t, rng, K0=K0, K1=K1, outl=0.0, expect=expect)
    return _subset(c, n, outl, rng)


def _subset(c, n, outl, rng):
    """first n points of a case, then a fraction of them replaced by uniform outliers in image 1"""
    c = dict(c)
    for k in ("pts0", "pts1", "inlier_gt"):
        c[k] = c[k][:n].copy()
    no = int(round(outl * len(c["pts0"])))
    if no:
        oi = rng.permutation(len(c["pts0"]))[:no]
        c["pts1"][oi] = np.stack([rng.uniform(1, W - 2, no), rng.uniform(1, H - 2, no)], 1).astype(np.float32)
        c["inlier_gt"][oi] = False
    return c


def _wall(name, pid, outl):
    """fronto-parallel wall 3 m ahead (every scene point at the same depth); the wall covers the whole view of camera 0"""
    rng = np.random.default_rng(pid)
    ui, vi = _pixels(rng, 200)
    R, t = _rot([0.1, 1.0, 0.0], 10.0), np.array([0.5, 0.05, 0.1])
    c = _case(name, pid, ui, vi, np.full(len(ui), 3.0), R, t, rng, outl=outl,
              expect=("pnp", "procrustes", "emat"))
    d0 = np.full((H, W), 3.0, np.float32)
    d0[100:104, 150:156] = 0.0                       # a hole: without it the map is constant and every point is rejected (Q6)
    d0[c["pts0"][:, 1].astype(int), c["pts0"][:, 0].astype(int)] = 3.0
    c["depth0"] = d0
    return c


def _floor(name, pid, outl):
    """oblique floor: the plane n.X = 1.5 m with n = (0, 0.94, 0.34), seen from 2 m to 8 m"""
    rng = np.random.default_rng(pid)
    nrm = np.array([0.0, 0.94, 0.34])
    nrm = nrm / np.linalg.norm(nrm)
    ui, vi = _pixels(rng, 1200)
    with np.errstate(divide="ignore"):
        z = 1.5 / (nrm[1] * (vi - (H / 2 - 0.5)) / F + nrm[2])
    keep = (z > 2.0) & (z < 8.0)
    ui, vi, z = ui[keep][:200], vi[keep][:200], z[keep][:200]
    R, t = _rot([0.0, 1.0, 0.3], 15.0), np.array([-0.6, 0.0, 0.3])
    return _case(name, pid, ui, vi, z, R, t, rng, outl=outl, expect=("pnp", "procrustes", "emat"))


def _baseline(name, pid, tnorm):
    """pure rotation (t = 0 exactly) and baselines of 1 mm and 1 um: the direction of t is undefined or ill-defined for the
    Essential matrix"""
    t = np.array([0.6, -0.3, 0.74]) / np.linalg.norm([0.6, -0.3, 0.74]) * tnorm
    return _general(name, pid, n=160, R=_rot([0.3, 1.0, -0.2], 20.0), t=t, outl=0.2,
                    expect=("pnp", "procrustes", "rot_only"))


def _orbit(name, pid, deg):
    """points in a 0.5 m ball 2 m ahead; camera 1 orbits the ball's centre c by `deg` about the vertical axis: X1 = R (X0 - c) + c"""
    rng = np.random.default_rng(pid)
    c = np.array([0.0, 0.0, 2.0])
    if deg == 180.0:
        R = np.diag([-1.0, 1.0, -1.0])               # exactly 180 deg
    else:
        R = _rot([0.0, 1.0, 0.0], deg)
    m = 600
    X = rng.normal(size=(m, 3))
    X = X / np.linalg.norm(X, axis=1, keepdims=True) * 0.5 * rng.uniform(0, 1, (m, 1)) ** (1 / 3) + c
    ui = np.round(F * X[:, 0] / X[:, 2] + (W / 2 - 0.5)).astype(int)
    vi = np.round(F * X[:, 1] / X[:, 2] + (H / 2 - 0.5)).astype(int)
    _, first = np.unique(vi * W + ui, return_index=True)    # one point per pixel
    first = np.sort(first)[:200]
    return _case(name, pid, ui[first], vi[first], X[first, 2], R, c - R @ c, rng, outl=0.2,
                 expect=("pnp", "procrustes", "emat"))


def _collinear(name, pid):
    """every scene point on one 3-D line (in the plane of pixel row 60: Z = a + b X there, hit at integer columns)"""
    rng = np.random.default_rng(pid)
    ui = np.arange(20, 300, 2)
    vi = np.full(len(ui), 60)
    a, b = 3.0, 0.4
    z = a / (1 - b * (ui - (W / 2 - 0.5)) / F)
    return _case(name, pid, ui, vi, z, _rot([0, 1, 0], 8.0), np.array([0.3, 0.0, 0.05]), rng, outl=0.0)


def _duplicates(name, pid):
    c = _general(name, pid, n=60, outl=0.3)
    for k in ("pts0", "pts1", "inlier_gt"):
        c[k] = np.repeat(c[k], 3, axis=0)            # every correspondence three times in a row (ratio-test / LoFTR repeats)
    return c


def _single_match(name, pid, n=50):
    c = _general(name, pid, n=10, outl=0.0)
    for k in ("pts0", "pts1", "inlier_gt"):
        c[k] = np.repeat(c[k][:1], n, axis=0)
    c["expect"] = set()
    return c


F32_BELOW_W = float(np.nextafter(np.float32(W), np.float32(0)))
F32_BELOW_H = float(np.nextafter(np.float32(H), np.float32(0)))
U_EDGES = (-0.999, -1.0, 0.0, W - 1.0, F32_BELOW_W, float(W), float(H), 1e9, -1e9)
V_EDGES = (-0.999, -1.0, 0.0, H - 1.0, F32_BELOW_H, float(H), float(W), 1e9, -1e9)


def _border(name, pid):
    """a healthy scene whose first rows carry keypoints on the truncation edges of both images"""
    c = _general(name, pid, n=160, outl=0.2, expect=())
    p0, p1 = c["pts0"], c["pts1"]
    r = 0
    for e in U_EDGES:
        p0[r] = (e, 50.0); p1[r + 40] = (e, 70.0); r += 1
    for e in V_EDGES:
        p0[r] = (60.0, e); p1[r + 40] = (80.0, e); r += 1
    p0[r] = (F32_BELOW_W, F32_BELOW_H); p1[r + 40] = (F32_BELOW_W, F32_BELOW_H)
    return c


def _nonfinite(name, pid, key):
    """NaN and +-inf in single rows (one coordinate or both) of pts0 or pts1"""
    c = _general(name, pid, n=160, outl=0.2, expect=())
    p = c[key]
    bad = [(np.nan, 50.0), (50.0, np.nan), (np.nan, np.nan), (np.inf, 40.0), (-np.inf, 40.0), (40.0, np.inf),
           (40.0, -np.inf), (np.inf, -np.inf)]
    for i, v in enumerate(bad):
        p[3 + 7 * i] = v
    return c


def _bad_depth(name, pid):
    """NaN, +inf, 0 and negative depth under keypoints of both images"""
    c = _general(name, pid, n=160, outl=0.2, expect=())
    for j, v in enumerate((np.nan, np.inf, 0.0, -1.0, np.nan, -np.inf)):
        i0, i1 = 5 + 9 * j, 8 + 9 * j
        c["depth0"][int(c["pts0"][i0, 1]), int(c["pts0"][i0, 0])] = v
        c["depth1"][int(c["pts1"][i1, 1]), int(c["pts1"][i1, 0])] = v
    return c


def _nan_at_origin(name, pid):
    """the first depth pixel is NaN and a keypoint sits on it: a NaN pixel is invalid and takes no part in the depth minimum"""
    c = _general(name, pid, n=160, outl=0.2, expect=())
    c["depth0"][0, 0] = np.nan
    c["depth1"][0, 0] = np.nan
    c["pts0"][0] = (0.0, 0.0)
    c["pts1"][1] = (0.25, 0.5)
    return c


def _flat_depth(name, pid, value):
    c = _general(name, pid, n=160, outl=0.2, expect=())
    c["depth0"] = np.full((H, W), value, np.float32)
    c["depth1"] = np.full((H, W), value, np.float32)
    return c


def _intrinsics(name, pid, k64):
    """non-square pixels and an off-centre principal point"""
    K0 = _K(fx=320.0, fy=270.0, cx=101.25, cy=151.75)
    K1 = _K(fx=290.0, fy=335.0, cx=190.5, cy=92.0)
    c = _general(name, pid, n=160, outl=0.3, K0=K0, K1=K1)
    if k64:
        c["K0"], c["K1"] = c["K0"].astype(np.float64), c["K1"].astype(np.float64)
    return c


def catalogue(k64=False):
    """the hard cases, K as float32 (k64=False) or only the float64-intrinsics case (k64=True)"""
    if k64:
        return [_intrinsics("intrinsics_f64", 7041, True)]
    return [
        _wall("wall_0", 7001, 0.0), _wall("wall_30", 7002, 0.3),
        _floor("floor_0", 7003, 0.0), _floor("floor_30", 7004, 0.3),
        _baseline("baseline_0", 7010, 0.0), _baseline("baseline_1e-3", 7011, 1e-3), _baseline("baseline_1e-6", 7012, 1e-6),
        _orbit("orbit_90", 7020, 90.0), _orbit("orbit_150", 7021, 150.0), _orbit("orbit_179.9", 7022, 179.9),
        _orbit("orbit_180", 7023, 180.0),
        _collinear("collinear", 7030),
        _duplicates("duplicates_x3", 7031), _single_match("single_match_x50", 7032),
        _border("border", 7033),
        _nonfinite("nonfinite_pts0", 7034, "pts0"), _nonfinite("nonfinite_pts1", 7035, "pts1"),
        _bad_depth("bad_depth", 7036), _nan_at_origin("nan_depth_at_origin", 7037),
        _flat_depth("depth_all_zero", 7038, 0.0), _flat_depth("depth_constant", 7039, 4.0),
        _intrinsics("intrinsics_f32", 7040, False),
    ]


def healthy(pid, n=160):
    """an ordinary pair in the catalogue's image size (the neighbours of the batch-independence test)"""
    return _general(f"healthy_{pid}", pid, n=n, outl=0.3)


def make_batch(cases, maxN=None):
    """stack cases into the fixed-stride device layout (the dict synth.make_batch returns; K keeps the cases' dtype)"""
    B = len(cases)
    n_list = [len(c["pts0"]) for c in cases]
    maxN = maxN or max(max(n_list), 8)
    out = dict(pts0=np.zeros((B, maxN, 2), np.float32), pts1=np.zeros((B, maxN, 2), np.float32),
               n_corr=np.array(n_list, np.int32),
               depth0=np.stack([c["depth0"] for c in cases]), depth1=np.stack([c["depth1"] for c in cases]),
               K0=np.stack([c["K0"] for c in cases]), K1=np.stack([c["K1"] for c in cases]),
               R_gt=np.stack([c["R_gt"] for c in cases]), t_gt=np.stack([c["t_gt"] for c in cases]),
               pair_ids=np.array([c["pair_id"] for c in cases], np.int64), pairs=cases)
    for b, c in enumerate(cases):
        out["pts0"][b, :n_list[b]] = c["pts0"]
        out["pts1"][b, :n_list[b]] = c["pts1"]
    return out


def degenerate_translation():
    """lifted points and observations straight for pnp_ransac, from a pose with |t| = 1500 m > 1000 (pose_solver.py:223-225):
    -> (xyz [n,3] f64, obs [n,2] f64, K1 f32, R_gt, t_gt)"""
    rng = np.random.default_rng(7050)
    R = _rot([0.0, 1.0, 0.2], 25.0)
    t = np.array([1200.0, -300.0, 840.0])
    n = 120
    X1 = np.stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(4, 12, n)], 1)   # in front of camera 1
    X0 = (X1 - t) @ R                                                                       # R^T (X1 - t)
    K1 = _K()
    obs = np.stack([F * X1[:, 0] / X1[:, 2] + (W / 2 - 0.5), F * X1[:, 1] / X1[:, 2] + (H / 2 - 0.5)], 1)
    return X0, obs, K1, R, t
