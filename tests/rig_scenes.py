"""Seeded camera rigs for the rig PnP tests (csrc/pnp_rig.hip, tests/rig_pnp_ref.py): one reference view with a depth map and T query
frames that form a rig around the last one.

  points      reference pixels with a depth of 1-10 m (a tilted plane plus relief, stored in the depth map the solver lifts from)
  pose        reference -> last frame: rotation <= 30 degrees, |t| in [0.2, 2] m
  rig         window frames within 0.3 m and 10 degrees of the last one (A_j: last frame's camera -> frame j's camera; A_last = identity)
  noise       Gaussian, 1 px per coordinate by default;  outliers: 30 % of a frame's correspondences get a uniform random observation

Everything is a pure function of the seed.  Correspondences are float32 like the matchers' output; the reference pixels sit at
(u + 0.25, v + 0.5) so that the solver's integer truncation lands on (u, v)."""
import numpy as np

H, W = 120, 160
K_REF = np.array([[150.0, 0.0, 80.0], [0.0, 150.0, 60.0], [0.0, 0.0, 1.0]])


def rodrigues(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(angle) * Kx + (1.0 - np.cos(angle)) * (Kx @ Kx)


def _rigid(rng, max_deg, tmin, tmax):
    R = rodrigues(rng.normal(size=3), np.deg2rad(rng.uniform(0.0, max_deg)))
    d = rng.normal(size=3)
    return R, d / np.linalg.norm(d) * rng.uniform(tmin, tmax)


def make_rig_scene(seed, T, n_per_frame, noise_px=1.0, outlier_frac=0.3, zero_depth=False):
    """n_per_frame: int or a list of T counts.  Returns a dict:
      depth0 [H,W] f32, K0 [3,3] f64, K1 [T,3,3] f64, rig_T [T,4,4] f64, pts0 / pts1: lists of T float32 [n_j,2] arrays,
      R, t: the true pose reference -> last frame, inl: list of T bool arrays (True = a true correspondence)"""
    rng = np.random.default_rng(seed)
    ns = [int(n_per_frame)] * T if np.isscalar(n_per_frame) else [int(n) for n in n_per_frame]
    assert len(ns) == T
    vv, uu = np.mgrid[0:H, 0:W]
    depth = 4.0 + 0.02 * (uu - W / 2) + 0.015 * (vv - H / 2) + 1.5 * np.sin(uu / 9.0) * np.cos(vv / 7.0)
    depth = np.clip(depth, 1.0, 10.0).astype(np.float32)
    depth[0, 0] = 0.0                                           # the map's minimum: pixel (0,0) is the one invalid pixel (d > depth.min())
    if zero_depth:
        depth[:] = 0.0
    R, t = _rigid(rng, 30.0, 0.2, 2.0)
    rig = np.tile(np.eye(4), (T, 1, 1))
    K1 = np.tile(K_REF, (T, 1, 1))
    for j in range(T - 1):
        RA, tA = _rigid(rng, 10.0, 0.0, 0.3)
        rig[j, :3, :3], rig[j, :3, 3] = RA, tA
        K1[j, 0, 0] = K1[j, 1, 1] = 150.0 + rng.uniform(-5.0, 5.0)         # every frame its own intrinsics
    Ki = np.linalg.inv(K_REF)
    pts0, pts1, inl = [], [], []
    for j, n in enumerate(ns):
        pix = rng.choice(np.arange(1, H * W), size=n, replace=False) if n else np.zeros(0, np.int64)
        u, v = (pix % W).astype(np.float64), (pix // W).astype(np.float64)
        X = depth[pix // W, pix % W].astype(np.float64)[:, None] * (Ki @ np.stack([u, v, np.ones(n)])).T
        Y = (rig[j, :3, :3] @ (R @ X.T + t[:, None]) + rig[j, :3, 3:4]).T
        x = (K1[j] @ (Y / Y[:, 2:3]).T).T[:, :2] + noise_px * rng.normal(size=(n, 2))
        good = rng.uniform(size=n) >= outlier_frac
        x[~good] = rng.uniform([0.0, 0.0], [W, H], size=(n, 2))[~good]
        pts0.append(np.stack([u + 0.25, v + 0.5], 1).astype(np.float32))
        pts1.append(x.astype(np.float32))
        inl.append(good)
    return dict(depth0=depth, K0=K_REF.copy(), K1=K1, rig_T=rig, pts0=pts0, pts1=pts1, R=R, t=t, inl=inl, T=T)


def pack(scenes, maxN=None):
    """scenes of one T -> the solver's arrays: pts0 / pts1 [B,T,maxN,2] f32, n_corr [B,T] i32, depth0 [B,H,W], K0 [B,3,3], K1 [B,T,3,3], rig_T [B,T,4,4]"""
    B, T = len(scenes), scenes[0]["T"]
    maxN = maxN or max(max(len(p) for s in scenes for p in s["pts0"]), 4)
    p0 = np.zeros((B, T, maxN, 2), np.float32); p1 = np.zeros((B, T, maxN, 2), np.float32)
    n = np.zeros((B, T), np.int32)
    for b, s in enumerate(scenes):
        for j in range(T):
            k = len(s["pts0"][j])
            p0[b, j, :k], p1[b, j, :k], n[b, j] = s["pts0"][j], s["pts1"][j], k
    st = lambda key: np.stack([s[key] for s in scenes])
    return dict(pts0=p0, pts1=p1, n_corr=n, depth0=st("depth0"), K0=st("K0"), K1=st("K1"), rig_T=st("rig_T"))


def pose_error(R, t, Rgt, tgt):
    """(rotation angle between R and Rgt in rad, |t - tgt| in m)"""
    d = np.linalg.norm(np.asarray(R, np.float64).reshape(3, 3) - Rgt)             # |R - Rgt|_F = 2 sqrt(2) sin(angle / 2): no arccos near 1
    return float(2.0 * np.arcsin(min(d / (2.0 * np.sqrt(2.0)), 1.0))), float(np.linalg.norm(np.asarray(t, np.float64).reshape(3) - tgt))


# ---------------------------------------------------------------- a written Map-free val scene with device-tracking poses
def mat2quat(R):
    """(w, x, y, z) of a rotation matrix, w >= 0"""
    R = np.asarray(R, np.float64)
    q = np.array([1.0 + R[0, 0] + R[1, 1] + R[2, 2], R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    k = int(np.argmax([R[0, 0] + R[1, 1] + R[2, 2], R[0, 0], R[1, 1], R[2, 2]]))
    if k == 1:
        q = np.array([R[2, 1] - R[1, 2], 1.0 + R[0, 0] - R[1, 1] - R[2, 2], R[0, 1] + R[1, 0], R[0, 2] + R[2, 0]])
    elif k == 2:
        q = np.array([R[0, 2] - R[2, 0], R[0, 1] + R[1, 0], 1.0 - R[0, 0] + R[1, 1] - R[2, 2], R[1, 2] + R[2, 1]])
    elif k == 3:
        q = np.array([R[1, 0] - R[0, 1], R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], 1.0 - R[0, 0] - R[1, 1] + R[2, 2]])
    q = q / np.linalg.norm(q)
    return q if q[0] >= 0 else -q


TREE_H, TREE_W = 120, 160


def tree_depth():
    """the reference view's depth: a tilted plane, metres (stored as uint16 millimetres)"""
    vv, uu = np.mgrid[0:TREE_H, 0:TREE_W]
    return 3.0 + 0.004 * uu + 0.003 * vv


def write_rig_tree(root, seed=0, n_frames=8, n_corr=150, with_device=True, scene="s00000"):
    """root/val/<scene>/: seq0/frame_00000 (the world frame) and n_frames seq1 frames as JPEG + plane-depth PNG, intrinsics.txt, poses.txt,
    correspondences_exact.npz (one row per seq1 frame in file order: exact projections of reference pixels lifted with the plane depth) and,
    with_device, poses_device.txt: the same trajectory in a world rotated and shifted against that of poses.txt, so only relative device
    poses mean anything.  Returns dict(scene_root, poses {name: (R, t)}, K)."""
    import os
    from PIL import Image
    rng = np.random.default_rng(seed)
    sc = os.path.join(str(root), "val", scene)
    os.makedirs(os.path.join(sc, "seq0")); os.makedirs(os.path.join(sc, "seq1"))
    K = K_REF
    depth = tree_depth()
    rv0, t0 = rng.normal(size=3), rng.normal(size=3)
    rv0 = rv0 / np.linalg.norm(rv0) * np.deg2rad(15.0); t0 = t0 / np.linalg.norm(t0) * 0.8
    RG, tG = rodrigues(rng.normal(size=3), 1.1), np.array([3.0, -2.0, 5.0])
    names = ["seq0/frame_00000.jpg"] + [f"seq1/frame_{i:05d}.jpg" for i in range(n_frames)]
    poses = {names[0]: (np.eye(3), np.zeros(3))}
    for n in names[1:]:
        rv = rv0 + np.deg2rad(3.0) * rng.uniform(-1, 1, 3)
        poses[n] = (rodrigues(rv, np.linalg.norm(rv)), t0 + 0.1 * rng.uniform(-1, 1, 3))
    line = lambda n, R, t: n + " " + " ".join(repr(float(v)) for v in list(mat2quat(R)) + list(t))
    lp, ld, lk = ["# frame qw qx qy qz tx ty tz"], ["# frame qw qx qy qz tx ty tz"], ["# frame fx fy cx cy W H"]
    for n in names:
        R, t = poses[n]
        lp.append(line(n, R, t))
        Rd = R @ RG.T
        ld.append(line(n, Rd, t - Rd @ tG))
        lk.append(f"{n} {K[0, 0]} {K[1, 1]} {K[0, 2]} {K[1, 2]} {TREE_W} {TREE_H}")
        img = rng.integers(0, 256, size=(TREE_H // 8, TREE_W // 8, 3), dtype=np.uint8).repeat(8, 0).repeat(8, 1)
        Image.fromarray(img).save(os.path.join(sc, n), format="JPEG", quality=92)
        Image.fromarray(np.round(depth * 1000).astype(np.uint16)).save(os.path.join(sc, n).replace(".jpg", ".dptkitti.png"))
    open(os.path.join(sc, "poses.txt"), "w").write("\n".join(lp) + "\n")
    open(os.path.join(sc, "intrinsics.txt"), "w").write("\n".join(lk) + "\n")
    if with_device:
        open(os.path.join(sc, "poses_device.txt"), "w").write("\n".join(ld) + "\n")
    Ki = np.linalg.inv(K)
    rows = []
    for n in names[1:]:
        R, t = poses[n]
        pix = rng.choice(np.arange(1, TREE_H * TREE_W), size=n_corr, replace=False)
        u, v = (pix % TREE_W).astype(np.float64), (pix // TREE_W).astype(np.float64)
        X = depth[pix // TREE_W, pix % TREE_W][:, None] * (Ki @ np.stack([u, v, np.ones(n_corr)])).T
        Y = X @ R.T + t
        x = (Y / Y[:, 2:3]) @ K.T
        rows.append(np.concatenate([np.stack([u + 0.25, v + 0.5], 1), x[:, :2]], 1))
    np.savez_compressed(os.path.join(sc, "correspondences_exact.npz"), correspondences=np.stack(rows))
    return dict(scene_root=sc, poses=poses, K=K.copy(), names=names)
