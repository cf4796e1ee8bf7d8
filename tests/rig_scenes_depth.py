"""Query-side depth for the seeded rigs of tests/rig_scenes.py: what a 3-D/3-D rig solver (POSE_SOLVER 'RigProcrustes', the rig entry point of
csrc/procrustes.hip, tests/rig_procrustes_ref.py) reads beside the reference view's map.

  depth1 [T,H,W]   per window frame a smooth background plane (5 m, tilted) and, at the TRUNCATED pixel of every true correspondence, the true
                   depth of that point in frame j's camera.  Pixel (0,0) is 0, the map's minimum and its one invalid pixel, as in depth0.
  outliers         keep the background plane under their random observation: their lifted point is wrong by metres
  noise            0.5 px per coordinate by default.  The solver lifts the INTEGER pixel (np.int32 truncation, as upstream), so a true
                   correspondence is off by up to one pixel per axis before any noise: (1 + noise) px * Z / f, 2.7 cm per pixel at 4 m.
  MAX_CORR_DIST    0.1 m: 3.75 px at the scenes' typical 4 m, 1.5 px at their far end of 10 m.  The host test asserts on the mirror that at
                   least half of the true correspondences of every seeded scene it uses are inliers.

Two true correspondences that truncate to one pixel of a frame share the later one's depth (the earlier becomes an outlier).  rig_scenes
keeps observations that project outside the 160 x 120 image (rig PnP reads no query-side pixel); here such a point has no pixel to carry a
depth, no matcher could have reported it, and `inl` marks it False: a true correspondence is one observed inside its frame.  Everything is
a pure function of the seed."""
import os

import numpy as np

import rig_scenes as S

MAX_CORR_DIST = 0.1
NOISE_PX = 0.5


def background():
    vv, uu = np.mgrid[0:S.H, 0:S.W]
    d = (5.0 + 0.01 * (uu - S.W / 2) - 0.008 * (vv - S.H / 2)).astype(np.float32)
    d[0, 0] = 0.0
    return d


def _true_depths(pts0, depth0, K0, R, t, A):
    """depth in frame j's camera of the reference pixels pts0 (u + 0.25, v + 0.5) lifted through depth0"""
    u, v = np.floor(pts0[:, 0]).astype(int), np.floor(pts0[:, 1]).astype(int)
    X = depth0[v, u].astype(np.float64)[:, None] * (np.linalg.inv(K0) @ np.stack([u, v, np.ones(len(u))])).T
    Y = (A[:3, :3] @ (R @ X.T + t[:, None]) + A[:3, 3:4]).T
    return Y[:, 2]


def _stamp(depth, pts1, z, good):
    """depth[v, u] = z at the truncated pixel of every good observation inside the map -> (depth, which observations those were)"""
    x = np.asarray(pts1, np.float32)
    inside = (x[:, 0] > -1.0) & (x[:, 0] < depth.shape[1]) & (x[:, 1] > -1.0) & (x[:, 1] < depth.shape[0]) & good & (z > 0.0)
    u, v = x[inside, 0].astype(np.int32), x[inside, 1].astype(np.int32)
    depth[v, u] = z[inside]
    return depth, inside


def make_rig_scene(seed, T, n_per_frame, noise_px=NOISE_PX, outlier_frac=0.3, zero_query_depth=False):
    """rig_scenes.make_rig_scene plus depth1 [T,H,W] f32"""
    sc = S.make_rig_scene(seed, T, n_per_frame, noise_px=noise_px, outlier_frac=outlier_frac)
    d1 = np.zeros((T, S.H, S.W), np.float32)
    if not zero_query_depth:
        for j in range(T):
            z = _true_depths(sc["pts0"][j], sc["depth0"], sc["K0"], sc["R"], sc["t"], sc["rig_T"][j]) if len(sc["pts0"][j]) else np.zeros(0)
            d1[j], sc["inl"][j] = _stamp(background(), sc["pts1"][j], z.astype(np.float32), sc["inl"][j])
    sc["depth1"] = d1
    return sc


def pack(scenes, maxN=None):
    """rig_scenes.pack plus depth1 [B,T,H,W]"""
    pk = S.pack(scenes, maxN)
    pk["depth1"] = np.stack([s["depth1"] for s in scenes])
    return pk


def write_rig_tree(root, **kw):
    """rig_scenes.write_rig_tree, then every seq1 depth PNG rewritten to agree with the geometry: the plane of rig_scenes.tree_depth as the
    background and, at the truncated pixel of each of the frame's exact correspondences, that point's depth in the frame's camera (uint16
    millimetres).  The tree rig_scenes writes stores the REFERENCE view's plane for every frame, which no 3-D/3-D solve can use."""
    from PIL import Image
    tree = S.write_rig_tree(root, **kw)
    rows = np.load(os.path.join(tree["scene_root"], "correspondences_exact.npz"))["correspondences"]
    depth0 = (np.round(S.tree_depth() * 1000).astype(np.uint16).astype(np.float64) / 1000).astype(np.float32)      # what the loader reads back
    for k, name in enumerate(tree["names"][1:]):
        R, t = tree["poses"][name]
        z = _true_depths(rows[k][:, :2], depth0, tree["K"], R, t, np.eye(4))
        d, _ = _stamp(S.tree_depth().astype(np.float32), rows[k][:, 2:].astype(np.float32), z.astype(np.float32), np.ones(len(z), bool))
        Image.fromarray(np.round(d.astype(np.float64) * 1000).astype(np.uint16)).save(os.path.join(tree["scene_root"], name).replace(".jpg", ".dptkitti.png"))
    return tree
