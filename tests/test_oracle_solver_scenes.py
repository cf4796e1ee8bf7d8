"""The CPU oracle on the hard scenes of tests/solver_scenes.py: planes, tiny baselines, orbits up to 180 deg, collinear points,
repeated matches, keypoints on the truncation edges, non-finite keypoints and depths, flat depth maps, off-centre intrinsics.

Invariants on every case and solver: the status is one of ST_*; status OK means a finite pose with a proper rotation
(|R^T R - I| < 1e-12, det R = +1); a failed status means a NaN pose and no inliers; the inlier mask sums to n_inliers.  The
lifts are checked against a plain numpy statement of the validity rules.  Known answers are asserted where the geometry
defines them, with the bars of the existing known-answer tests:
  PnP          rotation < 0.2 deg, |t - t_gt| < 0.02 m (test_oracle_known_answers.test_pnp_and_emat_recover_known_pose)
  Procrustes   rotation < 0.3 deg, |t - t_gt| < 0.02 m (test_gpu_procrustes_parity.test_procrustes_known_answer)
  E-matrix     rotation < 0.5 deg, direction of t < 3 deg (test_gpu_emat_parity.test_emat_known_answer_pose), on the orbit
               scenes (a general 3-D point set seen from 90 to 180 deg apart) and rotation only on the pure-rotation and tiny-
               baseline scenes.  No bar on the planar scenes: a plane admits two Essential matrices that explain every match
               (the oracle lands 8.8 deg off on wall_0 with either score, 24 deg off on floor_30 with MAGSAC++), so neither
               answer is wrong for the data.
"""
import numpy as np
import pytest

from mapfree_reloc_amd import synth
from oracle import oracle_lib as O
from tests import solver_scenes as S

ST_ALL = (O.ST_OK, O.ST_TOO_FEW, O.ST_BAD_DEPTH, O.ST_NO_MODEL, O.ST_DEGENERATE)
CASES = S.catalogue() + S.catalogue(k64=True)
BY_NAME = {c["name"]: c for c in CASES}
NAMES = list(BY_NAME)
ORBITS = ("orbit_90", "orbit_150", "orbit_179.9", "orbit_180")

# measured misses of a known answer (oracle and device alike: the device is bit-exact with the oracle)
EMAT_MISSES = {
    ("count", "orbit_179.9"): "inlier-count score + LM polish: rotation 1.69 deg off (bar 0.5 deg); MAGSAC++ gets 0.12 deg",
    ("count", "orbit_180"): "inlier-count score + LM polish: rotation 0.535 deg off (bar 0.5 deg); MAGSAC++ gets 0.14 deg",
}


def check_pose(st, R, t, n_inl, mask=None):
    assert st in ST_ALL, st
    R, t = np.asarray(R).reshape(3, 3), np.asarray(t).reshape(3)
    if st == O.ST_OK:
        assert np.isfinite(R).all() and np.isfinite(t).all()
        assert np.abs(R.T @ R - np.eye(3)).max() < 1e-12
        assert abs(np.linalg.det(R) - 1.0) < 1e-12
    else:
        assert np.isnan(R).all() and np.isnan(t).all() and n_inl == 0
    if mask is not None:
        assert int(np.asarray(mask).astype(np.int64).sum()) == n_inl


def t_angle_deg(t, t_gt):
    return float(np.degrees(np.arccos(np.clip(np.ravel(t) @ (np.ravel(t_gt) / np.linalg.norm(t_gt)), -1, 1))))


def expected_rows(pts0, depth0, pts1=None, depth1=None, dmin=True):
    """plain statement of the lift rules: a coordinate is a pixel iff -1 < x < size (NaN and +-inf are not), truncated toward
    zero; depth valid iff d > min over the map's numbers (PnP / Procrustes, quirk Q6) or d > 0 (scale)"""
    def pix(p, d):
        Hh, Ww = d.shape
        ok = (p[:, 0] > -1) & (p[:, 0] < Ww) & (p[:, 1] > -1) & (p[:, 1] < Hh)
        u = np.where(ok, p[:, 0], 0).astype(np.int32); v = np.where(ok, p[:, 1], 0).astype(np.int32)
        z = d[v, u]
        with np.errstate(invalid="ignore"):
            lim = np.nanmin(np.where(np.isnan(d), np.inf, d)) if dmin else np.float32(0)
            return ok & (z > lim), u, v, z
    ok, u, v, z = pix(pts0, depth0)
    if pts1 is not None:
        ok1, _, _, _ = pix(pts1, depth1)
        ok = ok & ok1
    return ok, u, v, z


def test_catalogue_is_stable():
    ids = [c["pair_id"] for c in CASES]
    assert len(set(ids)) == len(ids) and len(set(NAMES)) == len(NAMES)
    for c in CASES:
        assert c["depth0"].shape == (S.H, S.W) and c["pts0"].dtype == np.float32 and len(c["pts0"]) >= 50, c["name"]
    # the non-finite rows really are there
    assert np.isnan(BY_NAME["nonfinite_pts0"]["pts0"]).any() and np.isinf(BY_NAME["nonfinite_pts1"]["pts1"]).any()
    assert np.isnan(BY_NAME["bad_depth"]["depth0"]).any() and (BY_NAME["bad_depth"]["depth0"] < 0).any()


@pytest.mark.parametrize("name", NAMES)
def test_pnp_on_hard_scenes(name):
    c = BY_NAME[name]
    xyz, obs, src = O.pnp_lift(c["pts0"], c["pts1"], c["depth0"], c["K0"])
    ok, u, v, z = expected_rows(c["pts0"], c["depth0"])
    np.testing.assert_array_equal(src, np.nonzero(ok)[0])
    K = c["K0"].astype(np.float64)
    ray = np.stack([(u[ok] - K[0, 2]) / K[0, 0], (v[ok] - K[1, 2]) / K[1, 1], np.ones(ok.sum())], 1)
    np.testing.assert_allclose(xyz, z[ok, None].astype(np.float64) * ray, rtol=1e-6, atol=1e-6)   # inv(K) in float32
    np.testing.assert_array_equal(obs, c["pts1"][ok].astype(np.float64))
    r = O.pnp_ransac(xyz, obs, c["K1"], seed=0, pair_id=c["pair_id"], want_counts=True)
    check_pose(r["status"], r["R"], r["t"], r["n_inl"], r["mask"])
    st, R, t, ninl = O.pnp_solve(c["pts0"], c["pts1"], c["depth0"], c["K0"], c["K1"], seed=0, pair_id=c["pair_id"])
    check_pose(st, R, t, ninl)
    if len(xyz) >= 4:
        assert st == r["status"] and ninl == r["n_inl"]
        np.testing.assert_array_equal(R, r["R"])
    else:
        assert st == O.ST_BAD_DEPTH
    if "pnp" in c["expect"]:
        assert st == O.ST_OK
        assert synth.rot_err_deg(R, c["R_gt"]) < 0.2 and np.linalg.norm(t.ravel() - c["t_gt"]) < 0.02


def test_pnp_lift_rejects_non_finite_and_edge_keypoints():
    """NaN / +-inf keypoints are invalid (not pixel 0); -0.999 truncates to column 0, -1.0 and W do not lift"""
    c = BY_NAME["nonfinite_pts0"]
    _, _, src = O.pnp_lift(c["pts0"], c["pts1"], c["depth0"], c["K0"])
    bad = np.nonzero(~np.isfinite(c["pts0"]).all(1))[0]
    assert len(bad) == 8 and not np.isin(bad, src).any()
    c = BY_NAME["border"]
    _, _, src = O.pnp_lift(c["pts0"], c["pts1"], c["depth0"], c["K0"])
    lifted = set(src.tolist())
    for r, e in enumerate(S.U_EDGES):
        assert (r in lifted) == (e in (-0.999, 0.0, S.W - 1.0, S.F32_BELOW_W, float(S.H))), e
    for r, e in enumerate(S.V_EDGES, start=len(S.U_EDGES)):
        assert (r in lifted) == (e in (-0.999, 0.0, S.H - 1.0, S.F32_BELOW_H)), e


def test_pnp_degenerate_translation():
    """|t| > 1000 m (pose_solver.py:223-225): the pose is found, then refused with ST_DEGENERATE, a NaN pose and no inliers"""
    X, obs, K1, _, _ = S.degenerate_translation()
    r = O.pnp_ransac(X, obs, K1, seed=0, pair_id=7050)
    assert r["status"] == O.ST_DEGENERATE and r["best_iter"] >= 0
    check_pose(r["status"], r["R"], r["t"], r["n_inl"], r["mask"])
    assert not r["mask"].any()


EMAT_PARAMS = [pytest.param(name, score, id=f"{name}-{score}",
                             marks=[pytest.mark.xfail(strict=True, reason=EMAT_MISSES[(score, name)])] if (score, name) in EMAT_MISSES else [])
               for name in NAMES for score in ("magsac", "count")]


@pytest.mark.parametrize("name,score", EMAT_PARAMS)
def test_emat_and_scale_on_hard_scenes(name, score):
    c = BY_NAME[name]
    e = O.emat_solve(c["pts0"], c["pts1"], c["K0"], c["K1"], 2.0, 0.9999, 1000, 0, c["pair_id"],
                     score=O.EMAT_MAGSAC if score == "magsac" else O.EMAT_COUNT)
    check_pose(e["status"], e["R"], e["t"], e["n_inl"], e["mask"])
    if e["status"] == O.ST_OK:
        assert abs(np.linalg.norm(e["t"]) - 1.0) < 1e-12                       # recoverPose's unit translation
        assert not (e["mask"].astype(bool) & ~e["ransac_mask"].astype(bool)).any()
        sc = O.scale_lift(c["pts0"], c["pts1"], e["mask"], c["depth0"], c["depth1"], c["K0"], c["K1"], e["R"], e["t"])
        ok, _, _, _ = expected_rows(c["pts0"], c["depth0"], c["pts1"], c["depth1"], dmin=False)
        assert len(sc) == int((ok & (e["mask"] == 1)).sum())
        cnt, bs, bi = O.scale_ransac(sc, 0.1)
        assert 0 <= cnt <= len(sc) and (cnt == 0) == (len(sc) == 0)
        if cnt:
            assert bs == sc[bi]
    if name in ORBITS:
        assert e["status"] == O.ST_OK
        assert synth.rot_err_deg(e["R"], c["R_gt"]) < 0.5 and t_angle_deg(e["t"], c["t_gt"]) < 3.0
    if "rot_only" in c["expect"]:
        assert e["status"] == O.ST_OK and synth.rot_err_deg(e["R"], c["R_gt"]) < 0.5


@pytest.mark.parametrize("name", NAMES)
def test_procrustes_on_hard_scenes(name):
    c = BY_NAME[name]
    P, Q = O.procrustes_lift(c["pts0"], c["pts1"], c["depth0"], c["depth1"], c["K0"], c["K1"])
    ok0, _, _, _ = expected_rows(c["pts0"], c["depth0"])
    ok1, _, _, _ = expected_rows(c["pts1"], c["depth1"])
    assert len(P) == int((ok0 & ok1).sum())
    st, R, t, ninl = O.procrustes_solve(c["pts0"], c["pts1"], c["depth0"], c["depth1"], c["K0"], c["K1"], seed=0,
                                        pair_id=c["pair_id"])
    check_pose(st, R, t, ninl)
    assert st == (O.ST_OK if len(P) >= 3 else O.ST_BAD_DEPTH)
    assert 0 <= ninl <= len(P)
    if "procrustes" in c["expect"]:
        assert synth.rot_err_deg(R, c["R_gt"]) < 0.3 and np.linalg.norm(t.ravel() - c["t_gt"]) < 0.02
    if st == O.ST_OK:
        ref = O.procrustes_icp(c["depth0"], c["depth1"], c["K0"], c["K1"], R, t.reshape(3), 0.05)
        check_pose(O.ST_OK, ref["R"], ref["t"], ref["n_inliers"])
        assert 0 <= ref["iters"] <= 30 and 0.0 <= ref["fitness"] <= 1.0 and ref["n_inliers"] >= 0
