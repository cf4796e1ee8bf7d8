"""-m gpu: the rig PnP solver (csrc/pnp_rig.hip through solver_ops) against its two yardsticks -- the single-camera PnP solver, which it must
equal bit for bit with one frame and the identity rig, and the numpy mirror tests/rig_pnp_ref.py for T > 1 -- and the multi-frame model
end to end on a written scene."""
import numpy as np
import pytest
import torch

from mapfree_reloc_amd import solver_ops as ops, submission
from mapfree_reloc_amd.builder import build_model
from mapfree_reloc_amd.config import get_cfg_defaults
from mapfree_reloc_amd.datasets import MissingDataError, list_scenes, make_loader

import rig_pnp_ref as M
import rig_scenes as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _lift(pk):
    """the packed scenes' rows lifted by mfr_pnp_lift (every row with its sample's depth map): xyz [B,T,maxN,3], obs, n_valid [B,T]"""
    B, T, maxN, _ = pk["pts0"].shape
    rep = lambda a: np.repeat(a, T, axis=0)
    xyz, obs, _, nv = ops.pnp_lift(_dev(pk["pts0"].reshape(B * T, maxN, 2)), _dev(pk["pts1"].reshape(B * T, maxN, 2)),
                                   _dev(pk["n_corr"].reshape(-1)), _dev(rep(pk["depth0"])), _dev(rep(pk["K0"])))
    return xyz.reshape(B, T, maxN, 3), obs.reshape(B, T, maxN, 2), nv.reshape(B, T)


def _solve(pk, pair_ids, iters, seed=0, want_mask=True):
    return _np(ops.RigPnPBatchSolver(iters, 3.0, 0.9999, seed)(
        _dev(pk["pts0"]), _dev(pk["pts1"]), _dev(pk["n_corr"]), _dev(pk["depth0"]), _dev(pk["K0"]), _dev(pk["K1"]), _dev(pk["rig_T"]),
        _dev(np.asarray(pair_ids, np.int64)), want_mask=want_mask))


# ---------------------------------------------------------------- T = 1, identity rig: the PnP solver itself
@pytest.mark.parametrize("iters", [64, 1000])
@pytest.mark.parametrize("n", [0, 3, 4, 5, 65, 769, 1024])
def test_one_frame_identity_rig_equals_pnp_bit_for_bit(n, iters):
    """n: the sample-size edge (3, 4, 5), one past a wavefront (65), one past the 768-point tile (769), the keypoint budget (1024)"""
    pk = S.pack([S.make_rig_scene(40 + 7 * n + b, 1, n) for b in range(3)])
    assert np.array_equal(pk["rig_T"], np.tile(np.eye(4), (3, 1, 1, 1)))
    pids = np.array([5, 70000, 123456789012], np.int64)
    xyz, obs, nv = _lift(pk)
    assert nv.cpu().numpy().tolist() == [[n]] * 3
    a = _np(ops.pnp_ransac(xyz[:, 0].contiguous(), obs[:, 0].contiguous(), nv[:, 0].contiguous(), _dev(pk["K1"][:, 0]), _dev(pids), iters, seed=9))
    b = _np(ops.rig_pnp_ransac(xyz, obs, nv, _dev(pk["K1"]), ops.rig_rows(_dev(pk["rig_T"])), _dev(pids), iters, seed=9))
    for k in ("counts", "best_iter", "iters_run", "status", "n_inliers", "R", "t"):
        assert np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), k
    assert np.array_equal(a["mask"], b["mask"][:, 0])
    if n >= 65:
        assert (a["status"] == 0).all() and (a["n_inliers"] >= n // 2).all()     # real poses were compared, not three failures
    # ... and from raw correspondences (lift, pre-status, mask scatter)
    c = _np(ops.PnPBatchSolver(iters, 3.0, 0.9999, 9)(_dev(pk["pts0"][:, 0]), _dev(pk["pts1"][:, 0]), _dev(pk["n_corr"][:, 0]), _dev(pk["depth0"]),
                                                       _dev(pk["K0"]), _dev(pk["K1"][:, 0]), _dev(pids), want_mask=True))
    d = _solve(pk, pids, iters, seed=9)
    for k in ("status", "n_inliers", "R", "t"):
        assert np.array_equal(c[k], d[k], equal_nan=c[k].dtype.kind == "f"), k
        assert np.array_equal(c[k], a[k], equal_nan=c[k].dtype.kind == "f"), k
    assert np.array_equal(c["mask"], d["mask"][:, 0])


# ---------------------------------------------------------------- T > 1 against the mirror
CASES = {
    "plain_T2": (2, [[40, 40]]),
    "plain_T9": (9, [[30] * 9]),
    "frame_with_0_points": (3, [[40, 0, 30]]),
    "frame_with_4_points": (3, [[4, 50, 20]]),
    "one_eligible_frame_not_last": (3, [[2, 30, 3]]),
    "no_eligible_frame_one_with_4": (3, [[3, 4, 2]]),
    "too_few": (2, [[3, 2]]),
    "bad_depth": (2, [[10, 10]]),
    "mixed_B3": (9, [[25] * 9, [0, 4, 3, 6, 0, 4, 1, 0, 2], [3, 3, 0, 1, 2, 3, 3, 0, 3]]),
    "tile_boundary_inside_a_frame": (2, [[800, 30]]),
}
ITERS = 64


def _case_scenes(case):
    """the four points of the no-eligible-frame case are true correspondences: its one model is then a pose, and the refinement over so few
    points a well-posed problem whose result does not hang on the order of a sum"""
    T, counts = CASES[case]
    return [S.make_rig_scene(300 + 11 * b + len(case), T, ns, zero_depth=(case == "bad_depth"),
                             outlier_frac=0.0 if case == "no_eligible_frame_one_with_4" else 0.3) for b, ns in enumerate(counts)]


@pytest.mark.parametrize("case", sorted(CASES))
def test_rig_against_mirror(case):
    T = CASES[case][0]
    scenes = _case_scenes(case)
    pk = S.pack(scenes)
    B = len(scenes)
    pids = np.array([17, 4242, 99][:B], np.int64)
    xyz, obs, nv = _lift(pk)
    low = _np(ops.rig_pnp_ransac(xyz, obs, nv, _dev(pk["K1"]), ops.rig_rows(_dev(pk["rig_T"])), _dev(pids), ITERS, seed=2))
    top = _solve(pk, pids, ITERS, seed=2)
    nv = nv.cpu().numpy()
    worst = [0.0, 0.0]
    for b, sc in enumerate(scenes):
        ref = M.rig_pnp_solve(sc["pts0"], sc["pts1"], sc["depth0"], sc["K0"], sc["K1"], sc["rig_T"], max_iters=ITERS, seed=2, pair_id=int(pids[b]))
        assert nv[b].tolist() == ref["n_valid"]
        assert ref["margin"] > 1e-7, "a point of this seeded input sits on the threshold: pick another seed"
        assert top["status"][b] == ref["status"], (b, top["status"][b], ref["status"])
        if ref["status"] not in (M.TOO_FEW, M.BAD_DEPTH):                      # (on lifted rows alone the two are not told apart)
            assert low["status"][b] == ref["status"]
        assert np.array_equal(low["counts"][b], ref["counts"]), np.flatnonzero(low["counts"][b] != ref["counts"])[:5]
        assert low["best_iter"][b] == ref["best_iter"] and low["iters_run"][b] == ref["iters_run"]
        assert low["n_inliers"][b] == top["n_inliers"][b] == ref["n_inl"]
        for j in range(T):
            n, nc = nv[b, j], len(sc["pts0"][j])
            assert np.array_equal(low["mask"][b, j, :n].astype(bool), ref["masks"][j]) and not low["mask"][b, j, n:].any()
            assert np.array_equal(top["mask"][b, j, :nc].astype(bool), ref["masks_orig"][j]) and not top["mask"][b, j, nc:].any()
        if ref["status"] == M.OK:
            assert np.array_equal(low["R"][b], top["R"][b]) and np.array_equal(low["t"][b], top["t"][b])
            er, et = S.pose_error(top["R"][b], top["t"][b], ref["R"], ref["t"])
            worst = [max(worst[0], er), max(worst[1], et)]
            assert er < 1e-4 and et < 1e-4, (er, et)
        else:
            assert np.isnan(top["R"][b]).all() and np.isnan(top["t"][b]).all() and top["n_inliers"][b] == 0
    print(f"{case}: device vs mirror, max {worst[0]:.3e} rad, {worst[1]:.3e} m")
    want = {"too_few": M.TOO_FEW, "bad_depth": M.BAD_DEPTH}.get(case)
    if want is not None:
        assert top["status"].tolist() == [want]
    elif case != "mixed_B3":
        assert top["status"].tolist() == [M.OK]
    else:
        assert top["status"][0] == M.OK and top["status"][2] == M.TOO_FEW


def test_last_frame_with_fewer_than_4_correspondences():
    """the single-frame solver has nothing to work with, the rig solver has the other frames.  Bar against the truth: 1 px noise at f = 150 px
    and 3-7 m depth is 2-5 cm per point across the ray; ~80 true correspondences bring the pose to the centimetre (the noisy scenes of
    test_rig_pnp_host.py have a median of 0.8 cm), 0.05 m is several times that"""
    sc = S.make_rig_scene(77, 3, [60, 60, 3])
    pk = S.pack([sc])
    pid = np.array([31], np.int64)
    last = _np(ops.PnPBatchSolver(1000, 3.0, 0.9999, 0)(_dev(pk["pts0"][:, 2]), _dev(pk["pts1"][:, 2]), _dev(pk["n_corr"][:, 2]), _dev(pk["depth0"]),
                                                          _dev(pk["K0"]), _dev(pk["K1"][:, 2]), _dev(pid)))
    assert last["status"].tolist() == [ops.ST_TOO_FEW] and np.isnan(last["R"]).all()
    got = _solve(pk, pid, 1000)
    ref = M.rig_pnp_solve(sc["pts0"], sc["pts1"], sc["depth0"], sc["K0"], sc["K1"], sc["rig_T"], max_iters=1000, pair_id=31, all_counts=False)
    assert got["status"].tolist() == [ops.ST_OK] == [ref["status"]] and got["n_inliers"][0] == ref["n_inl"] >= 60
    er, et = S.pose_error(got["R"][0], got["t"][0], ref["R"], ref["t"])
    gr, gt = S.pose_error(got["R"][0], got["t"][0], sc["R"], sc["t"])
    print(f"device vs mirror {er:.3e} rad {et:.3e} m; device vs truth {gr:.4f} rad {gt:.4f} m")
    assert er < 1e-4 and et < 1e-4 and gt < 0.05


def test_repeatable_and_follows_pair_ids():
    scenes = [S.make_rig_scene(500 + b, 3, [50, 45, 40]) for b in range(3)]
    pk = S.pack(scenes)
    pids = np.array([3, 1000, 77], np.int64)
    a, b = _solve(pk, pids, 200), _solve(pk, pids, 200)
    perm = [2, 0, 1]
    c = _solve({k: v[perm] for k, v in pk.items()}, pids[perm], 200)
    assert (a["status"] == 0).all()
    for k in a:
        assert np.array_equal(a[k], b[k]), k
        assert np.array_equal(a[k][perm], c[k]), k


# ---------------------------------------------------------------- end to end
def _cfg(root, matcher):
    cfg = get_cfg_defaults()
    cfg.MODEL, cfg.FEATURE_MATCHING, cfg.POSE_SOLVER = "FeatureMatchingMultiFrame", matcher, "PNP"
    cfg.MATCHES_FILE_PATH = "{scene_root}/correspondences_exact.npz"
    cfg.PNP.RANSAC_ITER, cfg.PNP.REPROJECTION_INLIER_THRESHOLD, cfg.PNP.CONFIDENCE = 1000, 3, 0.9999
    cfg.DATASET.DATA_ROOT, cfg.DATASET.HEIGHT, cfg.DATASET.WIDTH, cfg.DATASET.ESTIMATED_DEPTH = str(root), S.TREE_H, S.TREE_W, "dptkitti"
    cfg.DATASET.QUERY_FRAME_COUNT = 3
    cfg.ALLOW_SYNTHETIC_WEIGHTS = True
    return cfg


def test_multiframe_model_end_to_end(tmp_path):
    """8 seq1 frames, T = 3: two samples (windows 1-3 and 5-7).  Exact projections, plane depth stored in millimetres, device poses in another
    world than poses.txt: the two poses come out within 0.05 m of T_0to1 (the bar test_gpu_scannet_routes.py uses for millimetre depth)"""
    S.write_rig_tree(tmp_path)
    cfg = _cfg(tmp_path, "Precomputed")
    model = build_model(cfg)
    res = submission.predict(make_loader(cfg, "val"), model)
    lines = submission.scene_text(res["s00000"]).split("\n")
    assert [l.split(" ")[0] for l in lines] == ["seq1/frame_00003.jpg", "seq1/frame_00007.jpg"]
    sc = list_scenes(cfg, "val")[0]
    for k, line in enumerate(lines):
        f = line.split(" ")
        gt = sc[k]["T_0to1"].numpy().astype(np.float64)
        from mapfree_reloc_amd.evaluation import quat2mat
        er, et = S.pose_error(quat2mat(np.array(f[1:5], np.float64)), np.array(f[5:8], np.float64), gt[:3, :3], gt[:3, 3])
        print(f"{f[0]}: {er:.2e} rad, {et:.2e} m, {f[8]} inliers")
        assert et < 0.05 and er < 0.02 and int(f[8]) > 300                        # 3 frames x 150 exact correspondences
    # a scene without poses_device.txt is an error, not a single-frame solve
    S.write_rig_tree(tmp_path / "nodev", with_device=False)
    cfg2 = _cfg(tmp_path / "nodev", "Precomputed")
    with pytest.raises(MissingDataError, match="poses_device.txt"):
        build_model(cfg2)(next(iter(make_loader(cfg2, "val"))))


def test_multiframe_model_superglue_runs_the_reference_once(tmp_path):
    """synthetic weights: poses mean nothing; the matcher stage must have run SuperPoint on the reference view once for the T = 3 pairs"""
    S.write_rig_tree(tmp_path)
    cfg = _cfg(tmp_path, "SuperGlue")
    model = build_model(cfg)
    data = next(iter(make_loader(cfg, "val")))
    R, t = model(data)
    assert model.stats["reference_views_run"] == 1 and model.stats["reference_views_reused"] == 2
    assert tuple(R.shape) == (1, 3, 3) and tuple(t.shape) == (1, 1, 3) and R.dtype == t.dtype == torch.float32
    assert isinstance(data["inliers"], int)
