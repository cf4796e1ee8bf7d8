"""-m gpu: the rig Procrustes solver (the rig entry point of csrc/procrustes.hip through solver_ops.RigProcrustesBatchSolver) against its two
yardsticks -- the single-frame Procrustes solver, which it must equal bit for bit with one frame and the identity rig, and the numpy mirror
tests/rig_procrustes_ref.py for T > 1 --, the rig essential-matrix solver (csrc/emat_rig.hip: stage 2 against the mirror tests/rig_emat_ref.py
fed with the device's own stage-1 outputs; T = 1 passes stage 1 through), and the multi-frame model with POSE_SOLVER 'RigProcrustes' /
'RigEssentialMatrix' end to end on a written scene.

Bars (those of test_gpu_rig_pnp.py): counts, best index, iters_run, n_valid and masks equal the mirror exactly, with margin > 1e-7 asserted on
the input; the pose is within 1e-4 rad and 1e-4 m of the mirror."""
import glob
import os

import numpy as np
import pytest
import torch

from mapfree_reloc_amd import solver_ops as ops
from mapfree_reloc_amd.builder import build_model
from mapfree_reloc_amd.config import get_cfg_defaults
from mapfree_reloc_amd.datasets import make_loader

import rig_emat_ref as ME
import rig_procrustes_ref as M
import rig_scenes as S
import rig_scenes_depth as D

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ITERS = 256
DIST = D.MAX_CORR_DIST


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _solve(pk, pair_ids, iters=ITERS, seed=2):
    return _np(ops.RigProcrustesBatchSolver(DIST, 0.999, seed, iters)(
        _dev(pk["pts0"]), _dev(pk["pts1"]), _dev(pk["n_corr"]), _dev(pk["depth0"]), _dev(pk["depth1"]), _dev(pk["K0"]), _dev(pk["K1"]),
        _dev(pk["rig_T"]), _dev(np.asarray(pair_ids, np.int64)), want_mask=True, diagnostics=True))


def _mirror(sc, pid, iters=ITERS, seed=2):
    return M.rig_procrustes_solve(sc["pts0"], sc["pts1"], sc["depth0"], sc["depth1"], sc["K0"], sc["K1"], sc["rig_T"], max_dist=DIST,
                                  max_iters=iters, seed=seed, pair_id=int(pid))


def _keep(sc, j, idx):
    """frame j of the scene cut down to the correspondences idx (the depth maps keep the stamps of the others: harmless)"""
    for k in ("pts0", "pts1", "inl"):
        sc[k][j] = sc[k][j][idx]
    return sc


def _valid(sc, j):
    return M.valid_rows(sc["pts0"][j], sc["pts1"][j], sc["depth0"], sc["depth1"][j])


# ---------------------------------------------------------------- T = 1, identity rig: the Procrustes solver itself
@pytest.mark.parametrize("n", [3, 40, 600])
def test_one_frame_identity_rig_equals_procrustes_bit_for_bit(n):
    """n: the fixed sample {0,1,2} (three valid points), one tile, past the 512-point tile"""
    scenes = [D.make_rig_scene(40 + 7 * n + b, 1, max(n, 40)) for b in range(3)]
    if n == 3:
        scenes = [_keep(sc, 0, [i for i in _valid(sc, 0) if sc["inl"][0][i]][:3]) for sc in scenes]     # three valid TRUE correspondences
    pk = D.pack(scenes)
    assert np.array_equal(pk["rig_T"], np.tile(np.eye(4), (3, 1, 1, 1)))
    pids = np.array([5, 70000, 123456789012], np.int64)
    a = _np(ops.ProcrustesBatchSolver(DIST, 0.999, 9, ITERS)(
        _dev(pk["pts0"][:, 0]), _dev(pk["pts1"][:, 0]), _dev(pk["n_corr"][:, 0]), _dev(pk["depth0"]), _dev(pk["depth1"][:, 0]), _dev(pk["K0"]),
        _dev(pk["K1"][:, 0]), _dev(pids), diagnostics=True))
    b = _solve(pk, pids, seed=9)
    for k in ("counts", "best_iter", "iters_run", "status", "n_inliers", "R", "t"):
        assert np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), k
    assert (a["status"] == 0).all() and (b["mask"].sum((1, 2)) == b["n_inliers"]).all()
    if n == 3:
        assert b["n_valid"].tolist() == [[3]] * 3 and b["n_inliers"].tolist() == [3] * 3
    else:
        assert (b["n_valid"][:, 0] > (512 if n == 600 else 16)).all() and (b["n_inliers"] > 3).all()   # real poses were compared


# ---------------------------------------------------------------- T > 1 against the mirror
def _scenes(case):
    mk = lambda k, T, ns, **kw: D.make_rig_scene(300 + 11 * k + len(case), T, ns, **kw)
    if case == "plain_T2":
        return [mk(0, 2, [40, 40])]
    if case == "plain_T9":
        return [mk(0, 9, [30] * 9)]
    if case == "frame_with_0_points":
        return [mk(0, 3, [40, 0, 30])]
    if case == "tile_boundary_inside_a_frame":               # the pooled list passes 512 points inside frame 1
        sc = mk(0, 2, [550, 550])
        assert len(_valid(sc, 0)) < 512 < len(_valid(sc, 0)) + len(_valid(sc, 1))
        return [sc]
    if case == "tile_boundary_at_a_frame_boundary":          # frame 0 holds exactly 512 valid points: frame 1 opens the second tile
        sc = mk(0, 2, [1100, 60])
        return [_keep(sc, 0, np.arange(_valid(sc, 0)[511] + 1))]
    if case == "pooled_N_3":                                 # 2 + 1 valid true correspondences: the fixed sample over two frames
        sc = mk(0, 2, [40, 40], outlier_frac=0.0)
        return [_keep(_keep(sc, 0, _valid(sc, 0)[:2]), 1, _valid(sc, 1)[:1])]
    if case == "too_few":
        return [mk(0, 2, [1, 1])]
    if case == "bad_depth":
        return [mk(0, 2, [10, 10], zero_query_depth=True)]
    if case == "mixed_B3":
        return [mk(b, 9, ns) for b, ns in enumerate([[25] * 9, [0, 4, 3, 6, 0, 4, 1, 0, 2], [1, 0, 0, 0, 1, 0, 0, 0, 0]])]
    if case == "T16":
        return [mk(0, 16, [12] * 16)]
    raise KeyError(case)


CASES = ["plain_T2", "plain_T9", "frame_with_0_points", "tile_boundary_inside_a_frame", "tile_boundary_at_a_frame_boundary", "pooled_N_3",
         "too_few", "bad_depth", "mixed_B3", "T16"]


@pytest.mark.parametrize("case", CASES)
def test_rig_procrustes_against_mirror(case):
    scenes = _scenes(case)
    pk = D.pack(scenes)
    B, T = len(scenes), scenes[0]["T"]
    pids = np.array([17, 4242, 99][:B], np.int64)
    got = _solve(pk, pids)
    worst = [0.0, 0.0]
    for b, sc in enumerate(scenes):
        ref = _mirror(sc, pids[b])
        assert got["n_valid"][b].tolist() == ref["n_valid"]
        assert got["status"][b] == ref["status"], (b, got["status"][b], ref["status"])
        if ref["status"] != M.OK:
            assert np.isnan(got["R"][b]).all() and np.isnan(got["t"][b]).all() and got["n_inliers"][b] == 0 and not got["mask"][b].any()
            continue
        assert ref["margin"] > 1e-7, "a point of this seeded input sits on the threshold: pick another seed"
        run = ref["iters_run"]
        assert got["iters_run"][b] == run and got["best_iter"][b] == ref["best_iter"]
        assert np.array_equal(got["counts"][b, :run], ref["counts"][:run]), np.flatnonzero(got["counts"][b, :run] != ref["counts"][:run])[:5]
        assert got["n_inliers"][b] == ref["n_inl"]
        for j in range(T):
            nc = len(sc["pts0"][j])
            assert np.array_equal(got["mask"][b, j, :nc].astype(bool), ref["masks_orig"][j]) and not got["mask"][b, j, nc:].any()
        er, et = S.pose_error(got["R"][b], got["t"][b], ref["R"], ref["t"])
        worst = [max(worst[0], er), max(worst[1], et)]
        assert er < 1e-4 and et < 1e-4, (er, et)
    print(f"{case}: device vs mirror, max {worst[0]:.3e} rad, {worst[1]:.3e} m")
    st = got["status"].tolist()
    if case == "too_few":
        assert st == [M.TOO_FEW]
    elif case == "bad_depth":
        assert st == [M.BAD_DEPTH]
    elif case == "mixed_B3":
        assert st[0] == M.OK and st[2] == M.TOO_FEW
    else:
        assert st == [M.OK] and got["n_inliers"][0] >= 3
    if case == "tile_boundary_at_a_frame_boundary":
        assert got["n_valid"][0, 0] == 512
    if case == "pooled_N_3":
        assert got["n_valid"][0].tolist() == [2, 1] and got["n_inliers"][0] == 3


def test_repeatable_and_follows_pair_ids():
    scenes = [D.make_rig_scene(500 + b, 3, [50, 45, 40]) for b in range(3)]
    pk = D.pack(scenes)
    pids = np.array([3, 1000, 77], np.int64)
    a, b = _solve(pk, pids), _solve(pk, pids)
    perm = [2, 0, 1]
    c = _solve({k: v[perm] for k, v in pk.items()}, pids[perm])
    assert (a["status"] == 0).all() and (a["n_inliers"] > 10).all()
    for k in a:
        assert np.array_equal(a[k], b[k]), k
        assert np.array_equal(a[k][perm], c[k]), k
    d = _solve(pk, pids + 1)                                                     # another pair id draws other samples
    assert not np.array_equal(a["counts"], d["counts"])


# ---------------------------------------------------------------- the essential-matrix rig solver
E_ITERS, PIX = 400, 2.0


def _emat_stage1(pk, pids, seed=4):
    return ops.rig_emat_stage1(ops.EssentialBatchSolver(PIX, 0.9999, seed, E_ITERS), _dev(pk["pts0"]), _dev(pk["pts1"]), _dev(pk["n_corr"]),
                               _dev(pk["K0"]), _dev(pk["K1"]), _dev(np.asarray(pids, np.int64)))


def _emat_stage2(pk, s1):
    return _np(ops.rig_emat_stage2(_dev(pk["pts0"]), _dev(pk["pts1"]), _dev(pk["n_corr"]), _dev(pk["K0"]), _dev(pk["K1"]), _dev(pk["rig_T"]), s1,
                                   PIX, want_mask=True, diagnostics=True))


def _emat_mirror(sc, s1, b):
    T = sc["T"]
    return ME.rig_emat_stage2(sc["pts0"], sc["pts1"], sc["K0"], sc["K1"], sc["rig_T"], s1["R"][b], s1["t"][b], s1["n_inliers"][b], s1["status"][b],
                              [s1["mask"][b, j, :len(sc["pts0"][j])].astype(bool) for j in range(T)], pix_thr=PIX)


def _zero_baseline():
    """two frames with the same rig pose, intrinsics and (noise-free) correspondences: both bearings point the same way, det M = 2 sin^2 ~ 0"""
    sc = S.make_rig_scene(350, 2, [120, 120], noise_px=0.0)
    sc["rig_T"][0] = np.eye(4); sc["K1"][0] = sc["K1"][1]
    for k in ("pts0", "pts1", "inl"):
        sc[k][0] = sc[k][1].copy()
    return sc


def _emat_scenes(case):
    mk = lambda k, T, ns, **kw: S.make_rig_scene(600 + 13 * k + len(case), T, ns, **kw)
    return {"T1": lambda: [mk(b, 1, 150) for b in range(2)],
            "T2_one_pair": lambda: [mk(0, 2, [120, 120])],
            "T9_72_hypotheses": lambda: [mk(0, 9, [60] * 9)],
            "one_frame_with_3_correspondences": lambda: [mk(0, 3, [100, 3, 100])],
            "one_usable_frame_of_three": lambda: [mk(0, 3, [100, 3, 2])],
            "zero_baseline": lambda: [_zero_baseline()],
            # (seed index 1: the rig of index 0 has a baseline of 1.1 cm, its two bearings 0.5 degrees apart: rightly skipped, nothing to score)
            "frame_past_the_1024_tile": lambda: [mk(1, 2, [1100, 80])],
            "mixed_B3": lambda: [mk(0, 3, [80, 80, 80]), mk(1, 3, [100, 3, 2]), mk(2, 3, [60, 0, 60])]}[case]()


EMAT_CASES = ["T1", "T2_one_pair", "T9_72_hypotheses", "one_frame_with_3_correspondences", "one_usable_frame_of_three", "zero_baseline",
              "frame_past_the_1024_tile", "mixed_B3"]


@pytest.mark.parametrize("case", EMAT_CASES)
def test_rig_emat_stage2_against_mirror(case):
    scenes = _emat_scenes(case)
    pk = S.pack(scenes, maxN=max(max(len(p) for s in scenes for p in s["pts0"]), 8))
    B, T = len(scenes), scenes[0]["T"]
    pids = np.array([17, 4242, 99][:B], np.int64)
    s1d = _emat_stage1(pk, pids)
    got, s1 = _emat_stage2(pk, s1d), _np(s1d)
    if case == "T1":                                                             # stage 1 passes through bit for bit
        assert (s1["status"] == 0).all()
        for k in ("R", "t", "n_inliers", "status", "mask"):
            assert np.array_equal(got[k], s1[k][:, 0] if k != "mask" else s1[k]), k
        assert (got["best_hyp"] == -1).all() and np.abs(np.linalg.norm(got["t"], axis=1) - 1.0).max() < 1e-12
    worst = [0.0, 0.0]
    for b, sc in enumerate(scenes):
        ref = _emat_mirror(sc, s1, b)
        assert got["status"][b] == ref["status"], (b, got["status"][b], ref["status"])
        if T > 1:
            assert np.array_equal(got["hyp_counts"][b], ref["hyp_counts"]), np.flatnonzero(got["hyp_counts"][b] != ref["hyp_counts"])[:5]
            assert got["best_hyp"][b] == ref["best_hyp"]
        if ref["status"] != ME.OK:
            assert np.isnan(got["R"][b]).all() and np.isnan(got["t"][b]).all() and got["n_inliers"][b] == 0 and not got["mask"][b].any()
            continue
        if T > 1:
            assert ref["margin"] > 1e-7, "a point of this seeded input sits on the threshold: pick another seed"
        assert got["n_inliers"][b] == ref["n_inl"]
        for j in range(T):
            nc = len(sc["pts0"][j])
            assert np.array_equal(got["mask"][b, j, :nc].astype(bool), ref["masks"][j]) and not got["mask"][b, j, nc:].any()
        er, et = S.pose_error(got["R"][b], got["t"][b], ref["R"], ref["t"])
        worst = [max(worst[0], er), max(worst[1], et)]
        assert er < 1e-4 and et < 1e-4, (er, et)
        if T > 1:
            gr, gt = S.pose_error(got["R"][b], got["t"][b], sc["R"], sc["t"])
            print(f"  sample {b}: device vs truth {gr:.3e} rad {gt:.3e} m (|t| = {np.linalg.norm(sc['t']):.2f} m), {got['n_inliers'][b]} inliers")
    print(f"{case}: device vs mirror, max {worst[0]:.3e} rad, {worst[1]:.3e} m")
    st = got["status"].tolist()
    if case in ("one_usable_frame_of_three", "zero_baseline"):
        assert st == [ME.NO_MODEL]
        if case == "zero_baseline":
            assert (s1["status"] == 0).all() and (got["hyp_counts"][0] == -1).all()      # both frames usable, every hypothesis skipped
    elif case == "mixed_B3":
        assert st == [ME.OK, ME.NO_MODEL, ME.OK] and s1["status"][2].tolist() == [0, ME.TOO_FEW, 0]
    else:
        assert st == [ME.OK] * B
    if case == "T9_72_hypotheses":
        assert (got["hyp_counts"][0] >= 0).sum() > 64                            # past one wavefront of hypotheses
    if case == "one_frame_with_3_correspondences":
        assert s1["status"][0].tolist() == [0, ME.TOO_FEW, 0] and (got["hyp_counts"][0, 2:] == -1).all() and got["mask"][0, 1].sum() <= 3


def test_rig_emat_both_stages_chained_equal_the_two_calls():
    scenes = [S.make_rig_scene(700 + b, 3, [90, 80, 70]) for b in range(3)]
    pk = S.pack(scenes)
    pids = np.array([3, 1000, 77], np.int64)
    two = _emat_stage2(pk, _emat_stage1(pk, pids))
    one = _np(ops.RigEssentialBatchSolver(PIX, 0.9999, 4, E_ITERS)(
        _dev(pk["pts0"]), _dev(pk["pts1"]), _dev(pk["n_corr"]), _dev(pk["K0"]), _dev(pk["K1"]), _dev(pk["rig_T"]), _dev(pids), want_mask=True,
        diagnostics=True))
    assert (one["status"] == 0).all() and (one["n_inliers"] > 100).all()
    for k in one:
        assert np.array_equal(one[k], two[k]), k


# ---------------------------------------------------------------- end to end
def _cfg(root, solver="RigProcrustes"):
    cfg = get_cfg_defaults()
    cfg.MODEL, cfg.FEATURE_MATCHING, cfg.POSE_SOLVER = "FeatureMatchingMultiFrame", "Precomputed", solver
    cfg.EMAT_RANSAC.PIX_THRESHOLD, cfg.EMAT_RANSAC.SCALE_THRESHOLD, cfg.EMAT_RANSAC.CONFIDENCE = PIX, 0.1, 0.9999
    cfg.MATCHES_FILE_PATH = "{scene_root}/correspondences_exact.npz"
    cfg.PROCRUSTES.MAX_CORR_DIST = DIST
    cfg.DATASET.DATA_ROOT, cfg.DATASET.HEIGHT, cfg.DATASET.WIDTH, cfg.DATASET.ESTIMATED_DEPTH = str(root), S.TREE_H, S.TREE_W, "dptkitti"
    cfg.DATASET.QUERY_FRAME_COUNT = 3
    cfg.ALLOW_SYNTHETIC_WEIGHTS = True
    return cfg


def test_multiframe_model_rig_procrustes_end_to_end(tmp_path):
    """8 seq1 frames, T = 3: two samples (windows 1-3 and 5-7), exact projections, query depth PNGs consistent with the geometry
    (rig_scenes_depth.write_rig_tree), millimetre depth.  The model's pose is the mirror's on the sample's own tensors (within the bars above;
    the model returns float32).  The mirror's own error against T_0to1, printed below, is the lift's integer truncation of the query pixel:
    measured 5.9e-4 / 5.5e-4 rad and 1.81e-2 / 1.82e-2 m on the two samples (the truncation moves every query point the same way, by up to a
    pixel = 2-3 cm at this depth, and the translation takes that bias)."""
    tree = D.write_rig_tree(tmp_path)
    cfg = _cfg(tmp_path)
    model = build_model(cfg)
    rows = np.load(os.path.join(tree["scene_root"], "correspondences_exact.npz"))["correspondences"].astype(np.float32)
    n = 0
    for data in make_loader(cfg, "val"):
        frames = [int(os.path.basename(p)[6:11]) for p in data["pair_names"][1][0]]
        R, t = model(data)
        ref = M.rig_procrustes_solve([rows[f][:, :2] for f in frames], [rows[f][:, 2:] for f in frames], data["depth0"][0].numpy(),
                                     data["depth1"][0].numpy(), data["K_color0"][0].numpy(), data["K_color1_multi"][0].numpy(),
                                     data["rig_T"][0].numpy(), max_dist=DIST, pair_id=int(data["pair_id"][0]))
        gt = data["T_0to1"][0].numpy().astype(np.float64)
        er, et = S.pose_error(R[0].numpy(), t[0, 0].numpy(), ref["R"], ref["t"])
        gr, gtt = S.pose_error(ref["R"], ref["t"], gt[:3, :3], gt[:3, 3])
        print(f"frames {frames}: device vs mirror {er:.3e} rad {et:.3e} m; mirror vs truth {gr:.3e} rad {gtt:.3e} m; {data['inliers']} inliers")
        assert ref["status"] == M.OK and ref["margin"] > 1e-7
        assert er < 1e-4 and et < 1e-4 and data["inliers"] == ref["n_inl"] > 300       # 3 frames x 150 exact correspondences
        n += 1
    assert n == 2


def test_multiframe_model_rig_procrustes_online_depth(tmp_path):
    """DPT.SOURCE 'online' (the reduced DPT of test_gpu_dpt._stage_cfg at 64 x 96 on the 120 x 160 tree, perturbed synthetic weights: poses mean
    nothing): the depth stage ran T + 1 views for one sample -- the reference view once and the T window frames -- and no depth file was read"""
    import dpt_ref
    from mapfree_reloc_amd.datasets import clear_frame_cache
    from mapfree_reloc_amd.nets import weights as WT
    from test_gpu_dpt import _stage_cfg
    D.write_rig_tree(tmp_path / "tree")
    cfg = _stage_cfg(tmp_path / "tree", tmp_path, dpt_ref.perturbed(WT.dpt_state_dict(arch=dpt_ref.REDUCED)), "online", "dptkitti")
    cfg.MODEL, cfg.POSE_SOLVER, cfg.DATASET.QUERY_FRAME_COUNT = "FeatureMatchingMultiFrame", "RigProcrustes", 3
    cfg.PROCRUSTES.MAX_CORR_DIST = DIST
    model = build_model(cfg)
    data = next(iter(make_loader(cfg, "val")))
    for f in glob.glob(os.path.join(str(tmp_path / "tree"), "**", "*.dptkitti.png"), recursive=True):
        os.rename(f, f + ".away")                              # from here on whoever opens a depth file fails
    clear_frame_cache()
    R, t = model(data)
    assert model.depth.stats["depth_views_run"] == 4 and model.depth.stats["depth_views_reused"] == 0
    assert tuple(data["depth0"].shape) == (1, S.TREE_H, S.TREE_W) and tuple(data["depth1"].shape) == (1, 3, S.TREE_H, S.TREE_W)
    assert data["depth0"].is_cuda and data["depth1"].is_cuda
    assert tuple(R.shape) == (1, 3, 3) and tuple(t.shape) == (1, 1, 3) and isinstance(data["inliers"], int)


def test_multiframe_model_rig_emat_end_to_end_without_depth_files(tmp_path):
    """the same tree with every depth PNG deleted and DATASET.ESTIMATED_DEPTH None: 'RigEssentialMatrix' reads no depth.  The model's pose is
    the mirror's on the device's own stage-1 outputs for the sample (within the bars above; float32 out).  The mirror's error against T_0to1
    is printed: the window's baselines are at most 0.2 m (rig_scenes.write_rig_tree), the pose's translation 0.8 m."""
    tree = S.write_rig_tree(tmp_path)
    for f in glob.glob(os.path.join(tree["scene_root"], "**", "*.png"), recursive=True):
        os.remove(f)
    cfg = _cfg(tmp_path, "RigEssentialMatrix")
    cfg.DATASET.ESTIMATED_DEPTH = None
    model = build_model(cfg)
    assert model.depth is None
    rows = np.load(os.path.join(tree["scene_root"], "correspondences_exact.npz"))["correspondences"].astype(np.float32)
    n = 0
    for data in make_loader(cfg, "val"):
        frames = [int(os.path.basename(p)[6:11]) for p in data["pair_names"][1][0]]
        R, t = model(data)
        p0, p1 = np.stack([rows[f][:, :2] for f in frames])[None], np.stack([rows[f][:, 2:] for f in frames])[None]
        s1 = _np(ops.rig_emat_stage1(ops.EssentialBatchSolver(PIX, 0.9999, 0), _dev(p0), _dev(p1), _dev(np.full((1, 3), p0.shape[2], np.int32)),
                                     data["K_color0"].to(DEV), data["K_color1_multi"].to(DEV), data["pair_id"].to(DEV, torch.int64).reshape(1)))
        ref = ME.rig_emat_stage2(list(p0[0]), list(p1[0]), data["K_color0"][0].numpy(), data["K_color1_multi"][0].numpy(), data["rig_T"][0].numpy(),
                                 s1["R"][0], s1["t"][0], s1["n_inliers"][0], s1["status"][0], [m.astype(bool) for m in s1["mask"][0]], pix_thr=PIX)
        gt = data["T_0to1"][0].numpy().astype(np.float64)
        er, et = S.pose_error(R[0].numpy(), t[0, 0].numpy(), ref["R"], ref["t"])
        gr, gtt = S.pose_error(ref["R"], ref["t"], gt[:3, :3], gt[:3, 3])
        print(f"frames {frames}: device vs mirror {er:.3e} rad {et:.3e} m; mirror vs truth {gr:.3e} rad {gtt:.3e} m; {data['inliers']} inliers")
        assert ref["status"] == ME.OK and ref["margin"] > 1e-7
        assert er < 1e-4 and et < 1e-4 and data["inliers"] == ref["n_inl"] > 300       # 3 frames x 150 exact correspondences
        n += 1
    assert n == 2
