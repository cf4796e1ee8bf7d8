"""CPU tests of the rig Procrustes and rig essential-matrix solvers (POSE_SOLVER 'RigProcrustes' / 'RigEssentialMatrix'): the numpy mirrors
tests/rig_procrustes_ref.py and tests/rig_emat_ref.py on the seeded rigs of tests/rig_scenes_depth.py / tests/rig_scenes.py, the builder's
solver names, and the argument checks of the C-ABI entry points."""
import numpy as np
import pytest

import mapfree_reloc_amd as mfr
from mapfree_reloc_amd.builder import build_model
from mapfree_reloc_amd.config import get_cfg_defaults
from oracle import oracle_lib as O

import rig_emat_ref as ME
import rig_procrustes_ref as M
import rig_scenes as S
import rig_scenes_depth as D


def _solve(sc, frames=slice(None), **kw):
    kw.setdefault("max_dist", D.MAX_CORR_DIST)
    return M.rig_procrustes_solve(sc["pts0"][frames], sc["pts1"][frames], sc["depth0"], sc["depth1"][frames], sc["K0"], sc["K1"][frames],
                                  sc["rig_T"][frames], **kw)


def _true_kept(sc, r, frames=slice(None)):
    """(true correspondences the model keeps as inliers, true correspondences) over the frames solved"""
    kept = sum(int((m & g).sum()) for m, g in zip(r["masks_orig"], sc["inl"][frames]))
    return kept, sum(int(g.sum()) for g in sc["inl"][frames])


# ---------------------------------------------------------------- the mirror
def test_mirror_one_frame_identity_rig_is_the_oracle():
    """T = 1, identity rig: Q' = Q, the pooled list is the frame's list, and the mirror's counts, best iteration, inlier count and pose are the
    oracle's Procrustes solver's -- from lifted points and from raw correspondences"""
    for seed, n in ((5, 200), (6, 40), (7, 3), (8, 2)):
        sc = D.make_rig_scene(seed, 1, n)
        assert np.array_equal(sc["rig_T"][0], np.eye(4))
        r = _solve(sc, max_iters=64, seed=3, pair_id=11)
        P, Q = O.procrustes_lift(sc["pts0"][0], sc["pts1"][0], sc["depth0"], sc["depth1"][0], sc["K0"], sc["K1"][0])
        assert np.array_equal(r["P"], P) and np.array_equal(r["Q"], Q) and r["n_valid"] == [len(P)]
        st, R, t, n_inl = O.procrustes_solve(sc["pts0"][0], sc["pts1"][0], sc["depth0"], sc["depth1"][0], sc["K0"], sc["K1"][0],
                                             max_dist=D.MAX_CORR_DIST, max_iters=64, seed=3, pair_id=11)
        assert r["status"] == st and r["n_inl"] == n_inl
        assert np.array_equal(r["R"], R, equal_nan=True) and np.array_equal(r["t"], t.reshape(3), equal_nan=True)
        if st == O.ST_OK:
            ref = O.procrustes_ransac(P, Q, D.MAX_CORR_DIST, 0.999, 64, 3, 11, want_counts=True)
            assert r["best_iter"] == ref["best_iter"] and r["iters_run"] == ref["iters_run"] and np.array_equal(r["counts"], ref["counts"])
            assert sum(int(m.sum()) for m in r["masks_orig"]) == n_inl            # the inlier set: as many points as the oracle counts ...
            d = M.dist2(R, t, P, Q)                                               # ... and they are the points within the threshold
            idx = M.valid_rows(sc["pts0"][0], sc["pts1"][0], sc["depth0"], sc["depth1"][0])
            assert np.array_equal(np.flatnonzero(r["masks_orig"][0]), idx[d < D.MAX_CORR_DIST ** 2])
    assert _solve(D.make_rig_scene(8, 1, 2))["status"] == M.TOO_FEW


# measured when the seeds were fixed (noise_px = 0: what is left is the lift's integer truncation of the query pixel, up to 1 px * Z / f):
#   T = 2: 2.61e-3 rad, 9.18e-3 m      T = 9: 4.03e-3 rad, 2.31e-3 m.   The bars are twice the measured values.
NOISE_FREE_BARS = {2: (5.3e-3, 1.9e-2), 9: (8.1e-3, 4.7e-3)}


@pytest.mark.parametrize("T", [2, 9])
def test_mirror_recovers_noise_free_pose(T):
    sc = D.make_rig_scene(100 + T, T, 80, noise_px=0.0)
    r = _solve(sc)
    er, et = S.pose_error(r["R"], r["t"], sc["R"], sc["t"])
    kept, true = _true_kept(sc, r)
    print(f"T={T}: {er:.3e} rad, {et:.3e} m, {r['n_inl']} inliers, {kept} of {true} true correspondences kept")
    assert r["status"] == M.OK and er < NOISE_FREE_BARS[T][0] and et < NOISE_FREE_BARS[T][1]
    assert 2 * kept >= true


NOISY_SEEDS = range(1000, 1032)


def noisy_errors():
    """per seed: (rotation, translation) error of the 9-frame rig solve and of the same solver on the last frame alone"""
    e9, e1 = [], []
    for seed in NOISY_SEEDS:
        sc = D.make_rig_scene(seed, 9, 60)
        a, b = _solve(sc, pair_id=seed), _solve(sc, slice(8, 9), pair_id=seed)
        assert a["status"] == M.OK and b["status"] == M.OK
        for r, fr in ((a, slice(None)), (b, slice(8, 9))):                         # the helper's noise and MAX_CORR_DIST keep the problem well posed
            kept, true = _true_kept(sc, r, fr)
            assert 2 * kept >= true, (seed, kept, true)
        e9.append(S.pose_error(a["R"], a["t"], sc["R"], sc["t"])); e1.append(S.pose_error(b["R"], b["t"], sc["R"], sc["t"]))
    return np.array(e9), np.array(e1)


def test_mirror_nine_frames_not_worse_than_the_last_frame_alone():
    """32 seeded rigs, 60 correspondences per frame, 0.5 px noise, 30 % outliers, MAX_CORR_DIST 0.1 m: the median translation error of the
    pooled T = 9 solve must not be above that of Procrustes on the last frame alone.  Measured when the seeds were fixed: 0.0079 m (T = 9)
    against 0.0123 m (last frame alone); rotation 0.0032 rad against 0.0042 rad."""
    e9, e1 = noisy_errors()
    m9, m1 = np.median(e9, 0), np.median(e1, 0)
    print(f"median error: T=9 {m9[0]:.4f} rad {m9[1]:.4f} m, last frame alone {m1[0]:.4f} rad {m1[1]:.4f} m")
    assert m9[1] <= m1[1]


# ---------------------------------------------------------------- the essential-matrix rig mirror
def emat_stage1_oracle(sc, pair_id, iters=1000):
    """stage 1 from the ORACLE's single-frame E-matrix solver (its binding offers one: oracle_lib.emat_solve), frame j keyed pair_id T + j"""
    T = sc["T"]
    r = [O.emat_solve(sc["pts0"][j], sc["pts1"][j], sc["K0"], sc["K1"][j], 2.0, 0.9999, iters, 0, pair_id * T + j) for j in range(T)]
    return dict(R1=[x["R"] for x in r], t1=[x["t"] for x in r], n1=[x["n_inl"] for x in r], st1=[x["status"] for x in r],
                mask1=[x["mask"].astype(bool) for x in r])


def emat_solve(sc, pair_id=0):
    return ME.rig_emat_stage2(sc["pts0"], sc["pts1"], sc["K0"], sc["K1"], sc["rig_T"], pix_thr=2.0, **emat_stage1_oracle(sc, pair_id))


# measured when the seeds were fixed (noise_px = 0, 30 % outliers; a random outlier lies within 2 px of its epipolar line a few per cent of
# the time and is then an inlier of the Sampson test, and the scale hangs on baselines of at most 0.3 m against 4 m of depth):
#   T = 2: 5.93e-3 rad, 6.04e-3 m      T = 9: 3.84e-3 rad, 1.23e-2 m.   The bars are twice the measured values.
EMAT_NOISE_FREE_BARS = {2: (1.2e-2, 1.3e-2), 9: (7.7e-3, 2.5e-2)}


@pytest.mark.parametrize("T", [2, 9])
def test_emat_mirror_recovers_noise_free_metric_pose(T):
    """no depth map is read: the rig's baselines alone give the translation its length"""
    sc = S.make_rig_scene(100 + T, T, 80, noise_px=0.0)
    r = emat_solve(sc)
    er, et = S.pose_error(r["R"], r["t"], sc["R"], sc["t"])
    print(f"T={T}: {er:.3e} rad, {et:.3e} m (|t| = {np.linalg.norm(sc['t']):.3f} m), {r['n_inl']} inliers, hypothesis {r['best_hyp']} of {T * (T - 1)}")
    assert r["status"] == ME.OK and er < EMAT_NOISE_FREE_BARS[T][0] and et < EMAT_NOISE_FREE_BARS[T][1]
    assert r["n_inl"] >= int(0.6 * 80 * T)
    assert (r["hyp_counts"] >= 0).sum() > 0 and r["hyp_counts"][r["best_hyp"]] == r["hyp_counts"].max()


def test_emat_mirror_status_rules():
    sc = S.make_rig_scene(7, 3, [80, 3, 2])                                       # one usable frame of three
    r = emat_solve(sc)
    assert r["status"] == ME.NO_MODEL and np.isnan(r["R"]).all() and r["n_inl"] == 0
    sc = S.make_rig_scene(8, 3, [3, 3, 2])                                        # none usable, all TOO_FEW
    assert emat_solve(sc)["status"] == ME.TOO_FEW
    sc = S.make_rig_scene(9, 1, 80)                                               # T = 1: stage 1 passes through
    s1 = emat_stage1_oracle(sc, 0)
    r = emat_solve(sc)
    assert r["status"] == s1["st1"][0] == ME.OK and np.array_equal(r["R"], s1["R1"][0]) and np.array_equal(r["t"], s1["t1"][0])
    assert r["n_inl"] == s1["n1"][0] and np.array_equal(r["masks"][0], s1["mask1"][0])
    assert abs(np.linalg.norm(r["t"]) - 1.0) < 1e-12                              # no rig, no scale: the unit translation


# ---------------------------------------------------------------- builder
def _cfg(root, model, solver):
    cfg = get_cfg_defaults()
    cfg.MODEL, cfg.FEATURE_MATCHING, cfg.POSE_SOLVER = model, "Precomputed", solver
    cfg.MATCHES_FILE_PATH = "{scene_root}/correspondences_exact.npz"
    cfg.PNP.RANSAC_ITER, cfg.PNP.REPROJECTION_INLIER_THRESHOLD, cfg.PNP.CONFIDENCE = 1000, 3, 0.9999
    cfg.PROCRUSTES.MAX_CORR_DIST = D.MAX_CORR_DIST
    cfg.EMAT_RANSAC.PIX_THRESHOLD, cfg.EMAT_RANSAC.SCALE_THRESHOLD, cfg.EMAT_RANSAC.CONFIDENCE = 2.0, 0.1, 0.9999
    cfg.DATASET.DATA_ROOT, cfg.DATASET.HEIGHT, cfg.DATASET.WIDTH, cfg.DATASET.ESTIMATED_DEPTH = str(root), S.TREE_H, S.TREE_W, "dptkitti"
    cfg.DATASET.QUERY_FRAME_COUNT = 3
    return cfg


@pytest.mark.parametrize("solver", ["RigPNP", "RigProcrustes", "RigEssentialMatrix"])
def test_builder_accepts_the_rig_names_under_the_multi_frame_model_only(tmp_path, solver):
    """the name passes the multi-frame model's solver check: the model is built where there is a GPU, and without one the next thing to
    fail is the library's own 'no HIP device' -- not the NotImplementedError of an unknown solver"""
    try:
        model = build_model(_cfg(tmp_path, "FeatureMatchingMultiFrame", solver))
    except mfr._lib.MfrLibraryError as e:
        assert "no HIP device" in str(e)
    else:
        assert model.kind == {"RigPNP": "PNP", "RigProcrustes": "Procrustes", "RigEssentialMatrix": "EssentialMatrix"}[solver]
        assert (model.depth is None)                                             # DPT.SOURCE 'file': nobody builds a depth stage
    with pytest.raises(NotImplementedError, match="Invalid pose solver"):
        build_model(_cfg(tmp_path, "FeatureMatching", solver))


def test_rig_procrustes_refuses_icp_refinement(tmp_path):
    cfg = _cfg(tmp_path, "FeatureMatchingMultiFrame", "RigProcrustes")
    cfg.PROCRUSTES.REFINE = True
    with pytest.raises(NotImplementedError, match="PROCRUSTES.REFINE"):
        build_model(cfg)


# ---------------------------------------------------------------- C-ABI
def test_rig_procrustes_entry_points_exported_and_reject_bad_arguments():
    """wrong arguments return a status before anything is launched (so this runs without a GPU: no pointer is ever dereferenced)"""
    lib = mfr._lib.load()
    for n in ("mfr_rig_procrustes_workspace_bytes", "mfr_rig_procrustes_solve_batch"):
        assert hasattr(lib, n) and n in mfr._lib.SIGNATURES
    ws = lib.mfr_rig_procrustes_workspace_bytes
    assert ws(2, 9, 1024, 1000) > ws(2, 1, 1024, 1000) >= lib.mfr_procrustes_workspace_bytes(2, 1024, 1000) > 0
    assert ws(2, 0, 1024, 1000) == 0 and ws(2, 17, 1024, 1000) == 0 and ws(0, 3, 1024, 1000) == 0 and ws(2, 3, 0, 1000) == 0
    buf = np.zeros(64)
    p = buf.ctypes.data                                        # a valid host address standing in for every pointer: never read

    def solve(T=3, B=2, maxN=8, null=None, ws_bytes=0, dist=0.1):
        a = [p, p, p, B, T, maxN, p, p, 4, 4, p, p, 1, p, dist, 0.999, 10, 0, p, p, ws_bytes, p, p, p, p, None, None, None, None, None, None]
        if null is not None:
            a[null] = None
        return lib.mfr_rig_procrustes_solve_batch(*a)
    E_ARG, E_WS = -1, -3
    for T in (0, -1, 17):
        assert solve(T=T) == E_ARG
    assert solve(B=0) == E_ARG and solve(maxN=0) == E_ARG and solve(dist=0.0) == E_ARG
    for k in (0, 1, 2, 6, 7, 10, 11, 13, 18, 19, 21, 22, 23, 24):   # pts0, pts1, n_corr, depth0, depth1, K0, K1, rig, pair_ids, workspace, R, t, n_inliers, status
        assert solve(null=k) == E_ARG, k
    assert solve(ws_bytes=ws(2, 3, 8, 10) - 1) == E_WS         # a workspace one byte short


def test_rig_emat_entry_points_exported_and_reject_bad_arguments():
    lib = mfr._lib.load()
    for n in ("mfr_rig_emat_workspace_bytes", "mfr_rig_emat_solve", "mfr_rig_emat_batch_workspace_bytes", "mfr_rig_emat_solve_batch"):
        assert hasattr(lib, n) and n in mfr._lib.SIGNATURES
    ws, wsb = lib.mfr_rig_emat_workspace_bytes, lib.mfr_rig_emat_batch_workspace_bytes
    assert ws(2, 9, 1024) > ws(2, 2, 1024) > 0 and ws(2, 1, 1024) > 0
    assert ws(2, 0, 1024) == 0 and ws(2, 17, 1024) == 0 and ws(0, 3, 1024) == 0 and ws(2, 3, 0) == 0
    assert wsb(2, 9, 1024, 1000) > ws(2, 9, 1024) + lib.mfr_emat_workspace_bytes(18, 1024, 1000) and wsb(2, 17, 8, 10) == 0 and wsb(2, 0, 8, 10) == 0
    buf = np.zeros(64)
    p = buf.ctypes.data                                        # a valid host address standing in for every pointer: never read

    def stage2(T=3, B=2, maxN=8, null=None, ws_bytes=0, thr=2.0):
        a = [p, p, p, B, T, maxN, p, p, 1, p, thr, p, p, p, p, p, p, ws_bytes, p, p, p, p, None, None, None, None]
        if null is not None:
            a[null] = None
        return lib.mfr_rig_emat_solve(*a)

    def batch(T=3, B=2, maxN=8, null=None, ws_bytes=0, thr=2.0):
        a = [p, p, p, B, T, maxN, p, p, 1, p, thr, 0.9999, 10, 0, p, 1, None, 2048, 1.0, p, ws_bytes, p, p, p, p, None, None, None, None]
        if null is not None:
            a[null] = None
        return lib.mfr_rig_emat_solve_batch(*a)
    E_ARG, E_WS = -1, -3
    for T in (0, -1, 17):
        assert stage2(T=T) == E_ARG and batch(T=T) == E_ARG
    assert stage2(B=0) == E_ARG and stage2(maxN=0) == E_ARG and stage2(thr=0.0) == E_ARG and batch(B=0) == E_ARG and batch(thr=0.0) == E_ARG
    for k in (0, 1, 2, 6, 7, 9, 11, 12, 13, 14, 15, 16, 18, 19, 20, 21):   # pts0, pts1, n_corr, K0, K1, rig, stage 1's five outputs, workspace, R, t, n_inliers, status
        assert stage2(null=k) == E_ARG, k
    for k in (0, 1, 2, 6, 7, 9, 14, 19, 21, 22, 23, 24):                   # pts0, pts1, n_corr, K0, K1, rig, pair_ids, workspace, R, t, n_inliers, status
        assert batch(null=k) == E_ARG, k
    assert stage2(ws_bytes=ws(2, 3, 8) - 1) == E_WS and batch(ws_bytes=wsb(2, 3, 8, 10) - 1) == E_WS    # a workspace one byte short
