"""mapfree_reloc_amd/localize.py -- error measures, precision / recall, report lines and pose_<scene>.txt lines -- against the reference's
own lib/utils/localize.py run (tests/golden/ref_sevenscenes.npz parts (b) and (c)).  The fused poses are handed in from the fixture
(`fuse=`), so these tests need no GPU; tests/test_gpu_abs_pose_fuse.py puts the device in that place."""
import os

import numpy as np
import pytest

from mapfree_reloc_amd import localize as L

GROUPS = (1, 2, 3, 5, 8, 12)
FIELDS = ("train_q", "train_c", "R_pred", "t_pred", "R_gt", "t_gt", "sim", "inliers")


@pytest.fixture(scope="module")
def ref(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "ref_sevenscenes.npz")))


def scene_of(ref, members, names, invalid_tail=False):
    """ScenePairs from (k, index) members of the fixture's groups, and the reference's fused results in localize_ops' layout.
    invalid_tail: the last query gets one more pair, without a pose (NaN: the reference's no_pt_pairs), which must not reach the fusion"""
    kw = {f: [] for f in FIELDS}
    pq, qq, qc, rec = [], [], [], dict(abs_q=[], abs_c=[], abs_q0=[], abs_c0=[], mask=[], status=[])
    for n, (k, i) in enumerate(members):
        qq.append(ref["k2_query_q"][0] if k == 0 else ref[f"k{k}_query_q"][i]); qc.append(ref["k2_query_c"][0] if k == 0 else ref[f"k{k}_query_c"][i])
        for key in ("abs_q", "abs_c", "abs_q0", "abs_c0"):
            rec[key].append(np.full(4 if "q" in key else 3, np.nan) if k == 0 else ref[f"k{k}_{key}"][i])
        rec["status"].append(2 if k == 0 else int(ref[f"k{k}_approx"][i]))
        if k:
            pq += [n] * k
            rec["mask"].append(ref[f"k{k}_inlier_mask"][i])
            for f in FIELDS:
                kw[f].append(ref[f"k{k}_{f}"][i])
    cat = lambda a, *shape: np.concatenate(a) if a else np.zeros((0, *shape))
    valid = np.ones(len(pq), bool)
    if invalid_tail:
        pq, valid = pq + [len(members) - 1], np.r_[valid, False]
        for f in FIELDS:
            last = np.asarray(kw[f][-1][-1:])
            kw[f].append(np.full_like(last, np.nan) if f in ("R_pred", "t_pred") else last)
    sp = L.ScenePairs(query_names=names, query_q=np.stack(qq), query_c=np.stack(qc), pair_query=pq, valid=valid,
                      **{f: cat(kw[f]) for f in FIELDS})

    def fuse(train_q, train_c, pred_R, pred_t, offsets, mode, *a):
        assert np.array_equal(train_q, sp.train_q[valid]) and np.array_equal(pred_R.reshape(-1, 3, 3), sp.R_pred[valid]) and np.isfinite(pred_t).all()
        m = cat(rec["mask"]).astype(np.int32)
        return dict(abs_q=np.stack(rec["abs_q" if mode else "abs_q0"]), abs_c=np.stack(rec["abs_c" if mode else "abs_c0"]),
                    inlier_mask=m if mode else np.ones_like(m), status=np.array(rec["status"] if mode else [s & 2 for s in rec["status"]], np.int32))
    return sp, fuse


def group_scene(ref, k):
    n = len(ref[f"k{k}_query_c"])
    return scene_of(ref, [(k, i) for i in range(n)], [f"seq-k{k}/frame-{i:06d}.color.png" for i in range(n)])


def test_error_measures_and_quaternions():
    assert L.cal_vec_angle_error(np.array([1.0, 0, 0]), np.array([0, 2.0, 0])).tolist() == [[90.0]]
    assert L.cal_vec_angle_error(np.zeros(3), np.ones(3)).tolist() == [[0.0]]                       # NaN -> 0 (:31)
    assert abs(L.cal_vec_angle_error(np.array([1.0, 0, 0]), np.array([1.0, 0.00999, 0])).item()) == 0.0     # the cosine is rounded to 4 decimals
    q = np.array([0.5, -0.5, 0.5, 0.5])
    assert L.cal_quat_angle_error(q, -3 * q).item() == 0.0 and L.cal_quat_angle_error(q, q).shape == (1, 1)
    R = L.quat2mat(q)
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-15) and np.allclose(L.mat2quat(R), q, atol=1e-15)
    assert np.array_equal(L.quat2mat(np.zeros(4)), np.eye(3)) and L.mat2quat(L.quat2mat(-q))[0] > 0


@pytest.mark.parametrize("k", GROUPS)
def test_ransac_route_numbers_and_pose_lines(ref, k):
    pre = f"k{k}_"
    sp, fuse = group_scene(ref, k)
    r = L.eval_scene_with_ransac(sp, L.fuse_scene(sp, True, fuse=fuse))
    assert r["tested"] == int(ref[pre + "r_tested"]) and len(r["approx_queries"]) == int(ref[pre + "r_approx_num"])
    assert np.array_equal(r["pass_rate"], ref[pre + "r_pass_rate"])
    assert np.allclose(r["err_res"], ref[pre + "r_err_res"], rtol=0, atol=1e-9)
    assert np.allclose(r["abs_t_errs"], ref[pre + "r_abs_t_err"], rtol=0, atol=1e-12) and np.allclose(r["abs_r_errs"], ref[pre + "r_abs_r_err"], rtol=0, atol=1e-9)
    assert np.array_equal(r["confidence"], ref[pre + "r_conf"])
    assert [l.rstrip("\n") for l in L.pose_file_lines(r)] == ref[pre + "r_pose_lines"].tolist()
    prec, rec, ap = L.precision_recall_pose_error(r["confidence"], r["abs_t_errs"], r["abs_r_errs"], 3, L.ERR_THRES[1])
    assert np.array_equal(prec, ref[pre + "pr_prec"]) and np.array_equal(rec, ref[pre + "pr_rec"]) and ap == float(ref[pre + "pr_ap"])


@pytest.mark.parametrize("k", GROUPS)
def test_median_route_numbers_and_pose_lines(ref, k):
    pre = f"k{k}_"
    sp, fuse = group_scene(ref, k)
    r = L.eval_scene_without_ransac(sp, L.fuse_scene(sp, False, fuse=fuse))
    assert np.allclose([r["abs_c_dist_err"], r["abs_c_ang_err"], r["abs_q_err"]], ref[pre + "m_medians"], rtol=0, atol=1e-9)
    assert np.allclose([r["rela_t_err"], r["rela_q_err"]], ref[pre + "m_rela"], rtol=0, atol=1e-9)
    assert np.allclose(L.cal_rela_pose_err(sp), ref[pre + "m_rela"], rtol=0, atol=1e-9)
    assert np.array_equal(r["passed"], ref[pre + "m_passed"]) and abs(r["average_precision"] - float(ref[pre + "m_ap"])) <= 1e-12
    assert np.allclose(r["abs_t_errs"], ref[pre + "m_abs_t_err"], rtol=0, atol=1e-12) and np.allclose(r["abs_r_errs"], ref[pre + "m_abs_r_err"], rtol=0, atol=1e-9)
    assert [l.rstrip("\n") for l in L.pose_file_lines(r)] == ref[pre + "m_pose_lines"].tolist()


def report_scenes(ref):
    out = {}
    for name in ref["report_scenes"].tolist():
        if name.startswith("k"):
            out[name] = group_scene(ref, int(name[1:]))
        else:
            out[name] = scene_of(ref, ref["mixed_members"].tolist(), [f"seq-mix/frame-{n:06d}.color.png" for n in range(len(ref["mixed_members"]))],
                                 invalid_tail=True)                       # the fixture's scene lists one pair without a pose
    return out


def test_report_lines_of_both_routes(ref):
    """the printed lines, with the reference's conventions: a query without pairs is 1000 m / 180 deg and tested in the RANSAC route, a
    failure of the AP and a miss of the recall (divided by all queries) without RANSAC; names cut to 10 characters"""
    scenes = report_scenes(ref)
    res = {n: L.eval_scene_with_ransac(sp, L.fuse_scene(sp, True, fuse=fuse)) for n, (sp, fuse) in scenes.items()}
    lines, avg_err, avg_pass = L.report_with_ransac(res, 15)
    assert "\n".join(lines).split("\n") == ref["report_ransac_lines"].tolist()
    assert res["mixed_scene_long_name"]["tested"] == 5 and "Dataset:mixed_scen Bad/All:1/5" in "\n".join(lines)
    assert [l.rstrip("\n") for l in L.pose_file_lines(res["mixed_scene_long_name"])] == ref["mixed_r_pose_lines"].tolist()
    res0 = {n: L.eval_scene_without_ransac(sp, L.fuse_scene(sp, False, fuse=fuse)) for n, (sp, fuse) in scenes.items()}
    assert res0["mixed_scene_long_name"]["no_pt_pairs"] == 1
    lines0, ev, passed = L.report_without_ransac(res0)
    assert lines0 == ref["report_median_lines"].tolist()
    assert np.allclose(ev, ref["report_median_eval"], rtol=0, atol=1e-9) and np.array_equal(passed, ref["report_median_passed"])
    assert res0["mixed_scene_long_name"]["failures"] == 1 and len(res0["mixed_scene_long_name"]["names"]) == 4
    assert [l.rstrip("\n") for l in L.pose_file_lines(res0["mixed_scene_long_name"])] == ref["mixed_m_pose_lines"].tolist()


def test_invalid_pairs_leave_the_fusion_inputs():
    sp = L.ScenePairs(query_names=["a", "b", "c"], query_q=np.tile([1.0, 0, 0, 0], (3, 1)), query_c=np.zeros((3, 3)), pair_query=[0, 0, 1, 2, 2],
                      train_q=np.tile([1.0, 0, 0, 0], (5, 1)), train_c=np.zeros((5, 3)), R_pred=np.tile(np.eye(3), (5, 1, 1)), t_pred=np.ones((5, 3)),
                      R_gt=np.tile(np.eye(3), (5, 1, 1)), t_gt=np.ones((5, 3)), sim=np.zeros(5), inliers=np.arange(5), valid=[True, False, False, True, True])
    keep, offsets = sp.fusion_inputs()
    assert keep.tolist() == [0, 3, 4] and offsets.tolist() == [0, 1, 1, 3] and offsets.dtype == np.int32
    with pytest.raises(AssertionError):
        L.ScenePairs(**{**sp.arrays(), "pair_query": [1, 0, 1, 2, 2]})
