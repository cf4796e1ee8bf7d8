"""tests/abs_pose_ref.py -- the numpy mirror of csrc/abs_pose.hip -- against the reference's own run of lib/utils/localize.py
(tests/golden/ref_sevenscenes.npz part (b)): identical inlier lists, approximated flags and pass counts, poses to 1e-9.  On these queries
the reference never shuffles, so the mirror's Philox subsets take no part."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abs_pose_ref as M  # noqa: E402

GROUPS = (1, 2, 3, 5, 8, 12)
ERR_THRES = ((0.1, 5), (0.25, 5), (0.5, 10), (1, 20))


@pytest.fixture(scope="module")
def ref(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "ref_sevenscenes.npz")))


def group_inputs(ref, k):
    """the group's queries as one mfr_abs_pose_fuse call"""
    pre = f"k{k}_"
    nq = len(ref[pre + "query_c"])
    return dict(train_q=ref[pre + "train_q"].reshape(-1, 4), train_c=ref[pre + "train_c"].reshape(-1, 3), pred_R=ref[pre + "R_pred"].reshape(-1, 9),
                pred_t=ref[pre + "t_pred"].reshape(-1, 3), offsets=np.arange(nq + 1, dtype=np.int32) * k), int(ref[pre + "in_iter"])


def quat_angle(a, b):
    d = abs(np.sum(a / np.linalg.norm(a) * b / np.linalg.norm(b)))
    return 2 * np.degrees(np.arccos(min(d, 1.0)))


@pytest.mark.parametrize("k", GROUPS)
def test_ransac_mirror_equals_the_reference(ref, k):
    pre = f"k{k}_"
    inp, in_iter = group_inputs(ref, k)
    out = M.fuse(**inp, mode=1, thr_deg=15.0, thr_mult=1.414, lo_iters=in_iter, seed=0)
    assert np.array_equal(out["inlier_mask"].reshape(-1, k), ref[pre + "inlier_mask"])
    assert np.array_equal(out["status"] == M.APPROXIMATED, ref[pre + "approx"]) and set(out["status"].tolist()) <= {M.OK, M.APPROXIMATED}
    assert np.abs(out["abs_c"] - ref[pre + "abs_c"]).max() <= 1e-9 and np.abs(out["abs_q"] - ref[pre + "abs_q"]).max() <= 1e-9
    if k == 1:
        assert ref[pre + "approx"].all()
    if k >= 3:
        assert not ref[pre + "approx"].any() and (ref[pre + "inlier_mask"].sum(1) >= 2).all()
    # pass counts of the reference's DSAC criterion, from the mirror's poses
    cerr = np.linalg.norm(ref[pre + "query_c"] - out["abs_c"], axis=1)
    qerr = np.array([quat_angle(a, b) for a, b in zip(ref[pre + "query_q"], out["abs_q"])])
    counts = [int(((cerr < t) & (qerr < r)).sum()) for t, r in ERR_THRES]
    assert counts == np.rint(ref[pre + "r_pass_rate"] * len(cerr) / 100).astype(int).tolist()


@pytest.mark.parametrize("k", GROUPS)
def test_median_mirror_equals_the_reference(ref, k):
    pre = f"k{k}_"
    inp, _ = group_inputs(ref, k)
    out = M.fuse(**inp, mode=0)
    assert (out["status"] == M.OK).all() and out["inlier_mask"].all()
    assert np.abs(out["abs_c"] - ref[pre + "abs_c0"]).max() <= 1e-9
    sign = np.sign(np.sum(out["abs_q"] * ref[pre + "abs_q0"], axis=1, keepdims=True))
    assert np.abs(out["abs_q"] * sign - ref[pre + "abs_q0"]).max() <= 1e-9
    cerr = np.linalg.norm(ref[pre + "query_c"] - out["abs_c"], axis=1)
    qerr = np.array([quat_angle(a, b) for a, b in zip(ref[pre + "query_q"], out["abs_q"])])
    counts = [int(((cerr < t) & (qerr < r)).sum()) for t, r in ERR_THRES]
    assert counts == np.rint(ref[pre + "m_passed"] * len(cerr) / 100).astype(int).tolist()


def test_mirror_edge_rules():
    rng = np.random.default_rng(5)
    eye = np.eye(3).reshape(9)
    q0 = np.array([1.0, 0, 0, 0])
    # no pairs, more than 64 pairs
    out = M.fuse(np.zeros((0, 4)), np.zeros((0, 3)), np.zeros((0, 9)), np.zeros((0, 3)), [0, 0], 1)
    assert out["status"].tolist() == [M.NO_PAIRS] and np.isnan(out["abs_c"]).all()
    n = 65
    out = M.fuse(np.tile(q0, (n, 1)), rng.normal(size=(n, 3)), np.tile(eye, (n, 1)), rng.normal(size=(n, 3)), [0, n], 1)
    assert out["status"].tolist() == [M.TOO_MANY] and not out["inlier_mask"].any()
    # Philox known answer (Random123 kat_vectors) and a subset draw: distinct members of the base list
    assert [hex(x) for x in M.philox4x32_10([0, 0, 0, 0], (0, 0))] == ['0x6627e8d5', '0xe169c58d', '0xbc57ac4c', '0x9b00dbd8']
    base = [0, 2, 3, 5, 7, 8, 9, 11]
    sub = M.lo_subset(3, 4, 1, 2, base, 4)
    assert len(set(sub)) == 4 and set(sub) <= set(base) and sub == sorted(sub) and sub == M.lo_subset(3, 4, 1, 2, base, 4)
    assert any(M.lo_subset(3, 4, 1, it, base, 4) != sub for it in range(8))
