"""CPU: the numpy restatement of the SIFT detector (tests/sift_cpu_ref.py, the spec csrc/sift.hip is pinned against) on known
answers, and the opencv/hip switch of the SIFT plugin.  No GPU needed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sift_cpu_ref as R  # noqa: E402


def _blobs(H, W, blobs, bg=60.0, amp=150.0):
    yy, xx = np.mgrid[:H, :W].astype(np.float64)
    img = np.full((H, W), bg)
    for cy, cx, s in blobs:
        img += amp * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
    return np.round(img).astype(np.uint8)


def test_flat_image_has_no_keypoints():
    out = R.detect(np.full((64, 80), 128, np.uint8))
    assert len(out["kpts"]) == 0 and out["desc"].shape == (0, 128)


def test_gaussian_blobs_found_at_position_and_scale():
    """isotropic blobs of known sigma: every blob is found within 0.5 px (OpenCV's doubled base image puts points a quarter pixel
    right / down of the centre: the upsample has half-pixel centres, the output halves the doubled coordinates), and the keypoint
    size is within 15 % of 2 sigma (the diameter SIFT reports for a blob of scale sigma)"""
    blobs = [(30, 40, 4.0), (60, 90, 3.0), (70, 30, 5.0)]
    out = R.detect(_blobs(110, 130, blobs))
    k, s = out["kpts"], out["size"]
    assert len(k) > 0
    for cy, cx, sig in blobs:
        d = np.hypot(k[:, 0] - cx, k[:, 1] - cy)
        j = int(np.argmin(d))
        assert d[j] < 0.5, (cx, cy, k[j])
        assert abs(s[j] - 2 * sig) < 0.15 * 2 * sig, (sig, s[j])
    # nothing else: every keypoint sits on one of the blobs
    dmin = np.min([np.hypot(k[:, 0] - cx, k[:, 1] - cy) for cy, cx, _ in blobs], 0)
    assert (dmin < 0.5).all()


def test_rotation_by_90_degrees():
    """np.rot90 (an exact pixel permutation).  The detector is not exactly rotation-equivariant -- OpenCV's neither: each
    octave after the first keeps the EVEN pixels of the previous one, which a flip of an axis turns into the odd ones, and the
    row pass / column pass order swaps -- so the test looks at the first octave (octave byte 255), where sampling is symmetric:
    its keypoints map to (y, W - 1/2 - x) (the quarter-pixel offset of the doubled base flips with the axis), their angles shift
    by one common 90-degree step, and their descriptors stay close"""
    from mapfree_reloc_amd import images as IM
    g = np.round(np.clip(IM.synthetic_pair(11, 200, 160)["img0"], 0, 1) * 255).astype(np.uint8)
    H, W = g.shape
    a, b = R.detect(g), R.detect(np.ascontiguousarray(np.rot90(g)))
    sel = (a["octave"] & 255) == 255
    assert sel.sum() >= 20
    ka, kb = a["kpts"][sel], b["kpts"]
    mapped = np.stack([ka[:, 1], (W - 0.5) - ka[:, 0]], 1)
    hits, shifts, dd = 0, [], []
    for i in range(len(ka)):
        d = np.hypot(kb[:, 0] - mapped[i, 0], kb[:, 1] - mapped[i, 1]) + np.abs(b["size"] - a["size"][sel][i])
        d = d + np.minimum(np.abs(((b["angle"] - a["angle"][sel][i]) % 360) - 90), np.abs(((b["angle"] - a["angle"][sel][i]) % 360) - 270))
        j = int(np.argmin(d))
        if d[j] < 1e-2:
            hits += 1
            shifts.append(round(float((b["angle"][j] - a["angle"][sel][i]) % 360)))
            dd.append(np.linalg.norm(b["desc"][j] - a["desc"][np.nonzero(sel)[0][i]]))
    assert hits >= 0.9 * len(ka), (hits, len(ka))
    assert len(set(s % 360 for s in shifts)) == 1 and shifts[0] in (90, 270)
    assert np.median(dd) < 0.02 * 512 and max(dd) < 0.1 * 512


def test_nfeatures_keeps_ties_and_sorted_order():
    rows = [(5.0, 1.0, 3.0, 10.0, 0.5, 1), (1.0, 2.0, 3.0, 10.0, 0.875, 1), (1.0, 2.0, 4.0, 10.0, 0.25, 1),
            (1.0, 1.0, 3.0, 20.0, 0.5, 1), (1.0, 1.0, 3.0, 5.0, 0.5, 1), (1.0, 1.0, 3.0, 5.0, 0.75, 1),    # an exact duplicate (x, y, size, angle)
            (9.0, 9.0, 3.0, 5.0, 0.125, 1)]
    keep = R.select([tuple(np.float32(v) if i < 5 else v for i, v in enumerate(r)) for r in rows], 3)
    # duplicates removed (the higher response stays), then retainBest(3): responses 0.875, 0.75, 0.5, 0.5 -> the two 0.5 ties both stay
    assert [tuple(float(v) for v in k[:5]) for k in keep] == [(1.0, 1.0, 3.0, 5.0, 0.75), (1.0, 1.0, 3.0, 20.0, 0.5),
                                                              (1.0, 2.0, 3.0, 10.0, 0.875), (5.0, 1.0, 3.0, 10.0, 0.5)]
    assert [tuple(float(v) for v in k[:4]) for k in R.select([tuple(np.float32(v) if i < 5 else v for i, v in enumerate(r)) for r in rows[1:3]], 0)] \
        == [(1.0, 2.0, 4.0, 10.0), (1.0, 2.0, 3.0, 10.0)]                                                 # equal x, y: larger size first


def test_nfeatures_on_an_image():
    from mapfree_reloc_amd import images as IM
    g = np.round(np.clip(IM.synthetic_pair(5, 96, 128)["img0"], 0, 1) * 255).astype(np.uint8)
    full = R.detect(g)
    top = R.detect(g, 40, pyr=full["pyr"])
    assert len(full["kpts"]) > 40 and len(top["kpts"]) >= 40
    thr = np.sort(full["response"])[::-1][39]
    assert (top["response"] >= thr).all() and len(top["kpts"]) == int((full["response"] >= thr).sum())
    order = np.lexsort((top["angle"], -top["size"], top["kpts"][:, 1], top["kpts"][:, 0]))
    assert np.array_equal(order, np.arange(len(order)))
    assert (top["desc"] == np.round(top["desc"])).all() and top["desc"].min() >= 0 and top["desc"].max() <= 255


def test_library_blur_taps_equal_the_restatement():
    import mapfree_reloc_amd as mfr
    import ctypes as C
    lib = mfr._lib.load()
    for lvl in range(6):
        taps = (C.c_float * 17)()
        rad = C.c_int(0)
        assert lib.mfr_sift_blur_taps(lvl, taps, C.byref(rad)) == 0
        c, Rr = R.gauss_taps(R.level_sigma(lvl))
        assert rad.value == Rr and np.array_equal(np.array(taps[:Rr + 1], np.float32), c)
    assert [R.gauss_taps(R.level_sigma(l))[1] for l in range(6)] == [5, 5, 6, 8, 10, 13]
    assert lib.mfr_sift_workspace_bytes(1, 720, 540, 0) > 0 and lib.mfr_sift_workspace_bytes(1, 4, 4, 0) == 0
    assert R.n_octaves(720, 540) == 9


def test_sift_plugin_default_still_needs_opencv():
    from mapfree_reloc_amd.config import get_cfg_defaults
    from mapfree_reloc_amd.matching.feature_matching import SIFTMatching
    cfg = get_cfg_defaults()
    cfg.FEATURE_MATCHING, cfg.SIFT.NUM_FEATURES, cfg.SIFT.RATIO_THRESHOLD = "SIFT", 2048, 0.8
    assert cfg.SIFT.DETECTOR == "opencv"
    try:
        import cv2  # noqa: F401
        have_cv2 = True
    except ImportError:
        have_cv2 = False
    if have_cv2:
        SIFTMatching(cfg)
    else:
        with pytest.raises(ImportError):
            SIFTMatching(cfg)
