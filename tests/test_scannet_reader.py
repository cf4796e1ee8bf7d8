"""The ScanNet reader (mapfree_reloc_amd/scannet.py) against what the reference's own ScanNetScene made of the same tiny tree
(tests/golden/ref_scannet.npz, written by tools/gen_scannet_golden.py; the tree is rebuilt here from the parameters the fixture stores),
the data-source dispatch of list_scenes, and the host gray_pair on files larger than the network size.  The fixture was computed with the
same numpy / torch, so equality is exact: K in float64, T in float32, depth in float32."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scannet_tree as ST  # noqa: E402

from mapfree_reloc_amd import datasets as D  # noqa: E402
from mapfree_reloc_amd.config import get_cfg_defaults  # noqa: E402
from mapfree_reloc_amd.scannet import ScanNetScene, list_scannet_scenes, pair_image_paths  # noqa: E402


@pytest.fixture(scope="module")
def ref(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "ref_scannet.npz")))


@pytest.fixture(scope="module")
def tree(ref, tmp_path_factory):
    p = {k[5:]: v for k, v in ref.items() if k.startswith("tree_")}
    return p, ST.write_tree(tmp_path_factory.mktemp("scannet"), p)


def _cfg(tr, p, est=None):
    cfg = get_cfg_defaults()
    cfg.DATASET.DATA_SOURCE, cfg.DATASET.DATA_ROOT, cfg.DATASET.NPZ_ROOT = "ScanNet", tr["data_root"], tr["npz_root"]
    cfg.DATASET.WIDTH, cfg.DATASET.HEIGHT, cfg.DATASET.MIN_OVERLAP_SCORE = int(p["width"]), int(p["height"]), float(p["min_overlap_score"])
    cfg.DATASET.ESTIMATED_DEPTH = est
    return cfg


def test_samples_equal_the_reference(ref, tree):
    p, tr = tree
    scenes = D.list_scenes(_cfg(tr, p), "test")
    assert len(scenes) == 1 and isinstance(scenes[0], ScanNetScene) and len(scenes[0]) == 5
    sc = scenes[0]
    assert sc.shared_reference is False and sc.has_gray_pair and sc.scene_id == "test" and sc.scene_root == tr["scans"]
    for i in range(len(sc)):
        s = sc[i]
        assert list(s["pair_names"]) == ref["pair_names"][i].tolist() and s["scene_id"] == str(ref["scene_id"][i])
        assert s["pair_id"] == int(ref["pair_id"][i]) == i and s["dataset_name"] == "ScanNet"
        for k in ("K_color0", "K_color1", "K_depth"):
            assert s[k].dtype == torch.float64 and np.array_equal(s[k].numpy(), ref[k][i]), k
        for k in ("T_0to1", "T_1to0"):
            assert s[k].dtype == torch.float32 and np.array_equal(s[k].numpy(), ref[k][i]), k
        for k in ("depth0", "depth1"):
            assert s[k].dtype == torch.float32 and np.array_equal(s[k].numpy(), ref["gt_" + k][i]), k
        assert s["image0"].shape == (3, int(p["height"]), int(p["width"])) and s["image0"].dtype == torch.float32
    # the constants 1296 x 968 scale K whatever the files' size (the tree's JPEGs are 13 x 10)
    assert not np.array_equal(ref["K_color0"][0], ref["K_color0"][2])                     # two scene folders, two calibrations


def test_estimated_depth_and_empty_depth(ref, tree):
    p, tr = tree
    sc = D.list_scenes(_cfg(tr, p, est=tr["est_npz"]), "test")[0]
    for i in range(len(sc)):
        s = sc[i]
        for k in ("depth0", "depth1"):
            assert s[k].dtype == torch.float32 and np.array_equal(s[k].numpy(), ref["est_" + k][i]), k
    val = ScanNetScene(tr["scans"], tr["test_npz"], mode="val", resize=(int(p["width"]), int(p["height"])))
    assert val[0]["depth0"].numel() == int(ref["val_depth_numel"]) == 0 and val.batch_layout() == (6, 8, False)


def test_score_filter_quirk(ref, tree):
    """`mode not in ['val' or 'test']` tests against 'val' only: an index file with a score column is filtered in TEST mode too"""
    p, tr = tree
    for mode in ("train", "val", "test"):
        sc = ScanNetScene(tr["scans"], tr["scored_npz"], mode=mode, min_overlap_score=float(p["min_overlap_score"]), resize=(8, 6))
        assert np.array_equal(np.asarray(sc.data_names, np.int64), ref[f"scored_names_{mode}"]), mode
    assert len(ref["scored_names_val"]) == 5 and len(ref["scored_names_test"]) == len(ref["scored_names_train"]) == 3


def test_make_loader_and_pair_paths(ref, tree):
    p, tr = tree
    batches = list(D.make_loader(_cfg(tr, p), "test"))
    assert len(batches) == 5 and batches[3]["T_0to1"].shape == (1, 4, 4) and int(batches[3]["pair_id"]) == 3
    assert batches[3]["pair_names"][1][0] == ref["pair_names"][3][1] and "scene_root" not in batches[3]
    paths = pair_image_paths(tr["test_npz"], tr["scans"])
    assert paths[2] == (os.path.join(tr["scans"], "scene0711_01", "sensor_data", "frame-000015.color.jpg"),
                        os.path.join(tr["scans"], "scene0711_01", "sensor_data", "frame-000300.color.jpg"))
    assert all(os.path.exists(a) and os.path.exists(b) for a, b in paths)


def test_other_data_sources_stay_mapfree(tmp_path):
    sc = tmp_path / "val" / "s00000"
    (sc / "seq0").mkdir(parents=True); (sc / "seq1").mkdir()
    (sc / "poses.txt").write_text("seq0/frame_00000.jpg 1 0 0 0 0 0 0\nseq1/frame_00000.jpg 1 0 0 0 0.1 0 0\n")
    (sc / "intrinsics.txt").write_text("seq0/frame_00000.jpg 500 500 270 360 540 720\nseq1/frame_00000.jpg 500 500 270 360 540 720\n")
    for src in (None, "MapFree"):
        cfg = get_cfg_defaults()
        cfg.DATASET.DATA_SOURCE, cfg.DATASET.DATA_ROOT, cfg.DATASET.WIDTH, cfg.DATASET.HEIGHT = src, str(tmp_path), 540, 720
        scenes = D.list_scenes(cfg, "val")
        assert [type(s) for s in scenes] == [D.MapFreeScene] and len(scenes[0]) == 1


def test_missing_index_is_an_error(tree):
    p, tr = tree
    with pytest.raises(D.MissingDataError):
        list_scannet_scenes(_cfg(tr, p), "val")


def _big_tree(tmp_path, W=20, H=14, fw=41, fh=29):
    """files (fw x fh) larger than the network size (W x H), depth at W x H"""
    p = ST.default_params(5)
    rng = np.random.default_rng(9)
    n = len(p["frames"])
    yy, xx = np.mgrid[0:fh, 0:fw]
    p["color_u8"] = np.stack([np.clip(np.stack([4 * xx + 3 * k, 6 * yy, 255 - 3 * xx - 2 * yy], -1) + rng.integers(0, 30, (fh, fw, 3)), 0, 255)
                              for k in range(n)]).astype(np.uint8)
    p["depth_u16"] = rng.integers(0, 65536, size=(n, H, W)).astype(np.uint16)
    p["est_depth"] = rng.uniform(0.3, 6.0, size=(n, H, W))
    p["width"], p["height"] = np.int64(W), np.int64(H)
    return p, ST.write_tree(tmp_path, p)


def test_host_gray_pair_resizes_gray_first(tmp_path):
    p, tr = _big_tree(tmp_path)
    sc = D.list_scenes(_cfg(tr, p), "test")[0]
    W, H = int(p["width"]), int(p["height"])
    paths = pair_image_paths(tr["test_npz"], tr["scans"])
    for i in (0, 2):
        out = (np.zeros((H, W), np.float32), np.zeros((H, W), np.float32), np.zeros((H, W), np.float32), np.zeros((H, W), np.float32))
        got = sc.gray_pair(i, True, out=out)
        assert got is not None
        g0, d0, g1, d1, K0, K1, pid, names = got
        for g, o, path in ((g0, out[0], paths[i][0]), (g1, out[2], paths[i][1])):
            want = D.read_gray_plane(path, (W, H))
            assert want.shape == (H, W) and np.array_equal(o, want) and np.array_equal(g, want)
        smp = sc[i]
        assert np.array_equal(out[1], smp["depth0"].numpy()) and np.array_equal(out[3], smp["depth1"].numpy())
        assert K0.dtype == np.float64 and np.array_equal(K0, smp["K_color0"].numpy()) and pid == i and names == smp["pair_names"]
        # the dataset's own order (8-bit RGB resized, then luma) is a different plane: the routes must not be mixed
        assert not np.array_equal(D.to_gray(smp["image0"]).numpy(), out[0])


def test_thread_loader_serves_gray_pair_planes(tmp_path):
    """PairBatchLoader on the host route: every row of every batch, the first included, is read_gray_plane(path, (W, H)); depth straight
    from the PGM files; no reference-view sharing"""
    p, tr = _big_tree(tmp_path)
    scenes = D.list_scenes(_cfg(tr, p), "test")
    W, H = int(p["width"]), int(p["height"])
    paths = pair_image_paths(tr["test_npz"], tr["scans"])
    loader = D.PairBatchLoader(scenes, 2, prefetch=0, pin=False, workers=2, decode="thread")
    seen = 0
    for b in loader:
        assert b["images"].shape[1:] == (1, H, W) and b["K0"].dtype == torch.float64 and b["ref_keys"] == [None] * len(b["names"])
        for q, gid in enumerate(b["global_ids"].tolist()):
            assert np.array_equal(b["images"][2 * q, 0].numpy(), D.read_gray_plane(paths[gid][0], (W, H)))
            assert np.array_equal(b["images"][2 * q + 1, 0].numpy(), D.read_gray_plane(paths[gid][1], (W, H)))
            assert np.array_equal(b["depth0"][q].numpy(), scenes[0][gid]["depth0"].numpy()) and int(b["seed_ids"][q]) == gid
            seen += 1
    loader.close()
    assert seen == 5


def test_depth_of_another_size_is_an_error(tmp_path):
    p, tr = _big_tree(tmp_path)
    cfg = _cfg(tr, p)
    cfg.DATASET.WIDTH = 22
    sc = D.list_scenes(cfg, "test")[0]
    out = tuple(np.zeros((14, 22), np.float32) for _ in range(4))
    with pytest.raises(ValueError, match="depth map"):
        sc.gray_pair(0, True, out=out)


def test_device_route_host_fallback_resizes(tmp_path):
    """the device JPEG route's host half: a frame over the record cap is not handed to the device -- its row is filled on the host with
    the RESIZED plane; a frame under the cap is only parsed (its header says the file's size, the row's plane is left for the device)"""
    from mapfree_reloc_amd import jpeg_ops as J
    p, tr = _big_tree(tmp_path)
    scenes = D.list_scenes(_cfg(tr, p), "test")
    W, H = int(p["width"]), int(p["height"])
    paths = pair_image_paths(tr["test_npz"], tr["scans"])
    for cap, on_device in ((64, False), (D.JPEG_RECORD_CAP, True)):
        loader = D.PairBatchLoader(scenes, 5, prefetch=0, pin=False, workers=1, decode="thread", jpeg_decode="device", jpeg_cap=cap)
        b, = list(loader)
        loader.close()
        rows, hdr = b["jpeg"]["rows"], b["jpeg"]["headers"].numpy()
        for gid in range(5):
            for j in (0, 1):
                st, nb, path = rows[2 * gid + j]
                assert path == paths[gid][j]
                if on_device:
                    assert st == J.OK and nb > 0 and hdr[2 * gid + j, 4:12].view(np.int32).tolist() == [41, 29]
                else:
                    assert st == J.CAPACITY and nb == 0
                    assert np.array_equal(b["images"][2 * gid + j, 0].numpy(), D.read_gray_plane(path, (W, H)))
