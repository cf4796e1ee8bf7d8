"""Host side of DPT depth on the fused route (DPT.SOURCE 'online' in submission.predict_fused), no GPU: the colour bytes PairBatchLoader(rgb=True) carries,
what it refuses, the DPT.FUSED_CHUNK check, and when predict_fused asks its loader for the bytes.  The device half: tests/test_gpu_dpt_fused.py."""
import glob
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rig_scenes as S  # noqa: E402

from mapfree_reloc_amd.config import get_cfg_defaults  # noqa: E402
from mapfree_reloc_amd.datasets import PairBatchLoader, clear_frame_cache, list_scenes  # noqa: E402


def _cfg(root, width=S.TREE_W, height=S.TREE_H, depth="dptkitti"):
    cfg = get_cfg_defaults()
    cfg.DATASET.DATA_ROOT, cfg.DATASET.HEIGHT, cfg.DATASET.WIDTH, cfg.DATASET.ESTIMATED_DEPTH = str(root), height, width, depth
    return cfg


def _pil(scene_root, name):
    from PIL import Image
    return np.asarray(Image.open(os.path.join(scene_root, name)).convert("RGB"))


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """3 pairs that share the keyframe, and NO depth file: whoever opens one fails"""
    root = tmp_path_factory.mktemp("tree")
    t = S.write_rig_tree(root, n_frames=11)
    for f in glob.glob(os.path.join(str(root), "**", "*.dptkitti.png"), recursive=True):
        os.remove(f)
    clear_frame_cache()
    return root, t


def _check_batches(loader, scene_root, n_pairs):
    seen = 0
    try:
        for b in loader:
            assert b["depth0"] is None and b["depth1"] is None and "png" not in b
            n = len(b["names"])
            assert b["rgb"].dtype == torch.uint8 and b["rgb"].shape == (2 * n, S.TREE_H, S.TREE_W, 3) and b["images"].shape == (2 * n, 1, S.TREE_H, S.TREE_W)
            for p, name in enumerate(b["names"]):
                for row, frame in ((2 * p, "seq0/frame_00000.jpg"), (2 * p + 1, name)):
                    want = _pil(scene_root, frame)
                    assert np.array_equal(b["rgb"][row].numpy(), want), (row, frame)
                    luma = ((want.astype(np.uint32) * np.array([19595, 38470, 7471], np.uint32)).sum(-1) + 0x8000) >> 16
                    assert np.array_equal(b["images"][row, 0].numpy(), luma.astype(np.float32) / np.float32(255))       # the plane the matchers read
            seen += n
    finally:
        loader.close()
    assert seen == n_pairs


@pytest.mark.parametrize("decode,workers", [("thread", 1), ("thread", 3), ("process", 2)])
def test_loader_carries_rgb_and_opens_no_depth_file(tree, decode, workers):
    root, t = tree
    _check_batches(PairBatchLoader(list_scenes(_cfg(root), "val"), 2, prefetch=1, pin=False, workers=workers, decode=decode, rgb=True), t["scene_root"], 3)


@pytest.mark.parametrize("decode", ["thread", "process"])
def test_loader_without_the_argument_is_unchanged(tmp_path, decode):
    S.write_rig_tree(tmp_path / "tree", n_frames=6)                          # with its depth files
    scenes = list_scenes(_cfg(tmp_path / "tree"), "val")
    out = []
    for kw in ({}, dict(rgb=False)):
        loader = PairBatchLoader(scenes, 2, prefetch=0, pin=False, workers=2, decode=decode, **kw)
        try:
            out.append([{k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in b.items() if k != "_slot"} for b in loader])
        finally:
            loader.close()
    assert len(out[0]) == len(out[1]) == 1
    for a, b in zip(*out):
        assert list(a) == list(b) and "rgb" not in a and a["depth0"] is not None and a["depth0"].shape == (2, S.TREE_H, S.TREE_W)
        for k in a:
            if isinstance(a[k], torch.Tensor):
                assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
            else:
                assert a[k] == b[k], k


class _GenericScene:
    """a scene without the loaders' fast route: samples come from __getitem__ (image0 / image1 are byte / 255 in float32)"""
    has_gray_pair = False

    def __init__(self, sc):
        self.sc, self.scene_id, self.scene_root, self.shared_reference = sc, sc.scene_id, sc.scene_root, sc.shared_reference

    def __len__(self):
        return len(self.sc)

    def __getitem__(self, i):
        return self.sc[i]


@pytest.mark.parametrize("decode", ["thread", "process"])
def test_generic_route_recovers_the_bytes(tree, decode):
    root, t = tree
    scenes = [_GenericScene(sc) for sc in list_scenes(_cfg(root, depth=None), "val")]
    _check_batches(PairBatchLoader(scenes, 2, prefetch=0, pin=False, workers=2, decode=decode, rgb=True), t["scene_root"], 3)


def test_resized_and_multi_frame_scenes_are_refused(tree):
    root, _ = tree
    with pytest.raises(NotImplementedError, match="size"):
        PairBatchLoader(list_scenes(_cfg(root, width=80, height=60), "val"), 2, rgb=True)
    cfg = _cfg(root)
    cfg.DATASET.QUERY_FRAME_COUNT = 2
    multi = list_scenes(cfg, "val")
    assert len(multi[0]) > 0
    with pytest.raises(NotImplementedError, match="multi-frame"):
        PairBatchLoader(multi, 2, rgb=True)
    PairBatchLoader(multi, 2).close()                                        # without the argument both are served as before
    PairBatchLoader(list_scenes(_cfg(root, width=80, height=60), "val"), 2).close()


def test_check_cfg_validates_the_chunk():
    from mapfree_reloc_amd.nets import dpt
    cfg = get_cfg_defaults()
    assert cfg.DPT.FUSED_CHUNK == 16 and dpt.check_cfg(cfg).FUSED_CHUNK == 16
    cfg.DPT.FUSED_CHUNK = 1
    dpt.check_cfg(cfg)
    for bad in (0, -3, 2.5, "16", True):
        cfg.DPT.FUSED_CHUNK = bad
        with pytest.raises(ValueError, match="FUSED_CHUNK"):
            dpt.check_cfg(cfg)


class _StubPipeline:
    """stands in for FusedPosePipeline on the host: records what the loader handed over"""
    device = "cpu"

    def __init__(self):
        self.seen = []

    def __call__(self, b):
        n = b["seed_ids"].numel()
        self.seen.append(("rgb" in b, b.get("depth0") is not None))
        if "rgb" in b:
            assert b["rgb"].shape[0] == 2 * n and b["rgb"].dtype == torch.uint8
        return dict(R=torch.eye(3, dtype=torch.float64).repeat(n, 1, 1), t=torch.ones(n, 3, dtype=torch.float64), n_inliers=torch.full((n,), 9, dtype=torch.int32),
                    status=torch.zeros(n, dtype=torch.int32))


@pytest.mark.parametrize("source,solver,rgb", [("online", "PNP", True), ("online", "EssentialMatrixMetric", True), ("online", "Procrustes", True),
                                               ("online", "EssentialMatrix", False), ("file", "PNP", False)])
def test_predict_fused_asks_for_rgb_iff_the_solver_reads_online_depth(tmp_path, source, solver, rgb):
    from mapfree_reloc_amd import submission
    S.write_rig_tree(tmp_path / "tree", n_frames=6)                          # with its depth files: SOURCE 'file' reads them
    cfg = _cfg(tmp_path / "tree")
    cfg.POSE_SOLVER, cfg.DPT.SOURCE, cfg.HIP.LOADER_WORKERS, cfg.HIP.LOADER_DECODE = solver, source, 2, "thread"
    assert submission.wants_rgb(cfg) is rgb
    pipe = _StubPipeline()
    z = submission.predict_fused(cfg, "val", tmp_path / "out", pipeline=pipe, batch_pairs=2, prefetch=0)
    assert z is not None and pipe.seen == [(rgb, not rgb)]                   # the colour bytes INSTEAD of the depth maps, never both
    pipe.needs_rgb = not rgb                                                 # a pipeline that says what it needs is believed
    assert submission.wants_rgb(cfg, pipe) is (not rgb)
