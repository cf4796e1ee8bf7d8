"""-m gpu: HIP.DEPTH_DECODE 'device' in the fused path's loader adjacency (datasets.PairBatchLoader + DevicePrefetcher, submission.predict_fused)
yields what the host route yields, tensor for tensor and byte for byte, on a tree written like tools/bench_fused_split.write_scene with one
depth file rewritten as Adam7 (decoded on the host by both routes)."""
import os
import shutil
import struct
import sys
import zipfile
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

import mapfree_reloc_amd  # noqa: F401
from mapfree_reloc_amd import datasets as D, png_ops as P, submission
from mapfree_reloc_amd.config import get_cfg_defaults
from tools.bench_fused_split import write_scene

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_craft as PC  # noqa: E402

pytestmark = pytest.mark.gpu

INTERLACED = os.path.join("test", "s00000", "seq1", "frame_00005.dptkitti.png")


def adam7(a):
    """a u16 [H, W] -> an Adam7-interlaced 16-bit gray file, filter type 0 throughout"""
    raw = b""
    for x0, y0, dx, dy in ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2)):
        sub = a[y0::dy, x0::dx]
        if sub.size:
            raw += PC.filter_rows(sub, [0] * sub.shape[0])
    return PC.assemble(a.shape[1], a.shape[0], zlib.compress(raw), interlace=1)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("png_tree"))
    for s in range(2):
        write_scene((root, s, 3))
    p = os.path.join(root, INTERLACED)
    a = np.asarray(Image.open(p), dtype=np.uint16)
    open(p, "wb").write(adam7(a))
    assert np.array_equal(np.asarray(Image.open(p), dtype=np.uint16), a) and P.parse(open(p, "rb").read())[0] == P.UNSUPPORTED
    return root


def cfg_for(root, depth_decode, decode="thread", jpeg_decode="host"):
    cfg = get_cfg_defaults()
    cfg.DATASET.DATA_ROOT = root; cfg.DATASET.WIDTH = 540; cfg.DATASET.HEIGHT = 720; cfg.DATASET.ESTIMATED_DEPTH = "dptkitti"
    cfg.MODEL = "FeatureMatching"; cfg.ALLOW_SYNTHETIC_WEIGHTS = True
    cfg.FEATURE_MATCHING, cfg.POSE_SOLVER = "SuperGlue", "PNP"
    cfg.PNP.RANSAC_ITER, cfg.PNP.REPROJECTION_INLIER_THRESHOLD, cfg.PNP.CONFIDENCE = 1000, 3, 0.9999
    cfg.HIP.LOADER_DECODE, cfg.HIP.LOADER_WORKERS, cfg.HIP.JPEG_DECODE, cfg.HIP.DEPTH_DECODE = decode, 2, jpeg_decode, depth_decode
    return cfg


def batches(root, decode, jpeg_decode, depth_decode):
    scenes = D.list_scenes(cfg_for(root, depth_decode), "test")
    loader = D.PairBatchLoader(scenes, 4, prefetch=1, pin=True, workers=2, decode=decode, jpeg_decode=jpeg_decode, depth_decode=depth_decode)
    try:
        out = []
        for b in D.DevicePrefetcher(loader, "cuda"):
            out.append({k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in b.items()})
        torch.cuda.synchronize()
        return out
    finally:
        loader.close()


@pytest.fixture(scope="module")
def host_batches(tree):
    return batches(tree, "thread", "host", "host")


@pytest.mark.parametrize("jpeg_decode", ["host", "device"])
@pytest.mark.parametrize("decode", ["thread", "process"])
def test_loader_device_route_equals_host_route(tree, host_batches, decode, jpeg_decode):
    dev = batches(tree, decode, jpeg_decode, "device")
    assert len(host_batches) == len(dev) > 0
    for a, b in zip(host_batches, dev):
        assert "png" not in b and "jpeg" not in b and set(a) == set(b)
        for k, v in a.items():
            if isinstance(v, torch.Tensor):
                assert v.shape == b[k].shape and v.dtype == b[k].dtype and torch.equal(v, b[k]), k
            else:
                assert v == b[k], k


def test_corrupt_depth_raises_naming_its_path(tree, tmp_path):
    root = str(tmp_path / "corrupt")
    shutil.copytree(tree, root)
    p = os.path.join(root, "test", "s00001", "seq1", "frame_00010.dptkitti.png")
    st, h, rec = P.parse(open(p, "rb").read())
    assert st == P.OK
    stream = rec[:h.stream_bytes].tobytes()
    open(p, "wb").write(PC.assemble(540, 720, stream[:len(stream) // 2]))    # well-formed chunks, the stream ends early: the device must catch it
    assert P.parse(open(p, "rb").read())[0] == P.OK
    D.clear_frame_cache()
    with pytest.raises(OSError, match="frame_00010.dptkitti.png"):
        batches(root, "thread", "host", "device")


def test_predict_fused_device_depth_writes_the_same_submission(tree, tmp_path):
    zs = [submission.predict_fused(cfg_for(tree, d, "process", "device"), "test", str(tmp_path / d), batch_pairs=4) for d in ("host", "device")]
    with zipfile.ZipFile(zs[0]) as z0, zipfile.ZipFile(zs[1]) as z1:
        assert sorted(z0.namelist()) == sorted(z1.namelist()) and len(z0.namelist()) == 2
        for n in z0.namelist():
            assert z0.read(n) == z1.read(n), n
    assert submission.LAST_RUN_STATS.get("depth_decode") == "device"
