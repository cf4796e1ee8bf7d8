"""-m gpu: HIP.JPEG_DECODE 'device' in the fused path's loader adjacency (datasets.PairBatchLoader + DevicePrefetcher, submission.predict_fused)
yields what the host route yields, tensor for tensor and byte for byte, on a tree written like tools/bench_fused_split.write_scene plus one
progressive frame (decoded on the host by both routes)."""
import io
import os
import zipfile

import numpy as np
import pytest
import torch
from PIL import Image

import mapfree_reloc_amd  # noqa: F401
from mapfree_reloc_amd import datasets as D, jpeg_ops as J, submission
from mapfree_reloc_amd.config import get_cfg_defaults
from tools.bench_fused_split import write_scene

pytestmark = pytest.mark.gpu

PROGRESSIVE = os.path.join("test", "s00000", "seq1", "frame_00005.jpg")


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("jpeg_tree"))
    for s in range(2):
        write_scene((root, s, 3))
    p = os.path.join(root, PROGRESSIVE)
    Image.open(p).convert("RGB").save(p, quality=92, progressive=True)
    assert J.parse(open(p, "rb").read())[0] == J.UNSUPPORTED
    return root


def cfg_for(root, jpeg_decode, decode="thread"):
    cfg = get_cfg_defaults()
    cfg.DATASET.DATA_ROOT = root; cfg.DATASET.WIDTH = 540; cfg.DATASET.HEIGHT = 720; cfg.DATASET.ESTIMATED_DEPTH = "dptkitti"
    cfg.MODEL = "FeatureMatching"; cfg.ALLOW_SYNTHETIC_WEIGHTS = True
    cfg.FEATURE_MATCHING, cfg.POSE_SOLVER = "SuperGlue", "PNP"
    cfg.PNP.RANSAC_ITER, cfg.PNP.REPROJECTION_INLIER_THRESHOLD, cfg.PNP.CONFIDENCE = 1000, 3, 0.9999
    cfg.HIP.LOADER_DECODE, cfg.HIP.LOADER_WORKERS, cfg.HIP.JPEG_DECODE = decode, 2, jpeg_decode
    return cfg


def batches(root, decode, jpeg_decode):
    scenes = D.list_scenes(cfg_for(root, jpeg_decode), "test")
    loader = D.PairBatchLoader(scenes, 4, prefetch=1, pin=True, workers=2, decode=decode, jpeg_decode=jpeg_decode)
    try:
        out = []
        for b in D.DevicePrefetcher(loader, "cuda"):
            out.append({k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in b.items()})
        torch.cuda.synchronize()
        return out
    finally:
        loader.close()


@pytest.mark.parametrize("decode", ["thread", "process"])
def test_loader_device_route_equals_host_route(tree, decode):
    host, dev = batches(tree, decode, "host"), batches(tree, decode, "device")
    assert len(host) == len(dev) > 0
    for a, b in zip(host, dev):
        assert "jpeg" not in b
        for k, v in a.items():
            if isinstance(v, torch.Tensor):
                assert torch.equal(v, b[k]), k
            else:
                assert v == b[k], k


def test_corrupt_frame_raises_naming_its_path(tree, tmp_path):
    import shutil
    root = str(tmp_path / "corrupt")
    shutil.copytree(tree, root)
    p = os.path.join(root, "test", "s00001", "seq1", "frame_00010.jpg")
    d = open(p, "rb").read()
    i = d.index(b"\xff\xda")
    a = i + 2 + int.from_bytes(d[i + 2:i + 4], "big")
    open(p, "wb").write(d[:a + (len(d) - a) // 3] + b"\xff\xd9")          # well-formed markers, the scan ends early: the device must catch it
    assert J.parse(open(p, "rb").read())[0] == J.OK
    D.clear_frame_cache()
    with pytest.raises(OSError, match="frame_00010.jpg"):
        batches(root, "thread", "device")


def test_predict_fused_device_jpeg_writes_the_same_submission(tree, tmp_path):
    zs = [submission.predict_fused(cfg_for(tree, j, "process"), "test", str(tmp_path / j), batch_pairs=4) for j in ("host", "device")]
    with zipfile.ZipFile(zs[0]) as z0, zipfile.ZipFile(zs[1]) as z1:
        assert sorted(z0.namelist()) == sorted(z1.namelist()) and len(z0.namelist()) == 2
        for n in z0.namelist():
            assert z0.read(n) == z1.read(n), n
    assert submission.LAST_RUN_STATS.get("jpeg_decode") == "device"


def test_default_subsequence_length_synchronises_on_bench_frames():
    """the bench tree's encoding (540x720 q92 4:2:0 texture): the fixed point takes a few rounds, far below the subsequence count"""
    from tools.bench_jpeg import frames
    files, _ = frames(8)
    dec = J.JpegDecoder("cuda")
    g, st = dec.decode(files)
    assert int(st.abs().max()) == 0
    assert min(len(f) for f in files) > 40000                             # >= 500 subsequences per frame at the default length (<= 640 bits)
    assert int(dec.rounds.max()) < 100, dec.rounds.cpu().numpy()
    for i in (0, 7):
        assert np.array_equal(g[i, 0].cpu().numpy(), D.read_gray_plane(io.BytesIO(files[i]), None))
