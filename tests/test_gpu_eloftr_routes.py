"""-m gpu: the routes of the EfficientLoFTR stage agree on the same files (the pattern of tests/test_gpu_routes_agree.py, on a 2-scene Map-free tree of
lossy coloured JPEGs): the per-pair plugin (FEATURE_MATCHING 'EfficientLoFTR' through FeatureMatchingModel) and submission.predict_fused write the same
pose lines; `compute -m ELoFTR` + 'Precomputed' holds the correspondences the fused matcher stage produces; HIP.REF_FEATURE_CACHE on and off give the
same bytes.

The tree is this file's own: the seeded weights' features are local, and on the smooth synthetic views of the other route tests they tell 1 - 2 of
6256 cells apart (measured with the CPU module).  Here a scene's key frame is white noise and the sampled query frames are the key frame + N(0, 0.01^2)
over a tilted depth plane: after the JPEG round trip the CPU module still matches ~1400 cells of such a pair, so real poses are compared."""
import os
import zipfile

import numpy as np
import pytest
import torch

from mapfree_reloc_amd import compute, submission, wire
from mapfree_reloc_amd.builder import build_model
from mapfree_reloc_amd.config import get_cfg_defaults
from mapfree_reloc_amd.datasets import DevicePrefetcher, PairBatchLoader, list_scenes, make_loader

pytestmark = pytest.mark.gpu


def _write_tree(root, frames=(6, 1)):
    """val/<scene>/{seq0,seq1}/frame_XXXXX.jpg (JPEG quality 92, tinted so that the luma is not a byte already), frame_XXXXX.dptkitti.png (uint16 mm),
    poses.txt, intrinsics.txt; pairs = key frame x every 5th seq1 frame: those are the key frame + noise, the others unrelated noise"""
    from PIL import Image
    yy, xx = np.mgrid[0:720, 0:540]
    depth = (2.0 + 0.001 * xx + 0.0005 * yy).astype(np.float32)
    for s, nf in enumerate(frames):
        sc = root / "val" / f"s{s:05d}"
        (sc / "seq0").mkdir(parents=True); (sc / "seq1").mkdir()
        rng = np.random.default_rng(100 * s + 7)
        key = rng.random((720, 540)).astype(np.float32)

        def save(gray, rel):
            rgb = np.stack([0.92 * gray + 0.03, gray, 0.8 * gray + 0.1 * gray * gray], -1)
            Image.fromarray(np.round(np.clip(rgb, 0, 1) * 255).astype(np.uint8)).save(sc / rel, format="JPEG", quality=92)
            Image.fromarray(np.round(depth * 1000).astype(np.uint16)).save(str(sc / rel).replace(".jpg", ".dptkitti.png"))
        lp, lk = ["# frame qw qx qy qz tx ty tz"], ["# frame fx fy cx cy W H"]
        save(key, "seq0/frame_00000.jpg")
        lp.append("seq0/frame_00000.jpg 1 0 0 0 0 0 0"); lk.append("seq0/frame_00000.jpg 590.0 590.0 270.0 360.0 540 720")
        for i in range(nf):
            q = np.clip(key + 0.01 * rng.standard_normal(key.shape), 0, 1) if i % 5 == 0 else rng.random((720, 540))
            save(q.astype(np.float32), f"seq1/frame_{i:05d}.jpg")
            lp.append(f"seq1/frame_{i:05d}.jpg 1 0 0 0 0 0 0"); lk.append(f"seq1/frame_{i:05d}.jpg 590.0 590.0 270.0 360.0 540 720")
        (sc / "poses.txt").write_text("\n".join(lp) + "\n"); (sc / "intrinsics.txt").write_text("\n".join(lk) + "\n")


def _cfg(root, matcher, cache=True):
    cfg = get_cfg_defaults()
    cfg.MODEL, cfg.FEATURE_MATCHING, cfg.POSE_SOLVER = "FeatureMatching", matcher, "PNP"
    cfg.MATCHES_FILE_PATH = "{scene_root}/correspondences_ELoFTR.npz"
    cfg.PNP.RANSAC_ITER, cfg.PNP.REPROJECTION_INLIER_THRESHOLD, cfg.PNP.CONFIDENCE = 1000, 3, 0.9999
    cfg.DATASET.DATA_ROOT, cfg.DATASET.HEIGHT, cfg.DATASET.WIDTH, cfg.DATASET.ESTIMATED_DEPTH = str(root), 720, 540, "dptkitti"
    cfg.ALLOW_SYNTHETIC_WEIGHTS = True
    cfg.HIP.REF_FEATURE_CACHE = bool(cache)
    return cfg


def _lines(path):
    with zipfile.ZipFile(path) as z:
        return {n: z.read(n).decode().split("\n") for n in z.namelist()}


def test_plugin_fused_offline_and_reference_cache_agree(tmp_path):
    from mapfree_reloc_amd.pipeline import FusedPosePipeline
    _write_tree(tmp_path)                                                           # pairs: frames 0 and 5 of scene 0, frame 0 of scene 1
    # per-pair plugin
    cfg_p = _cfg(tmp_path, "EfficientLoFTR")
    res = submission.predict(make_loader(cfg_p, "val"), build_model(cfg_p))
    submission.save_submission(res, tmp_path / "plugin.zip", deterministic=True)
    # fused, reference-view cache on (batches of 2 pairs straddle the scene boundary) and off
    pipe = FusedPosePipeline(_cfg(tmp_path, "EfficientLoFTR", True))
    z_on = submission.predict_fused(_cfg(tmp_path, "EfficientLoFTR", True), "val", tmp_path / "fused_on", pipeline=pipe, batch_pairs=2)
    z_off = submission.predict_fused(_cfg(tmp_path, "EfficientLoFTR", False), "val", tmp_path / "fused_off",
                                     pipeline=FusedPosePipeline(_cfg(tmp_path, "EfficientLoFTR", False)), batch_pairs=2)
    assert pipe.stats["reference_views_reused"] >= 1
    on = _lines(z_on)
    assert on == _lines(z_off) == _lines(tmp_path / "plugin.zip") and sorted(on) == ["pose_s00000.txt", "pose_s00001.txt"]
    first = on["pose_s00000.txt"][0].split(" ")
    assert first[0] == "seq1/frame_00000.jpg" and int(first[8]) > 100 and "nan" not in first          # a real pose was compared, not two failures
    # offline: compute -m ELoFTR over every seq1 frame -> npz; its rows == the fused matcher stage on the loader's batches, and 'Precomputed' writes the same lines
    compute.main(["-ds", "Mapfree", "-m", "ELoFTR", "--data_root", str(tmp_path)])
    cfg_a = _cfg(tmp_path, "Precomputed")
    res_a = submission.predict(make_loader(cfg_a, "val"), build_model(cfg_a))
    submission.save_submission(res_a, tmp_path / "offline.zip", deterministic=True)
    assert _lines(tmp_path / "offline.zip") == _lines(z_on)
    scenes = list_scenes(cfg_p, "val")
    loader = PairBatchLoader(scenes, 2, prefetch=1, pin=True, global_offsets=[0, len(scenes[0])], workers=2, decode="thread")
    seen = total = 0
    for batch in DevicePrefetcher(loader, pipe.device):
        m = pipe.match(batch)
        torch.cuda.synchronize()
        for p in range(len(batch["seed_ids"])):
            corr = np.load(os.path.join(batch["scene_roots"][p], "correspondences_ELoFTR.npz"))["correspondences"]
            want0, want1 = wire.strip_nan(corr[int(batch["seed_ids"][p])].astype(np.float32))
            n = int(m["n_corr"][p])
            assert n == len(want0), (batch["scene_roots"][p], int(batch["seed_ids"][p]), n, len(want0))
            if n:
                assert np.array_equal(m["pts0"][p, :n].cpu().numpy(), want0) and np.array_equal(m["pts1"][p, :n].cpu().numpy(), want1)
                assert float(m["pts0"][p, :n, 0].max()) < 540 and float(m["pts1"][p, :n, 1].max()) < 720
            seen, total = seen + 1, total + n
    loader.close()
    assert seen == 3 and total > 300
