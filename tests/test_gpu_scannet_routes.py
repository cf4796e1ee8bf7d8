"""-m gpu: on a ScanNet-layout tree whose frames (648 x 484 JPEGs) are larger than the network size (320 x 240), the reference's two-stage
flow and the fused routes are the same estimator (the manner of tests/test_gpu_routes_agree.py):

  (i)   compute.py -ds Scannet -m SG -> correspondences_SG_scannet_test.npz -> scannet_benchmark per pair with Precomputed + PnP
  (ii)  scannet_benchmark --fused, online SuperGlue + PnP, frames decoded and resized on the host
  (iii) the same with HIP.JPEG_DECODE 'device': frames decoded at their own size and resized on the GPU (csrc/resize.hip)

(ii) and (iii) see bit-equal image batches; all three give identical correspondence sets, R, t and inlier counts per pair, hence identical
printed lines and saved arrays.  Content: tests/scannet_tree.routes_params (images.synthetic_pair views; on the CPU oracle pipeline five
pairs recover the known pose with ~200 inliers each and the sixth, two unrelated views, gives a 6-inlier pose)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scannet_tree as ST  # noqa: E402

from mapfree_reloc_amd import compute, scannet_benchmark as SB, wire  # noqa: E402
from mapfree_reloc_amd.config import get_cfg_defaults  # noqa: E402

pytestmark = pytest.mark.gpu
W, H = 320, 240


def _cfg(tr, matcher, jpeg="host", matches=None):
    cfg = get_cfg_defaults()
    cfg.MODEL, cfg.FEATURE_MATCHING, cfg.POSE_SOLVER, cfg.MATCHES_FILE_PATH = "FeatureMatching", matcher, "PNP", matches
    cfg.PNP.RANSAC_ITER, cfg.PNP.REPROJECTION_INLIER_THRESHOLD, cfg.PNP.CONFIDENCE = 1000, 3, 0.9999
    cfg.DATASET.DATA_SOURCE, cfg.DATASET.DATA_ROOT, cfg.DATASET.NPZ_ROOT = "ScanNet", tr["data_root"], tr["npz_root"]
    cfg.DATASET.WIDTH, cfg.DATASET.HEIGHT, cfg.DATASET.MIN_OVERLAP_SCORE = W, H, 0.4
    cfg.HIP.JPEG_DECODE, cfg.HIP.LOADER_DECODE, cfg.HIP.LOADER_WORKERS = jpeg, "thread", 2
    cfg.ALLOW_SYNTHETIC_WEIGHTS = True                          # no checkpoints offline: the seeded synthetic networks, on purpose
    return cfg


def test_offline_fused_host_and_fused_device_routes_agree(tmp_path):
    tr = ST.write_tree(tmp_path / "tree", ST.routes_params(W, H))
    # ---- (i) offline matcher stage -> npz -> Precomputed + PnP, one pair at a time
    compute.main(["-ds", "Scannet", "-m", "SG", "--pair_npz", tr["test_npz"], "--data_root", tr["scans"], "--output_dir", str(tmp_path / "misc"),
                  "--resize", str(W), str(H)])
    npz = tmp_path / "misc" / "correspondences_SG_scannet_test.npz"
    corr = wire.load_correspondences(npz)
    assert corr.shape[0] == 6
    per_pair = []
    lines_i, agg_i = SB.run(_cfg(tr, "Precomputed", matches=str(npz)), "sg_pnp", output_root=tmp_path / "i",
                            hook=lambda data, R, t: per_pair.append((R[0].numpy().copy(), t.reshape(3).numpy().copy(), int(data["inliers"]))))
    assert len(per_pair) == 6 and sum(bool(np.isfinite(R).all() and np.isfinite(t).all()) for R, t, _ in per_pair) >= 5
    assert sum(n > 100 for _, _, n in per_pair) >= 5                  # real poses were compared, not failures

    # ---- (ii) / (iii) fused: loaders + online SuperGlue + PnP in batches of 4 (the second batch is short)
    from mapfree_reloc_amd.pipeline import FusedPosePipeline
    pipe = FusedPosePipeline(_cfg(tr, "SuperGlue"))
    fused = {}
    for tag, jpeg in (("ii", "host"), ("iii", "device")):
        seen = dict(images=[], pairs={})

        def hook(batch, out, seen=seen):
            if jpeg == "device":
                assert "jpeg" not in batch and batch["images"].is_cuda
            seen["images"].append(batch["images"].cpu())
            m = pipe.match(batch)
            for q, gid in enumerate(batch["global_ids"].tolist()):
                n = int(m["n_corr"][q])
                seen["pairs"][gid] = (m["pts0"][q, :n].cpu().numpy(), m["pts1"][q, :n].cpu().numpy(), out["R"][q].to(torch.float32).cpu().numpy(),
                                      out["t"][q].to(torch.float32).cpu().numpy(), int(out["n_inliers"][q]), int(batch["seed_ids"][q]))
        lines, agg = SB.run(_cfg(tr, "SuperGlue", jpeg), "sg_pnp", fused=True, batch_pairs=4, output_root=tmp_path / tag, pipeline=pipe, hook=hook)
        fused[tag] = (lines, agg, seen)
    # the loaders' planes: device decode + device resize == host decode + host resize, and both are the offline stage's read_image
    from mapfree_reloc_amd.datasets import read_gray_plane
    from mapfree_reloc_amd.scannet import pair_image_paths
    im_ii, im_iii = torch.cat(fused["ii"][2]["images"]), torch.cat(fused["iii"][2]["images"])
    assert im_ii.shape == (12, 1, H, W) and torch.equal(im_ii, im_iii)
    for gid, (p0, p1) in enumerate(pair_image_paths(tr["test_npz"], tr["scans"])):
        assert np.array_equal(im_iii[2 * gid, 0].numpy(), read_gray_plane(p0, (W, H))) and np.array_equal(im_iii[2 * gid + 1, 0].numpy(), read_gray_plane(p1, (W, H)))
    for tag in ("ii", "iii"):
        lines, agg, seen = fused[tag]
        assert sorted(seen["pairs"]) == list(range(6))
        for gid in range(6):
            pts0, pts1, R, t, ninl, pid = seen["pairs"][gid]
            want0, want1 = wire.strip_nan(corr[gid])
            assert pid == gid and len(pts0) == len(want0) and np.array_equal(pts0, want0) and np.array_equal(pts1, want1), (tag, gid)
            Ri, ti, ni = per_pair[gid]
            assert np.array_equal(R, Ri, equal_nan=True) and np.array_equal(t, ti, equal_nan=True) and ninl == ni, (tag, gid, ninl, ni)
        assert lines == lines_i, (tag, lines, lines_i)
        assert set(agg) == set(agg_i) and all(np.array_equal(agg[k], agg_i[k], equal_nan=True) for k in agg), tag
        saved = np.load(tmp_path / tag / "scannet" / "sg_pnp.npz")
        assert all(np.array_equal(saved[k], agg_i[k], equal_nan=True) for k in agg_i)
        assert (tmp_path / tag / "scannet" / "sg_pnp.txt").read_text().splitlines() == lines_i
    assert float(np.nanmedian(agg_i["t_err_euc"])) < 0.05 and len(lines_i) == 10      # the known pose, to centimetres
