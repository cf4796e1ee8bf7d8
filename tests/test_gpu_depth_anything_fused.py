"""-m gpu: Depth Anything on the fused route (DPT.NETWORK 'depth_anything', DPT.SOURCE 'online' in pipeline.FusedPosePipeline): nets/dpt.FusedDepthStage drives the
network through the same seam as DPT-Hybrid (prep_rows / features / tail_rows), here mfr_da_patch_rows_tab and mfr_da_head_tail_rows.

The yardstick is the per-pair plugin with DPT.SOURCE 'online' (tests/test_gpu_depth_anything.py pins it to compute_depth's files); every comparison is BIT
FOR BIT: the same kernels run on the same bytes, and a map does not depend on its batch neighbours.  Trees: rig_scenes.write_rig_tree (120 x 160 JPEGs);
network: depth_anything_ref.REDUCED at 70 x 98."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_anything_ref as R  # noqa: E402
import rig_scenes as S  # noqa: E402
from test_gpu_depth_anything import _stage_cfg  # noqa: E402
from test_gpu_dpt_fused import _hide_depth_files, _run_fused, _same  # noqa: E402

from mapfree_reloc_amd.builder import build_model  # noqa: E402
from mapfree_reloc_amd.datasets import make_loader  # noqa: E402
from mapfree_reloc_amd.nets import depth_anything as DA, weights as WT  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sd():
    return R.perturbed(WT.depth_anything_state_dict(arch=R.REDUCED))


def _cfg(root, tmp_path, sd, solver):
    cfg = _stage_cfg(root, tmp_path, sd, "online", "dptkitti")
    cfg.POSE_SOLVER = solver
    cfg.EMAT_RANSAC.PIX_THRESHOLD, cfg.EMAT_RANSAC.SCALE_THRESHOLD, cfg.EMAT_RANSAC.CONFIDENCE = 2.0, 0.1, 0.9999
    cfg.HIP.LOADER_DECODE, cfg.HIP.LOADER_WORKERS = "thread", 2
    return cfg


@pytest.mark.parametrize("solver", ["PNP", "EssentialMatrixMetric"])
def test_fused_pipeline_equals_the_per_pair_plugin(sd, tmp_path, solver):
    """PNP: the reference views only, the shared one once; EssentialMatrixMetric: both views"""
    S.write_rig_tree(tmp_path / "tree", n_frames=11)                        # 3 pairs: a full batch of 2 and a ragged one
    cfg = _cfg(tmp_path / "tree", tmp_path, sd, solver)
    model, plug = build_model(cfg), []
    for data in make_loader(cfg, "val"):
        Rm, t = model(data)
        plug.append((data["depth0"][0].clone(), data["depth1"][0].clone(), Rm[0], t.reshape(3), int(data["inliers"])))
    _hide_depth_files(tmp_path / "tree")                                    # the fused route must not read them
    pipe, rows = _run_fused(cfg, 2)
    assert isinstance(pipe.depth.net, DA.DepthAnythingHIP)
    assert len(rows) == len(plug) == 3
    for (d0, d1, Rf, tf, nf, st), (pd0, pd1, Rp, tp, npl) in zip(rows, plug):
        print(f"[depth anything fused] {solver}: status {st}, inliers {nf} / {npl}, t {tf.tolist()}")
        assert d0.shape == (S.TREE_H, S.TREE_W) and torch.equal(d0, pd0) and float(d0.std()) > 0.5
        if solver != "PNP":
            assert torch.equal(d1, pd1)
        else:
            assert d1 is None                                               # PnP reads depth0 only: the query views never went through the network
        assert _same(Rf, Rp) and _same(tf, tp) and nf == npl
    if solver == "PNP":
        assert pipe.stats["depth_views_run"] == 1 and pipe.stats["depth_views_reused"] == 1
