"""-m gpu test of the whole SuperPoint + SuperGlue matcher at a keypoint budget other than 1024 (SUPERGLUE.MAX_KEYPOINTS is a user setting):
tests/test_gpu_nets_parity.py::test_superpoint_superglue_end_to_end_vs_oracle with max_keypoints = K on both sides, the same synthetic 540 x 720 pair
and the same margins.  K = 500: the one-sweep Sinkhorn kernel at ldS = 500.  K = 333: the general row path, and an odd row pitch in the batched score
product and in the attention.  Both operand-splitting arithmetics."""
import numpy as np
import pytest
import torch

from mapfree_reloc_amd import images as IM, options
from mapfree_reloc_amd.nets import weights as WT
from mapfree_reloc_amd.nets.superpoint import SuperPointHIP
from mapfree_reloc_amd.nets.superglue import SuperGlueHIP
from oracle import nets_ref as NR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_ref = {}


def reference(K):
    """(matches [N, 4], keypoints of image 0) of the CPU oracle at max_keypoints = K; once per K"""
    if K not in _ref:
        sp = NR.SuperPointRef(max_keypoints=K).eval(); sp.load_state_dict(WT.superpoint_state_dict(1234))
        sg = NR.SuperGlueRef().eval(); sg.load_state_dict(WT.superglue_state_dict(4321))
        pr = IM.synthetic_pair(7, 720, 540)
        im0, im1 = torch.from_numpy(pr["img0"])[None, None], torch.from_numpy(pr["img1"])[None, None]
        with torch.no_grad():
            want = NR.superglue_match_pair(sp, sg, im0, im1)
            (rk0, rs0, _), = sp(im0)
        _ref[K] = (want, rk0.numpy(), float(rs0.min()), pr)
    return _ref[K]


@pytest.mark.parametrize("split", ["f16x2", "bf16x3"])
@pytest.mark.parametrize("K", [500, 333])
def test_matcher_end_to_end_vs_oracle_at_k(K, split):
    want, rk0, last_score, pr = reference(K)
    assert len(rk0) == K and not np.isnan(want).any() and len(want) > 50, "synthetic weights must produce matches"
    options.reset()
    with options.override(SPLIT=split):
        sp_hip = SuperPointHIP(WT.superpoint_state_dict(1234), DEV, max_keypoints=K)
        sg_hip = SuperGlueHIP(WT.superglue_state_dict(4321), DEV)
        ims = torch.from_numpy(np.stack([pr["img0"], pr["img1"]]))[:, None].to(DEV)
        spo = sp_hip(ims)
        out = sg_hip(spo, (720, 540))
        torch.cuda.synchronize()
    assert tuple(spo["kpts"].shape) == (2, K, 2) and tuple(out["matches0"].shape) == (1, K)
    k0 = spo["kpts"][0, :int(spo["n"][0])].cpu().numpy()
    set_ref = {tuple(p) for p in rk0.tolist()}
    set_hip = {tuple(p) for p in k0.tolist()}
    nc = int(out["n_corr"][0])
    got = torch.cat([out["pts0"][0, :nc], out["pts1"][0, :nc]], 1).cpu().numpy()
    sw = {tuple(r) for r in want.tolist()}
    sg_ = {tuple(r) for r in got.tolist()}
    print(f"K {K} {split}: keypoints {len(set_ref & set_hip)} of {len(set_ref)} shared (last kept score {last_score:.3f}); "
          f"matches: reference {len(sw)}, here {len(sg_)}, shared {len(sw & sg_)}")
    assert len(set_ref & set_hip) >= 0.99 * len(set_ref)
    assert len(sw & sg_) >= 0.95 * max(len(sw), len(sg_)), (len(sw), len(sg_), len(sw & sg_))
