"""-m gpu test of SuperPoint's keypoint selection (sp_select_kernel, csrc/superpoint_post.hip) at max_keypoints != 1024: the radix select for the K-th
key, the bitonic sort with 1024 - K empty slots and the store of K rows -- tests/test_gpu_nets_parity.py::test_select_topk_and_raster_order's
construction and stable-sort oracle, on the smallest map that keeps more than 1000 candidates through simple_nms (223 x 215, nearly every pixel set).
Scores take 200 levels, so the cut at K falls inside a group of equal scores and the raster-order rule decides the set."""
import numpy as np
import pytest
import torch

from mapfree_reloc_amd.nets import weights as WT
from mapfree_reloc_amd.nets.superpoint import SuperPointHIP
from oracle import nets_ref as NR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W = 223, 215
DENSITIES = (0.4, 0.0008, 0.0)          # more than 1000 candidates / a few dozen / none
KS = (1, 70, 333, 500, 1000)


def nms_stable_maps():
    g = torch.Generator().manual_seed(2)
    B = len(DENSITIES)
    s = torch.zeros(B, H, W)
    mask = torch.rand(B, H, W, generator=g) < torch.tensor(DENSITIES).view(B, 1, 1)
    vals = torch.round(torch.rand(B, H, W, generator=g) * 200) / 200 + 0.01     # many exact ties
    s[mask] = vals[mask]
    return NR.simple_nms(s, 4)                                                 # only points that survive the NMS: the device's pass changes nothing


def candidates(s):
    """raster-ordered (row, col) and scores of one map's candidates (threshold 0.005, border 4)"""
    kp = torch.nonzero(s > 0.005)
    v = s[kp[:, 0], kp[:, 1]]
    m = (kp[:, 0] >= 4) & (kp[:, 0] < H - 4) & (kp[:, 1] >= 4) & (kp[:, 1] < W - 4)
    return kp[m], v[m]


@pytest.fixture(scope="module")
def maps():
    s = nms_stable_maps()
    cands = [candidates(s[b]) for b in range(len(DENSITIES))]
    counts = [len(kp) for kp, _ in cands]
    print(f"select: {counts} candidates on {H} x {W}")
    assert counts[0] > 1000 and 1 < counts[1] < 70 and counts[2] == 0
    return s, cands


@pytest.mark.parametrize("K", KS)
def test_select_topk_below_1024(maps, K):
    s, cands = maps
    hip = SuperPointHIP(WT.superpoint_state_dict(1234), DEV, max_keypoints=K)
    cand, cnt, _ = hip.nms_candidates(s.to(DEV))
    kpts, sc, n = hip.select(cand, cnt, W)
    assert tuple(kpts.shape) == (len(cands), K, 2) and tuple(sc.shape) == (len(cands), K)
    kpts, sc, n, cnt = kpts.cpu(), sc.cpu(), n.cpu(), cnt.cpu()
    cut_in_tie = False
    for b, (kp, v) in enumerate(cands):
        assert int(cnt[b]) == len(kp)
        if len(kp) > K:
            vs, order = torch.sort(v, descending=True, stable=True)
            cut_in_tie |= bool(vs[K - 1] == vs[K])
            kp, v = kp[order[:K]], v[order[:K]]
        assert int(n[b]) == len(kp)
        np.testing.assert_array_equal(kpts[b, :len(kp)].numpy().view(np.int32), torch.flip(kp, [1]).float().numpy().view(np.int32))
        np.testing.assert_array_equal(sc[b, :len(kp)].numpy().view(np.int32), v.numpy().view(np.int32))
        assert (kpts[b, len(kp):].numpy().view(np.int32) == 0).all() and (sc[b, len(kp):].numpy().view(np.int32) == 0).all()
    assert len(cands[0][0]) > K and (K == 1 or len(cands[1][0]) < K)          # both regimes: score-sorted top-K, and raster order
    assert K == 1 or cut_in_tie, "the cut must fall inside a group of equal scores"
