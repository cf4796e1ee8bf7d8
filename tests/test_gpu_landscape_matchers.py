"""-m gpu: LoFTR and the HIP SIFT detector at 480 x 640 -- the LANDSCAPE shape of ScanNet's matcher stage (coarse grid 60 x 80, not the
90 x 68 of Map-free) -- through matchers.LoFTR_matcher.match / SIFT_matcher.match on one synthetic pair, against the CPU references the
portrait parity tests use (oracle/loftr_ref.py; tests/sift_cpu_ref.py + the oracle's descriptor stage), with those tests' bars."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sift_cpu_ref as R  # noqa: E402

from mapfree_reloc_amd import images as IM, matchers  # noqa: E402
from oracle import oracle_lib as O  # noqa: E402

pytestmark = pytest.mark.gpu
W, H = 640, 480


@pytest.fixture(scope="module")
def pair_files(tmp_path_factory):
    from PIL import Image
    d = tmp_path_factory.mktemp("landscape")
    pr = IM.synthetic_pair(7, H, W)
    paths = []
    for k in ("img0", "img1"):
        g = np.round(np.clip(pr[k], 0, 1) * 255).astype(np.uint8)
        Image.fromarray(np.stack([g, g, g], -1)).save(d / f"{k}.jpg", format="JPEG", quality=95)
        paths.append(str(d / f"{k}.jpg"))
    return tuple(paths)


@pytest.mark.filterwarnings("ignore:.*synthetic weights")
def test_loftr_matcher_at_480x640_vs_oracle(pair_files):
    """the bars of tests/test_gpu_loftr_parity.py::test_loftr_end_to_end_vs_oracle"""
    from mapfree_reloc_amd.nets import weights as WT
    from oracle import loftr_ref as LR
    ref = LR.LoFTRRef().eval(); ref.load_state_dict(WT.loftr_state_dict())
    ims = [torch.from_numpy(matchers.read_image(p, (W, H)))[None, None] for p in pair_files]
    assert ims[0].shape == (1, 1, H, W)
    torch.set_num_threads(16)
    want = LR.loftr_match_pair(ref, ims[0], ims[1])
    got = matchers.LoFTR_matcher((W, H)).match(pair_files)
    assert len(want) > 100 and not np.isnan(want).any() and not np.isnan(got).any()
    assert got[:, [0, 2]].max() < W and got[:, [1, 3]].max() < H and got[:, [0, 2]].max() > H      # x runs over the long side
    kw = {(int(r[0]), int(r[1])): r for r in want}
    kg = {(int(r[0]), int(r[1])): r for r in got}
    common = set(kw) & set(kg)
    assert len(common) >= 0.998 * max(len(kw), len(kg)), (len(kw), len(kg), len(common))
    d = np.array([np.abs(kw[k] - kg[k]).max() for k in common])
    print("LoFTR 480x640:", len(kw), len(kg), len(common), np.quantile(d, [0.5, 0.9, 0.99, 1.0]), (d > 0).mean())
    assert np.quantile(d, 0.99) < 1e-3 and d.max() < 2e-2 and (d > 0).mean() < 0.15, (np.quantile(d, [0.5, 0.9, 0.99, 1.0]), (d > 0).mean())


def test_sift_matcher_at_480x640_vs_references(pair_files):
    """detector: the bars of tests/test_gpu_sift.py (_compare) on the first view; descriptor stage: the rule of
    tests/test_gpu_descriptor_parity.py::test_2nn_vs_oracle -- every match the oracle decides with a clear margin is found, and nothing
    else but rows inside the margins"""
    from mapfree_reloc_amd import sift_ops
    g = [np.round(matchers.read_image(p, (W, H)) * 255.0).astype(np.uint8) for p in pair_files]
    assert g[0].shape == (H, W)
    det = sift_ops.SiftDetector(2048, "cuda:0")
    out = det(torch.from_numpy(g[0]).to("cuda:0"))
    ref = R.detect(g[0], 2048)
    n = int(out["n"][0])
    gpu = lambda k: out[k][0, :n].cpu().numpy()
    assert int(out["status"][0]) == 0 and n == len(ref["kpts"]) > 1000
    assert np.array_equal(gpu("kpts"), ref["kpts"]) and np.array_equal(gpu("octave"), ref["octave"]) and np.array_equal(gpu("response"), ref["response"])
    assert np.allclose(gpu("size"), ref["size"], rtol=1e-5, atol=0)
    da = np.abs(gpu("angle") - ref["angle"])
    assert (np.minimum(da, 360 - da) <= 1e-3).all()
    dd = np.abs(gpu("desc") - ref["desc"])
    assert dd.max() <= 1 and (dd == 0).mean() >= 0.999
    assert gpu("kpts")[:, 0].max() > H                                   # keypoints over the whole long side
    # the whole matcher on the two files against the oracle's rootSIFT + exact 2-NN + ratio test on the same features
    m = matchers.SIFT_matcher((W, H), detector="hip")
    got = m.match(pair_files)
    (kp0, d0), (kp1, d1) = det.per_image(torch.from_numpy(g[0]).to("cuda:0")), det.per_image(torch.from_numpy(g[1]).to("cuda:0"))
    r0, q0 = O.rootsift(d0); r1, q1 = O.rootsift(d1)
    idx, d2 = O.desc_2nn(r0, r1, q0, q1)
    s = np.sqrt(d2.astype(np.float64))
    clear = ((d2[:, 1] - d2[:, 0]) > 4e-6) & (np.abs(s[:, 0] - 0.8 * s[:, 1]) > 1e-4)
    keep = s[:, 0] < 0.8 * s[:, 1]
    # (compared as sets of coordinate rows: several orientations of one keypoint give rows with equal coordinates)
    sure = {tuple(np.concatenate([kp0[i], kp1[idx[i]]]).tolist()) for i in np.nonzero(clear & keep)[0]}
    have = {tuple(r) for r in got.astype(np.float32).tolist()}
    print("SIFT 480x640:", n, len(got), len(sure), int((~clear).sum()))
    assert len(sure) > 100 and sure <= have and len(have) - len(sure) <= int((~clear).sum())
