"""-m gpu: the SIFT detector of csrc/sift.hip (sift_ops.SiftDetector) against the numpy restatement tests/sift_cpu_ref.py --
Gaussian pyramid, keypoints, descriptors -- plus batching, edge cases and the SIFT leg end to end (per-pair plugin, the batched
FusedPosePipeline stage, the offline npz route)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sift_cpu_ref as R  # noqa: E402

from mapfree_reloc_amd import images as IM, sift_ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _u8(img):
    return np.round(np.clip(img, 0, 1) * 255).astype(np.uint8)


def _textured(seed, H=720, W=540, which="img0"):
    return _u8(IM.synthetic_pair(seed, H, W)[which])


@pytest.mark.parametrize("HW", [(720, 540), (719, 537), (48, 64)])
def test_pyramid_bit_identical(HW):
    H, W = HW
    g = _textured(3, H, W)
    det = sift_ops.SiftDetector(2048, DEV)
    det(torch.from_numpy(g).to(DEV)[None])
    torch.cuda.synchronize()
    pyr = R.gaussian_pyramid(g)
    assert len(pyr) == sift_ops.num_octaves(H, W)
    for o, G in enumerate(pyr):
        for l in range(6):
            got = det.level(1, H, W, o, l)[0].cpu().numpy()
            assert got.shape == G[l].shape and np.array_equal(got, G[l]), (o, l, np.abs(got - G[l]).max())


def _compare(gpu, ref, b=0):
    n = int(gpu["n"][b])
    assert n == len(ref["kpts"]), (n, len(ref["kpts"]))
    g = lambda k: gpu[k][b, :n].cpu().numpy()
    assert np.array_equal(g("kpts"), ref["kpts"])
    assert np.array_equal(g("octave"), ref["octave"])
    assert np.array_equal(g("response"), ref["response"])
    # size goes through exp2 (binary64 on both sides, rounded to f32): identical up to an ulp of the binary64 result
    assert np.allclose(g("size"), ref["size"], rtol=1e-5, atol=0)
    da = np.abs(g("angle") - ref["angle"])
    assert (np.minimum(da, 360 - da) <= 1e-3).all()
    dd = np.abs(g("desc") - ref["desc"])
    assert dd.max() <= 1 and (dd == 0).mean() >= 0.999
    return n


def test_keypoints_and_descriptors_equal_the_restatement():
    g = _textured(3)
    ref = R.detect(g, 0)
    assert len(ref["kpts"]) > 1500
    for nf in (0, 1000):                      # every keypoint (about 2000 on this image), and retainBest(1000)
        out = sift_ops.SiftDetector(nf, DEV)(torch.from_numpy(g).to(DEV))
        assert int(out["status"][0]) == 0
        n = _compare(out, R.detect(g, nf, pyr=ref["pyr"]) if nf else ref)
        assert n >= (1000 if nf else 1500)


def test_small_image_and_all_keypoints():
    g = _textured(8, 96, 128)
    out = sift_ops.SiftDetector(0, DEV)(torch.from_numpy(g).to(DEV))
    assert int(out["status"][0]) == 0 and _compare(out, R.detect(g, 0)) > 20


def test_batch_equals_single_calls():
    gs = [_textured(s, 240, 200) for s in (1, 2, 3)]
    det = sift_ops.SiftDetector(300, DEV)
    batch = det(torch.from_numpy(np.stack(gs)).to(DEV))
    for b, g in enumerate(gs):
        one = det(torch.from_numpy(g).to(DEV))
        n = int(one["n"][0])
        assert int(batch["n"][b]) == n > 0
        for k in ("kpts", "desc", "size", "angle", "response", "octave"):
            assert torch.equal(batch[k][b], one[k][0]), k
    # f32 input holding whole numbers: the same result
    f = det(torch.from_numpy(gs[0].astype(np.float32)).to(DEV))
    assert torch.equal(f["desc"], det(torch.from_numpy(gs[0]).to(DEV))["desc"])


def test_blank_image():
    out = sift_ops.SiftDetector(2048, DEV)(torch.full((2, 120, 160), 77, dtype=torch.uint8, device=DEV))
    torch.cuda.synchronize()
    assert out["n"].tolist() == [0, 0] and out["status"].tolist() == [0, 0]


def test_candidate_overflow_status():
    g = _textured(3, 240, 200)
    det = sift_ops.SiftDetector(0, DEV, cand_cap=16)
    out = det(torch.from_numpy(np.stack([g, g])).to(DEV))
    torch.cuda.synchronize()
    st = out["status"].tolist()
    assert all(s & sift_ops.ST_CAND_OVERFLOW for s in st)
    assert all(0 < n <= 16 * 18 for n in out["n"].tolist())            # <= 18 orientation peaks per candidate
    assert float(out["desc"][:, int(out["n"].max()):].abs().sum()) == 0      # nothing written past the kept rows


def _sift_cfg(solver="EssentialMatrixMetric"):
    from mapfree_reloc_amd.config import get_cfg_defaults
    cfg = get_cfg_defaults()
    cfg.MODEL, cfg.FEATURE_MATCHING, cfg.POSE_SOLVER = "FeatureMatching", "SIFT", solver
    cfg.SIFT.NUM_FEATURES, cfg.SIFT.RATIO_THRESHOLD, cfg.SIFT.DETECTOR = 2048, 0.8, "hip"
    cfg.EMAT_RANSAC.PIX_THRESHOLD, cfg.EMAT_RANSAC.SCALE_THRESHOLD, cfg.EMAT_RANSAC.CONFIDENCE = 2.0, 0.1, 0.9999
    cfg.PNP.RANSAC_ITER, cfg.PNP.REPROJECTION_INLIER_THRESHOLD, cfg.PNP.CONFIDENCE = 1000, 3, 0.9999
    return cfg


def _byte_scene(n=3):
    """SyntheticScene samples whose images are bytes / 255 (what the loaders decode), so the per-pair plugin's u8
    ((255 x).astype(uint8) + OpenCV's 14-bit luma, feature_matching.py:61-65) and the batched stage's u8 (rint(255 x) of the loaders'
    gray plane) are the same bytes"""
    from mapfree_reloc_amd.datasets import SyntheticScene, collate_batch1
    sc = SyntheticScene(2, frames=n)
    out = []
    for i in range(n):
        s = sc[i]
        for k in ("image0", "image1"):
            s[k] = torch.from_numpy(_u8(s[k].numpy()).astype(np.float32) / np.float32(255))
        out.append(collate_batch1(s))
    return out


def _rot_err_deg(R1, R2):
    c = (np.trace(R1.T @ R2) - 1) / 2
    return float(np.degrees(np.arccos(np.clip(c, -1, 1))))


def test_end_to_end_plugin_fused_and_offline_agree(tmp_path):
    from mapfree_reloc_amd import wire
    from mapfree_reloc_amd.builder import build_model
    from mapfree_reloc_amd.datasets import to_gray
    from mapfree_reloc_amd.matching.feature_matching import SIFTMatching
    from mapfree_reloc_amd.pipeline import FusedPosePipeline
    samples = _byte_scene(3)
    cfg = _sift_cfg()
    model = build_model(cfg)
    plugin = SIFTMatching(cfg)
    per_pair = []
    for s in samples:
        R_, t_ = model(s)[:2]
        Rn = np.asarray(R_).reshape(3, 3)
        assert _rot_err_deg(Rn, s["T_0to1"][0, :3, :3].numpy()) < 2.0          # known pose recovered on every pair
        per_pair.append((Rn, np.asarray(t_).reshape(3), plugin.get_correspondences(s)))
    # batched: gray planes as the loaders deliver them, reference / query interleaved
    ims = torch.stack([to_gray(s[k][0]) for s in samples for k in ("image0", "image1")])[:, None].contiguous().to(DEV)
    u8 = sift_ops.plane_to_u8(ims[:, 0]).cpu().numpy()
    for i, s in enumerate(samples):
        assert np.array_equal(u8[2 * i], SIFTMatching.transform_grayscale(s["image0"][0]))
        assert np.array_equal(u8[2 * i + 1], SIFTMatching.transform_grayscale(s["image1"][0]))
    d = lambda k: torch.cat([s[k] for s in samples]).to(DEV)
    batch = dict(images=ims, depth0=d("depth0"), depth1=d("depth1"), K0=d("K_color0"), K1=d("K_color1"),
                 seed_ids=torch.tensor([int(s["pair_id"]) for s in samples], dtype=torch.int64, device=DEV))
    pipe = FusedPosePipeline(cfg)
    m = pipe.match(batch)
    out = pipe(batch)
    for i, (Rn, tn, (p0, p1)) in enumerate(per_pair):
        n = int(m["n_corr"][i])
        assert n == len(p0) > 50
        assert np.array_equal(m["pts0"][i, :n].cpu().numpy(), p0) and np.array_equal(m["pts1"][i, :n].cpu().numpy(), p1)
        assert int(out["status"][i]) == 0
        assert np.array_equal(out["R"][i].cpu().numpy().astype(np.float32), Rn.astype(np.float32))
        assert np.array_equal(out["t"][i].cpu().numpy().astype(np.float32), tn.astype(np.float32))
    # offline: the npz the SIFT route writes (rows indexed by pair_id), read back through Precomputed, gives the same poses
    pids = [int(s["pair_id"]) for s in samples]
    rows = [np.full((1, 4), np.nan)] * (max(pids) + 1)
    for pid, (_, _, (p0, p1)) in zip(pids, per_pair):
        rows[pid] = np.concatenate([p0, p1], 1)
    wire.save_correspondences(tmp_path / "correspondences_SIFT.npz", rows)
    cfg2 = _sift_cfg()
    cfg2.FEATURE_MATCHING, cfg2.MATCHES_FILE_PATH = "Precomputed", str(tmp_path / "correspondences_SIFT.npz")
    pre = build_model(cfg2)
    for i, s in enumerate(samples):
        R2, t2 = pre(s)[:2]
        assert np.array_equal(np.asarray(R2).reshape(3, 3), per_pair[i][0])
        assert np.array_equal(np.asarray(t2).reshape(3), per_pair[i][1])


def test_compute_sift_route_writes_the_npz(tmp_path):
    """compute.py -m SIFT --sift-detector hip over a small Map-free tree: the npz equals SIFT_matcher's own matches, and
    Precomputed + E-mat on it gives the pose the online plugin gives"""
    from PIL import Image
    from mapfree_reloc_amd import compute, wire
    from mapfree_reloc_amd.matchers import SIFT_matcher
    sc = tmp_path / "val" / "s00000"
    (sc / "seq0").mkdir(parents=True); (sc / "seq1").mkdir()
    p = IM.synthetic_pair(21)
    Image.fromarray(_u8(p["img0"])).save(sc / "seq0" / "frame_00000.jpg", quality=95)
    lp = ["# frame qw qx qy qz tx ty tz", "seq0/frame_00000.jpg 1 0 0 0 0 0 0"]
    for i in range(2):
        q = IM.synthetic_pair(21 if i == 0 else 40)
        Image.fromarray(_u8(q["img1"])).save(sc / "seq1" / f"frame_{i:05d}.jpg", quality=95)
        lp.append(f"seq1/frame_{i:05d}.jpg 1 0 0 0 0 0 0")
    (sc / "poses.txt").write_text("\n".join(lp) + "\n")
    compute.main(["-ds", "Mapfree", "-m", "SIFT", "--sift-detector", "hip", "--data_root", str(tmp_path)])
    got = wire.load_correspondences(str(sc / "correspondences_SIFT.npz"))
    m = SIFT_matcher((540, 720), detector="hip")
    for i in range(2):
        want = m.match((str(sc / "seq0" / "frame_00000.jpg"), str(sc / "seq1" / f"frame_{i:05d}.jpg")))
        g = wire.strip_nan(got[i])
        assert np.array_equal(np.concatenate(g, 1), want.astype(np.float32))
    assert len(wire.strip_nan(got[0])[0]) > 100
