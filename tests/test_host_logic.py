"""CPU tests of the host-side logic (no GPU): config schema + merge rules, wire format, sharding,
quaternion / submission formatting, C-ABI symbol export, gloo world-size-2 gather."""
import ctypes
import io
import os
import re
import subprocess
import sys
import zipfile

import numpy as np
import pytest
import torch

import mapfree_reloc_amd as mfr
from mapfree_reloc_amd import parallel, wire
from mapfree_reloc_amd.config import get_cfg_defaults
from mapfree_reloc_amd.submission import Pose, mat2quat, records_to_results, save_submission

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_config_rejects_unknown_keys_and_decodes_none(tmp_path):
    cfg = get_cfg_defaults()
    y = tmp_path / "a.yaml"
    y.write_text("MODEL: 'FeatureMatching'\nPOSE_SOLVER: 'PNP'\nDATASET:\n  SCENES: None\n  HEIGHT: 720\nPNP:\n  RANSAC_ITER: 1000\n")
    cfg.merge_from_file(str(y))
    assert cfg.MODEL == "FeatureMatching" and cfg.DATASET.SCENES is None and cfg.PNP.RANSAC_ITER == 1000
    bad = tmp_path / "b.yaml"
    bad.write_text("NOT_A_KEY: 1\n")
    with pytest.raises(KeyError):
        cfg.merge_from_file(str(bad))


def test_every_reference_matching_config_merges(golden_dir):
    """the reference's own yaml files must load unchanged (drop-in config surface); copies of its config/{mapfree,scannet,sevenscenes}.yaml
    and config/matching/ are kept under tests/golden/ref_config/"""
    import glob
    conf = os.path.join(golden_dir, "ref_config")
    files = glob.glob(os.path.join(conf, "matching", "**", "*.yaml"), recursive=True)
    assert len(files) >= 50
    for ds in ("mapfree", "scannet", "sevenscenes"):
        for f in [x for x in files if f"/{ds}/" in x]:
            cfg = get_cfg_defaults()
            cfg.merge_from_file(os.path.join(conf, f"{ds}.yaml"))
            cfg.merge_from_file(f)
            assert cfg.MODEL == "FeatureMatching" and cfg.POSE_SOLVER in ("EssentialMatrix", "EssentialMatrixMetric", "PNP", "Procrustes")


def test_wire_format_roundtrip_and_device_layout(tmp_path, golden_dir):
    g = np.load(os.path.join(golden_dir, "ref_wire_format.npz"))
    pts_list = [g[f"in{i}"] for i in range(int(g["n_pairs"]))]
    np.testing.assert_array_equal(wire.stack_pts(pts_list), g["stack"])                 # == reference stack_pts
    path = str(tmp_path / "correspondences_SG.npz")
    wire.save_correspondences(path, pts_list)
    corr = wire.load_correspondences(path)
    assert corr.dtype == np.float32
    for i in range(len(pts_list)):
        p1, p2 = wire.strip_nan(corr[i])
        np.testing.assert_array_equal(p1, g[f"p1_{i}"]); np.testing.assert_array_equal(p2, g[f"p2_{i}"])
    p0, p1, n = wire.pts_rows_to_device_batch(list(corr))
    assert n.tolist() == [17, 0, 5, 1, 33, 8]
    back = wire.device_batch_to_pts_list(p0, p1, n)
    assert np.isnan(back[1]).all() and back[1].shape == (1, 4)                          # matchers.py:59,120
    np.testing.assert_array_equal(back[4].astype(np.float32), pts_list[4].astype(np.float32))


def test_shard_helpers():
    for n, w in [(10, 4), (3, 8), (15000, 8), (0, 2)]:
        rs = [parallel.shard_range(n, w, r) for r in range(w)]
        assert rs[0][0] == 0 and rs[-1][1] == n and all(a[1] == b[0] for a, b in zip(rs, rs[1:]))
        sizes = [b - a for a, b in rs]
        assert max(sizes) - min(sizes) <= 1
    sc = parallel.shard_scenes([116] * 130, 8)
    assert sc[0][0] == 0 and sc[-1][1] == 130 and all(a[1] == b[0] for a, b in zip(sc, sc[1:]))
    assert max(b - a for a, b in sc) - min(b - a for a, b in sc) <= 1


def test_mat2quat_and_pose_line_format():
    rng = np.random.default_rng(0)
    from mapfree_reloc_amd import synth
    for _ in range(50):
        R = synth.rand_rot(rng, 180)
        q = mat2quat(R)
        w, x, y, z = q
        R2 = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                       [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                       [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        np.testing.assert_allclose(R2, R, atol=1e-12)
        assert q[0] >= 0 and abs(np.linalg.norm(q) - 1) < 1e-12
    p = Pose("seq1/frame_00005.jpg", np.array([0.9990001, -0.01, 0.02, 0.03], np.float32),
             np.array([0.5, -1.25, 2.0], np.float32), 457)
    assert str(p) == "seq1/frame_00005.jpg 0.999000 -0.010000 0.020000 0.030000 0.500000 -1.250000 2.000000 457"


def test_records_to_submission_zip(tmp_path):
    rec = np.array([[5, 1, 0, 0, 0, 0.1, 0.2, 0.3, 40, 0],
                    [0, np.nan, np.nan, np.nan, np.nan, np.nan, np.nan, np.nan, 0, 3],
                    [10, 0.5, 0.5, 0.5, 0.5, 1, 2, 3, 7, 0]], dtype=np.float64)
    names = {0: ("s00001", "seq1/frame_00000.jpg"), 5: ("s00001", "seq1/frame_00005.jpg"), 10: ("s00002", "seq1/frame_00010.jpg")}
    res = records_to_results(rec, names)
    assert list(res) == ["s00001", "s00002"] and len(res["s00001"]) == 1          # failed pair dropped (:48-49)
    out = tmp_path / "submission.zip"
    save_submission(res, out)
    with zipfile.ZipFile(out) as z:
        assert sorted(z.namelist()) == ["pose_s00001.txt", "pose_s00002.txt"]
        assert z.read("pose_s00001.txt").decode() == "seq1/frame_00005.jpg 1.000000 0.000000 0.000000 0.000000 0.100000 0.200000 0.300000 40"


def test_cabi_library_exports_every_declared_symbol():
    """libmfr_hip.so loads without a GPU and exports exactly what include/mfr_hip.h declares"""
    hdr = open(os.path.join(ROOT, "include", "mfr_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(mfr_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) >= 20
    lib = mfr._lib.load()
    assert set(mfr._lib.SIGNATURES) == declared
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.mfr_abi_version() == 6 and lib.mfr_target_arch() == b"gfx950"
    assert lib.mfr_pnp_workspace_bytes(16, 1024, 1000) > 0
    # ... and INTEGRATION.md's table names every one of them beside the reference interface it replaces (workspace-size queries as a family)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert [n for n in sorted(declared) if n not in doc and not n.endswith("_workspace_bytes")] == []


def test_no_cpu_fallback_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from mapfree_reloc_amd import solver_ops as ops
    with pytest.raises(mfr._lib.MfrLibraryError):
        ops.PnPBatchSolver()(torch.zeros(1, 4, 2), torch.zeros(1, 4, 2), torch.zeros(1, dtype=torch.int32),
                             torch.zeros(1, 8, 8), torch.eye(3)[None], torch.eye(3)[None], torch.zeros(1, dtype=torch.int64))


def test_product_never_imports_oracle():
    """the oracle is test infrastructure: nothing under the product package may import / link it"""
    pkg = os.path.join(ROOT, "map-free-reloc_amd")
    pat = re.compile(r"^\s*(from\s+oracle|import\s+oracle|#include\s+.*oracle)", re.M)
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith((".py", ".hip", ".h")) or f == "Makefile":
                src = open(os.path.join(dp, f)).read()
                assert not pat.search(src), (dp, f)
                assert "libmfr_oracle" not in src and "oracle_lib" not in src, (dp, f)


_GLOO_WORKER = r'''
import os, sys
sys.path.insert(0, %r)
import numpy as np, torch, torch.distributed as dist
from mapfree_reloc_amd import parallel
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo")
lo, hi = parallel.shard_range(11, world, rank)
n = hi - lo
ids = torch.arange(lo, hi, dtype=torch.int64)
R = torch.eye(3, dtype=torch.float64)[None].repeat(n, 1, 1)
if rank == 1 and n:
    R[0] = float("nan")
out = dict(R=R, t=torch.arange(lo, hi, dtype=torch.float64)[:, None].repeat(1, 3), n_inliers=torch.arange(lo, hi, dtype=torch.int32),
           status=torch.zeros(n, dtype=torch.int32))
rec = parallel.gather_pose_records(ids, out, world)
assert rec.shape == (11, 10), rec.shape
assert rec[:, 0].tolist() == list(range(11))
assert torch.equal(rec[:, 8], torch.arange(11, dtype=torch.float64))
assert torch.isnan(rec[6, 1:5]).all() and not torch.isnan(rec[5, 1:5]).any()
dist.destroy_process_group()
print("rank", rank, "ok")
'''


def test_gather_pose_records_gloo_world2(tmp_path):
    script = tmp_path / "w.py"
    script.write_text(_GLOO_WORKER % ROOT)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29617", str(script)],
                       capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.count("ok") == 2


def test_mapfree_scene_reader_on_synthetic_tree(tmp_path):
    """directory layout / file formats of README.md:60-120 read back with the reference's conventions"""
    from PIL import Image
    from mapfree_reloc_amd.datasets import MapFreeScene, collate_batch1
    sc = tmp_path / "val" / "s00460"
    (sc / "seq0").mkdir(parents=True); (sc / "seq1").mkdir()
    rng = np.random.default_rng(0)
    lines_p, lines_k = ["# comment"], ["# comment"]
    names = ["seq0/frame_00000.jpg"] + [f"seq1/frame_{i:05d}.jpg" for i in range(12)]
    for i, nme in enumerate(names):
        Image.fromarray(rng.integers(0, 255, (96, 72, 3), dtype=np.uint8)).save(sc / nme, format="PNG")
        depth = (rng.uniform(0.5, 6.0, (48, 36)) * 1000).astype(np.uint16)
        Image.fromarray(depth).save(str(sc / nme).replace(".jpg", ".dptkitti.png"))
        q = np.array([1.0, 0, 0, 0]) if i == 0 else rng.normal(size=4); q /= np.linalg.norm(q)
        t = np.zeros(3) if i == 0 else rng.normal(size=3)
        lines_p.append(nme + " " + " ".join(f"{v:.8f}" for v in np.r_[q, t]))
        lines_k.append(nme + " 100.0 110.0 35.5 47.5 72 96")
    (sc / "poses.txt").write_text("\n".join(lines_p) + "\n"); (sc / "intrinsics.txt").write_text("\n".join(lines_k) + "\n")
    ds = MapFreeScene(sc, resize=(36, 48), sample_factor=5, estimated_depth="dptkitti")
    assert len(ds) == 3 and [p[3] for p in ds.pairs] == [0, 5, 10]                     # every 5th query frame
    d = ds[1]
    assert d["pair_id"] == 5 and d["pair_names"] == ("seq0/frame_00000.jpg", "seq1/frame_00005.jpg")
    assert d["image0"].shape == (3, 48, 36) and d["image0"].dtype == torch.float32 and float(d["image0"].max()) <= 1.0
    assert d["depth0"].shape == (48, 36) and 0.4 < float(d["depth0"].mean()) < 7.0      # uint16 mm / 1000
    K = d["K_color0"].numpy()
    np.testing.assert_allclose(K, [[50.0, 0, 0.5 * 35.5 + 0.25 - 0.5], [0, 55.0, 0.5 * 47.5 + 0.25 - 0.5], [0, 0, 1]])
    # seq0 pose is the identity -> relative pose == absolute pose of the query (mapfree.py:240-243)
    from mapfree_reloc_amd import evaluation as E
    q2 = np.array(list(map(float, lines_p[1 + 1 + 5].split(" ")[1:5]))); t2 = np.array(list(map(float, lines_p[1 + 1 + 5].split(" ")[5:])))
    np.testing.assert_allclose(d["T_0to1"][:3, :3].numpy(), E.quat2mat(q2), atol=1e-6)
    np.testing.assert_allclose(d["T_0to1"][:3, 3].numpy(), t2, atol=1e-6)
    b = collate_batch1(d)
    assert b["depth0"].shape == (1, 48, 36) and b["scene_id"] == ["s00460"] and b["pair_names"][1] == ["seq1/frame_00005.jpg"]


def test_superglue_weight_folding_is_exact_algebra():
    """nets/superglue.fold_weights re-associates the upstream GNN layer (merge projection folded into mlp.0, b2 carried
    as an offset, BatchNorm folded, head-major channels): the fused f32 operands, driven by a plain float64 softmax
    attention, must reproduce the upstream graph (oracle/nets_ref.SuperGlueRef, a restatement with upstream
    parameter names) to rounding."""
    import torch
    from mapfree_reloc_amd.nets import weights as WT
    from mapfree_reloc_amd.nets.superglue import fold_weights
    from oracle import nets_ref
    torch.manual_seed(0)
    sd = WT.superglue_state_dict()
    # make every folded term matter: random biases and non-trivial BatchNorm statistics
    g = torch.Generator().manual_seed(1)
    for k in sd:
        if k.endswith(".bias") and ("gnn" in k or "final_proj" in k):
            sd[k] = 0.1 * torch.randn(sd[k].shape, generator=g)
        if k.endswith("running_mean"):
            sd[k] = 0.1 * torch.randn(sd[k].shape, generator=g)
        if k.endswith("running_var"):
            sd[k] = 0.5 + torch.rand(sd[k].shape, generator=g)
    # ... and the terms the recipe leaves trivial: the last keypoint-encoder bias (zero), gamma / beta of the keypoint encoder's
    # BatchNorms (1 +- 0.05 / 0.05) and the dustbin score (1.0)
    sd["kenc.encoder.12.bias"] = 0.1 * torch.randn(256, generator=g)
    for i in (1, 4, 7, 10):
        c = sd[f"kenc.encoder.{i}.weight"].numel()
        sd[f"kenc.encoder.{i}.weight"] = 0.5 + torch.rand(c, generator=g)
        sd[f"kenc.encoder.{i}.bias"] = 0.2 * torch.randn(c, generator=g)
    sd["bin_score"] = torch.tensor(2.37)
    ref = nets_ref.SuperGlueRef().double().eval()
    ref.load_state_dict({k: v.double() for k, v in sd.items()})
    n0, n1, H, W = 37, 29, 120, 160
    k0 = torch.rand(1, n0, 2, generator=g).double() * torch.tensor([W, H]); k1 = torch.rand(1, n1, 2, generator=g).double() * torch.tensor([W, H])
    s0, s1 = torch.rand(1, n0, generator=g).double(), torch.rand(1, n1, generator=g).double()
    d0 = torch.nn.functional.normalize(torch.randn(1, 256, n0, generator=g).double(), dim=1)
    d1 = torch.nn.functional.normalize(torch.randn(1, 256, n1, generator=g).double(), dim=1)
    out = ref(k0, s0, d0, k1, s1, d1, (H, W))

    fw = fold_weights(sd)
    assert fw["bin_score"] == float(torch.tensor(2.37)) == float(ref.bin_score.detach())

    def run(kp, sc, de, kp_o, sc_o, de_o):
        def enc(kp, sc, de):
            kn = (kp[0] - torch.tensor([W / 2, H / 2])) / (max(W, H) * 0.7)
            h = torch.cat([kn, sc[0, :, None]], -1)
            for i, (w, b) in enumerate(fw["kenc"]):
                h = h @ w.double().t() + b.double()
                if i < 4:
                    h = h.relu()
            return de[0].t() + h
        xs = [enc(kp, sc, de), enc(kp_o, sc_o, de_o)]
        for L in fw["layers"]:
            qkv = [x @ L["wqkv"].double().t() + L["bqkv"].double() for x in xs]
            new = []
            for i in (0, 1):
                src = qkv[1 - i] if L["cross"] else qkv[i]
                a = []
                for h in range(4):
                    q, k, v = qkv[i][:, 64 * h:64 * h + 64], src[:, 256 + 64 * h:256 + 64 * h + 64], src[:, 512 + 64 * h:512 + 64 * h + 64]
                    a.append(torch.softmax(q @ k.t() / 8.0, -1) @ v)
                hid = (torch.cat([xs[i]] + a, -1) @ L["w1"].double().t() + L["b1"].double()).relu()
                new.append(xs[i] + hid @ L["w2"].double().t())
            xs = new
        return [x @ fw["wf"].double().t() + fw["bf"].double() for x in xs]

    m0, m1 = run(k0, s0, d0, k1, s1, d1)
    np.testing.assert_allclose(m0.t().numpy(), out["mdesc0"][0].numpy(), rtol=0, atol=2e-5)
    np.testing.assert_allclose(m1.t().numpy(), out["mdesc1"][0].numpy(), rtol=0, atol=2e-5)


def test_descriptor_matcher_packs_ragged_inputs():
    """host-side packing of per-image (keypoints, descriptors) lists into the fixed-stride layout of the C-ABI
    (descriptor_ops.DescriptorRatioMatcher._pack; pure host code, runs without a GPU)"""
    import torch
    from mapfree_reloc_amd.descriptor_ops import DescriptorRatioMatcher
    rng = np.random.default_rng(0)
    items = [(rng.random((n, 2)).astype(np.float32), rng.random((n, 128)).astype(np.float32)) for n in (5, 0, 17)]
    kp, de, n = DescriptorRatioMatcher(0.8, "cpu")._pack(items)
    assert kp.shape == (3, 17, 2) and de.shape == (3, 17, 128) and n.dtype == torch.int32 and n.tolist() == [5, 0, 17]
    np.testing.assert_array_equal(kp[0, :5].numpy(), items[0][0]); assert (kp[0, 5:] == 0).all() and (de[1] == 0).all()
    np.testing.assert_array_equal(de[2].numpy(), items[2][1])
    # all-empty batch still yields a valid (1-row) stride
    kp, de, n = DescriptorRatioMatcher(0.8, "cpu")._pack([(np.zeros((0, 2), np.float32), np.zeros((0, 128), np.float32))])
    assert kp.shape == (1, 1, 2) and n.tolist() == [0]


def test_plugin_image_staging_equals_the_torch_path():
    """matching/feature_matching._GrayPairStage (numpy on the calling thread, persistent buffer) produces bit for bit what
    datasets.to_gray + torch.stack produced, for colour and single-channel inputs, and reuses its buffer across pairs"""
    from mapfree_reloc_amd.datasets import to_gray
    from mapfree_reloc_amd.matching.feature_matching import _GrayPairStage
    st = _GrayPairStage()
    g = torch.Generator().manual_seed(0)
    for C in (3, 1, 3):
        d = {"image0": torch.rand(1, C, 48, 36, generator=g), "image1": torch.rand(1, C, 48, 36, generator=g)}
        out = st(d)
        ref = torch.stack([to_gray(d["image0"][0]), to_gray(d["image1"][0])])[:, None].to(torch.float32)
        assert out.shape == (2, 1, 48, 36) and out.dtype == torch.float32 and torch.equal(out, ref)
    assert st(d) is out                                        # same persistent buffer
    assert st({"image0": torch.rand(1, 3, 24, 20), "image1": torch.rand(1, 3, 24, 20)}).shape == (2, 1, 24, 20)


def test_sharding_and_sampler_properties():
    """size-independent properties: shard_range partitions [0, n) in order for any world size; shard_scenes keeps scenes whole, in order
    and balanced to within one scene's weight; the scene-balanced sampler's epoch is the same multiset whatever the world size"""
    from hypothesis import given, settings, strategies as st
    from mapfree_reloc_amd.datasets import SceneBalancedSampler
    from mapfree_reloc_amd.parallel import shard_range, shard_scenes

    @settings(max_examples=60, deadline=None)
    @given(st.integers(0, 5000), st.integers(1, 16))
    def ranges(n, world):
        parts = [shard_range(n, world, r) for r in range(world)]
        flat = [i for lo, hi in parts for i in range(lo, hi)]
        assert flat == list(range(n)) and max(hi - lo for lo, hi in parts) - min(hi - lo for lo, hi in parts) <= 1
    ranges()

    @settings(max_examples=60, deadline=None)
    @given(st.lists(st.integers(1, 600), min_size=1, max_size=40), st.integers(1, 8))
    def scenes(sizes, world):
        blocks = shard_scenes(sizes, world)
        assert len(blocks) == world
        flat = [i for b in blocks for i in (range(*b) if isinstance(b, tuple) else b)]
        assert flat == list(range(len(sizes)))                  # every scene exactly once, in order, contiguous blocks
    scenes()

    @settings(max_examples=30, deadline=None)
    @given(st.lists(st.integers(1, 50), min_size=1, max_size=8), st.integers(1, 12), st.booleans(), st.integers(1, 5))
    def sampler(sizes, n, repl, world):
        whole = sorted(SceneBalancedSampler(sizes, n, repl).epoch_indices().tolist())
        dealt = sorted(i for r in range(world) for i in SceneBalancedSampler(sizes, n, repl, rank=r, world=world))
        assert whole == dealt and len(whole) == n * len(sizes)
        bounds = np.cumsum([0] + sizes)
        assert all(sum(bounds[k] <= i < bounds[k + 1] for i in whole) == n for k in range(len(sizes)))
    sampler()


def test_resize_is_cv2_inter_linear_not_pil_bilinear():
    """cv2.resize(INTER_LINEAR) = half-pixel bilinear without antialiasing; at the exact 2x downscale of the regression
    configs (720x540 -> 360x270) that is the 2x2 box average, which PIL's Image.BILINEAR (widened triangle filter) is not"""
    from mapfree_reloc_amd.datasets import resize_bilinear_u8
    rng = np.random.default_rng(0)
    a = rng.integers(0, 256, (72, 54, 3), dtype=np.uint8)
    got = resize_bilinear_u8(a, (27, 36))
    box = np.floor(a.reshape(36, 2, 27, 2, 3).astype(np.float32).mean((1, 3)) + 0.5).astype(np.uint8)
    assert np.array_equal(got, box)
    # identity and an up-scale: corners map with edge clamping, interior is the 4-tap interpolation
    assert resize_bilinear_u8(a, (54, 72)) is a
    up = resize_bilinear_u8(a, (108, 144))
    assert up.shape == (144, 108, 3) and np.array_equal(up[0, 0], a[0, 0]) and np.array_equal(up[-1, -1], a[-1, -1])
    # against torch's half-pixel bilinear (antialias off) at a non-integer factor: same arithmetic up to the final rounding
    import torch.nn.functional as F
    t = torch.from_numpy(a).permute(2, 0, 1)[None].float()
    ref = F.interpolate(t, size=(50, 31), mode="bilinear", align_corners=False, antialias=False)[0].permute(1, 2, 0).numpy()
    assert np.abs(resize_bilinear_u8(a, (31, 50)).astype(np.float32) - ref).max() <= 0.5 + 1e-3


def test_run_signature_ties_resume_to_the_configuration():
    from mapfree_reloc_amd.config import get_cfg_defaults
    from mapfree_reloc_amd.submission import _run_signature
    a, b = get_cfg_defaults(), get_cfg_defaults()
    assert _run_signature(a, "val") == _run_signature(b, "val") != _run_signature(a, "test")
    b.POSE_SOLVER = "EssentialMatrixMetric"
    assert _run_signature(a, "val") != _run_signature(b, "val")


def test_pair_batch_loader_equals_the_per_sample_reader(tmp_path):
    """PairBatchLoader (decode threads writing straight into the batch buffers, the scene keyframe decoded once, batches spanning
    scenes) hands out exactly what the per-pair reader + to_gray produce, pair by pair, in submission order"""
    from PIL import Image
    from mapfree_reloc_amd.datasets import MapFreeScene, PairBatchLoader, to_gray
    rng = np.random.default_rng(1)
    scenes = []
    for s in range(3):
        sc = tmp_path / "test" / f"s{s:05d}"
        (sc / "seq0").mkdir(parents=True); (sc / "seq1").mkdir()
        lp, lk = ["# c"], ["# c"]
        for nme in ["seq0/frame_00000.jpg"] + [f"seq1/frame_{i:05d}.jpg" for i in range(7)]:
            Image.fromarray(rng.integers(0, 255, (48, 36, 3), dtype=np.uint8)).save(sc / nme, format="PNG")
            Image.fromarray((rng.uniform(0.5, 6.0, (48, 36)) * 1000).astype(np.uint16)).save(str(sc / nme).replace(".jpg", ".dptkitti.png"))
            lp.append(nme + " 1 0 0 0 0 0 0"); lk.append(nme + f" {100.0 + s} 110.0 17.5 23.5 36 48")
        (sc / "poses.txt").write_text("\n".join(lp) + "\n"); (sc / "intrinsics.txt").write_text("\n".join(lk) + "\n")
        scenes.append(MapFreeScene(sc, resize=(36, 48), sample_factor=1, estimated_depth="dptkitti"))
    ref = [(si, i, sc[i]) for si, sc in enumerate(scenes) for i in range(len(sc))]
    assert len(ref) == 21
    from mapfree_reloc_amd import datasets as D
    # the loaders decode gray planes / depth straight from the files' bytes (read_gray_plane / read_depth_plane: csrc/libmfr_host.so, or the
    # numpy expressions without it): both must hand out the per-sample reader's values bit for bit
    modes = [(1, "thread", True), (4, "thread", True), (3, "process", True), (2, "thread", False), (2, "process", False)]
    for workers, decode, use_host_lib in modes:               # "process": worker processes writing into shared-memory batch slots
        D._HOST_LIB = False if use_host_lib else None
        D.clear_frame_cache()
        got = 0
        ld = PairBatchLoader(scenes, batch_pairs=8, prefetch=2, pin=False, workers=workers, decode=decode)
        for b in ld:
            for p in range(len(b["names"])):
                si, i, smp = ref[got]
                assert b["scene_ids"][p] == scenes[si].scene_id and b["names"][p] == smp["pair_names"][1] and int(b["seed_ids"][p]) == smp["pair_id"]
                assert torch.equal(b["images"][2 * p, 0], to_gray(smp["image0"])) and torch.equal(b["images"][2 * p + 1, 0], to_gray(smp["image1"]))
                assert torch.equal(b["depth0"][p], smp["depth0"]) and torch.equal(b["depth1"][p], smp["depth1"])
                assert b["K0"].dtype == torch.float64 and torch.equal(b["K0"][p], smp["K_color0"]) and torch.equal(b["K1"][p], smp["K_color1"])
                assert b["ref_keys"][p][:2] == (scenes[si].scene_root, smp["pair_names"][0])  # every pair of these scenes shares its keyframe
                st = os.stat(os.path.join(scenes[si].scene_root, smp["pair_names"][0]))
                assert b["ref_keys"][p][2:] == (st.st_mtime_ns, st.st_size)                   # ... identified by its file, not only by its name
                got += 1
        ld.close()
        assert got == 21
    D._HOST_LIB = False


def test_gray_and_depth_planes_equal_the_reference_readers(tmp_path):
    """read_gray_plane == the matcher's read_image (8-bit luma of the file, float resize, / 255: PIL's own "L" conversion is the independent
    statement here) == to_gray(read_color_image) at the file's own size, and read_depth_plane == read_depth_image, bit for bit: with and
    without the C helper, with real resizes, for a JPEG, a gray-mode file (converted to RGB like the reference's loader) and depth values
    over the whole uint16 range"""
    from PIL import Image
    from mapfree_reloc_amd import datasets as D, matchers as MT
    rng = np.random.default_rng(5)
    Image.fromarray(rng.integers(0, 256, (90, 70, 3), dtype=np.uint8)).save(tmp_path / "a.jpg", quality=90)
    Image.fromarray(rng.integers(0, 256, (90, 70), dtype=np.uint8)).save(tmp_path / "b.png")
    Image.fromarray(np.concatenate([np.arange(65536, dtype=np.uint16), rng.integers(0, 65536, 6464, dtype=np.uint16)]).reshape(300, 240)).save(tmp_path / "d.png")
    try:
        for lib in (False, None):
            D._HOST_LIB = lib
            if lib is False and D._host_lib() is None:
                continue                                        # helper not built here: the numpy leg below covers the values
            for f in ("a.jpg", "b.png"):
                l8 = np.asarray(Image.open(tmp_path / f).convert("RGB").convert("L"))
                for rs in (None, (70, 90), (35, 45), (140, 181)):
                    want = D.resize_bilinear_f32(l8.astype(np.float32), rs) / np.float32(255) if rs else l8.astype(np.float32) / np.float32(255)
                    got = D.read_gray_plane(str(tmp_path / f), rs)
                    out = np.full(want.shape, -1.0, np.float32)
                    assert got.dtype == np.float32 and np.array_equal(got, want) and np.array_equal(D.read_gray_plane(str(tmp_path / f), rs, out), want)
                    if rs is not None:
                        assert np.array_equal(MT.read_image(str(tmp_path / f), rs), want)            # the offline matchers read THIS plane
                    if rs in (None, (70, 90)):                  # the per-sample route (colour image / 255 -> to_gray) lands on the same bytes
                        assert np.array_equal(D.to_gray(D.read_color_image(str(tmp_path / f), rs)).numpy(), want)
            want = D.read_depth_image(str(tmp_path / "d.png")).numpy()
            assert np.array_equal(D.read_depth_plane(str(tmp_path / "d.png")), want)
            out = np.empty_like(want)
            D.read_depth_plane(str(tmp_path / "d.png"), out)
            assert np.array_equal(out, want)
    finally:
        D._HOST_LIB = False


def test_loader_routes_agree_at_a_real_resize(tmp_path):
    """with a NON-native cfg resize the fast loader route (luma first, float resize) and the per-sample route (8-bit RGB resize
    first, rounded luma) are different planes, so the fast route must not be taken: gray_pair() returns None, and the batched loader delivers exactly
    to_gray(sample image) -- the plane of the per-pair plugin -- for every pair; at the native size the fast route is taken and gives the same bytes"""
    from PIL import Image
    from mapfree_reloc_amd import datasets as D
    rng = np.random.default_rng(3)
    sc = tmp_path / "s00000"
    (sc / "seq0").mkdir(parents=True); (sc / "seq1").mkdir()
    names = ["seq0/frame_00000.jpg"] + [f"seq1/frame_{5 * k:05d}.jpg" for k in range(3)]
    for nme in names:
        Image.fromarray(rng.integers(0, 256, (96, 72, 3), dtype=np.uint8)).save(sc / nme, quality=95)
    (sc / "poses.txt").write_text("\n".join(f"{n} 1 0 0 0 0 0 0" for n in names))
    (sc / "intrinsics.txt").write_text("\n".join(f"{n} 60.0 60.0 35.5 47.5 72 96" for n in names))
    D.clear_frame_cache()
    for rs, native in (((72, 96), True), ((54, 72), False), (None, True)):
        scene = D.MapFreeScene(str(sc), rs, sample_factor=1)
        assert scene.resize_is_native() == native and (scene.gray_pair(0) is None) == (not native)
        loader = D.PairBatchLoader([scene], 2, prefetch=1, pin=False, workers=2, decode="thread")
        try:
            got = [b for b in loader]
        finally:
            loader.close()
        ims = np.concatenate([b["images"].numpy() for b in got])                   # [2 n, 1, h, w]
        for i in range(len(scene)):
            smp = scene[i]
            assert np.array_equal(ims[2 * i, 0], D.to_gray(smp["image0"]).numpy()), (rs, i)
            assert np.array_equal(ims[2 * i + 1, 0], D.to_gray(smp["image1"]).numpy()), (rs, i)
        if not native:                                                              # ... and that is NOT what the fast route would have produced
            fast = D.read_gray_plane(str(sc / names[1]), rs)
            assert np.abs(fast - ims[1, 0]).max() > 0.5 / 255
    # float inputs a hair outside [0, 1] clip instead of wrapping modulo 256
    x = np.zeros((3, 2, 2), np.float32); x[:, 0, 0] = 1.0 + 3e-3; x[:, 1, 1] = -2e-3
    g = D.to_gray(torch.from_numpy(x).requires_grad_(False)).numpy()
    assert g[0, 0] == 1.0 and g[1, 1] == 0.0


def test_gray_plane_is_byte_rounded_luma_on_every_route():
    """VERDICT r4 missing-4: the online / fused routes used to feed SuperPoint the UNROUNDED float luma while the offline route reads an 8-bit
    gray image.  Now to_gray (CPU numpy, torch CPU tensor) and the online plugin's stage give exactly float32(luma_u8) / 255."""
    import torch
    from mapfree_reloc_amd import datasets as D
    from mapfree_reloc_amd.matching.feature_matching import _GrayPairStage
    rng = np.random.default_rng(11)
    rgb = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    want = D.luma_u8(rgb).astype(np.float32) / np.float32(255)
    assert set(np.unique(np.rint(want * 255) - want * 255)) <= {0.0} or np.abs(np.rint(want * 255) - want * 255).max() < 1e-4
    img = torch.from_numpy(np.ascontiguousarray(rgb.transpose(2, 0, 1)).astype(np.float32) / np.float32(255))
    assert np.array_equal(D.to_gray(img).numpy(), want)
    assert np.array_equal(D.to_gray(img[:1])[None].numpy()[0], img[0].numpy())                     # single channel: passes through
    st = _GrayPairStage()({"image0": img[None], "image1": img[None].flip(-1)})
    assert st.shape == (2, 1, 37, 53) and np.array_equal(st[0, 0].numpy(), want) and np.array_equal(st[1, 0].numpy(), want[:, ::-1])
    # and it is NOT the float luma of rounds 1-4 (up to half a grey level away)
    old = np.float32(0.299) * img[0].numpy() + np.float32(0.587) * img[1].numpy() + np.float32(0.114) * img[2].numpy()
    assert 0.4 / 255 < np.abs(old - want).max() <= 0.51 / 255


def test_bench_module_contract_pieces_importable():
    """bench.py parses its defaults, its workloads carry the strings the JSON line prints, the census summary reads the committed
    profiles (no GPU needed for any of this)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    a = b.parse([])
    assert a.gpus == 1 and a.config == "sg_pnp" and a.steps > 0 and a.rpr_opts == "siamese,graph"
    for wl in (b.SgPnpWorkload, b.LoftrEmatWorkload):
        dt = wl.dtype.fget(None)                            # (a property: the string names the arithmetic HIP.SPLIT selects)
        assert isinstance(dt, str) and "f16" in dt and isinstance(wl.metric, str) and isinstance(wl.workload, str)
    c = b.census_summary()
    assert c["hard2"]["sg_pnp"]["pose_within_bar"] == c["hard2"]["sg_pnp"]["pairs"] and c["hard1"]["sg_pnp"]["inlier_index_sets_identical"] == 64


def test_bench_plain_run_is_lean_and_dumps_outputs(tmp_path):
    """a plain bench.py run measures only the headline (no kernel timers, CPU baseline or secondary lines: those are --full), and
    --dump-outputs writes float32 / float64 .npy files, sampling an array that exceeds its share of the 64 MB budget"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    a = b.parse(["--steps", "7", "--dump-outputs", str(tmp_path)])
    assert a.steps == 7 and not a.full and a.no_kernel_timer and a.no_cpu_baseline and a.no_secondary and a.dump_outputs == str(tmp_path)
    f = b.parse(["--full"])
    assert f.full and not f.no_kernel_timer and not f.no_cpu_baseline and not f.no_secondary
    big = torch.arange(9 << 20, dtype=torch.float32)
    b.dump_outputs(str(tmp_path), {"R": torch.eye(3, dtype=torch.float64)[None], "status": torch.tensor([0, 7], dtype=torch.int32), "big": big})
    R, st, s = (np.load(tmp_path / f"{n}.npy") for n in ("R", "status", "big"))
    assert R.dtype == np.float64 and R.shape == (1, 3, 3) and st.dtype == np.float64 and st.tolist() == [0.0, 7.0]
    assert s.dtype == np.float32 and s.nbytes <= b.DUMP_LIMIT_BYTES // 3 and np.all(np.diff(s) > 0)
    b.dump_outputs(str(tmp_path / "again"), {"R": torch.eye(3, dtype=torch.float64)[None], "status": torch.zeros(2), "big": big})
    assert np.array_equal(np.load(tmp_path / "again" / "big.npy"), s)                 # the same sample every time


def test_round5_entry_points_reject_bad_arguments_before_touching_a_device():
    """argument validation of the entry points added in round 5 (no GPU needed: MFR_E_ARG comes back before any launch)"""
    lib = mfr._lib.load()
    E_ARG = -1
    assert lib.mfr_gemm_f16x2_pack_bytes(8, 33) == 0 and lib.mfr_gemm_f16x2_pack_bytes(8, 64) > 0          # K % 32
    assert lib.mfr_gemm_f16x2_pack_batched(None, 32, 1, 0, 8, 32, 1.0, None, None) == E_ARG                 # null operands
    assert lib.mfr_gemm_f16x2_batched(None, 32, 0, None, None, None, 8, 0, 1, 8, 8, 32, 0, None) == E_ARG
    assert lib.mfr_sp_conv1ab_f16x2(None, None, None, None, None, 1, 8, 8, None, None) == E_ARG
    assert lib.mfr_conv_igemm_f16x2(None, None, None, None, 1, 1, 8, 8, 1, 3, 3, 1, 1, 0, None) == E_ARG


def test_round6_entry_points_reject_bad_arguments_before_touching_a_device():
    """argument validation of the entry points added in round 6 (no GPU needed: MFR_E_ARG comes back before any launch)"""
    import ctypes as C
    lib = mfr._lib.load()
    E_ARG = -1
    dummy = C.create_string_buffer(64)
    p = C.cast(dummy, C.c_void_p)
    assert lib.mfr_conv3x3_direct_f16x2_filter_bytes(64, 64) == 4 * 54 * 1024 + 256 and lib.mfr_conv3x3_direct_f16x2_filter_bytes(0, 64) == 0
    assert lib.mfr_conv3x3_direct_f16x2_filter_bytes(196, 196) == 4 * 13 * 54 * 1024 + 4 * 256           # channels padded to 16 / 64 inside the packed filter
    assert lib.mfr_conv3x3_direct_f16x2_filter_pack(None, 4, 4, None, None) == E_ARG
    assert lib.mfr_conv3x3_direct_f16x2(None, None, None, None, 1, 4, 4, 8, 8, 0, 0, None, None) == E_ARG                 # null operands
    assert lib.mfr_conv3x3_direct_f16x2(p, p, None, None, 1, 4, 4, 8, 8, 3, 0, p, None) == E_ARG                          # unknown activation
    assert lib.mfr_conv3x3_direct_f16x2(p, p, None, p, 1, 4, 4, 8, 8, 0, 1, p, None) == E_ARG                             # residual with pooling
    assert lib.mfr_conv3x3_direct_f16x2(p, p, None, None, 1, 4, 4, 1, 8, 0, 1, p, None) == E_ARG                          # pooling needs H, W >= 2
    assert lib.mfr_conv3x3_direct_f16x2(p, p, None, None, 1, 64, 64, 40000, 40000, 0, 0, p, None) == E_ARG                # an image beyond a 2 GB buffer descriptor
    assert lib.mfr_conv3x3s2_direct_f16x2(None, None, None, 1, 4, 4, 8, 8, 0, None, None) == E_ARG
    assert lib.mfr_conv3x3s2_direct_f16x2(p, p, None, 1, 4, 4, 8, 8, 5, p, None) == E_ARG
    assert lib.mfr_conv3x3_direct_f16x2_rows(p, p, None, 1, 4, 6, 8, 8, 0, p, 8, None) == E_ARG                           # Cout % 4
    assert lib.mfr_conv3x3_direct_f16x2_rows(p, p, None, 1, 4, 8, 8, 8, 0, p, 4, None) == E_ARG                           # row stride < Cout
    assert lib.mfr_conv3x3_direct_f16x2_rows(p, p, None, 1, 4, 8, 8, 8, 0, p, 10, None) == E_ARG                          # row stride % 4
    assert lib.mfr_mlp_ln_f16x2(None, 256, 256, None, None, None, None, None, None, 1e-5, None, 128, 16, 0, None) == E_ARG


def test_wino_variant_entry_takes_only_the_kernels_that_compute_the_convolution():
    """mfr_conv3x3_wino_variant names kernel variants 0-4; the former timing-ablation numbers (10-16, 27-33: wrong results by design) are
    rejected like any other value, before any launch"""
    import ctypes as C
    lib = mfr._lib.load()
    p = C.cast(C.create_string_buffer(64), C.c_void_p)
    for v in [-1, 5, 9] + list(range(10, 17)) + [26] + list(range(27, 35)):
        assert lib.mfr_conv3x3_wino_variant(p, p, None, None, 1, 4, 32, 8, 8, 1, 0, v, p, None) == -1, v
