"""-m gpu: DPT depth on the fused route (DPT.SOURCE 'online' in submission.predict_fused): the two row-table entry points of csrc/dpt.hip, the loaders'
colour bytes, nets/dpt.FusedDepthStage inside pipeline.FusedPosePipeline.

The yardstick is code that was there before: mfr_dpt_prep / mfr_dpt_head_tail, PIL, and the per-pair plugin with DPT.SOURCE 'online'.  Every comparison is
BIT FOR BIT: the same kernels run on the same bytes (the u8 and the f32 entry of prep both compute byte / 255.f), and a map does not depend on its batch
neighbours.  Trees: rig_scenes.write_rig_tree (120 x 160 JPEGs); network: dpt_ref.REDUCED at 64 x 96 with INVERT False (test_gpu_dpt._stage_cfg)."""
import glob
import os
import sys
import zipfile

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dpt_ref as R  # noqa: E402
import rig_scenes as S  # noqa: E402
from test_gpu_dpt import _stage_cfg  # noqa: E402

from mapfree_reloc_amd import options, submission  # noqa: E402
from mapfree_reloc_amd.builder import build_model  # noqa: E402
from mapfree_reloc_amd.datasets import DevicePrefetcher, PairBatchLoader, clear_frame_cache, list_scenes, make_loader  # noqa: E402
from mapfree_reloc_amd.nets import dpt, weights as WT  # noqa: E402
from mapfree_reloc_amd.pipeline import ST_RANGE, FusedPosePipeline  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -7.0


@pytest.fixture(scope="module")
def sd():
    return R.perturbed(WT.dpt_state_dict(arch=R.REDUCED))


def _cfg(root, tmp_path, sd, solver="PNP", source="online", name="dptkitti"):
    cfg = _stage_cfg(root, tmp_path, sd, source, name)
    cfg.POSE_SOLVER = solver
    cfg.EMAT_RANSAC.PIX_THRESHOLD, cfg.EMAT_RANSAC.SCALE_THRESHOLD, cfg.EMAT_RANSAC.CONFIDENCE = 2.0, 0.1, 0.9999
    cfg.PROCRUSTES.MAX_CORR_DIST = 0.05
    cfg.HIP.LOADER_DECODE, cfg.HIP.LOADER_WORKERS = "thread", 2             # predict_fused: no decode processes to fork (seconds each, from a process this size)
    return cfg


def _hide_depth_files(root):
    """the tree's own depth maps out of the way: whoever opens one fails"""
    files = glob.glob(os.path.join(str(root), "**", "*.dptkitti.png"), recursive=True)
    assert files
    for f in files:
        os.rename(f, f + ".away")
    clear_frame_cache()


def _pil(scene_root, name):
    from PIL import Image
    return torch.from_numpy(np.asarray(Image.open(os.path.join(scene_root, name)).convert("RGB")).copy())


def _status():
    return torch.zeros(1, dtype=torch.int32, device=DEV)


# ------------------------------------------------------------------------------------------------ 1. prep_rows
@pytest.mark.parametrize("shape", [(120, 160, 64, 96), (37, 53, 32, 64)])
def test_prep_rows_equals_prep_of_the_gathered_images(shape):
    H, W, Hn, Wn = shape
    g = torch.Generator().manual_seed(H)
    img = torch.randint(0, 256, (3, H, W, 3), generator=g, dtype=torch.uint8).to(DEV)
    rows = torch.tensor([2, 0, 2], dtype=torch.int32, device=DEV)
    st = _status()
    got = dpt.prep_rows(img, rows, Hn, Wn, st)
    assert got.shape == (3, 3, Hn, Wn) and torch.equal(got, dpt.prep(img[[2, 0, 2]].contiguous(), Hn, Wn)) and int(st) == 0


def test_prep_rows_out_of_range_index_reads_nothing():
    """the three images lie between sentinel-filled neighbours: an index one past either end would read the sentinel, and its prep is not zero"""
    H, W, Hn, Wn = 37, 53, 32, 64
    g = torch.Generator().manual_seed(1)
    big = torch.full((5, H, W, 3), 200, dtype=torch.uint8, device=DEV)
    big[1:4] = torch.randint(0, 256, (3, H, W, 3), generator=g, dtype=torch.uint8).to(DEV)
    img = big[1:4]
    assert img.is_contiguous()
    st = _status()
    got = dpt.prep_rows(img, torch.tensor([2, 3, -1, 1 << 30], dtype=torch.int32, device=DEV), Hn, Wn, st)
    assert int(st) == 1
    assert torch.equal(got[0], dpt.prep(img[2:3].contiguous(), Hn, Wn)[0])
    assert not bool(got[1:].any())                                          # zeros: unlike the prep of every source, the sentinel images included
    for src in big:
        assert bool(dpt.prep(src[None].contiguous(), Hn, Wn).abs().min() > 0)   # (byte / 255 is never 0.5: no prep value is zero)


# ------------------------------------------------------------------------------------------------ 2. head_tail_rows
def _head_inputs():
    g = torch.Generator().manual_seed(4)
    f = torch.rand(2, 32, 16, 24, generator=g).to(DEV)
    w = (torch.rand(32, generator=g) * 0.2).to(DEV)
    return f, w, 0.5


@pytest.mark.parametrize("quantize", [False, True])
@pytest.mark.parametrize("with_mm", [False, True])
@pytest.mark.parametrize("invert", [False, True])
def test_head_tail_rows_scatters_the_maps(invert, with_mm, quantize):
    f, w, bias = _head_inputs()
    Ho, Wo, kw = 50, 70, dict(invert=invert, scale=0.1, shift=0.05)
    ref_m, ref_mm = dpt.head_tail(f, w, bias, Ho, Wo, millimetres=True, **kw)
    assert 0 < int(ref_mm.cpu().numpy().min()) and int(ref_mm.cpu().numpy().max()) < 65535
    src = torch.tensor([0, 1, 0], dtype=torch.int32, device=DEV)
    dst = torch.tensor([3, 0, 2], dtype=torch.int32, device=DEV)
    metres = torch.full((5, Ho, Wo), SENTINEL, device=DEV)
    mm = torch.from_numpy(np.full((5, Ho, Wo), 7, np.uint16)).to(DEV) if with_mm else None
    st = _status()
    dpt.head_tail_rows(f, w, bias, src, dst, metres, st, mm=mm, quantize=quantize, **kw)
    assert int(st) == 0
    want = dpt.millimetres_to_metres(ref_mm) if quantize else ref_m
    for s, d in ((0, 3), (1, 0), (0, 2)):
        assert torch.equal(metres[d], want[s])
        if with_mm:
            assert np.array_equal(mm[d].cpu().numpy(), ref_mm[s].cpu().numpy())
            if quantize:
                assert torch.equal(metres[d], dpt.millimetres_to_metres(mm[d]))
    for d in (1, 4):
        assert bool((metres[d] == SENTINEL).all()) and (mm is None or bool((mm[d].cpu().numpy() == 7).all()))


def test_head_tail_rows_out_of_range_indices():
    f, w, bias = _head_inputs()
    metres = torch.full((3, 20, 30), SENTINEL, device=DEV)
    st = _status()
    dpt.head_tail_rows(f, w, bias, torch.tensor([2, 0, -1], dtype=torch.int32, device=DEV), torch.tensor([1, 3, -1], dtype=torch.int32, device=DEV), metres, st)
    assert int(st) == 1
    assert not bool(metres[1].any())                                       # a feature image that does not exist: zeros
    assert bool((metres[0] == SENTINEL).all()) and bool((metres[2] == SENTINEL).all())     # planes that do not exist: nothing written anywhere


# ------------------------------------------------------------------------------------------------ 3. loader
@pytest.fixture(scope="module")
def loader_tree(tmp_path_factory):
    """2 pairs that share the keyframe; one query frame re-saved as a progressive JPEG, which the device decoder leaves to the host"""
    from PIL import Image
    root = tmp_path_factory.mktemp("loader_tree")
    tree = S.write_rig_tree(root, n_frames=6)
    p = os.path.join(tree["scene_root"], "seq1", "frame_00005.jpg")
    Image.open(p).convert("RGB").save(p, format="JPEG", quality=90, progressive=True)
    return root, tree


def _scenes(root, depth="dptkitti"):
    from mapfree_reloc_amd.config import get_cfg_defaults
    cfg = get_cfg_defaults()
    cfg.DATASET.DATA_ROOT, cfg.DATASET.HEIGHT, cfg.DATASET.WIDTH, cfg.DATASET.ESTIMATED_DEPTH = str(root), S.TREE_H, S.TREE_W, depth
    return list_scenes(cfg, "val")


@pytest.mark.parametrize("decode,jpeg", [("thread", "host"), ("process", "host"), ("thread", "device")])
def test_loader_carries_the_files_rgb_bytes(loader_tree, decode, jpeg):
    """(the process route's colour ring is also exercised without a device, tests/test_dpt_fused_host.py; here once, for the pinned ring and its H2D copy)"""
    root, tree = loader_tree
    scenes = _scenes(root)
    loader = PairBatchLoader(scenes, 2, prefetch=1, pin=True, workers=2, decode=decode, jpeg_decode=jpeg, rgb=True)
    try:
        batches = list(DevicePrefetcher(loader, DEV))
        torch.cuda.synchronize()
        assert len(batches) == 1
        b = batches[0]
        assert b["depth0"] is None and b["depth1"] is None and b["rgb"].dtype == torch.uint8 and b["rgb"].shape == (4, S.TREE_H, S.TREE_W, 3)
        assert b["rgb"].is_cuda and b["names"] == ["seq1/frame_00000.jpg", "seq1/frame_00005.jpg"]
        for p, name in enumerate(b["names"]):                               # rows 0 and 2: the duplicated reference view
            assert torch.equal(b["rgb"][2 * p].cpu(), _pil(tree["scene_root"], "seq0/frame_00000.jpg"))
            assert torch.equal(b["rgb"][2 * p + 1].cpu(), _pil(tree["scene_root"], name))
    finally:
        loader.close()
    plain = PairBatchLoader(scenes, 2, prefetch=0, pin=False, workers=2, decode="thread", jpeg_decode="host")
    try:
        ref = next(iter(plain))
        assert torch.equal(b["images"].cpu(), ref["images"])                # the gray planes are the ones the depth-file route carries
    finally:
        plain.close()


@pytest.mark.parametrize("decode,jpeg", [("thread", "host"), ("thread", "device")])
def test_loader_without_the_argument_is_unchanged(loader_tree, decode, jpeg):
    root, _ = loader_tree
    scenes = _scenes(root)
    out = []
    for kw in ({}, dict(rgb=False)):
        loader = PairBatchLoader(scenes, 2, prefetch=0, pin=True, workers=2, decode=decode, jpeg_decode=jpeg, **kw)
        try:
            out.append(list(DevicePrefetcher(loader, DEV)))
            torch.cuda.synchronize()
        finally:
            loader.close()
    for a, b in zip(*out):
        assert list(a) == list(b) and "rgb" not in a and a["depth0"] is not None
        for k in a:
            if isinstance(a[k], torch.Tensor):
                assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
            else:
                assert a[k] == b[k], k


# ------------------------------------------------------------------------------------------------ 4. pipeline against the per-pair plugin
def _same(u, v):
    return torch.equal(torch.isnan(u), torch.isnan(v)) and torch.equal(torch.nan_to_num(u), torch.nan_to_num(v))


def _run_fused(cfg, batch_pairs, pipe=None):
    """-> (pipeline, per pair (depth0, depth1 or None, R f32, t f32, n_inliers, status))"""
    pipe = pipe or FusedPosePipeline(cfg, DEV)
    loader = PairBatchLoader(list_scenes(cfg, "val"), batch_pairs, prefetch=1, pin=True, workers=2, decode="thread", rgb=submission.wants_rgb(cfg, pipe))
    rows = []
    try:
        for batch in DevicePrefetcher(loader, DEV):
            out = pipe(batch)
            for p in range(len(batch["names"])):
                d1 = out["depth1"][p].cpu() if "depth1" in out else None
                rows.append((out["depth0"][p].cpu() if "depth0" in out else None, d1, out["R"][p].to(torch.float32).cpu(), out["t"][p].to(torch.float32).cpu(),
                             int(out["n_inliers"][p]), int(out["status"][p])))
    finally:
        loader.close()
    return pipe, rows


@pytest.mark.parametrize("solver", ["PNP", "EssentialMatrixMetric", "Procrustes"])
def test_fused_pipeline_equals_the_per_pair_plugin(sd, tmp_path, solver):
    S.write_rig_tree(tmp_path / "tree", n_frames=11)                        # 3 pairs: a full batch of 2 and a ragged one
    cfg = _cfg(tmp_path / "tree", tmp_path, sd, solver)
    model, plug = build_model(cfg), []
    for data in make_loader(cfg, "val"):
        Rm, t = model(data)
        plug.append((data["depth0"][0].clone(), data["depth1"][0].clone(), Rm[0], t.reshape(3), int(data["inliers"])))
    _hide_depth_files(tmp_path / "tree")                                    # the fused route must not read them
    pipe, rows = _run_fused(cfg, 2)
    assert len(rows) == len(plug) == 3
    for (d0, d1, Rf, tf, nf, st), (pd0, pd1, Rp, tp, npl) in zip(rows, plug):
        print(f"[dpt fused] {solver}: status {st}, inliers {nf} / {npl}, t {tf.tolist()}")
        assert d0.shape == (S.TREE_H, S.TREE_W) and torch.equal(d0, pd0) and float(d0.std()) > 0
        if solver != "PNP":
            assert torch.equal(d1, pd1)
        else:
            assert d1 is None                                               # PnP reads depth0 only: the query views never went through the network
        assert _same(Rf, Rp) and _same(tf, tp) and nf == npl


# ------------------------------------------------------------------------------------------------ 5. only what is needed
@pytest.fixture()
def six_pairs(tmp_path):
    S.write_rig_tree(tmp_path / "tree", n_frames=26)                        # the keyframe against seq1 frames 0, 5, ..., 25
    _hide_depth_files(tmp_path / "tree")
    return tmp_path / "tree"


def test_network_runs_only_for_the_views_the_solver_reads(sd, six_pairs, tmp_path):
    pipe, rows = _run_fused(_cfg(six_pairs, tmp_path, sd, "PNP"), 2)
    assert len(rows) == 6 and pipe.stats["depth_views_run"] == 1 and pipe.stats["depth_views_reused"] == 2     # one hit per later batch
    assert all(torch.equal(r[0], rows[0][0]) for r in rows)
    pipe, _ = _run_fused(_cfg(six_pairs, tmp_path, sd, "EssentialMatrixMetric"), 2)
    assert pipe.stats["depth_views_run"] == 1 + 6 and pipe.stats["depth_views_reused"] == 2
    cfg = _cfg(six_pairs, tmp_path, sd, "PNP")
    cfg.HIP.REF_FEATURE_CACHE = False
    pipe, rows2 = _run_fused(cfg, 2)
    assert pipe.stats["depth_views_run"] == 3 and pipe.stats["depth_views_reused"] == 0
    assert all(torch.equal(a[0], b[0]) and _same(a[2], b[2]) for a, b in zip(rows, rows2))


def test_essential_matrix_builds_no_depth_stage(sd, six_pairs, tmp_path):
    cfg = _cfg(six_pairs, tmp_path, sd, "EssentialMatrix")
    cfg.DPT.WEIGHTS, cfg.DATASET.ESTIMATED_DEPTH = "", None                 # no DPT weights, and synthetic ones are not allowed: building DPT would raise
    assert not cfg.ALLOW_SYNTHETIC_WEIGHTS
    pipe, rows = _run_fused(cfg, 2)
    assert pipe.depth is None and not pipe.needs_rgb and len(rows) == 6 and rows[0][0] is None
    assert any(r[5] == 0 for r in rows)


def test_chunk_size_does_not_change_the_maps(sd, six_pairs, tmp_path):
    out = []
    for chunk in (3, 16):                                                   # 7 views per batch: chunks of 3 + 3 + 1 against one launch
        cfg = _cfg(six_pairs, tmp_path, sd, "EssentialMatrixMetric")
        cfg.DPT.FUSED_CHUNK = chunk
        out.append(_run_fused(cfg, 6)[1])
    for a, b in zip(*out):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and _same(a[2], b[2]) and _same(a[3], b[3]) and a[4:] == b[4:]


# ------------------------------------------------------------------------------------------------ 6. range guard
def _out_of_range_weights(sd):
    """test_gpu_dpt.test_range_guard_takes_the_bf16x3_rerun's: fc1 of one ViT layer times 2^20, fc2 times 2^-20 -- the hidden activations leave the f16x2 range"""
    sd = {k: v.clone() for k, v in sd.items()}
    p = "dpt.encoder.layer.1"
    sd[f"{p}.intermediate.dense.weight"] *= 2.0 ** 20; sd[f"{p}.intermediate.dense.bias"] *= 2.0 ** 20
    sd[f"{p}.output.dense.weight"] *= 2.0 ** -20
    return sd


def _members(z):
    with zipfile.ZipFile(z) as a:
        return {n: a.read(n) for n in a.namelist()}


def test_range_guard_marks_rows_and_the_second_pass_takes_the_twin(sd, six_pairs, tmp_path):
    (tmp_path / "w").mkdir()
    cfg = _cfg(six_pairs, tmp_path / "w", _out_of_range_weights(sd), "PNP")
    with options.override(SPLIT="f16x2"):
        pipe, rows = _run_fused(cfg, 2)
        assert pipe.guard.active and pipe.stats["depth_views_run"] == 1 and pipe.stats["depth_views_reused"] == 2
        assert [r[5] for r in rows] == [ST_RANGE] * 6                       # batches 2 and 3 only reuse the flagged map: marked all the same
        assert all(bool(torch.isnan(r[2]).all()) for r in rows)
        z = submission.predict_fused(cfg, "val", tmp_path / "guarded", pipeline=FusedPosePipeline(cfg, DEV), batch_pairs=2)
    with options.override(SPLIT="bf16x3"):
        exact = FusedPosePipeline(cfg, DEV)
        assert not exact.guard.active
        ze = submission.predict_fused(cfg, "val", tmp_path / "exact", pipeline=exact, batch_pairs=2)
    assert _members(z) == _members(ze) and list(_members(z)) == ["pose_s00000.txt"] and len(_members(z)["pose_s00000.txt"]) > 0
    with options.override(SPLIT="f16x2"):                                   # ... and the test's own weights do not fire it
        _, rows = _run_fused(_cfg(six_pairs, tmp_path, sd, "PNP"), 2)
        assert ST_RANGE not in [r[5] for r in rows]


# ------------------------------------------------------------------------------------------------ 7. predict_fused
def test_predict_fused_equals_the_per_pair_loop_and_the_file_route(sd, tmp_path):
    from mapfree_reloc_amd import compute_depth as CD
    S.write_rig_tree(tmp_path / "tree", n_frames=11)
    cfg = _cfg(tmp_path / "tree", tmp_path, sd, "PNP")
    res = submission.predict(make_loader(cfg, "val"), build_model(cfg))
    submission.save_submission(res, tmp_path / "loop.zip", deterministic=True)
    est = dpt.DepthEstimator(cfg)
    assert CD.run_scene(est, "Mapfree", CD.list_scene_dirs("Mapfree", tmp_path / "tree")[0], "dptsynth", batch=3) == (12, 0)
    _hide_depth_files(tmp_path / "tree")
    z = submission.predict_fused(cfg, "val", tmp_path / "online", batch_pairs=2)
    assert _members(z) == _members(tmp_path / "loop.zip") and list(_members(z)) == ["pose_s00000.txt"]
    assert len(_members(z)["pose_s00000.txt"].decode().split("\n")) >= 1 and len(_members(z)["pose_s00000.txt"]) > 0
    zf = submission.predict_fused(_cfg(tmp_path / "tree", tmp_path, sd, "PNP", source="file", name="dptsynth"), "val", tmp_path / "file", batch_pairs=2)
    assert _members(zf) == _members(z)
