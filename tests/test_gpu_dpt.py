"""-m gpu: DPT-Hybrid depth in HIP (nets/dpt.py, csrc/dpt.hip) against the `transformers` module (tests/dpt_ref.py), stage by stage and end to end.

The bar is the project's established one (tests/test_gpu_lightglue.py): a stage is fed the float32 oracle's INPUT tensors and compared with the float64
oracle's output; err(device) <= 10 x err(float32 oracle), max and rms (both relative to the float64 tensor's scale), printed before the assert.  For the
kernels that are driven directly (GroupNorm, LayerNorm at C = 768, the pixel shuffle) the two oracles are the same torch function in float32 and float64.
Weights: nets/weights.dpt_state_dict with every norm and bias perturbed (dpt_ref.perturbed); reduced architecture dpt_ref.REDUCED, and DPT-Hybrid itself
once at 128x160 (81 tokens, 12 heads)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dpt_ref as R  # noqa: E402

from mapfree_reloc_amd import options  # noqa: E402
from mapfree_reloc_amd.nets import dpt, weights as WT  # noqa: E402
from mapfree_reloc_amd.nets.linear import SplitLinear  # noqa: E402

pytestmark = pytest.mark.gpu
FACTOR = 10.0
DEV = "cuda"
SHAPES = [(64, 96), (96, 32)]
SPLITS = ["f16x2", "bf16x3"]


def _err(t, ref64):
    d = t.detach().double().cpu() - ref64
    return float(d.abs().max() / ref64.abs().max()), float(d.pow(2).mean().sqrt() / ref64.pow(2).mean().sqrt())


def _check(stage, got, f32, f64):
    assert got.shape == f64.shape, (stage, got.shape, f64.shape)
    eg, eo = _err(got, f64), _err(f32, f64)
    print(f"[dpt] {stage}: device max {eg[0]:.3e} rms {eg[1]:.3e} | f32 oracle max {eo[0]:.3e} rms {eo[1]:.3e} | ratio max {eg[0] / eo[0]:.2f} rms {eg[1] / eo[1]:.2f}")
    assert np.isfinite(eg[0]) and eo[0] > 0
    assert eg[0] <= FACTOR * eo[0] and eg[1] <= FACTOR * eo[1], (stage, eg, eo)


def _normalised(img):
    return (img - 0.5) / 0.5


class _Oracle:
    """both twins on one weight set, run once per shape; the captures are shared by the tests and never written to"""

    def __init__(self, arch, shapes, batch):
        self.arch = arch
        self.sd = R.perturbed(WT.dpt_state_dict(arch=arch))
        self.m32, self.m64 = R.make_models(self.sd, dpt.check_arch(arch))
        self.img, self.d32, self.d64, self.c32, self.c64 = {}, {}, {}, {}, {}
        for hw in shapes:
            self.img[hw] = R.make_images(batch, hw[0], hw[1], seed=hw[0])
            x = _normalised(self.img[hw])
            self.d32[hw], self.c32[hw] = R.run(self.m32, x)
            self.d64[hw], self.c64[hw] = R.run(self.m64, x)

    def io(self, hw, name):
        """(float32 inputs, float32 output, float64 output) of module `name`"""
        return self.c32[hw][name][0], self.c32[hw][name][1], self.c64[hw][name][1]


@pytest.fixture(scope="module")
def orc():
    return _Oracle(R.REDUCED, SHAPES, 2)


@pytest.fixture(scope="module")
def full():
    return _Oracle(None, [(128, 160)], 1)


_NETS = {}


def _net(o, split):
    key = (id(o), split)
    if key not in _NETS:
        with options.override(SPLIT=split):
            _NETS[key] = dpt.DPTHIP(o.sd, DEV, arch=o.arch)
    return _NETS[key]


def _d(t):
    return t.detach().float().contiguous().to(DEV)


BIT = "dpt.embeddings.backbone.bit"


# ------------------------------------------------------------------------------------------------ prep
@pytest.mark.parametrize("u8", [False, True])
def test_prep(u8):
    img = R.make_images(2, 50, 70, seed=3)
    if u8:
        raw = (img * 255).round().to(torch.uint8)
        got = dpt.prep(raw.permute(0, 2, 3, 1).contiguous().to(DEV), 64, 96)
        x32, x64 = raw.float() / 255, raw.double() / 255
    else:
        got = dpt.prep(img.to(DEV), 64, 96)
        x32, x64 = img, img.double()
    ref = lambda x: (F.interpolate(x, size=(64, 96), mode="bilinear", align_corners=False) - 0.5) / 0.5
    _check(f"prep u8={u8}", got, ref(x32), ref(x64))
    with pytest.raises(Exception):
        dpt.prep(img.to(DEV), 64, 100)                                   # not a multiple of 32: refused


# ------------------------------------------------------------------------------------------------ stem
@pytest.mark.parametrize("hw", SHAPES)
def test_stem_conv_and_pool_with_asymmetric_padding(orc, hw):
    net = _net(orc, "f16x2")
    (x,), f32, f64 = orc.io(hw, f"{BIT}.embedder.convolution")
    _check(f"stem conv {hw}", net.stem_conv(_d(x)), f32, f64)
    (x,), f32, f64 = orc.io(hw, f"{BIT}.embedder.pooler")
    got = dpt.maxpool3s2(_d(x))
    _check(f"stem pool {hw}", got, f32, f64)
    assert torch.equal(got.cpu(), f32)                                   # a selection: the same bits as the float32 oracle
    (x,), f32, f64 = orc.io(hw, f"{BIT}.embedder")
    _check(f"embedder {hw}", net.embed(_d(x)), f32, f64)


def test_pool_odd_sizes_and_explicit_padding():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, 7, 9, generator=g) - 0.5                       # mostly negative: the zero padding wins at the border
    ref = F.max_pool2d(F.pad(x, (1, 1, 1, 1)), 3, 2)                     # TF-"SAME" on odd sizes is (1, 1)
    assert torch.equal(dpt.maxpool3s2(x.to(DEV)).cpu(), ref)
    ref = F.max_pool2d(F.pad(x, (2, 0, 0, 1)), 3, 2)
    assert torch.equal(dpt.maxpool3s2(x.to(DEV), pad_h=(0, 1), pad_w=(2, 0)).cpu(), ref)
    with pytest.raises(Exception):
        dpt.maxpool3s2(x.to(DEV), pad_h=(3, 0))


# ------------------------------------------------------------------------------------------------ GroupNorm
@pytest.mark.parametrize("groups", [8, 32])
@pytest.mark.parametrize("plane", [(16, 24), (3, 5)])
@pytest.mark.parametrize("tail", [False, True])
def test_groupnorm(groups, plane, tail):
    g = torch.Generator().manual_seed(groups + plane[0])
    x = torch.randn(2, 64, *plane, generator=g) * 3 + 1
    gamma, beta = 0.5 + torch.rand(64, generator=g), torch.randn(64, generator=g)
    res = torch.randn(2, 64, *plane, generator=g) if tail else None

    def ref(dt):
        y = F.group_norm(x.to(dt), groups, gamma.to(dt), beta.to(dt), 1e-5)
        return F.relu(y + res.to(dt)) if tail else y
    got = dpt.groupnorm(x.to(DEV), gamma.to(DEV), beta.to(DEV), groups, relu=tail, residual=None if res is None else res.to(DEV))
    _check(f"groupnorm G={groups} plane={plane} tail={tail}", got, ref(torch.float32), ref(torch.float64))
    if not tail:                                                         # ... and the ReLU alone
        got = dpt.groupnorm(x.to(DEV), gamma.to(DEV), beta.to(DEV), groups, relu=True)
        _check(f"groupnorm+relu G={groups} plane={plane}", got, F.relu(ref(torch.float32)), F.relu(ref(torch.float64)))


# ------------------------------------------------------------------------------------------------ bottlenecks
@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("where", [(0, 0), (1, 0), (2, 1)], ids=["downsample", "stride2", "plain"])
def test_bottleneck(orc, where, split):
    """conv2 of a stride-1 bottleneck is the direct kernel under f16x2 and a Winograd kernel under bf16x3 (16 and 64 channels here); stride 2: implicit GEMM"""
    net, hw = _net(orc, split), SHAPES[0]
    s, l = where
    (x,), f32, f64 = orc.io(hw, f"{BIT}.encoder.stages.{s}.layers.{l}")
    _check(f"bottleneck {where} {split}", net.bottleneck(net.stages[s][l], _d(x)), f32, f64)


# ------------------------------------------------------------------------------------------------ tokens
@pytest.mark.parametrize("hw", SHAPES)
def test_token_assembly(orc, hw):
    net = _net(orc, "f16x2")
    (x,), _, _ = orc.io(hw, "dpt.embeddings.projection")
    f32, f64 = orc.c32[hw]["dpt.embeddings"][1].last_hidden_states, orc.c64[hw]["dpt.embeddings"][1].last_hidden_states
    assert f64.shape == (2, 1 + (hw[0] // 16) * (hw[1] // 16), 192)
    _check(f"tokens {hw}", net.tokenize(_d(x)), f32, f64)


def test_tokens_inverse_round_trip():
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 70, 5, 13, generator=g)                           # C and HW beyond one 64 x 64 tile, neither a multiple of it
    pos = torch.zeros(1 + 65, 70)
    rows = dpt.tokens(x.to(DEV), torch.ones(70, device=DEV), pos.to(DEV))
    assert torch.equal(rows[:, 0].cpu(), torch.ones(2, 70)) and torch.equal(rows[:, 1:].cpu(), x.flatten(2).transpose(1, 2))
    assert torch.equal(dpt.tokens_inverse(rows, 5, 13).cpu(), x)


# ------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("hw", SHAPES)
def test_layernorm_192(orc, hw):
    net = _net(orc, "f16x2")
    (x,), f32, f64 = orc.io(hw, "dpt.encoder.layer.0.layernorm_before")
    rows = x[0]                                                          # 25 / 13 rows
    _check(f"layernorm C=192 rows={rows.shape[0]}", dpt.layernorm(_d(rows), *net.layers[0]["ln1"]), f32[0], f64[0])


@pytest.mark.parametrize("rows", [25, 13])
def test_layernorm_768_strided_with_residual(rows):
    g = torch.Generator().manual_seed(rows)
    wide = torch.randn(rows, 1024, generator=g) * 2 + 0.5
    x, res = wide[:, 128:896], torch.randn(rows, 768, generator=g)
    gamma, beta = 0.5 + torch.rand(768, generator=g), torch.randn(768, generator=g)
    ref = lambda dt: res.to(dt) + F.layer_norm(x.to(dt), (768,), gamma.to(dt), beta.to(dt), 1e-12)
    wd = wide.to(DEV)
    out = torch.zeros(rows, 800, device=DEV)
    dpt.layernorm(wd[:, 128:896], gamma.to(DEV), beta.to(DEV), residual=res.to(DEV), out=out[:, :768])
    _check(f"layernorm C=768 rows={rows}", out[:, :768], ref(torch.float32), ref(torch.float64))
    assert not bool(out[:, 768:].any())                                  # nothing written beyond the row


# ------------------------------------------------------------------------------------------------ ViT layer
@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("hw", SHAPES)
def test_vit_layer(orc, hw, split):
    net = _net(orc, split)
    (x,), f32, f64 = orc.io(hw, "dpt.encoder.layer.1")
    B, T, h = x.shape
    got = net.vit_layer(net.layers[1], _d(x).reshape(B * T, h).clone(), B, T).view(B, T, h)
    _check(f"vit layer N={T} {split}", got, f32, f64)


@pytest.mark.parametrize("split", SPLITS)
def test_vit_layer_full_width(full, split):
    net, hw = _net(full, split), (128, 160)
    (x,), f32, f64 = full.io(hw, "dpt.encoder.layer.3")
    B, T, h = x.shape
    assert (T, h) == (81, 768)
    got = net.vit_layer(net.layers[3], _d(x).reshape(B * T, h).clone(), B, T).view(B, T, h)
    _check(f"vit layer N=81 12 heads {split}", got, f32, f64)


# ------------------------------------------------------------------------------------------------ readout, reassemble, shuffle
@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("i", [2, 3])
def test_readout_and_reassemble(orc, i, split):
    net, hw = _net(orc, split), SHAPES[0]
    hidden = orc.c32[hw]["__taps__"][0][i]
    f32, f64 = orc.c32[hw][f"neck.reassemble_stage.layers.{i}"][1], orc.c64[hw][f"neck.reassemble_stage.layers.{i}"][1]
    _check(f"reassemble tap {i} {split}", net.reassemble(i, _d(hidden), hw[0] // 16, hw[1] // 16), f32, f64)


@pytest.mark.parametrize("s", [4, 2])
def test_transposed_conv_as_gemm_and_shuffle(s):
    g = torch.Generator().manual_seed(s)
    B, ci, co, H, W = 2, 32, 8, 2, 3
    x, w, b = torch.randn(B, ci, H, W, generator=g), torch.randn(ci, co, s, s, generator=g) * 0.2, torch.randn(co, generator=g)
    ref = lambda dt: F.conv_transpose2d(x.to(dt), w.to(dt), b.to(dt), stride=s)
    lin = SplitLinear(dpt.fold_conv_transpose(w).float().to(DEV), None)
    rows = x.permute(0, 2, 3, 1).reshape(B * H * W, ci).contiguous().to(DEV)
    got = dpt.shuffle(lin(rows), b.to(DEV), B, co, H, W, s)
    _check(f"shuffle x{s}", got, ref(torch.float32), ref(torch.float64))


# ------------------------------------------------------------------------------------------------ fusion
@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("i", [0, 1], ids=["no_residual", "residual"])
def test_fusion_layer(orc, i, split):
    net, hw = _net(orc, split), SHAPES[0]
    inp, f32, f64 = orc.io(hw, f"neck.fusion_stage.layers.{i}")
    assert len(inp) == 1 + i
    _check(f"fusion layer {i} {split}", net.fusion_layer(net.fusion[i], *[_d(t) for t in inp]), f32, f64)


# ------------------------------------------------------------------------------------------------ head tail
@pytest.mark.parametrize("invert", [False, True])
def test_head_tail(orc, invert):
    net, hw = _net(orc, "f16x2"), SHAPES[0]
    f_32, f_64 = orc.c32[hw]["head.head.3"][1], orc.c64[hw]["head.head.3"][1]
    out_hw, scale, shift = (50, 70), 0.1, 0.05

    def ref(m, f):
        p = m.head.head[5](m.head.head[4](f))
        if invert:
            p = 1.0 / (scale * p + shift).clamp_min(1e-8)
        return F.interpolate(p, size=out_hw, mode="bilinear", align_corners=False)[:, 0]
    with torch.no_grad():
        r32, r64 = ref(orc.m32, f_32), ref(orc.m64, f_64)
    metres, mm = dpt.head_tail(_d(f_32), net.head4_w, net.head4_b, *out_hw, invert=invert, scale=scale, shift=shift, millimetres=True)
    _check(f"head tail invert={invert}", metres, r32, r64)
    want = np.clip(np.rint(1000.0 * metres.cpu().numpy().astype(np.float64)), 0, 65535).astype(np.uint16)
    assert mm.dtype == torch.uint16 and np.array_equal(mm.cpu().numpy(), want)
    assert want.min() > 0 and want.max() < 65535                         # the planes are inside the format's range: the comparison is not a clamp's
    m2, none = dpt.head_tail(_d(f_32), net.head4_w, net.head4_b, *out_hw, invert=invert, scale=scale, shift=shift)
    assert none is None and torch.equal(m2, metres)


def test_head_tail_clamps_millimetres():
    f = torch.ones(1, 32, 4, 4, device=DEV)
    w = torch.full((32,), 1.0, device=DEV)
    metres, mm = dpt.head_tail(f, w, 68.0, 4, 4, millimetres=True)        # 100 m
    assert float(metres.min()) == 100.0 and int(mm.cpu().numpy().min()) == 65535
    metres, mm = dpt.head_tail(f, w, -40.0, 4, 4, millimetres=True)       # the ReLU's zero
    assert float(metres.max()) == 0.0 and int(mm.cpu().numpy().max()) == 0


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("hw", SHAPES)
def test_end_to_end_reduced(orc, hw, split):
    net = _net(orc, split)
    metres, _ = net(orc.img[hw].to(DEV), hw)
    assert float((orc.d64[hw] == 0).double().mean()) <= 0.01
    _check(f"end to end reduced {hw} {split}", metres, orc.d32[hw], orc.d64[hw])


@pytest.mark.parametrize("split", SPLITS)
def test_end_to_end_full_configuration(full, split):
    hw = (128, 160)
    net = _net(full, split)
    metres, _ = net(full.img[hw].to(DEV), hw)
    assert float((full.d64[hw] == 0).double().mean()) <= 0.01
    _check(f"end to end DPT-Hybrid {hw} {split}", metres, full.d32[hw], full.d64[hw])


# ------------------------------------------------------------------------------------------------ the config's stage: routes, range guard
def _stage_cfg(root, tmp_path, sd, source, name):
    import rig_scenes as S
    from mapfree_reloc_amd.config import get_cfg_defaults
    cfg = get_cfg_defaults()
    cfg.MODEL, cfg.FEATURE_MATCHING, cfg.POSE_SOLVER = "FeatureMatching", "Precomputed", "PNP"
    cfg.MATCHES_FILE_PATH = "{scene_root}/correspondences_exact.npz"
    cfg.PNP.RANSAC_ITER, cfg.PNP.REPROJECTION_INLIER_THRESHOLD, cfg.PNP.CONFIDENCE = 1000, 3, 0.9999
    cfg.DATASET.DATA_ROOT, cfg.DATASET.HEIGHT, cfg.DATASET.WIDTH, cfg.DATASET.ESTIMATED_DEPTH = str(root), S.TREE_H, S.TREE_W, name
    wpath = tmp_path / "dpt_weights.pth"
    if not wpath.exists():
        torch.save(sd, wpath)
    cfg.DPT.WEIGHTS, cfg.DPT.NET_HEIGHT, cfg.DPT.NET_WIDTH, cfg.DPT.INVERT, cfg.DPT.SOURCE = str(wpath), 64, 96, False, source
    for k, v in R.REDUCED.items():
        cfg.DPT.ARCH[k] = list(v) if isinstance(v, tuple) else v
    return cfg


def test_file_route_and_online_route_agree(orc, tmp_path):
    """(a) compute_depth writes the PNGs and the ordinary file route solves; (b) DPT.SOURCE 'online': the same depth bits reach the solver, and the same pose
    comes out.  The tree's own plane-depth PNGs (.dptkitti.png) stay where they are: the online route must not read them"""
    import rig_scenes as S
    from mapfree_reloc_amd import compute_depth as CD
    from mapfree_reloc_amd.builder import build_model
    from mapfree_reloc_amd.datasets import clear_frame_cache, make_loader
    tree = S.write_rig_tree(tmp_path / "tree", n_frames=6)                    # 7 frames; pairs: the keyframe against seq1 frames 0 and 5
    cfg_a = _stage_cfg(tmp_path / "tree", tmp_path, orc.sd, "file", "dptsynth")
    est = dpt.DepthEstimator(cfg_a)
    scene = CD.list_scene_dirs("Mapfree", tmp_path / "tree")[0]
    assert CD.run_scene(est, "Mapfree", scene, "dptsynth", batch=3) == (7, 0)
    assert CD.run_scene(est, "Mapfree", scene, "dptsynth", batch=3) == (0, 7)                 # files that exist are skipped
    assert os.path.exists(os.path.join(tree["scene_root"], "seq1", "frame_00005.dptsynth.png"))
    clear_frame_cache()

    def solve(cfg):
        model, out = build_model(cfg), []
        for data in make_loader(cfg, "val"):
            Rm, t = model(data)
            out.append((data["depth0"].clone(), data["depth1"].clone(), Rm, t, data["inliers"]))
        return out
    a = solve(cfg_a)
    b = solve(_stage_cfg(tmp_path / "tree", tmp_path, orc.sd, "online", "dptkitti"))
    assert len(a) == len(b) == 2
    for (d0a, d1a, Ra, ta, ia), (d0b, d1b, Rb, tb, ib) in zip(a, b):
        assert d0a.shape == (1, S.TREE_H, S.TREE_W) and torch.equal(d0a, d0b) and torch.equal(d1a, d1b)
        assert 0.2 < float(d0a.min()) and float(d0a.max()) < 20.0 and float(d0a.std()) > 0    # a network's map, not the tree's plane
        print(f"[dpt] routes: inliers {ia} / {ib}, t {ta.flatten().tolist()}")
        same = lambda u, v: torch.equal(torch.isnan(u), torch.isnan(v)) and torch.equal(torch.nan_to_num(u), torch.nan_to_num(v))
        assert same(Ra, Rb) and same(ta, tb) and ia == ib                # bit for bit (a pair the solver gives up on is NaN on both routes)


def test_range_guard_takes_the_bf16x3_rerun(orc, tmp_path):
    """fc1 of one ViT layer scaled by 2^20 and fc2 by 2^-20: the same function in exact arithmetic, but the hidden activations (~3e5) leave the f16x2 range.
    The guard fires, the batch runs again through the bf16x3 twin, and the result meets the bar against the float64 oracle on the SAME weights"""
    import rig_scenes as S
    sd = {k: v.clone() for k, v in orc.sd.items()}
    p = "dpt.encoder.layer.1"
    sd[f"{p}.intermediate.dense.weight"] *= 2.0 ** 20; sd[f"{p}.intermediate.dense.bias"] *= 2.0 ** 20
    sd[f"{p}.output.dense.weight"] *= 2.0 ** -20
    hw = SHAPES[0]
    m32, m64 = R.make_models(sd, dpt.check_arch(R.REDUCED))
    x = _normalised(orc.img[hw])
    d32, d64 = R.run(m32, x, capture=False)[0], R.run(m64, x, capture=False)[0]
    (tmp_path / "w").mkdir()
    with options.override(SPLIT="f16x2"):
        est = dpt.DepthEstimator(_stage_cfg(tmp_path, tmp_path / "w", sd, "file", "unused"))
        assert est.guard.active and est.guard.reruns == 0
        metres, mm = est(orc.img[hw])
        assert est.guard.reruns == 1
    _check("range guard: bf16x3 re-run", metres, d32, d64)
    with options.override(SPLIT="f16x2"):                                # ... and the test's own weights do not fire it
        est = dpt.DepthEstimator(_stage_cfg(tmp_path, tmp_path, orc.sd, "file", "unused"))
        est(orc.img[hw])
        assert est.guard.reruns == 0


def test_scannet_route_writes_what_the_reader_loads(orc, tmp_path):
    """compute_depth -ds Scannet on the reader tests' tree: the .npz holds the estimator's metres at WIDTH x HEIGHT, and ScanNetScene hands them out"""
    import scannet_tree as ST
    from mapfree_reloc_amd import compute_depth as CD
    from mapfree_reloc_amd.scannet import ScanNetScene
    from PIL import Image
    p = ST.default_params()
    tr = ST.write_tree(tmp_path / "scannet", p)
    W, H = 24, 16
    est = dpt.DepthEstimator(_stage_cfg(tmp_path, tmp_path, orc.sd, "file", "unused"))
    out = str(tmp_path / "dpt_scannet.npz")
    assert CD.run_scannet(est, tr["scans"], tr["test_npz"], out, (W, H), batch=3) == (5, 0)
    sc = ScanNetScene(tr["scans"], tr["test_npz"], mode="test", resize=(W, H), estimated_depth=out)
    a = np.array(Image.open(os.path.join(tr["scans"], "scene0711_01", "sensor_data", "frame-000300.color.jpg")).convert("RGB"))
    metres, mm = est(torch.from_numpy(a[None]), (H, W))
    got = sc._depth("scene0711_01", 300, out=np.empty((H, W), np.float32))
    assert np.array_equal(got, dpt.millimetres_to_metres(mm)[0].cpu().numpy()) and 0.2 < got.min() and got.max() < 20.0 and got.std() > 0
    assert float((torch.from_numpy(got) - metres[0].cpu()).abs().max()) <= 0.0005 + 1e-6      # the millimetre rounding, no more
