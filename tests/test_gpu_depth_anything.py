"""-m gpu: Depth Anything V2 depth in HIP (nets/depth_anything.py, csrc/depth_anything.hip) against the `transformers` module (tests/depth_anything_ref.py),
stage by stage and end to end.

The bar is the project's established one (tests/test_gpu_dpt.py): a stage is fed the float32 oracle's INPUT tensors and compared with the float64 oracle's
output; err(device) <= 10 x err(float32 oracle), max and rms (both relative to the float64 tensor's scale), printed before the assert.  Kernels that only
select or move values (patch rows of an image already at network size, the pixel shuffle, the cls drop) are compared bit for bit with float32 torch.
Weights: nets/weights.depth_anything_state_dict with every norm, bias and LayerScale perturbed (depth_anything_ref.perturbed); reduced architecture
depth_anything_ref.REDUCED at batch 2 and the three shapes of depth_anything_ref.SHAPES, and ViT-S itself once at 70 x 98."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_anything_ref as R  # noqa: E402

from mapfree_reloc_amd import options  # noqa: E402
from mapfree_reloc_amd.nets import depth_anything as DA, dpt, weights as WT  # noqa: E402

pytestmark = pytest.mark.gpu
FACTOR = 10.0
DEV = "cuda"
SHAPES = R.SHAPES
SPLITS = ["f16x2", "bf16x3"]
MAX_DEPTH = R.REDUCED["MAX_DEPTH"]


def _err(t, ref64):
    d = t.detach().double().cpu() - ref64
    return float(d.abs().max() / ref64.abs().max()), float(d.pow(2).mean().sqrt() / ref64.pow(2).mean().sqrt())


def _check(stage, got, f32, f64):
    assert got.shape == f64.shape, (stage, got.shape, f64.shape)
    eg, eo = _err(got, f64), _err(f32, f64)
    print(f"[depth anything] {stage}: device max {eg[0]:.3e} rms {eg[1]:.3e} | f32 oracle max {eo[0]:.3e} rms {eo[1]:.3e} | ratio max {eg[0] / eo[0]:.2f} rms {eg[1] / eo[1]:.2f}")
    assert np.isfinite(eg[0]) and eo[0] > 0
    assert eg[0] <= FACTOR * eo[0] and eg[1] <= FACTOR * eo[1], (stage, eg, eo)


def _t(out):
    return out[0] if isinstance(out, tuple) else out


class _Oracle:
    """both twins on one weight set, run once per shape; the captures are shared by the tests and never written to"""

    def __init__(self, arch, shapes, batch):
        self.arch = arch
        self.sd = R.perturbed(WT.depth_anything_state_dict(arch=arch))
        self.m32, self.m64 = R.make_models(self.sd, DA.check_arch(arch))
        self.img, self.d32, self.d64, self.c32, self.c64 = {}, {}, {}, {}, {}
        for hw in shapes:
            self.img[hw] = R.make_images(batch, hw[0], hw[1], seed=hw[0])
            self.d32[hw], self.c32[hw] = R.run(self.m32, R.normalise(self.img[hw]))
            self.d64[hw], self.c64[hw] = R.run(self.m64, R.normalise(self.img[hw].double()))

    def io(self, hw, name):
        """(float32 inputs, float32 output, float64 output) of module `name`"""
        return self.c32[hw][name][0], _t(self.c32[hw][name][1]), _t(self.c64[hw][name][1])


@pytest.fixture(scope="module")
def orc():
    return _Oracle(R.REDUCED, SHAPES, 2)


@pytest.fixture(scope="module")
def vits():
    return _Oracle(None, [(70, 98)], 1)


_NETS = {}


def _net(o, split):
    key = (id(o), split)
    if key not in _NETS:
        with options.override(SPLIT=split):
            _NETS[key] = DA.DepthAnythingHIP(o.sd, DEV, arch=o.arch)
    return _NETS[key]


def _d(t):
    return t.detach().float().contiguous().to(DEV)


def _unfold(x):
    """normalised image [B, 3, 14 gh, 14 gw] -> patch rows [B, gh, gw, 588], column (c 14 + i) 14 + j: a pure rearrangement"""
    B, _, H, W = x.shape
    gh, gw = H // 14, W // 14
    return x.reshape(B, 3, gh, 14, gw, 14).permute(0, 2, 4, 1, 3, 5).reshape(B, gh, gw, 588)


def _status():
    return torch.zeros(1, dtype=torch.int32, device=DEV)


# ------------------------------------------------------------------------------------------------ patch rows
@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("hw", [(70, 98), (28, 126)])          # 7 and 9 patches per band: one partial workgroup, and a full one plus one patch
def test_patch_rows_at_network_size_are_the_unfold_bit_for_bit(u8, hw):
    img = R.make_images(2, hw[0], hw[1], seed=1)
    if u8:
        raw = (img * 255).round().to(torch.uint8)
        got = DA.patch_rows(raw.permute(0, 2, 3, 1).contiguous().to(DEV), *hw)
        x = raw.float() / 255
    else:
        got, x = DA.patch_rows(img.to(DEV), *hw), img
    assert got.shape == (2, hw[0] // 14, hw[1] // 14, DA.PATCH_LDK)
    assert torch.equal(got[..., :588].cpu(), _unfold(R.normalise(x)))         # float32 (x - mean) / std: the same bits
    assert not bool(got[..., 588:].any())                                    # the K padding is zeros
    with pytest.raises(Exception):
        DA.patch_rows(img.to(DEV), 70, 100)                                  # not a multiple of 14: refused


@pytest.mark.parametrize("u8", [False, True])
def test_patch_rows_resized(u8):
    img = R.make_images(2, 75, 101, seed=3)
    if u8:
        raw = (img * 255).round().to(torch.uint8)
        got = DA.patch_rows(raw.permute(0, 2, 3, 1).contiguous().to(DEV), 70, 98)
        x32, x64 = raw.float() / 255, raw.double() / 255
    else:
        got = DA.patch_rows(img.to(DEV), 70, 98)
        x32, x64 = img, img.double()
    ref = lambda x: _unfold(R.normalise(F.interpolate(x, size=(70, 98), mode="bilinear", align_corners=False)))
    _check(f"patch rows 75x101 -> 70x98 u8={u8}", got[..., :588], ref(x32), ref(x64))
    assert not bool(got[..., 588:].any())


def test_patch_rows_tab_equals_the_plain_entry_and_checks_its_table():
    """the three images lie between sentinel-filled neighbours: an index one past either end would read the sentinel, whose rows are not zero"""
    H, W, hw = 75, 101, (70, 98)
    g = torch.Generator().manual_seed(1)
    big = torch.full((5, H, W, 3), 200, dtype=torch.uint8, device=DEV)
    big[1:4] = torch.randint(0, 256, (3, H, W, 3), generator=g, dtype=torch.uint8).to(DEV)
    img = big[1:4]
    assert img.is_contiguous()
    st = _status()
    got = DA.patch_rows_tab(img, torch.tensor([2, 0, 2], dtype=torch.int32, device=DEV), *hw, st)
    assert int(st) == 0 and torch.equal(got, DA.patch_rows(img[[2, 0, 2]].contiguous(), *hw))
    got = DA.patch_rows_tab(img, torch.tensor([2, 3, -1, 1 << 30], dtype=torch.int32, device=DEV), *hw, st)
    assert int(st) == 1
    assert torch.equal(got[0], DA.patch_rows(img[2:3].contiguous(), *hw)[0])
    assert not bool(got[1:].any())                                           # zeros: unlike the rows of every source, the sentinel images included
    assert bool(DA.patch_rows(big[:1].contiguous(), *hw)[..., :588].abs().min() > 0)


# ------------------------------------------------------------------------------------------------ embedding product and token assembly
@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("hw", SHAPES)
def test_embedding_and_token_assembly(orc, hw, split):
    """the oracle's backbone.embeddings from the rows of its own input image: the K = 588 product, the cls row, the bicubic position resize 5x5 -> this grid"""
    net = _net(orc, split)
    (x,), f32, f64 = orc.io(hw, "backbone.embeddings")
    rows = torch.zeros(2, hw[0] // 14, hw[1] // 14, DA.PATCH_LDK)
    rows[..., :588] = _unfold(x)
    assert f64.shape == (2, 1 + (hw[0] // 14) * (hw[1] // 14), 192)
    _check(f"embeddings {hw} {split}", net.tokenize(rows.to(DEV)), f32, f64)


# ------------------------------------------------------------------------------------------------ ViT layer
@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("hw", SHAPES)
def test_vit_layer(orc, hw, split):
    net = _net(orc, split)
    (x,), f32, f64 = orc.io(hw, "backbone.encoder.layer.1")
    B, T, h = x.shape
    got = net.vit_layer(net.layers[1], _d(x).reshape(B * T, h).clone(), B, T).view(B, T, h)
    _check(f"vit layer N={T} {split}", got, f32, f64)


def _single_layer(width, heads, mlp_ratio, seed):
    """one Dinov2 layer of the module's own class on seeded, perturbed weights -> (state dict under `backbone.encoder.layer.0`, float32 twin, float64 twin)"""
    from transformers import Dinov2Config
    from transformers.models.dinov2.modeling_dinov2 import Dinov2Layer
    g = torch.Generator().manual_seed(seed)
    cfg = Dinov2Config(hidden_size=width, num_attention_heads=heads, mlp_ratio=mlp_ratio, layer_norm_eps=1e-6, attn_implementation="eager")
    layer = Dinov2Layer(cfg).eval()
    sd = {}
    for k, v in layer.state_dict().items():
        if k.endswith("lambda1"):
            sd[k] = 0.5 + torch.rand(v.shape, generator=g)
        elif "norm" in k:
            sd[k] = (0.7 + 0.6 * torch.rand(v.shape, generator=g)) if k.endswith("weight") else 0.3 * torch.randn(v.shape, generator=g)
        else:
            sd[k] = torch.randn(v.shape, generator=g) * (0.02 if k.endswith("weight") else 0.05)
    layer.load_state_dict(sd, strict=True)
    import copy
    return {f"backbone.encoder.layer.0.{k}": v for k, v in sd.items()}, layer, copy.deepcopy(layer).double()


def _run_single(split, width, heads, mlp_ratio, B, T, seed):
    sd, l32, l64 = _single_layer(width, heads, mlp_ratio, seed)
    x = torch.randn(B, T, width, generator=torch.Generator().manual_seed(seed + 1))
    with torch.no_grad():
        f32, f64 = _t(l32(x)), _t(l64(x.double()))
    with options.override(SPLIT=split):
        enc = DA.ViTLayers(width, heads, DEV)
        L = DA.layer_weights(sd, "backbone.encoder.layer.0", enc.device)
    got = enc.vit_layer(L, _d(x).reshape(B * T, width).clone(), B, T).view(B, T, width)
    _check(f"vit layer width {width} heads {heads} N={T} {split}", got, f32, f64)


@pytest.mark.parametrize("split", SPLITS)
def test_vit_layer_width_1024(split):
    """ViT-L's width: 16 heads, LayerNorm with 16 values per lane, 36 tokens"""
    _run_single(split, 1024, 16, 4, 1, 36, seed=11)


@pytest.mark.parametrize("split", SPLITS)
def test_vit_layer_at_the_production_token_count(split):
    """1814 tokens (518 x 686): no multiple of the attention kernel's 32-key tile, and more than any count DPT-Hybrid runs"""
    _run_single(split, 192, 3, 2, 1, 1814, seed=12)


# ------------------------------------------------------------------------------------------------ tap, reassemble
@pytest.mark.parametrize("hw", SHAPES)
def test_tap_is_the_final_layernorm_without_the_cls_row(orc, hw):
    net = _net(orc, "f16x2")
    gh, gw = hw[0] // 14, hw[1] // 14
    for i in (0, 3):
        state = _t(orc.c32[hw][f"backbone.encoder.layer.{i}"][1])
        (x,), _, _ = orc.io(hw, f"neck.reassemble_stage.layers.{i}")
        (x64,) = orc.c64[hw][f"neck.reassemble_stage.layers.{i}"][0]
        _check(f"tap {i} {hw}", net.tap_map(_d(state), gh, gw), x, x64)
    rows = _d(state)
    assert torch.equal(dpt.tokens_inverse(rows, gh, gw, skip=1).cpu(), state[:, 1:].transpose(1, 2).reshape(2, 192, gh, gw))     # the cls drop alone: a move


def _as_rows(x):
    """NCHW map -> token rows with a cls row in front (which the reassemble stage must not read: NaN)"""
    B, C = x.shape[:2]
    return torch.cat([torch.full((B, 1, C), float("nan")), x.flatten(2).transpose(1, 2)], 1)


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("hw", SHAPES[:2])
@pytest.mark.parametrize("i", [0, 1, 2, 3])
def test_reassemble(orc, i, hw, split):
    """x4 and x2: ConvTranspose2d(k = s) as GEMM + mfr_dpt_shuffle on a network's data, 48 and 96 channels (K padded to 64 / 96); identity; 3x3 / stride 2 on an odd grid"""
    net = _net(orc, split)
    (x,), f32, f64 = orc.io(hw, f"neck.reassemble_stage.layers.{i}")
    got = net.reassemble(i, _d(_as_rows(x)), hw[0] // 14, hw[1] // 14)
    _check(f"reassemble {i} {hw} {split}", got, f32, f64)


@pytest.mark.parametrize("s", [4, 2])
@pytest.mark.parametrize("grid", [(5, 7), (7, 3)])
def test_shuffle_per_image_behind_the_cls_row_moves_bits(s, grid):
    """the calling pattern of DepthAnythingHIP.reassemble, without a product in front of it: the GEMM's output holds a cls row per image, and mfr_dpt_shuffle
    runs once per image on the rows behind it, into that image's slice of the output.  Seeded rows (the cls rows NaN: never read) and a bias; the result is
    the float32 view / permute + bias, bit for bit: a move and one float32 add.  C = 48 (ViT-S' first reassemble width), odd grids"""
    B, C, (gh, gw) = 2, 48, grid
    g = torch.Generator().manual_seed(10 * s + gh)
    rows = torch.randn(B, 1 + gh * gw, C * s * s, generator=g)
    rows[:, 0] = float("nan")
    bias = torch.randn(C, generator=g)
    want = rows[:, 1:].reshape(B, gh, gw, C, s, s).permute(0, 3, 1, 4, 2, 5).reshape(B, C, gh * s, gw * s) + bias.view(1, C, 1, 1)
    gd, bd = rows.to(DEV), bias.to(DEV)
    out = torch.full((B + 1, C, gh * s, gw * s), -7.0, device=DEV)           # a sentinel image behind the last: nothing is written beyond an image's slice
    for b in range(B):
        dpt.shuffle(gd[b, 1:], bd, 1, C, gh, gw, s, out=out[b:b + 1])
    assert torch.equal(out[:B].cpu(), want) and bool((out[B] == -7.0).all())
    assert torch.equal(dpt.shuffle(gd[:, 1:].reshape(B * gh * gw, C * s * s).contiguous(), bd, B, C, gh, gw, s).cpu(), want)      # ... and the batched call on compact rows


# ------------------------------------------------------------------------------------------------ neck convolutions, fusion
@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("i", [0, 1, 2, 3])
def test_neck_convolutions(orc, i, split):
    """48 and 96 input channels (no multiple of the kernels' channel step of 16 x 2), and the 3 x 4 map"""
    net, hw = _net(orc, split), SHAPES[0]
    (x,), f32, f64 = orc.io(hw, f"neck.convs.{i}")
    _check(f"neck conv {i} {split}", net.neck_convs[i](_d(x)), f32, f64)


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("hw", [SHAPES[0], SHAPES[2]], ids=["odd_grid", "even_grid"])
@pytest.mark.parametrize("i", [0, 1, 2, 3])
def test_fusion_layer(orc, i, hw, split):
    """layer 0 has no residual; on the odd grid layers 0 and 1 up-sample 3x4 -> 5x7 -> 10x14 (not x2), layer 2 takes the 10x14 map; layer 3 always x2"""
    net = _net(orc, split)
    inp, f32, f64 = orc.io(hw, f"neck.fusion_stage.layers.{i}")
    assert len(inp) == (1 if i == 0 else 2)
    size = None if i == 3 else tuple(f64.shape[2:])
    if hw == SHAPES[0] and i == 0:
        assert tuple(inp[0].shape[2:]) == (3, 4) and size == (5, 7)
    _check(f"fusion layer {i} {hw} {split}", net.fusion_layer(net.fusion[i], *[_d(t) for t in inp], size=size), f32, f64)


# ------------------------------------------------------------------------------------------------ head, tail
@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("hw", SHAPES)
def test_head(orc, hw, split):
    net = _net(orc, split)
    gh, gw = hw[0] // 14, hw[1] // 14
    fused = orc.c32[hw]["head"][0][0][-1]
    f = net.head_features(_d(fused), gh, gw)
    _check(f"head features {hw} {split}", f, _t(orc.c32[hw]["head.activation1"][1]), _t(orc.c64[hw]["head.activation1"][1]))
    metres, _ = net.tail(f, hw)                                              # at the network's size the resize is the identity
    _check(f"head {hw} {split}", metres, orc.d32[hw], orc.d64[hw])


@pytest.mark.parametrize("metric", [True, False])
def test_head_tail(orc, metric):
    net, hw = _net(orc, "f16x2"), SHAPES[0]
    f_32, f_64 = _t(orc.c32[hw]["head.activation1"][1]), _t(orc.c64[hw]["head.activation1"][1])
    out_hw = (50, 70)

    def ref(m, f):
        p = m.head.conv3(f)
        p = torch.sigmoid(p) * MAX_DEPTH if metric else F.relu(p)
        return F.interpolate(p, size=out_hw, mode="bilinear", align_corners=False)[:, 0]
    with torch.no_grad():
        r32, r64 = ref(orc.m32, f_32), ref(orc.m64, f_64)
    metres, mm = DA.head_tail(_d(f_32), net.conv3_w, net.conv3_b, *out_hw, metric=metric, max_depth=MAX_DEPTH, millimetres=True)
    _check(f"head tail metric={metric}", metres, r32, r64)
    want = np.clip(np.rint(1000.0 * metres.cpu().numpy().astype(np.float64)), 0, 65535).astype(np.uint16)
    assert mm.dtype == torch.uint16 and np.array_equal(mm.cpu().numpy(), want)         # the exact round-half-even of the device's own metres
    if metric:
        assert want.min() > 0 and want.max() < 65535                         # inside the format's range: the comparison is not a clamp's
    m2, none = DA.head_tail(_d(f_32), net.conv3_w, net.conv3_b, *out_hw, metric=metric, max_depth=MAX_DEPTH)
    assert none is None and torch.equal(m2, metres)
    # the row-table twin: the same bits, scattered; quantize: the metres are those of the millimetres
    src, dst = torch.tensor([1, 0, 1], dtype=torch.int32, device=DEV), torch.tensor([0, 3, 2], dtype=torch.int32, device=DEV)
    for quantize in (False, True):
        planes, st = torch.full((4, *out_hw), -7.0, device=DEV), _status()
        mm4 = torch.from_numpy(np.full((4, *out_hw), 7, np.uint16)).to(DEV)
        DA.head_tail_rows(_d(f_32), net.conv3_w, net.conv3_b, src, dst, planes, st, mm=mm4, metric=metric, max_depth=MAX_DEPTH, quantize=quantize)
        assert int(st) == 0 and bool((planes[1] == -7.0).all())
        for s, d in ((1, 0), (0, 3), (1, 2)):
            assert np.array_equal(mm4[d].cpu().numpy(), mm[s].cpu().numpy())
            assert torch.equal(planes[d], dpt.millimetres_to_metres(mm[s]) if quantize else metres[s])
    planes, st = torch.full((2, *out_hw), -7.0, device=DEV), _status()
    DA.head_tail_rows(_d(f_32), net.conv3_w, net.conv3_b, torch.tensor([2, 0], dtype=torch.int32, device=DEV), torch.tensor([1, 5], dtype=torch.int32, device=DEV), planes, st,
                      metric=metric, max_depth=MAX_DEPTH)
    assert int(st) == 1 and not bool(planes[1].any()) and bool((planes[0] == -7.0).all())


def test_head_tail_clamps_millimetres():
    f = torch.ones(1, 32, 4, 4, device=DEV)
    w = torch.full((32,), 1.0, device=DEV)
    metres, mm = DA.head_tail(f, w, 0.0, 4, 4, metric=True, max_depth=100.0, millimetres=True)       # sigmoid(32) = 1: 100 m
    assert float(metres.min()) == 100.0 and int(mm.cpu().numpy().min()) == 65535
    metres, mm = DA.head_tail(f, w, -232.0, 4, 4, metric=True, max_depth=100.0, millimetres=True)    # sigmoid(-200) = 0
    assert float(metres.max()) == 0.0 and int(mm.cpu().numpy().max()) == 0
    metres, mm = DA.head_tail(f, w, 68.0, 4, 4, metric=False, millimetres=True)                      # relative: ReLU(100)
    assert float(metres.min()) == 100.0 and int(mm.cpu().numpy().min()) == 65535
    metres, mm = DA.head_tail(f, w, -40.0, 4, 4, metric=False, millimetres=True)                     # the ReLU's zero
    assert float(metres.max()) == 0.0 and int(mm.cpu().numpy().max()) == 0


# ------------------------------------------------------------------------------------------------ end to end
def _spread_ok(d64, max_depth):
    inside, std = R.spread(d64, max_depth)
    print(f"[depth anything] reference map: {inside:.3f} inside (0.05, 0.95) max_depth, std {std:.3f} max_depth")
    assert inside >= 0.9 and std >= 0.05                                     # not a saturated sigmoid's comparison (tests/test_depth_anything_host.py)


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("hw", SHAPES)
def test_end_to_end_reduced(orc, hw, split):
    net = _net(orc, split)
    metres, _ = net(orc.img[hw].to(DEV), hw)
    _spread_ok(orc.d64[hw], MAX_DEPTH)
    _check(f"end to end reduced {hw} {split}", metres, orc.d32[hw], orc.d64[hw])


@pytest.mark.parametrize("split", SPLITS)
def test_end_to_end_vits(vits, split):
    hw = (70, 98)
    net = _net(vits, split)
    metres, _ = net(vits.img[hw].to(DEV), hw)
    _spread_ok(vits.d64[hw], 20.0)
    _check(f"end to end ViT-S {hw} {split}", metres, vits.d32[hw], vits.d64[hw])


# ------------------------------------------------------------------------------------------------ the config's stage: routes, range guard
def _stage_cfg(root, tmp_path, sd, source, name, hw=SHAPES[0]):
    import rig_scenes as S
    from mapfree_reloc_amd.config import get_cfg_defaults
    cfg = get_cfg_defaults()
    cfg.MODEL, cfg.FEATURE_MATCHING, cfg.POSE_SOLVER = "FeatureMatching", "Precomputed", "PNP"
    cfg.MATCHES_FILE_PATH = "{scene_root}/correspondences_exact.npz"
    cfg.PNP.RANSAC_ITER, cfg.PNP.REPROJECTION_INLIER_THRESHOLD, cfg.PNP.CONFIDENCE = 1000, 3, 0.9999
    cfg.DATASET.DATA_ROOT, cfg.DATASET.HEIGHT, cfg.DATASET.WIDTH, cfg.DATASET.ESTIMATED_DEPTH = str(root), S.TREE_H, S.TREE_W, name
    wpath = tmp_path / "da_weights.pth"
    if not wpath.exists():
        torch.save(sd, wpath)
    cfg.DPT.NETWORK, cfg.DPT.SOURCE = "depth_anything", source
    cfg.DA.WEIGHTS, cfg.DA.NET_HEIGHT, cfg.DA.NET_WIDTH, cfg.DA.MAX_DEPTH, cfg.DA.METRIC = str(wpath), hw[0], hw[1], MAX_DEPTH, True
    for k, v in R.REDUCED.items():
        cfg.DA.ARCH[k] = list(v) if isinstance(v, tuple) else v
    return cfg


def test_file_route_and_online_route_agree(orc, tmp_path):
    """(a) compute_depth writes the PNGs and the ordinary file route solves; (b) DPT.SOURCE 'online': the same depth bits reach the solver, and the same pose
    comes out.  The tree's own plane-depth PNGs (.dptkitti.png) stay where they are: the online route must not read them"""
    import rig_scenes as S
    from mapfree_reloc_amd import compute_depth as CD
    from mapfree_reloc_amd.builder import build_model
    from mapfree_reloc_amd.datasets import clear_frame_cache, make_loader
    tree = S.write_rig_tree(tmp_path / "tree", n_frames=6)                    # 7 frames; pairs: the keyframe against seq1 frames 0 and 5
    cfg_a = _stage_cfg(tmp_path / "tree", tmp_path, orc.sd, "file", "dasynth")
    est = dpt.DepthEstimator(cfg_a)
    assert isinstance(est.net, DA.DepthAnythingHIP)
    scene = CD.list_scene_dirs("Mapfree", tmp_path / "tree")[0]
    assert CD.run_scene(est, "Mapfree", scene, "dasynth", batch=3) == (7, 0)
    assert os.path.exists(os.path.join(tree["scene_root"], "seq1", "frame_00005.dasynth.png"))
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
        assert 0.0 < float(d0a.min()) and float(d0a.max()) < MAX_DEPTH and float(d0a.std()) > 0.5    # max_depth sigmoid of a network's logits, not the tree's plane
        print(f"[depth anything] routes: inliers {ia} / {ib}, t {ta.flatten().tolist()}")
        same = lambda u, v: torch.equal(torch.isnan(u), torch.isnan(v)) and torch.equal(torch.nan_to_num(u), torch.nan_to_num(v))
        assert same(Ra, Rb) and same(ta, tb) and ia == ib                # bit for bit (a pair the solver gives up on is NaN on both routes)


def test_range_guard_takes_the_bf16x3_rerun(orc, tmp_path):
    """fc1 of one ViT layer scaled by 2^20 and fc2 by 2^-20: the same function in exact arithmetic, but the hidden activations leave the f16x2 range.
    The guard fires, the batch runs again through the bf16x3 twin, and the result meets the bar against the float64 oracle on the SAME weights"""
    sd = {k: v.clone() for k, v in orc.sd.items()}
    p = "backbone.encoder.layer.1.mlp"
    sd[f"{p}.fc1.weight"] *= 2.0 ** 20; sd[f"{p}.fc1.bias"] *= 2.0 ** 20
    sd[f"{p}.fc2.weight"] *= 2.0 ** -20
    hw = SHAPES[0]
    m32, m64 = R.make_models(sd, DA.check_arch(R.REDUCED))
    d32 = R.run(m32, R.normalise(orc.img[hw]), capture=False)[0]
    d64 = R.run(m64, R.normalise(orc.img[hw].double()), capture=False)[0]
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
