"""CPU: the host side of the EfficientLoFTR stage (nets/eloftr.py) -- the float64 weight folding against the `transformers` module's blocks, the
seeded weight recipe against the oracle ALONE (it must produce matches, and the float32 module must meet, against the float64 module, every
condition tests/test_gpu_eloftr.py puts on the device), the config node, the registries and the errors for unsupported settings."""
import pytest
import torch

import eloftr_ref as R
import mapfree_reloc_amd as mfr  # noqa: F401
from mapfree_reloc_amd.config.default import cfg as default_cfg
from mapfree_reloc_amd.nets import eloftr as EL


@pytest.fixture(scope="module")
def oracle64():
    return R.modules("perturbed")[1]


def test_perturbed_weights_have_no_trivial_term():
    sd = R.weights("perturbed")
    for k, v in sd.items():
        if k.endswith("running_var"):
            p = k[:-len("running_var")]
            assert float((sd[p + "weight"] - 1).abs().min()) > 1e-4 and float(sd[p + "bias"].abs().min()) > 0 and float(sd[p + "running_mean"].abs().min()) > 0
            assert float((v - 1).abs().min()) > 1e-6
        if k.endswith("layer_norm.bias") or k.endswith("aggregation.norm.bias"):
            assert float(v.abs().min()) > 0
    assert abs(float(sd["efficientloftr.backbone.stages.1.blocks.0.identity.running_var"][3]) - 1e-3) < 1e-9


@pytest.mark.parametrize("prefix,cin,stride", [("efficientloftr.backbone.stages.0.blocks.0", 1, 2),           # no identity branch, stride 2, one input channel
                                               ("efficientloftr.backbone.stages.1.blocks.0", 64, 1),          # identity branch, the channel with running_var 1e-3
                                               ("efficientloftr.backbone.stages.2.blocks.0", 64, 2),
                                               ("efficientloftr.backbone.stages.3.blocks.13", 256, 1)])
def test_folded_repvgg_block_equals_module_block(oracle64, prefix, cin, stride):
    """folded 3x3 + bias + ReLU == the module's three-branch block, float64, 1e-12 relative"""
    sd = {k: v.double() for k, v in R.weights("perturbed").items()}
    blk = oracle64.get_submodule(prefix)
    x = torch.randn(2, cin, 12, 10, dtype=torch.float64, generator=torch.Generator().manual_seed(1)) * 2.0
    w, b = EL.fold_repvgg_block(sd, prefix)
    with torch.no_grad():
        want = blk(x)
    got = torch.relu(torch.nn.functional.conv2d(x, w, b, stride=stride, padding=1))
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_fold_weights_backbone_and_outconv_equal_module(oracle64):
    """the whole folded backbone (f32 operands evaluated in float64: only the cast separates them) and the BN-folded OutConvBlock against the module"""
    sd = R.weights("perturbed")
    fw = EL.fold_weights(sd)
    assert [f["stride"] for f in fw["backbone"]] == [2, 1, 1, 2, 1, 1, 1, 2] + [1] * 13 and len(fw["layers"]) == 4
    assert [f["w_skip"] is not None for f in fw["backbone"]] == [False, True, True, False, True, True, True, False] + [True] * 13
    # the skip form of a block with an identity branch is the same map: conv(x; w - I) + x == conv(x; w), float64
    f = fw["backbone"][8]
    x = torch.randn(1, 256, 6, 5, dtype=torch.float64, generator=torch.Generator().manual_seed(4))
    a = torch.nn.functional.conv2d(x, f["w"].double(), padding=1)
    b = torch.nn.functional.conv2d(x, f["w_skip"].double(), padding=1) + x
    assert float((a - b).abs().max()) <= 1e-6 * float(a.abs().max())          # f32 casts of w and w - I, not 1e-12: the two are rounded separately
    g = torch.Generator().manual_seed(2)
    for i in range(2):
        blk = oracle64.refinement_layer.out_conv_layers[i]
        mid, hid = blk.out_conv2.weight.shape[0], blk.out_conv3.weight.shape[0]
        h, res = torch.randn(1, mid, 8, 6, dtype=torch.float64, generator=g), torch.randn(1, hid, 8, 6, dtype=torch.float64, generator=g)
        sd64 = {k: v.double() for k, v in sd.items()}
        s, b = EL._bn_fold(sd64, f"refinement_layer.out_conv_layers.{i}.batch_norm", EL.BN_EPS_DEFAULT)
        w2 = sd64[f"refinement_layer.out_conv_layers.{i}.out_conv2.weight"] * s[:, None, None, None]
        assert torch.equal(w2.float(), fw["fine"][i]["w2"]) and torch.equal(b.float(), fw["fine"][i]["b2"])
        F = torch.nn.functional
        with torch.no_grad():
            want = blk(h, res)
        r = F.conv2d(res, sd64[f"refinement_layer.out_conv_layers.{i}.out_conv1.weight"]) + h
        r = F.conv2d(F.leaky_relu(F.conv2d(r, w2, b, padding=1), 0.01), sd64[f"refinement_layer.out_conv_layers.{i}.out_conv3.weight"], padding=1)
        got = F.interpolate(r, scale_factor=2.0, mode="bilinear", align_corners=False)
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_rotary_table_is_the_modules():
    """cos | sin of the 128 angles per aggregated cell == the float32 module's embedding with every angle repeated twice, bit for bit (odd height 5 x 3)"""
    x = torch.zeros(1, 256, 20, 12)
    cos, sin = R.modules("perturbed")[0].efficientloftr.rotary_emb(x)
    cs = EL.rotary_table(5, 3, "cpu")
    assert torch.equal(cs[:, :128].repeat_interleave(2, -1), cos.reshape(15, 256).float()) and torch.equal(cs[:, 128:].repeat_interleave(2, -1), sin.reshape(15, 256).float())


def test_recipe_matches_with_the_oracle_alone():
    """the end-to-end pair on the perturbed recipe: the float32 module finds matches on BOTH pairs, the same ones as the float64 module on safe cells,
    <= 2 % of the cells are unsafe, and its coordinates are within 1e-3 px -- the conditions the GPU test puts on the device"""
    m32, m64 = R.modules("perturbed")
    im = R.end_to_end_images()
    o32, o64 = R.end_to_end(m32, im), R.end_to_end(m64, im.double())
    safe = R.coarse_safe(o64["conf"])
    assert float((~safe).float().mean()) <= 0.02
    for p in range(2):
        a, b = o32["pairs"][p], o64["pairs"][p]
        assert b["i"].numel() >= 20, (p, b["i"].numel())
        ja, jb = torch.full((safe.shape[1],), -1), torch.full((safe.shape[1],), -1)
        ja[a["i"]], jb[b["i"]] = a["j"], b["j"]
        assert torch.equal(ja[safe[p]], jb[safe[p]])
        both = torch.isin(a["i"], b["i"])
        ia = a["i"][both]
        pos = torch.searchsorted(b["i"], ia)
        d = max(float((a["pts0"][both].double() - b["pts0"][pos]).abs().max()), float((a["pts1"][both].double() - b["pts1"][pos]).abs().max()))
        print(f"[eloftr host] pair {p}: {b['i'].numel()} matches, f32 vs f64 coordinates {d:.2e} px")
        assert d <= R.COORD_FLOOR


@pytest.mark.parametrize("hw", R.SHAPES)
def test_constructed_inputs_are_decidable_for_the_oracle(hw):
    """the constructed coarse features and fine windows of the GPU test: float64 confidences of true pairs above 0.2 with some near it, <= 2 % unsafe
    cells / matches, and the forced winners on rows / columns 0 and 7 are there"""
    hc, wc = hw[0] // 8, hw[1] // 8
    f0, f1, perm = R.constructed_coarse((hc, wc))
    conf = R.coarse_confidence(f0, f1)
    true = conf.gather(2, perm[..., None])[..., 0]
    assert float((true > 0.2).float().mean()) > 0.5 and int(((true > 0.1) & (true < 0.4)).sum()) >= 3
    assert float((~R.coarse_safe(conf)).float().mean()) <= 0.02
    w0, w1, _, _ = R.constructed_windows()
    arg, safe = R.fine_stage1(w0, w1)
    assert float((~safe).float().mean()) <= 0.02
    i1 = arg % 64
    rows, cols = set((i1 // 8).tolist()), set((i1 % 8).tolist())
    assert {0, 7} <= rows and {0, 7} <= cols


def test_config_node_and_registries():
    from mapfree_reloc_amd import matchers
    from mapfree_reloc_amd.matching import feature_matching as FM, model
    el = default_cfg.ELOFTR
    assert (el.MATCH_THRESHOLD, el.BORDER_RM, el.TEMPERATURE) == (0.2, 2, 0.1) and not el.WEIGHTS and isinstance(el.SYNTHETIC_SEED, int)
    assert model.FEATURE_MATCHERS["EfficientLoFTR"] is FM.EfficientLoFTRMatching
    assert matchers.MATCHERS["ELoFTR"] is matchers.ELoFTR_matcher
    assert EL.check_cfg(default_cfg) is el


@pytest.mark.parametrize("key,value", [("MATCH_THRESHOLD", 1.5), ("BORDER_RM", -1), ("TEMPERATURE", 0.0), ("SKIP_SOFTMAX", True), ("HALF_PRECISION", True)])
def test_unsupported_settings_raise(key, value):
    c = default_cfg.clone()
    c.ELOFTR[key] = value
    with pytest.raises(ValueError, match=f"ELOFTR.{key}"):
        EL.check_cfg(c)


def test_synthetic_weights_need_the_opt_in():
    c = default_cfg.clone()
    c.ALLOW_SYNTHETIC_WEIGHTS = False
    with pytest.raises(FileNotFoundError, match="EfficientLoFTR"):
        EL.from_cfg(c, "cpu")


def test_seed_changes_the_recipe_and_names_are_the_modules():
    from mapfree_reloc_amd.nets import weights as WT
    a, b = WT.eloftr_state_dict(1), WT.eloftr_state_dict(2)
    m = R.module(a)
    assert set(a) == set(m.state_dict()) and not torch.equal(a["refinement_layer.out_conv.weight"], b["refinement_layer.out_conv.weight"])
