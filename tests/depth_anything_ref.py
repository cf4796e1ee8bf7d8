"""The oracle of the Depth Anything tests: `transformers.DepthAnythingForDepthEstimation` on a Dinov2 backbone in float32 and float64 on OUR state dict, run
at any input size that is a multiple of 14, with every module's inputs and output captured.  Test infrastructure only: the product never imports it."""
import torch

BIAS_STD = 0.05
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

# the reduced architecture of the tests (config/depth_anything_arch keys): a CPU oracle in milliseconds, every code path of the full one.  The 48- and
# 96-channel neck layers of ViT-S are kept: they are the widths that are no multiple of the GEMM's K step
REDUCED = dict(VIT_WIDTH=192, VIT_LAYERS=4, VIT_HEADS=3, VIT_MLP=384, TAPS=(0, 1, 2, 3), REASSEMBLE_WIDTH=192, NECK_SIZES=(48, 96, 192, 192), FUSION_WIDTH=64,
               HEAD_WIDTH=32, PATCH=14, POS_GRID=5, MAX_DEPTH=20.0, METRIC=True)
SHAPES = [(70, 98), (98, 42), (56, 84)]          # grids 5x7 (both odd: the fusion upsamples 3 -> 5 and 4 -> 7), 7x3, 4x6 (every fusion step is x2)


def hf_config(arch):
    """architecture dict -> DepthAnythingConfig"""
    from transformers import DepthAnythingConfig, Dinov2Config
    assert arch["VIT_MLP"] % arch["VIT_WIDTH"] == 0
    bc = Dinov2Config(hidden_size=arch["VIT_WIDTH"], num_hidden_layers=arch["VIT_LAYERS"], num_attention_heads=arch["VIT_HEADS"],
                      mlp_ratio=arch["VIT_MLP"] // arch["VIT_WIDTH"], image_size=14 * arch["POS_GRID"], patch_size=14, layer_norm_eps=1e-6,
                      out_indices=[t + 1 for t in arch["TAPS"]], apply_layernorm=True, reshape_hidden_states=False, attn_implementation="eager")
    return DepthAnythingConfig(backbone_config=bc, patch_size=14, reassemble_hidden_size=arch["REASSEMBLE_WIDTH"], neck_hidden_sizes=list(arch["NECK_SIZES"]),
                               fusion_hidden_size=arch["FUSION_WIDTH"], head_hidden_size=arch["HEAD_WIDTH"], reassemble_factors=[4, 2, 1, 0.5], head_in_index=-1,
                               depth_estimation_type="metric" if arch["METRIC"] else "relative", max_depth=int(arch["MAX_DEPTH"]) if arch["METRIC"] else 1)      # (whole metres)


def perturbed(sd, seed=0):
    """every norm's gain and bias and every (zero) bias moved off its initial value, and every LayerScale vector drawn from [0.5, 1.5]: a dropped or
    misplaced term, or a dropped LayerScale fold, shows"""
    g = torch.Generator().manual_seed(int(seed))
    out = {k: v.clone() for k, v in sd.items()}
    norm = lambda k: ".norm" in k or "layernorm" in k
    for k in sorted(sd):
        if k.endswith(".weight") and norm(k) and sd[k].dim() == 1:
            c = sd[k].numel()
            gamma = sd[k] * (0.7 + 0.6 * torch.rand(c, generator=g))
            out[k] = gamma
            out[k[:-len("weight")] + "bias"] = sd[k[:-len("weight")] + "bias"] + 0.3 * gamma.abs().mean() * torch.randn(c, generator=g)
        elif k.endswith(".lambda1"):
            out[k] = 0.5 + torch.rand(sd[k].numel(), generator=g)
    for k in sorted(sd):
        if k.endswith(".bias") and not norm(k) and not bool(sd[k].any()):
            out[k] = BIAS_STD * torch.randn(sd[k].numel(), generator=g)
    return out


def make_models(sd, arch):
    """float32 and float64 twins on one state dict (strict: every key of the module, no other)"""
    from transformers import DepthAnythingForDepthEstimation
    out = []
    for dt in (torch.float32, torch.float64):
        m = DepthAnythingForDepthEstimation(hf_config(arch)).eval()
        m.load_state_dict(sd, strict=True)
        out.append(m.to(dt))
    return out


@torch.no_grad()
def run(m, x, capture=True):
    """x [B, 3, H, W] normalised (H, W multiples of 14) -> (predicted depth [B, H, W], {module name: (inputs, output)}) in the module's dtype"""
    dt = next(m.parameters()).dtype
    caps, hooks = {}, []
    if capture:
        for name, mod in m.named_modules():
            hooks.append(mod.register_forward_hook(lambda mod_, inp, out, name=name: caps.__setitem__(name, (inp, out))))
    try:
        depth = m(pixel_values=x.to(dt)).predicted_depth
    finally:
        for h in hooks:
            h.remove()
    return depth, caps


def normalise(img):
    """[B, 3, H, W] in [0, 1] -> ImageNet-normalised, in the tensor's dtype"""
    mean, std = (torch.tensor(v, dtype=img.dtype).view(1, 3, 1, 1) for v in (MEAN, STD))
    return (img - mean) / std


def make_images(B, H, W, seed=0):
    """smooth random images in [0, 1], a different one per batch entry: f32 [B, 3, H, W]"""
    g = torch.Generator().manual_seed(100 + int(seed))
    lo = torch.rand(B, 3, max(H // 8, 2), max(W // 8, 2), generator=g)
    img = torch.nn.functional.interpolate(lo, size=(H, W), mode="bicubic", align_corners=False) + 0.05 * torch.randn(B, 3, H, W, generator=g)
    return img.clamp(0, 1).contiguous()


def spread(d64, max_depth):
    """(fraction of the map inside (0.05, 0.95) max_depth, its standard deviation / max_depth): the conditions that keep a comparison from being a saturated
    sigmoid's (>= 0.9 and >= 0.05)"""
    d = d64.double() / float(max_depth)
    return float(((d > 0.05) & (d < 0.95)).double().mean()), float(d.std())
