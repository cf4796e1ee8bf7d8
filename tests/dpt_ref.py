"""The oracle of the DPT-Hybrid tests: `transformers.DPTForDepthEstimation` (is_hybrid=True) in float32 and float64 on OUR state dict, run at any
input size that is a multiple of 32, with every module's inputs and output captured.  Test infrastructure only: the product never imports it.

The module's own forward takes square inputs of the configured size only; for another size `run` sets dpt.embeddings.image_size, calls
model.dpt(x, output_hidden_states=True), assembles the hybrid tap list (the two BiT feature maps, then the tapped ViT layers), and calls model.neck and
model.head -- on a square input of the configured size this equals model(pixel_values=x).predicted_depth exactly."""
import torch

BIAS_STD = 0.05

# the reduced architecture of the tests (nets/dpt.ARCH keys) -- small enough for a CPU oracle in milliseconds, every code path of the full one
REDUCED = dict(BIT_DEPTHS=(1, 1, 2), BIT_HIDDEN_SIZES=(64, 128, 256), BIT_EMBEDDING_SIZE=32, NUM_GROUPS=8, VIT_WIDTH=192, VIT_LAYERS=4, VIT_HEADS=3,
               VIT_MLP=384, NECK_SIZES=(64, 128, 192, 192), FUSION_WIDTH=64, TAPS=(0, 1, 2, 3))


def hf_config(arch, image_size=384):
    """nets/dpt architecture dict -> DPTConfig"""
    from transformers import BitConfig, DPTConfig
    bit = BitConfig(depths=list(arch["BIT_DEPTHS"]), hidden_sizes=list(arch["BIT_HIDDEN_SIZES"]) + [2 * arch["BIT_HIDDEN_SIZES"][-1]],
                    embedding_size=arch["BIT_EMBEDDING_SIZE"], num_groups=arch["NUM_GROUPS"], global_padding="same", layer_type="bottleneck",
                    embedding_dynamic_padding=True, out_features=["stage1", "stage2", "stage3"])
    return DPTConfig(is_hybrid=True, backbone_config=bit, hidden_size=arch["VIT_WIDTH"], num_hidden_layers=arch["VIT_LAYERS"],
                     num_attention_heads=arch["VIT_HEADS"], intermediate_size=arch["VIT_MLP"], patch_size=16, image_size=image_size, readout_type="project",
                     neck_hidden_sizes=list(arch["NECK_SIZES"]), fusion_hidden_size=arch["FUSION_WIDTH"], backbone_out_indices=list(arch["TAPS"]),
                     backbone_featmap_shape=[1, arch["BIT_HIDDEN_SIZES"][-1], image_size // 16, image_size // 16], attn_implementation="eager")


def perturbed(sd, seed=0):
    """every norm's gain and bias and every (zero) bias moved off its initial value, so that a dropped or misplaced term shows"""
    g = torch.Generator().manual_seed(int(seed))
    out = {k: v.clone() for k, v in sd.items()}
    norm = lambda k: ".norm" in k or "layernorm" in k
    for k in sorted(sd):
        if k.endswith(".weight") and norm(k) and sd[k].dim() == 1:
            c = sd[k].numel()
            gamma = sd[k] * (0.7 + 0.6 * torch.rand(c, generator=g))
            out[k] = gamma
            out[k[:-len("weight")] + "bias"] = sd[k[:-len("weight")] + "bias"] + 0.3 * gamma.abs().mean() * torch.randn(c, generator=g)
    for k in sorted(sd):
        if k.endswith(".bias") and not norm(k) and not bool(sd[k].any()):
            out[k] = BIAS_STD * torch.randn(sd[k].numel(), generator=g)
    return out


def make_models(sd, arch):
    """float32 and float64 twins on one state dict (strict: every key of the module, no other)"""
    from transformers import DPTForDepthEstimation
    n = sd["dpt.embeddings.position_embeddings"].shape[1] - 1
    out = []
    for dt in (torch.float32, torch.float64):
        m = DPTForDepthEstimation(hf_config(arch, image_size=16 * int(round(n ** 0.5)))).eval()
        m.load_state_dict(sd, strict=True)
        out.append(m.to(dt))
    return out


@torch.no_grad()
def run(m, x, capture=True):
    """x [B, 3, H, W] (H, W multiples of 32) -> (predicted depth [B, H, W], {module name: (inputs, output)}) in the module's dtype"""
    dt = next(m.parameters()).dtype
    x = x.to(dt)
    B, _, H, W = x.shape
    caps, hooks = {}, []
    if capture:
        for name, mod in m.named_modules():
            hooks.append(mod.register_forward_hook(lambda mod_, inp, out, name=name: caps.__setitem__(name, (inp, out))))
    old = m.dpt.embeddings.image_size
    try:
        m.dpt.embeddings.image_size = (H, W)
        o = m.dpt(x, output_hidden_states=True)
        hs = list(o.hidden_states[1:])
        taps = list(o.intermediate_activations) + [hs[i] for i in m.config.backbone_out_indices[2:]]
        feats = m.neck(taps, H // 16, W // 16)
        depth = m.head(feats)
    finally:
        m.dpt.embeddings.image_size = old
        for h in hooks:
            h.remove()
    caps["__taps__"] = (tuple(taps), None)
    return depth, caps


def make_images(B, H, W, seed=0):
    """smooth random images in [0, 1], a different one per batch entry: f32 [B, 3, H, W]"""
    g = torch.Generator().manual_seed(100 + int(seed))
    lo = torch.rand(B, 3, max(H // 8, 2), max(W // 8, 2), generator=g)
    img = torch.nn.functional.interpolate(lo, size=(H, W), mode="bicubic", align_corners=False) + 0.05 * torch.randn(B, 3, H, W, generator=g)
    return img.clamp(0, 1).contiguous()
