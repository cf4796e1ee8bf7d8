"""Deterministic synthetic weights with upstream parameter names.

No checkpoints exist offline (superpoint_v1.pth / superglue_{indoor,outdoor}.pth /
{indoor,outdoor}_ot.ckpt; matchers.py:17,70), so benchmarks and parity tests run on seeded random
weights of the exact upstream architectures.  The state-dict keys are upstream's, so the real
checkpoints load through the same path (`load_checkpoint`) when they are available.

Plain i.i.d. weights make SuperGlue's assignment flat (no matches -> the solver stage would be
idle), so the SuperGlue recipe is "structured random": the GNN updates and the keypoint encoder
are scaled down (the network stays a mild perturbation of its input descriptors) and the final
projection is scaled up so that the score matrix is peaky.  Accuracy of such weights is
meaningless; shapes, arithmetic and control flow are exactly those of the trained network.

What these recipes make TRIVIAL (a trained checkpoint has none of these properties, and a device module that drops, doubles or swaps
one of the terms still agrees with the oracle on these weights):
  * LoFTR: all 17 BatchNorms are the identity (gamma 1, beta 0, mean 0, var 1); every norm1 has gamma 1, beta 0; every norm2 a constant
    gamma and beta 0; `fine_preprocess.down_proj.bias` and `fine_preprocess.merge_feat.bias` are zero;
  * SuperPoint: all 12 convolution biases are zero;
  * SuperGlue: `mlp.3.bias` of all 18 layers and `kenc.encoder.12.bias` are zero (so the offset nets/superglue.fold_weights carries from
    layer to layer is identically 0), BatchNorm is within 5 % of the identity, `bin_score` is 1.0.
tests/trained_like.py turns any of the three state dicts into one where every such term is non-trivial; the wiring of the device modules
is tested on those (tests/test_gpu_matcher_wiring.py, tests/test_weight_folding_host.py).  The defaults here stay as they are: the
benchmark, the parity census and every other test depend on these bits.
"""
import torch


def _randn(g, shape, std):
    return torch.randn(shape, generator=g) * std


def superpoint_state_dict(seed=1234):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    chans = [("conv1a", 1, 64, 3), ("conv1b", 64, 64, 3), ("conv2a", 64, 64, 3), ("conv2b", 64, 64, 3),
             ("conv3a", 64, 128, 3), ("conv3b", 128, 128, 3), ("conv4a", 128, 128, 3), ("conv4b", 128, 128, 3),
             ("convPa", 128, 256, 3), ("convPb", 256, 65, 1), ("convDa", 128, 256, 3), ("convDb", 256, 256, 1)]
    for name, ci, co, k in chans:
        fan_in = ci * k * k
        w = _randn(g, (co, ci, k, k), 1.0)
        # zero-sum filters and zero biases: an untrained ReLU stack otherwise responds mostly to
        # the image's DC level and every descriptor comes out (almost) the same vector
        w = w - w.mean(dim=(1, 2, 3), keepdim=True)
        sd[f"{name}.weight"] = w / (w.std(dim=(1, 2, 3), keepdim=True) + 1e-9) * (2.0 / fan_in) ** 0.5
        sd[f"{name}.bias"] = torch.zeros(co)
    # a peaky detector head: logits of the zero-bias stack scale with image contrast (~1e-2)
    sd["convPb.weight"] = sd["convPb.weight"] * 80.0
    return sd


def superglue_state_dict(seed=4321, gnn_gain=0.1, kenc_gain=0.1, proj_gain=12.0, n_layers=18):
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def conv1d(name, ci, co, gain=1.0, zero_bias=False):
        sd[f"{name}.weight"] = _randn(g, (co, ci, 1), gain / ci ** 0.5)
        sd[f"{name}.bias"] = torch.zeros(co) if zero_bias else _randn(g, (co,), 0.02 * gain)

    def bn(name, c):
        sd[f"{name}.weight"] = 1.0 + _randn(g, (c,), 0.05)
        sd[f"{name}.bias"] = _randn(g, (c,), 0.05)
        sd[f"{name}.running_mean"] = _randn(g, (c,), 0.05)
        sd[f"{name}.running_var"] = 1.0 + 0.1 * torch.rand((c,), generator=g)
        sd[f"{name}.num_batches_tracked"] = torch.tensor(0)
    ch = [3, 32, 64, 128, 256, 256]
    for i in range(1, 6):
        last = i == 5
        conv1d(f"kenc.encoder.{3 * (i - 1)}", ch[i - 1], ch[i], gain=kenc_gain if last else 1.4, zero_bias=last)
        if not last:
            bn(f"kenc.encoder.{3 * (i - 1) + 1}", ch[i])
    for l in range(n_layers):
        p = f"gnn.layers.{l}"
        for j in range(3):
            conv1d(f"{p}.attn.proj.{j}", 256, 256, gain=2.0 if j < 2 else 1.0)
        conv1d(f"{p}.attn.merge", 256, 256)
        conv1d(f"{p}.mlp.0", 512, 512, gain=1.4)
        bn(f"{p}.mlp.1", 512)
        conv1d(f"{p}.mlp.3", 512, 256, gain=gnn_gain, zero_bias=True)
    conv1d("final_proj", 256, 256, gain=proj_gain)
    sd["bin_score"] = torch.tensor(1.0)
    return sd


def loftr_state_dict(seed=2468, feat_gain=20.0, msg_gain=0.1, bin_score=None):
    """LoFTR (default_cfg architecture) with upstream parameter names (`backbone.*`,
    `loftr_coarse.layers.N.*`, `fine_preprocess.*`, `loftr_fine.layers.N.*`).  Structured random like
    the SuperGlue recipe: zero-sum conv filters, identity-like BatchNorm, coarse features scaled so
    that the dual-softmax is peaky (conf > 0.2 needs a ~9 nat margin over 6120 candidates), and
    transformer messages scaled down through norm2 so the GNN stays a perturbation.  bin_score: add the
    optimal-transport matcher's `coarse_matching.bin_score` (what an `*_ot.ckpt` carries); left out by default,
    as in a dual-softmax model's state dict."""
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def conv(name, ci, co, k, gain=1.0):
        w = _randn(g, (co, ci, k, k), 1.0)
        w = w - w.mean(dim=(1, 2, 3), keepdim=True)
        sd[f"{name}.weight"] = w / (w.std(dim=(1, 2, 3), keepdim=True) + 1e-9) * (gain * (2.0 / (ci * k * k)) ** 0.5)

    def bn(name, c):
        sd[f"{name}.weight"] = torch.ones(c); sd[f"{name}.bias"] = torch.zeros(c)
        sd[f"{name}.running_mean"] = torch.zeros(c); sd[f"{name}.running_var"] = torch.ones(c)
        sd[f"{name}.num_batches_tracked"] = torch.tensor(0)

    def block(name, ci, co, stride):
        conv(f"{name}.conv1", ci, co, 3); conv(f"{name}.conv2", co, co, 3); bn(f"{name}.bn1", co); bn(f"{name}.bn2", co)
        if stride != 1:
            conv(f"{name}.downsample.0", ci, co, 1); bn(f"{name}.downsample.1", co)
    conv("backbone.conv1", 1, 128, 7, gain=8.0); bn("backbone.bn1", 128)
    dims = [128, 196, 256]
    block("backbone.layer1.0", 128, 128, 1); block("backbone.layer1.1", 128, 128, 1)
    block("backbone.layer2.0", 128, 196, 2); block("backbone.layer2.1", 196, 196, 1)
    block("backbone.layer3.0", 196, 256, 2); block("backbone.layer3.1", 256, 256, 1)
    conv("backbone.layer3_outconv", 256, 256, 1, gain=feat_gain)
    conv("backbone.layer2_outconv", 196, 256, 1)
    conv("backbone.layer2_outconv2.0", 256, 256, 3); bn("backbone.layer2_outconv2.1", 256); conv("backbone.layer2_outconv2.3", 256, 196, 3)
    conv("backbone.layer1_outconv", 128, 196, 1)
    conv("backbone.layer1_outconv2.0", 196, 196, 3); bn("backbone.layer1_outconv2.1", 196); conv("backbone.layer1_outconv2.3", 196, 128, 3)

    def lin(name, ci, co, gain=1.0, bias=False):
        sd[f"{name}.weight"] = _randn(g, (co, ci), gain / ci ** 0.5)
        if bias:
            sd[f"{name}.bias"] = torch.zeros(co)

    def encoder(prefix, d, n):
        for l in range(n):
            p = f"{prefix}.layers.{l}"
            for nm in ("q_proj", "k_proj", "v_proj", "merge"):
                lin(f"{p}.{nm}", d, d)
            lin(f"{p}.mlp.0", 2 * d, 2 * d, gain=1.4); lin(f"{p}.mlp.2", 2 * d, d)
            sd[f"{p}.norm1.weight"] = torch.ones(d); sd[f"{p}.norm1.bias"] = torch.zeros(d)
            sd[f"{p}.norm2.weight"] = torch.full((d,), msg_gain); sd[f"{p}.norm2.bias"] = torch.zeros(d)
    encoder("loftr_coarse", 256, 8)
    lin("fine_preprocess.down_proj", 256, 128, gain=0.05, bias=True)
    lin("fine_preprocess.merge_feat", 256, 128, bias=True)
    encoder("loftr_fine", 128, 2)
    if bin_score is not None:
        sd["coarse_matching.bin_score"] = torch.tensor(float(bin_score))
    return sd


def lightglue_state_dict(seed=9753, n_layers=9, proj_gain=10.0, match_bias=6.0):
    """LightGlue (SuperPoint variant: descriptor_dim 256, 4 heads, no input_projection) with the parameter names of the `transformers`
    module.  Plain initialisation (N(0, 0.02) weights, zero biases, identity LayerNorm) leaves the double softmax flat: the best assignment
    score on planted twin descriptors is ~2e-3, far below the 0.1 filter threshold, and nothing matches.  So, structured random as for
    SuperGlue: the transformer stays the mild perturbation of its input that the plain initialisation makes it, and the LAST assignment layer
    is peaky and confident -- final_projection = proj_gain * I with zero bias, matchability weight x 0.1 with bias match_bias (sigmoid(6) =
    0.9975).  What this makes TRIVIAL: every bias of the transformer is zero and every LayerNorm is the identity affine map;
    tests/lightglue_ref.py perturbs them for the parity tests, as tests/trained_like.py does for the other nets."""
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def lin(name, ci, co):
        sd[f"{name}.weight"] = _randn(g, (co, ci), 0.02)
        sd[f"{name}.bias"] = torch.zeros(co)
    sd["positional_encoder.projector.weight"] = _randn(g, (32, 2), 0.02)
    for l in range(n_layers):
        for kind in ("self", "cross"):
            for n in "qkvo":
                lin(f"transformer_layers.{l}.{kind}_attention.{n}_proj", 256, 256)
            lin(f"transformer_layers.{l}.{kind}_mlp.fc1", 512, 512)
            lin(f"transformer_layers.{l}.{kind}_mlp.fc2", 512, 256)
            sd[f"transformer_layers.{l}.{kind}_mlp.layer_norm.weight"] = torch.ones(512)
            sd[f"transformer_layers.{l}.{kind}_mlp.layer_norm.bias"] = torch.zeros(512)
        lin(f"match_assignment_layers.{l}.final_projection", 256, 256)
        lin(f"match_assignment_layers.{l}.matchability", 256, 1)
        if l < n_layers - 1:
            lin(f"token_confidence.{l}.token", 256, 1)
    p = f"match_assignment_layers.{n_layers - 1}"
    sd[f"{p}.final_projection.weight"] = proj_gain * torch.eye(256)
    sd[f"{p}.matchability.weight"] = sd[f"{p}.matchability.weight"] * 0.1
    sd[f"{p}.matchability.bias"] = torch.full((1,), float(match_bias))
    return sd


def dpt_state_dict(seed=8642, arch=None, head_bias=3.0, pos_grid=24):
    """DPT-Hybrid with the parameter names of `transformers.DPTForDepthEstimation` (is_hybrid=True); `arch`: nets/dpt.ARCH keys (None: DPT-Hybrid).
    Activations stay O(1) through the whole network: BiT's convolutions are weight-standardised and every one is followed by a GroupNorm, the ViT is the
    mild perturbation of its input that N(0, 0.02) weights make it, and the neck / head convolutions are He-scaled (the pre-activation residual units at a
    third of that: sixteen of them add up).  The LAST layer's bias is lifted (the map reads as 1 - 5 metres): with a zero bias a third of the depth map sits at the
    final ReLU's zero, where errors upstream of it do not show.  What this makes TRIVIAL: every norm is the identity affine map and every other bias (but the last) is zero;
    tests/dpt_ref.perturbed moves them for the parity tests."""
    from .dpt import check_arch
    a = check_arch(arch)
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def conv(name, ci, co, k, gain=1.0, bias=True, std=None):
        sd[f"{name}.weight"] = _randn(g, (co, ci, k, k), gain * (2.0 / (ci * k * k)) ** 0.5 if std is None else std)
        if bias:
            sd[f"{name}.bias"] = torch.zeros(co)

    def norm(name, c):
        sd[f"{name}.weight"], sd[f"{name}.bias"] = torch.ones(c), torch.zeros(c)

    def lin(name, ci, co, std=0.02):
        sd[f"{name}.weight"], sd[f"{name}.bias"] = _randn(g, (co, ci), std), torch.zeros(co)

    h = a["VIT_WIDTH"]
    sd["dpt.embeddings.cls_token"] = _randn(g, (1, 1, h), 0.02)
    sd["dpt.embeddings.position_embeddings"] = _randn(g, (1, 1 + pos_grid * pos_grid, h), 0.02)
    bit = "dpt.embeddings.backbone.bit"
    conv(f"{bit}.embedder.convolution", 3, a["BIT_EMBEDDING_SIZE"], 7, bias=False)
    norm(f"{bit}.embedder.norm", a["BIT_EMBEDDING_SIZE"])
    prev = a["BIT_EMBEDDING_SIZE"]
    for s, (depth, out) in enumerate(zip(a["BIT_DEPTHS"], a["BIT_HIDDEN_SIZES"])):
        mid = out // 4
        for l in range(depth):
            p = f"{bit}.encoder.stages.{s}.layers.{l}"
            if l == 0:
                conv(f"{p}.downsample.conv", prev, out, 1, bias=False)
                norm(f"{p}.downsample.norm", out)
            conv(f"{p}.conv1", prev, mid, 1, bias=False); norm(f"{p}.norm1", mid)
            conv(f"{p}.conv2", mid, mid, 3, bias=False); norm(f"{p}.norm2", mid)
            conv(f"{p}.conv3", mid, out, 1, bias=False); norm(f"{p}.norm3", out)
            prev = out
    conv("dpt.embeddings.projection", prev, h, 1, std=prev ** -0.5)
    for l in range(a["VIT_LAYERS"]):
        p = f"dpt.encoder.layer.{l}"
        for n in ("query", "key", "value"):
            lin(f"{p}.attention.attention.{n}", h, h)
        lin(f"{p}.attention.output.dense", h, h)
        lin(f"{p}.intermediate.dense", h, a["VIT_MLP"])
        lin(f"{p}.output.dense", a["VIT_MLP"], h)
        norm(f"{p}.layernorm_before", h); norm(f"{p}.layernorm_after", h)
    norm("dpt.layernorm", h)
    ns, f = a["NECK_SIZES"], a["FUSION_WIDTH"]
    for i in (2, 3):
        conv(f"neck.reassemble_stage.layers.{i}.projection", h, ns[i], 1, std=h ** -0.5)
    conv("neck.reassemble_stage.layers.3.resize", ns[3], ns[3], 3, std=(9 * ns[3]) ** -0.5)
    for i in (2, 3):
        lin(f"neck.reassemble_stage.readout_projects.{i}.0", 2 * h, h, std=(2 * h) ** -0.5)
    for i in range(4):
        conv(f"neck.convs.{i}", ns[i], f, 3, bias=False, std=(9 * ns[i]) ** -0.5)
    for i in range(4):
        p = f"neck.fusion_stage.layers.{i}"
        conv(f"{p}.projection", f, f, 1, std=f ** -0.5)
        for r in (1, 2):
            for c in (1, 2):
                conv(f"{p}.residual_layer{r}.convolution{c}", f, f, 3, gain=1.0 / 3.0)
    conv("head.head.0", f, f // 2, 3)
    conv("head.head.2", f // 2, 32, 3)
    conv("head.head.4", 32, 1, 1, std=0.05)
    sd["head.head.4.bias"] = torch.full((1,), float(head_bias))
    return sd


def _depth_anything_logit(sd, a, x):
    """the pre-activation output of head.conv3 of Depth Anything on x [B, 3, 14 gh, 14 gw] (already normalised): plain float32 torch on the host, used by
    depth_anything_state_dict to calibrate the last layer -- the tests' oracle is the `transformers` module, never this"""
    import torch.nn.functional as F
    B, _, H, W = x.shape
    gh, gw, h, heads = H // 14, W // 14, a["VIT_WIDTH"], a["VIT_HEADS"]
    e = "backbone.embeddings"
    tok = F.conv2d(x, sd[f"{e}.patch_embeddings.projection.weight"], sd[f"{e}.patch_embeddings.projection.bias"], stride=14).flatten(2).transpose(1, 2)
    pos = sd[f"{e}.position_embeddings"]
    g = a["POS_GRID"]
    grid = F.interpolate(pos[:, 1:].reshape(1, g, g, h).permute(0, 3, 1, 2), size=(gh, gw), mode="bicubic", align_corners=False)
    t = torch.cat([sd[f"{e}.cls_token"].expand(B, -1, -1), tok], 1) + torch.cat([pos[:, :1], grid.permute(0, 2, 3, 1).reshape(1, gh * gw, h)], 1)
    ln = lambda v, n: F.layer_norm(v, (h,), sd[f"{n}.weight"], sd[f"{n}.bias"], 1e-6)
    lin = lambda v, n: F.linear(v, sd[f"{n}.weight"], sd[f"{n}.bias"])
    taps = []
    for l in range(max(a["TAPS"]) + 1):
        p = f"backbone.encoder.layer.{l}"
        y = ln(t, f"{p}.norm1")
        q, k, v = (lin(y, f"{p}.attention.attention.{n}").view(B, -1, heads, 64).transpose(1, 2) for n in ("query", "key", "value"))
        y = (torch.softmax(q @ k.transpose(-1, -2) / 8.0, -1) @ v).transpose(1, 2).reshape(B, -1, h)
        t = t + sd[f"{p}.layer_scale1.lambda1"] * lin(y, f"{p}.attention.output.dense")
        t = t + sd[f"{p}.layer_scale2.lambda1"] * lin(F.gelu(lin(ln(t, f"{p}.norm2"), f"{p}.mlp.fc1")), f"{p}.mlp.fc2")
        if l in a["TAPS"]:
            taps.append(ln(t, "backbone.layernorm")[:, 1:].transpose(1, 2).reshape(B, h, gh, gw))
    rs = "neck.reassemble_stage.layers"
    feats = []
    for i, y in enumerate(taps):
        y = F.conv2d(y, sd[f"{rs}.{i}.projection.weight"], sd[f"{rs}.{i}.projection.bias"])
        if i < 2:
            y = F.conv_transpose2d(y, sd[f"{rs}.{i}.resize.weight"], sd[f"{rs}.{i}.resize.bias"], stride=4 >> i)
        elif i == 3:
            y = F.conv2d(y, sd[f"{rs}.3.resize.weight"], sd[f"{rs}.3.resize.bias"], stride=2, padding=1)
        feats.append(F.conv2d(y, sd[f"neck.convs.{i}.weight"], padding=1))
    c3 = lambda v, n: F.conv2d(v, sd[f"{n}.weight"], sd[f"{n}.bias"], padding=1)
    unit = lambda v, n: c3(F.relu(c3(F.relu(v), f"{n}.convolution1")), f"{n}.convolution2") + v
    y = None
    for i in range(4):
        p = f"neck.fusion_stage.layers.{i}"
        y = feats[3 - i] if y is None else y + unit(feats[3 - i], f"{p}.residual_layer1")
        y = unit(y, f"{p}.residual_layer2")
        size = feats[2 - i].shape[2:] if i < 3 else (2 * y.shape[2], 2 * y.shape[3])
        y = F.conv2d(F.interpolate(y, size=tuple(size), mode="bilinear", align_corners=True), sd[f"{p}.projection.weight"], sd[f"{p}.projection.bias"])
    y = F.interpolate(c3(y, "head.conv1"), size=(H, W), mode="bilinear", align_corners=True)
    return F.conv2d(F.relu(c3(y, "head.conv2")), sd["head.conv3.weight"], sd["head.conv3.bias"])


def depth_anything_state_dict(seed=7531, arch=None, calib_hw=(70, 98)):
    """Depth Anything V2 with the parameter names of `transformers.DepthAnythingForDepthEstimation` on a Dinov2 backbone; `arch`: the keys of
    config/depth_anything_arch (None: ViT-S).  Activations stay O(1): the patch projection and the neck / head convolutions are fan-in scaled (the sixteen
    pre-activation residual units at a third of He: they add up), the ViT is the mild perturbation of its input that N(0, 0.02) weights make it, LayerScale is 1.
    The LAST layer (head.conv3) is calibrated on one seeded image at `calib_hw`: its weight is scaled and its bias set so that the pre-sigmoid logit has zero
    mean and unit spread over that image.  Plain initialisation gives a map constant to 1e-4, He scaling everywhere saturates the sigmoid at 0 and MAX_DEPTH:
    both hide every error upstream of the head.  What this makes TRIVIAL: every norm is the identity affine map, every LayerScale is 1 and every bias (but the
    last) is zero; tests/depth_anything_ref.perturbed moves them for the parity tests."""
    from .depth_anything import check_arch
    a = check_arch(arch)
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def conv(name, ci, co, k, std, bias=True, transpose=False):
        sd[f"{name}.weight"] = _randn(g, (ci, co, k, k) if transpose else (co, ci, k, k), std)
        if bias:
            sd[f"{name}.bias"] = torch.zeros(co)

    def norm(name, c):
        sd[f"{name}.weight"], sd[f"{name}.bias"] = torch.ones(c), torch.zeros(c)

    def lin(name, ci, co, std=0.02):
        sd[f"{name}.weight"], sd[f"{name}.bias"] = _randn(g, (co, ci), std), torch.zeros(co)

    h, e = a["VIT_WIDTH"], "backbone.embeddings"
    sd[f"{e}.cls_token"] = _randn(g, (1, 1, h), 0.02)
    sd[f"{e}.mask_token"] = torch.zeros(1, h)                              # part of the module's state dict; inference never reads it
    sd[f"{e}.position_embeddings"] = _randn(g, (1, 1 + a["POS_GRID"] ** 2, h), 0.02)
    conv(f"{e}.patch_embeddings.projection", 3, h, 14, std=588 ** -0.5)
    for l in range(a["VIT_LAYERS"]):
        p = f"backbone.encoder.layer.{l}"
        norm(f"{p}.norm1", h); norm(f"{p}.norm2", h)
        for n in ("query", "key", "value"):
            lin(f"{p}.attention.attention.{n}", h, h)
        lin(f"{p}.attention.output.dense", h, h)
        lin(f"{p}.mlp.fc1", h, a["VIT_MLP"])
        lin(f"{p}.mlp.fc2", a["VIT_MLP"], h)
        sd[f"{p}.layer_scale1.lambda1"], sd[f"{p}.layer_scale2.lambda1"] = torch.ones(h), torch.ones(h)
    norm("backbone.layernorm", h)
    ns, f, rs = a["NECK_SIZES"], a["FUSION_WIDTH"], "neck.reassemble_stage.layers"
    for i in range(4):
        conv(f"{rs}.{i}.projection", a["REASSEMBLE_WIDTH"], ns[i], 1, std=a["REASSEMBLE_WIDTH"] ** -0.5)
    conv(f"{rs}.0.resize", ns[0], ns[0], 4, std=ns[0] ** -0.5, transpose=True)
    conv(f"{rs}.1.resize", ns[1], ns[1], 2, std=ns[1] ** -0.5, transpose=True)
    conv(f"{rs}.3.resize", ns[3], ns[3], 3, std=(9 * ns[3]) ** -0.5)
    for i in range(4):
        conv(f"neck.convs.{i}", ns[i], f, 3, std=(9 * ns[i]) ** -0.5, bias=False)
    for i in range(4):
        p = f"neck.fusion_stage.layers.{i}"
        conv(f"{p}.projection", f, f, 1, std=f ** -0.5)
        for r in (1, 2):
            for c in (1, 2):
                conv(f"{p}.residual_layer{r}.convolution{c}", f, f, 3, std=(2.0 / (9 * f)) ** 0.5 / 3.0)
    conv("head.conv1", f, f // 2, 3, std=(2.0 / (9 * f)) ** 0.5)
    conv("head.conv2", f // 2, a["HEAD_WIDTH"], 3, std=(2.0 / (9 * (f // 2))) ** 0.5)
    conv("head.conv3", a["HEAD_WIDTH"], 1, 1, std=1.0)
    # the calibration image: smooth structure plus a little noise, normalised as the network's input is
    H, W = calib_hw
    lo = torch.rand(2, 3, max(H // 8, 2), max(W // 8, 2), generator=g)
    img = (torch.nn.functional.interpolate(lo, size=(H, W), mode="bicubic", align_corners=False) + 0.05 * torch.randn(2, 3, H, W, generator=g)).clamp(0, 1)
    x = (img - torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1)) / torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
    with torch.no_grad():
        logit = _depth_anything_logit(sd, a, x)
    s = 1.0 / float(logit.std())
    sd["head.conv3.weight"] = sd["head.conv3.weight"] * s
    sd["head.conv3.bias"] = torch.full((1,), -float(logit.mean()) * s)
    return sd


ELOFTR_STAGES = ((1, 64, 2, 1), (64, 64, 1, 2), (64, 128, 2, 4), (128, 256, 2, 14))      # (Cin, Cout, stride of the first block, blocks) of the RepVGG stages


def eloftr_state_dict(seed=1357, branch_gain=0.15, feat_gain=4.0, msg_gain=0.5, beta_gain=0.1, calib_hw=(96, 96)):
    """EfficientLoFTR with the parameter names of `transformers.EfficientLoFTRForKeypointMatching` (default configuration).  The module's own
    initialisation (BatchNorm gains ~ N(0, 0.02)) finds no match, and fan-in weights with arbitrary BatchNorm statistics grow to 1e5 through the 21
    RepVGG blocks' three summed branches.  So:
      * convolution / linear weights N(0, 1 / fan_in);
      * every BatchNorm's running statistics are those of its input on ONE seeded calibration pair, layer by layer (activations stay O(1));
      * in the blocks that have an identity branch, the two convolution branches' gains are scaled by `branch_gain`: features stay local, so a cell
        of one image resembles the same cell of a near-identical image more than its neighbours;
      * the last block is scaled by `feat_gain` (peaky dual softmax), the MLP LayerNorms by `msg_gain` / `beta_gain` (the transformer perturbs mildly).
    Every affine term is NON-trivial here (BatchNorm gains x U(0.7, 1.3), biases N(0, 0.05), LayerNorm gains U(0.7, 1.3), biases N(0, 0.3)), so a
    device module that drops or swaps one disagrees with the oracle on these weights.  Tuned on the CPU module alone (tests/test_eloftr_host.py);
    parity with the published zju-community/efficientloftr weights is unpinned offline."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def conv(name, ci, co, k):
        sd[f"{name}.weight"] = _randn(g, (co, ci, k, k), (ci * k * k) ** -0.5)
        return sd[f"{name}.weight"]

    def bn(name, y, gain, bias_gain=1.0):
        """seeded affine terms, statistics of y: returns the normalised y"""
        c = y.shape[1]
        w = gain * (0.7 + 0.6 * torch.rand(c, generator=g))
        b = 0.05 * bias_gain * torch.randn(c, generator=g)
        m, v = y.mean((0, 2, 3)), y.var((0, 2, 3), unbiased=False)
        sd[f"{name}.weight"], sd[f"{name}.bias"], sd[f"{name}.running_mean"], sd[f"{name}.running_var"] = w, b, m, v
        sd[f"{name}.num_batches_tracked"] = torch.tensor(1)
        return (y - m[None, :, None, None]) / torch.sqrt(v[None, :, None, None] + 1e-5) * w[None, :, None, None] + b[None, :, None, None]

    x = torch.rand(2, 1, *calib_hw, generator=g)
    feats = []
    base = 3 ** -0.5                                                    # three (or two) branches of unit variance sum to ~1
    for s, (ci, co, stride, blocks) in enumerate(ELOFTR_STAGES):
        for b in range(blocks):
            p = f"efficientloftr.backbone.stages.{s}.blocks.{b}"
            cin, st = (ci, stride) if b == 0 else (co, 1)
            ident = cin == co and st == 1
            last = s == len(ELOFTR_STAGES) - 1 and b == blocks - 1
            fg = feat_gain if last else 1.0
            gain = base * (branch_gain if ident else 1.0) * fg
            y = bn(f"{p}.conv1.norm", F.conv2d(x, conv(f"{p}.conv1.conv", cin, co, 3), stride=st, padding=1), gain, fg)
            y = y + bn(f"{p}.conv2.norm", F.conv2d(x, conv(f"{p}.conv2.conv", cin, co, 1), stride=st), gain, fg)
            if ident:
                y = y + bn(f"{p}.identity", x, fg, fg)
            x = F.relu(y)
        feats.append(x)
    for l in range(4):
        for kind in ("self", "cross"):
            p = f"efficientloftr.local_feature_transformer.layers.{l}.{kind}_attention"
            sd[f"{p}.aggregation.q_aggregation.weight"] = _randn(g, (256, 1, 4, 4), 0.25)
            sd[f"{p}.aggregation.norm.weight"] = 0.7 + 0.6 * torch.rand(256, generator=g)
            sd[f"{p}.aggregation.norm.bias"] = _randn(g, (256,), 0.3)
            for n in "qkvo":
                sd[f"{p}.attention.{n}_proj.weight"] = _randn(g, (256, 256), 256 ** -0.5)
            sd[f"{p}.mlp.fc1.weight"] = _randn(g, (512, 512), 512 ** -0.5)
            sd[f"{p}.mlp.fc2.weight"] = _randn(g, (256, 512), 512 ** -0.5)
            sd[f"{p}.mlp.layer_norm.weight"] = msg_gain * (0.7 + 0.6 * torch.rand(256, generator=g))
            sd[f"{p}.mlp.layer_norm.bias"] = _randn(g, (256,), 0.3 * beta_gain)
    # the fine pyramid, calibrated on the backbone's coarse map (the transformer changes it mildly)
    up = lambda t: F.interpolate(t, scale_factor=2.0, mode="bilinear", align_corners=False)
    h = up(F.conv2d(feats[3] / 16.0, conv("refinement_layer.out_conv", 256, 256, 1)))
    for i, (res, hid, mid) in enumerate(((feats[2], 128, 256), (feats[1], 64, 128))):
        p = f"refinement_layer.out_conv_layers.{i}"
        r = F.conv2d(res, conv(f"{p}.out_conv1", hid, mid, 1)) + h
        r = F.leaky_relu(bn(f"{p}.batch_norm", F.conv2d(r, conv(f"{p}.out_conv2", mid, mid, 3), padding=1), 1.0))
        h = up(F.conv2d(r, conv(f"{p}.out_conv3", mid, hid, 3), padding=1))
    return sd


def load_checkpoint(path):
    """upstream .pth / .ckpt -> flat state dict.  superpoint_v1.pth / superglue_*.pth are plain state dicts;
    LoFTR's *_ot.ckpt are Lightning checkpoints that keep it under 'state_dict' with a `matcher.` prefix
    (matchers.py:17-18 loads them strict=False after upstream strips nothing -- see strip_prefix).  Tensors only:
    weights_only=True refuses pickled code in user-supplied files."""
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if isinstance(sd, dict) and "state_dict" in sd:
        sd = sd["state_dict"]
    return sd


def strip_prefix(sd, prefix):
    return {(k[len(prefix):] if k.startswith(prefix) else k): v for k, v in sd.items()}


def synthetic_or_raise(what, cfg, maker):
    """seeded synthetic weights are only handed out when the config opted into synthetic operation
    (DATASET.SYNTHETIC or ALLOW_SYNTHETIC_WEIGHTS): a real run without checkpoints must not produce
    plausible-looking poses from random networks"""
    import warnings
    allow = bool(cfg.get("ALLOW_SYNTHETIC_WEIGHTS", False)) or bool(cfg.DATASET.get("SYNTHETIC", None))
    if not allow:
        raise FileNotFoundError(f"{what}: no checkpoint configured (set the *_WEIGHTS key), and synthetic weights were not "
                                f"requested (ALLOW_SYNTHETIC_WEIGHTS: True or DATASET.SYNTHETIC)")
    warnings.warn(f"{what}: seeded synthetic weights in use (results are NOT meaningful)")
    return maker()


def from_cfg(what, cfg, path, maker, strip=None):
    """the state dict of a config's network: the checkpoint `path` (keys without the prefix `strip`), or -- no path configured -- synthetic_or_raise"""
    if not path:
        return synthetic_or_raise(what, cfg, maker)
    sd = load_checkpoint(path)
    return strip_prefix(sd, strip) if strip else sd
