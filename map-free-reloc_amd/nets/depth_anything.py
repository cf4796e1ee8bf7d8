"""Depth Anything V2 metric depth (Yang et al., NeurIPS 2024: a DINOv2 ViT-S / B / L behind a DPT head): architecture table, host-side weight folding and the
launches of csrc/depth_anything.hip.

The architecture of record is `transformers.DepthAnythingForDepthEstimation` on a Dinov2 backbone, and the state-dict keys are its keys
(`backbone.embeddings.*`, `backbone.encoder.layer.{i}.*`, `backbone.layernorm.*`, `neck.reassemble_stage.layers.{i}.{projection,resize}`, `neck.convs.{i}`,
`neck.fusion_stage.layers.{i}.*`, `head.conv{1,2,3}`); the product never imports that package (tests/depth_anything_ref.py drives it as the oracle).

What is here:
  * check_arch             the architecture dict (config/depth_anything_arch: ViT-S / B / L presets); refuses what the kernels do not have;
  * fold_layerscale, resize_position_embeddings, from_upstream / to_upstream   host code, run once per weight set (q / k / v and the transposed convolutions
                           fold with nets/dpt's fold_qkv / fold_conv_transpose);
  * patch_rows (_tab), tokens, head_tail (_rows)   the launches of include/mfr_hip.h mfr_da_*;
  * DepthAnythingHIP       the network, inference only, on nets/dpt.DepthNetBase: the ViT layer, the fusion layer and the residual unit are DPT-Hybrid's code.
                           The patch embedding is ONE SplitLinear product with K = 588 (padded to 640) on mfr_da_patch_rows' output; the x4 / x2 reassemble
                           layers are ConvTranspose2d(k = s) as a GEMM + mfr_dpt_shuffle; each stage is a method, which is what the stage-level tests call.
  * check_cfg / network_from_cfg   the config's DA node behind nets/dpt.build_network (DPT.NETWORK 'depth_anything')."""
import re

import torch

from .. import _lib, options
from ..config.depth_anything_arch import ARCH, PRESETS
from . import dpt
from .conv import IgemmConv, WinoConv3x3
from .linear import SplitLinear

HEAD_DIM = 64                       # mfr_sg_attention's head width
LN_EPS = 1e-6                       # Dinov2Config.layer_norm_eps
PATCH = 14
PATCH_K = 3 * PATCH * PATCH         # 588 real terms of the patch embedding
PATCH_LDK = 640                     # ... padded to the GEMM's K step of 64 (the LDS-DMA kernel; 52 zero columns)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)     # ImageNet normalisation of the authors' transform
REASSEMBLE_FACTORS = (4, 2, 1, 0.5)


def check_arch(arch=None):
    """the architecture dict with the defaults (ViT-S) filled in; refuses what the kernels do not have"""
    a = dict(ARCH, SWIGLU=False)
    unknown = set(arch or {}) - set(a)
    if unknown:
        raise ValueError(f"DepthAnything: unknown architecture keys {sorted(unknown)}")
    a.update(arch or {})
    if a["SWIGLU"]:
        raise ValueError("DepthAnything: the SwiGLU MLP (ViT-g) has no kernel here; ViT-S / B / L use the GELU MLP")
    if a["VIT_WIDTH"] != HEAD_DIM * a["VIT_HEADS"]:
        raise ValueError(f"DepthAnything: head dimension {a['VIT_WIDTH']}/{a['VIT_HEADS']} is not {HEAD_DIM}, the only width the attention kernel has")
    if a["VIT_WIDTH"] % 64 or a["VIT_WIDTH"] > 1024:
        raise ValueError("DepthAnything: ViT width must be a multiple of 64, at most 1024 (mfr_dpt_layernorm)")
    if a["HEAD_WIDTH"] > 64 or a["HEAD_WIDTH"] < 1:
        raise ValueError("DepthAnything: the head's last layer takes at most 64 channels (mfr_da_head_tail)")
    if len(a["NECK_SIZES"]) != 4 or len(a["TAPS"]) != 4 or max(a["TAPS"]) >= a["VIT_LAYERS"] or min(a["TAPS"]) < 0:
        raise ValueError("DepthAnything: four neck sizes and four taps, each tap a ViT layer")
    if a["PATCH"] != PATCH or a["REASSEMBLE_WIDTH"] != a["VIT_WIDTH"] or a["VIT_MLP"] % 32 or a["FUSION_WIDTH"] % 2 or a["POS_GRID"] < 1:
        raise ValueError("DepthAnything: patch size 14, REASSEMBLE_WIDTH = VIT_WIDTH, VIT_MLP a multiple of 32, an even FUSION_WIDTH")
    if a["METRIC"] and not float(a["MAX_DEPTH"]) > 0:
        raise ValueError("DepthAnything: the metric head needs MAX_DEPTH > 0")
    return a


# ------------------------------------------------------------------------------------------------ host-side folding
def fold_layerscale(weight, bias, lam):
    """LayerScale behind a linear layer, folded into it (float64): lam * (W x + b) = (diag(lam) W) x + lam b -- no kernel and no extra pass over the tokens"""
    lam = lam.detach().double()
    return lam[:, None] * weight.detach().double(), lam * bias.detach().double()


def resize_position_embeddings(pos, gh, gw):
    """pos [1, 1 + g^2, h] -> [1 + gh gw, h] float32 as Dinov2Embeddings.interpolate_pos_encoding does: the grid rows through F.interpolate(size=(gh, gw),
    mode='bicubic', align_corners=False) in float32, the cls row kept; the trained grid itself is returned as it is.  Host code; cached per grid shape"""
    p = pos.detach().float().cpu()
    n, h = p.shape[1] - 1, p.shape[2]
    g = int(round(n ** 0.5))
    assert g * g == n, "position embeddings must come from a square grid"
    if (int(gh), int(gw)) == (g, g):
        return p[0].contiguous()
    grid = p[0, 1:].reshape(1, g, g, h).permute(0, 3, 1, 2)
    grid = torch.nn.functional.interpolate(grid, size=(int(gh), int(gw)), mode="bicubic", align_corners=False)
    return torch.cat([p[0, :1], grid.permute(0, 2, 3, 1).reshape(int(gh) * int(gw), h)], 0).contiguous()


_BLOCK = {"norm1": "norm1", "norm2": "norm2", "attn.proj": "attention.output.dense", "mlp.fc1": "mlp.fc1", "mlp.fc2": "mlp.fc2"}
_HEAD = {"output_conv1": "conv1", "output_conv2.0": "conv2", "output_conv2.2": "conv3"}


def from_upstream(sd):
    """UNPINNED.  A Depth Anything V2 checkpoint with the parameter names of the authors' repository (DepthAnything/Depth-Anything-V2: `pretrained.*` is the
    DINOv2 ViT, `depth_head.*` the DPT head) -> the names used here.  The renames follow the published architecture and the public conversion of these
    checkpoints to `transformers`; no such file exists offline, so nothing pins this against a real checkpoint -- only the round trip through to_upstream is
    tested (tests/test_depth_anything_host.py).  attn.qkv is split into query / key / value; anything unknown raises."""
    out = {}
    for k, v in sd.items():
        n = None
        m = re.match(r"pretrained\.blocks\.(\d+)\.(.+)\.(weight|bias|gamma)$", k)
        if m:
            i, what, wb = m.groups()
            base = f"backbone.encoder.layer.{i}."
            if what == "attn.qkv" and wb != "gamma":
                h = v.shape[0] // 3
                for j, name in enumerate(("query", "key", "value")):
                    out[f"{base}attention.attention.{name}.{wb}"] = v[j * h:(j + 1) * h].clone()
                continue
            if what in ("ls1", "ls2") and wb == "gamma":
                n = f"{base}layer_scale{what[2]}.lambda1"
            elif what in _BLOCK and wb != "gamma":
                n = f"{base}{_BLOCK[what]}.{wb}"
        elif k in ("pretrained.cls_token", "pretrained.mask_token"):
            n = "backbone.embeddings." + k.split(".")[1]
        elif k == "pretrained.pos_embed":
            n = "backbone.embeddings.position_embeddings"
        elif re.match(r"pretrained\.patch_embed\.proj\.(weight|bias)$", k):
            n = "backbone.embeddings.patch_embeddings.projection." + k.rsplit(".", 1)[1]
        elif re.match(r"pretrained\.norm\.(weight|bias)$", k):
            n = "backbone.layernorm." + k.rsplit(".", 1)[1]
        else:
            m = re.match(r"depth_head\.(projects|resize_layers)\.([0-3])\.(weight|bias)$", k)
            if m and not (m.group(1) == "resize_layers" and m.group(2) == "2"):
                n = f"neck.reassemble_stage.layers.{m.group(2)}.{'projection' if m.group(1) == 'projects' else 'resize'}.{m.group(3)}"
            m = re.match(r"depth_head\.scratch\.layer([1-4])_rn\.weight$", k)
            if m:
                n = f"neck.convs.{int(m.group(1)) - 1}.weight"
            m = re.match(r"depth_head\.scratch\.refinenet([1-4])\.(out_conv|resConfUnit[12]\.conv[12])\.(weight|bias)$", k)
            if m:
                what = m.group(2).replace("out_conv", "projection").replace("resConfUnit", "residual_layer").replace("conv", "convolution")
                n = f"neck.fusion_stage.layers.{4 - int(m.group(1))}.{what}.{m.group(3)}"
            m = re.match(r"depth_head\.scratch\.(output_conv1|output_conv2\.[02])\.(weight|bias)$", k)
            if m:
                n = f"head.{_HEAD[m.group(1)]}.{m.group(2)}"
        if n is None:
            raise KeyError(f"DepthAnything.from_upstream: no place for {k!r}")
        out[n] = v
    return out


def to_upstream(sd):
    """the inverse of from_upstream (our names -> the authors'), for its round-trip test and for handing weights back; anything unknown raises"""
    out, qkv = {}, {}
    inv_block, inv_head = {v: k for k, v in _BLOCK.items()}, {v: k for k, v in _HEAD.items()}
    for k, v in sd.items():
        n = None
        m = re.match(r"backbone\.encoder\.layer\.(\d+)\.(.+)\.(weight|bias|lambda1)$", k)
        if m:
            i, what, wb = m.groups()
            mq = re.match(r"attention\.attention\.(query|key|value)$", what)
            if mq and wb != "lambda1":
                qkv.setdefault((i, wb), {})[mq.group(1)] = v
                continue
            if what in ("layer_scale1", "layer_scale2") and wb == "lambda1":
                n = f"pretrained.blocks.{i}.ls{what[-1]}.gamma"
            elif what in inv_block and wb != "lambda1":
                n = f"pretrained.blocks.{i}.{inv_block[what]}.{wb}"
        elif k in ("backbone.embeddings.cls_token", "backbone.embeddings.mask_token"):
            n = "pretrained." + k.rsplit(".", 1)[1]
        elif k == "backbone.embeddings.position_embeddings":
            n = "pretrained.pos_embed"
        elif re.match(r"backbone\.embeddings\.patch_embeddings\.projection\.(weight|bias)$", k):
            n = "pretrained.patch_embed.proj." + k.rsplit(".", 1)[1]
        elif re.match(r"backbone\.layernorm\.(weight|bias)$", k):
            n = "pretrained.norm." + k.rsplit(".", 1)[1]
        else:
            m = re.match(r"neck\.reassemble_stage\.layers\.([0-3])\.(projection|resize)\.(weight|bias)$", k)
            if m:
                n = f"depth_head.{'projects' if m.group(2) == 'projection' else 'resize_layers'}.{m.group(1)}.{m.group(3)}"
            m = re.match(r"neck\.convs\.([0-3])\.weight$", k)
            if m:
                n = f"depth_head.scratch.layer{int(m.group(1)) + 1}_rn.weight"
            m = re.match(r"neck\.fusion_stage\.layers\.([0-3])\.(projection|residual_layer[12]\.convolution[12])\.(weight|bias)$", k)
            if m:
                what = m.group(2).replace("projection", "out_conv").replace("residual_layer", "resConfUnit").replace("convolution", "conv")
                n = f"depth_head.scratch.refinenet{4 - int(m.group(1))}.{what}.{m.group(3)}"
            m = re.match(r"head\.(conv[123])\.(weight|bias)$", k)
            if m:
                n = f"depth_head.scratch.{inv_head[m.group(1)]}.{m.group(2)}"
        if n is None:
            raise KeyError(f"DepthAnything.to_upstream: no place for {k!r}")
        out[n] = v
    for (i, wb), parts in qkv.items():
        out[f"pretrained.blocks.{i}.attn.qkv.{wb}"] = torch.cat([parts["query"], parts["key"], parts["value"]], 0)
    return out


# ------------------------------------------------------------------------------------------------ the launches
def _grid_of(net_h, net_w):
    if net_h % PATCH or net_w % PATCH or net_h < PATCH or net_w < PATCH:
        raise ValueError(f"DepthAnything: network size {net_h} x {net_w}: both must be multiples of {PATCH}")
    return int(net_h) // PATCH, int(net_w) // PATCH


def patch_rows(img, net_h, net_w, ldk=PATCH_LDK, mean=MEAN, std=STD):
    """img u8 [B, H, W, 3] or f32 [B, 3, H, W] in [0, 1] -> patch rows [B, gh, gw, ldk]: bilinear resize (align_corners=False) to (net_h, net_w), (x - mean) / std,
    the 14 x 14 unfold with column (c 14 + i) 14 + j, zero columns from 588 (mfr_da_patch_rows)"""
    _lib.load(require_gpu=True)
    gh, gw = _grid_of(net_h, net_w)
    assert img.is_cuda and img.dim() == 4
    if img.dtype == torch.uint8:
        assert img.shape[3] == 3
        dtype, (B, H, W) = 0, img.shape[:3]
    else:
        assert img.dtype == torch.float32 and img.shape[1] == 3
        dtype, B, (H, W) = 1, img.shape[0], img.shape[2:]
    img = img.contiguous()
    out = torch.empty(B, gh, gw, int(ldk), dtype=torch.float32, device=img.device)
    _lib.call("mfr_da_patch_rows", img.data_ptr(), dtype, B, H, W, gh, gw, *[float(v) for v in mean], *[float(v) for v in std], out.data_ptr(), int(ldk))
    return out


def patch_rows_tab(img, rows, net_h, net_w, status, ldk=PATCH_LDK, mean=MEAN, std=STD):
    """img u8 [N, H, W, 3], rows i32 [m] on the GPU -> [m, gh, gw, ldk] = patch_rows(img[rows]) without the gather (mfr_da_patch_rows_tab).  status: i32 [1] on the
    GPU, bit 0 is set when a row index is outside [0, N) (that image's rows are zeros); the caller clears it"""
    _lib.load(require_gpu=True)
    gh, gw = _grid_of(net_h, net_w)
    assert img.is_cuda and img.dtype == torch.uint8 and img.dim() == 4 and img.shape[3] == 3 and img.is_contiguous()
    assert status.is_cuda and status.dtype == torch.int32 and status.numel() >= 1
    N, H, W = img.shape[:3]
    m = dpt._i32_table(rows).numel()
    out = torch.empty(m, gh, gw, int(ldk), dtype=torch.float32, device=img.device)
    _lib.call("mfr_da_patch_rows_tab", img.data_ptr(), N, rows.data_ptr(), m, H, W, gh, gw, *[float(v) for v in mean], *[float(v) for v in std], out.data_ptr(),
              int(ldk), status.data_ptr())
    return out


def tokens(x, cls, pos, B):
    """x [B HW, C] (the embedding product's rows; unit column stride, any row stride), cls [C], pos [1 + HW, C] -> token rows [B, 1 + HW, C]"""
    _lib.load(require_gpu=True)
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1 and x.shape[0] % B == 0
    HW, C = x.shape[0] // B, x.shape[1]
    pos = dpt._f32(pos)
    assert pos.shape == (1 + HW, C) and cls.numel() == C
    out = torch.empty(B, 1 + HW, C, dtype=torch.float32, device=x.device)
    _lib.call("mfr_da_tokens", x.data_ptr(), x.stride(0), dpt._f32(cls).reshape(C), pos.data_ptr(), B, C, HW, out.data_ptr(), C)
    return out


def head_tail(f, w, bias, out_h, out_w, metric=True, max_depth=20.0, millimetres=False):
    """f [B, C, Hh, Wh] (ReLU(conv2)'s output), w [C] and bias of conv3 -> metres [B, out_h, out_w] f32 (and u16 millimetres, or None): max_depth sigmoid (metric) or
    ReLU, then F.interpolate(bilinear, align_corners=False) to the output size"""
    _lib.load(require_gpu=True)
    f = dpt._f32(f)
    B, C, Hh, Wh = f.shape
    metres = torch.empty(B, out_h, out_w, dtype=torch.float32, device=f.device)
    mm = torch.empty(B, out_h, out_w, dtype=torch.uint16, device=f.device) if millimetres else None
    _lib.call("mfr_da_head_tail", f.data_ptr(), dpt._f32(w).reshape(C), float(bias), B, C, Hh, Wh, 1 if metric else 0, float(max_depth), int(out_h), int(out_w),
              metres.data_ptr(), mm)
    return metres, mm


def head_tail_rows(f, w, bias, src, dst, metres, status, mm=None, metric=True, max_depth=20.0, quantize=False):
    """plane dst[k] of metres [D, Ho, Wo] (and of mm, or None) <- head_tail(f[src[k]]): nets/dpt.head_tail_rows' tables, quantize and status (mfr_da_head_tail_rows)"""
    _lib.load(require_gpu=True)
    f = dpt._f32(f)
    B, C, Hh, Wh = f.shape
    assert metres.is_cuda and metres.dtype == torch.float32 and metres.dim() == 3 and metres.is_contiguous()
    D, Ho, Wo = metres.shape
    assert mm is None or (mm.is_cuda and mm.dtype == torch.uint16 and mm.shape == metres.shape and mm.is_contiguous())
    assert status.is_cuda and status.dtype == torch.int32 and status.numel() >= 1
    d = dpt._i32_table(src).numel()
    dpt._i32_table(dst, d)
    _lib.call("mfr_da_head_tail_rows", f.data_ptr(), dpt._f32(w).reshape(C), float(bias), B, C, Hh, Wh, 1 if metric else 0, float(max_depth), Ho, Wo,
              src.data_ptr(), dst.data_ptr(), d, metres.data_ptr(), mm, D, 1 if quantize else 0, status.data_ptr())
    return metres


def _pad32(n):
    return -(-int(n) // 32) * 32


def layer_weights(sd, p, device):
    """the packed weights of ViT layer `p` (a `backbone.encoder.layer.N` prefix) for DepthNetBase.vit_layer: q / k / v as one product, LayerScale folded into
    attention.output.dense and mlp.fc2, in the arithmetic `HIP.SPLIT` names now"""
    dev = lambda t: t.float().to(device).contiguous()
    pair = lambda name: (dev(sd[f"{p}.{name}.weight"]), dev(sd[f"{p}.{name}.bias"]))
    wqkv, bqkv = dpt.fold_qkv(sd, p)
    wo, bo = fold_layerscale(sd[f"{p}.attention.output.dense.weight"], sd[f"{p}.attention.output.dense.bias"], sd[f"{p}.layer_scale1.lambda1"])
    w2, b2 = fold_layerscale(sd[f"{p}.mlp.fc2.weight"], sd[f"{p}.mlp.fc2.bias"], sd[f"{p}.layer_scale2.lambda1"])
    return dict(ln1=pair("norm1"), ln2=pair("norm2"), qkv=SplitLinear(dev(wqkv), dev(bqkv)), out=SplitLinear(dev(wo), dev(bo)), fc1=SplitLinear(*pair("mlp.fc1")),
                fc2=SplitLinear(dev(w2), dev(b2)))


class ViTLayers(dpt.DepthNetBase):
    """the encoder alone: what vit_layer needs of a network object (width, heads, the attention variant).  DepthAnythingHIP is one; the tests build a bare one
    to run a single layer at a width or a token count the reduced network does not have"""

    ln_eps = LN_EPS

    def __init__(self, width, heads, device="cuda"):
        _lib.load(require_gpu=True)
        self.arch = dict(VIT_WIDTH=int(width), VIT_HEADS=int(heads))
        self.device = torch.device(device)
        self.split = options.get("SPLIT")
        self.att_variant = 0 if self.split == "f16x2" else 2
        self._n_tok = {}


# ------------------------------------------------------------------------------------------------ the network
class DepthAnythingHIP(ViTLayers):
    """Depth Anything V2, inference only.  state_dict: the keys of `transformers.DepthAnythingForDepthEstimation`; arch: config/depth_anything_arch keys (None:
    ViT-S).  fp32 storage; linear layers in the `HIP.SPLIT` arithmetic, attention in mfr_sg_attention's matching variant, 3x3 / stride 1 layers through
    nets/conv.WinoConv3x3 (the direct kernel under f16x2), the 1x1 layers of the fusion neck and the 3x3 / stride 2 layer through the f16x2 kernels, as DPTHIP.

    Widths that are no multiple of the GEMM's K step of 32 (ViT-S' 48- and 96-channel reassemble layers) are PADDED, not refused: the 1x1 projection gets zero
    output rows up to the next multiple of 32 and the transposed convolution behind it zero K columns, so the padding contributes exact zeros; the 3x3
    kernels take any channel count."""

    def __init__(self, state_dict, device="cuda", arch=None):
        a = check_arch(arch)
        super().__init__(a["VIT_WIDTH"], a["VIT_HEADS"], device)
        self.arch = a
        self.metric, self.max_depth = bool(a["METRIC"]), float(a["MAX_DEPTH"])
        sd = state_dict
        dev = lambda t: t.float().to(self.device).contiguous()
        pair = lambda name: (dev(sd[name + ".weight"]), dev(sd[name + ".bias"]))
        nobias = lambda c: torch.zeros(c, dtype=torch.float32, device=self.device)
        h, e = a["VIT_WIDTH"], "backbone.embeddings"
        w = torch.zeros(h, PATCH_LDK, dtype=torch.float64)
        w[:, :PATCH_K] = sd[f"{e}.patch_embeddings.projection.weight"].double().reshape(h, PATCH_K)
        self.patch = SplitLinear(dev(w), dev(sd[f"{e}.patch_embeddings.projection.bias"]))
        self.cls = dev(sd[f"{e}.cls_token"].reshape(h))
        self.pos = sd[f"{e}.position_embeddings"].detach().float().cpu()
        assert self.pos.shape == (1, 1 + a["POS_GRID"] ** 2, h), "position embeddings do not match POS_GRID"
        self._pos = {}
        self.layers = [layer_weights(sd, f"backbone.encoder.layer.{l}", self.device) for l in range(a["VIT_LAYERS"])]
        self.final_ln = pair("backbone.layernorm")
        rs, ns, f = "neck.reassemble_stage.layers", a["NECK_SIZES"], a["FUSION_WIDTH"]
        self.reassemble_layers = []
        for i in range(4):
            c, cp = ns[i], _pad32(ns[i])
            wp = torch.zeros(cp, h, dtype=torch.float64)
            wp[:c] = sd[f"{rs}.{i}.projection.weight"].double().reshape(c, h)
            bp = torch.zeros(cp, dtype=torch.float64)
            bp[:c] = sd[f"{rs}.{i}.projection.bias"].double()
            R = dict(c=c, proj=SplitLinear(dev(wp), dev(bp)))
            if i < 2:
                s = int(REASSEMBLE_FACTORS[i])
                wt = torch.zeros(c * s * s, cp, dtype=torch.float64)
                wt[:, :c] = dpt.fold_conv_transpose(sd[f"{rs}.{i}.resize.weight"])
                R.update(s=s, up=SplitLinear(dev(wt), None), up_bias=dev(sd[f"{rs}.{i}.resize.bias"]))
            elif i == 3:
                R["down"] = IgemmConv(*pair(f"{rs}.3.resize"), stride=2, padding=1)
            self.reassemble_layers.append(R)
        self.neck_convs = [WinoConv3x3(dev(sd[f"neck.convs.{i}.weight"]), nobias(f)) for i in range(4)]
        self.fusion = []
        for i in range(4):
            p = f"neck.fusion_stage.layers.{i}"
            c3 = lambda n: WinoConv3x3(*pair(f"{p}.{n}"))
            self.fusion.append(dict(r1=(c3("residual_layer1.convolution1"), c3("residual_layer1.convolution2")),
                                    r2=(c3("residual_layer2.convolution1"), c3("residual_layer2.convolution2")),
                                    proj=dpt.PadIgemmConv(*pair(f"{p}.projection"))))
        self.conv1 = WinoConv3x3(*pair("head.conv1"))
        self.conv2 = WinoConv3x3(*pair("head.conv2"))
        self.conv3_w = dev(sd["head.conv3.weight"].reshape(-1))
        self.conv3_b = float(sd["head.conv3.bias"].reshape(-1)[0])
        assert self.conv3_w.numel() == a["HEAD_WIDTH"]

    # ---- stages ----
    def position_embeddings(self, gh, gw):
        if (gh, gw) not in self._pos:
            self._pos[(gh, gw)] = resize_position_embeddings(self.pos, gh, gw).to(self.device).contiguous()
        return self._pos[(gh, gw)]

    def embed(self, rows):
        """patch rows [B, gh, gw, ldk] -> the patch embeddings [B gh gw, h]: ONE product over all images"""
        B, gh, gw, ldk = rows.shape
        return self.patch(rows.view(B * gh * gw, ldk))

    def tokenize(self, rows):
        """patch rows [B, gh, gw, ldk] -> token rows [B, 1 + gh gw, h]: embedding product, then cls row and position embeddings in a second pass"""
        B, gh, gw, _ = rows.shape
        return tokens(self.embed(rows), self.cls, self.position_embeddings(gh, gw), B)

    def tap(self, state):
        """a tapped hidden state [B, T, h] -> the backbone's shared final LayerNorm of it [B, T, h] (what the reassemble stage reads; the cls row is dropped there)"""
        B, T, h = state.shape
        return dpt.layernorm(state.reshape(B * T, h), *self.final_ln, eps=LN_EPS).view(B, T, h)

    def tap_map(self, state, gh, gw):
        """the same as the NCHW map the module's reassemble layer takes: tokens_inverse(skip=1) of tap()"""
        return dpt.tokens_inverse(self.tap(state), gh, gw, skip=1)

    def encoder(self, tok):
        """token rows [B, T, h] -> the four tapped states behind the final LayerNorm"""
        B, T, h = tok.shape
        x, taps = tok.reshape(B * T, h).clone(), {}
        for l, L in enumerate(self.layers[:max(self.arch["TAPS"]) + 1]):
            self.vit_layer(L, x, B, T)
            if l in self.arch["TAPS"]:
                taps[l] = self.tap(x.view(B, T, h))
        return [taps[l] for l in self.arch["TAPS"]]

    def reassemble(self, i, normed, gh, gw):
        """tap i as token rows [B, 1 + gh gw, h] (tap()'s output; row 0 of each image, the cls row, is not used) -> the reassembled map: 1x1 projection as a
        product over the rows, then x4 / x2 ConvTranspose2d(k = s) as GEMM + mfr_dpt_shuffle (i = 0, 1), nothing (2), or 3x3 / stride 2 / pad 1 (3).  The
        products run over every row, the cls rows included (1 in 1 + gh gw): their rows are evenly spaced, the patch rows alone are not"""
        R = self.reassemble_layers[i]
        B, T, h = normed.shape
        assert T == 1 + gh * gw
        c = R["c"]
        y = R["proj"](normed.reshape(B * T, h))                              # [B T, cp]
        if i < 2:
            s = R["s"]
            g = R["up"](y).view(B, T, c * s * s)
            out = torch.empty(B, c, gh * s, gw * s, dtype=torch.float32, device=y.device)
            for b in range(B):                                                 # the shuffle indexes rows (b H + h) W + w: one image at a time skips its cls row
                dpt.shuffle(g[b, 1:], R["up_bias"], 1, c, gh, gw, s, out=out[b:b + 1])
            return out
        m = dpt.tokens_inverse(y.view(B, T, -1)[:, :, :c], gh, gw, skip=1)
        return R["down"](m) if i == 3 else m

    def neck(self, feats):
        """four reassembled maps (finest first) -> the last fused map [B, F, 8 gh, 8 gw].  Layers 0..2 up-sample to the NEXT map's size (3 -> 5 on an odd
        grid: not x2), the last one x2"""
        f = [c(x) for c, x in zip(self.neck_convs, feats)]
        y = self.fusion_layer(self.fusion[0], f[3], size=f[2].shape[2:])
        for i in (1, 2, 3):
            y = self.fusion_layer(self.fusion[i], y, f[3 - i], size=f[2 - i].shape[2:] if i < 3 else None)
        return y

    def head_features(self, fused, gh, gw):
        """conv1 (3x3), bilinear (align_corners=True) to (14 gh, 14 gw), conv2 (3x3) + ReLU -> [B, HEAD_WIDTH, 14 gh, 14 gw]"""
        return self.conv2(dpt.upsample(self.conv1(fused), (PATCH * gh, PATCH * gw)), act=1)

    def features(self, rows):
        """patch rows [B, gh, gw, ldk] (prep's output) -> the head's last feature map"""
        B, gh, gw, _ = rows.shape
        taps = self.encoder(self.tokenize(rows))
        return self.head_features(self.neck([self.reassemble(i, t, gh, gw) for i, t in enumerate(taps)]), gh, gw)

    def __call__(self, img, net_hw, out_hw=None, millimetres=False):
        """img u8 [B, H, W, 3] or f32 [B, 3, H, W] in [0, 1] -> (metres f32 [B, H, W], u16 millimetres or None) at out_hw (None: the image's size)"""
        return self.depth(img, net_hw, out_hw, millimetres=millimetres)

    # ---- the seam (nets/dpt.DepthNetBase) ----
    def prep(self, img, net_hw):
        return patch_rows(img, int(net_hw[0]), int(net_hw[1]))

    def prep_rows(self, img, rows, net_hw, status):
        return patch_rows_tab(img, rows, int(net_hw[0]), int(net_hw[1]), status)

    def tail(self, f, out_hw, millimetres=False):
        return head_tail(f, self.conv3_w, self.conv3_b, int(out_hw[0]), int(out_hw[1]), metric=self.metric, max_depth=self.max_depth, millimetres=millimetres)

    def tail_rows(self, f, src, dst, metres, status, quantize=False):
        return head_tail_rows(f, self.conv3_w, self.conv3_b, src, dst, metres, status, metric=self.metric, max_depth=self.max_depth, quantize=quantize)


# ------------------------------------------------------------------------------------------------ the config's stage
def arch_from_cfg(cfg):
    """the architecture dict of a config's DA node: the DA.ENCODER preset, DA.ARCH's keys over it, DA.MAX_DEPTH / DA.METRIC over both"""
    node = cfg.DA
    if node.ENCODER not in PRESETS:
        raise ValueError(f"DA.ENCODER = {node.ENCODER!r}: one of {sorted(PRESETS)}")
    arch = dict(PRESETS[node.ENCODER])
    arch.update({k: (tuple(v) if isinstance(v, list) else v) for k, v in dict(node.ARCH).items() if v is not None})
    arch["MAX_DEPTH"], arch["METRIC"] = float(node.MAX_DEPTH), bool(node.METRIC)
    return check_arch(arch)


def check_cfg(cfg):
    """the DA node of a config, checked: network sizes are multiples of 14, the architecture is one the kernels have"""
    if "DA" not in cfg:
        raise ValueError("DPT.NETWORK 'depth_anything' needs the config's DA node")
    node = cfg.DA
    for name in ("NET_HEIGHT", "NET_WIDTH"):
        v = node[name]
        if isinstance(v, bool) or not isinstance(v, int) or v < PATCH or v % PATCH:
            raise ValueError(f"DA.NET_HEIGHT x NET_WIDTH = {node.NET_HEIGHT} x {node.NET_WIDTH}: both must be multiples of {PATCH}")
    arch_from_cfg(cfg)
    return node


def network_from_cfg(cfg, device="cuda"):
    """-> (maker, net_hw) for nets/dpt.build_network: DA.WEIGHTS (a state dict with the `transformers` names; convert an authors' checkpoint with from_upstream
    first), or the synthetic weights when the config allows them"""
    from . import weights as WT
    node = check_cfg(cfg)
    arch = arch_from_cfg(cfg)
    sd = WT.from_cfg("DepthAnything", cfg, node.WEIGHTS, lambda: WT.depth_anything_state_dict(int(node.SYNTHETIC_SEED), arch=arch))
    return (lambda: DepthAnythingHIP(sd, device, arch=arch)), (int(node.NET_HEIGHT), int(node.NET_WIDTH))
