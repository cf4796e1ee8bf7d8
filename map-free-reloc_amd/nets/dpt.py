"""DPT-Hybrid monocular depth (Ranftl et al., ICCV 2021): architecture table, host-side weight folding and the launches of csrc/dpt.hip.

The architecture of record is `transformers.DPTForDepthEstimation` with is_hybrid=True, and the state-dict keys are its keys (`dpt.embeddings.backbone.bit.*`,
`dpt.encoder.layer.{i}.*`, `neck.*`, `head.head.*`); the product never imports that package (tests/dpt_ref.py drives it as the oracle).

What is here:
  * ARCH / check_arch      the architecture as a small dict (DPT-Hybrid's values as defaults); head dimension 64 only -- what mfr_sg_attention has;
  * fold_*                 pure float64 host code, run once per weight set: BiT's weight standardisation into plain conv weights, q / k / v into one product,
                           the readout projection Linear(2h -> h) on [token ; cls] into W_a token + (W_b cls + b), ConvTranspose2d(k = s) into a GEMM with
                           N = C s^2, and the position embeddings resized to a token grid (cached per grid shape);
  * the stage launches     prep, groupnorm, maxpool3s2, layernorm, bias_gelu, tokens, tokens_inverse, shuffle, head_tail (include/mfr_hip.h mfr_dpt_*): fp32 tensors
                           on the GPU in, fp32 tensors out, no fallback -- a missing kernel or a refused argument raises.
  * DPTHIP                 the network, inference only: fp32 storage; linear layers in the `HIP.SPLIT` arithmetic (nets/linear.SplitLinear), attention in
                           mfr_sg_attention's matching variant, 3x3 / stride 1 / pad 1 layers through nets/conv.WinoConv3x3 (the direct kernel under f16x2), every
                           other convolution through the implicit-GEMM kernel (f16x2, mfr_conv_igemm_f16x2_pad: BiT's TF-"SAME" padding is asymmetric).  Each stage
                           is a method, which is what the stage-level tests call.
  * DepthNetBase           what DPTHIP shares with nets/depth_anything.DepthAnythingHIP (the ViT layer, the fusion layer, the residual unit) and the seam the two
                           classes below drive either network through: prep / prep_rows, features, tail / tail_rows; build_network builds the configured one
                           (DPT.NETWORK 'hybrid' | 'depth_anything');
  * DepthEstimator         the config's stage (DPT.*) for compute_depth and the per-pair plugin: images in, maps out, the range guard's re-run taken here;
  * FusedDepthStage        DPT.SOURCE 'online' on the batched route (pipeline.FusedPosePipeline): the maps the pose solver reads, from the batch's colour bytes --
                           only the views it reads, a shared reference view once, through the row-table ends prep_rows / head_tail_rows."""
import torch

from .. import _lib, options
from ..config.dpt_arch import ARCH              # DPT-Hybrid's values (config/dpt_arch.py: shared with the config's DPT.ARCH node)
from .conv import IgemmConv, WinoConv3x3
from .linear import SplitLinear

HEAD_DIM = 64                       # mfr_sg_attention's head width
NETWORKS = ("hybrid", "depth_anything")     # DPT.NETWORK: DPTHIP (this file) | nets/depth_anything.DepthAnythingHIP
STEM_EPS, BOTTLENECK_EPS = 1e-8, 1e-8   # weight standardisation: BitEmbeddings' conv and the bottlenecks' convs
GN_EPS, LN_EPS = 1e-5, 1e-12        # BitGroupNormActivation / the ViT's layer_norm_eps


def check_arch(arch=None):
    """the architecture dict with the defaults filled in; refuses what the kernels do not have"""
    a = dict(ARCH)
    unknown = set(arch or {}) - set(a)
    if unknown:
        raise ValueError(f"DPT: unknown architecture keys {sorted(unknown)}")
    a.update(arch or {})
    if a["VIT_WIDTH"] != HEAD_DIM * a["VIT_HEADS"]:
        raise ValueError(f"DPT: head dimension {a['VIT_WIDTH']}/{a['VIT_HEADS']} is not {HEAD_DIM}, the only width the attention kernel has")
    if a["VIT_WIDTH"] % 64 or a["VIT_WIDTH"] > 1024:
        raise ValueError("DPT: ViT width must be a multiple of 64, at most 1024 (mfr_dpt_layernorm)")
    if len(a["BIT_DEPTHS"]) != 3 or len(a["BIT_HIDDEN_SIZES"]) != 3 or len(a["NECK_SIZES"]) != 4 or len(a["TAPS"]) != 4:
        raise ValueError("DPT: the hybrid has three BiT stages, four neck sizes and four taps")
    if any(c % a["NUM_GROUPS"] for c in (a["BIT_EMBEDDING_SIZE"],) + tuple(a["BIT_HIDDEN_SIZES"])):
        raise ValueError("DPT: every BiT width must be a multiple of the group count")
    if max(a["TAPS"]) >= a["VIT_LAYERS"] or a["PATCH"] != 16:
        raise ValueError("DPT: taps must be ViT layers; patch size 16 only")
    return a


# ------------------------------------------------------------------------------------------------ host-side folding (float64)
def fold_weight_standardisation(w, eps):
    """BiT's WeightStandardizedConv2d as a plain conv weight: per output filter (w - mean) / sqrt(var + eps), biased variance over (Cin, kh, kw) -- what
    F.batch_norm(training=True) does to the [1, Cout, -1] view of the weight at every forward pass"""
    w64 = w.detach().double()
    flat = w64.reshape(w64.shape[0], -1)
    mean = flat.mean(dim=1, keepdim=True)
    var = (flat - mean).pow(2).mean(dim=1, keepdim=True)
    return ((flat - mean) / torch.sqrt(var + float(eps))).reshape(w64.shape)


def fold_qkv(sd, prefix):
    """-> (W [3h, h], b [3h]) from `prefix`.attention.attention.{query,key,value}: one product for the three"""
    ws = [sd[f"{prefix}.attention.attention.{n}.weight"].double() for n in ("query", "key", "value")]
    bs = [sd[f"{prefix}.attention.attention.{n}.bias"].double() for n in ("query", "key", "value")]
    return torch.cat(ws, 0), torch.cat(bs, 0)


def fold_readout(weight, bias):
    """Linear(2h -> h) on [token ; cls] -> (W_a [h, h], W_b [h, h], b [h]):  W [token ; cls] + b = W_a token + (W_b cls + b); the bracket is one vector per image"""
    w = weight.detach().double()
    h = w.shape[0]
    assert w.shape == (h, 2 * h)
    return w[:, :h].contiguous(), w[:, h:].contiguous(), bias.detach().double()


def readout_image_bias(w_b, b, cls):
    """cls [B, h] -> the per-image bias W_b cls + b [B, h] (float64 in, float64 out)"""
    return cls.double() @ w_b.t() + b


def fold_conv_transpose(weight):
    """ConvTranspose2d(C_in, C_out, kernel = stride = s).weight [C_in, C_out, s, s] -> the GEMM's W [N = C_out s^2, K = C_in] with column n = (co s + i) s + j:
    row (b, h, w) of x W^T holds the s x s output patch of every channel, which mfr_dpt_shuffle stores (and adds the bias to)"""
    w = weight.detach().double()
    ci, co, s, s2 = w.shape
    assert s == s2 and s in (2, 4)
    return w.reshape(ci, co * s * s).t().contiguous()


def from_upstream(sd):
    """UNPINNED.  A DPT-Hybrid checkpoint with the parameter names of the authors' repository (isl-org/DPT: `pretrained.model.*`, `pretrained.act_postprocess*`,
    `scratch.*`) -> the names used here.  The renames follow the published architecture and the public conversion of these checkpoints to `transformers`; no
    such file exists offline, so nothing pins this against a real checkpoint -- only the round trip through the inverse map is tested (tests/test_dpt_host.py).
    attn.qkv is split into query / key / value; the semantic-segmentation heads (`auxlayer`) and anything else unknown raise."""
    import re
    out = {}
    vit = "pretrained.model."
    for k, v in sd.items():
        n = None
        if k.startswith(vit + "patch_embed.backbone."):
            r = k[len(vit + "patch_embed.backbone."):]
            r = r.replace("stem.conv.", "embedder.convolution.").replace("stem.norm.", "embedder.norm.")
            r = re.sub(r"^stages\.(\d+)\.blocks\.(\d+)\.", r"encoder.stages.\1.layers.\2.", r)
            n = "dpt.embeddings.backbone.bit." + r
        elif k.startswith(vit + "patch_embed.proj."):
            n = "dpt.embeddings.projection." + k.rsplit(".", 1)[1]
        elif k == vit + "cls_token":
            n = "dpt.embeddings.cls_token"
        elif k == vit + "pos_embed":
            n = "dpt.embeddings.position_embeddings"
        elif k.startswith(vit + "norm."):
            n = "dpt.layernorm." + k.rsplit(".", 1)[1]
        elif k.startswith(vit + "blocks."):
            m = re.match(r"blocks\.(\d+)\.(.+)\.(weight|bias)$", k[len(vit):])
            if m:
                i, what, wb = m.groups()
                base = f"dpt.encoder.layer.{i}."
                if what == "attn.qkv":
                    h = v.shape[0] // 3
                    for j, name in enumerate(("query", "key", "value")):
                        out[f"{base}attention.attention.{name}.{wb}"] = v[j * h:(j + 1) * h].clone()
                    continue
                table = {"norm1": "layernorm_before", "norm2": "layernorm_after", "attn.proj": "attention.output.dense", "mlp.fc1": "intermediate.dense",
                         "mlp.fc2": "output.dense"}
                if what in table:
                    n = f"{base}{table[what]}.{wb}"
        elif k.startswith("pretrained.act_postprocess"):
            m = re.match(r"pretrained\.act_postprocess([34])\.(0\.project\.0|3|4)\.(weight|bias)$", k)
            if m:
                stage, what, wb = int(m.group(1)) - 1, m.group(2), m.group(3)
                if what == "0.project.0":
                    n = f"neck.reassemble_stage.readout_projects.{stage}.0.{wb}"
                elif what == "3":
                    n = f"neck.reassemble_stage.layers.{stage}.projection.{wb}"
                elif stage == 3:
                    n = f"neck.reassemble_stage.layers.3.resize.{wb}"
        elif k.startswith("scratch.layer"):
            m = re.match(r"scratch\.layer([1-4])_rn\.weight$", k)
            if m:
                n = f"neck.convs.{int(m.group(1)) - 1}.weight"
        elif k.startswith("scratch.refinenet"):
            m = re.match(r"scratch\.refinenet([1-4])\.(out_conv|resConfUnit[12]\.conv[12])\.(weight|bias)$", k)
            if m:
                what = m.group(2).replace("out_conv", "projection").replace("resConfUnit", "residual_layer").replace("conv", "convolution")
                n = f"neck.fusion_stage.layers.{4 - int(m.group(1))}.{what}.{m.group(3)}"
        elif k.startswith("scratch.output_conv."):
            m = re.match(r"scratch\.output_conv\.([024])\.(weight|bias)$", k)
            if m:
                n = f"head.head.{m.group(1)}.{m.group(2)}"
        if n is None:
            raise KeyError(f"DPT.from_upstream: no place for {k!r}")
        out[n] = v
    return out


def resize_position_embeddings(pos, gh, gw):
    """pos [1, 1 + g^2, h] -> [1 + gh gw, h] float64: the grid rows resized with F.interpolate(bilinear, align_corners=False), the cls row kept.  Host code;
    DPTHIP.position_embeddings keeps the result per grid shape"""
    p = pos.detach().double().cpu()
    n, h = p.shape[1] - 1, p.shape[2]
    g = int(round(n ** 0.5))
    assert g * g == n, "position embeddings must come from a square grid"
    grid = p[0, 1:].reshape(1, g, g, h).permute(0, 3, 1, 2)
    grid = torch.nn.functional.interpolate(grid, size=(int(gh), int(gw)), mode="bilinear", align_corners=False)
    return torch.cat([p[0, :1], grid.permute(0, 2, 3, 1).reshape(int(gh) * int(gw), h)], 0).contiguous()


def same_padding(n, kernel, stride):
    """TF-"SAME" (lo, hi) padding of one axis: BiT's DynamicPad2d.  Even n: (2, 3) for the 7x7 / 2 stem, (0, 1) for the 3x3 / 2 pool and convs"""
    total = max((-(-n // stride) - 1) * stride + kernel - n, 0)
    return total // 2, total - total // 2


# ------------------------------------------------------------------------------------------------ the launches
def _f32(t):
    assert t.is_cuda and t.dtype == torch.float32, "DPT kernels take float32 tensors on the GPU"
    return t.contiguous()


def prep(img, net_h, net_w):
    """img u8 [B, H, W, 3] or f32 [B, 3, H, W] in [0, 1] -> [B, 3, net_h, net_w]: bilinear resize (align_corners=False) and (x - 0.5) / 0.5"""
    _lib.load(require_gpu=True)
    assert img.is_cuda and img.dim() == 4
    if img.dtype == torch.uint8:
        assert img.shape[3] == 3
        dtype, (B, H, W) = 0, img.shape[:3]
    else:
        assert img.dtype == torch.float32 and img.shape[1] == 3
        dtype, B, (H, W) = 1, img.shape[0], img.shape[2:]
    img = img.contiguous()
    out = torch.empty(B, 3, net_h, net_w, dtype=torch.float32, device=img.device)
    _lib.call("mfr_dpt_prep", img.data_ptr(), dtype, B, H, W, out.data_ptr(), int(net_h), int(net_w))
    return out


def groupnorm(x, gamma, beta, groups, eps=GN_EPS, relu=False, residual=None):
    """GroupNorm over NCHW [+ residual] [ReLU]"""
    _lib.load(require_gpu=True)
    x = _f32(x)
    B, C, H, W = x.shape
    res = None if residual is None else _f32(residual)
    assert res is None or res.shape == x.shape
    y = torch.empty_like(x)
    _lib.call("mfr_dpt_groupnorm", x.data_ptr(), _f32(gamma), _f32(beta), res, B, C, H * W, int(groups), float(eps), 1 if relu else 0, y.data_ptr())
    return y


def maxpool3s2(x, pad_h=None, pad_w=None):
    """3x3 / 2 max-pool behind a zero padding of (lo, hi) per axis; None: TF-"SAME" for that axis"""
    _lib.load(require_gpu=True)
    x = _f32(x)
    B, C, H, W = x.shape
    (pt, pb), (pl, pr) = pad_h or same_padding(H, 3, 2), pad_w or same_padding(W, 3, 2)
    Ho, Wo = (H + pt + pb - 3) // 2 + 1, (W + pl + pr - 3) // 2 + 1
    y = torch.empty(B, C, max(Ho, 0), max(Wo, 0), dtype=torch.float32, device=x.device)
    _lib.call("mfr_dpt_maxpool3s2", x.data_ptr(), B * C, H, W, int(pt), int(pb), int(pl), int(pr), y.data_ptr())
    return y


def layernorm(x, gamma, beta, eps=LN_EPS, residual=None, out=None):
    """rows of x [M, C] (unit column stride, any row stride), C a multiple of 64: out = [residual +] LayerNorm(x) gamma + beta"""
    _lib.load(require_gpu=True)
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
    M, C = x.shape
    if out is None:
        out = torch.empty(M, C, dtype=torch.float32, device=x.device)
    assert out.shape == (M, C) and out.stride(1) == 1 and (residual is None or (residual.shape == (M, C) and residual.stride(1) == 1))
    _lib.call("mfr_dpt_layernorm", x.data_ptr(), x.stride(0), _f32(gamma), _f32(beta), None if residual is None else residual.data_ptr(),
              0 if residual is None else residual.stride(0), M, C, float(eps), out.data_ptr(), out.stride(0))
    return out


def bias_gelu(x, bias=None):
    """x [M, N] <- GELU_erf(x + bias), in place"""
    _lib.load(require_gpu=True)
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
    _lib.call("mfr_dpt_bias_gelu", x.data_ptr(), x.stride(0), x.shape[0], x.shape[1], None if bias is None else _f32(bias))
    return x


def tokens(x, cls, pos):
    """x [B, C, gh, gw] (the patch projection's output), cls [C], pos [1 + gh gw, C] -> token rows [B, 1 + gh gw, C]"""
    _lib.load(require_gpu=True)
    x = _f32(x)
    B, C, gh, gw = x.shape
    pos = _f32(pos)
    assert pos.shape == (1 + gh * gw, C) and cls.numel() == C
    out = torch.empty(B, 1 + gh * gw, C, dtype=torch.float32, device=x.device)
    _lib.call("mfr_dpt_tokens", x.data_ptr(), _f32(cls).reshape(C), pos.data_ptr(), B, C, gh * gw, out.data_ptr(), C)
    return out


def tokens_inverse(rows, gh, gw, bias_img=None, gelu=False, skip=1):
    """rows [B, skip + gh gw, C] -> NCHW [B, C, gh, gw] = act(rows without the first `skip` + bias_img [B, C])"""
    _lib.load(require_gpu=True)
    assert rows.is_cuda and rows.dtype == torch.float32 and rows.dim() == 3 and rows.stride(2) == 1
    B, T, C = rows.shape
    assert T == skip + gh * gw and (bias_img is None or bias_img.shape == (B, C))
    out = torch.empty(B, C, gh, gw, dtype=torch.float32, device=rows.device)
    _lib.call("mfr_dpt_tokens_inverse", rows.data_ptr(), rows.stride(1), rows.stride(0), int(skip), None if bias_img is None else _f32(bias_img),
              1 if gelu else 0, B, C, gh * gw, out.data_ptr())
    return out


def shuffle(g, bias, B, C, H, W, s, out=None):
    """g [B H W, C s^2] (the GEMM of fold_conv_transpose) -> ConvTranspose2d's output [B, C, H s, W s] (`out`: written there, contiguous)"""
    _lib.load(require_gpu=True)
    assert g.is_cuda and g.dtype == torch.float32 and g.shape == (B * H * W, C * s * s) and g.stride(1) == 1
    if out is None:
        out = torch.empty(B, C, H * s, W * s, dtype=torch.float32, device=g.device)
    assert out.shape == (B, C, H * s, W * s) and out.dtype == torch.float32 and out.is_contiguous()
    _lib.call("mfr_dpt_shuffle", g.data_ptr(), g.stride(0), None if bias is None else _f32(bias), B, C, H, W, int(s), out.data_ptr())
    return out


def head_tail(f, w, bias, out_h, out_w, invert=False, scale=1.0, shift=0.0, millimetres=False):
    """f [B, C, Hh, Wh] (the head's ReLU(conv3x3) output), w [C] and bias of the 1x1 layer -> metres [B, out_h, out_w] f32 (and u16 millimetres, or None)"""
    _lib.load(require_gpu=True)
    f = _f32(f)
    B, C, Hh, Wh = f.shape
    metres = torch.empty(B, out_h, out_w, dtype=torch.float32, device=f.device)
    mm = torch.empty(B, out_h, out_w, dtype=torch.uint16, device=f.device) if millimetres else None
    _lib.call("mfr_dpt_head_tail", f.data_ptr(), _f32(w).reshape(C), float(bias), B, C, Hh, Wh, 1 if invert else 0, float(scale), float(shift),
              int(out_h), int(out_w), metres.data_ptr(), mm)
    return metres, mm


def _i32_table(t, n=None):
    assert t.is_cuda and t.dtype == torch.int32 and t.dim() == 1 and t.is_contiguous() and (n is None or t.numel() == n), "row tables are int32 [n] on the GPU"
    return t


def prep_rows(img, rows, net_h, net_w, status):
    """img u8 [N, H, W, 3], rows i32 [m] on the GPU -> [m, 3, net_h, net_w] = prep(img[rows]) without the gather (mfr_dpt_prep_rows).  status: i32 [1] on the GPU,
    bit 0 is set when a row index is outside [0, N) (that image is zeros); the caller clears it"""
    _lib.load(require_gpu=True)
    assert img.is_cuda and img.dtype == torch.uint8 and img.dim() == 4 and img.shape[3] == 3 and img.is_contiguous()
    assert status.is_cuda and status.dtype == torch.int32 and status.numel() >= 1
    N, H, W = img.shape[:3]
    m = _i32_table(rows).numel()
    out = torch.empty(m, 3, net_h, net_w, dtype=torch.float32, device=img.device)
    _lib.call("mfr_dpt_prep_rows", img.data_ptr(), N, rows.data_ptr(), m, H, W, out.data_ptr(), int(net_h), int(net_w), status.data_ptr())
    return out


def head_tail_rows(f, w, bias, src, dst, metres, status, mm=None, invert=False, scale=1.0, shift=0.0, quantize=False):
    """plane dst[k] of metres [D, Ho, Wo] f32 (and of mm, u16 [D, Ho, Wo] or None) <- head_tail(f[src[k]]), for every entry of the i32 tables src / dst [d] on the
    GPU (mfr_dpt_head_tail_rows): one feature image may feed several planes, planes not listed keep their contents.  quantize: the metres written are
    millimetres_to_metres(mm).  status as in prep_rows"""
    _lib.load(require_gpu=True)
    f = _f32(f)
    B, C, Hh, Wh = f.shape
    assert metres.is_cuda and metres.dtype == torch.float32 and metres.dim() == 3 and metres.is_contiguous()
    D, Ho, Wo = metres.shape
    assert mm is None or (mm.is_cuda and mm.dtype == torch.uint16 and mm.shape == metres.shape and mm.is_contiguous())
    assert status.is_cuda and status.dtype == torch.int32 and status.numel() >= 1
    d = _i32_table(src).numel()
    _i32_table(dst, d)
    _lib.call("mfr_dpt_head_tail_rows", f.data_ptr(), _f32(w).reshape(C), float(bias), B, C, Hh, Wh, 1 if invert else 0, float(scale), float(shift), Ho, Wo,
              src.data_ptr(), dst.data_ptr(), d, metres.data_ptr(), mm, D, 1 if quantize else 0, status.data_ptr())
    return metres


def add_relu(a, b=None, want_sum=True):
    """-> (a + b, relu(a + b)) in one pass (b None: (a, relu(a)))"""
    _lib.load(require_gpu=True)
    a = _f32(a)
    b = None if b is None else _f32(b)
    assert b is None or b.shape == a.shape
    s = torch.empty_like(a) if (want_sum and b is not None) else None
    r = torch.empty_like(a)
    _lib.call("mfr_dpt_add_relu", a.data_ptr(), b, a.numel(), s, r.data_ptr())
    return (a if b is None else s), r


# ------------------------------------------------------------------------------------------------ the network
class PadIgemmConv(IgemmConv):
    """IgemmConv behind an explicit (lo, hi) zero padding, the same on both axes (mfr_conv_igemm_f16x2_pad)"""

    def __init__(self, weight, bias, stride=1):
        super().__init__(weight, bias, stride=stride, padding=0)

    def __call__(self, x, pad=(0, 0), relu=False):
        x = _f32(x)
        B, C, H, W = x.shape
        assert C == self.ci
        lo, hi = int(pad[0]), int(pad[1])
        Ho, Wo = (H + lo + hi - self.kh) // self.stride + 1, (W + lo + hi - self.kw) // self.stride + 1
        y = torch.empty(B, self.co, Ho, Wo, dtype=torch.float32, device=x.device)
        _lib.call("mfr_conv_igemm_f16x2_pad", x.data_ptr(), self.packed, self.b, y.data_ptr(), B, C, H, W, self.co, self.kh, self.kw, self.stride,
                  lo, hi, 1 if relu else 0)
        return y


def upsample(x, size):
    """F.interpolate(x, size=size, mode='bilinear', align_corners=True) (mfr_upsample_bilinear)"""
    x = _f32(x)
    B, C, H, W = x.shape
    Ho, Wo = int(size[0]), int(size[1])
    y = torch.empty(B, C, Ho, Wo, dtype=torch.float32, device=x.device)
    _lib.call("mfr_upsample_bilinear", x.data_ptr(), y.data_ptr(), B * C, H, W, Ho, Wo, 0)
    return y


def upsample2x(x):
    """F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=True)"""
    return upsample(x, (2 * x.shape[2], 2 * x.shape[3]))


class DepthNetBase:
    """What the depth networks share (DPTHIP here, nets/depth_anything.DepthAnythingHIP): the pre-norm ViT layer on SplitLinear and mfr_sg_attention, the
    fusion neck's layer and its residual unit, and the SEAM through which DepthEstimator and FusedDepthStage drive either network:
        prep / prep_rows     images (or scattered rows of a u8 batch) -> the network's input
        features             the network's input -> the head's last feature map
        tail / tail_rows     that map -> metres (and millimetres) at the output size, with the network's own last-layer weights and output convention
    A subclass sets arch (VIT_WIDTH, VIT_HEADS), device, att_variant, ln_eps, _n_tok = {} and implements the five."""

    ln_eps = LN_EPS

    def attention(self, qkv, B, T, out):
        h = self.arch["VIT_WIDTH"]
        if (B, T) not in self._n_tok:                                  # the token counts of the attention kernel's mask: built once per (B, T)
            self._n_tok[(B, T)] = torch.full((B,), T, dtype=torch.int32, device=self.device)
        n_tok = self._n_tok[(B, T)]
        base = qkv.data_ptr()
        _lib.call("mfr_sg_attention_variant", base, base + h * 4, base + 2 * h * 4, 3 * h, B, T, self.arch["VIT_HEADS"], n_tok.data_ptr(), 0, out.data_ptr(), h,
                  self.att_variant)
        return out

    def vit_layer(self, L, x, B, T):
        """one pre-norm layer on x [B T, h], in place (a LayerScale, where the network has one, is folded into L['out'] and L['fc2'])"""
        y = layernorm(x, *L["ln1"], eps=self.ln_eps)
        qkv = L["qkv"](y)
        self.attention(qkv, B, T, y)
        L["out"](y, out=x, accumulate=True)
        y = layernorm(x, *L["ln2"], eps=self.ln_eps, out=y)
        hid = bias_gelu(L["fc1"](y))
        L["fc2"](hid, out=x, accumulate=True)
        return x

    def residual_unit(self, convs, x, rx):
        """the pre-activation residual unit: conv2(relu(conv1(relu(x)))) + x; rx = relu(x) comes from the launch that produced x"""
        return convs[1](convs[0](rx, act=1), residual=x)

    def fusion_layer(self, F, hidden, residual=None, size=None):
        """size: the map the layer up-samples to (align_corners=True); None: x2"""
        if residual is not None:
            _, rr = add_relu(residual)
            hidden, rh = add_relu(hidden, self.residual_unit(F["r1"], residual, rr))
        else:
            _, rh = add_relu(hidden)
        y = self.residual_unit(F["r2"], hidden, rh)
        return F["proj"](upsample(y, (2 * y.shape[2], 2 * y.shape[3]) if size is None else size))

    def depth(self, img, net_hw, out_hw=None, millimetres=False):
        """img u8 [B, H, W, 3] or f32 [B, 3, H, W] in [0, 1] -> (metres f32 [B, *out_hw], u16 millimetres or None); out_hw None: the image's size"""
        if out_hw is None:
            out_hw = tuple(img.shape[1:3]) if img.dtype == torch.uint8 else tuple(img.shape[2:4])
        return self.tail(self.features(self.prep(img, net_hw)), out_hw, millimetres=millimetres)


class DPTHIP(DepthNetBase):
    """DPT-Hybrid depth, inference only.  state_dict: the keys of `transformers.DPTForDepthEstimation`; arch: ARCH keys (None: DPT-Hybrid)."""

    def __init__(self, state_dict, device="cuda", arch=None):
        _lib.load(require_gpu=True)
        self.arch = a = check_arch(arch)
        self.device = torch.device(device)
        self.split = options.get("SPLIT")
        self.att_variant = 0 if self.split == "f16x2" else 2
        self.convention = dict(invert=False, scale=1.0, shift=0.0)      # the output convention tail / tail_rows apply (build_network: the config's)
        sd = state_dict
        dev = lambda t: t.float().to(self.device).contiguous()
        ws = lambda name, eps: dev(fold_weight_standardisation(sd[name + ".weight"], eps))
        gn = lambda name: (dev(sd[name + ".weight"]), dev(sd[name + ".bias"]))
        nobias = lambda c: torch.zeros(c, dtype=torch.float32, device=self.device)
        bit = "dpt.embeddings.backbone.bit"
        self.stem = PadIgemmConv(ws(f"{bit}.embedder.convolution", STEM_EPS), None, stride=2)
        self.stem_norm = gn(f"{bit}.embedder.norm")
        self.stages = []
        for s, depth in enumerate(a["BIT_DEPTHS"]):
            layers = []
            for l in range(depth):
                p = f"{bit}.encoder.stages.{s}.layers.{l}"
                stride = 2 if (l == 0 and s > 0) else 1
                L = dict(stride=stride, conv1=PadIgemmConv(ws(f"{p}.conv1", BOTTLENECK_EPS), None), norm1=gn(f"{p}.norm1"), norm2=gn(f"{p}.norm2"),
                         conv3=PadIgemmConv(ws(f"{p}.conv3", BOTTLENECK_EPS), None), norm3=gn(f"{p}.norm3"))
                w2 = ws(f"{p}.conv2", BOTTLENECK_EPS)
                L["conv2"] = PadIgemmConv(w2, None, stride=2) if stride == 2 else WinoConv3x3(w2, nobias(w2.shape[0]))
                if l == 0:
                    L["down"] = PadIgemmConv(ws(f"{p}.downsample.conv", BOTTLENECK_EPS), None, stride=stride)
                    L["down_norm"] = gn(f"{p}.downsample.norm")
                layers.append(L)
            self.stages.append(layers)
        h = a["VIT_WIDTH"]
        e = "dpt.embeddings"
        self.patch = PadIgemmConv(dev(sd[f"{e}.projection.weight"]), dev(sd[f"{e}.projection.bias"]))
        self.cls = dev(sd[f"{e}.cls_token"].reshape(h))
        self.pos = sd[f"{e}.position_embeddings"].detach().double().cpu()
        self._pos, self._n_tok = {}, {}
        self.layers = []
        for l in range(a["VIT_LAYERS"]):
            p = f"dpt.encoder.layer.{l}"
            wqkv, bqkv = fold_qkv(sd, p)
            lin = lambda n: SplitLinear(dev(sd[f"{p}.{n}.weight"]), dev(sd[f"{p}.{n}.bias"]))
            self.layers.append(dict(ln1=gn(f"{p}.layernorm_before"), ln2=gn(f"{p}.layernorm_after"), qkv=SplitLinear(dev(wqkv), dev(bqkv)),
                                    out=lin("attention.output.dense"), fc1=lin("intermediate.dense"), fc2=lin("output.dense")))
        rs = "neck.reassemble_stage"
        self.readout = {}
        for i in (2, 3):
            wa, wb, b = fold_readout(sd[f"{rs}.readout_projects.{i}.0.weight"], sd[f"{rs}.readout_projects.{i}.0.bias"])
            self.readout[i] = dict(tok=SplitLinear(dev(wa), None), cls=SplitLinear(dev(wb), dev(b)),
                                   proj=PadIgemmConv(dev(sd[f"{rs}.layers.{i}.projection.weight"]), dev(sd[f"{rs}.layers.{i}.projection.bias"])))
        self.resize3 = IgemmConv(dev(sd[f"{rs}.layers.3.resize.weight"]), dev(sd[f"{rs}.layers.3.resize.bias"]), stride=2, padding=1)
        self.neck_convs = [WinoConv3x3(dev(sd[f"neck.convs.{i}.weight"]), nobias(a["FUSION_WIDTH"])) for i in range(4)]
        self.fusion = []
        for i in range(4):
            p = f"neck.fusion_stage.layers.{i}"
            c3 = lambda n: WinoConv3x3(dev(sd[f"{p}.{n}.weight"]), dev(sd[f"{p}.{n}.bias"]))
            self.fusion.append(dict(r1=(c3("residual_layer1.convolution1"), c3("residual_layer1.convolution2")),
                                    r2=(c3("residual_layer2.convolution1"), c3("residual_layer2.convolution2")),
                                    proj=PadIgemmConv(dev(sd[f"{p}.projection.weight"]), dev(sd[f"{p}.projection.bias"]))))
        self.head0 = WinoConv3x3(dev(sd["head.head.0.weight"]), dev(sd["head.head.0.bias"]))
        self.head2 = WinoConv3x3(dev(sd["head.head.2.weight"]), dev(sd["head.head.2.bias"]))
        self.head4_w = dev(sd["head.head.4.weight"].reshape(-1))
        self.head4_b = float(sd["head.head.4.bias"].reshape(-1)[0])
        if self.head4_w.numel() > 64:
            raise ValueError("DPT: the head's last layer takes at most 64 channels (mfr_dpt_head_tail)")

    # ---- stages ----
    def stem_conv(self, x):
        """the 7x7 / 2 weight-standardised convolution behind TF-"SAME" padding: (2, 3) on the even sizes the network sees"""
        H, W = x.shape[2:]
        assert H % 32 == 0 and W % 32 == 0, "DPT: network sizes are multiples of 32"
        return self.stem(x, pad=same_padding(H, 7, 2))

    def embed(self, x):
        """BitEmbeddings: conv, GroupNorm + ReLU, max-pool"""
        g, b = self.stem_norm
        return maxpool3s2(groupnorm(self.stem_conv(x), g, b, self.arch["NUM_GROUPS"], relu=True))

    def bottleneck(self, L, x):
        G = self.arch["NUM_GROUPS"]
        short = x
        if "down" in L:
            short = groupnorm(L["down"](x), *L["down_norm"], G)
        y = groupnorm(L["conv1"](x), *L["norm1"], G, relu=True)
        y = L["conv2"](y, pad=same_padding(y.shape[2], 3, 2)) if L["stride"] == 2 else L["conv2"](y)
        y = groupnorm(y, *L["norm2"], G, relu=True)
        return groupnorm(L["conv3"](y), *L["norm3"], G, relu=True, residual=short)

    def backbone(self, x):
        """-> the three BiT stage outputs (1/4, 1/8, 1/16 of the network size)"""
        y, outs = self.embed(x), []
        for layers in self.stages:
            for L in layers:
                y = self.bottleneck(L, y)
            outs.append(y)
        return outs

    def position_embeddings(self, gh, gw):
        if (gh, gw) not in self._pos:
            self._pos[(gh, gw)] = resize_position_embeddings(self.pos, gh, gw).float().to(self.device).contiguous()
        return self._pos[(gh, gw)]

    def tokenize(self, feat):
        """stage-3 feature map -> token rows [B, 1 + gh gw, h]: patch projection (1x1), cls row, position embeddings"""
        return tokens(self.patch(feat), self.cls, self.position_embeddings(feat.shape[2], feat.shape[3]))

    def encoder(self, tok):
        """token rows [B, T, h] -> the tapped hidden states (the last two taps: the first two are BiT's feature maps)"""
        B, T, h = tok.shape
        x, taps = tok.reshape(B * T, h).clone(), {}
        last = max(self.arch["TAPS"][2:])
        for l, L in enumerate(self.layers[:last + 1]):
            self.vit_layer(L, x, B, T)
            if l in self.arch["TAPS"][2:]:
                taps[l] = x.clone().view(B, T, h)
        return [taps[l] for l in self.arch["TAPS"][2:]]

    def reassemble(self, i, hidden, gh, gw):
        """tap i (2 or 3) of the hybrid: readout projection (split: W_a token + (W_b cls + b)), GELU, 1x1 projection, and for i = 3 the 3x3 / 2 resize"""
        R = self.readout[i]
        B, T, h = hidden.shape
        rows = R["tok"](hidden.reshape(B * T, h)).view(B, T, h)
        bias_img = R["cls"](hidden[:, 0])                          # [B, h]: one small product per image set
        y = R["proj"](tokens_inverse(rows, gh, gw, bias_img=bias_img, gelu=True))
        return self.resize3(y) if i == 3 else y

    def neck(self, feats):
        """four reassembled maps (finest first) -> the last fused map [B, F, Hn / 2, Wn / 2]"""
        f = [c(x) for c, x in zip(self.neck_convs, feats)]
        y = self.fusion_layer(self.fusion[0], f[3])
        for i in (1, 2, 3):
            y = self.fusion_layer(self.fusion[i], y, f[3 - i])
        return y

    def head_features(self, fused):
        """head.0 (3x3), x2 bilinear (align_corners=True), head.2 (3x3) + ReLU -> [B, 32, Hn, Wn]"""
        return self.head2(upsample2x(self.head0(fused)), act=1)

    def features(self, x):
        """network input [B, 3, Hn, Wn] -> the head's last feature map"""
        s1, s2, s3 = self.backbone(x)
        gh, gw = s3.shape[2:]
        t2, t3 = self.encoder(self.tokenize(s3))
        return self.head_features(self.neck([s1, s2, self.reassemble(2, t2, gh, gw), self.reassemble(3, t3, gh, gw)]))

    def __call__(self, img, net_hw, out_hw=None, invert=False, scale=1.0, shift=0.0, millimetres=False):
        """img u8 [B, H, W, 3] or f32 [B, 3, H, W] in [0, 1] -> (metres f32 [B, H, W], u16 millimetres or None) at out_hw (None: the image's size)"""
        if out_hw is None:
            out_hw = tuple(img.shape[1:3]) if img.dtype == torch.uint8 else tuple(img.shape[2:4])
        f = self.features(prep(img, int(net_hw[0]), int(net_hw[1])))
        return head_tail(f, self.head4_w, self.head4_b, int(out_hw[0]), int(out_hw[1]), invert=invert, scale=scale, shift=shift, millimetres=millimetres)

    # ---- the seam (DepthNetBase) ----
    def prep(self, img, net_hw):
        return prep(img, int(net_hw[0]), int(net_hw[1]))

    def prep_rows(self, img, rows, net_hw, status):
        return prep_rows(img, rows, int(net_hw[0]), int(net_hw[1]), status)

    def tail(self, f, out_hw, millimetres=False):
        return head_tail(f, self.head4_w, self.head4_b, int(out_hw[0]), int(out_hw[1]), millimetres=millimetres, **self.convention)

    def tail_rows(self, f, src, dst, metres, status, quantize=False):
        return head_tail_rows(f, self.head4_w, self.head4_b, src, dst, metres, status, quantize=quantize, **self.convention)


# ------------------------------------------------------------------------------------------------ the config's stage
def check_cfg(cfg):
    """the DPT node of a config, checked: network sizes are multiples of 32, SOURCE is 'file' or 'online', the architecture is one the kernels have"""
    node = cfg.DPT
    network = node.get("NETWORK", "hybrid")
    if network not in NETWORKS:
        raise ValueError(f"DPT.NETWORK = {network!r}: one of {NETWORKS}")
    if network == "depth_anything":                                            # its sizes and architecture live in the DA node
        from .depth_anything import check_cfg as check_da
        check_da(cfg)
    elif node.NET_HEIGHT % 32 or node.NET_WIDTH % 32 or node.NET_HEIGHT < 32 or node.NET_WIDTH < 32:
        raise ValueError(f"DPT.NET_HEIGHT x NET_WIDTH = {node.NET_HEIGHT} x {node.NET_WIDTH}: both must be multiples of 32")
    if node.SOURCE not in ("file", "online"):
        raise ValueError(f"DPT.SOURCE = {node.SOURCE!r}: 'file' (depth maps come with the dataset) or 'online' (computed per pair)")
    chunk = node.get("FUSED_CHUNK", 16)
    if isinstance(chunk, bool) or not isinstance(chunk, int) or chunk < 1:
        raise ValueError(f"DPT.FUSED_CHUNK = {chunk!r}: the views per DPT launch on the fused route, an integer >= 1")
    if network == "hybrid":
        check_arch(dict(node.ARCH))
    return node


def state_dict_from_cfg(cfg):
    """(state dict, architecture dict) of a config's DPT node: DPT.WEIGHTS, or the synthetic weights when the config allows them"""
    from . import weights as WT
    node = check_cfg(cfg)
    arch = dict(node.ARCH)
    return WT.from_cfg("DPT", cfg, node.WEIGHTS, lambda: WT.dpt_state_dict(int(node.SYNTHETIC_SEED), arch=arch)), arch


def build_network(cfg, device="cuda"):
    """the ONE place where the configured depth network is built -> (maker, net_hw): maker() returns a new network object (DepthNetBase's seam) in the
    arithmetic `HIP.SPLIT` names at that moment -- the range guard's twin is a second call -- and net_hw is the network's input size.  DPT.NETWORK 'hybrid':
    DPTHIP with the DPT node's SCALE / SHIFT / INVERT as its output convention; 'depth_anything': nets/depth_anything.DepthAnythingHIP (the DA node)"""
    node = check_cfg(cfg)
    if node.get("NETWORK", "hybrid") == "depth_anything":
        from . import depth_anything as DA
        return DA.network_from_cfg(cfg, device)
    sd, arch = state_dict_from_cfg(cfg)
    convention = dict(invert=bool(node.INVERT), scale=float(node.SCALE), shift=float(node.SHIFT))

    def maker():
        net = DPTHIP(sd, device, arch=arch)
        net.convention = dict(convention)
        return net
    return maker, (int(node.NET_HEIGHT), int(node.NET_WIDTH))


FUSED_DEPTH_VIEWS = {"PNP": "ref", "EssentialMatrixMetric": "both", "Procrustes": "both"}     # the depth maps each pose solver reads; EssentialMatrix: none


def fused_depth_views(cfg):
    """what the batched route has to compute itself: None (DPT.SOURCE 'file', or a solver that reads no depth), 'ref' (depth0 only) or 'both'"""
    if "DPT" not in cfg or cfg.DPT.SOURCE != "online":
        return None
    return FUSED_DEPTH_VIEWS.get(cfg.POSE_SOLVER)


def millimetres_to_metres(mm):
    """u16 millimetres (a torch tensor on any device) -> float32 metres with the arithmetic of datasets.read_depth_image: float32(v / 1000.0) in float64"""
    v = mm.view(torch.int16).to(torch.int32) & 0xFFFF
    return (v.to(torch.float64) / 1000).to(torch.float32)


class DepthEstimator:
    """DPTHIP behind a config's DPT node: images in, depth maps at the images' size out.  `metres` is what a consumer of depth maps reads: with QUANTIZE_MM
    the millimetre-rounded map -- the bits the 16-bit PNG of compute_depth holds, read back as datasets.read_depth_image does -- else the float32 map."""

    def __init__(self, cfg, device="cuda"):
        node = check_cfg(cfg)
        maker, self.net_hw = build_network(cfg, device)
        from ..pipeline import RangeGuard
        self.net = maker()
        self.device = self.net.device
        # the f16x2 range guard, as for the matcher networks: a launch whose accumulators left the fp32-finite range (an operand beyond 65504) sets the flag,
        # and the batch runs again through the bf16x3 twin (linear layers, attention and the 3x3 / stride 1 layers; the implicit-GEMM layers exist in f16x2 only)
        self.guard = RangeGuard(self.device, maker)
        self.quantize = bool(node.QUANTIZE_MM)

    @torch.no_grad()
    def __call__(self, images, out_hw=None):
        """images u8 [B, H, W, 3] or f32 [B, 3, H, W] in [0, 1] (any device) -> (metres f32, millimetres u16), both [B, *out_hw] on the GPU (out_hw None: the
        images' own size)"""
        images = images.to(self.device)
        with self.guard:
            out = self.net.depth(images, self.net_hw, out_hw, millimetres=True)
        if self.guard.active and int(self.guard.flag.item()):           # the maps are read on the host next anyway: this is not an extra synchronisation
            self.guard.reruns += 1
            out = self.guard.twin().depth(images, self.net_hw, out_hw, millimetres=True)
        return out

    def metres(self, images, out_hw=None):
        m, mm = self(images, out_hw)
        return millimetres_to_metres(mm) if self.quantize else m


class FusedDepthStage:
    """DPT.SOURCE 'online' on the batched route (pipeline.FusedPosePipeline): fills batch['depth0'] (views 'ref') or batch['depth0'] and batch['depth1'] (views
    'both') [b, H, W] f32 from batch['rgb'], the u8 [2b, H, W, 3] colour bytes PairBatchLoader(rgb=True) carries (row 2p = pair p's reference view).

    Only the views the solver reads go through the network, and a reference view once: the batch's pairs are grouped by `ref_keys` (the semantics of
    ref_cache.RefViewCache: None = a view nobody shares, never retained; the last `keep` maps are kept, `cache=False`: none across batches).  The
    selected rows are read in place (mfr_dpt_prep_rows: no gather copy of the images), pass DPTHIP in chunks of DPT.FUSED_CHUNK views, and the tail writes
    each map straight into every plane that wants it (mfr_dpt_head_tail_rows: a shared reference map lands in the depth0 row of each of its pairs).  With
    DPT.QUANTIZE_MM the planes hold millimetres_to_metres of the rounded map: the bits the per-pair plugin's DepthEstimator.metres hands its solver.

    Runs INSIDE the caller's RangeGuard window and never reads the flag on the host: a flagged launch marks the batch's rows ST_RANGE through the caller's
    fold, and the scene is recomputed through the bf16x3 twin (submission._rerun_out_of_range_scenes)."""

    def __init__(self, cfg, device, guard=None, views="both", cache=True, keep=4):
        from ..ref_cache import RefViewCache
        assert views in ("ref", "both")
        node = check_cfg(cfg)
        maker, self.net_hw = build_network(cfg, device)
        self.net = maker()
        self.device, self.guard, self.views, self.use_cache, self.keep = self.net.device, guard, views, bool(cache), int(keep)
        self.quantize = bool(node.QUANTIZE_MM)
        self.chunk = int(node.get("FUSED_CHUNK", 16))
        self.cache = RefViewCache(guard)                                          # key -> RefEntry(flag, metres: the map [H, W] the solver reads)
        self.stats = dict(depth_views_run=0, depth_views_reused=0)
        self.table_status = torch.zeros(1, dtype=torch.int32, device=self.device)  # bit 0: a row table of this class left its range (a bug here, never data)

    def _table(self, values):
        """int32 table on the device through pinned memory: an asynchronous copy, the stream is not drained"""
        return torch.tensor(values, dtype=torch.int32).pin_memory().to(self.device, non_blocking=True)

    @torch.no_grad()
    def maps(self, rgb, ref_rows, ref_keys, query_rows=()):
        """rgb u8 [N, H, W, 3] on the device; ref_rows[p] / ref_keys[p]: pair p's reference row of `rgb` and its identity (None: not shared); query_rows: rows
        that always run -> planes [len(ref_rows) + len(query_rows), H, W] f32: the reference maps in pair order, then the query maps"""
        assert rgb.is_cuda and rgb.dtype == torch.uint8 and rgb.dim() == 4 and rgb.shape[3] == 3
        rgb = rgb.contiguous()
        H, W = rgb.shape[1:3]
        b, nq = len(ref_rows), len(query_rows)
        plan = self.cache.plan(ref_keys)
        first, pairs_of, need = plan.first, plan.pairs_of, plan.need
        rows = [int(ref_rows[first[k]]) for k in need] + [int(r) for r in query_rows]
        dsts = [pairs_of[k] for k in need] + [[b + q] for q in range(nq)]
        planes = torch.empty(b + nq, H, W, dtype=torch.float32, device=self.device)
        flags = {}
        for c0 in range(0, len(rows), self.chunk):
            c1 = min(c0 + self.chunk, len(rows))
            src = [j - c0 for j in range(c0, c1) for _ in dsts[j]]
            dst = [t for j in range(c0, c1) for t in dsts[j]]
            m, d = c1 - c0, len(src)
            tab = self._table(rows[c0:c1] + src + dst)
            f = self.net.features(self.net.prep_rows(rgb, tab[:m], self.net_hw, self.table_status))
            self.net.tail_rows(f, tab[m:m + d], tab[m + d:], planes, self.table_status, quantize=self.quantize)
            if c0 < len(need):                                                    # one flag copy per chunk that holds reference rows
                flag = self.cache.take_flag()
                flags.update({k: flag for k in need[c0:c1]})
        self.stats["depth_views_run"] += len(rows)
        self.stats["depth_views_reused"] += len(plan.reused)
        for k in plan.reused:
            for p in pairs_of[k]:
                planes[p].copy_(self.cache[k].metres)
        self.cache.carry(plan)
        if self.use_cache:
            for k in need:
                if k not in plan.solo:
                    self.cache.put(k, flags[k], metres=planes[first[k]].clone())
            self.cache.settle(plan, self.keep)
        return planes

    def __call__(self, batch):
        rgb = batch.get("rgb")
        if rgb is None:
            raise ValueError("DPT.SOURCE 'online' on the fused route needs the batch's colour bytes: build the loader with PairBatchLoader(..., rgb=True)")
        b = rgb.shape[0] // 2
        keys = batch.get("ref_keys")
        if keys is None or len(keys) != b:
            keys = [None] * b
        both = self.views == "both"
        planes = self.maps(rgb, [2 * p for p in range(b)], keys, [2 * p + 1 for p in range(b)] if both else ())
        batch["depth0"] = planes[:b]
        if both:
            batch["depth1"] = planes[b:]
        return batch
