"""EfficientLoFTR (Wang et al., CVPR 2024) on MI355X: the successor of LoFTR with the same semi-dense contract -- a gray pair in, [N, 4] sub-pixel
correspondences out -- through a re-parameterised RepVGG backbone, attention on a 4x-aggregated token grid and a two-stage correlation refinement.

The architecture of record is the `transformers` module EfficientLoFTRForKeypointMatching (default EfficientLoFTRConfig); its state-dict names are the
names this stage loads (`efficientloftr.backbone.stages.{s}.blocks.{b}.conv1.conv.weight` ..., `refinement_layer.*`).  Where the module and the paper
differ the module is followed, except where the module's own batch handling is at odds with both (stated here; they show for B > 1, for non-mutual
slots, or in the fine stage):
  * the module pairs, in output slot s, the image-0 cell matched to image-1 cell s with the image-1 cell matched to image-0 cell s.  This stage emits
    MATCHES (i, j = the mutual maximum of i), one slot per matched image-0 cell, ascending;
  * the module takes the second-stage expectation of batch element 0 for every pair of a batch (`spatial_expectation2d(...)[0]`) and mixes the pairs'
    index tensors when it reshapes them (`torch.cat(...).reshape(B, 2, -1)`).  Here every pair uses its own: what the module computes for a batch of one;
  * in the fine stage the module's tensors carry a leading batch axis its code does not count: the first stage's `softmax(., 1) * softmax(., 2)` runs over
    the MATCH axis and the 64 axis, and the offsets are gathered along the match axis (always grid[0]).  This stage computes what the paper and upstream
    compute on their 3-D tensors: both softmaxes on each match's own 64 x 100 matrix, offsets grid[arg-max] - 4 + 0.5 (tests/eloftr_ref.py restates it).
Parity with the published `zju-community/efficientloftr` weights is unpinned offline: no checkpoint exists there; every stage is pinned against
the module on seeded weights (tests/test_gpu_eloftr.py).

What runs where:
  * backbone: every RepVGG block folded into ONE 3x3 convolution + bias + ReLU (`fold_weights`, float64 on the host); the 1 -> 64 stride-2 stem is
    mfr_eloftr_stem_s2, the rest the project's 3x3 kernels (nets/conv.py), under the f16x2 range guard like LoFTR's backbone.  In the 18 blocks with an
    identity branch the unit part of that branch is added through the same launch's fp32 residual operand (`skip_form`).  Under bf16x3 the three
    stride-2 layers are the framework's convolution (the implicit-GEMM kernel is f16x2 only), restricted to the library's deterministic solvers;
  * transformer: tokens live in xm [2, B L, 512] (side-major; x in the left half, the up-sampled message in the right half: the MLP's concatenation
    exists in place, as in nets/loftr.py).  Aggregation + LayerNorm, rotary encoding, short-sequence attention, x4 up-sampling, leaky ReLU:
    csrc/eloftr.hip; projections and the MLP: csrc/gemm_split.hip (HIP.SPLIT arithmetic); LayerNorm + residual: mfr_layernorm;
  * coarse matching: mfr_loftr_coarse_match (the same dual-softmax / threshold / border / mutual-maximum contract as LoFTR's);
  * fine pyramid: 1x1 and 3x3 convolutions through the project's kernels, the x2 up-samplings (align_corners=False) through mfr_eloftr_upsample2x.
    The LAST x2 up-sampling is NOT materialised: at 544 x 736 the full-resolution map is 102 MB per image and only the matched cells' windows are
    read, so mfr_eloftr_gather_windows evaluates it per window pixel from the half-resolution map;
  * two-stage fine matching: mfr_eloftr_fine_match, one wavefront per match; the drop of matches outside the unpadded frame and the ordered
    compaction: mfr_eloftr_compact.  No host synchronisation anywhere in the stage: slots behind a pair's match count are skipped on the device.
"""
import contextlib
import ctypes
import typing

import torch
import torch.nn.functional as F

from .. import _lib, options
from .loftr import LoFTRHIP
from .weights import ELOFTR_STAGES

HIDDEN, HEADS, AGG = 256, 8, 4
PAD_TO = 32                                  # the 1/8 map must be divisible by the aggregation's 4
BN_EPS_CONV = 1e-5                           # EfficientLoFTRConfig.batch_norm_eps: the conv + norm branches
BN_EPS_DEFAULT = 1e-5                        # nn.BatchNorm2d's default: the identity branch and OutConvBlock.batch_norm
N_LAYERS = 4


def _bn_fold(sd, name, eps):
    s = sd[f"{name}.weight"] / torch.sqrt(sd[f"{name}.running_var"] + eps)
    return s, sd[f"{name}.bias"] - sd[f"{name}.running_mean"] * s


def fold_repvgg_block(sd, prefix, eps_conv=BN_EPS_CONV, eps_identity=BN_EPS_DEFAULT):
    """one RepVGG block (3x3 conv + BN, 1x1 conv + BN, identity BN where present) -> (w [Cout, Cin, 3, 3], b [Cout]) in float64"""
    w3, w1 = sd[f"{prefix}.conv1.conv.weight"].double(), sd[f"{prefix}.conv2.conv.weight"].double()
    s3, b3 = _bn_fold(sd, f"{prefix}.conv1.norm", eps_conv)
    s1, b1 = _bn_fold(sd, f"{prefix}.conv2.norm", eps_conv)
    w = w3 * s3[:, None, None, None]
    w[:, :, 1, 1] += w1[:, :, 0, 0] * s1[:, None]
    b = b3 + b1
    if f"{prefix}.identity.weight" in sd:
        si, bi = _bn_fold(sd, f"{prefix}.identity", eps_identity)
        idx = torch.arange(w.shape[0])
        w[idx, idx, 1, 1] += si
        b = b + bi
    return w, b


def skip_form(w):
    """the folded filter of a block WITH an identity branch, minus the unit centre tap: conv(x; w) = conv(x; w - I) + x.  The device adds that x
    through the convolution kernel's fp32 residual operand (the same launch), so the block's dominant term -- the identity branch, whose folded
    gain is near 1 -- does not pass through the 22-bit split product of the f16x2 arithmetic in each of the 18 such blocks; only (gain - 1) x does."""
    w = w.clone()
    idx = torch.arange(w.shape[0])
    w[idx, idx, 1, 1] -= 1.0
    return w


def fold_weights(state_dict):
    """Module parameters -> the f32 operands the GPU path multiplies with (pure host code, float64):
      * every RepVGG block as one 3x3 convolution + bias (`backbone`: list of dict(w, b, stride, w_skip); w_skip: `skip_form` of w for the blocks with an
        identity branch, None for the others);
      * k_proj and v_proj stacked into one [512, 256] product;
      * `refinement_layer.out_conv` scaled by 1 / sqrt(256) = 1/16 is NOT folded (the scale rides on the NCHW hand-over, exact);
        OutConvBlock.batch_norm folded into out_conv2 (`fine`: list of dict(w1, w2, b2, w3)).
    Returns dict(backbone, layers=[dict(self=blk, cross=blk)], out_conv, fine), blk = dict(wagg, ln, wq, wkv, wo, w1, w2, mlp_ln)."""
    sd = {k: v.double() for k, v in state_dict.items() if v.is_floating_point()}
    f32 = lambda t: t.float().contiguous()
    backbone = []
    for s, (ci, co, stride, blocks) in enumerate(ELOFTR_STAGES):
        for b in range(blocks):
            p = f"efficientloftr.backbone.stages.{s}.blocks.{b}"
            w, bias = fold_repvgg_block(sd, p)
            backbone.append(dict(w=f32(w), b=f32(bias), stride=stride if b == 0 else 1, w_skip=f32(skip_form(w)) if f"{p}.identity.weight" in sd else None))
    layers = []
    for l in range(N_LAYERS):
        pair = {}
        for kind in ("self", "cross"):
            p = f"efficientloftr.local_feature_transformer.layers.{l}.{kind}_attention"
            pair[kind] = dict(wagg=f32(sd[f"{p}.aggregation.q_aggregation.weight"].reshape(HIDDEN, AGG * AGG)),
                              ln=(f32(sd[f"{p}.aggregation.norm.weight"]), f32(sd[f"{p}.aggregation.norm.bias"])),
                              wq=f32(sd[f"{p}.attention.q_proj.weight"]),
                              wkv=f32(torch.cat([sd[f"{p}.attention.k_proj.weight"], sd[f"{p}.attention.v_proj.weight"]], 0)),
                              wo=f32(sd[f"{p}.attention.o_proj.weight"]), w1=f32(sd[f"{p}.mlp.fc1.weight"]), w2=f32(sd[f"{p}.mlp.fc2.weight"]),
                              mlp_ln=(f32(sd[f"{p}.mlp.layer_norm.weight"]), f32(sd[f"{p}.mlp.layer_norm.bias"])))
        layers.append(pair)
    fine = []
    for i in range(2):
        p = f"refinement_layer.out_conv_layers.{i}"
        s, b = _bn_fold(sd, f"{p}.batch_norm", BN_EPS_DEFAULT)
        fine.append(dict(w1=f32(sd[f"{p}.out_conv1.weight"]), w2=f32(sd[f"{p}.out_conv2.weight"] * s[:, None, None, None]), b2=f32(b),
                         w3=f32(sd[f"{p}.out_conv3.weight"])))
    return dict(backbone=backbone, layers=layers, out_conv=f32(sd["refinement_layer.out_conv.weight"]), fine=fine)


def check_cfg(cfg):
    """the ELOFTR node of a config: what this stage does not build is an error, not a silent default"""
    el = cfg.ELOFTR
    if float(el.MATCH_THRESHOLD) < 0.0 or float(el.MATCH_THRESHOLD) >= 1.0:
        raise ValueError(f"ELOFTR.MATCH_THRESHOLD = {el.MATCH_THRESHOLD!r}: a dual-softmax confidence lies in [0, 1)")
    if int(el.BORDER_RM) < 0:
        raise ValueError(f"ELOFTR.BORDER_RM = {el.BORDER_RM!r} must be >= 0")
    if float(el.TEMPERATURE) <= 0.0:
        raise ValueError(f"ELOFTR.TEMPERATURE = {el.TEMPERATURE!r} must be > 0")
    if bool(el.get("SKIP_SOFTMAX", False)):
        raise ValueError("ELOFTR.SKIP_SOFTMAX: coarse matching on the raw similarity (upstream's 'optimized' variant) is out of scope of this stage")
    if bool(el.get("HALF_PRECISION", False)):
        raise ValueError("ELOFTR.HALF_PRECISION: the fp16 variant of upstream is out of scope; the stage computes at fp32 accuracy")
    return el


def from_cfg(cfg, device):
    """-> EfficientLoFTRHIP of a config (ELOFTR.*)"""
    from . import weights as WT
    el = check_cfg(cfg)
    sd = WT.from_cfg("EfficientLoFTR", cfg, el.WEIGHTS, lambda: WT.eloftr_state_dict(el.SYNTHETIC_SEED))
    return EfficientLoFTRHIP(sd, device, el.MATCH_THRESHOLD, el.BORDER_RM, el.TEMPERATURE, el.get("MAX_MATCHES", None))


class ELoFTRFeatures(typing.NamedTuple):
    """the per-image part: the backbone's three kept maps (NCHW).  Everything after reads images only through these, so a view shared by many
    pairs runs the backbone once (features / match_features, as LoFTRHIP)"""
    s1: torch.Tensor                # [n,  64, H/2, W/2]
    s2: torch.Tensor                # [n, 128, H/4, W/4]
    s3: torch.Tensor                # [n, 256, H/8, W/8]


@contextlib.contextmanager
def _deterministic_library():
    """the framework's convolution restricted to the library's deterministic solvers for the calls inside (the flag alone: torch.backends.cudnn.flags
    would also set a benchmark limit the library does not have, and warn)"""
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        yield
    finally:
        torch.backends.cudnn.deterministic = before


class _Conv:
    """one folded convolution layer (3x3 stride 1 / 2 or 1x1): the project's kernels where they exist for the arithmetic, as nets/loftr.LoFTRHIP._c"""

    def __init__(self, w, b, stride=1):
        self.w, self.b, self.stride, self.k = w, b, int(stride), int(w.shape[-1])
        self.wino = self.igemm = None
        if options.get("CONV") == "wino":
            from .conv import IgemmConv, WinoConv3x3
            if self.k == 3 and self.stride == 1:
                self.wino = WinoConv3x3(w, b)
            elif options.get("SPLIT") == "f16x2":
                self.igemm = IgemmConv(w, b, self.stride)

    def rows(self, x, act=0):
        return self.wino.rows(x, act=act) if self.wino is not None else None

    def __call__(self, x, act=0, residual=None):
        """act: 0 none, 1 ReLU, 2 LeakyReLU(0.01); residual [B,Cout,H,W]: added before the activation, in fp32"""
        if self.wino is not None:
            return self.wino(x, act=act, residual=residual)
        if self.igemm is not None and act in (0, 1) and residual is None:
            return self.igemm(x, relu=act == 1)
        if self.k == 1 and self.stride == 1:
            B, C, H, W = x.shape
            w3 = self.w.view(1, self.w.shape[0], C).expand(B, -1, -1)
            y = torch.bmm(w3, x.reshape(B, C, H * W)).view(B, -1, H, W)
            if self.b is not None:
                y = y + self.b.view(1, -1, 1, 1)
        else:
            # the library's convolution (bf16x3: the stride-2 3x3 layers; CONV = "miopen": all of them).  Its default choice for the 64 -> 128 stride-2
            # layer returned different bits from run to run on the same input (tests/test_gpu_pool_poison.py found it, docs/HISTORY.md); restricted to
            # its deterministic solvers it is reproducible like every kernel of the project
            with _deterministic_library():
                y = F.conv2d(x, self.w, self.b, stride=self.stride, padding=self.k // 2)
        if residual is not None:
            y = y + residual
        return F.relu_(y) if act == 1 else F.leaky_relu_(y, 0.01) if act == 2 else y


def rotary_table(ha, wa, device):
    """cos | sin [ha wa, 256] of the module's 128 angles per aggregated cell: 64 inverse frequencies (theta 10000 over dim 128), even slots the
    1-based row index, odd slots the 1-based column index (compute_embeddings); the repeat of every angle is the kernel's pairing"""
    inv_freq = 1.0 / (10000.0 ** (torch.arange(0, 128, 2, dtype=torch.float) / 128))
    i = torch.ones(ha, wa).cumsum(0).unsqueeze(-1)
    j = torch.ones(ha, wa).cumsum(1).unsqueeze(-1)
    emb = torch.zeros(ha, wa, HIDDEN // 2)
    emb[:, :, 0::2] = i * inv_freq
    emb[:, :, 1::2] = j * inv_freq
    return torch.cat([emb.cos(), emb.sin()], -1).reshape(ha * wa, HIDDEN).contiguous().to(device)


class EfficientLoFTRHIP:
    def __init__(self, state_dict, device="cuda", thr=0.2, border_rm=2, temperature=0.1, max_matches=None):
        _lib.load(require_gpu=True)
        self.device = torch.device(device)
        self.thr, self.border, self.temp = float(thr), int(border_rm), float(temperature)
        self.max_matches = None if max_matches in (None, 0) else int(max_matches)
        self.match_type = "dual_softmax"
        fw = fold_weights(state_dict)
        dev = lambda t: t.to(self.device).contiguous()
        self.stem = (dev(fw["backbone"][0]["w"]), dev(fw["backbone"][0]["b"]))
        # blocks with an identity branch run conv(x; w - I) + x: the x rides the kernel's fp32 residual operand (skip_form)
        self.convs = [_Conv(dev(f["w"] if f["w_skip"] is None else f["w_skip"]), dev(f["b"]), f["stride"]) for f in fw["backbone"][1:]]
        self.skip = [f["w_skip"] is not None for f in fw["backbone"][1:]]
        self.stage_end = []                                              # index into self.convs of the last block of stages 1, 2, 3
        n = -1
        for _, _, _, blocks in ELOFTR_STAGES:
            n += blocks
            self.stage_end.append(n - 1)
        self.stage_end = self.stage_end[1:]
        from .linear import SplitLinear
        self.layers = []
        for pair in fw["layers"]:
            blk = {}
            for kind, p in pair.items():
                blk[kind] = dict(wagg=dev(p["wagg"]), ln=tuple(dev(t) for t in p["ln"]), mlp_ln=tuple(dev(t) for t in p["mlp_ln"]),
                                 lq=SplitLinear(dev(p["wq"])), lkv=SplitLinear(dev(p["wkv"])), lo=SplitLinear(dev(p["wo"])),
                                 l1=SplitLinear(dev(p["w1"])), l2=SplitLinear(dev(p["w2"])))
            self.layers.append(blk)
        self.out_conv = _Conv(dev(fw["out_conv"]), None)
        self.fine = [dict(c1=_Conv(dev(f["w1"]), None), c2=_Conv(dev(f["w2"]), dev(f["b2"])), c3=_Conv(dev(f["w3"]), None)) for f in fw["fine"]]
        if options.get("SPLIT") == "f16x2":
            from .linear import SplitBatchedNT
            self.sim_gemm = SplitBatchedNT()
        else:
            self.sim_gemm = None
        self._ws_cm = None
        self._cs = {}
        self.frame_hw = None                                             # the unpadded (H, W) when the CALLER padded the images (pipeline._RefCachedLoFTR)

    # the dual-softmax coarse matcher is LoFTR's, the same contract: similarity (f0 / 16) . (f1 / 16), temperature, strict threshold, border, mutual maximum
    coarse_match = LoFTRHIP.coarse_match
    coarse_match_features = LoFTRHIP.coarse_match_features
    layernorm = staticmethod(LoFTRHIP.layernorm)

    # ------------------------------------------------------------------ backbone
    def stem_s2(self, x):
        B, _, H, W = x.shape
        w, b = self.stem
        y = torch.empty(B, w.shape[0], H // 2, W // 2, dtype=torch.float32, device=x.device)
        _lib.call("mfr_eloftr_stem_s2", x.contiguous(), w, b, B, H, W, w.shape[0], y)
        return y

    def backbone(self, x):
        """x [n,1,H,W] (H, W multiples of 32) -> ELoFTRFeatures"""
        x = self.stem_s2(x)
        kept = []
        for i, c in enumerate(self.convs):
            x = c(x, act=1, residual=x if self.skip[i] else None)
            if i in self.stage_end:
                kept.append(x)
        return ELoFTRFeatures(*kept)

    # ------------------------------------------------------------------ transformer stages
    def aggregate(self, blk, x, nimg, hw, want_q=True, want_kv=True):
        """x: token rows [nimg * L, >= 256] (row-strided view, images L rows apart) -> (q tokens, kv tokens) [nimg * La, 256] after the shared LayerNorm"""
        hc, wc = hw
        La = (hc // AGG) * (wc // AGG)
        assert x.stride(1) == 1 and x.shape[0] == nimg * hc * wc
        q = torch.empty(nimg * La, HIDDEN, dtype=torch.float32, device=x.device) if want_q else None
        kv = torch.empty(nimg * La, HIDDEN, dtype=torch.float32, device=x.device) if want_kv else None
        _lib.call("mfr_eloftr_aggregate", x.data_ptr(), x.stride(0), hc * wc * x.stride(0), nimg, hc, wc, blk["wagg"], blk["ln"][0], blk["ln"][1], 1e-5, q, kv)
        return q, kv

    def rotary(self, qkv, hw_agg):
        """rotary encoding in place on the q and k columns of qkv [rows, 768] (q | k | v)"""
        if hw_agg not in self._cs:
            self._cs[hw_agg] = rotary_table(hw_agg[0], hw_agg[1], qkv.device)
        La = hw_agg[0] * hw_agg[1]
        _lib.call("mfr_eloftr_rotary", qkv.data_ptr(), qkv.data_ptr() + HIDDEN * 4, qkv.stride(0), self._cs[hw_agg], qkv.shape[0], La)
        return qkv

    def attention(self, qkv, nimg, La):
        """qkv [nimg * La, 768] -> softmax attention per image and head [nimg * La, 256]"""
        out = torch.empty(nimg * La, HIDDEN, dtype=torch.float32, device=qkv.device)
        base, ld = qkv.data_ptr(), qkv.stride(0)
        _lib.call("mfr_eloftr_attention", base, ld, base + HIDDEN * 4, base + 2 * HIDDEN * 4, ld, nimg, La, La, HEADS, out, HIDDEN)
        return out

    def block(self, blk, xq, xkv, nimg, hw, rotary):
        """one EfficientLoFTRAggregatedAttention on the rows xq [nimg * L, 512] (x | message; x updated in place) attending to the x half of xkv"""
        hc, wc = hw
        L, hw_agg = hc * wc, (hc // AGG, wc // AGG)
        La = hw_agg[0] * hw_agg[1]
        if xq.data_ptr() == xkv.data_ptr():
            q_tok, kv_tok = self.aggregate(blk, xq[:, :HIDDEN], nimg, hw)
        else:
            q_tok = self.aggregate(blk, xq[:, :HIDDEN], nimg, hw, want_kv=False)[0]
            kv_tok = self.aggregate(blk, xkv[:, :HIDDEN], nimg, hw, want_q=False)[1]
        qkv = torch.empty(nimg * La, 3 * HIDDEN, dtype=torch.float32, device=xq.device)
        blk["lq"](q_tok, out=qkv[:, :HIDDEN])
        blk["lkv"](kv_tok, out=qkv[:, HIDDEN:])
        if rotary:
            self.rotary(qkv, hw_agg)
        msg = blk["lo"](self.attention(qkv, nimg, La))
        right = xq[:, HIDDEN:]
        _lib.call("mfr_eloftr_upsample4_rows", msg, HIDDEN, nimg, hw_agg[0], hw_agg[1], right.data_ptr(), xq.stride(0), L * xq.stride(0))
        hid = blk["l1"](xq)
        _lib.call("mfr_eloftr_leaky_relu", hid, hid.stride(0), hid.shape[0], hid.shape[1], 0.01)
        x = xq[:, :HIDDEN]
        self.layernorm(blk["l2"](hid), blk["mlp_ln"], x, residual=x)            # x += LayerNorm(fc2(leaky(fc1([x | up(msg)]))))
        return xq

    def transformer(self, xm, B, hw, n_layers=N_LAYERS):
        """xm [2, B L, 512] in place: per layer, self attention (rotary) on all 2B images, then the cross pair -- image 0 attends to image 1, image 1 to the
        UPDATED image 0 (the module's order)"""
        both = xm.view(-1, 2 * HIDDEN)
        for blk in self.layers[:n_layers]:
            self.block(blk["self"], both, both, 2 * B, hw, True)
            self.block(blk["cross"], xm[0], xm[1], B, hw, False)
            self.block(blk["cross"], xm[1], xm[0], B, hw, False)
        return xm

    def tokens(self, src0, idx0, src1, idx1):
        """the two sides' 1/8 maps -> xm [2, B L, 512], side-major, x in the left half"""
        B = len(idx0)
        C, hc, wc = src0.s3.shape[1:]
        L = hc * wc
        xm = torch.empty(2, B * L, 2 * C, dtype=torch.float32, device=src0.s3.device)
        for s, (src, idx) in enumerate(((src0, idx0), (src1, idx1))):
            tab = (ctypes.c_int32 * B)(*idx)
            _lib.call("mfr_nchw_to_rows_gather", src.s3, None, src.s3.shape[0], C, L, ctypes.addressof(tab), B, xm[s], L * 2 * C, 2 * C)
        return xm

    # ------------------------------------------------------------------ fine level
    def upsample2x(self, x, add=None):
        B, C, H, W = x.shape
        out = torch.empty(B, C, 2 * H, 2 * W, dtype=torch.float32, device=x.device)
        assert add is None or (add.shape == out.shape and add.is_contiguous())
        _lib.call("mfr_eloftr_upsample2x", x.contiguous(), add, out, B * C, H, W)
        return out

    def coarse_map(self, xm, nimg, hw):
        """the transformer's tokens as the NCHW map the pyramid convolves, scaled by 1 / sqrt(256) (the module divides AFTER coarse matching)"""
        hc, wc = hw
        out = torch.empty(nimg, HIDDEN, hc, wc, dtype=torch.float32, device=xm.device)
        rows = xm.view(-1, 2 * HIDDEN)
        _lib.call("mfr_eloftr_rows_to_nchw", rows.data_ptr(), rows.stride(0), hc * wc * rows.stride(0), nimg, HIDDEN, hc * wc, 1.0 / 16.0, out)
        return out

    def pyramid(self, coarse, s2, s1):
        """coarse [n,256,h,w] (already / 16), the backbone's 1/4 and 1/2 maps -> the HALF-resolution 64-channel map in NHWC memory [n, H/2, W/2, 64]:
        out_conv, x2, then two OutConvBlocks without the last block's x2 up-sampling (mfr_eloftr_gather_windows evaluates it per window pixel)"""
        h = self.out_conv(coarse)
        for i, (f, res) in enumerate(zip(self.fine, (s2, s1))):
            r = self.upsample2x(h, add=f["c1"](res).contiguous())
            r = f["c2"](r, act=2)
            if i == 0:
                h = f["c3"](r)
            else:
                rows = f["c3"].rows(r)
                return rows if rows is not None else LoFTRHIP._fine_nhwc(None, f["c3"](r))

    def gather_windows(self, half, img_ids, cells, n, maxN, wc, win, pad):
        """half [nimg, Hh, Wh, 64]; img_ids [B] i32; cells [B, >= maxN] i32; n [B] i32 -> windows [B * maxN, win^2, 64] (zeros behind a pair's count)"""
        nimg, Hh, Wh, C = half.shape
        B = n.numel()
        out = torch.zeros(B * maxN, win * win, C, dtype=torch.float32, device=half.device)
        _lib.call("mfr_eloftr_gather_windows", half, nimg, Hh, Wh, C, img_ids, cells, cells.stride(0), n, B, maxN, wc, 8, win, pad, out)
        return out

    def fine_match(self, w0, w1, ci, cj, n, maxN, wc, return_arg=False):
        """windows -> pts0, pts1 [B, maxN, 2] in pixels of the padded frame (zeros behind a pair's count) [, the stage-1 arg-max index [B, maxN]]"""
        B = n.numel()
        pts0 = torch.zeros(B, maxN, 2, dtype=torch.float32, device=w0.device); pts1 = torch.zeros_like(pts0)
        arg = torch.full((B, maxN), -1, dtype=torch.int32, device=w0.device) if return_arg else None
        _lib.call("mfr_eloftr_fine_match", w0, w1, ci, cj, ci.stride(0), n, B, maxN, wc, 8, pts0, pts1, arg)
        return (pts0, pts1, arg) if return_arg else (pts0, pts1)

    def compact(self, pts0, pts1, conf, n, frame_hw):
        B, maxN = pts0.shape[:2]
        o0, o1 = torch.empty_like(pts0), torch.empty_like(pts1)
        oc = torch.empty(B, maxN, dtype=torch.float32, device=pts0.device)
        n_out = torch.empty(B, dtype=torch.int32, device=pts0.device)
        _lib.call("mfr_eloftr_compact", pts0, pts1, conf, conf.stride(0), n, B, maxN, int(frame_hw[1]), int(frame_hw[0]), o0, o1, oc, n_out)
        return o0, o1, oc, n_out

    # ------------------------------------------------------------------ full forward
    @staticmethod
    def pad(images):
        H, W = images.shape[-2:]
        ph, pw = (-H) % PAD_TO, (-W) % PAD_TO
        return F.pad(images, (0, pw, 0, ph)) if ph or pw else images

    @torch.no_grad()
    def __call__(self, images, maxN=None):
        """images [2B,1,H,W] (interleaved pairs, any H, W: zero-padded right / bottom to multiples of 32 here) -> dict(pts0, pts1 [B,maxN,2] in pixels of
        the unpadded frame, n_corr [B], mconf [B,maxN], i_ids, j_ids): LoFTRHIP's dictionary.  Matches in ascending image-0 cell index, the first maxN
        (default: every cell) refined, those with an end point at x >= W or y >= H dropped."""
        f, n = self.features(images), images.shape[0]
        return self.match_features(f, range(0, n, 2), f, range(1, n, 2), f.s3.shape[2] * 8, frame_hw=self.frame_hw or tuple(images.shape[-2:]), maxN=maxN)

    @torch.no_grad()
    def features(self, images):
        """images [n,1,H,W] -> ELoFTRFeatures of the zero-padded images.  Every backbone kernel tiles per image and sums in a fixed order, so an image's maps
        do not depend on what else is in the batch."""
        return self.backbone(self.pad(images).contiguous())

    @torch.no_grad()
    def match_features(self, src0, idx0, src1, idx1, H, frame_hw=None, maxN=None):
        """everything after the backbone for B = len(idx0) pairs; side s of pair p is image idx_s[p] of the feature set src_s (host sequences of ints).
        H: the padded image height; frame_hw: the unpadded (H, W) (None: the padded frame)."""
        B = len(idx0)
        hc, wc = src0.s3.shape[2:]
        assert len(idx1) == B and B > 0 and src1.s3.shape[1:] == src0.s3.shape[1:] and H == hc * 8
        L = hc * wc
        dev = src0.s3.device
        maxN = min(L, int(maxN or self.max_matches or L))
        xm = self.transformer(self.tokens(src0, idx0, src1, idx1), B, (hc, wc))
        f0, f1 = xm[0].view(B, L, 2 * HIDDEN)[..., :HIDDEN], xm[1].view(B, L, 2 * HIDDEN)[..., :HIDDEN]
        i_ids, j_ids, mconf, n = self.coarse_match_features(f0, f1, (hc, wc))
        # the residual maps in the token buffer's side-major order; slices and per-image views, no index tensor (an H2D copy would synchronise the stream)
        pick = lambda t, idx: t[idx.start:idx.stop:idx.step] if isinstance(idx, range) else torch.stack([t[i] for i in idx])
        half = self.pyramid(self.coarse_map(xm, 2 * B, (hc, wc)), torch.cat([pick(src0.s2, idx0), pick(src1.s2, idx1)]),
                            torch.cat([pick(src0.s1, idx0), pick(src1.s1, idx1)]))
        side = torch.arange(2 * B, dtype=torch.int32, device=dev)
        w0 = self.gather_windows(half, side[:B], i_ids, n, maxN, wc, 8, 0)
        w1 = self.gather_windows(half, side[B:], j_ids, n, maxN, wc, 10, 1)
        p0, p1 = self.fine_match(w0, w1, i_ids, j_ids, n, maxN, wc)
        o0, o1, oc, n_out = self.compact(p0, p1, mconf, n, frame_hw or self.frame_hw or (H, wc * 8))
        return dict(pts0=o0, pts1=o1, n_corr=n_out, mconf=oc, i_ids=i_ids, j_ids=j_ids, n_coarse=n)
