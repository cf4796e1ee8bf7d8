"""LightGlue (Lindenberger, Sarlin, Pollefeys, ICCV 2023) on MI355X for SuperPoint features: 9 layers of self + cross attention with rotary
positional encoding, then double softmax + matchability.  No adaptive depth (early exit) and no adaptive width (point pruning): the stage
is a fixed sequence of launches without host synchronisation, batched like nets/superglue.py.

The reference has no LightGlue; this stage takes SuperGlue_matcher's place (etc/feature_matching_baselines/matchers.py:62-120) and returns
the same dictionary as SuperGlueHIP.__call__, so the solvers and the npz wire format take it unchanged.  State-dict keys are those of the
`transformers` LightGlue module (`positional_encoder.projector`, `transformer_layers.{i}.self_attention.q_proj` ...,
`match_assignment_layers.{i}.final_projection` / `.matchability`); `token_confidence.*` and the assignment layers before the last are
accepted and unused.  Parity with the PUBLISHED LightGlue weights is unpinned: no checkpoint exists offline (see `from_upstream`).

Layout is token-major [2B, K, 256] (image 2p = reference view, 2p + 1 = query view of pair p); a head is the contiguous 64-channel slice
the module's `view(..., 4, 64)` makes, which is what csrc/attention.hip reads.  Linear layers: csrc/gemm_split.hip (HIP.SPLIT arithmetic,
range guard); attention: mfr_sg_attention; rotary encoding, LayerNorm + GELU and the assignment: csrc/lightglue.hip.
"""
import torch

from .. import _lib, options
from .linear import SplitBatchedNT, SplitLinear


# How the MLP's LayerNorm + GELU run (LightGlueHIP's `mlp`).  'pass': fc1 by the default split GEMM, then mfr_lg_ln_gelu in place; 'epilogue': fc1 with
# both in its epilogue (mfr_gemm_*_ln_gelu, hidden row written once).  Measured per launch on 65536 rows (profiles/lightglue_stage.json, f16x2):
# 0.105 + 0.043 ms against 0.264 ms -- holding four accumulator blocks leaves one workgroup per CU and the register-staged K loop then runs at about
# a third of the LDS-DMA kernel's rate, which costs more than the saved pass over the hidden rows.  So the default is 'pass'; both are tested.
MLP_DEFAULT = "pass"


def fold_weights(state_dict, n_layers=9):
    """Module parameters -> the f32 operands the GPU path multiplies with (pure host code, float64 re-associations):
      * q, k, v projections of a block concatenated into one [768, 256] product;
      * o_proj only feeds fc1:  fc1 [x ; Wo a + bo] = [W1x | W1m Wo] [x ; a] + (b1 + W1m bo)  -> one 256 x 256 GEMM per block disappears and
        [x | a] is a single buffer the attention kernel writes into;
      * the last layer's final_projection scaled by 256^(-1/4) = 1/4 (a power of two: exact) and stacked on `matchability`: one [257, 256] product
        gives the scaled match descriptors and the matchability logit.
    Returns dict(wr, blocks=[dict(wqkv, bqkv, w1, b1, ln_g, ln_b, w2, b2, cross)...], wfz, bfz)."""
    sd = {k: v.double() for k, v in state_dict.items()}
    f32 = lambda t: t.float().contiguous()
    blocks = []
    for l in range(n_layers):
        for kind, cross in (("self", False), ("cross", True)):
            a, m = f"transformer_layers.{l}.{kind}_attention", f"transformer_layers.{l}.{kind}_mlp"
            wqkv = torch.cat([sd[f"{a}.{n}_proj.weight"] for n in "qkv"], 0)
            bqkv = torch.cat([sd[f"{a}.{n}_proj.bias"] for n in "qkv"], 0)
            w1, b1 = sd[f"{m}.fc1.weight"], sd[f"{m}.fc1.bias"]
            w1x, w1m = w1[:, :256], w1[:, 256:]
            blocks.append(dict(wqkv=f32(wqkv), bqkv=f32(bqkv), w1=f32(torch.cat([w1x, w1m @ sd[f"{a}.o_proj.weight"]], 1)),
                               b1=f32(b1 + w1m @ sd[f"{a}.o_proj.bias"]), ln_g=f32(sd[f"{m}.layer_norm.weight"]), ln_b=f32(sd[f"{m}.layer_norm.bias"]),
                               w2=f32(sd[f"{m}.fc2.weight"]), b2=f32(sd[f"{m}.fc2.bias"]), cross=cross))
    p = f"match_assignment_layers.{n_layers - 1}"
    wfz = torch.cat([sd[f"{p}.final_projection.weight"] * 0.25, sd[f"{p}.matchability.weight"]], 0)
    bfz = torch.cat([sd[f"{p}.final_projection.bias"] * 0.25, sd[f"{p}.matchability.bias"]], 0)
    return dict(wr=f32(sd["positional_encoder.projector.weight"]), blocks=blocks, wfz=f32(wfz), bfz=f32(bfz))


def from_upstream(sd, n_layers=9):
    """cvg/LightGlue checkpoint names -> the `transformers` names this module loads.  UNPINNED: no upstream checkpoint exists offline, so only
    the renaming and the tensor re-arrangement are tested (a CPU round trip, tests/test_lightglue_host.py), not parity with a published file.
    Upstream packs a self block's q, k, v as `self_attn.Wqkv` with output channel (head, dim, 3) and shares one projection for the cross block's
    queries and keys (`cross_attn.to_qk`); `log_assignment.{i}.final_proj` / `.matchability`, `posenc.Wr`, `token_confidence.{i}.token.0`."""
    out = {"positional_encoder.projector.weight": sd["posenc.Wr.weight"]}
    for l in range(n_layers):
        u, t = f"transformers.{l}", f"transformer_layers.{l}"
        wqkv, bqkv = sd[f"{u}.self_attn.Wqkv.weight"], sd[f"{u}.self_attn.Wqkv.bias"]
        for j, n in enumerate("qkv"):
            out[f"{t}.self_attention.{n}_proj.weight"] = wqkv.reshape(256, 3, 256)[:, j].contiguous()
            out[f"{t}.self_attention.{n}_proj.bias"] = bqkv.reshape(256, 3)[:, j].contiguous()
        out[f"{t}.self_attention.o_proj.weight"], out[f"{t}.self_attention.o_proj.bias"] = sd[f"{u}.self_attn.out_proj.weight"], sd[f"{u}.self_attn.out_proj.bias"]
        for n, src in (("q", "to_qk"), ("k", "to_qk"), ("v", "to_v"), ("o", "to_out")):
            out[f"{t}.cross_attention.{n}_proj.weight"], out[f"{t}.cross_attention.{n}_proj.bias"] = sd[f"{u}.cross_attn.{src}.weight"], sd[f"{u}.cross_attn.{src}.bias"]
        for kind, src in (("self", "self_attn"), ("cross", "cross_attn")):
            for dst, i in (("fc1", 0), ("layer_norm", 1), ("fc2", 3)):
                for wb in ("weight", "bias"):
                    out[f"{t}.{kind}_mlp.{dst}.{wb}"] = sd[f"{u}.{src}.ffn.{i}.{wb}"]
        for dst, src in (("final_projection", "final_proj"), ("matchability", "matchability")):
            for wb in ("weight", "bias"):
                out[f"match_assignment_layers.{l}.{dst}.{wb}"] = sd[f"log_assignment.{l}.{src}.{wb}"]
        if l < n_layers - 1:
            for wb in ("weight", "bias"):
                out[f"token_confidence.{l}.token.{wb}"] = sd[f"token_confidence.{l}.token.0.{wb}"]
    return out


def check_cfg(cfg):
    """the LIGHTGLUE node of a config: only the fixed-depth, fixed-width network is built"""
    lg = cfg.LIGHTGLUE
    for key in ("DEPTH_CONFIDENCE", "WIDTH_CONFIDENCE"):
        if float(lg[key]) != -1.0:
            raise ValueError(f"LIGHTGLUE.{key} = {lg[key]!r}: adaptive depth (early exit) and adaptive width (point pruning) are out of scope of "
                             f"this LightGlue stage; only -1 (off) is supported")
    return lg


def from_cfg(cfg, device):
    """-> (SuperPointHIP, LightGlueHIP) of a config (LIGHTGLUE.*; SuperPoint's weights are the SuperGlue stage's: SUPERGLUE.SUPERPOINT_WEIGHTS)"""
    from . import weights as WT
    from .superglue import superpoint_from_cfg
    lg = check_cfg(cfg)
    sp = superpoint_from_cfg(cfg, device, lg)
    return sp, LightGlueHIP(WT.from_cfg("LightGlue", cfg, lg.WEIGHTS, WT.lightglue_state_dict), device, lg.FILTER_THRESHOLD, lg.NUM_LAYERS)


class Assignment:
    """LightGlue's match assignment on a similarity matrix (mfr_lg_assign, csrc/lightglue.hip): double softmax + matchability, mutual arg-max,
    exp(score) > threshold.  Keeps the kernel's workspace (one allocation per size)."""

    def __init__(self, threshold=0.1):
        _lib.load(require_gpu=True)
        self.thr, self._ws = float(threshold), None

    def __call__(self, S, z0, z1, n0, n1, kpts0=None, kpts1=None, maxN=None):
        """mfr_lg_assign on S [B, N0, ldS] (a view with ldS = S.stride(1) >= N1 is used in place)"""
        lib = _lib.load()
        B, N0, N1 = S.shape
        assert S.stride(2) == 1 and S.stride(0) == N0 * S.stride(1) and S.dtype == torch.float32
        dev = S.device
        need = lib.mfr_lg_assign_workspace_bytes(B, N0, N1)
        if self._ws is None or self._ws.numel() < need or self._ws.device != dev:
            self._ws = torch.empty(need, dtype=torch.uint8, device=dev)
        m0 = torch.empty(B, N0, dtype=torch.int32, device=dev)
        m1 = torch.empty(B, N1, dtype=torch.int32, device=dev)
        ms0 = torch.empty(B, N0, dtype=torch.float32, device=dev)
        ms1 = torch.empty(B, N1, dtype=torch.float32, device=dev)
        out = dict(matches0=m0, matches1=m1, matching_scores0=ms0, matching_scores1=ms1)
        pts0 = pts1 = nc = None
        K = 0
        if kpts0 is not None:
            K = kpts0.shape[1]
            maxN = maxN or N0
            pts0 = torch.zeros(B, maxN, 2, dtype=torch.float32, device=dev)
            pts1 = torch.zeros(B, maxN, 2, dtype=torch.float32, device=dev)
            nc = torch.empty(B, dtype=torch.int32, device=dev)
            kpts0, kpts1 = kpts0.contiguous(), kpts1.contiguous()
            out.update(pts0=pts0, pts1=pts1, n_corr=nc)
        _lib.call("mfr_lg_assign", S.data_ptr(), B, N0, N1, S.stride(1), z0.contiguous(), z1.contiguous(), n0, n1, self.thr, kpts0, kpts1, K,
                  self._ws, self._ws.numel(), m0, m1, ms0, ms1, pts0, pts1, maxN or 0, nc)
        return out


class LightGlueHIP:
    def __init__(self, state_dict, device="cuda", filter_threshold=0.1, n_layers=9, mlp=MLP_DEFAULT):
        """mlp: 'epilogue' = LayerNorm + GELU in fc1's epilogue (mfr_gemm_*_ln_gelu) | 'pass' = fc1, then mfr_lg_ln_gelu in place (A/B, tests)"""
        _lib.load(require_gpu=True)
        assert mlp in ("epilogue", "pass")
        self.mlp = mlp
        self.device = torch.device(device)
        self.thr, self.n_layers = float(filter_threshold), int(n_layers)
        self.att_variant = 0 if options.get("SPLIT") == "f16x2" else 2       # the arithmetic of the attention kernel, resolved once (options.py)
        fw = fold_weights(state_dict, n_layers)
        dev = lambda t: t.to(self.device).contiguous()
        self.wr = dev(fw["wr"])
        self.blocks = []
        for L in fw["blocks"]:
            self.blocks.append(dict(lin_qkv=SplitLinear(dev(L["wqkv"]), dev(L["bqkv"])), lin1=SplitLinear(dev(L["w1"]), dev(L["b1"])),
                                    lin2=SplitLinear(dev(L["w2"]), dev(L["b2"])), ln=(dev(L["ln_g"]), dev(L["ln_b"])), cross=L["cross"]))
        self.lin_final = SplitLinear(dev(fw["wfz"]), dev(fw["bfz"]))
        self.score_gemm = SplitBatchedNT() if self.lin_final.split == "f16x2" else None      # (the bf16x3 arithmetic keeps the library's batched fp32 GEMM)
        self.assign = Assignment(self.thr)
        self._size = {}

    # ---- stages (each one is what the stage-level tests call) ----
    def rotary_table(self, kn):
        """normalised keypoints [B2, K, 2] -> cs [B2 * K, 64] = (cos | sin) of the 32 angles"""
        M = kn.shape[0] * kn.shape[1]
        cs = torch.empty(M, 64, dtype=torch.float32, device=kn.device)
        _lib.call("mfr_lg_rotary_table", kn.contiguous(), self.wr, M, cs)
        return cs

    def rotate(self, qkv, cs):
        """qkv [M, 768] (q | k | v): q and k rotated in place"""
        base = qkv.data_ptr()
        _lib.call("mfr_lg_rotary_apply", base, base + 256 * 4, qkv.stride(0), qkv.shape[0], cs)
        return qkv

    def attention(self, qkv, n_tok, cross, out, ldo):
        B2, K, _ = qkv.shape
        base = qkv.data_ptr()
        _lib.call("mfr_sg_attention_variant", base, base + 256 * 4, base + 512 * 4, 768, B2, K, 4, n_tok, 1 if cross else 0, out.data_ptr(), ldo, self.att_variant)
        return out

    def block(self, L, xa, qkv, hid, cs, n, B2, K):
        """one self / cross block on xa = [x | a] [B2 * K, 512], in place: x += fc2(GELU(LN(fc1([x | attention(x)]))))"""
        xv, av = xa[:, :256], xa[:, 256:]
        L["lin_qkv"](xv, out=qkv)
        if not L["cross"]:
            self.rotate(qkv, cs)
        self.attention(qkv.view(B2, K, 768), n, L["cross"], av, 512)
        if self.mlp == "epilogue":
            L["lin1"].ln_gelu(xa, L["ln"], hid)
        else:
            L["lin1"](xa, out=hid)
            _lib.call("mfr_lg_ln_gelu", hid.data_ptr(), hid.stride(0), hid.shape[0], L["ln"][0], L["ln"][1], 1e-5)
        L["lin2"](hid, out=xv, accumulate=True)                           # x += W2 hid + b2, in place
        return xa

    def normalize_keypoints(self, kpts, image_hw):
        H, W = image_hw
        key = (H, W, kpts.device)
        if key not in self._size:
            self._size[key] = torch.tensor([float(W), float(H)], device=kpts.device)
        return (kpts - self._size[key] / 2) / (float(max(W, H)) / 2)                  # LightGlue's: max(W, H) / 2, not SuperGlue's 0.7 max

    @torch.no_grad()
    def final_descriptors(self, kpts, desc, n, image_hw):
        """-> the descriptors after all layers, [B2, K, 256]"""
        B2, K, _ = kpts.shape
        cs = self.rotary_table(self.normalize_keypoints(kpts, image_hw))
        xa = torch.empty(B2 * K, 512, dtype=torch.float32, device=kpts.device)
        xa[:, :256].copy_(desc.reshape(B2 * K, 256))
        qkv = torch.empty(B2 * K, 768, dtype=torch.float32, device=kpts.device)
        hid = torch.empty(B2 * K, 512, dtype=torch.float32, device=kpts.device)
        for L in self.blocks:
            self.block(L, xa, qkv, hid, cs, n, B2, K)
        return xa[:, :256].view(B2, K, 256)

    @torch.no_grad()
    def similarity(self, x):
        """descriptors [B2, K, 256] (any row stride) -> S [B, K, K] = m0 m1^T of the scaled final projections, z0, z1 [B, K] matchability logits"""
        B2, K, _ = x.shape
        mdz = torch.empty(B2 * K, 260, dtype=torch.float32, device=x.device)            # 257 columns; rows stay 16-byte aligned
        self.lin_final(x.reshape(B2 * K, 256), out=mdz[:, :257])                         # (a view of the [x | a] buffer: no copy)
        md = mdz.view(B2, K, 260)[:, :, :256]
        z = mdz.view(B2, K, 260)[:, :, 256]
        if self.score_gemm is not None:
            S = self.score_gemm(md[0::2], md[1::2])
        else:
            S = torch.bmm(md[0::2], md[1::2].transpose(1, 2))
        return S, z[0::2].contiguous(), z[1::2].contiguous()

    @torch.no_grad()
    def __call__(self, sp_out, image_hw, maxN=None):
        """sp_out: SuperPointHIP output for the interleaved [2B] images (scores are not used) -> dict(pts0, pts1 [B,maxN,2], n_corr [B],
        matches0 / matches1, matching_scores0 / matching_scores1)"""
        kpts, desc, n = sp_out["kpts"], sp_out["desc"], sp_out["n"]
        x = self.final_descriptors(kpts, desc, n, image_hw)
        S, z0, z1 = self.similarity(x)
        return self.assign(S, z0, z1, n[0::2].contiguous(), n[1::2].contiguous(), kpts[0::2], kpts[1::2], maxN)
