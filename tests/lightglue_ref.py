"""LightGlue oracle for the tests (CPU only, deterministic): the `transformers` LightGlue module built from its config -- no adaptive depth,
no adaptive width, eager attention -- as float32 and float64 twins on ONE state dict, the planted-twin inputs every LightGlue test uses, and
the module's stages called one by one so that a device stage can be fed the float32 oracle's tensors and compared with float64 on those
same tensors (the bar of tests/test_gpu_matcher_wiring.py).

`perturbed` does for nets/weights.lightglue_state_dict what tests/trained_like.py does for the other recipes: every zero bias and every
identity LayerNorm becomes non-trivial, so a device module that drops or swaps one of them no longer agrees with the oracle.  The last
assignment layer's peaky projection is kept (its bias is perturbed too): the gains are checked on the CPU oracle alone
(tests/test_lightglue_host.py: all planted twins still match, float32 and float64 agree, no score near the threshold)."""
import torch

H, W = 96, 128                      # image height, width
B, N = 2, 80                        # pairs, padded keypoints per image
COUNTS = [[80, 80], [65, 50]]       # valid keypoints (image 0, image 1) of each pair
TWINS = 40                          # the first 40 keypoints of image 1 are noisy copies of image 0's
THRESHOLD = 0.1
BIAS_STD = 0.02                     # = the std of the recipe's weights
LAYERS = 9


def perturbed(sd, seed=0):
    g = torch.Generator().manual_seed(int(seed))
    out = {k: v.clone() for k, v in sd.items()}
    for k in sorted(sd):
        if k.endswith("layer_norm.weight"):
            c = sd[k].numel()
            gamma = sd[k] * (0.7 + 0.6 * torch.rand(c, generator=g))
            out[k] = gamma
            out[k[:-len("weight")] + "bias"] = 0.3 * gamma.abs().mean() * torch.randn(c, generator=g)
    for k in sorted(sd):
        if k.endswith(".bias") and "layer_norm" not in k and not bool(sd[k].any()):
            out[k] = BIAS_STD * torch.randn(sd[k].numel(), generator=g)
    return out


def make_inputs(seed=0):
    """-> kpts [B, 2, N, 2] pixels (x, y), desc [B, 2, N, 256] unit norm, mask [B, 2, N] (1 = valid), counts [B, 2]; padded rows are zero"""
    g = torch.Generator().manual_seed(1000 + int(seed))
    size = torch.tensor([float(W), float(H)])
    kpts = torch.rand(B, 2, N, 2, generator=g) * (size - 8) + 4
    desc = torch.nn.functional.normalize(torch.randn(B, 2, N, 256, generator=g), dim=-1)
    kpts[:, 1, :TWINS] = kpts[:, 0, :TWINS] + 2.0 * torch.randn(B, TWINS, 2, generator=g)
    desc[:, 1, :TWINS] = torch.nn.functional.normalize(desc[:, 0, :TWINS] + 0.02 * torch.randn(B, TWINS, 256, generator=g), dim=-1)
    counts = torch.tensor(COUNTS, dtype=torch.int32)
    mask = (torch.arange(N)[None, None] < counts[:, :, None]).to(torch.int32)
    kpts = kpts * mask[..., None]
    desc = desc * mask[..., None]
    return kpts.contiguous(), desc.contiguous(), mask, counts


def make_models(sd):
    """float32 and float64 twins of LightGlueForKeypointMatching on one state dict (the detector it embeds keeps its own initialisation: unused)"""
    from transformers import LightGlueConfig, LightGlueForKeypointMatching
    out = []
    for dt in (torch.float32, torch.float64):
        cfg = LightGlueConfig(depth_confidence=-1.0, width_confidence=-1.0, filter_threshold=THRESHOLD, attn_implementation="eager")
        m = LightGlueForKeypointMatching(cfg).eval()
        missing, unexpected = m.load_state_dict(sd, strict=False)
        assert not unexpected and all(k.startswith("keypoint_detector.") for k in missing), (missing[:3], unexpected[:3])
        out.append(m.to(dt))
    return out


@torch.no_grad()
def run(m, kpts, desc, mask):
    """the whole matcher -> matches [2B, N] (rows 2p, 2p + 1 = images 0, 1 of pair p), matching_scores [2B, N], hidden states (63 tensors)"""
    dt = next(m.parameters()).dtype
    mt, sc, _, hs, _ = m._match_image_pair(kpts.to(dt), desc.to(dt), H, W, mask=mask, output_hidden_states=True)
    return mt, sc, hs


# ---- the module's stages, one by one (x [2B, N, 256] in the module's dtype) ----
def _additive(mask2, dt):
    return torch.zeros(mask2.shape, dtype=dt).masked_fill(mask2 == 0, torch.finfo(dt).min)[:, None, None, :]


@torch.no_grad()
def rotary(m, kpts):
    """-> (cos, sin) [2B, N, 64] of the normalised keypoints"""
    from transformers.models.lightglue.modeling_lightglue import normalize_keypoints
    dt = next(m.parameters()).dtype
    return m.positional_encoder(normalize_keypoints(kpts.to(dt).reshape(2 * B, N, 2), H, W))[0]


@torch.no_grad()
def rotated_qk(m, l, x, cs):
    """q, k [2B, N, 256] (head-major channels) of layer l's self attention after the rotary encoding"""
    from transformers.models.lightglue.modeling_lightglue import apply_rotary_pos_emb
    att = m.transformer_layers[l].self_attention
    q = att.q_proj(x).view(2 * B, N, 4, 64).transpose(1, 2)
    k = att.k_proj(x).view(2 * B, N, 4, 64).transpose(1, 2)
    q, k = apply_rotary_pos_emb(q, k, cs[0], cs[1])
    return q.transpose(1, 2).reshape(2 * B, N, 256), k.transpose(1, 2).reshape(2 * B, N, 256)


@torch.no_grad()
def self_block(m, l, x, cs, mask):
    layer = m.transformer_layers[l]
    a, _ = layer.self_attention(x, position_embeddings=cs, attention_mask=_additive(mask.reshape(2 * B, N), x.dtype))
    return x + layer.self_mlp(torch.cat([x, a], -1))


@torch.no_grad()
def cross_block(m, l, x, mask):
    layer = m.transformer_layers[l]
    other = x.reshape(B, 2, N, 256).flip(1).reshape(2 * B, N, 256)
    a, _ = layer.cross_attention(x, encoder_hidden_states=other, encoder_attention_mask=_additive(mask.flip(1).reshape(2 * B, N), x.dtype))
    return x + layer.cross_mlp(torch.cat([x, a], -1))


@torch.no_grad()
def similarity(m, x):
    """-> S [B, N, N] (unmasked), z0, z1 [B, N] of the last assignment layer"""
    lay = m.match_assignment_layers[LAYERS - 1]
    md = (lay.final_projection(x) / 4.0).reshape(B, 2, N, 256)
    z = lay.matchability(x).reshape(B, 2, N)
    return md[:, 0] @ md[:, 1].transpose(1, 2), z[:, 0], z[:, 1]


@torch.no_grad()
def assign64(S, z0, z1, n0, n1, threshold=THRESHOLD):
    """float64 sigmoid_log_double_softmax + get_matches_from_scores on S [b, N0, N1] with the module's masking -> matches0 [b, N0], matches1 [b, N1],
    scores0, scores1, and the log-assignment block [b, N0, N1] (for the safe rule)"""
    from transformers.models.lightglue.modeling_lightglue import get_matches_from_scores, sigmoid_log_double_softmax
    b, N0, N1 = S.shape
    assert N0 == N1, "the module stacks the two sides: square padded blocks only"
    S, z0, z1 = S.double(), z0.double(), z1.double()
    valid = (torch.arange(N0)[None, :, None] < n0[:, None, None]) & (torch.arange(N1)[None, None, :] < n1[:, None, None])
    sc = sigmoid_log_double_softmax(S.masked_fill(~valid, torch.finfo(S.dtype).min), z0[..., None], z1[..., None])
    mt, ms = get_matches_from_scores(sc, threshold)
    mt, ms = mt.reshape(b, 2, N0), ms.reshape(b, 2, N0)
    return mt[:, 0], mt[:, 1], ms[:, 0], ms[:, 1], sc[:, :-1, :-1]


def safe_masks(logp, n0, n1, threshold=THRESHOLD, gap=1e-3):
    """the keypoints on which two correct evaluations must agree: valid, float64 best and second-best log-score along the row (image 0) / column
    (image 1) at least `gap` apart, and exp(best) at least `gap` from the threshold.  -> safe0 [b, N0], safe1 [b, N1] bool"""
    b, N0, N1 = logp.shape
    out = []
    for dim, cnt_self, cnt_other, L in ((2, n0, n1, N0), (1, n1, n0, N1)):
        ok_other = torch.arange(logp.shape[dim])[None] < cnt_other[:, None]
        lp = logp.masked_fill(~(ok_other[:, None, :] if dim == 2 else ok_other[:, :, None]), -float("inf"))
        k = min(2, lp.shape[dim])
        top = lp.topk(k, dim=dim).values
        best = top.select(dim, 0)
        second = top.select(dim, 1) if k == 2 else torch.full_like(best, -float("inf"))
        safe = (best - second >= gap) & ((best.exp() - threshold).abs() >= gap)
        safe &= (torch.arange(L)[None] < cnt_self[:, None]) & (cnt_other[:, None] > 0)
        out.append(safe)
    return out[0], out[1]
