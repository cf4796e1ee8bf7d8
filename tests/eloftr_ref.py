"""The CPU oracle of the EfficientLoFTR stage: the `transformers` module EfficientLoFTRForKeypointMatching in float32 and float64, cut into the
stages nets/eloftr.py has (backbone, aggregation, rotary, self block, cross pair, transformer, fine pyramid, windows, coarse matching, two-stage
fine matching), the test inputs, and the SAFE masks of the discrete decisions.

Every stage function calls the module's own sub-modules / methods on tensors it is GIVEN, so the device stage and the float64 oracle can be fed
the float32 oracle's inputs: one stage's round-off is not the next one's input.

Two things the whole module does that only show with B > 1 or non-mutual slots are NOT the oracle's (nets/eloftr.py states them): the fine stage is
evaluated here per MATCH (i, j) -- the module's slot s pairs the image-0 partner of column s with the image-1 partner of row s -- and per pair (the
module takes the second-stage expectation of batch element 0 for the whole batch); and the first stage's two softmaxes run over each match's own
64 x 100 matrix (see fine_confidences) and the first-stage offsets are gathered along the window axis (see fine_match).  The second stage is the
module's own method, on a batch of one.

Images are interleaved [2B,1,H,W] (2p = image 0 of pair p) as LoFTRHIP / EfficientLoFTRHIP take them."""
import functools
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FACTOR = 10.0                       # err(device) <= FACTOR x err(float32 oracle): the project's bar (tests/test_gpu_matcher_wiring.py)
COORD_FLOOR = 1e-3                  # px: the coordinate bar of tests/test_gpu_loftr_parity.py
SAFE_REL = 1e-3
SHAPES = ((96, 128), (160, 96))     # coarse 12 x 16 / aggregated 3 x 4; coarse 20 x 12 / aggregated 5 x 3 (odd height)


def module(sd, dtype=torch.float32):
    from transformers import EfficientLoFTRConfig, EfficientLoFTRForKeypointMatching
    m = EfficientLoFTRForKeypointMatching(EfficientLoFTRConfig()).eval()
    m.load_state_dict(sd, strict=True)
    return m.to(dtype)


def perturbed(sd, seed=11):
    """a copy of a state dict in which every BatchNorm and LayerNorm term has moved again (the way tests/trained_like.py does it for the other nets):
    gains x U(0.8, 1.25), biases and running means shifted, running variances x U(0.6, 1.6), and ONE channel of the first identity branch with a
    running variance of ~1e-3 (where eps = 1e-5 is 1 % of the variance: a fold that forgets eps, or adds it twice, shows)."""
    g = torch.Generator().manual_seed(seed)
    out = {k: v.clone() for k, v in sd.items()}
    u = lambda n, lo, hi: lo + (hi - lo) * torch.rand(n, generator=g)
    for k in sd:
        if k.endswith("running_var"):
            p, c = k[:-len("running_var")], sd[k].numel()
            s = sd[k].sqrt()
            out[k] = sd[k] * u(c, 0.6, 1.6)
            out[p + "running_mean"] = sd[p + "running_mean"] + 0.1 * s * torch.randn(c, generator=g)
            out[p + "weight"] = sd[p + "weight"] * u(c, 0.8, 1.25)
            out[p + "bias"] = sd[p + "bias"] + 0.02 * torch.randn(c, generator=g)
        elif "norm.weight" in k and "aggregation" in k or k.endswith("layer_norm.weight"):
            out[k] = sd[k] * u(sd[k].numel(), 0.9, 1.1)
        elif "norm.bias" in k and "aggregation" in k or k.endswith("layer_norm.bias"):
            out[k] = sd[k] + 0.01 * torch.randn(sd[k].numel(), generator=g)
    p = "efficientloftr.backbone.stages.1.blocks.0.identity."
    ratio = 1e-3 / out[p + "running_var"][3]
    out[p + "running_var"][3] = 1e-3
    out[p + "weight"][3] *= ratio.sqrt()                    # the channel's output keeps its scale
    return out


@functools.lru_cache(maxsize=None)
def weights(which="recipe"):
    from mapfree_reloc_amd.nets import weights as WT
    sd = WT.eloftr_state_dict()
    return perturbed(sd) if which == "perturbed" else sd


@functools.lru_cache(maxsize=None)
def modules(which="perturbed"):
    sd = weights(which)
    return module(sd, torch.float32), module(sd, torch.float64)


def noise_pair(hw, seed, sigma=0.01):
    """uniform noise and the same image + N(0, sigma^2): the pair on which the recipe's local features match cell to cell"""
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(1, 1, *hw, generator=g)
    return torch.cat([a, (a + sigma * torch.randn(1, 1, *hw, generator=g)).clamp(0, 1)])


def end_to_end_images(hw=(160, 128)):
    """[4,1,H,W]: the near-identical pair and a second, different pair (another image, 3 x the noise) in the same batch"""
    return torch.cat([noise_pair(hw, 5), noise_pair(hw, 6, 0.03)])


def px(images, dtype):
    """interleaved gray planes -> the module's pixel_values [B,2,3,H,W]"""
    n, _, H, W = images.shape
    return images.to(dtype).reshape(n // 2, 2, 1, H, W).expand(-1, -1, 3, -1, -1).contiguous()


# ---------------------------------------------------------------------------------------------------- continuous stages
def backbone(m, x):
    """x [n,1,H,W] -> [s1, s2, s3]"""
    return m.efficientloftr.backbone(x)


def block_of(m, l, kind):
    return getattr(m.efficientloftr.local_feature_transformer.layers[l], f"{kind}_attention")


def aggregation(m, l, kind, x, enc=None):
    """-> (q tokens, kv tokens) [n, ha wa, 256] after the shared LayerNorm"""
    q, kv = block_of(m, l, kind).aggregation(x, enc)
    return q.reshape(x.shape[0], -1, 256), kv.reshape(x.shape[0], -1, 256)


def position_embeddings(m, x):
    cos, sin = m.efficientloftr.rotary_emb(x)
    n = x.shape[0]
    return (cos.to(x.dtype).expand(n, -1, -1, -1).reshape(n, -1, 256), sin.to(x.dtype).expand(n, -1, -1, -1).reshape(n, -1, 256))


def rotary_qk(m, l, q_tok, kv_tok, x):
    """projected and rotated q, k [n, La, 256] of self block l"""
    from transformers.models.efficientloftr.modeling_efficientloftr import apply_rotary_pos_emb
    att = block_of(m, l, "self").attention
    n, La, _ = q_tok.shape
    cos, sin = position_embeddings(m, x)
    q, k = apply_rotary_pos_emb(att.q_proj(q_tok).view(n, La, -1, 256), att.k_proj(kv_tok).view(n, La, -1, 256), cos, sin, unsqueeze_dim=2)
    return q.reshape(n, La, 256).to(q_tok.dtype), k.reshape(n, La, 256).to(q_tok.dtype)


def self_block(m, l, x):
    return block_of(m, l, "self")(x, position_embeddings=position_embeddings(m, x))


def cross_pair(m, l, x0, x1):
    """image 0 attends to image 1, then image 1 to the UPDATED image 0"""
    c = block_of(m, l, "cross")
    y0 = c(x0, x1)
    return y0, c(x1, y0)


def transformer(m, s3):
    """s3 [2B,256,h,w] interleaved -> the same layout after the 4 layers"""
    n, C, h, w = s3.shape
    return m.efficientloftr.local_feature_transformer(s3.reshape(n // 2, 2, C, h, w), position_embeddings=position_embeddings(m, s3)).reshape(n, C, h, w)


def pyramid_half(m, coarse, s2, s1):
    """coarse [n,256,h,w] (NOT yet / 16), the 1/4 and 1/2 maps -> the 64-channel map at HALF resolution, i.e. the pyramid before its last x2 up-sampling"""
    rl = m.refinement_layer
    up = lambda t: torch.nn.functional.interpolate(t, scale_factor=2.0, mode="bilinear", align_corners=False)
    h = rl.out_conv_layers[0](up(rl.out_conv(coarse / 256 ** 0.5)), s2)
    b = rl.out_conv_layers[1]
    return b.out_conv3(b.activation(b.batch_norm(b.out_conv2(b.out_conv1(s1) + h))))


def windows(m, coarse, s2, s1):
    """the module's refinement layer: every cell's windows, ([B, L, 64, 64], [B, L, 100, 64]) for interleaved inputs"""
    n, C, h, w = coarse.shape
    return m.refinement_layer((coarse / 256 ** 0.5).reshape(n // 2, 2, C, h, w), [s1, s2])                 # the layer reverses the list itself


def to_side_major(t):
    """interleaved [2B, ...] -> side-major [2B, ...] (all images 0, then all images 1)"""
    return torch.cat([t[0::2], t[1::2]])


# ---------------------------------------------------------------------------------------------------- coarse matching
def coarse_confidence(f0, f1, temperature=0.1):
    """the module's `_coarse_matching` up to the confidence matrix: f [B, L, 256] token-major"""
    sim = (f0 / f0.shape[-1] ** 0.5) @ (f1 / f1.shape[-1] ** 0.5).transpose(-1, -2) / temperature
    return torch.softmax(sim, 1) * torch.softmax(sim, 2)


def coarse_matches(m, conf, hw):
    """the module's threshold / border / mutual-maximum selection: j [B, L] (-1: no match) per image-0 cell, and the confidences"""
    # one pair at a time: the module concatenates the two index tensors along the batch axis before it reshapes them to [B, 2, L], which mixes the
    # pairs of a batch of more than one
    out = [m._get_matches_from_scores(c.reshape(1, hw[0], hw[1], hw[0], hw[1]).clone()) for c in conf]
    return torch.cat([idx[:, 1] for idx, _ in out]), torch.cat([score[:, 1] for _, score in out])


def coarse_safe(conf64, thr=0.2, rel=SAFE_REL):
    """SAFE image-0 cells: float64 best and second best along the cell's row, and along its best column, differ by >= rel (relative), and the best
    confidence is >= rel away from the threshold"""
    top = conf64.topk(2, dim=2).values
    j = conf64.argmax(2)
    col = conf64.transpose(1, 2).gather(1, j[..., None].expand(-1, -1, conf64.shape[1]))          # [B, L, L0]: column j(i)
    ctop = col.topk(2, dim=2).values
    gap = lambda t: (t[..., 0] - t[..., 1]) >= rel * t[..., 0]
    return gap(top) & gap(ctop) & ((top[..., 0] - thr).abs() >= rel)


def constructed_coarse(hw, B=2, seed=3, dim=256, lo=10.0, hi=17.0, noise=0.02):
    """coarse features for the matcher alone: image 1's rows are a seeded permutation of image 0's plus noise.  A true pair's similarity is
    |f|^2 / 25.6 (both sides / 16, temperature 0.1) against a background of about |f|^2 / 410, so with the rows' norms spread over [lo, hi] the
    float64 confidences of true pairs run from ~0.05 to ~0.98: most exceed the threshold 0.2, some sit near it"""
    g = torch.Generator().manual_seed(seed)
    L = hw[0] * hw[1]
    f0 = torch.randn(B, L, dim, generator=g, dtype=torch.float64)
    norms = lo + (hi - lo) * torch.rand(B, L, 1, generator=g, dtype=torch.float64)
    f0 = f0 / f0.norm(dim=-1, keepdim=True) * norms
    perm = torch.stack([torch.randperm(L, generator=g) for _ in range(B)])
    n1 = f0 + noise * norms * torch.randn(B, L, dim, generator=g, dtype=torch.float64) / dim ** 0.5
    f1 = torch.empty_like(f0)
    for b in range(B):
        f1[b, perm[b]] = n1[b]
    return f0, f1, perm


# ---------------------------------------------------------------------------------------------------- fine matching
def constructed_windows(M=48, seed=9, noise=0.05):
    """windows for the fine matcher alone: image 1's 10 x 10 window holds image 0's 8 x 8 features displaced by a known (dx, dy) in [-3, 3]^2 plus noise.
    The first matches force the stage-1 winner onto row 0, column 0 (the wrap-around read of stage 2), row 7 and column 7 of the 8 x 8 grid by boosting
    one feature of image 0 there.  Returns w0 [M, 64, 64], w1 [M, 100, 64] float64 and the cells ci, cj [M]."""
    g = torch.Generator().manual_seed(seed)
    field = torch.randn(M, 20, 20, 64, generator=g, dtype=torch.float64) * 1.5           # a true partner scores ~2.25 +- 0.4 against a background of 0 +- 0.3: no saturated ties
    w0 = torch.empty(M, 8, 8, 64, dtype=torch.float64); w1 = torch.empty(M, 10, 10, 64, dtype=torch.float64)
    d = torch.randint(-3, 4, (M, 2), generator=g)
    corners = [(0, 0), (0, 5), (5, 0), (7, 7), (7, 2), (2, 7), (0, 7), (7, 0)]
    for k in range(M):
        dx, dy = int(d[k, 0]), int(d[k, 1])
        w0[k] = field[k, 6:14, 6:14]
        w1[k] = field[k, 5 + dy:15 + dy, 5 + dx:15 + dx]
        if k < 2 * len(corners):
            # a winner with its image-1 partner at (r, c) of the interior grid: zero displacement, one boosted feature
            r, c = corners[k % len(corners)]
            w1[k] = field[k, 5:15, 5:15]
            w0[k, r, c, :56] *= 1.6
            w1[k, r + 1, c + 1, :56] *= 1.6
    w1 = w1 + noise * torch.randn(w1.shape, generator=g, dtype=torch.float64)
    ci = torch.randint(0, 192, (M,), generator=g); cj = torch.randint(0, 192, (M,), generator=g)
    return w0.reshape(M, 64, 64), w1.reshape(M, 100, 64), ci, cj


def fine_confidences(w0, w1):
    """first- and second-stage confidences of M matches, w0 [M, 64, 64], w1 [M, 100, 64]: `_fine_matching`'s arithmetic line by line, with the
    two softmaxes of the first stage over the 64 and the 100 axis of each match's OWN 64 x 100 matrix.  (Called on its 4-D tensors the module's
    `softmax(.., 1) * softmax(.., 2)` runs over the match axis and the 64 axis instead -- a match's refinement would depend on every other cell of
    the image; the per-match form is the one the paper and upstream's 3-D tensors have, and the one the device kernel computes.)"""
    a, b = w0[..., :56] / 56 ** 0.5, w1[..., :56] / 56 ** 0.5
    c = a @ b.transpose(-1, -2)
    c = torch.softmax(c, 1) * torch.softmax(c, 2)
    first = c.reshape(-1, 64, 10, 10)[..., 1:-1, 1:-1].reshape(-1, 64, 64)
    second = w0[..., 56:] @ (w1[..., 56:] / 8 ** 0.5).transpose(-1, -2)
    return first, second


def fine_match(m, w0, w1, ci, cj, wc):
    """M matches -> pts0, pts1 [M, 2] in pixels (coarse key point = the cell's corner).  First stage: arg-max over the flattened 64 x 64 and the
    offsets grid[index] - 4 + 0.5 on both sides, with the module's own grid (`create_meshgrid`).  (`_get_first_stage_fine_matching` itself gathers
    the grid along the MATCH axis: every offset comes out as grid[0] = (-3.5, -3.5), and fewer than 64 matches raise an IndexError; the intended
    gather is along the window axis.)  Second stage: the module's `_get_second_stage_fine_matching` as it is, on a batch of one."""
    from transformers.models.efficientloftr.modeling_efficientloftr import create_meshgrid
    kp = lambda c: torch.stack([c % wc, c // wc], -1).to(w0.dtype) * 8.0
    first, second = fine_confidences(w0, w1)
    index = first.reshape(-1, 64 * 64).max(-1).indices
    i0, i1 = index // 64, index % 64
    grid = (create_meshgrid(8, 8, normalized_coordinates=False, dtype=w0.dtype) - 4 + 0.5).reshape(64, 2)
    pts = torch.stack([kp(ci) + grid[i0], kp(cj) + grid[i1]])[None]
    out = m._get_second_stage_fine_matching(torch.stack([i0, i1])[None, :, :, None], pts, second[None], 64, 1.0)
    return out[0, 0], out[0, 1]


def fine_stage1(w0, w1):
    """(arg-max over the flattened 64 x 64, SAFE: best vs second best >= 1e-3 relative) of the first-stage confidence"""
    top = fine_confidences(w0, w1)[0].reshape(-1, 64 * 64).topk(2, dim=1)
    return top.indices[:, 0], (top.values[:, 0] - top.values[:, 1]) >= SAFE_REL * top.values[:, 0]


# ---------------------------------------------------------------------------------------------------- end to end
def end_to_end(m, images, thr=0.2):
    """the module, stage by stage, on interleaved images (H, W multiples of 32): per pair the matches (i, j) in ascending i with their refined
    points, the confidence matrix and the coarse features.  Match selection is the module's; the fine stage runs per match (see the module docstring)."""
    dt = next(m.parameters()).dtype
    with torch.no_grad():
        s1, s2, s3 = backbone(m, images.to(dt))
        c = transformer(m, s3)
        n, C, h, w = c.shape
        tok = c.permute(0, 2, 3, 1).reshape(n, h * w, C)
        conf = coarse_confidence(tok[0::2], tok[1::2])
        j, score = coarse_matches(m, conf, (h, w))
        f0, f1 = windows(m, c, s2, s1)
        pairs = []
        for p in range(n // 2):
            i = torch.nonzero(j[p] >= 0)[:, 0]
            jj = j[p, i]
            if i.numel():
                p0, p1 = fine_match(m, f0[p, i], f1[p, jj], i, jj, w)
            else:
                p0 = p1 = torch.zeros(0, 2, dtype=dt)
            pairs.append(dict(i=i, j=jj, pts0=p0, pts1=p1, conf=score[p, i]))
    return dict(pairs=pairs, conf=conf, hw=(h, w))


def err(t, ref64):
    d = t.double() - ref64
    return float(d.abs().max() / ref64.abs().max()), float(d.pow(2).mean().sqrt() / ref64.pow(2).mean().sqrt())


def check(stage, got, f32, f64):
    """err(device) <= 10 x err(float32 oracle), max and rms, both against the float64 oracle; printed before it is asserted"""
    assert tuple(got.shape) == tuple(f64.shape), (stage, got.shape, f64.shape)
    eg, eo = err(got, f64), err(f32, f64)
    print(f"[eloftr] {stage}: device max {eg[0]:.3e} rms {eg[1]:.3e} | f32 oracle max {eo[0]:.3e} rms {eo[1]:.3e} | ratio max {eg[0] / eo[0]:.2f} rms {eg[1] / eo[1]:.2f}")
    assert eg[0] == eg[0] and eo[0] > 0
    assert eg[0] <= FACTOR * eo[0] and eg[1] <= FACTOR * eo[1], (stage, eg, eo)
