"""State dicts with the affine terms of a TRAINED network (test helper, CPU only, deterministic).

The seeded recipes of nets/weights.py make almost every affine term trivial (identity BatchNorm in LoFTR, LayerNorm beta = 0, zero
biases in SuperPoint, zero `mlp.3.bias` / `kenc.encoder.12.bias` and bin_score 1.0 in SuperGlue), so a device module that drops, doubles
or swaps one of them still agrees with the oracle on those weights.  `trained_like(sd, seed)` returns a copy of any of the three state
dicts in which none of these terms is trivial any more:

  BatchNorm   gamma ~ U[0.5, 1.5], beta ~ 0.05 N, running_mean ~ 0.1 N, running_var ~ U[0.25, 2]; about a tenth of the channels get
              running_var ~ U[1e-3, 1e-2] with gamma scaled by sqrt(var) (the activations keep their scale, and eps = 1e-5 is ~1e-3 of
              the denominator there: a dropped or misplaced eps shows)
  LayerNorm   gamma *= U[0.7, 1.3], beta = 0.3 mean|gamma| N
  biases      every convolution / linear bias that is all zero becomes BIAS_STD * gain * N, gain = the gain the recipe gives that
              layer's weight (BIAS_GAIN below); SuperPoint's recipe has no gains: its biases are sized against the activations of its
              zero-sum filters on [0, 1] images (SUPERPOINT_BIAS)
  bin_score   SuperGlue's dustbin score 1.0 -> 2.37

The gains are tuned on the CPU oracle alone so that the networks still match (tests/test_gpu_matcher_wiring.py asserts the counts).
Tensors that are not named above are returned unchanged (same bits)."""
import torch

BIAS_STD = 0.1
# gain of the layer's weight in nets/weights.py (key suffix -> gain)
BIAS_GAIN = {
    "fine_preprocess.down_proj.bias": 0.05,      # loftr_state_dict: lin(down_proj, gain=0.05)
    "fine_preprocess.merge_feat.bias": 1.0,
    "mlp.3.bias": 0.1,                           # superglue_state_dict: gnn_gain
    "kenc.encoder.12.bias": 0.1,                 # superglue_state_dict: kenc_gain
}
# SuperPoint: the zero-sum filters answer to image contrast only (activations ~1e-2 .. 1e-1 on [0, 1] images), so a bias of 0.1 would
# bury the image; the detector head's weight carries a gain of 80 and its logits are O(1)
SUPERPOINT_BIAS = {"convPb.bias": 0.3}
SUPERPOINT_BIAS_DEFAULT = 0.005
BIN_SCORE = 2.37


def _is_superpoint(sd):
    return "conv1a.weight" in sd


def trained_like(sd, seed=0):
    """copy of a nets/weights.py state dict (SuperPoint, SuperGlue or LoFTR) with non-trivial BatchNorm, LayerNorm, biases and bin_score"""
    g = torch.Generator().manual_seed(int(seed))
    randn = lambda n: torch.randn(n, generator=g)
    rand = lambda n, lo, hi: lo + (hi - lo) * torch.rand(n, generator=g)
    out = {k: v.clone() for k, v in sd.items()}
    affine = set()                                # keys of BatchNorm / LayerNorm parameters: not "biases that are zero today"
    for k in sorted(sd):
        if k.endswith(".running_var"):
            p = k[:-len(".running_var")]
            c = sd[k].numel()
            gamma, var = rand(c, 0.5, 1.5), rand(c, 0.25, 2.0)
            small = torch.rand(c, generator=g) < 0.1
            small[int(torch.randint(0, c, (1,), generator=g))] = True           # at least one channel, whatever the width
            var_small = rand(c, 1e-3, 1e-2)
            var = torch.where(small, var_small, var)
            gamma = torch.where(small, gamma * var_small.sqrt(), gamma)
            out[p + ".weight"], out[p + ".bias"] = gamma, 0.05 * randn(c)
            out[p + ".running_mean"], out[p + ".running_var"] = 0.1 * randn(c), var
            affine.update((p + ".weight", p + ".bias"))
    for k in sorted(sd):
        if k.endswith((".norm1.weight", ".norm2.weight")):
            p = k[:-len(".weight")]
            c = sd[k].numel()
            gamma = sd[k] * rand(c, 0.7, 1.3)
            out[p + ".weight"], out[p + ".bias"] = gamma, 0.3 * gamma.abs().mean() * randn(c)
            affine.update((p + ".weight", p + ".bias"))
    sp = _is_superpoint(sd)
    for k in sorted(sd):
        if not k.endswith(".bias") or k in affine or bool(sd[k].any()):
            continue
        if sp:
            std = SUPERPOINT_BIAS.get(k, SUPERPOINT_BIAS_DEFAULT)
        else:
            gains = [v for s, v in BIAS_GAIN.items() if k.endswith(s)]
            std = BIAS_STD * (gains[0] if gains else 1.0)
        out[k] = std * randn(sd[k].numel())
    if "bin_score" in sd:
        out["bin_score"] = torch.tensor(BIN_SCORE)
    return out
