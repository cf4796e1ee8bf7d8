"""Host-side weight folding on weights with the affine terms of a trained network (tests/trained_like.py): no GPU.

nets/loftr._fold turns conv -> BatchNorm(eval) into one convolution with a bias; with the identity BatchNorm of nets/weights.py it is
the identity and nothing checks it.  (SuperGlue's folding algebra: tests/test_host_logic.py::test_superglue_weight_folding_is_exact_algebra.)"""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from trained_like import BIN_SCORE, trained_like  # noqa: E402

from mapfree_reloc_amd.nets import weights as WT  # noqa: E402
from mapfree_reloc_amd.nets.loftr import _fold  # noqa: E402


def _loftr_folded_pairs():
    """(convolution, BatchNorm, stride) of every pair LoFTRHIP.__init__ folds: the stem, two per BasicBlock, the stride-2 blocks' downsample,
    and the first convolution of the two FPN output heads -- 17 BatchNorms"""
    pairs = [("backbone.conv1", "backbone.bn1", 2)]
    for L, stride in (("layer1", 1), ("layer2", 2), ("layer3", 2)):
        for b in (0, 1):
            p = f"backbone.{L}.{b}"
            s = stride if b == 0 else 1
            pairs += [(f"{p}.conv1", f"{p}.bn1", s), (f"{p}.conv2", f"{p}.bn2", 1)]
            if s != 1:
                pairs.append((f"{p}.downsample.0", f"{p}.downsample.1", s))
    pairs += [("backbone.layer2_outconv2.0", "backbone.layer2_outconv2.1", 1), ("backbone.layer1_outconv2.0", "backbone.layer1_outconv2.1", 1)]
    return pairs


@pytest.fixture(scope="module")
def loftr_sd():
    return {k: v.double() for k, v in trained_like(WT.loftr_state_dict(), 11).items()}


def test_loftr_folded_pairs_are_all_batchnorms(loftr_sd):
    pairs = _loftr_folded_pairs()
    bns = {k[:-len(".running_var")] for k in loftr_sd if k.endswith(".running_var")}
    assert {bn for _, bn, _ in pairs} == bns and len(bns) == 17
    kinds = {(tuple(loftr_sd[c + ".weight"].shape[2:]), s) for c, _, s in pairs}
    assert kinds == {((7, 7), 2), ((3, 3), 1), ((3, 3), 2), ((1, 1), 2)}


@pytest.mark.parametrize("conv,bn,stride", _loftr_folded_pairs())
def test_loftr_fold_equals_batchnorm_of_conv(loftr_sd, conv, bn, stride):
    """conv2d(x, cw, cb) == batch_norm(conv2d(x, w)) in float64 to 1e-12 (eval statistics, eps 1e-5: a tenth of the channels have
    var ~ 1e-3 .. 1e-2, where eps is ~1e-3 of the denominator)"""
    sd = loftr_sd
    w = sd[conv + ".weight"]
    g = torch.Generator().manual_seed(w.shape[0] + 7 * stride)
    x = torch.randn(2, w.shape[1], 11, 9, generator=g, dtype=torch.float64)
    pad = w.shape[-1] // 2
    want = F.batch_norm(F.conv2d(x, w, None, stride=stride, padding=pad), sd[bn + ".running_mean"], sd[bn + ".running_var"],
                        sd[bn + ".weight"], sd[bn + ".bias"], training=False, eps=1e-5)
    cw, cb = _fold(w, sd, bn)
    got = F.conv2d(x, cw, cb, stride=stride, padding=pad)
    assert float(want.abs().max()) > 0.1
    assert float((got - want).abs().max()) <= 1e-12
    # and the terms the fold carries do matter on these weights: without the running mean, or without eps, the result is visibly another
    s = sd[bn + ".weight"] / torch.sqrt(sd[bn + ".running_var"] + 1e-5)
    no_mean = F.conv2d(x, cw, sd[bn + ".bias"], stride=stride, padding=pad)
    s0 = sd[bn + ".weight"] / torch.sqrt(sd[bn + ".running_var"])
    no_eps = F.conv2d(x, w * s0[:, None, None, None], sd[bn + ".bias"] - sd[bn + ".running_mean"] * s0, stride=stride, padding=pad)
    assert float((no_mean - want).abs().max()) > 1e-3 * float(want.abs().max())
    assert float((no_eps - want).abs().max()) > 1e-5 * float(want.abs().max())
    assert torch.equal(cb, sd[bn + ".bias"] - sd[bn + ".running_mean"] * s)


@pytest.mark.parametrize("maker", [WT.superpoint_state_dict, WT.superglue_state_dict, WT.loftr_state_dict])
def test_trained_like_leaves_no_trivial_term(maker):
    """deterministic, the recipe's own tensors untouched, same keys and shapes; every BatchNorm / LayerNorm is non-trivial, no bias is zero"""
    sd = maker()
    keep = {k: v.clone() for k, v in sd.items()}
    a, b = trained_like(sd, 5), trained_like(sd, 5)
    assert all(torch.equal(sd[k], keep[k]) for k in sd)
    assert set(a) == set(sd) and all(a[k].shape == sd[k].shape and a[k].dtype == sd[k].dtype for k in sd)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert any(not torch.equal(a[k], trained_like(sd, 6)[k]) for k in a)
    for k, v in a.items():
        if k.endswith(".bias"):
            assert float(v.abs().min()) > 0, k
        if k.endswith(".running_var"):
            p = k[:-len(".running_var")]
            assert 1e-3 <= float(v.min()) <= 1e-2 and 0.25 <= float(v.max()) <= 2.0, k
            assert float(a[p + ".running_mean"].abs().max()) > 0.05 and float(a[p + ".bias"].abs().max()) > 0.02
            assert float(a[p + ".weight"].max()) > 1.1
        if k.endswith((".norm1.weight", ".norm2.weight")):
            assert float(v.std()) > 0.1 * float(v.abs().mean()), k
        if k.endswith(".weight") and k[:-len(".weight")] + ".running_var" not in a and ".norm" not in k:
            assert torch.equal(v, sd[k]), k                     # convolution / linear weights: the recipe's bits
    if "bin_score" in a:
        assert float(a["bin_score"]) == pytest.approx(BIN_SCORE) and float(sd["bin_score"]) == 1.0
