"""-m gpu: every network, in both HIP.SPLIT arithmetics, built and run out of POISONED allocator memory (tests/pool_poison.py) under three byte
patterns -- 0x00, 0xFF (NaN as float, -1 as int32) and 0x7F (3.39e38 as float, a large positive int32).  Everything a network returns must be
bit-identical under the three and hold no NaN: an output that differs depends on memory no kernel wrote.

Per run the device module is built AFTER the poisoning, so its persistent workspaces come out of poisoned memory too, and the run may not obtain new
memory from the driver (asserted by the harness: a condition, not a measurement).  Inputs and weights are the ones each network's own test file uses.

What is compared: every returned tensor in full where include/mfr_hip.h (or the wrapper that allocates it) states what lies behind a count --
zeros behind n_corr in pts0 / pts1, zero rows behind SuperPoint's n, LightGlue's -1 / 0 fill; where the header leaves a tail open (the coarse matchers'
i_ids / j_ids / mconf behind n_match, SuperGlue's matches0 / mscores0 behind the image's keypoint count) the first n entries only, cut off in the stage.

Two controls show that the instrument can tell: a stage that sums a torch.empty is reported, a stage that writes all it returns is not."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pool_poison as PP  # noqa: E402

from mapfree_reloc_amd import options  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPLITS = ("f16x2", "bf16x3")


def _head(t, n):
    """the first n[p] entries of every row p: what an interface specifies of a tensor whose tail it leaves open"""
    n = n.cpu()
    return torch.cat([t[p, :int(n[p])] for p in range(n.numel())])


# ------------------------------------------------------------------------------------------------ controls
def test_control_a_sum_over_unwritten_memory_is_reported():
    found = PP.pattern_dependence(lambda: dict(total=torch.empty(1 << 20, device=DEV).sum().reshape(1)))
    print("[poison] control, unwritten:", found)
    assert any("differs" in f for f in found) and any("NaN under 0xFF" in f for f in found)


def test_control_a_stage_that_writes_its_output_passes():
    def stage():
        x = torch.empty(1 << 20, device=DEV)
        x.copy_(torch.arange(1 << 20, device=DEV))
        return dict(x=x, total=x.sum().reshape(1), count=torch.full((3,), 7, dtype=torch.int32, device=DEV))
    assert PP.pattern_dependence(stage) == []


# ------------------------------------------------------------------------------------------------ the networks
@pytest.fixture(scope="module")
def wiring():
    """the matcher-wiring builders' weights and inputs (tests/test_gpu_matcher_wiring.py), each built once on first use"""
    import test_gpu_matcher_wiring as MW
    built = {}

    def get(name):
        if name not in built:
            built[name] = getattr(MW, f"build_{name}_oracle")()
        return built[name]
    return get


def _eloftr(split, wiring):
    import eloftr_ref as R
    from mapfree_reloc_amd.nets import eloftr as EL
    sd, im = R.weights("perturbed"), R.end_to_end_images()

    def stage():
        with options.override(SPLIT=split):
            net = EL.EfficientLoFTRHIP(sd, DEV)
            x = im.to(DEV)
            out, capped = net(x), net(x, maxN=20)
        res = {}
        for tag, o in (("", out), ("capped ", capped)):
            n = o["n_coarse"]
            res.update({tag + k: o[k] for k in ("pts0", "pts1", "n_corr", "mconf", "n_coarse")})          # zero-filled behind n_corr (mfr_eloftr_compact)
            res.update({tag + k: _head(o[k], n) for k in ("i_ids", "j_ids")})                             # behind n_match the header leaves them open
        return res
    return stage


def _loftr(split, wiring):
    from mapfree_reloc_amd.nets.loftr import LoFTRHIP
    o = wiring("loftr")

    def stage():
        with options.override(SPLIT=split):
            out = LoFTRHIP(o["sd"], DEV)(o["x"].to(DEV))
        n = out["n_corr"]
        res = {k: out[k] for k in ("pts0", "pts1", "n_corr")}                                             # zeros wherever a slot holds no match
        res.update({k: _head(out[k], n) for k in ("mconf", "i_ids", "j_ids")})                            # open behind n_match in the header
        return res
    return stage


def _superpoint(split, wiring):
    from mapfree_reloc_amd.nets.superpoint import SuperPointHIP
    o = wiring("sp")

    def stage():
        with options.override(SPLIT=split):
            return dict(SuperPointHIP(o["sd"], DEV)(o["x"].to(DEV)))                                      # kpts, scores, desc: rows >= n are zero
    return stage


def _superglue(split, wiring):
    import test_gpu_matcher_wiring as MW
    from mapfree_reloc_amd.nets.superglue import SuperGlueHIP
    o = wiring("sg")

    def stage():
        with options.override(SPLIT=split):
            n = torch.tensor(MW.SG_N, dtype=torch.int32, device=DEV)
            out = SuperGlueHIP(o["sd"], DEV)(dict(kpts=o["kpts"].to(DEV), scores=o["scores"].to(DEV), desc=o["desc"].to(DEV), n=n), o["hw"])
        res = {k: out[k] for k in ("pts0", "pts1", "n_corr")}                                             # zeros from n_corr on (mfr_sg_sinkhorn_match)
        res.update({k: _head(out[k], n[0::2]) for k in ("matches0", "matching_scores0")})                 # rows >= n0: not specified
        return res
    return stage


def _lightglue(split, wiring):
    import lightglue_ref as LG
    from mapfree_reloc_amd.nets import weights as WT
    from mapfree_reloc_amd.nets.lightglue import LightGlueHIP
    sd = LG.perturbed(WT.lightglue_state_dict())
    kpts, desc, _, counts = LG.make_inputs(0)
    B2, N = 2 * LG.B, LG.N

    def stage():
        d = lambda t: t.reshape(B2, N, -1).to(DEV).contiguous()
        with options.override(SPLIT=split):
            net = LightGlueHIP(sd, DEV, filter_threshold=LG.THRESHOLD)
            return dict(net(dict(kpts=d(kpts), desc=d(desc), scores=torch.ones(B2, N, device=DEV), n=counts.reshape(-1).to(DEV).contiguous()), (LG.H, LG.W)))
    return stage


def _depth(module, ref, state_dict, hw):
    def make(split, wiring):
        sd = ref.perturbed(state_dict(arch=ref.REDUCED))
        img = ref.make_images(2, hw[0], hw[1], seed=hw[0])

        def stage():
            with options.override(SPLIT=split):
                metres, _ = module()(sd, DEV, arch=ref.REDUCED)(img.to(DEV), hw)
            return dict(metres=metres)
        return stage
    return make


def _dpt(split, wiring):
    import dpt_ref
    from mapfree_reloc_amd.nets import dpt, weights as WT
    return _depth(lambda: dpt.DPTHIP, dpt_ref, WT.dpt_state_dict, (64, 96))(split, wiring)


def _depth_anything(split, wiring):
    import depth_anything_ref
    from mapfree_reloc_amd.nets import depth_anything as DA, weights as WT
    return _depth(lambda: DA.DepthAnythingHIP, depth_anything_ref, WT.depth_anything_state_dict, depth_anything_ref.SHAPES[0])(split, wiring)


def test_eloftr_backbone_is_reproducible_across_fresh_builds():
    """Regression (found by the bisection of eloftr [bf16x3] below, stage by stage): under bf16x3 the stride-2 3x3 layers of the RepVGG backbone are the
    framework's convolution, and the library's default solver for the first of them (64 -> 128 channels, 4 x 80 x 64) returned different bits in about 8 %
    of its outputs from one freshly built module to the next -- under the SAME pattern, so no unwritten read: four of four repeated runs differed from
    the first, every later layer with them.  Back-to-back calls of one module agree, which is why no parity test saw it; the harness, which rebuilds the
    module between runs, does.  nets/eloftr.py now asks the library for its deterministic solvers.  0x00 twice, then the other patterns; every map."""
    import eloftr_ref as R
    from mapfree_reloc_amd.nets import eloftr as EL
    sd, im = R.weights("perturbed"), R.end_to_end_images()

    def stage():
        with options.override(SPLIT="bf16x3"):
            return dict(zip(("s1", "s2", "s3"), EL.EfficientLoFTRHIP(sd, DEV).features(im.to(DEV))))
    options.reset()
    found = PP.pattern_dependence(stage, (0x00, 0x00, 0xFF, 0x7F))
    print("[poison] eloftr backbone [bf16x3], 0x00 twice:", found or "the same bits in every run")
    assert found == []


NETWORKS = dict(eloftr=_eloftr, loftr=_loftr, superpoint=_superpoint, superglue=_superglue, lightglue=_lightglue, dpt=_dpt, depth_anything=_depth_anything)


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("network", list(NETWORKS))
def test_outputs_do_not_depend_on_what_the_pool_held(network, split, wiring):
    options.reset()
    found = PP.pattern_dependence(NETWORKS[network](split, wiring))
    print(f"[poison] {network} [{split}]: {'independent of the pattern' if not found else found}")
    assert found == [], (network, split, found)
