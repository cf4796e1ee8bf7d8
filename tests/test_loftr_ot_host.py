"""CPU: the host side of LoFTR's optimal-transport coarse matching (LOFTR.MATCH_TYPE 'sinkhorn'): config keys, the C-ABI
bookkeeping of mfr_loftr_ot_match, the bin_score key of the weights, the constructor surface of the routes, and the test helper's
reference statement against HuggingFace's log_optimal_transport."""
import ctypes
import inspect
import os
import re
import sys

import pytest
import torch

import mapfree_reloc_amd as mfr
from mapfree_reloc_amd.config import get_cfg_defaults
from mapfree_reloc_amd.nets import weights as WT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loftr_ot_ref as OT  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_config_declares_match_type_and_iterations(tmp_path):
    cfg = get_cfg_defaults()
    assert cfg.LOFTR.MATCH_TYPE == "dual_softmax" and cfg.LOFTR.SKH_ITERS == 3
    y = tmp_path / "ot.yaml"
    y.write_text("LOFTR:\n  MATCH_TYPE: sinkhorn\n")
    cfg.merge_from_file(str(y))
    assert cfg.LOFTR.MATCH_TYPE == "sinkhorn" and cfg.LOFTR.SKH_ITERS == 3
    assert "SKH_PREFILTER" not in cfg.LOFTR


def test_cabi_declares_and_exports_the_ot_entry_points():
    hdr = open(os.path.join(ROOT, "include", "mfr_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(mfr_[a-z0-9_]+)\s*\(", hdr))
    assert {"mfr_loftr_ot_match", "mfr_loftr_ot_match_workspace_bytes"} <= declared
    lib = mfr._lib.load()                                  # loads without a GPU
    assert hasattr(lib, "mfr_loftr_ot_match") and hasattr(lib, "mfr_loftr_ot_match_workspace_bytes")
    assert lib.mfr_abi_version() == 6                      # additive
    w16, w32 = lib.mfr_loftr_ot_match_workspace_bytes(16, 6120, 6120), lib.mfr_loftr_ot_match_workspace_bytes(32, 6120, 6120)
    assert w16 > 0 and w32 > w16 and lib.mfr_loftr_ot_match_workspace_bytes(1, 6120, 6120) < w16
    assert lib.mfr_loftr_ot_match_workspace_bytes(0, 6120, 6120) == 0
    # the sweeps' partials stay a small fraction of the 16 x 150 MB matrix
    assert w16 < 0.1 * 16 * 6120 * 6120 * 4


def test_ot_match_rejects_bad_arguments_before_any_launch():
    lib = mfr._lib.load()
    E_ARG, E_WS = -1, -3
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    call = lambda S=p, B=1, h0=2, w0=2, h1=2, w1=2, iters=3, ws=p, wsb=0, ids=p, variant=0: lib.mfr_loftr_ot_match(
        S, B, h0, w0, h1, w1, 1.0, iters, 0.2, 2, ws, wsb, ids, p, p, p, None, None, variant, None)
    assert call(S=None) == E_ARG and call(B=0) == E_ARG and call(h1=0) == E_ARG and call(iters=0) == E_ARG
    assert call(variant=2) == E_ARG and call(ids=None) == E_ARG and call(ws=None) == E_ARG
    assert call(wsb=16) == E_WS                            # a short workspace is its own code


def test_state_dict_bin_score_key_and_checkpoint_round_trip(tmp_path):
    sd = WT.loftr_state_dict()
    assert not any("bin_score" in k for k in sd)
    sd = WT.loftr_state_dict(bin_score=2.5)
    assert float(sd["coarse_matching.bin_score"]) == 2.5
    # a Lightning-style *_ot.ckpt: {"state_dict": {"matcher." + key: tensor}}
    path = tmp_path / "indoor_ot.ckpt"
    torch.save({"state_dict": {"matcher." + k: v for k, v in sd.items()}}, path)
    back = WT.strip_prefix(WT.load_checkpoint(str(path)), "matcher.")
    assert set(back) == set(sd) and float(back["coarse_matching.bin_score"]) == 2.5
    assert torch.equal(back["backbone.conv1.weight"], sd["backbone.conv1.weight"])


def test_routes_accept_match_type_with_the_dual_softmax_default():
    from mapfree_reloc_amd import compute
    from mapfree_reloc_amd.matchers import LoFTR_matcher
    from mapfree_reloc_amd.nets.loftr import LoFTRHIP
    from mapfree_reloc_amd.pipeline import LoFTREmatPipeline
    for cls in (LoFTR_matcher, LoFTREmatPipeline, LoFTRHIP):
        par = inspect.signature(cls.__init__).parameters
        assert "match_type" in par and par["match_type"].default == "dual_softmax", cls
    for cls in (LoFTREmatPipeline, LoFTRHIP):
        assert inspect.signature(cls.__init__).parameters["skh_iters"].default == 3
    with pytest.raises(ValueError):                        # checked before anything touches the GPU
        LoFTRHIP({}, match_type="softmax")
    # the offline stage's two LoFTR outputs cannot be confused
    assert compute.output_tag("LoFTR") == "LoFTR" and compute.output_tag("LoFTR", "sinkhorn") == "LoFTR_OT"
    assert compute.output_tag("SG", "sinkhorn") == "SG"


def test_reference_statement_equals_huggingface_log_optimal_transport():
    """test infrastructure checking itself: the helper's confidences are HuggingFace SuperGlue's log_optimal_transport on the
    same scores, dustbins cut off"""
    hf = pytest.importorskip("transformers.models.superglue.modeling_superglue")
    g = torch.Generator().manual_seed(5)
    S = torch.randn(2, 37, 29, generator=g) * 3.0
    for b, iters in ((1.0, 3), (2.5, 3), (1.0, 20)):
        want = hf.log_optimal_transport(S, torch.tensor(b), iters).exp()[:, :-1, :-1]
        assert torch.equal(OT.ot_conf(S, b, iters), want)
        z = OT.ot_log_assignment(S, b, iters)
        assert z.shape == (2, 38, 30)
        # the last half-iteration normalises the columns: every inner column plus its dustbin-row entry sums to one
        assert (z.exp()[:, :, :-1].sum(1) - 1).abs().max() < 1e-4
