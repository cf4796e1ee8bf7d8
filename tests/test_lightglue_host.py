"""LightGlue without a GPU: the surfaces exist (registries, config node, C-ABI entry points and their argument checks), the seeded weights make
the ORACLE match, the inputs of the GPU tests are well conditioned (checked on the oracle alone), and the checkpoint-name converter round-trips.

The oracle is the `transformers` LightGlue module (tests/lightglue_ref.py); the product never imports it."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lightglue_ref as LG  # noqa: E402

import mapfree_reloc_amd as mfr  # noqa: E402
from mapfree_reloc_amd.config import get_cfg_defaults  # noqa: E402
from mapfree_reloc_amd.nets import weights as WT  # noqa: E402

MFR_E_ARG = -1


# ------------------------------------------------------------------------------------------------ registry and config
def test_registries_and_config_node():
    from mapfree_reloc_amd import matchers
    from mapfree_reloc_amd.matching import feature_matching as fm, model
    assert model.FEATURE_MATCHERS["LightGlue"] is fm.LightGlueMatching
    assert matchers.MATCHERS["LG"] is matchers.LightGlue_matcher
    lg = get_cfg_defaults().LIGHTGLUE
    want = dict(WEIGHTS="", FILTER_THRESHOLD=0.1, NUM_LAYERS=9, MAX_KEYPOINTS=1024, KEYPOINT_THRESHOLD=0.005, NMS_RADIUS=4,
                DEPTH_CONFIDENCE=-1, WIDTH_CONFIDENCE=-1)
    assert {k: lg[k] for k in want} == want
    sg = get_cfg_defaults().SUPERGLUE                                   # the SuperPoint settings are the SuperGlue stage's: shapes and cache are shared
    assert all(lg[k] == sg[k] for k in ("MAX_KEYPOINTS", "KEYPOINT_THRESHOLD", "NMS_RADIUS"))


@pytest.mark.parametrize("key", ["DEPTH_CONFIDENCE", "WIDTH_CONFIDENCE"])
def test_adaptive_depth_and_width_are_refused(key):
    from mapfree_reloc_amd.nets import lightglue
    cfg = get_cfg_defaults()
    assert lightglue.check_cfg(cfg) is cfg.LIGHTGLUE
    cfg.LIGHTGLUE[key] = 0.95
    with pytest.raises(ValueError, match="out of scope"):
        lightglue.check_cfg(cfg)


# ------------------------------------------------------------------------------------------------ entry points
def test_entry_points_exported_and_reject_bad_arguments():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mfr_hip.h")).read()
    names = ["mfr_lg_rotary_table", "mfr_lg_rotary_apply", "mfr_lg_ln_gelu", "mfr_lg_assign_workspace_bytes", "mfr_lg_assign", "mfr_gemm_f16x2_ln_gelu",
             "mfr_gemm_bf16x3_ln_gelu"]
    lib = mfr._lib.load()                                                # loads without a GPU
    for n in names:
        assert n + "(" in hdr and n in mfr._lib.SIGNATURES and hasattr(lib, n), n
    buf = ctypes.create_string_buffer(4096)                              # a non-null pointer; no launch happens behind a refused argument
    p = ctypes.addressof(buf) // 16 * 16 + 16
    assert lib.mfr_lg_rotary_table(None, p, 4, p, None) == MFR_E_ARG
    assert lib.mfr_lg_rotary_table(p, p, 0, p, None) == MFR_E_ARG and lib.mfr_lg_rotary_table(p, p, -3, p, None) == MFR_E_ARG
    assert lib.mfr_lg_rotary_apply(None, p, 768, 4, p, None) == MFR_E_ARG
    assert lib.mfr_lg_rotary_apply(p, p, 255, 4, p, None) == MFR_E_ARG and lib.mfr_lg_rotary_apply(p, p, 768, -1, p, None) == MFR_E_ARG
    assert lib.mfr_lg_rotary_apply(p + 4, p, 768, 4, p, None) == MFR_E_ARG                       # pairs must be 8-byte aligned
    assert lib.mfr_lg_ln_gelu(None, 512, 4, p, p, 1e-5, None) == MFR_E_ARG
    assert lib.mfr_lg_ln_gelu(p, 511, 4, p, p, 1e-5, None) == MFR_E_ARG and lib.mfr_lg_ln_gelu(p, 512, 0, p, p, 1e-5, None) == MFR_E_ARG
    assert lib.mfr_lg_ln_gelu(p, 512, 4, p, p, -1.0, None) == MFR_E_ARG
    for fn in (lib.mfr_gemm_f16x2_ln_gelu, lib.mfr_gemm_bf16x3_ln_gelu):
        assert fn(None, 512, p, p, p, p, 1e-5, p, 512, 4, 512, 512, None) == MFR_E_ARG and fn(p, 512, None, p, p, p, 1e-5, p, 512, 4, 512, 512, None) == MFR_E_ARG
        assert fn(p, 512, p, p, None, p, 1e-5, p, 512, 4, 512, 512, None) == MFR_E_ARG and fn(p, 512, p, p, p, p, 1e-5, None, 512, 4, 512, 512, None) == MFR_E_ARG
        assert fn(p, 512, p, p, p, p, 1e-5, p, 512, -4, 512, 512, None) == MFR_E_ARG and fn(p, 512, p, p, p, p, 1e-5, p, 512, 4, 256, 512, None) == MFR_E_ARG
        assert fn(p, 512, p, p, p, p, 1e-5, p, 512, 4, 512, 500, None) == MFR_E_ARG and fn(p, 256, p, p, p, p, 1e-5, p, 512, 4, 512, 512, None) == MFR_E_ARG
        assert fn(p, 512, p, p, p, p, 1e-5, p, 511, 4, 512, 512, None) == MFR_E_ARG and fn(p, 512, p, p, p, p, -1.0, p, 512, 4, 512, 512, None) == MFR_E_ARG
    assert lib.mfr_lg_assign_workspace_bytes(0, 8, 8) == 0 and lib.mfr_lg_assign_workspace_bytes(2, -1, 8) == 0
    small, big = lib.mfr_lg_assign_workspace_bytes(2, 80, 80), lib.mfr_lg_assign_workspace_bytes(32, 1024, 1024)
    assert 0 < small < big
    ok = dict(S=p, B=2, N0=8, N1=8, ldS=8, z0=p, z1=p, n0=p, n1=p, thr=0.1, k0=None, k1=None, K=0, ws=p, wsb=1 << 30, m0=p, m1=p, s0=p, s1=p,
              p0=None, p1=None, maxN=0, nc=None)
    for bad in (dict(S=None), dict(z1=None), dict(n0=None), dict(ws=None), dict(m1=None), dict(s0=None), dict(B=0), dict(B=-2), dict(N0=-8), dict(N1=0),
                dict(ldS=7), dict(thr=-0.5), dict(k0=p), dict(k0=p, k1=p, p0=p, p1=p, nc=p, maxN=0, K=8), dict(k0=p, k1=p, p0=p, p1=p, nc=p, maxN=8, K=7)):
        a = dict(ok, **bad)
        assert lib.mfr_lg_assign(a["S"], a["B"], a["N0"], a["N1"], a["ldS"], a["z0"], a["z1"], a["n0"], a["n1"], a["thr"], a["k0"], a["k1"], a["K"], a["ws"],
                                 a["wsb"], a["m0"], a["m1"], a["s0"], a["s1"], a["p0"], a["p1"], a["maxN"], a["nc"], None) == MFR_E_ARG, bad
    a = dict(ok, wsb=16)                                                                          # too small a workspace: its own code, still nothing launched
    assert lib.mfr_lg_assign(a["S"], a["B"], a["N0"], a["N1"], a["ldS"], a["z0"], a["z1"], a["n0"], a["n1"], a["thr"], a["k0"], a["k1"], a["K"], a["ws"],
                             a["wsb"], a["m0"], a["m1"], a["s0"], a["s1"], a["p0"], a["p1"], a["maxN"], a["nc"], None) == -3


# ------------------------------------------------------------------------------------------------ seeded weights, on the oracle
@pytest.fixture(scope="module")
def inputs():
    return LG.make_inputs(0)


def _twins_matched(matches, counts):
    out = []
    for p in range(LG.B):
        m0, m1 = matches[2 * p], matches[2 * p + 1]
        ar = torch.arange(LG.TWINS)
        out.append((int((m0[:counts[p, 0]] >= 0).sum()), bool((m0[:LG.TWINS] == ar).all() and (m1[:LG.TWINS] == ar).all())))
    return out


@pytest.mark.parametrize("perturb", [False, True])
def test_seeded_weights_match_the_planted_twins(inputs, perturb):
    """plain initialisation leaves the assignment flat (no matches); the recipe of nets/weights.lightglue_state_dict recovers every planted twin, also
    with the biases and LayerNorm terms of tests/lightglue_ref.perturbed"""
    kpts, desc, mask, counts = inputs
    sd = WT.lightglue_state_dict()
    assert sd["match_assignment_layers.8.final_projection.weight"].shape == (256, 256) and "token_confidence.7.token.weight" in sd
    m32, _ = LG.make_models(LG.perturbed(sd) if perturb else sd)
    mt, sc, hs = LG.run(m32, kpts, desc, mask)
    assert len(hs) == 63
    for n_match, twins in _twins_matched(mt, counts):
        assert n_match >= LG.TWINS and twins, (n_match, twins)
    plain = dict(sd)                                                     # ... and without the recipe's last assignment layer nothing matches
    g = torch.Generator().manual_seed(1)
    plain["match_assignment_layers.8.final_projection.weight"] = 0.02 * torch.randn(256, 256, generator=g)
    plain["match_assignment_layers.8.matchability.bias"] = torch.zeros(1)
    mt0, _, _ = LG.run(LG.make_models(plain)[0], kpts, desc, mask)
    assert int((mt0 >= 0).sum()) == 0


def test_oracle_is_stable_on_the_test_inputs(inputs):
    """the condition on the inputs of tests/test_gpu_lightglue.py, on the oracle alone: float32 and float64 give identical matches, every accepted
    score is at least 0.05 from the threshold, and no keypoint is unsafe under the rule the GPU tests apply"""
    kpts, desc, mask, counts = inputs
    m32, m64 = LG.make_models(LG.perturbed(WT.lightglue_state_dict()))
    mt32, sc32, _ = LG.run(m32, kpts, desc, mask)
    mt64, sc64, hs64 = LG.run(m64, kpts, desc, mask)
    assert torch.equal(mt32, mt64)
    acc = sc64[mt64 >= 0]
    assert acc.numel() >= 2 * 2 * LG.TWINS and float((acc - LG.THRESHOLD).abs().min()) >= 0.05
    assert float((sc32.double() - sc64).abs().max()) < 1e-3
    S, z0, z1 = LG.similarity(m64, hs64[60])
    n0, n1 = counts[:, 0], counts[:, 1]
    a0, a1, s0, s1, logp = LG.assign64(S, z0, z1, n0, n1)
    for p in range(LG.B):                                                # the stage-wise helper is the module's own result
        assert torch.equal(a0[p, :n0[p]], mt64[2 * p, :n0[p]]) and torch.equal(a1[p, :n1[p]], mt64[2 * p + 1, :n1[p]])
        assert torch.allclose(s0[p, :n0[p]], sc64[2 * p, :n0[p]], rtol=0, atol=1e-12)
    safe0, safe1 = LG.safe_masks(logp, n0, n1)
    assert int(safe0.sum()) == int(n0.sum()) and int(safe1.sum()) == int(n1.sum())


# ------------------------------------------------------------------------------------------------ checkpoint names
def _to_upstream(sd, n_layers=9):
    """the inverse renaming of nets/lightglue.from_upstream, written independently (cvg/LightGlue's module tree)"""
    out = {"posenc.Wr.weight": sd["positional_encoder.projector.weight"]}
    for l in range(n_layers):
        t, u = f"transformer_layers.{l}", f"transformers.{l}"
        w = torch.stack([sd[f"{t}.self_attention.{n}_proj.weight"] for n in "qkv"], 1)            # [256 (head, dim), 3, 256]
        b = torch.stack([sd[f"{t}.self_attention.{n}_proj.bias"] for n in "qkv"], 1)
        out[f"{u}.self_attn.Wqkv.weight"], out[f"{u}.self_attn.Wqkv.bias"] = w.reshape(768, 256), b.reshape(768)
        for wb in ("weight", "bias"):
            out[f"{u}.self_attn.out_proj.{wb}"] = sd[f"{t}.self_attention.o_proj.{wb}"]
            out[f"{u}.cross_attn.to_qk.{wb}"] = sd[f"{t}.cross_attention.q_proj.{wb}"]
            out[f"{u}.cross_attn.to_v.{wb}"] = sd[f"{t}.cross_attention.v_proj.{wb}"]
            out[f"{u}.cross_attn.to_out.{wb}"] = sd[f"{t}.cross_attention.o_proj.{wb}"]
            for kind, src in (("self", "self_attn"), ("cross", "cross_attn")):
                for name, i in (("fc1", 0), ("layer_norm", 1), ("fc2", 3)):
                    out[f"{u}.{src}.ffn.{i}.{wb}"] = sd[f"{t}.{kind}_mlp.{name}.{wb}"]
            out[f"log_assignment.{l}.final_proj.{wb}"] = sd[f"match_assignment_layers.{l}.final_projection.{wb}"]
            out[f"log_assignment.{l}.matchability.{wb}"] = sd[f"match_assignment_layers.{l}.matchability.{wb}"]
            if l < n_layers - 1:
                out[f"token_confidence.{l}.token.0.{wb}"] = sd[f"token_confidence.{l}.token.{wb}"]
    return out


def test_upstream_checkpoint_names_round_trip():
    """UNPINNED against a published file (none exists offline): only the renaming and the Wqkv de-interleave are checked.  Upstream shares one
    projection between the cross block's queries and keys, so the round trip starts from weights with k_proj = q_proj there"""
    from mapfree_reloc_amd.nets.lightglue import from_upstream
    sd = LG.perturbed(WT.lightglue_state_dict(3), 5)
    for l in range(9):
        for wb in ("weight", "bias"):
            sd[f"transformer_layers.{l}.cross_attention.k_proj.{wb}"] = sd[f"transformer_layers.{l}.cross_attention.q_proj.{wb}"]
    up = _to_upstream(sd)
    assert up["transformers.0.self_attn.Wqkv.weight"].shape == (768, 256)
    w = up["transformers.2.self_attn.Wqkv.weight"]                       # output channel (head h, dim d, j): row 3 (64 h + d) + j
    assert torch.equal(w[3 * (64 * 2 + 5) + 1], sd["transformer_layers.2.self_attention.k_proj.weight"][64 * 2 + 5])
    back = from_upstream(up)
    assert set(back) == set(sd)
    for k in sd:
        assert torch.equal(back[k], sd[k]), k


# ------------------------------------------------------------------------------------------------ weight folding
def test_folded_weights_are_the_module_in_float64(inputs):
    """nets/lightglue.fold_weights (concatenated q/k/v, o_proj folded into fc1, final_projection / 4 stacked on matchability) evaluated with plain
    float64 tensor algebra == the module in float64: descriptors after all layers, similarity and matchability logits.  Bar 1e-6 of the tensor's
    scale: the module rounds q and k to float32 inside its rotary encoding whatever its dtype (measured here: 3e-8), a wiring error is >= 1e-3"""
    from mapfree_reloc_amd.nets.lightglue import fold_weights
    kpts, desc, mask, counts = inputs
    sd = LG.perturbed(WT.lightglue_state_dict())
    _, m64 = LG.make_models(sd)
    _, _, hs64 = LG.run(m64, kpts, desc, mask)
    fw = fold_weights(sd)
    d = lambda t: t.double()
    B2, N = 2 * LG.B, LG.N
    x = d(desc).reshape(B2, N, 256)
    kn = (d(kpts).reshape(B2, N, 2) - torch.tensor([LG.W / 2, LG.H / 2], dtype=torch.float64)) / (max(LG.W, LG.H) / 2)
    th = kn @ d(fw["wr"]).t()
    c, s = th.cos()[:, :, None], th.sin()[:, :, None]                    # [B2, N, 1, 32]: the same angles for every head
    keymask = mask.reshape(B2, N).bool()
    flip = lambda t: t.reshape(LG.B, 2, *t.shape[1:]).flip(1).reshape(t.shape)

    def rot(t):                                                          # t [B2, N, 4, 64], pairs (2i, 2i + 1)
        e, o = t[..., 0::2], t[..., 1::2]
        return torch.stack([e * c - o * s, o * c + e * s], -1).flatten(-2)
    for L in fw["blocks"]:
        q, k, v = (x @ d(L["wqkv"]).t() + d(L["bqkv"])).reshape(B2, N, 3, 4, 64).unbind(2)
        if L["cross"]:
            k, v, km = flip(k), flip(v), flip(keymask)
        else:
            q, k, km = rot(q), rot(k), keymask
        logits = torch.einsum("bnhd,bmhd->bhnm", q, k) / 8.0
        a = torch.einsum("bhnm,bmhd->bnhd", logits.masked_fill(~km[:, None, None, :], -float("inf")).softmax(-1), v).reshape(B2, N, 256)
        h = torch.cat([x, a], -1) @ d(L["w1"]).t() + d(L["b1"])
        h = torch.nn.functional.gelu(torch.nn.functional.layer_norm(h, (512,), d(L["ln_g"]), d(L["ln_b"]), 1e-5))
        x = x + h @ d(L["w2"]).t() + d(L["b2"])
    assert float((x - hs64[60]).abs().max()) < 1e-6 * float(hs64[60].abs().max())
    mdz = x @ d(fw["wfz"]).t() + d(fw["bfz"])
    md = mdz[..., :256].reshape(LG.B, 2, N, 256)
    S, z0, z1 = LG.similarity(m64, hs64[60])
    assert float((md[:, 0] @ md[:, 1].transpose(1, 2) - S).abs().max()) < 1e-6 * float(S.abs().max())
    z = mdz[..., 256].reshape(LG.B, 2, N)
    assert float((z[:, 0] - z0).abs().max()) < 1e-6 and float((z[:, 1] - z1).abs().max()) < 1e-6
