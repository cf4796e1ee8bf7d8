"""Depth Anything without a GPU: the host-side folds of nets/depth_anything.py against the `transformers` module (tests/depth_anything_ref.py), the config's
checks, the architecture's refusals, the spread of the reference maps the GPU tests compare against, and the C-ABI's argument checks."""
import ctypes
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_anything_ref as R  # noqa: E402

import mapfree_reloc_amd as mfr  # noqa: E402
from mapfree_reloc_amd.config import get_cfg_defaults  # noqa: E402
from mapfree_reloc_amd.nets import depth_anything as DA, dpt, weights as WT  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MFR_E_ARG = -1


@pytest.fixture(scope="module")
def sd():
    return R.perturbed(WT.depth_anything_state_dict(arch=R.REDUCED))


@pytest.fixture(scope="module")
def models(sd):
    return R.make_models(sd, DA.check_arch(R.REDUCED))          # strict: the generator's keys are the module's, no more and no fewer


# ------------------------------------------------------------------------------------------------ folds
def test_layerscale_fold_equals_the_unfolded_layer(sd, models):
    """one oracle layer in float64 against the same layer written out with the folded weights: lambda1 into attention.output.dense, lambda2 into mlp.fc2"""
    m64 = models[1]
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 36, 192, generator=g, dtype=torch.float64)
    p = "backbone.encoder.layer.2"
    assert float((sd[f"{p}.layer_scale1.lambda1"] - 1).abs().min()) > 0          # a perturbed LayerScale: a dropped fold would show
    with torch.no_grad():
        want = m64.backbone.encoder.layer[2](x)
    want = want[0] if isinstance(want, tuple) else want
    d = {k[len(p) + 1:]: v.double() for k, v in sd.items() if k.startswith(p + ".")}
    wo, bo = DA.fold_layerscale(d["attention.output.dense.weight"], d["attention.output.dense.bias"], d["layer_scale1.lambda1"])
    w2, b2 = DA.fold_layerscale(d["mlp.fc2.weight"], d["mlp.fc2.bias"], d["layer_scale2.lambda1"])
    wqkv, bqkv = dpt.fold_qkv(sd, p)
    y = F.layer_norm(x, (192,), d["norm1.weight"], d["norm1.bias"], 1e-6)
    q, k, v = (t.view(2, 36, 3, 64).transpose(1, 2) for t in F.linear(y, wqkv, bqkv).split(192, dim=-1))
    att = (torch.softmax(q @ k.transpose(-1, -2) / 8.0, -1) @ v).transpose(1, 2).reshape(2, 36, 192)
    t = x + F.linear(att, wo, bo)
    got = t + F.linear(F.gelu(F.linear(F.layer_norm(t, (192,), d["norm2.weight"], d["norm2.bias"], 1e-6), d["mlp.fc1.weight"], d["mlp.fc1.bias"])), w2, b2)
    assert float((got - want).abs().max()) < 1e-12 * float(want.abs().max())


@pytest.mark.parametrize("grid", [(5, 7), (7, 3), (4, 6), (5, 5)])
def test_position_resize_is_dinov2s(sd, models, grid):
    m32 = models[0]
    gh, gw = grid
    emb = torch.zeros(1, 1 + gh * gw, 192)
    with torch.no_grad():
        want = m32.backbone.embeddings.interpolate_pos_encoding(emb, 14 * gh, 14 * gw)[0]
    got = DA.resize_position_embeddings(sd["backbone.embeddings.position_embeddings"], gh, gw)
    assert got.shape == want.shape == (1 + gh * gw, 192) and got.dtype == torch.float32 and torch.equal(got, want)


@pytest.mark.parametrize("i,s", [(0, 4), (1, 2)])
def test_conv_transpose_fold_on_depth_anythings_shapes(sd, i, s):
    w, b = sd[f"neck.reassemble_stage.layers.{i}.resize.weight"].double(), sd[f"neck.reassemble_stage.layers.{i}.resize.bias"].double()
    c = R.REDUCED["NECK_SIZES"][i]
    assert w.shape == (c, c, s, s)
    g = torch.Generator().manual_seed(i)
    x = torch.randn(2, c, 5, 7, generator=g, dtype=torch.float64)
    want = F.conv_transpose2d(x, w, b, stride=s)
    rows = x.permute(0, 2, 3, 1).reshape(-1, c) @ dpt.fold_conv_transpose(w).t()                   # [B H W, C s^2], column (co s + i) s + j
    got = rows.view(2, 5, 7, c, s, s).permute(0, 3, 1, 4, 2, 5).reshape(2, c, 5 * s, 7 * s) + b.view(1, c, 1, 1)
    assert float((got - want).abs().max()) < 1e-12


def test_from_upstream_round_trip_and_refusals(sd):
    up = DA.to_upstream(sd)
    assert "pretrained.blocks.1.attn.qkv.weight" in up and up["pretrained.blocks.1.attn.qkv.weight"].shape == (576, 192)
    assert "pretrained.blocks.3.ls2.gamma" in up and "depth_head.scratch.refinenet1.resConfUnit2.conv1.bias" in up and "depth_head.scratch.output_conv2.2.weight" in up
    assert torch.equal(up["depth_head.scratch.refinenet4.out_conv.weight"], sd["neck.fusion_stage.layers.0.projection.weight"])
    back = DA.from_upstream(up)
    assert set(back) == set(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    for bad in ("pretrained.blocks.0.attn.rope.weight", "depth_head.resize_layers.2.weight", "depth_head.scratch.stem_transpose.weight", "model.foo"):
        with pytest.raises(KeyError):
            DA.from_upstream(dict(up, **{bad: torch.zeros(1)}))
    with pytest.raises(KeyError):
        DA.to_upstream(dict(sd, **{"neck.extra.weight": torch.zeros(1)}))


# ------------------------------------------------------------------------------------------------ architecture and config
def test_presets_and_check_arch_refusals():
    from mapfree_reloc_amd.config.depth_anything_arch import PRESETS
    for name, (w, layers, heads) in dict(vits=(384, 12, 6), vitb=(768, 12, 12), vitl=(1024, 24, 16)).items():
        a = DA.check_arch(PRESETS[name])
        assert (a["VIT_WIDTH"], a["VIT_LAYERS"], a["VIT_HEADS"], a["PATCH"]) == (w, layers, heads, 14)
    assert PRESETS["vits"]["NECK_SIZES"] == (48, 96, 192, 384) and PRESETS["vitl"]["TAPS"] == (4, 11, 17, 23)      # ViT-S' 48 / 96 channels are not refused
    for bad in (dict(VIT_HEADS=4), dict(VIT_WIDTH=1536, VIT_HEADS=24), dict(SWIGLU=True), dict(HEAD_WIDTH=128), dict(VIT_WIDTH=1088, VIT_HEADS=17), dict(NOPE=1)):
        with pytest.raises(ValueError):
            DA.check_arch(dict(R.REDUCED, **bad))


def test_config_checks():
    cfg = get_cfg_defaults()
    assert cfg.DPT.NETWORK == "hybrid" and (cfg.DA.NET_HEIGHT, cfg.DA.NET_WIDTH) == (686, 518) and cfg.DA.NET_HEIGHT % 14 == 0 and cfg.DA.NET_WIDTH % 14 == 0
    dpt.check_cfg(cfg)                                                       # the defaults: DPT-Hybrid, as before
    cfg.DPT.NETWORK = "depth_anything"
    cfg.DPT.NET_HEIGHT = 70                                                  # DPT-Hybrid's size keys do not apply: not a multiple of 32, not refused
    dpt.check_cfg(cfg)
    assert DA.arch_from_cfg(cfg)["VIT_WIDTH"] == 384
    cfg.DA.ENCODER, cfg.DA.MAX_DEPTH = "vitl", 80.0
    a = DA.arch_from_cfg(cfg)
    assert (a["VIT_WIDTH"], a["MAX_DEPTH"], a["METRIC"]) == (1024, 80.0, True)
    cfg.DA.ARCH.VIT_LAYERS = 30
    assert DA.arch_from_cfg(cfg)["VIT_LAYERS"] == 30
    for key, bad in (("NET_HEIGHT", 512), ("NET_WIDTH", 0), ("NET_WIDTH", 100)):
        c = cfg.clone()
        c.DA[key] = bad
        with pytest.raises(ValueError):
            dpt.check_cfg(c)
    c = cfg.clone()
    c.DA.ENCODER = "vitg"
    with pytest.raises(ValueError):
        dpt.check_cfg(c)
    c = cfg.clone()
    c.DPT.NETWORK = "midas"
    with pytest.raises(ValueError):
        dpt.check_cfg(c)


# ------------------------------------------------------------------------------------------------ the reference maps are not a saturated sigmoid's
def test_reference_maps_are_spread(models):
    """what tests/test_gpu_depth_anything.py's end-to-end comparisons rest on, for every shape used there: >= 90 % of the float64 map inside
    (0.05, 0.95) max_depth and a standard deviation of at least 0.05 max_depth"""
    for hw in R.SHAPES:
        d64 = R.run(models[1], R.normalise(R.make_images(2, hw[0], hw[1], seed=hw[0])), capture=False)[0]
        inside, std = R.spread(d64, R.REDUCED["MAX_DEPTH"])
        print(f"[depth anything] reference {hw}: {inside:.3f} inside, std {std:.3f} of max_depth, range {float(d64.min()):.2f} .. {float(d64.max()):.2f} m")
        assert inside >= 0.9 and std >= 0.05


def test_reference_map_is_spread_vits():
    m64 = R.make_models(R.perturbed(WT.depth_anything_state_dict()), DA.check_arch(None))[1]
    inside, std = R.spread(R.run(m64, R.normalise(R.make_images(1, 70, 98, seed=70)), capture=False)[0], 20.0)
    print(f"[depth anything] reference ViT-S (70, 98): {inside:.3f} inside, std {std:.3f} of max_depth")
    assert inside >= 0.9 and std >= 0.05


# ------------------------------------------------------------------------------------------------ the C-ABI
NAMES = ["mfr_da_patch_rows", "mfr_da_patch_rows_tab", "mfr_da_tokens", "mfr_da_head_tail", "mfr_da_head_tail_rows"]


def test_entry_points_exported_and_reject_bad_arguments():
    """wrong arguments return MFR_E_ARG before anything is launched (so this runs without a GPU: no pointer is ever dereferenced)"""
    hdr = open(os.path.join(ROOT, "include", "mfr_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = mfr._lib.load()
    for n in NAMES:
        assert n + "(" in hdr and n in mfr._lib.SIGNATURES and hasattr(lib, n) and n in doc, n
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf) // 16 * 16 + 16
    E = MFR_E_ARG
    nrm = (0.485, 0.456, 0.406, 0.229, 0.224, 0.225)
    def pr(**k):
        d = dict(dict(img=p, dt=0, B=2, H=75, W=101, gh=5, gw=7, nrm=nrm, rows=p, ldk=640), **k)
        return lib.mfr_da_patch_rows(d["img"], d["dt"], d["B"], d["H"], d["W"], d["gh"], d["gw"], *d["nrm"], d["rows"], d["ldk"], None)
    for bad in (dict(img=None), dict(rows=None), dict(dt=2), dict(B=0), dict(H=0), dict(W=0), dict(gh=0), dict(gw=0), dict(ldk=584), dict(ldk=590), dict(rows=p + 4),
                dict(nrm=(0.5, 0.5, 0.5, 0.2, 0.0, 0.2)), dict(nrm=(float("nan"), 0.5, 0.5, 0.2, 0.2, 0.2))):
        assert pr(**bad) == E, bad
    def pt(**k):
        d = dict(dict(img=p, N=3, tab=p, m=2, H=75, W=101, gh=5, gw=7, rows=p, ldk=640, st=p), **k)
        return lib.mfr_da_patch_rows_tab(d["img"], d["N"], d["tab"], d["m"], d["H"], d["W"], d["gh"], d["gw"], *nrm, d["rows"], d["ldk"], d["st"], None)
    for bad in (dict(img=None), dict(tab=None), dict(rows=None), dict(st=None), dict(N=0), dict(m=0), dict(H=0), dict(gw=0), dict(ldk=100)):
        assert pt(**bad) == E, bad
    tk = lambda **k: lib.mfr_da_tokens(*[dict(dict(x=p, ldx=192, cls=p, pos=p, B=2, C=192, HW=35, out=p, ldo=192, s=None), **k)[a]
                                         for a in ("x", "ldx", "cls", "pos", "B", "C", "HW", "out", "ldo", "s")])
    for bad in (dict(x=None), dict(cls=None), dict(pos=None), dict(out=None), dict(B=0), dict(C=0), dict(C=190), dict(HW=0), dict(ldx=188), dict(ldo=190), dict(x=p + 4)):
        assert tk(**bad) == E, bad
    ht = lambda **k: lib.mfr_da_head_tail(*[dict(dict(f=p, w=p, bias=0.5, B=2, C=32, Hh=70, Wh=98, metric=1, md=20.0, Ho=50, Wo=70, m=p, mm=None, s=None), **k)[a]
                                            for a in ("f", "w", "bias", "B", "C", "Hh", "Wh", "metric", "md", "Ho", "Wo", "m", "mm", "s")])
    for bad in (dict(f=None), dict(w=None), dict(m=None), dict(B=0), dict(C=0), dict(C=65), dict(Hh=0), dict(Wo=0), dict(metric=2), dict(md=0.0), dict(md=float("nan"))):
        assert ht(**bad) == E, bad
    hr = lambda **k: lib.mfr_da_head_tail_rows(*[dict(dict(f=p, w=p, bias=0.5, B=2, C=32, Hh=70, Wh=98, metric=1, md=20.0, Ho=50, Wo=70, src=p, dst=p, d=2, m=p, mm=None, D=3, q=0,
                                                           st=p, s=None), **k)[a]
                                                 for a in ("f", "w", "bias", "B", "C", "Hh", "Wh", "metric", "md", "Ho", "Wo", "src", "dst", "d", "m", "mm", "D", "q", "st", "s")])
    for bad in (dict(f=None), dict(w=None), dict(m=None), dict(src=None), dict(dst=None), dict(st=None), dict(B=0), dict(D=0), dict(d=0), dict(C=65), dict(Ho=0), dict(metric=-1),
                dict(md=-1.0), dict(q=2)):
        assert hr(**bad) == E, bad
