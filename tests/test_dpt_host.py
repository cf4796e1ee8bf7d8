"""DPT-Hybrid depth without a GPU: the surfaces exist (config node, C-ABI entry points and their argument checks), the host-side folding equals the
float64 `transformers` module, the seeded weights keep the GPU tests' inputs well conditioned (checked on the oracle alone), the checkpoint-name
converter round-trips, and the offline writer's PNGs read back as the planes that were written.

The oracle is `transformers.DPTForDepthEstimation` (tests/dpt_ref.py); the product never imports it."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dpt_ref as R  # noqa: E402

import mapfree_reloc_amd as mfr  # noqa: E402
from mapfree_reloc_amd import compute_depth as CD  # noqa: E402
from mapfree_reloc_amd.config import get_cfg_defaults  # noqa: E402
from mapfree_reloc_amd.datasets import read_depth_image, read_depth_plane  # noqa: E402
from mapfree_reloc_amd.nets import dpt, weights as WT  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MFR_E_ARG = -1
HW = (64, 96)


# ------------------------------------------------------------------------------------------------ config and architecture
def test_config_node_and_defaults():
    node = get_cfg_defaults().DPT
    want = dict(WEIGHTS="", NET_HEIGHT=384, NET_WIDTH=512, SOURCE="file", QUANTIZE_MM=True, INVERT=True, SYNTHETIC_SEED=8642)
    assert {k: node[k] for k in want} == want and node.SCALE > 0 and node.SHIFT > 0
    assert {k: (tuple(v) if isinstance(v, list) else v) for k, v in node.ARCH.items()} == dpt.ARCH
    cfg = get_cfg_defaults()
    assert dpt.check_cfg(cfg) is cfg.DPT
    for key, bad in (("NET_HEIGHT", 380), ("NET_WIDTH", 0), ("SOURCE", "sometimes")):
        c = get_cfg_defaults()
        c.DPT[key] = bad
        with pytest.raises(ValueError):
            dpt.check_cfg(c)


def test_architecture_refuses_other_head_dimensions():
    assert dpt.check_arch(None) == dpt.ARCH and dpt.check_arch(R.REDUCED)["VIT_HEADS"] == 3
    with pytest.raises(ValueError, match="head dimension"):
        dpt.check_arch(dict(VIT_WIDTH=768, VIT_HEADS=8))                 # 96-wide heads
    with pytest.raises(ValueError, match="head dimension"):
        dpt.check_arch(dict(VIT_WIDTH=384, VIT_HEADS=12))                # 32-wide heads
    with pytest.raises(ValueError):
        dpt.check_arch(dict(NO_SUCH_KEY=1))
    with pytest.raises(ValueError):
        dpt.check_arch(dict(TAPS=(2, 5, 8, 12)))


def test_same_padding_is_asymmetric_on_even_sizes():
    assert dpt.same_padding(384, 7, 2) == (2, 3) and dpt.same_padding(96, 3, 2) == (0, 1) and dpt.same_padding(7, 3, 2) == (1, 1)
    assert dpt.same_padding(24, 1, 2) == (0, 0) and dpt.same_padding(24, 3, 1) == (1, 1)


# ------------------------------------------------------------------------------------------------ entry points
NAMES = ["mfr_dpt_prep", "mfr_dpt_groupnorm", "mfr_dpt_maxpool3s2", "mfr_dpt_layernorm", "mfr_dpt_bias_gelu", "mfr_dpt_add_relu", "mfr_dpt_tokens",
         "mfr_dpt_tokens_inverse", "mfr_dpt_shuffle", "mfr_dpt_head_tail", "mfr_conv_igemm_f16x2_pad"]


def test_entry_points_exported_and_reject_bad_arguments():
    """wrong arguments return MFR_E_ARG before anything is launched (so this runs without a GPU: no pointer is ever dereferenced)"""
    hdr = open(os.path.join(ROOT, "include", "mfr_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = mfr._lib.load()
    for n in NAMES:
        assert n + "(" in hdr and n in mfr._lib.SIGNATURES and hasattr(lib, n) and n in doc, n
    assert lib.mfr_abi_version() == 6
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf) // 16 * 16 + 16
    E = MFR_E_ARG
    assert lib.mfr_dpt_prep(None, 0, 1, 50, 70, p, 64, 96, None) == E and lib.mfr_dpt_prep(p, 0, 1, 50, 70, None, 64, 96, None) == E
    assert lib.mfr_dpt_prep(p, 2, 1, 50, 70, p, 64, 96, None) == E and lib.mfr_dpt_prep(p, 0, 0, 50, 70, p, 64, 96, None) == E
    assert lib.mfr_dpt_prep(p, 0, 1, 50, 70, p, 60, 96, None) == E and lib.mfr_dpt_prep(p, 1, 1, 50, 70, p, 64, 100, None) == E
    assert lib.mfr_dpt_prep(p, 1, 1, 0, 70, p, 64, 96, None) == E and lib.mfr_dpt_prep(p, 1, 1, 50, 70, p, 0, 96, None) == E
    gn = lambda **k: lib.mfr_dpt_groupnorm(*[dict(dict(x=p, g=p, b=p, r=None, B=2, C=64, HW=15, G=8, eps=1e-5, relu=1, y=p, s=None), **k)[a]
                                             for a in ("x", "g", "b", "r", "B", "C", "HW", "G", "eps", "relu", "y", "s")])
    for bad in (dict(x=None), dict(g=None), dict(b=None), dict(y=None), dict(B=0), dict(C=0), dict(HW=0), dict(G=0), dict(G=7), dict(eps=-1.0), dict(relu=2)):
        assert gn(**bad) == E, bad
    mp = lambda **k: lib.mfr_dpt_maxpool3s2(*[dict(dict(x=p, n=4, H=8, W=8, pt=0, pb=1, pl=0, pr=1, y=p, s=None), **k)[a] for a in ("x", "n", "H", "W", "pt", "pb", "pl", "pr", "y", "s")])
    for bad in (dict(x=None), dict(y=None), dict(n=0), dict(H=0), dict(W=-3), dict(pt=3), dict(pb=-1), dict(pl=3), dict(pr=3), dict(H=1, pt=0, pb=1)):
        assert mp(**bad) == E, bad
    ln = lambda **k: lib.mfr_dpt_layernorm(*[dict(dict(x=p, ldx=192, g=p, b=p, r=None, ldr=0, rows=4, C=192, eps=1e-12, o=p, ldo=192, s=None), **k)[a]
                                             for a in ("x", "ldx", "g", "b", "r", "ldr", "rows", "C", "eps", "o", "ldo", "s")])
    for bad in (dict(x=None), dict(g=None), dict(b=None), dict(o=None), dict(rows=0), dict(C=100), dict(C=0), dict(C=2048), dict(ldx=128), dict(ldo=191),
                dict(r=p, ldr=64), dict(eps=-1.0)):
        assert ln(**bad) == E, bad
    assert lib.mfr_dpt_bias_gelu(None, 384, 4, 384, p, None) == E and lib.mfr_dpt_bias_gelu(p, 384, 0, 384, p, None) == E
    assert lib.mfr_dpt_bias_gelu(p, 384, 4, 382, p, None) == E and lib.mfr_dpt_bias_gelu(p, 380, 4, 384, p, None) == E
    assert lib.mfr_dpt_bias_gelu(p + 4, 384, 4, 384, p, None) == E and lib.mfr_dpt_bias_gelu(p, 384, 4, 384, p + 8, None) == E
    assert lib.mfr_dpt_add_relu(None, p, 64, p, p, None) == E and lib.mfr_dpt_add_relu(p, p, 64, p, None, None) == E
    assert lib.mfr_dpt_add_relu(p, p, 62, p, p, None) == E and lib.mfr_dpt_add_relu(p, p, 0, p, p, None) == E and lib.mfr_dpt_add_relu(p, p + 4, 64, p, p, None) == E
    assert lib.mfr_dpt_tokens(None, p, p, 2, 192, 24, p, 192, None) == E and lib.mfr_dpt_tokens(p, None, p, 2, 192, 24, p, 192, None) == E
    assert lib.mfr_dpt_tokens(p, p, None, 2, 192, 24, p, 192, None) == E and lib.mfr_dpt_tokens(p, p, p, 2, 192, 24, None, 192, None) == E
    assert lib.mfr_dpt_tokens(p, p, p, 0, 192, 24, p, 192, None) == E and lib.mfr_dpt_tokens(p, p, p, 2, 192, 0, p, 192, None) == E
    assert lib.mfr_dpt_tokens(p, p, p, 2, 192, 24, p, 191, None) == E
    assert lib.mfr_dpt_tokens_inverse(None, 192, 25 * 192, 1, p, 1, 2, 192, 24, p, None) == E
    assert lib.mfr_dpt_tokens_inverse(p, 192, 25 * 192, 1, p, 1, 2, 192, 24, None, None) == E
    assert lib.mfr_dpt_tokens_inverse(p, 191, 25 * 192, 1, p, 1, 2, 192, 24, p, None) == E            # rows shorter than C
    assert lib.mfr_dpt_tokens_inverse(p, 192, 24 * 192, 1, p, 1, 2, 192, 24, p, None) == E            # an image's rows would run into the next image
    assert lib.mfr_dpt_tokens_inverse(p, 192, 25 * 192, -1, p, 1, 2, 192, 24, p, None) == E and lib.mfr_dpt_tokens_inverse(p, 192, 25 * 192, 1, p, 2, 2, 192, 24, p, None) == E
    assert lib.mfr_dpt_shuffle(None, 128, p, 2, 8, 2, 3, 4, p, None) == E and lib.mfr_dpt_shuffle(p, 128, p, 2, 8, 2, 3, 4, None, None) == E
    assert lib.mfr_dpt_shuffle(p, 128, p, 2, 8, 2, 3, 3, p, None) == E and lib.mfr_dpt_shuffle(p, 127, p, 2, 8, 2, 3, 4, p, None) == E
    assert lib.mfr_dpt_shuffle(p, 128, p, 0, 8, 2, 3, 4, p, None) == E and lib.mfr_dpt_shuffle(p, 128, p, 2, 8, 0, 3, 4, p, None) == E
    ht = lambda **k: lib.mfr_dpt_head_tail(*[dict(dict(f=p, w=p, bias=1.0, B=2, C=32, Hh=64, Wh=96, inv=0, sc=1.0, sh=0.0, Ho=50, Wo=70, m=p, mm=None, s=None), **k)[a]
                                             for a in ("f", "w", "bias", "B", "C", "Hh", "Wh", "inv", "sc", "sh", "Ho", "Wo", "m", "mm", "s")])
    for bad in (dict(f=None), dict(w=None), dict(m=None), dict(B=0), dict(C=0), dict(C=65), dict(Hh=0), dict(Wo=0), dict(inv=2), dict(inv=1, sc=float("nan"))):
        assert ht(**bad) == E, bad
    cv = lambda **k: lib.mfr_conv_igemm_f16x2_pad(*[dict(dict(x=p, w=p, b=None, y=p, B=1, ci=3, H=64, W=96, co=32, kh=7, kw=7, st=2, lo=2, hi=3, relu=0, s=None), **k)[a]
                                                    for a in ("x", "w", "b", "y", "B", "ci", "H", "W", "co", "kh", "kw", "st", "lo", "hi", "relu", "s")])
    for bad in (dict(x=None), dict(w=None), dict(y=None), dict(B=0), dict(lo=-1), dict(hi=-1), dict(st=0), dict(H=0)):
        assert cv(**bad) == E, bad


# ------------------------------------------------------------------------------------------------ the oracle on the seeded weights
@pytest.fixture(scope="module")
def orc():
    sd = R.perturbed(WT.dpt_state_dict(arch=R.REDUCED))
    m32, m64 = R.make_models(sd, dpt.check_arch(R.REDUCED))
    x = (R.make_images(2, *HW, seed=HW[0]) - 0.5) / 0.5
    d64, c64 = R.run(m64, x)
    return dict(sd=sd, m32=m32, m64=m64, x=x, d64=d64, c64=c64)


def _close(a, b, what):
    err = float((a.double() - b.double()).abs().max() / b.double().abs().max())
    assert a.shape == b.shape and err <= 1e-6, (what, err)


def test_state_dict_is_the_modules(orc):
    """make_models loads strictly: the recipe names every parameter of the module and nothing else; DPT-Hybrid's own shapes likewise"""
    full = WT.dpt_state_dict()
    assert full["dpt.embeddings.position_embeddings"].shape == (1, 577, 768) and full["neck.convs.3.weight"].shape == (256, 768, 3, 3)
    assert sum(v.numel() for v in full.values()) > 120e6
    from transformers import DPTForDepthEstimation
    with torch.device("meta"):
        ref = DPTForDepthEstimation(R.hf_config(dpt.ARCH))
    assert {k: tuple(v.shape) for k, v in ref.state_dict().items()} == {k: tuple(v.shape) for k, v in full.items()}


BIT = "dpt.embeddings.backbone.bit"


def test_fold_weight_standardisation(orc):
    c64, sd = orc["c64"], orc["sd"]
    (x,), y = c64[f"{BIT}.embedder.convolution"]
    w = dpt.fold_weight_standardisation(sd[f"{BIT}.embedder.convolution.weight"], dpt.STEM_EPS)
    lo, hi = dpt.same_padding(HW[0], 7, 2)
    _close(F.conv2d(F.pad(x, (lo, hi, lo, hi)), w, stride=2), y, "stem")
    name = f"{BIT}.encoder.stages.1.layers.0.conv2"                       # 3x3 / 2: (0, 1)
    (x,), y = c64[name]
    w = dpt.fold_weight_standardisation(sd[name + ".weight"], dpt.BOTTLENECK_EPS)
    lo, hi = dpt.same_padding(x.shape[2], 3, 2)
    assert (lo, hi) == (0, 1)
    _close(F.conv2d(F.pad(x, (lo, hi, lo, hi)), w, stride=2), y, "conv2 / 2")
    name = f"{BIT}.encoder.stages.1.layers.0.downsample.conv"             # 1x1 / 2: no padding
    (x,), y = c64[name]
    _close(F.conv2d(x, dpt.fold_weight_standardisation(sd[name + ".weight"], dpt.BOTTLENECK_EPS), stride=2), y, "downsample")


def test_fold_qkv_and_readout_split(orc):
    c64, sd = orc["c64"], orc["sd"]
    (x,), _ = c64["dpt.encoder.layer.2.attention.attention.query"]
    w, b = dpt.fold_qkv(sd, "dpt.encoder.layer.2")
    got = x @ w.t() + b
    for j, n in enumerate(("query", "key", "value")):
        _close(got[..., 192 * j:192 * (j + 1)], c64[f"dpt.encoder.layer.2.attention.attention.{n}"][1], n)
    for i in (2, 3):
        hidden = c64["__taps__"][0][i]                                   # [B, 1 + gh gw, h]
        wa, wb, b = dpt.fold_readout(sd[f"neck.reassemble_stage.readout_projects.{i}.0.weight"], sd[f"neck.reassemble_stage.readout_projects.{i}.0.bias"])
        img_bias = dpt.readout_image_bias(wb, b, hidden[:, 0])           # [B, h]
        got = F.gelu(hidden[:, 1:] @ wa.t() + img_bias[:, None])
        _close(got, c64[f"neck.reassemble_stage.readout_projects.{i}"][1], f"readout {i}")


@pytest.mark.parametrize("s", [4, 2])
def test_fold_conv_transpose(s):
    g = torch.Generator().manual_seed(s)
    B, ci, co, H, W = 2, 32, 8, 2, 3
    x, w, b = (torch.randn(B, ci, H, W, generator=g, dtype=torch.float64), torch.randn(ci, co, s, s, generator=g, dtype=torch.float64),
               torch.randn(co, generator=g, dtype=torch.float64))
    rows = x.permute(0, 2, 3, 1).reshape(B * H * W, ci) @ dpt.fold_conv_transpose(w).t()      # [B H W, co s s], column (co s + i) s + j
    got = rows.reshape(B, H, W, co, s, s).permute(0, 3, 1, 4, 2, 5).reshape(B, co, H * s, W * s) + b[None, :, None, None]
    _close(got, F.conv_transpose2d(x, w, b, stride=s), f"conv transpose x{s}")


@pytest.mark.parametrize("grid", [(4, 6), (6, 2), (24, 24)])
def test_position_embedding_resize(orc, grid):
    pos = orc["sd"]["dpt.embeddings.position_embeddings"]
    want = orc["m64"].dpt.embeddings._resize_pos_embed(pos.double(), *grid)[0]
    got = dpt.resize_position_embeddings(pos, *grid)
    _close(got, want, grid)
    assert torch.equal(got[0], pos[0, 0].double())                                            # the cls row is kept


def test_gpu_test_inputs_are_well_conditioned(orc):
    """at most 1 % of the float64 output at the final ReLU's zero (dead pixels hide errors); every tapped activation finite and within 1e4 -- on the
    reduced configuration at both test shapes, and on DPT-Hybrid at the shape of its end-to-end test.  Without the lifted last bias the recipe fails this"""
    def conditions(m64, shapes, batch):
        for hw in shapes:
            d, caps = R.run(m64, (R.make_images(batch, *hw, seed=hw[0]) - 0.5) / 0.5)
            assert float((d == 0).double().mean()) <= 0.01, hw
            for t in caps["__taps__"][0]:
                assert bool(torch.isfinite(t).all()) and float(t.abs().max()) <= 1e4
            assert 0.2 < float(d.min()) and float(d.max()) < 20.0                              # reads as metres: the millimetre plane is inside u16
    conditions(orc["m64"], [(64, 96), (96, 32)], 2)
    conditions(R.make_models(R.perturbed(WT.dpt_state_dict()), dpt.ARCH)[1], [(128, 160)], 1)
    flat = R.perturbed(WT.dpt_state_dict(arch=R.REDUCED, head_bias=0.0))
    d, _ = R.run(R.make_models(flat, dpt.check_arch(R.REDUCED))[1], orc["x"], capture=False)
    assert float((d == 0).double().mean()) > 0.01


# ------------------------------------------------------------------------------------------------ checkpoint names
def _to_upstream(sd):
    """the inverse of nets/dpt.from_upstream, written independently: names as the authors' repository has them, q / k / v fused"""
    out = {}
    for k, v in sd.items():
        n = k
        n = re.sub(r"^dpt\.embeddings\.backbone\.bit\.embedder\.convolution\.", "pretrained.model.patch_embed.backbone.stem.conv.", n)
        n = re.sub(r"^dpt\.embeddings\.backbone\.bit\.embedder\.norm\.", "pretrained.model.patch_embed.backbone.stem.norm.", n)
        n = re.sub(r"^dpt\.embeddings\.backbone\.bit\.encoder\.stages\.(\d+)\.layers\.(\d+)\.", r"pretrained.model.patch_embed.backbone.stages.\1.blocks.\2.", n)
        n = n.replace("dpt.embeddings.projection.", "pretrained.model.patch_embed.proj.")
        n = n.replace("dpt.embeddings.cls_token", "pretrained.model.cls_token").replace("dpt.embeddings.position_embeddings", "pretrained.model.pos_embed")
        n = n.replace("dpt.layernorm.", "pretrained.model.norm.")
        m = re.match(r"dpt\.encoder\.layer\.(\d+)\.(.+)\.(weight|bias)$", n)
        if m:
            i, what, wb = m.groups()
            if what.startswith("attention.attention."):
                continue
            what = {"layernorm_before": "norm1", "layernorm_after": "norm2", "attention.output.dense": "attn.proj", "intermediate.dense": "mlp.fc1",
                    "output.dense": "mlp.fc2"}[what]
            n = f"pretrained.model.blocks.{i}.{what}.{wb}"
        m = re.match(r"neck\.reassemble_stage\.readout_projects\.(\d)\.0\.(weight|bias)$", n)
        if m:
            n = f"pretrained.act_postprocess{int(m.group(1)) + 1}.0.project.0.{m.group(2)}"
        m = re.match(r"neck\.reassemble_stage\.layers\.(\d)\.(projection|resize)\.(weight|bias)$", n)
        if m:
            n = f"pretrained.act_postprocess{int(m.group(1)) + 1}.{3 if m.group(2) == 'projection' else 4}.{m.group(3)}"
        m = re.match(r"neck\.convs\.(\d)\.weight$", n)
        if m:
            n = f"scratch.layer{int(m.group(1)) + 1}_rn.weight"
        m = re.match(r"neck\.fusion_stage\.layers\.(\d)\.(.+)\.(weight|bias)$", n)
        if m:
            what = m.group(2).replace("projection", "out_conv").replace("residual_layer", "resConfUnit").replace("convolution", "conv")
            n = f"scratch.refinenet{4 - int(m.group(1))}.{what}.{m.group(3)}"
        n = n.replace("head.head.", "scratch.output_conv.")
        out[n] = v
    layers = {int(m.group(1)) for m in (re.match(r"dpt\.encoder\.layer\.(\d+)\.", k) for k in sd) if m}
    for i in layers:
        for wb in ("weight", "bias"):
            out[f"pretrained.model.blocks.{i}.attn.qkv.{wb}"] = torch.cat([sd[f"dpt.encoder.layer.{i}.attention.attention.{n}.{wb}"] for n in ("query", "key", "value")])
    return out


def test_from_upstream_round_trip(orc):
    up = _to_upstream(orc["sd"])
    assert "pretrained.model.blocks.3.attn.qkv.weight" in up and "scratch.refinenet4.resConfUnit2.conv1.bias" in up and "scratch.output_conv.4.bias" in up
    assert not any(k.startswith(("dpt.", "neck.", "head.")) for k in up)
    back = dpt.from_upstream(up)
    assert set(back) == set(orc["sd"])
    assert all(torch.equal(back[k], orc["sd"][k]) for k in back)
    with pytest.raises(KeyError):
        dpt.from_upstream({"scratch.refinenet5.out_conv.weight": torch.zeros(1)})
    with pytest.raises(KeyError):
        dpt.from_upstream({"auxlayer.0.weight": torch.zeros(1)})


# ------------------------------------------------------------------------------------------------ millimetre planes on disk
def test_depth_png_reads_back_as_the_plane_written(tmp_path):
    rng = np.random.default_rng(0)
    mm = rng.integers(0, 65536, size=(37, 53), dtype=np.uint16)
    mm[0, :4] = (0, 1, 65535, 1000)
    frame = tmp_path / "seq1" / "frame_00003.jpg"
    frame.parent.mkdir()
    path = CD.depth_path("Mapfree", frame, "dptsynth")
    assert path == str(tmp_path / "seq1" / "frame_00003.dptsynth.png")
    assert CD.depth_path("7Scenes", "seq-01/frame-000012.color.png", "dptnyu") == "seq-01/frame-000012.depth.dptnyu.png"
    CD.write_depth_png(path, mm)
    assert sorted(os.listdir(frame.parent)) == ["frame_00003.dptsynth.png"]                   # no temporary file is left
    want = (mm / 1000).astype(np.float32)
    assert np.array_equal(read_depth_plane(path), want) and np.array_equal(read_depth_image(path).numpy(), want)
    from PIL import Image
    with Image.open(path) as im:
        assert im.mode in ("I;16", "I;16B", "I") and im.size == (53, 37)
    assert np.array_equal(dpt.millimetres_to_metres(torch.from_numpy(mm)).numpy(), want)      # the online route's conversion: the reader's bits
    with pytest.raises(AssertionError):
        CD.write_depth_png(path, mm.astype(np.int32))


def test_compute_depth_lists_frames_where_the_readers_look(tmp_path):
    for rel in ("val/s00001/seq0/frame_00000.jpg", "val/s00001/seq1/frame_00005.jpg", "val/s00001/seq1/frame_00005.dptkitti.png", "test/s00002/seq1/frame_00000.jpg"):
        (tmp_path / rel).parent.mkdir(parents=True, exist_ok=True)
        (tmp_path / rel).write_bytes(b"")
    dirs = CD.list_scene_dirs("Mapfree", tmp_path)
    assert [d.name for d in dirs] == ["s00001", "s00002"] and [d.name for d in CD.list_scene_dirs("Mapfree", tmp_path, ["s00002"])] == ["s00002"]
    assert [os.path.relpath(f, dirs[0]) for f in CD.scene_frames("Mapfree", dirs[0])] == ["seq0/frame_00000.jpg", "seq1/frame_00005.jpg"]


def test_scannet_depth_npz_reads_back_through_the_reader(tmp_path):
    """-ds Scannet: one .npz of float metres at WIDTH x HEIGHT under the reader's keys; ScanNetScene._depth loads what the estimator returned.  The estimator
    here is a stand-in (no GPU): what is under test is the frame list, the keys, the sizes, the atomic write and the skip"""
    import scannet_tree as ST
    from mapfree_reloc_amd.scannet import ScanNetScene
    p = ST.default_params()
    tr = ST.write_tree(tmp_path, p)
    W, H = int(p["width"]), int(p["height"])
    seen = []

    class Fake:
        def metres(self, images, out_hw):
            assert images.dtype == torch.uint8 and images.shape[1:] == (10, 13, 3) and out_hw == (H, W)
            seen.append(images.shape[0])
            base = images.reshape(images.shape[0], -1).float().mean(1)             # one value per frame, from its pixels
            return base[:, None, None] / 64 + torch.arange(H * W, dtype=torch.float32).reshape(1, H, W) / 1000
    frames = CD.scannet_frames(tr["test_npz"])
    assert frames == [(707, 0, 0), (707, 0, 45), (707, 0, 150), (711, 1, 15), (711, 1, 300)] and CD.scannet_key(707, 0, 45) == "0707_00_frame_000045"
    out = str(tmp_path / "misc" / "dpt.npz")
    assert CD.run_scannet(Fake(), tr["scans"], tr["test_npz"], out, (W, H), batch=2) == (5, 0) and seen == [2, 2, 1]
    assert os.listdir(tmp_path / "misc") == ["dpt.npz"]                              # no temporary file is left
    assert CD.run_scannet(Fake(), tr["scans"], tr["test_npz"], out, (W, H), batch=2) == (0, 5) and seen == [2, 2, 1]
    sc = ScanNetScene(tr["scans"], tr["test_npz"], mode="test", resize=(W, H), estimated_depth=out)
    from PIL import Image
    for scene, sub, stem in frames:
        a = torch.from_numpy(np.array(Image.open(os.path.join(tr["scans"], f"scene{scene:04d}_{sub:02d}", "sensor_data", f"frame-{stem:06}.color.jpg")).convert("RGB")))
        want = Fake().metres(a[None], (H, W))[0].numpy()
        got = sc._depth(f"scene{scene:04d}_{sub:02d}", stem, out=np.empty((H, W), np.float32))
        assert got.dtype == np.float32 and np.array_equal(got, want)
    assert sc[0]["depth0"].shape == (H, W)
    with pytest.raises(AssertionError):
        CD.write_depth_npz(str(tmp_path / "bad.npz"), {"k": np.zeros((2, 2))})       # float64 maps are refused
