"""-m gpu: the EfficientLoFTR stage (nets/eloftr.py, csrc/eloftr.hip) against the `transformers` module, stage by stage and end to end, in both
HIP.SPLIT arithmetics (tests/eloftr_ref.py is the oracle and says where the whole module is not).

Continuous stages: the device stage is fed the float32 oracle's INPUT tensors and compared with the float64 oracle on the same tensors;
err(device) <= 10 x err(float32 oracle), max and rms, both printed (the bar of tests/test_gpu_matcher_wiring.py).  Discrete decisions (coarse
matches, the fine stage's arg-max) must be EQUAL wherever the float64 oracle's decision is safe (eloftr_ref.coarse_safe / fine_stage1); coordinates:
error <= max(10 x the float32 oracle's, 1e-3 px).  Shapes: B = 2 pairs at 96 x 128 (coarse 12 x 16, aggregated 3 x 4) and 160 x 96 (coarse
20 x 12, aggregated 5 x 3: odd), weights with every BatchNorm / LayerNorm term non-trivial (eloftr_ref.perturbed)."""
import numpy as np
import pytest
import torch

import eloftr_ref as R
from mapfree_reloc_amd import options
from mapfree_reloc_amd.nets import eloftr as EL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPLITS = ("f16x2", "bf16x3")
LAYER = 1                         # the transformer layer of the single-block stages (not the first: its weights differ from layer 0's)


@pytest.fixture(scope="module")
def hip():
    """split -> the device module built under that arithmetic (built once; every call runs inside the same override)"""
    built = {}

    def get(split):
        if split not in built:
            with options.override(SPLIT=split):
                built[split] = EL.EfficientLoFTRHIP(R.weights("perturbed"), DEV)
        return built[split]
    return get


@pytest.fixture(scope="module")
def oracle():
    """(H, W) -> the oracle's tensors of every stage in float32 and, on the float32 inputs, in float64.  Computed once per shape, never modified."""
    m32, m64 = R.modules("perturbed")
    cache = {}

    @torch.no_grad()
    def get(hw):
        if hw in cache:
            return cache[hw]
        o = {}
        x = torch.cat([R.noise_pair(hw, 21), R.noise_pair(hw, 22, 0.05)])                        # [4,1,H,W]: two pairs
        o["x"] = x
        o["bb32"], o["bb64"] = R.backbone(m32, x), R.backbone(m64, x.double())
        s1, s2, s3 = o["bb32"]
        d = lambda t: t.double()
        o["agg32"], o["agg64"] = R.aggregation(m32, LAYER, "self", s3), R.aggregation(m64, LAYER, "self", d(s3))
        q, kv = o["agg32"]
        o["rot32"], o["rot64"] = R.rotary_qk(m32, LAYER, q, kv, s3), R.rotary_qk(m64, LAYER, d(q), d(kv), d(s3))
        o["self32"], o["self64"] = R.self_block(m32, LAYER, s3), R.self_block(m64, LAYER, d(s3))
        x0, x1 = s3[0::2], s3[1::2]
        o["cross32"], o["cross64"] = R.cross_pair(m32, LAYER, x0, x1), R.cross_pair(m64, LAYER, d(x0), d(x1))
        o["stale64"] = R.block_of(m64, LAYER, "cross")(d(x1), d(x0))                              # image 1 against the NOT updated image 0
        o["tr32"], o["tr64"] = R.transformer(m32, s3), R.transformer(m64, d(s3))
        c = o["tr32"]
        o["half32"], o["half64"] = R.pyramid_half(m32, c, s2, s1), R.pyramid_half(m64, d(c), d(s2), d(s1))
        # windows: the module's refinement layer (float64, on the float32 coarse map) == up-sample + unfold of ITS OWN half map; the stage under test
        # starts from the float32 half map, so that is the input both references take
        w64 = R.windows(m64, d(c), d(s2), d(s1))
        up = lambda t: torch.nn.functional.interpolate(t, scale_factor=2.0, mode="bilinear", align_corners=False)

        def unfold(half):
            full = up(half)
            n, C = full.shape[:2]
            a = torch.nn.functional.unfold(full[0::2], kernel_size=8, stride=8, padding=0).reshape(n // 2, C, 64, -1).permute(0, 3, 2, 1)
            b = torch.nn.functional.unfold(full[1::2], kernel_size=10, stride=8, padding=1).reshape(n // 2, C, 100, -1).permute(0, 3, 2, 1)
            return a, b
        mirror = unfold(o["half64"])
        assert all(float((a - b).abs().max()) <= 1e-12 * float(b.abs().max()) for a, b in zip(mirror, w64))
        o["win32"], o["win64"] = unfold(o["half32"]), unfold(d(o["half32"]))
        cache[hw] = o
        return o
    return get


def _rows(maps):
    """NCHW maps -> the transformer's token buffer [n * L, 512] on the device, x in the left half"""
    n, C, h, w = maps.shape
    xm = torch.zeros(n * h * w, 2 * C, dtype=torch.float32, device=DEV)
    xm[:, :C] = maps.permute(0, 2, 3, 1).reshape(n * h * w, C).to(DEV)
    return xm


def _maps(xm, n, hw):
    return xm[:, :EL.HIDDEN].reshape(n, hw[0], hw[1], EL.HIDDEN).permute(0, 3, 1, 2).cpu()


@pytest.mark.parametrize("hw", R.SHAPES)
@pytest.mark.parametrize("split", SPLITS)
def test_backbone_vs_float64(oracle, hip, split, hw):
    """21 folded RepVGG blocks: the stride-2 stem, the stride-1 and stride-2 3x3 kernels, the three kept maps"""
    o = oracle(hw)
    with options.override(SPLIT=split), torch.no_grad():
        f = hip(split).backbone(o["x"].to(DEV))
    for name, got, a, b in zip(("1/2", "1/4", "1/8"), f, o["bb32"], o["bb64"]):
        R.check(f"backbone {name} map [{split} {hw}]", got.cpu(), a, b)


@pytest.mark.parametrize("hw", R.SHAPES)
def test_stem_is_the_stride_2_convolution(hip, hw):
    """mfr_eloftr_stem_s2 alone against a float64 convolution of the folded filter (2e-5: the project's convolution tolerance)"""
    net = hip("f16x2")
    x = R.noise_pair(hw, 3)
    with torch.no_grad():
        got = net.stem_s2(x.to(DEV)).cpu()
    w, b = net.stem
    want = torch.relu(torch.nn.functional.conv2d(x.double(), w.cpu().double(), b.cpu().double(), stride=2, padding=1))
    assert got.shape == want.shape and float((got.double() - want).abs().max()) <= 2e-5 * float(want.abs().max())


@pytest.mark.parametrize("hw", R.SHAPES)
def test_aggregation_tokens_vs_float64(oracle, hip, hw):
    """q (depthwise 4x4 / 4 convolution) and kv (4x4 / 4 max-pool) through the SAME LayerNorm, separately"""
    o = oracle(hw)
    net = hip("f16x2")
    s3 = o["bb32"][2]
    n, _, h, w = s3.shape
    with torch.no_grad():
        q, kv = net.aggregate(net.layers[LAYER]["self"], _rows(s3)[:, :EL.HIDDEN], n, (h, w))
    R.check(f"aggregation q tokens [{hw}]", q.reshape(n, -1, 256).cpu(), o["agg32"][0], o["agg64"][0])
    R.check(f"aggregation kv tokens [{hw}]", kv.reshape(n, -1, 256).cpu(), o["agg32"][1], o["agg64"][1])


@pytest.mark.parametrize("hw", R.SHAPES)
@pytest.mark.parametrize("split", SPLITS)
def test_rotary_qk_vs_float64(oracle, hip, split, hw):
    """q_proj / k_proj (no bias) and the interleaved-pair rotation of the whole 256-vector by the aggregated grid's 1-based row / column angles"""
    o = oracle(hw)
    q_tok, kv_tok = (t.reshape(-1, 256).to(DEV) for t in o["agg32"])
    n = o["agg32"][0].shape[0]
    with options.override(SPLIT=split), torch.no_grad():
        net = hip(split)
        blk = net.layers[LAYER]["self"]
        qkv = torch.empty(q_tok.shape[0], 768, dtype=torch.float32, device=DEV)
        blk["lq"](q_tok, out=qkv[:, :256]); blk["lkv"](kv_tok, out=qkv[:, 256:])
        net.rotary(qkv, (hw[0] // 32, hw[1] // 32))
    R.check(f"rotary q [{split} {hw}]", qkv[:, :256].reshape(n, -1, 256).cpu(), o["rot32"][0], o["rot64"][0])
    R.check(f"rotary k [{split} {hw}]", qkv[:, 256:512].reshape(n, -1, 256).cpu(), o["rot32"][1], o["rot64"][1])


@pytest.mark.parametrize("hw", R.SHAPES)
@pytest.mark.parametrize("split", SPLITS)
def test_self_block_vs_float64(oracle, hip, split, hw):
    o = oracle(hw)
    s3 = o["bb32"][2]
    n, _, h, w = s3.shape
    with options.override(SPLIT=split), torch.no_grad():
        net = hip(split)
        xm = _rows(s3)
        net.block(net.layers[LAYER]["self"], xm, xm, n, (h, w), True)
    R.check(f"self block [{split} {hw}]", _maps(xm, n, (h, w)), o["self32"], o["self64"])


@pytest.mark.parametrize("hw", R.SHAPES)
@pytest.mark.parametrize("split", SPLITS)
def test_cross_pair_vs_float64(oracle, hip, split, hw):
    """image 0 attends to image 1, image 1 to the UPDATED image 0, no rotary: the stale variant lies far outside the bar, so a device that uses it fails"""
    o = oracle(hw)
    s3 = o["bb32"][2]
    B, (h, w) = s3.shape[0] // 2, s3.shape[2:]
    with options.override(SPLIT=split), torch.no_grad():
        net = hip(split)
        x0, x1 = _rows(s3[0::2]), _rows(s3[1::2])
        net.block(net.layers[LAYER]["cross"], x0, x1, B, (h, w), False)
        net.block(net.layers[LAYER]["cross"], x1, x0, B, (h, w), False)
    R.check(f"cross pair, image 0 [{split} {hw}]", _maps(x0, B, (h, w)), o["cross32"][0], o["cross64"][0])
    R.check(f"cross pair, image 1 [{split} {hw}]", _maps(x1, B, (h, w)), o["cross32"][1], o["cross64"][1])
    stale, e32 = R.err(o["stale64"], o["cross64"][1]), R.err(o["cross32"][1], o["cross64"][1])
    assert stale[0] > 10 * R.FACTOR * e32[0], (stale, e32)                 # ten times outside the bar


@pytest.mark.parametrize("hw", R.SHAPES)
@pytest.mark.parametrize("split", SPLITS)
def test_transformer_vs_float64(oracle, hip, split, hw):
    """tokens from the feature set (interleaved pairs, by index), 4 x (self, cross pair)"""
    o = oracle(hw)
    s1, s2, s3 = (t.to(DEV) for t in o["bb32"])
    n, _, h, w = s3.shape
    with options.override(SPLIT=split), torch.no_grad():
        net = hip(split)
        f = EL.ELoFTRFeatures(s1, s2, s3)
        xm = net.transformer(net.tokens(f, range(0, n, 2), f, range(1, n, 2)), n // 2, (h, w))
    got = _maps(xm.view(-1, 512), n, (h, w))                                                  # side-major
    R.check(f"transformer [{split} {hw}]", got, R.to_side_major(o["tr32"]), R.to_side_major(o["tr64"]))


@pytest.mark.parametrize("hw", R.SHAPES)
@pytest.mark.parametrize("split", SPLITS)
def test_fine_pyramid_vs_float64(oracle, hip, split, hw):
    """coarse map / 16 (the hand-over kernel), out_conv, x2, two OutConvBlocks with the folded BatchNorm: the half-resolution 64-channel map"""
    o = oracle(hw)
    s1, s2, _ = o["bb32"]
    c = o["tr32"]
    n, _, h, w = c.shape
    with options.override(SPLIT=split), torch.no_grad():
        net = hip(split)
        cm = net.coarse_map(_rows(c).view(1, -1, 512), n, (h, w))
        assert torch.equal(cm.cpu(), c / 16.0)
        half = net.pyramid(cm, s2.to(DEV), s1.to(DEV))
    R.check(f"fine pyramid [{split} {hw}]", half.cpu(), o["half32"].permute(0, 2, 3, 1), o["half64"].permute(0, 2, 3, 1))


@pytest.mark.parametrize("hw", R.SHAPES)
def test_windows_vs_float64(oracle, hip, hw):
    """EVERY cell's windows, border cells included (the 10 x 10 window reads unfold's zero padding there), with the last x2 up-sampling inside the gather"""
    o = oracle(hw)
    net = hip("f16x2")
    half = R.to_side_major(o["half32"]).permute(0, 2, 3, 1).contiguous().to(DEV)
    B, (hc, wc) = half.shape[0] // 2, (hw[0] // 8, hw[1] // 8)
    L = hc * wc
    cells = torch.arange(L, dtype=torch.int32, device=DEV).repeat(B, 1).contiguous()
    n = torch.full((B,), L, dtype=torch.int32, device=DEV)
    side = torch.arange(2 * B, dtype=torch.int32, device=DEV)
    with torch.no_grad():
        w0 = net.gather_windows(half, side[:B], cells, n, L, wc, 8, 0).reshape(B, L, 64, 64)
        w1 = net.gather_windows(half, side[B:], cells, n, L, wc, 10, 1).reshape(B, L, 100, 64)
    R.check(f"windows of image 0 [{hw}]", w0.cpu(), o["win32"][0], o["win64"][0])
    R.check(f"windows of image 1 [{hw}]", w1.cpu(), o["win32"][1], o["win64"][1])
    border = o["win64"][1][:, 0]                                                                # cell (0, 0): row 0 and column 0 of the window are padding
    assert float(border.reshape(-1, 10, 10, 64)[:, 0].abs().max()) == 0 and float(w1[:, 0].reshape(-1, 10, 10, 64)[:, :, 0].abs().max()) == 0


@pytest.mark.parametrize("hw", R.SHAPES)
@pytest.mark.parametrize("split", SPLITS)
def test_coarse_matching_on_constructed_features(hip, split, hw):
    """permuted features with confidences on both sides of the threshold: equal indices on every safe cell, nothing within 2 cells of an edge"""
    hc, wc = hw[0] // 8, hw[1] // 8
    f0, f1, _ = R.constructed_coarse((hc, wc))
    conf = R.coarse_confidence(f0, f1)
    want, _ = R.coarse_matches(R.modules("perturbed")[1], conf, (hc, wc))
    safe = R.coarse_safe(conf)
    with options.override(SPLIT=split), torch.no_grad():
        i_ids, j_ids, mconf, n = hip(split).coarse_match_features(f0.float().to(DEV), f1.float().to(DEV), (hc, wc))
    i_ids, j_ids, n = i_ids.cpu().long(), j_ids.cpu().long(), n.cpu()
    for b in range(f0.shape[0]):
        got = torch.full((hc * wc,), -1)
        ii = i_ids[b, :n[b]]
        assert torch.equal(ii, ii.sort().values) and ii.unique().numel() == ii.numel()          # ascending image-0 cell index
        got[ii] = j_ids[b, :n[b]]
        print(f"[eloftr] coarse matching [{split} {hw}] pair {b}: {int(n[b])} matches, oracle {int((want[b] >= 0).sum())}, safe cells {int(safe[b].sum())} of {hc * wc}")
        assert int((want[b] >= 0).sum()) > 20 and torch.equal(got[safe[b]], want[b][safe[b]])
        for ids, name in ((ii, "image 0"), (j_ids[b, :n[b]], "image 1")):
            y, x = ids // wc, ids % wc
            assert bool(((y >= 2) & (y < hc - 2) & (x >= 2) & (x < wc - 2)).all()), name


def test_fine_matching_on_constructed_windows(hip):
    """known displacements plus forced winners on row / column 0 (the wrap-around read of the second stage) and 7: arg-max equal on safe matches,
    coordinates within max(10 x the float32 oracle's error, 1e-3 px)"""
    m32, m64 = R.modules("perturbed")
    w0, w1, ci, cj = R.constructed_windows()
    M, wc = w0.shape[0], 16
    arg64, safe = R.fine_stage1(w0, w1)
    p32, p64 = R.fine_match(m32, w0.float(), w1.float(), ci, cj, wc), R.fine_match(m64, w0, w1, ci, cj, wc)
    n = torch.tensor([M], dtype=torch.int32, device=DEV)
    i32 = lambda t: t.to(torch.int32).reshape(1, M).contiguous().to(DEV)
    with torch.no_grad():
        g0, g1, arg = hip("f16x2").fine_match(w0.float().contiguous().to(DEV), w1.float().contiguous().to(DEV), i32(ci), i32(cj), n, M, wc, return_arg=True)
    arg = arg.cpu().long()[0]
    assert float((~safe).float().mean()) <= 0.02 and torch.equal(arg[safe], arg64[safe])
    for name, got, a, b in (("pts0", g0, p32[0], p64[0]), ("pts1", g1, p32[1], p64[1])):
        eg, eo = float((got.cpu()[0].double() - b)[safe].abs().max()), float((a.double() - b)[safe].abs().max())
        print(f"[eloftr] fine matching {name}: device {eg:.3e} px | f32 oracle {eo:.3e} px")
        assert eg <= max(R.FACTOR * eo, R.COORD_FLOOR)


def _by_cell(out, p, wc):
    """device output of pair p -> (cells i ascending per slot, rows [n, 4])"""
    n = int(out["n_corr"][p])
    pts = torch.cat([out["pts0"][p, :n], out["pts1"][p, :n]], 1).cpu()
    cell = torch.round(pts[:, :2] / 8.0).long()                                                # pts0 = 8 cell + [-3.5, 3.5]
    return cell[:, 1] * wc + cell[:, 0], pts


@pytest.fixture(scope="module")
def e2e_oracle():
    m32, m64 = R.modules("perturbed")
    im = R.end_to_end_images()
    o64 = R.end_to_end(m64, im.double())
    return dict(im=im, o32=R.end_to_end(m32, im), o64=o64, safe=R.coarse_safe(o64["conf"]))


def _check_pairs(tag, out, o32, o64, safe, wc, frame=None):
    for p in range(len(o64["pairs"])):
        a, b = o32["pairs"][p], o64["pairs"][p]
        inside = lambda q: torch.ones(q["i"].numel(), dtype=torch.bool) if frame is None else \
            (q["pts0"][:, 0] < frame[1]) & (q["pts0"][:, 1] < frame[0]) & (q["pts1"][:, 0] < frame[1]) & (q["pts1"][:, 1] < frame[0])
        ka, kb = inside(a), inside(b)
        cells, pts = _by_cell(out, p, wc)
        assert cells.numel() > 0 and torch.equal(cells, cells.sort().values) and cells.unique().numel() == cells.numel()
        L = safe.shape[1]
        got, want = torch.zeros(L, dtype=torch.bool), torch.zeros(L, dtype=torch.bool)
        got[cells] = True; want[a["i"][ka]] = True
        # the match set is the float32 module's on safe cells (a cell whose refined point sits within 1e-3 px of the frame's edge may fall either way)
        edge = torch.zeros(L, dtype=torch.bool)
        if frame is not None:
            near = lambda q: ((q["pts0"] - torch.tensor([frame[1], frame[0]])).abs().min(1).values < 1e-3) | ((q["pts1"] - torch.tensor([frame[1], frame[0]])).abs().min(1).values < 1e-3)
            edge[b["i"][near(b)]] = True
        ok = safe[p] & ~edge
        assert torch.equal(got[ok], want[ok]), (tag, p)
        common = torch.isin(cells, b["i"][kb]) & ok[cells]
        pos = torch.searchsorted(b["i"], cells[common])
        ref = torch.cat([b["pts0"], b["pts1"]], 1)[pos]
        eg = float((pts[common].double() - ref).abs().max())
        both = torch.isin(a["i"], cells[common]) & torch.isin(a["i"], b["i"])
        eo = float((torch.cat([a["pts0"], a["pts1"]], 1)[both].double() - torch.cat([b["pts0"], b["pts1"]], 1)[torch.searchsorted(b["i"], a["i"][both])]).abs().max())
        print(f"[eloftr] {tag} pair {p}: {cells.numel()} matches (oracle {int(ka.sum())}), coordinates device {eg:.3e} px | f32 oracle {eo:.3e} px")
        assert eg <= max(R.FACTOR * eo, R.COORD_FLOOR), (tag, p)
        if frame is not None:
            assert bool((pts[:, 0::2] < frame[1]).all() and (pts[:, 1::2] < frame[0]).all())


def _digest(out):
    """SHA-256 (first 16 hex digits) of the stage outputs that decide the end-to-end test, in pipeline order: two suite logs, one of a failing and one
    of a passing run, then show at which stage the runs part, without running anything again.  Only what the header specifies is hashed: of the
    coarse matcher's index rows the first n_coarse[p] entries of every pair, pts0 / pts1 whole (zero-filled behind n_corr)."""
    import hashlib
    h = lambda t: hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]
    n = out["n_coarse"].cpu()
    head = lambda t: torch.cat([t[p, :int(n[p])] for p in range(n.numel())])
    return " ".join(f"{k}={v}" for k, v in (("n_coarse", h(out["n_coarse"])), ("i_ids", h(head(out["i_ids"]))), ("j_ids", h(head(out["j_ids"]))),
                                            ("pts0", h(out["pts0"])), ("pts1", h(out["pts1"]))))


@pytest.mark.parametrize("split", SPLITS)
def test_end_to_end_vs_module(e2e_oracle, hip, split):
    """two pairs at 160 x 128: the match set, the coordinates, n_corr > 0 on both, ascending order, the maxN cap"""
    o = e2e_oracle
    with options.override(SPLIT=split):
        net = hip(split)
        out = net(o["im"].to(DEV))
        capped = net(o["im"].to(DEV), maxN=20)
    print(f"[eloftr] digest [{split}] " + _digest(out))
    assert bool((out["n_corr"] > 0).all())
    _check_pairs(f"end to end [{split}]", out, o["o32"], o["o64"], o["safe"], 16)
    assert capped["pts0"].shape[1] == 20 and bool((capped["n_corr"] == torch.clamp(out["n_corr"], max=20)).all())
    for p in range(2):
        n = int(capped["n_corr"][p])
        assert torch.equal(capped["pts0"][p, :n], out["pts0"][p, :n]) and torch.equal(capped["pts1"][p, :n], out["pts1"][p, :n])
        assert float(capped["pts0"][p, n:].abs().max() if n < 20 else 0.0) == 0


def test_padded_frame_drops_only_what_lies_outside(hip):
    """138 x 100 -> padded to 160 x 128 by the stage (22 / 28 pixels: more than the 2-cell border, so the oracle, run on the padded images, has matches
    beyond the frame: 10 of 62 and 6 of 42).  Every match it has inside the unpadded frame is there, and nothing lies at x >= 100 or y >= 138"""
    m32, m64 = R.modules("perturbed")
    H, W = 138, 100
    im = R.end_to_end_images((H, W))
    padded = torch.nn.functional.pad(im, (0, 128 - W, 0, 160 - H))
    o32, o64 = R.end_to_end(m32, padded), R.end_to_end(m64, padded.double())
    outside = [int(((p["pts0"][:, 0] >= W) | (p["pts0"][:, 1] >= H) | (p["pts1"][:, 0] >= W) | (p["pts1"][:, 1] >= H)).sum()) for p in o64["pairs"]]
    assert min(outside) > 0, outside
    out = hip("f16x2")(im.to(DEV))
    _check_pairs("padded frame", out, o32, o64, R.coarse_safe(o64["conf"]), 16, frame=(H, W))


def _plugin_cfg(tmp_path, sd, **hip_opts):
    from mapfree_reloc_amd.config.default import cfg
    c = cfg.clone()
    path = tmp_path / "eloftr.pth"
    torch.save(sd, path)
    c.ELOFTR.WEIGHTS = str(path)
    c.FEATURE_MATCHING = "EfficientLoFTR"
    for k, v in hip_opts.items():
        c.HIP[k] = v
    return c


def test_plugin_equals_the_stage_and_out_of_range_yields_the_bf16x3_result(tmp_path, hip):
    """per-pair plugin == the stage; with the stem scaled by 3e5 the next layer's inputs leave the f16x2 range: the guard fires and the plugin hands out
    what the exact (bf16x3) stage computes -- the oracle's matches"""
    from mapfree_reloc_amd.matching.model import FEATURE_MATCHERS
    options.reset()
    im = R.end_to_end_images()[:2]
    data = dict(image0=im[0:1], image1=im[1:2])
    plug = FEATURE_MATCHERS["EfficientLoFTR"](_plugin_cfg(tmp_path, R.weights("perturbed")))
    p0, p1 = plug.get_correspondences(data)
    out = hip("f16x2")(im.to(DEV))
    n = int(out["n_corr"][0])
    assert plug.guard.reruns == 0 and n == len(p0) and np.array_equal(p0, out["pts0"][0, :n].cpu().numpy()) and np.array_equal(p1, out["pts1"][0, :n].cpu().numpy())
    sd = dict(R.weights("perturbed"))
    for br in ("conv1", "conv2"):
        for t in ("weight", "bias"):
            k = f"efficientloftr.backbone.stages.0.blocks.0.{br}.norm.{t}"
            sd[k] = sd[k] * 3.0e5
    plug = FEATURE_MATCHERS["EfficientLoFTR"](_plugin_cfg(tmp_path, sd))
    p0, p1 = plug.get_correspondences(data)
    assert plug.guard.reruns == 1 and np.isfinite(p0).all() and np.isfinite(p1).all()
    with options.override(SPLIT="bf16x3"):
        exact = EL.EfficientLoFTRHIP(sd, DEV)(im.to(DEV))
    n = int(exact["n_corr"][0])
    assert n == len(p0) and np.array_equal(p0, exact["pts0"][0, :n].cpu().numpy()) and np.array_equal(p1, exact["pts1"][0, :n].cpu().numpy())
    o64 = R.end_to_end(R.module(sd, torch.float64), im.double())
    want, safe = o64["pairs"][0], R.coarse_safe(o64["conf"])[0]
    cell = np.round(p0 / 8.0).astype(np.int64)
    got = torch.zeros(safe.numel(), dtype=torch.bool); got[torch.from_numpy(cell[:, 1] * 16 + cell[:, 0])] = True
    ref = torch.zeros(safe.numel(), dtype=torch.bool); ref[want["i"]] = True
    assert want["i"].numel() > 20 and torch.equal(got[safe], ref[safe])
