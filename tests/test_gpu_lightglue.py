"""-m gpu: LightGlue on the device (nets/lightglue.py, csrc/lightglue.hip) against the `transformers` LightGlue module (tests/lightglue_ref.py), on
weights whose biases and LayerNorm terms are non-trivial, in both HIP.SPLIT arithmetics.

Continuous stages: the bar of tests/test_gpu_matcher_wiring.py -- every stage is fed the float32 oracle's tensors and compared with the float64
oracle on those same tensors; err(device) <= 10 x err(float32 oracle), max and rms, both printed before the assert.  Padded keypoints are not
compared: the device's attention writes a zero message for a query beyond its image's count, the module lets it attend to the valid keys (neither
ever reaches a valid keypoint).

Discrete outputs: equal on every SAFE keypoint (tests/lightglue_ref.safe_masks: float64 best and second-best log-score at least 1e-3 apart along
its row / column, score at least 1e-3 from the threshold); at most 2 % of the keypoints may be unsafe (on the network inputs the oracle alone has
none: tests/test_lightglue_host.py).  Scores: rtol 2e-4 / atol 2e-5, the bar of the SuperGlue score test."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lightglue_ref as LG  # noqa: E402

from mapfree_reloc_amd import options  # noqa: E402
from mapfree_reloc_amd.nets import weights as WT  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = 10.0
SPLITS = ["f16x2", "bf16x3"]
B2, N = 2 * LG.B, LG.N


def _err(t, ref64):
    d = t.detach().double().cpu() - ref64
    return float(d.abs().max() / ref64.abs().max()), float(d.pow(2).mean().sqrt() / ref64.pow(2).mean().sqrt())


def _check(stage, got, f32, f64):
    assert got.shape == f64.shape, (stage, got.shape, f64.shape)
    eg, eo = _err(got, f64), _err(f32, f64)
    print(f"[lightglue] {stage}: device max {eg[0]:.3e} rms {eg[1]:.3e} | f32 oracle max {eo[0]:.3e} rms {eo[1]:.3e} | ratio max {eg[0] / eo[0]:.2f} rms {eg[1] / eo[1]:.2f}")
    assert np.isfinite(eg[0]) and eo[0] > 0
    assert eg[0] <= FACTOR * eo[0] and eg[1] <= FACTOR * eo[1], (stage, eg, eo)


class _Oracle:
    def __init__(self):
        self.sd = LG.perturbed(WT.lightglue_state_dict())
        self.m32, self.m64 = LG.make_models(self.sd)
        self.kpts, self.desc, self.mask, self.counts = LG.make_inputs(0)
        self.mt32, self.sc32, self.hs32 = LG.run(self.m32, self.kpts, self.desc, self.mask)
        self.mt64, self.sc64, self.hs64 = LG.run(self.m64, self.kpts, self.desc, self.mask)
        self.cs32, self.cs64 = LG.rotary(self.m32, self.kpts), LG.rotary(self.m64, self.kpts)
        self.valid = self.mask.reshape(B2, N).bool()
        self.n0, self.n1 = self.counts[:, 0].contiguous(), self.counts[:, 1].contiguous()
        self.block = (torch.arange(N)[None, :, None] < self.n0[:, None, None]) & (torch.arange(N)[None, None, :] < self.n1[:, None, None])

    def sp_out(self):
        d = lambda t: t.reshape(B2, N, -1).to(DEV).contiguous()
        return dict(kpts=d(self.kpts), desc=d(self.desc), scores=torch.ones(B2, N, device=DEV), n=self.counts.reshape(-1).to(DEV).contiguous())


@pytest.fixture(scope="module")
def oracle():
    return _Oracle()


# (arithmetic, how the MLP's LayerNorm + GELU run): both arithmetics, with the stand-alone pass (the default) and with fc1's epilogue kernel
ROUTES = [("f16x2", "pass"), ("bf16x3", "pass"), ("f16x2", "epilogue"), ("bf16x3", "epilogue")]


@pytest.fixture(scope="module", params=ROUTES, ids=lambda r: f"{r[0]}-{r[1]}")
def hip(request, oracle):
    from mapfree_reloc_amd.nets.lightglue import MLP_DEFAULT, LightGlueHIP
    split, mlp = request.param
    assert MLP_DEFAULT in ("epilogue", "pass")
    options.reset()
    with options.override(SPLIT=split):
        net = LightGlueHIP(oracle.sd, DEV, filter_threshold=LG.THRESHOLD, mlp=mlp)
    assert net.lin_final.split == split and net.att_variant == (0 if split == "f16x2" else 2) and net.mlp == mlp
    return f"{split} {mlp}", net


def _buffers(x32):
    xa = torch.zeros(B2 * N, 512, device=DEV)
    xa[:, :256] = x32.reshape(B2 * N, 256).to(DEV)
    return xa, torch.empty(B2 * N, 768, device=DEV), torch.empty(B2 * N, 512, device=DEV)


# ------------------------------------------------------------------------------------------------ continuous stages
def test_rotary_q_k_vs_float64(oracle, hip):
    """layer 1's self-attention q and k after the rotary encoding (all rows: the projection and the rotation are per keypoint)"""
    route, net = hip
    o = oracle
    x32 = o.hs32[7]
    q32, k32 = LG.rotated_qk(o.m32, 1, x32, o.cs32)
    q64, k64 = LG.rotated_qk(o.m64, 1, x32.double(), o.cs64)
    sp = o.sp_out()
    cs = net.rotary_table(net.normalize_keypoints(sp["kpts"], (LG.H, LG.W)))
    c64 = torch.cat([o.cs64[0][..., 0::2], o.cs64[1][..., 0::2]], -1).reshape(B2 * N, 64)
    c32 = torch.cat([o.cs32[0][..., 0::2], o.cs32[1][..., 0::2]], -1).reshape(B2 * N, 64)
    _check(f"{route} cos | sin table", cs, c32, c64)
    xa, qkv, _ = _buffers(x32)
    net.blocks[2]["lin_qkv"](xa[:, :256], out=qkv)
    net.rotate(qkv, cs)
    _check(f"{route} q after rotary", qkv[:, :256].reshape(B2, N, 256), q32, q64)
    _check(f"{route} k after rotary", qkv[:, 256:512].reshape(B2, N, 256), k32, k64)


@pytest.mark.parametrize("kind", ["self", "cross"])
def test_one_block_vs_float64(oracle, hip, kind):
    route, net = hip
    o = oracle
    if kind == "self":
        x32, L = o.hs32[7], net.blocks[2]
        f32, f64 = LG.self_block(o.m32, 1, x32, o.cs32, o.mask), LG.self_block(o.m64, 1, x32.double(), o.cs64, o.mask)
    else:
        x32, L = o.hs32[8], net.blocks[3]
        f32, f64 = LG.cross_block(o.m32, 1, x32, o.mask), LG.cross_block(o.m64, 1, x32.double(), o.mask)
    assert L["cross"] == (kind == "cross")
    sp = o.sp_out()
    cs = net.rotary_table(net.normalize_keypoints(sp["kpts"], (LG.H, LG.W)))
    xa, qkv, hid = _buffers(x32)
    net.block(L, xa, qkv, hid, cs, sp["n"], B2, N)
    got = xa[:, :256].reshape(B2, N, 256).cpu()
    _check(f"{route} {kind} block", got[o.valid], f32[o.valid], f64[o.valid])


@pytest.mark.parametrize("split", SPLITS)
def test_fc1_layernorm_gelu_epilogue_vs_float64(oracle, split):
    """GELU(LayerNorm_512(fc1([x | message]))) of layer 1's self MLP in ONE launch (mfr_gemm_*_ln_gelu) on the module's own fc1 weights: 320 rows =
    two full row tiles and a half one.  The stand-alone pass behind a plain fc1 is held to the same bar"""
    from mapfree_reloc_amd import _lib
    from mapfree_reloc_amd.nets.linear import SplitLinear
    o = oracle
    cat32 = o.hs32[7 + 2].reshape(B2 * N, 512)
    ref = lambda m, x: m.activation_fn(m.layer_norm(m.fc1(x)))
    with torch.no_grad():
        f32, f64 = ref(o.m32.transformer_layers[1].self_mlp, cat32), ref(o.m64.transformer_layers[1].self_mlp, cat32.double())
    mlp = o.m32.transformer_layers[1].self_mlp
    options.reset()
    with options.override(SPLIT=split):
        lin = SplitLinear(mlp.fc1.weight.detach().to(DEV), mlp.fc1.bias.detach().to(DEV))
    ln = (mlp.layer_norm.weight.detach().to(DEV).contiguous(), mlp.layer_norm.bias.detach().to(DEV).contiguous())
    x = cat32.to(DEV).contiguous()
    got = lin.ln_gelu(x, ln, torch.full((B2 * N, 512), float("nan"), device=DEV))
    _check(f"{split} fc1 + LayerNorm + GELU epilogue", got, f32, f64)
    two = lin(x)
    _lib.check(_lib.load().mfr_lg_ln_gelu(two.data_ptr(), 512, B2 * N, _lib.ptr(ln[0]), _lib.ptr(ln[1]), 1e-5, _lib.stream_ptr()), "mfr_lg_ln_gelu")
    _check(f"{split} fc1, then LayerNorm + GELU pass", two, f32, f64)
    # a row stride wider than 512 on both sides, and rows beyond M untouched
    wide_in = torch.zeros(200, 520, device=DEV); wide_in[:, :512] = x[:200]
    wide_out = torch.full((201, 516), -7.0, device=DEV)
    lin.ln_gelu(wide_in[:, :512], ln, wide_out[:200, :512])
    assert torch.equal(wide_out[:200, :512], got[:200]) and bool((wide_out[200] == -7.0).all() and (wide_out[:, 512:] == -7.0).all())


def test_fc1_epilogue_kernel_flags_out_of_range_input(oracle):
    from mapfree_reloc_amd.nets.linear import SplitLinear
    from mapfree_reloc_amd.pipeline import RangeGuard
    options.reset()
    mlp = oracle.m32.transformer_layers[1].self_mlp
    lin = SplitLinear(mlp.fc1.weight.detach().to(DEV), mlp.fc1.bias.detach().to(DEV))
    ln = (mlp.layer_norm.weight.detach().to(DEV).contiguous(), mlp.layer_norm.bias.detach().to(DEV).contiguous())
    x = oracle.hs32[9].reshape(B2 * N, 512).to(DEV).contiguous()
    guard = RangeGuard(torch.device(DEV), lambda: None)
    out = torch.empty(B2 * N, 512, device=DEV)
    with guard:
        lin.ln_gelu(x, ln, out)
    assert int(guard.flag.item()) == 0 and bool(torch.isfinite(out).all())
    for (r, c) in ((0, 0), (B2 * N - 1, 511), (150, 300)):
        xb = x.clone(); xb[r, c] = 1.0e5
        with guard:
            lin.ln_gelu(xb, ln, out)
        assert int(guard.flag.item()) != 0, (r, c)


def test_all_layers_vs_float64(oracle, hip):
    route, net = hip
    o = oracle
    sp = o.sp_out()
    got = net.final_descriptors(sp["kpts"], sp["desc"], sp["n"], (LG.H, LG.W)).cpu()
    _check(f"{route} descriptors after 9 layers", got[o.valid], o.hs32[60][o.valid], o.hs64[60][o.valid])


def test_similarity_and_matchability_vs_float64(oracle, hip):
    route, net = hip
    o = oracle
    x32 = o.hs32[60]
    S32, a32, b32 = LG.similarity(o.m32, x32)
    S64, a64, b64 = LG.similarity(o.m64, x32.double())
    S, z0, z1 = net.similarity(x32.to(DEV))
    _check(f"{route} S", S.cpu()[o.block], S32[o.block], S64[o.block])
    v0, v1 = o.mask[:, 0].bool(), o.mask[:, 1].bool()
    _check(f"{route} matchability 0", z0.cpu()[v0], a32[v0], a64[v0])
    _check(f"{route} matchability 1", z1.cpu()[v1], b32[v1], b64[v1])


# ------------------------------------------------------------------------------------------------ assignment
@pytest.fixture(scope="module")
def assigner():
    """the assignment kernel is fp32 whatever HIP.SPLIT is: its tests run once"""
    from mapfree_reloc_amd.nets.lightglue import Assignment
    return Assignment(LG.THRESHOLD)


def _assign_check(tag, assign, S, z0, z1, n0, n1, max_unsafe=0.02, kpts=None):
    """mfr_lg_assign on (S, z0, z1) vs the float64 module functions; S may be a column-strided view (ldS > N1)"""
    b, N0, N1 = S.shape
    out = assign(S.to(DEV) if not S.is_cuda else S, z0.to(DEV), z1.to(DEV), n0.to(DEV), n1.to(DEV),
                     None if kpts is None else kpts[0].to(DEV), None if kpts is None else kpts[1].to(DEV))
    torch.cuda.synchronize()
    w0, w1, s0, s1, logp = LG.assign64(S.cpu(), z0, z1, n0, n1)
    safe0, safe1 = LG.safe_masks(logp, n0, n1)
    n_valid = int(n0.sum() + n1.sum())
    n_pairs_alive = ((n0 > 0) & (n1 > 0))
    n_cmp = int((n0 * n_pairs_alive).sum() + (n1 * n_pairs_alive).sum())
    unsafe = n_cmp - int(safe0.sum() + safe1.sum())
    print(f"[lightglue] {tag}: {n_valid} keypoints, {unsafe} unsafe, {int((w0 >= 0).sum())} matches")
    assert unsafe <= max_unsafe * max(n_cmp, 1), (tag, unsafe, n_cmp)
    m0, m1, g0, g1 = out["matches0"].cpu(), out["matches1"].cpu(), out["matching_scores0"].cpu(), out["matching_scores1"].cpu()
    assert m0.dtype == torch.int32 and m0.shape == (b, N0) and m1.shape == (b, N1)
    assert torch.equal(m0[safe0].long(), w0[safe0]) and torch.equal(m1[safe1].long(), w1[safe1]), tag
    np.testing.assert_allclose(g0[safe0].numpy(), s0[safe0].numpy(), rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(g1[safe1].numpy(), s1[safe1].numpy(), rtol=2e-4, atol=2e-5)
    # beyond the counts, and in a pair with an empty side: no match, score 0
    pad0 = ~((torch.arange(N0)[None] < n0[:, None]) & n_pairs_alive[:, None])
    pad1 = ~((torch.arange(N1)[None] < n1[:, None]) & n_pairs_alive[:, None])
    assert bool((m0[pad0] == -1).all() and (m1[pad1] == -1).all() and (g0[pad0] == 0).all() and (g1[pad1] == 0).all()), tag
    # the two sides are one set of pairs
    for p in range(b):
        i = torch.nonzero(m0[p] >= 0).flatten()
        assert torch.equal(m1[p][m0[p][i].long()].long(), i), tag
        assert int((m1[p] >= 0).sum()) == i.numel()
    return out, w0


def test_assignment_on_the_oracle_similarity(oracle, assigner):
    o = oracle
    S32, z0, z1 = LG.similarity(o.m32, o.hs32[60])
    kp = o.kpts[:, 0].contiguous(), o.kpts[:, 1].contiguous()
    out, w0 = _assign_check("assignment", assigner, S32, z0, z1, o.n0, o.n1, kpts=kp)
    for p in range(LG.B):                                                # the matched keypoints in ascending i, and their count
        i = torch.nonzero(w0[p] >= 0).flatten()
        assert int(out["n_corr"][p]) == i.numel() >= LG.TWINS
        assert torch.equal(out["pts0"][p, :i.numel()].cpu(), kp[0][p][i]) and torch.equal(out["pts1"][p, :i.numel()].cpu(), kp[1][p][w0[p][i]])


def _random_problem(b, n, seed, plant):
    g = torch.Generator().manual_seed(seed)
    S = 3.0 * torch.randn(b, n, n, generator=g)
    idx = torch.arange(plant)
    S[:, idx, (7 * idx + 3) % n] += 14.0                                 # planted assignments (7 is coprime to the sizes used), so that matches exist
    return S, 2.0 * torch.randn(b, n, generator=g) + 3.0, 2.0 * torch.randn(b, n, generator=g) + 3.0


def test_assignment_edge_cases(assigner):
    """an empty side (n1 = 0), a single row (n0 = 1), counts below the padded size, and a row stride that is no multiple of 4 (ldS = 39)"""
    n = 37
    S, z0, z1 = _random_problem(4, n, 11, 30)
    wide = torch.full((4, n, n + 2), float("nan"), device=DEV)            # the padding columns are never read: NaN there must not show
    wide[:, :, :n] = S.to(DEV)
    n0 = torch.tensor([37, 1, 37, 20], dtype=torch.int32)
    n1 = torch.tensor([0, 37, 30, 37], dtype=torch.int32)
    view = wide[:, :, :n]
    assert view.stride(1) == 39
    out, w0 = _assign_check("edge cases", assigner, view, z0, z1, n0, n1, max_unsafe=0.02)
    assert int((out["matches0"][0] >= 0).sum()) == 0 and int((out["matches1"][0] >= 0).sum()) == 0
    assert int((w0[2] >= 0).sum()) > 10                                  # a pair that really matches was compared
    # ties go to the lowest index: a constant S, equal logits -> keypoint 0 pairs with keypoint 0 (score sigmoid(9)^2 / 64), nothing else is mutual
    from mapfree_reloc_amd.nets.lightglue import Assignment
    flat = Assignment(0.001)(torch.zeros(1, 8, 8, device=DEV), torch.full((1, 8), 9.0, device=DEV), torch.full((1, 8), 9.0, device=DEV),
                      torch.tensor([8], dtype=torch.int32, device=DEV), torch.tensor([8], dtype=torch.int32, device=DEV))
    assert flat["matches0"][0].tolist() == [0] + [-1] * 7 and flat["matches1"][0].tolist() == [0] + [-1] * 7


def test_assignment_full_size(assigner):
    """N = 1024 with counts 1024 / 1000: 32 strips of rows, one full chunk of columns, on random S against float64"""
    S, z0, z1 = _random_problem(1, 1024, 5, 700)
    _assign_check("assignment 1024 x 1000", assigner, S, z0, z1, torch.tensor([1024], dtype=torch.int32), torch.tensor([1000], dtype=torch.int32))


def test_assignment_more_columns_than_one_chunk(assigner):
    """N = 1100 with counts 1100 / 1050: the columns span two chunks of 1024, so the row state is carried from chunk to chunk and the second chunk's
    column partials land behind the first's"""
    S, z0, z1 = _random_problem(1, 1100, 9, 800)
    out, w0 = _assign_check("assignment 1100 x 1050", assigner, S, z0, z1, torch.tensor([1100], dtype=torch.int32), torch.tensor([1050], dtype=torch.int32))
    assert int((w0[0] >= 1024).sum()) > 0 or int(((w0[0] >= 0) & (torch.arange(1100) >= 1024)).sum()) > 0


# ------------------------------------------------------------------------------------------------ end to end
def _safe_from_oracle(m64, hs64, n0, n1):
    S, z0, z1 = LG.similarity(m64, hs64[60])
    w0, w1, s0, s1, logp = LG.assign64(S, z0, z1, n0, n1)
    return w0, w1, LG.safe_masks(logp, n0, n1)


def test_end_to_end_matches_equal_float64(oracle, hip):
    route, net = hip
    o = oracle
    out = net(o.sp_out(), (LG.H, LG.W))
    w0, w1, (safe0, safe1) = _safe_from_oracle(o.m64, o.hs64, o.n0, o.n1)
    for p in range(LG.B):
        assert torch.equal(w0[p, :o.n0[p]], o.mt64[2 * p, :o.n0[p]])
    assert int((~safe0).sum()) - int((N - o.n0).sum()) == 0              # (asserted on the oracle alone in tests/test_lightglue_host.py)
    m0, m1 = out["matches0"].cpu().long(), out["matches1"].cpu().long()
    assert torch.equal(m0[safe0], w0[safe0]) and torch.equal(m1[safe1], w1[safe1])
    assert out["n_corr"].cpu().tolist() == [int((w0[p] >= 0).sum()) for p in range(LG.B)]
    assert all(int(c) >= LG.TWINS for c in out["n_corr"])
    assert out["pts0"].shape == (LG.B, N, 2) and {"matching_scores0", "matching_scores1", "pts1"} <= set(out)


# ------------------------------------------------------------------------------------------------ range guard
def test_out_of_range_activations_set_the_guard_and_the_bf16x3_rerun_is_the_oracle(oracle):
    """the last final_projection x 1e5: the match descriptors (~1e6) leave the f16x2 range, so the similarity product's accumulators overflow.  The f16x2
    network must raise the bound flag; the bf16x3 network must return the float64 oracle's matches (pattern: tests/test_gpu_range_guard.py).  The
    scaling keeps the assignment's structure: the oracle alone still matches every planted twin, all keypoints safe (asserted)"""
    from mapfree_reloc_amd.nets.lightglue import LightGlueHIP
    from mapfree_reloc_amd.pipeline import RangeGuard
    o = oracle
    options.reset()
    sd = dict(o.sd)
    key = "match_assignment_layers.8.final_projection.weight"
    sd[key] = sd[key] * 1.0e5
    _, m64 = LG.make_models(sd)
    mt64, _, hs64 = LG.run(m64, o.kpts, o.desc, o.mask)
    assert float((hs64[60] @ sd[key].double().t()).abs().max()) / 4 > 65504
    guard = RangeGuard(torch.device(DEV), lambda: None)
    assert guard.active
    with guard:
        LightGlueHIP(o.sd, DEV)(o.sp_out(), (LG.H, LG.W))
    assert int(guard.flag.item()) == 0                                   # the in-range network leaves the flag alone
    with guard:
        LightGlueHIP(sd, DEV)(o.sp_out(), (LG.H, LG.W))
    assert int(guard.flag.item()) != 0
    with options.override(SPLIT="bf16x3"):
        exact = LightGlueHIP(sd, DEV)
        out = exact(o.sp_out(), (LG.H, LG.W))
    w0, w1, (safe0, safe1) = _safe_from_oracle(m64, hs64, o.n0, o.n1)
    unsafe = int(o.n0.sum() + o.n1.sum()) - int(safe0.sum() + safe1.sum())
    print(f"[lightglue] range guard: {unsafe} unsafe keypoints, {int((w0 >= 0).sum())} matches")
    assert unsafe <= 0.02 * int(o.n0.sum() + o.n1.sum()) and int((w0 >= 0).sum()) >= 2 * LG.TWINS
    assert torch.equal(out["matches0"].cpu().long()[safe0], w0[safe0]) and torch.equal(out["matches1"].cpu().long()[safe1], w1[safe1])
    assert bool(torch.isfinite(out["matching_scores0"]).all())


# ------------------------------------------------------------------------------------------------ routes
RH, RW = 240, 176


def _write_tree(root):
    """two scenes of one pair each (images.synthetic_pair at 240 x 176, stored losslessly as 8-bit gray); -> per scene (scene dir, pair dict)"""
    from PIL import Image
    from mapfree_reloc_amd import images as IM
    out = []
    for s, seed in enumerate((21, 22)):
        sc = root / "val" / f"s{s:05d}"
        (sc / "seq0").mkdir(parents=True); (sc / "seq1").mkdir()
        p = IM.synthetic_pair(seed, RH, RW)
        for rel, im in (("seq0/frame_00000.jpg", p["img0"]), ("seq1/frame_00000.jpg", p["img1"])):
            Image.fromarray(np.round(im * 255).astype(np.uint8)).save(sc / rel, format="PNG")
        (sc / "poses.txt").write_text("# frame q t\nseq0/frame_00000.jpg 1 0 0 0 0 0 0\nseq1/frame_00000.jpg 1 0 0 0 0 0 0\n")
        out.append((sc, p))
    return out


def _cfg(matcher, cache=True):
    from mapfree_reloc_amd.config import get_cfg_defaults
    cfg = get_cfg_defaults()
    cfg.MODEL, cfg.FEATURE_MATCHING, cfg.POSE_SOLVER = "FeatureMatching", matcher, "PNP"
    cfg.MATCHES_FILE_PATH = "{scene_root}/correspondences_LG.npz"
    cfg.PNP.RANSAC_ITER, cfg.PNP.REPROJECTION_INLIER_THRESHOLD, cfg.PNP.CONFIDENCE = 1000, 3, 0.9999
    cfg.ALLOW_SYNTHETIC_WEIGHTS = True
    cfg.HIP.REF_FEATURE_CACHE = cache
    return cfg


def test_routes_give_the_same_correspondences_and_pose(tmp_path):
    """per-pair plugin, fused pipeline with the reference-view cache on and off, offline `compute -m LG` + Precomputed: the same correspondences and
    the same pose, bit for bit, on two synthetic pairs"""
    from mapfree_reloc_amd import compute, matchers, wire
    from mapfree_reloc_amd.builder import build_model
    from mapfree_reloc_amd.pipeline import FusedPosePipeline
    options.reset()
    scenes = _write_tree(tmp_path)
    compute.main(["-ds", "Mapfree", "-m", "LG", "--data_root", str(tmp_path), "--resize", str(RW), str(RH)])
    plugin, offline = build_model(_cfg("LightGlue")), build_model(_cfg("Precomputed"))
    datas, planes = [], []
    for sc, p in scenes:
        g = [matchers.read_image(str(sc / rel), (RW, RH)) for rel in ("seq0/frame_00000.jpg", "seq1/frame_00000.jpg")]
        assert g[0].shape == (RH, RW) and g[0].dtype == np.float32
        planes += g
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
        datas.append({"image0": t(g[0])[None, None], "image1": t(g[1])[None, None], "depth0": t(p["depth0"])[None], "depth1": t(p["depth1"])[None],
                      "K_color0": t(p["K"])[None], "K_color1": t(p["K"])[None], "pair_id": torch.tensor([0]), "scene_id": [sc.name],
                      "scene_root": [str(sc)], "pair_names": [["seq0/frame_00000.jpg"], ["seq1/frame_00000.jpg"]]})
    batch = dict(images=torch.from_numpy(np.stack(planes))[:, None].to(DEV), depth0=torch.stack([d["depth0"][0] for d in datas]).to(DEV),
                 depth1=torch.stack([d["depth1"][0] for d in datas]).to(DEV), K0=torch.stack([d["K_color0"][0] for d in datas]).to(DEV),
                 K1=torch.stack([d["K_color1"][0] for d in datas]).to(DEV), seed_ids=torch.zeros(2, dtype=torch.int64, device=DEV),
                 ref_keys=[(str(sc), "seq0/frame_00000.jpg") for sc, _ in scenes])
    fused = {}
    for cache in (True, False):
        pipe = FusedPosePipeline(_cfg("LightGlue", cache))
        m = pipe.match(batch)
        fused[cache] = (m, pipe(batch))
        if cache:
            assert pipe.match.stats == {"reference_views_run": 2, "reference_views_reused": 2}      # the second pass reads both reference views from the cache
    for i, ((sc, p), data) in enumerate(zip(scenes, datas)):
        a0, a1 = plugin.feature_matching.get_correspondences(data)
        assert len(a0) > 0
        corr = np.load(sc / "correspondences_LG.npz")["correspondences"]
        o0, o1 = wire.strip_nan(corr[0].astype(np.float32))
        assert np.array_equal(a0, o0) and np.array_equal(a1, o1)
        Rp, tp = plugin(dict(data))
        Ro, to = offline(dict(data))
        assert not torch.isnan(Rp).any() and torch.equal(Rp, Ro) and torch.equal(tp, to)
        for cache in (True, False):
            m, out = fused[cache]
            n = int(m["n_corr"][i])
            assert n == len(a0) > 0
            assert np.array_equal(m["pts0"][i, :n].cpu().numpy(), a0) and np.array_equal(m["pts1"][i, :n].cpu().numpy(), a1)
            assert int(out["status"][i]) == 0
            assert np.array_equal(out["R"][i].cpu().numpy().astype(np.float32), Rp[0].numpy())
            assert np.array_equal(out["t"][i].cpu().numpy().astype(np.float32), tp[0, 0].numpy())


def test_fused_pipeline_reruns_an_out_of_range_batch_in_bf16x3(tmp_path):
    """FusedPosePipeline with FEATURE_MATCHING 'LightGlue' on a checkpoint file whose last final_projection is x 1e5: every pair of the batch comes
    back ST_RANGE with a NaN pose, and rerun_out_of_range hands out what a bf16x3 pipeline computes, bit for bit"""
    from mapfree_reloc_amd import images as IM
    from mapfree_reloc_amd.pipeline import ST_RANGE, FusedPosePipeline, rerun_out_of_range
    options.reset()
    sd = WT.lightglue_state_dict()
    key = "match_assignment_layers.8.final_projection.weight"
    sd[key] = sd[key] * 1.0e5
    torch.save(sd, tmp_path / "lightglue_scaled.pth")
    cfg = _cfg("LightGlue")
    cfg.LIGHTGLUE.WEIGHTS = str(tmp_path / "lightglue_scaled.pth")
    sb = IM.synthetic_batch([21, 22], RH, RW)
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in sb.items() if isinstance(v, np.ndarray)}
    batch = dict(images=d["images"], depth0=d["depth0"], depth1=d["depth1"], K0=d["K0"], K1=d["K1"], seed_ids=d["pair_ids"])
    pipe = FusedPosePipeline(cfg)
    out = pipe(batch)
    assert (out["status"] == ST_RANGE).all() and torch.isnan(out["R"]).all()
    fixed = rerun_out_of_range(pipe, out, batch)
    assert pipe.guard.reruns == 1 and not (fixed["status"] == ST_RANGE).any()
    with options.override(SPLIT="bf16x3"):
        want = FusedPosePipeline(cfg)(batch)
    for k in ("status", "n_corr", "n_inliers"):
        assert torch.equal(fixed[k], want[k]), k
    ok = want["status"] == 0
    assert bool(ok.any()) and torch.equal(fixed["R"][ok], want["R"][ok]) and torch.equal(fixed["t"][ok], want["t"][ok])
    # the in-range network is left alone: no flag, no twin
    pipe2 = FusedPosePipeline(_cfg("LightGlue"))
    o2 = pipe2(batch)
    assert not (o2["status"] == ST_RANGE).any() and rerun_out_of_range(pipe2, o2, batch) is o2 and pipe2.guard._twin is None
