"""-m gpu parity tests of the LoFTR kernels (csrc/loftr.hip) and the LoFTR device module against the
PyTorch-CPU oracle (oracle/loftr_ref.py)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mapfree_reloc_amd import images as IM
from mapfree_reloc_amd.nets import weights as WT
from mapfree_reloc_amd.nets.loftr import LoFTRHIP
from oracle import loftr_ref as LR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def pair():
    sd = WT.loftr_state_dict()
    ref = LR.LoFTRRef().eval(); ref.load_state_dict(sd)
    return ref, LoFTRHIP(sd, DEV)


def test_linear_attention_vs_oracle(pair):
    ref, hip = pair
    g = torch.Generator().manual_seed(0)
    B, L = 3, 6120
    q = torch.randn(B, L, 256, generator=g); k = torch.randn(B, L, 256, generator=g); v = torch.randn(B, L, 256, generator=g)
    want = LR.linear_attention(q.view(B, L, 8, 32), k.view(B, L, 8, 32), v.view(B, L, 8, 32)).reshape(B, L, 256)
    got = hip.linear_attention(q.to(DEV), torch.cat([k, v], -1).to(DEV)).cpu()
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=2e-4, atol=2e-5)


def test_linear_attention_ragged_length(pair):
    ref, hip = pair
    g = torch.Generator().manual_seed(1)
    B, L = 2, 333
    q = torch.randn(B, L, 256, generator=g); k = torch.randn(B, L, 256, generator=g); v = torch.randn(B, L, 256, generator=g)
    want = LR.linear_attention(q.view(B, L, 8, 32), k.view(B, L, 8, 32), v.view(B, L, 8, 32)).reshape(B, L, 256)
    got = hip.linear_attention(q.to(DEV), torch.cat([k, v], -1).to(DEV)).cpu()
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=2e-4, atol=2e-5)


@pytest.mark.parametrize("Bw", [1, 2, 7, 4096])
def test_fine_attention_vs_oracle(pair, Bw):
    """fine transformer LinearAttention: 8 heads x 16, 25 tokens per window, one wavefront per window (odd window
    counts exercise the idle half of the last workgroup)"""
    ref, hip = pair
    g = torch.Generator().manual_seed(Bw)
    L = 25
    q = torch.randn(Bw, L, 128, generator=g); k = torch.randn(Bw, L, 128, generator=g); v = torch.randn(Bw, L, 128, generator=g)
    want = LR.linear_attention(q.double().view(Bw, L, 8, 16), k.double().view(Bw, L, 8, 16), v.double().view(Bw, L, 8, 16)).reshape(Bw, L, 128)
    got = hip.fine_attention(q.to(DEV), torch.cat([k, v], -1).to(DEV)).cpu()
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-4, atol=1e-5)
    legacy = hip._torch_linear_attention(8)(q.to(DEV), torch.cat([k, v], -1).to(DEV)).cpu()      # the einsum path it replaces
    np.testing.assert_allclose(got.numpy(), legacy.numpy(), rtol=1e-4, atol=1e-5)


def test_coarse_match_vs_oracle(pair):
    ref, hip = pair
    g = torch.Generator().manual_seed(2)
    h, w = 30, 22
    L = h * w
    B = 2
    f0 = torch.randn(B, L, 256, generator=g) * 2.2
    perm = torch.stack([torch.randperm(L, generator=g) for _ in range(B)])
    f1 = torch.gather(f0, 1, perm[..., None].expand(-1, -1, 256)) + 0.3 * torch.randn(B, L, 256, generator=g)
    cm = LR.coarse_matching(f0, f1, (h, w), (h, w))
    S = torch.bmm(f0 / 16.0, (f1 / 16.0).transpose(1, 2))
    i_ids, j_ids, mconf, n = [t.cpu() for t in hip.coarse_match(S.to(DEV), (h, w), (h, w))]
    conf = cm["conf_matrix"]
    for b in range(B):
        sel = cm["b_ids"] == b
        wi, wj, wc = cm["i_ids"][sel], cm["j_ids"][sel], cm["mconf"][sel]
        # matches whose confidence is within 1e-3 of the threshold may legitimately differ in fp32
        safe_w = (wc - 0.2).abs() > 1e-3
        gi, gj, gc = i_ids[b, :n[b]].long(), j_ids[b, :n[b]].long(), mconf[b, :n[b]]
        safe_g = (gc - 0.2).abs() > 1e-3
        assert len(wi) > L // 4
        # the near-threshold band is counted, not hidden: thin, and what differs inside it is printed
        n_band = int((~safe_w).sum()) + int((~safe_g).sum())
        pw = {(int(a), int(c)) for a, c in zip(wi.tolist(), wj.tolist())}; pg = {(int(a), int(c)) for a, c in zip(gi.tolist(), gj.tolist())}
        print(f"dual-softmax pair {b}: {len(pw)} oracle / {len(pg)} HIP matches, {n_band} within 1e-3 of the 0.2 threshold, {len(pw ^ pg)} differ in all")
        assert n_band <= max(4, len(wi) // 50) and len(pw ^ pg) <= n_band
        np.testing.assert_array_equal(gi[safe_g].numpy(), wi[safe_w].numpy())
        np.testing.assert_array_equal(gj[safe_g].numpy(), wj[safe_w].numpy())
        np.testing.assert_allclose(gc[safe_g].numpy(), wc[safe_w].numpy(), rtol=2e-4)


def test_coarse_match_pair_without_matches_between_pairs_with_some(pair):
    """the ordered compaction with no survivor (a grid cannot have 0 cells, so this is its empty case): pair 1 has flat scores, every
    confidence 1 / L^2; the counts and the neighbours' match sets come from the oracle"""
    ref, hip = pair
    g = torch.Generator().manual_seed(3)
    h, w, B = 30, 22, 3
    L = h * w
    f0 = torch.randn(B, L, 256, generator=g) * 2.2
    perm = torch.stack([torch.randperm(L, generator=g) for _ in range(B)])
    f1 = torch.gather(f0, 1, perm[..., None].expand(-1, -1, 256)) + 0.3 * torch.randn(B, L, 256, generator=g)
    f0[1] = 0.0
    cm = LR.coarse_matching(f0, f1, (h, w), (h, w))
    want = [int((cm["b_ids"] == k).sum()) for k in range(B)]
    assert want[1] == 0 and want[0] > L // 4 and want[2] > L // 4
    S = torch.bmm(f0 / 16.0, (f1 / 16.0).transpose(1, 2))
    for variant in (0, 1):
        i_ids, j_ids, mconf, n = [t.cpu() for t in hip.coarse_match(S.to(DEV), (h, w), (h, w), variant=variant)]
        assert int(n[1]) == 0
        for k in (0, 2):
            sel = cm["b_ids"] == k
            safe = (cm["mconf"][sel] - 0.2).abs() > 1e-3                  # (the band rule of test_coarse_match_vs_oracle)
            got = set(zip(i_ids[k, :n[k]].tolist(), j_ids[k, :n[k]].tolist()))
            sure = set(zip(cm["i_ids"][sel][safe].tolist(), cm["j_ids"][sel][safe].tolist()))
            assert sure <= got and len(got) - len(sure) <= int((~safe).sum())


@pytest.mark.parametrize("h,w,B", [(30, 22, 2), (90, 68, 1), (17, 13, 3)])
def test_coarse_match_two_sweep_equals_four_sweep(pair, h, w, B):
    """the tiled two-sweep kernels (default) against the row / column kernels of round 1 on the same S: identical mutual matches
    and confidences to fp32 round-off of the differently ordered logsumexp folds; sizes: a ragged tile (660 = not a multiple of the
    64-row stripe / 1024-column block), the Map-free size (6120: 6 column blocks, 96 stripes) and an odd width (221: scalar loads)"""
    ref, hip = pair
    g = torch.Generator().manual_seed(11 + h)
    L = h * w
    f0 = torch.randn(B, L, 256, generator=g) * 2.2
    perm = torch.stack([torch.randperm(L, generator=g) for _ in range(B)])
    f1 = torch.gather(f0, 1, perm[..., None].expand(-1, -1, 256)) + 0.3 * torch.randn(B, L, 256, generator=g)
    S = torch.bmm(f0.to(DEV) / 16.0, (f1.to(DEV) / 16.0).transpose(1, 2))
    a = [t.cpu() for t in hip.coarse_match(S, (h, w), (h, w), variant=0)]
    b = [t.cpu() for t in hip.coarse_match(S, (h, w), (h, w), variant=1)]
    for k in range(B):
        na, nb = int(a[3][k]), int(b[3][k])
        pa = {(int(i), int(j)): float(c) for i, j, c in zip(a[0][k, :na], a[1][k, :na], a[2][k, :na])}
        pb = {(int(i), int(j)): float(c) for i, j, c in zip(b[0][k, :nb], b[1][k, :nb], b[2][k, :nb])}
        assert nb > L // 4
        diff = set(pa) ^ set(pb)
        # a match can only appear / vanish if its confidence sits on the 0.2 threshold to round-off
        assert all(abs({**pa, **pb}[m] - 0.2) < 1e-5 for m in diff), (len(diff), na, nb)
        assert len(diff) <= 2
        common = set(pa) & set(pb)
        np.testing.assert_allclose([pa[m] for m in common], [pb[m] for m in common], rtol=2e-5)
        assert a[0][k, :na].tolist() == sorted(a[0][k, :na].tolist())           # ascending i, like upstream's nonzero order


def test_fine_window_gather_vs_unfold(pair):
    ref, hip = pair
    g = torch.Generator().manual_seed(3)
    Bimg, C, Hf, Wf, wc, hc = 4, 128, 60, 44, 11, 15
    feat = torch.randn(Bimg, C, Hf, Wf, generator=g)
    unf = F.unfold(feat, kernel_size=(5, 5), stride=4, padding=2).view(Bimg, C, 25, -1).permute(0, 3, 2, 1)   # [B, L, 25, C]
    M = 500
    img = torch.randint(0, Bimg, (M,), generator=g); cell = torch.randint(0, wc * hc, (M,), generator=g)
    got = hip.gather_windows(feat.permute(0, 2, 3, 1).contiguous().to(DEV), img.int().to(DEV), cell.int().to(DEV), wc, 4).cpu()
    np.testing.assert_array_equal(got.numpy(), unf[img, cell].numpy())


@pytest.mark.parametrize("hw", [(240, 176), (720, 544)])
def test_loftr_end_to_end_vs_oracle(pair, hw):
    """(720, 544) = the reference's padded Map-free input (matchers.py:41-46, quirk Q3)"""
    ref, hip = pair
    H, W = hw
    pr = IM.synthetic_pair(7, H, 540 if W == 544 else W)
    im0, im1 = torch.from_numpy(pr["img0"])[None, None], torch.from_numpy(pr["img1"])[None, None]
    torch.set_num_threads(16)
    want = LR.loftr_match_pair(ref, im0, im1)
    if W == 544:
        im0, im1 = F.pad(im0, (0, 4)), F.pad(im1, (0, 4))
    out = hip(torch.cat([im0, im1], 0).to(DEV))
    n = int(out["n_corr"][0])
    got = torch.cat([out["pts0"][0, :n], out["pts1"][0, :n]], 1).cpu().numpy()
    assert len(want) > 100 and not np.isnan(want).any()
    # same coarse matches (key = the two coarse cells); fine coordinates: the measured state of the shipped arithmetic with one unit of slack
    # (profiles/r06_loftr_stage_diff_hard2.json, 16 pairs: every coarse match common, 99th percentile <= 7.4e-4 px, maximum <= 9.3e-3 px, ~220 of ~5000
    # coordinates differ at all -- the SAME figures with the exact bf16x3 products: it is the backbone's fp32 summation order against oneDNN's, not the
    # f16x2 split).  This is the regression detector of the matcher: the pose-level census cannot be one (tests/test_gpu_parity_census.py).
    kw = {(int(r[0]), int(r[1])): r for r in want}
    kg = {(int(r[0]), int(r[1])): r for r in got}
    common = set(kw) & set(kg)
    assert len(common) >= 0.998 * max(len(kw), len(kg)), (len(kw), len(kg), len(common))
    d = np.array([np.abs(kw[k] - kg[k]).max() for k in common])
    assert np.quantile(d, 0.99) < 1e-3 and d.max() < 2e-2 and (d > 0).mean() < 0.15, (np.quantile(d, [0.5, 0.9, 0.99, 1.0]), (d > 0).mean())


@pytest.mark.parametrize("rows,C", [(1, 256), (1031, 256), (777, 128), (6120 * 3, 256)])
def test_fused_layernorm_vs_torch(rows, C):
    """csrc/loftr_fused.hip layernorm: strided input / residual / output (the [x | message] layout of nets/loftr.py) against
    torch.nn.functional.layer_norm in float64; in-place residual update included.  f32 tolerance 2e-6 * (1 + |y|)."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(rows + C)
    xm = torch.randn(rows, 2 * C, generator=g).to(DEV)
    m = (torch.randn(rows, C, generator=g) * 3 + 0.5).to(DEV)
    gam, bet = torch.randn(C, generator=g).to(DEV), torch.randn(C, generator=g).to(DEV)
    want1 = F.layer_norm(m.double().cpu(), (C,), gam.double().cpu(), bet.double().cpu(), 1e-5)
    keep = xm.clone()
    LoFTRHIP.layernorm(m, (gam, bet), xm[:, C:])                       # norm1 -> right half
    got1 = xm[:, C:].double().cpu()
    assert torch.equal(xm[:, :C], keep[:, :C])                         # left half untouched
    assert ((got1 - want1).abs() / (1 + want1.abs())).max().item() < 2e-6
    LoFTRHIP.layernorm(m, (gam, bet), xm[:, :C], residual=xm[:, :C])    # x += norm2(...) in place
    want2 = keep[:, :C].double().cpu() + want1
    assert ((xm[:, :C].double().cpu() - want2).abs() / (1 + want2.abs())).max().item() < 2e-6


@pytest.mark.parametrize("B,C,H,W", [(1, 3, 5, 7), (2, 8, 45, 34), (1, 4, 90, 68), (1, 2, 1, 1)])
def test_fused_upsample2x_add_vs_torch(pair, B, C, H, W):
    import torch.nn.functional as F
    _, hip = pair
    g = torch.Generator().manual_seed(H * W)
    lo = torch.randn(B, C, H, W, generator=g).to(DEV)
    y = torch.randn(B, C, 2 * H, 2 * W, generator=g).to(DEV)
    want = y.double().cpu() + F.interpolate(lo.double().cpu(), scale_factor=2.0, mode="bilinear", align_corners=True)
    lib32 = (y + F.interpolate(lo, scale_factor=2.0, mode="bilinear", align_corners=True)).double().cpu()     # the f32 library path it replaces
    got = hip.upsample2x_add(lo, y.clone()).double().cpu()
    # the source coordinate o * (H-1)/(2H-1) is formed in f32 (as in torch's kernel): ~1e-5 of a pixel at 180 rows, so
    # either f32 evaluation sits within a few 1e-5 of the f64 one (unit-scale data)
    assert (got - lib32).abs().max().item() < 5e-5 and (got - want).abs().max().item() < 5e-5


def test_fine_match_kernel_vs_torch_formula():
    """mfr_loftr_fine_match (FineMatching: matchers.py:50-55 -> mkpts1_f) against the torch statement of upstream's fine_matching.py:
    softmax(<f0 centre, f1 window> / sqrt C), dsnt.spatial_expectation2d over linspace(-1, 1, W)^2, mkpts1_f = mkpts1_c + expectation * (W // 2) * scale"""
    from mapfree_reloc_amd import _lib
    lib = _lib.load(require_gpu=True)
    g = torch.Generator().manual_seed(3)
    for M, W, C, ld in ((1, 5, 128, 256), (777, 5, 128, 256), (40, 3, 128, 128), (9, 7, 64, 96)):
        WW = W * W
        xf = torch.randn(2, M * WW, ld, generator=g).to(DEV) * 1.5
        L0 = 4 * M + 3
        k1 = (torch.rand(L0, 2, generator=g) * 500).to(DEV)
        lin = torch.randperm(L0, generator=g)[:M].int().to(DEV)
        pts1 = k1.clone(); expec = torch.empty(M, 2, device=DEV)
        _lib.check(lib.mfr_loftr_fine_match(_lib.ptr(xf[0]), _lib.ptr(xf[1]), ld, C, M, W, 4.0, _lib.ptr(lin), _lib.ptr(k1), _lib.ptr(pts1), _lib.ptr(expec),
                                            _lib.stream_ptr()), "fine_match")
        g0, g1 = xf[0].view(M, WW, ld)[..., :C].double(), xf[1].view(M, WW, ld)[..., :C].double()
        heat = torch.softmax(torch.einsum("mc,mrc->mr", g0[:, WW // 2], g1) / C ** .5, dim=1).view(M, W, W)
        l = torch.linspace(-1, 1, W, device=DEV, dtype=torch.float64)
        want = torch.stack([(heat * l[None, None, :]).sum((1, 2)), (heat * l[None, :, None]).sum((1, 2))], 1)
        assert (expec.double() - want).abs().max().item() < 2e-6
        ref = k1.double().clone(); ref[lin.long()] += want * 4.0
        assert (pts1.double() - ref).abs().max().item() < 2e-4           # 500-pixel coordinates in f32
        untouched = torch.ones(L0, dtype=torch.bool, device=DEV); untouched[lin.long()] = False
        assert torch.equal(pts1[untouched], k1[untouched])
