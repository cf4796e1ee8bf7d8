"""-m gpu: LoFTR's optimal-transport coarse matching (csrc/loftr_ot.hip, mfr_loftr_ot_match; LOFTR.MATCH_TYPE 'sinkhorn') against the
reference statement of tests/loftr_ot_ref.py (SuperGlue's log_optimal_transport + the oracle's get_coarse_match), kernel, module and
route level.  Inputs: the recipe of tests/test_gpu_loftr_parity.py with a gain (3.0 / 5.0: without the dual softmax's 1 / 0.1
temperature the gain 2.2 of those tests gives no optimal-transport match at all)."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mapfree_reloc_amd import _lib
from mapfree_reloc_amd import images as IM
from mapfree_reloc_amd.nets import weights as WT
from mapfree_reloc_amd.nets.loftr import LoFTRHIP
from oracle import loftr_ref as LR

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loftr_ot_ref as OT  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
THR = 0.2


def run_ot(S, hw0, hw1, bin_score=1.0, iters=3, variant=0, thr=THR, border=2, potentials=False):
    """mfr_loftr_ot_match through ctypes on a device tensor S [B, L0, L1] -> cpu (i_ids, j_ids, mconf, n[, u, v])"""
    lib = _lib.load(require_gpu=True)
    B, L0, L1 = S.shape
    assert S.is_cuda and S.is_contiguous() and L0 == hw0[0] * hw0[1] and L1 == hw1[0] * hw1[1]
    need = lib.mfr_loftr_ot_match_workspace_bytes(B, L0, L1)
    ws = torch.empty(need, dtype=torch.uint8, device=S.device)
    i_ids = torch.full((B, L0), -1, dtype=torch.int32, device=S.device); j_ids = torch.full_like(i_ids, -1)
    mconf = torch.zeros(B, L0, device=S.device); n = torch.full((B,), -1, dtype=torch.int32, device=S.device)
    u = torch.zeros(B, L0 + 1, device=S.device) if potentials else None
    v = torch.zeros(B, L1 + 1, device=S.device) if potentials else None
    _lib.check(lib.mfr_loftr_ot_match(_lib.ptr(S), B, hw0[0], hw0[1], hw1[0], hw1[1], bin_score, iters, thr, border, _lib.ptr(ws), need,
                                      _lib.ptr(i_ids), _lib.ptr(j_ids), _lib.ptr(mconf), _lib.ptr(n), _lib.ptr(u) if potentials else None,
                                      _lib.ptr(v) if potentials else None, variant, _lib.stream_ptr()), "mfr_loftr_ot_match")
    torch.cuda.synchronize()
    out = [i_ids.cpu(), j_ids.cpu(), mconf.cpu(), n.cpu()]
    return out + [u.cpu(), v.cpu()] if potentials else out


def scores(h, w, B, gain, hw1=None):
    f0, f1, perm = OT.make_features(h, w, B, gain)
    if hw1 is not None:
        f1 = f1[:, :hw1[0] * hw1[1]]
    return torch.bmm(f0 / 16.0, (f1 / 16.0).transpose(1, 2)).contiguous(), perm


def match_dict(out, k):
    n = int(out[3][k])
    return {(int(i), int(j)): float(c) for i, j, c in zip(out[0][k, :n], out[1][k, :n], out[2][k, :n])}


# (h, w, B, gain, bin_score, second grid or None): the cases checked on the CPU with the fp32 and the fp64 reference (identical match
# sets, the reference alone inside the band cap)
CASES = [(30, 22, 2, 3.0, 1.0, None), (30, 22, 2, 3.0, 2.5, None), (30, 22, 2, 3.0, 1.0, (24, 20)), (30, 22, 2, 3.0, 2.5, (24, 20)),
         (30, 22, 2, 5.0, 1.0, None), (90, 68, 1, 3.0, 1.0, None), (90, 68, 1, 5.0, 1.0, None), (17, 13, 3, 3.0, 1.0, None),
         (17, 13, 3, 3.0, 2.5, None)]
CASES_ITERS = [c + (3,) for c in CASES] + [c + (it,) for c in CASES if c[0] == 30 for it in (1, 20)]


@pytest.mark.parametrize("h,w,B,gain,bin_score,hw1,iters", CASES_ITERS)
def test_ot_match_sets_vs_reference(h, w, B, gain, bin_score, hw1, iters):
    """the rule of test_coarse_match_vs_oracle: matches within 1e-3 of the threshold (either side) are counted and printed, the band is
    thin, the symmetric difference fits in it, outside it ids are equal and confidences agree to rtol 2e-4"""
    S, _ = scores(h, w, B, gain, hw1)
    hw1 = hw1 or (h, w)
    cm = OT.select_matches(OT.ot_conf(S, bin_score, iters), (h, w), hw1, THR, 2)
    i_ids, j_ids, mconf, n = run_ot(S.to(DEV), (h, w), hw1, bin_score, iters)
    L = h * w
    for b in range(B):
        sel = cm["b_ids"] == b
        wi, wj, wc = cm["i_ids"][sel], cm["j_ids"][sel], cm["mconf"][sel]
        safe_w = (wc - THR).abs() > 1e-3
        gi, gj, gc = i_ids[b, :n[b]].long(), j_ids[b, :n[b]].long(), mconf[b, :n[b]]
        safe_g = (gc - THR).abs() > 1e-3
        assert len(wi) > L // 4
        n_band = int((~safe_w).sum()) + int((~safe_g).sum())
        pw = {(int(a), int(c)) for a, c in zip(wi.tolist(), wj.tolist())}; pg = {(int(a), int(c)) for a, c in zip(gi.tolist(), gj.tolist())}
        print(f"OT pair {b} ({h}x{w} vs {hw1}, gain {gain}, bin {bin_score}, {iters} iters): {len(pw)} reference / {len(pg)} HIP matches, "
              f"{n_band} within 1e-3 of the threshold, {len(pw ^ pg)} differ in all")
        assert n_band <= max(4, len(wi) // 50) and len(pw ^ pg) <= n_band
        np.testing.assert_array_equal(gi[safe_g].numpy(), wi[safe_w].numpy())
        np.testing.assert_array_equal(gj[safe_g].numpy(), wj[safe_w].numpy())
        np.testing.assert_allclose(gc[safe_g].numpy(), wc[safe_w].numpy(), rtol=2e-4)


def test_bin_score_moves_the_matches():
    """a kernel that ignored bin_score would give the same set for 1.0 and 2.5 (reference: 667 vs 657 matches on this S)"""
    S, _ = scores(30, 22, 2, 3.0)
    a = run_ot(S.to(DEV), (30, 22), (30, 22), 1.0)
    b = run_ot(S.to(DEV), (30, 22), (30, 22), 2.5)
    assert int(a[3].sum()) != int(b[3].sum())
    assert abs(float(a[2][0, :a[3][0]].median()) - float(b[2][0, :b[3][0]].median())) > 0.05


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("h,w,B,gain,bin_score,iters", [(30, 22, 2, 3.0, 1.0, 1), (30, 22, 2, 3.0, 1.0, 3), (30, 22, 2, 3.0, 2.5, 3),
                                                        (30, 22, 2, 5.0, 1.0, 20), (17, 13, 3, 3.0, 1.0, 3), (17, 13, 3, 3.0, 2.5, 20)])
def test_ot_potentials_vs_float64(h, w, B, gain, bin_score, iters, variant):
    """the full (L0 + 1) x (L1 + 1) log assignment rebuilt from the kernel's potentials against log_optimal_transport in float64 on the
    same S.  Bar: d_ref = max |Z_fp32ref - Z_fp64ref| measured here; the HIP result within max(4 * d_ref, 2e-5) of the fp64 reference
    (factor 4: hardware exp / log against libm's, tile-order folds against torch's pairwise sums)."""
    S, _ = scores(h, w, B, gain)
    z64 = OT.ot_log_assignment(S, bin_score, iters, torch.float64)
    d_ref = float((OT.ot_log_assignment(S, bin_score, iters).double() - z64).abs().max())
    out = run_ot(S.to(DEV), (h, w), (h, w), bin_score, iters, variant=variant, potentials=True)
    u, v = out[4].double(), out[5].double()
    m = n = h * w
    norm = -np.log(m + n)
    z0 = torch.full((B, m + 1, n + 1), float(bin_score), dtype=torch.float64)
    z0[:, :m, :n] = S.double()
    z = z0 + u[:, :, None] + v[:, None, :] - norm
    d_hip = float((z - z64).abs().max())
    print(f"OT potentials {h}x{w} gain {gain} bin {bin_score} {iters} iters variant {variant}: d_ref {d_ref:.3e}, HIP distance {d_hip:.3e}, "
          f"bar {max(4 * d_ref, 2e-5):.3e}")
    assert torch.isfinite(z).all()
    assert d_hip <= max(4 * d_ref, 2e-5)


@pytest.mark.parametrize("gain", [3.0, 5.0])
@pytest.mark.parametrize("h,w,B", [(30, 22, 2), (90, 68, 1), (17, 13, 3)])
def test_ot_one_sweep_per_iteration_equals_row_and_column_kernels(h, w, B, gain):
    """variant 0 against variant 1 on the same S (the rule of test_coarse_match_two_sweep_equals_four_sweep): a match may differ only if
    its confidence is within 1e-5 of the threshold -- at most 2 such plus however many the fp32 reference has there on this S"""
    S, _ = scores(h, w, B, gain)
    ref = OT.select_matches(OT.ot_conf(S, 1.0, 3), (h, w), (h, w), THR, 2)
    a = run_ot(S.to(DEV), (h, w), (h, w), variant=0)
    b = run_ot(S.to(DEV), (h, w), (h, w), variant=1)
    for k in range(B):
        n_edge = int(((ref["mconf"][ref["b_ids"] == k] - THR).abs() < 1e-5).sum())
        pa, pb = match_dict(a, k), match_dict(b, k)
        na, nb = len(pa), len(pb)
        assert nb > h * w // 4
        diff = set(pa) ^ set(pb)
        print(f"OT variants pair {k} ({h}x{w}, gain {gain}): {na} / {nb} matches, {len(diff)} differ, reference has {n_edge} within 1e-5 of the threshold")
        assert all(abs({**pa, **pb}[m] - THR) < 1e-5 for m in diff), (len(diff), na, nb)
        assert len(diff) <= 2 + n_edge
        common = sorted(set(pa) & set(pb))
        np.testing.assert_allclose([pa[m] for m in common], [pb[m] for m in common], rtol=2e-5)
        assert a[0][k, :na].tolist() == sorted(a[0][k, :na].tolist())


@pytest.mark.parametrize("variant", [0, 1])
def test_ot_match_is_deterministic_and_leaves_S_alone(variant):
    S, _ = scores(90, 68, 2, 3.0)
    Sd = S.to(DEV)
    keep = Sd.clone()
    a = run_ot(Sd, (90, 68), (90, 68), potentials=True, variant=variant)
    b = run_ot(Sd, (90, 68), (90, 68), potentials=True, variant=variant)
    assert torch.equal(Sd, keep)
    assert torch.equal(a[3], b[3]) and int(a[3].min()) > 1000
    for k in range(2):
        n = int(a[3][k])
        for x, y in zip(a[:3], b[:3]):
            assert torch.equal(x[k, :n], y[k, :n])
    assert torch.equal(a[4], b[4]) and torch.equal(a[5], b[5])


def test_ot_border_swallows_a_small_grid():
    g = torch.Generator().manual_seed(1)
    S = (torch.randn(1, 16, 16, generator=g) * 3).to(DEV)
    out = run_ot(S, (4, 4), (4, 4), border=2)
    assert int(out[3][0]) == 0


def test_ot_single_row():
    """L0 = 1: one row against 20 columns (border 0: the helper's border removal cannot express 'none', so the selection is stated here)"""
    S = torch.zeros(1, 1, 20); S[0, 0, 7] = 5.0
    conf = OT.ot_conf(S, 1.0, 3)
    assert float(conf[0, 0, 7]) > 0.5 and int(conf[0, 0].argmax()) == 7
    for variant in (0, 1):
        i_ids, j_ids, mconf, n, u, v = run_ot(S.to(DEV), (1, 1), (4, 5), border=0, variant=variant, potentials=True)
        assert int(n[0]) == 1 and int(i_ids[0, 0]) == 0 and int(j_ids[0, 0]) == 7
        np.testing.assert_allclose(float(mconf[0, 0]), float(conf[0, 0, 7]), rtol=2e-4)
        assert u.shape == (1, 2) and v.shape == (1, 21) and torch.isfinite(u).all() and torch.isfinite(v).all()
    # ... and a single column
    for variant in (0, 1):
        i_ids, j_ids, mconf, n = run_ot(S.transpose(1, 2).contiguous().to(DEV), (4, 5), (1, 1), border=0, variant=variant)
        want = OT.ot_conf(S.transpose(1, 2).contiguous(), 1.0, 3)
        assert int(n[0]) == 1 and int(i_ids[0, 0]) == 7 and int(j_ids[0, 0]) == 0
        np.testing.assert_allclose(float(mconf[0, 0]), float(want[0, 7, 0]), rtol=2e-4)


def test_ot_pair_without_matches_between_pairs_with_some():
    S, _ = scores(30, 22, 3, 3.0)
    S[1] = 0.0                                              # flat scores: every confidence far below the threshold
    cm = OT.select_matches(OT.ot_conf(S, 1.0, 3), (30, 22), (30, 22), THR, 2)
    want = [int((cm["b_ids"] == k).sum()) for k in range(3)]
    assert want[1] == 0 and want[0] > 100 and want[2] > 100
    for variant in (0, 1):
        out = run_ot(S.to(DEV), (30, 22), (30, 22), variant=variant)
        assert out[3].tolist() == want
        for k in (0, 2):
            sel = cm["b_ids"] == k
            assert set(match_dict(out, k)) == set(zip(cm["i_ids"][sel].tolist(), cm["j_ids"][sel].tolist()))


def test_ot_tie_reports_the_lower_column():
    """two bit-identical columns, both the best of one interior row (each gets about half of the row's mass, 0.4676 > 0.2): the LOWER j
    is reported -- the rule of the dual-softmax kernel.  Asserted against the rule, not the reference (torch's arg-max on ties is
    unspecified)."""
    S, perm = scores(30, 22, 1, 3.0)
    S[:, :, 47] = S[:, :, 46]
    i = int(perm[0, 46])
    y, x = divmod(i, 22)
    assert 2 <= y < 28 and 2 <= x < 20                      # an interior row; columns 46, 47 = cells (2, 2), (2, 3) are interior too
    conf = OT.ot_conf(S, 1.0, 3)
    assert conf[0, i, 46] == conf[0, i, 47] == conf[0, i].max() and float(conf[0, i, 46]) > 0.4
    seen = []
    for variant in (0, 1, 0):
        out = run_ot(S.to(DEV), (30, 22), (30, 22), variant=variant)
        m = match_dict(out, 0)
        assert (i, 46) in m and (i, 47) not in m
        np.testing.assert_allclose(m[(i, 46)], float(conf[0, i, 46]), rtol=2e-4)
        seen.append(m)
    assert seen[0] == seen[2]


# ---------------------------------------------------------------------------------------------------------------- module level
def _end_to_end(ref, hip, hw, b, monkeypatch):
    H, W = hw
    monkeypatch.setattr(LR, "coarse_matching",
                        lambda f0, f1, hw0, hw1, scale=8: OT.ot_coarse_matching(f0, f1, hw0, hw1, bin_score=b, iters=3, scale=scale))
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
    kw = {(int(r[0]), int(r[1])): r for r in want}
    kg = {(int(r[0]), int(r[1])): r for r in got}
    common = set(kw) & set(kg)
    d = np.array([np.abs(kw[k] - kg[k]).max() for k in common])
    print(f"OT end to end {hw} bin {b}: {len(kw)} reference / {len(kg)} HIP matches, {len(common)} common, fine 99th {np.quantile(d, 0.99):.2e} max {d.max():.2e}")
    assert len(common) >= 0.998 * max(len(kw), len(kg)), (len(kw), len(kg), len(common))
    assert np.quantile(d, 0.99) < 1e-3 and d.max() < 2e-2, np.quantile(d, [0.5, 0.9, 0.99, 1.0])
    return kg


@pytest.mark.parametrize("hw", [(240, 176), (720, 544)])
def test_loftr_sinkhorn_end_to_end_vs_oracle(hw, monkeypatch):
    """LoFTRHIP(match_type='sinkhorn') against LoFTRRef with the optimal-transport statement in place of coarse_matching; feat_gain 3.0
    (the default 20 saturates the confidences: the fp32 and fp64 reference then already disagree through exact ties).  (720, 544) = the
    padded Map-free input."""
    sets = {}
    for b in (1.0, 2.5):
        sd = WT.loftr_state_dict(feat_gain=3.0, bin_score=b)
        ref = LR.LoFTRRef().eval()
        ref.load_state_dict({k: v for k, v in sd.items() if k != "coarse_matching.bin_score"})
        hip = LoFTRHIP(sd, DEV, match_type="sinkhorn")
        assert hip.bin_score == b and hip.skh_iters == 3
        sets[b] = set(_end_to_end(ref, hip, hw, b, monkeypatch))
    assert sets[1.0] != sets[2.5]                           # the checkpoint's bin_score reaches the kernel (a dropped one gives the same set twice)


def test_default_match_type_is_unchanged_bit_for_bit():
    """a state dict WITH the bin_score key and no new argument runs the dual softmax exactly as a plain dict does"""
    pr = IM.synthetic_pair(7, 240, 176)
    ims = torch.from_numpy(np.stack([pr["img0"], pr["img1"]]))[:, None].to(DEV)
    a = LoFTRHIP(WT.loftr_state_dict(bin_score=2.5), DEV)(ims)
    b = LoFTRHIP(WT.loftr_state_dict(), DEV)(ims)
    c = LoFTRHIP(WT.loftr_state_dict(), DEV, match_type="sinkhorn")(ims)
    n = int(a["n_corr"][0])
    assert n > 100 and torch.equal(a["n_corr"], b["n_corr"])
    for k in ("pts0", "pts1", "mconf", "i_ids", "j_ids"):
        assert torch.equal(a[k][0, :n], b[k][0, :n]), k
    assert not torch.equal(a["mconf"][0, :n], c["mconf"][0, :n])      # ... and the switch does switch


# ---------------------------------------------------------------------------------------------------------------- route level
def test_emat_pipeline_with_sinkhorn_matching():
    from mapfree_reloc_amd.pipeline import LoFTREmatPipeline
    sb = IM.synthetic_batch([3, 4])
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in sb.items()}
    pipe = LoFTREmatPipeline("cuda", match_type="sinkhorn")
    assert pipe.loftr.match_type == "sinkhorn"
    lo = pipe(d["images"], d["depth0"], d["depth1"], d["K0"], d["K1"], d["pair_ids"])
    assert (lo["status"] == 0).all() and (lo["n_corr"] > 100).all()
    assert torch.isfinite(lo["R"]).all() and torch.isfinite(lo["t"]).all()


def test_plugin_sinkhorn_graph_replay_equals_eager(tmp_path):
    """LoFTRMatching from a cfg with LOFTR.MATCH_TYPE sinkhorn: the coarse stage (now with the Sinkhorn launches) still captures into one
    HIP graph and replays to the eager result; a failed capture would only warn and fall back, so warnings are errors here"""
    from mapfree_reloc_amd.config import get_cfg_defaults
    from mapfree_reloc_amd.datasets import SyntheticScene, collate_batch1
    from mapfree_reloc_amd.matching.feature_matching import LoFTRMatching
    cfg = get_cfg_defaults()
    y = tmp_path / "ot.yaml"
    y.write_text("LOFTR:\n  MATCH_TYPE: sinkhorn\n")
    cfg.merge_from_file(str(y))
    cfg.MODEL, cfg.FEATURE_MATCHING, cfg.POSE_SOLVER = "FeatureMatching", "LoFTR", "EssentialMatrixMetric"
    cfg.ALLOW_SYNTHETIC_WEIGHTS = True
    sc = SyntheticScene(5, frames=3)
    samples = [collate_batch1(sc[i]) for i in range(3)]
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        cfg.HIP.GRAPH_BATCH1 = False
        eager = LoFTRMatching(cfg)
        cfg.HIP.GRAPH_BATCH1 = True
        graphed = LoFTRMatching(cfg)
        assert eager.net.match_type == graphed.net.match_type == "sinkhorn"
        for s in samples + samples[:2]:
            a0, a1 = eager.get_correspondences(s)
            b0, b1 = graphed.get_correspondences(s)
            assert len(a0) > 100 and np.array_equal(a0, b0) and np.array_equal(a1, b1)
    assert not [str(r.message) for r in rec if "running eagerly" in str(r.message)]
    assert graphed.use_graph and len(graphed._graphs) == 1
