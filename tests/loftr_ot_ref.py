"""Reference statement of LoFTR's optimal-transport coarse matching for the tests (CPU, torch): upstream CoarseMatching with
MATCH_TYPE 'sinkhorn' = log_optimal_transport (oracle/nets_ref.py, SuperGlue's; bit-identical to HuggingFace's function, see
tests/test_loftr_ot_host.py) on the similarity matrix WITHOUT a temperature, the dustbins cut off, then get_coarse_match exactly
as in oracle/loftr_ref.coarse_matching.  Also the shared input recipe of the GPU tests."""
import torch

from oracle import loftr_ref as LR
from oracle import nets_ref as NR


def ot_log_assignment(S, bin_score, iters, dtype=None):
    """S [B, m, n] -> the full [B, m + 1, n + 1] log assignment (dustbin row / column last) in S's dtype or `dtype`"""
    S = S if dtype is None else S.to(dtype)
    return NR.log_optimal_transport(S, torch.tensor(bin_score, dtype=S.dtype), iters)


def ot_conf(S, bin_score, iters, dtype=None):
    return ot_log_assignment(S, bin_score, iters, dtype).exp()[:, :-1, :-1]


def select_matches(conf, hw0, hw1, thr=0.2, border_rm=2, scale=8):
    """get_coarse_match: oracle/loftr_ref.coarse_matching from the threshold on, verbatim"""
    mask = conf > thr
    n = conf.shape[0]
    mask = mask.view(n, hw0[0], hw0[1], hw1[0], hw1[1]).clone()
    LR.mask_border(mask, border_rm, False)
    mask = mask.view(n, hw0[0] * hw0[1], hw1[0] * hw1[1])
    mask = mask * (conf == conf.max(dim=2, keepdim=True)[0]) * (conf == conf.max(dim=1, keepdim=True)[0])
    mask_v, all_j_ids = mask.max(dim=2)
    b_ids, i_ids = torch.where(mask_v)
    j_ids = all_j_ids[b_ids, i_ids]
    mconf = conf[b_ids, i_ids, j_ids]
    mkpts0_c = torch.stack([i_ids % hw0[1], i_ids // hw0[1]], dim=1) * scale
    mkpts1_c = torch.stack([j_ids % hw1[1], j_ids // hw1[1]], dim=1) * scale
    return dict(b_ids=b_ids, i_ids=i_ids, j_ids=j_ids, mconf=mconf, mkpts0_c=mkpts0_c.float(), mkpts1_c=mkpts1_c.float(),
                conf_matrix=conf)


def similarity(f0, f1):
    C = f0.shape[-1]
    return torch.einsum("nlc,nsc->nls", f0 / C ** .5, f1 / C ** .5)


def ot_coarse_matching(feat_c0, feat_c1, hw0, hw1, bin_score=1.0, iters=3, thr=0.2, border_rm=2, scale=8, dtype=None):
    """drop-in for oracle/loftr_ref.coarse_matching with the sinkhorn match type"""
    conf = ot_conf(similarity(feat_c0, feat_c1), bin_score, iters, dtype)
    return select_matches(conf, hw0, hw1, thr, border_rm, scale)


def make_features(h, w, B, gain):
    """the input recipe of tests/test_gpu_loftr_parity.py:96-101 with a gain: features and a noisy permuted copy"""
    g = torch.Generator().manual_seed(11 + h)
    L = h * w
    f0 = torch.randn(B, L, 256, generator=g) * gain
    perm = torch.stack([torch.randperm(L, generator=g) for _ in range(B)])
    f1 = torch.gather(f0, 1, perm[..., None].expand(-1, -1, 256)) + 0.3 * gain / 2.2 * torch.randn(B, L, 256, generator=g)
    return f0, f1, perm
