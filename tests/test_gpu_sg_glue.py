"""-m gpu tests of SuperGlue's per-step glue as native code: mfr_sg_kenc_in (csrc/elementwise.hip), SuperPoint's descriptors sampled straight into
the [x | a] buffer (mfr_sp_sample_descriptors_ld + the accumulating last keypoint-encoder layer) and the match head on the interleaved [2B]
tensors (mfr_sg_sinkhorn_match_strided).  Every check is bit equality with the route it replaces; no tolerance anywhere."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mapfree_reloc_amd import _lib
from mapfree_reloc_amd.nets import weights as WT
from mapfree_reloc_amd.nets.superpoint import SuperPointHIP
from mapfree_reloc_amd.nets.superglue import SuperGlueHIP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B2, K, N_LIST, HW = 4, 70, [70, 33, 0, 1], (48, 36)


def bits(t):
    return t.detach().contiguous().cpu().numpy().view(np.int32)


def kenc_in_reference(kpts, scores, w0, b0, image_hw):
    """the framework expression mfr_sg_kenc_in replaces (nets/superglue.py before it): normalize_keypoints + layer 0 of the keypoint encoder"""
    H, W = image_hw
    size = torch.tensor([float(W), float(H)], device=kpts.device)
    kn = (kpts - size / 2) / (float(max(W, H)) * 0.7)
    h = (kn[..., 0:1] * w0[:, 0] + kn[..., 1:2] * w0[:, 1]) + (scores.unsqueeze(-1) * w0[:, 2] + b0)
    return F.relu_(h).reshape(-1, w0.shape[0])


@pytest.fixture(scope="module")
def nets():
    return SuperPointHIP(WT.superpoint_state_dict(1234), DEV, max_keypoints=K), SuperGlueHIP(WT.superglue_state_dict(4321), DEV)


@pytest.fixture(scope="module")
def keypoints():
    """integer pixel positions and scores for rows < n, zeros beyond (what SuperPointHIP.select leaves)"""
    g = torch.Generator().manual_seed(5)
    H, W = HW
    kpts, sc = torch.zeros(B2, K, 2), torch.zeros(B2, K)
    for b, n in enumerate(N_LIST):
        kpts[b, :n, 0] = torch.randint(0, W, (n,), generator=g).float()
        kpts[b, :n, 1] = torch.randint(0, H, (n,), generator=g).float()
        sc[b, :n] = torch.rand(n, generator=g)
    dense = torch.randn(B2, H // 8, W // 8, 256, generator=g)
    return kpts.to(DEV), sc.to(DEV), torch.tensor(N_LIST, dtype=torch.int32, device=DEV), dense.to(DEV)


def test_kenc_in_bit_equal_to_the_expression_it_replaces(nets, keypoints):
    _, sg = nets
    kpts, sc, _, _ = keypoints
    w0, b0 = sg.kenc[0]
    want = kenc_in_reference(kpts, sc, w0, b0, HW)
    got = torch.full((B2 * K, 32), float("nan"), device=DEV)
    _lib.check(_lib.load().mfr_sg_kenc_in(_lib.ptr(kpts), _lib.ptr(sc), _lib.ptr(w0), _lib.ptr(b0), B2 * K, HW[0], HW[1], _lib.ptr(got), _lib.stream_ptr()),
               "mfr_sg_kenc_in")
    np.testing.assert_array_equal(bits(got), bits(want))
    assert float(want.max()) > 0 and float((want == 0).float().mean()) > 0.05          # both sides of the ReLU occur
    # another aspect and size: W > H, a scale that is no power of two
    big = kpts * 7.25
    want = kenc_in_reference(big, sc, w0, b0, (540, 720))
    _lib.check(_lib.load().mfr_sg_kenc_in(_lib.ptr(big), _lib.ptr(sc), _lib.ptr(w0), _lib.ptr(b0), B2 * K, 540, 720, _lib.ptr(got), _lib.stream_ptr()),
               "mfr_sg_kenc_in")
    np.testing.assert_array_equal(bits(got), bits(want))


def test_sample_into_the_xa_buffer(nets, keypoints):
    sp, sg = nets
    kpts, _, n, dense = keypoints
    want = sp.sample(dense, kpts, n)
    pattern = 0x7fc12345
    xa = torch.full((B2 * K, 512), pattern, dtype=torch.int32, device=DEV).view(torch.float32)
    view = xa.view(B2, K, 512)[:, :, :256]
    got = sp.sample(dense, kpts, n, out=view)
    assert got.data_ptr() == xa.data_ptr()
    np.testing.assert_array_equal(bits(xa[:, :256]).reshape(B2, K, 256), bits(want))
    assert (bits(xa[:, 256:]) == pattern).all()
    for b, nb in enumerate(N_LIST):
        assert (bits(view[b, nb:]) == 0).all()
        assert nb == 0 or float(view[b, :nb].abs().sum()) > 0


def test_final_descriptors_in_place_equals_copy_route(nets, keypoints):
    sp, sg = nets
    kpts, sc, n, dense = keypoints
    want = sg.final_descriptors(kpts, sc, sp.sample(dense, kpts, n), n, HW).clone()
    assert sg._xa is None
    view = sg.xa_buffer(B2, K)
    sp.sample(dense, kpts, n, out=view)
    got = sg.final_descriptors(kpts, sc, view, n, HW)
    assert sg._xa is None                                          # the buffer was recognised and taken
    np.testing.assert_array_equal(bits(got), bits(want))
    assert np.isfinite(want[0].cpu().numpy()).all() and float(want[0].abs().sum()) > 0


def _structured_scores(g, B, m_list, n_list, ld):
    S = torch.randn(B, ld, ld, generator=g) * 0.5
    for b in range(B):
        k = min(m_list[b], n_list[b])
        perm = torch.randperm(n_list[b], generator=g)[:k]
        S[b, torch.arange(k), perm] += torch.rand(k, generator=g) * 12
    return S


@pytest.fixture(scope="module")
def match_case(nets):
    """the ragged m / n lists of tests/test_gpu_nets_parity.py::test_sinkhorn_one_sweep_equals_two_pass_bitwise at ldS = 1024, as the interleaved [2B]
    tensors the matcher holds, and the result of the contiguous entry point on copies of their halves"""
    _, sg = nets
    g = torch.Generator().manual_seed(61)
    m_list = [1024, 611, 40, 1, 1000, 65, 0, 777, 16, 49]
    n_list = [1024, 1000, 17, 5, 3, 64, 12, 778, 1023, 48]
    B, ld = len(m_list), 1024
    S = _structured_scores(g, B, [max(m, 1) for m in m_list], [max(n, 1) for n in n_list], ld).to(DEV)
    kp = (torch.rand(2 * B, ld, 2, generator=g) * 500).to(DEV)
    n = torch.tensor([v for mn in zip(m_list, n_list) for v in mn], dtype=torch.int32, device=DEV)
    want = _call_match(sg, S, n[0::2].contiguous(), n[1::2].contiguous(), kp[0::2].contiguous(), kp[1::2].contiguous(), ld, strided=False)
    assert int(want["n_corr"].sum()) > 1000
    return sg, S, kp, n, ld, want


def _call_match(sg, S, n0, n1, k0, k1, maxN, strided, prefill=0.0):
    """the C entry points on buffers of the test's own (pts0 / pts1 prefilled)"""
    lib = _lib.load()
    B, ld, _ = S.shape
    Kk = k0.shape[1]
    ws = torch.empty(lib.mfr_sg_match_workspace_bytes(B, ld), dtype=torch.uint8, device=DEV)
    o = dict(matches0=torch.empty(B, ld, dtype=torch.int32, device=DEV), matching_scores0=torch.empty(B, ld, device=DEV),
             pts0=torch.full((B, maxN, 2), prefill, device=DEV), pts1=torch.full((B, maxN, 2), prefill, device=DEV),
             n_corr=torch.empty(B, dtype=torch.int32, device=DEV))
    tail = (_lib.ptr(ws), ws.numel(), _lib.ptr(o["matches0"]), _lib.ptr(o["matching_scores0"]), _lib.ptr(o["pts0"]), _lib.ptr(o["pts1"]), maxN, _lib.ptr(o["n_corr"]),
            0, _lib.stream_ptr())
    if strided:
        assert n0.stride(0) == n1.stride(0) and k0.stride() == k1.stride() and k0.stride()[1:] == (2, 1)
        _lib.check(lib.mfr_sg_sinkhorn_match_strided(_lib.ptr(S), B, ld, n0.data_ptr(), n1.data_ptr(), n0.stride(0), sg.bin_score, sg.iters, sg.match_thr,
                                                     k0.data_ptr(), k1.data_ptr(), Kk, k0.stride(0), *tail), "mfr_sg_sinkhorn_match_strided")
    else:
        _lib.check(lib.mfr_sg_sinkhorn_match_variant(_lib.ptr(S), B, ld, _lib.ptr(n0), _lib.ptr(n1), sg.bin_score, sg.iters, sg.match_thr,
                                                     _lib.ptr(k0), _lib.ptr(k1), Kk, *tail), "mfr_sg_sinkhorn_match_variant")
    return o


def test_match_head_on_interleaved_views(match_case):
    sg, S, kp, n, ld, want = match_case
    assert not kp[0::2].is_contiguous() and not n[1::2].is_contiguous()
    got = sg.sinkhorn_match(S, n[0::2], n[1::2], kp[0::2], kp[1::2])
    for k in want:
        np.testing.assert_array_equal(bits(got[k]), bits(want[k]), err_msg=k)
    # NaN-prefilled point lists: every row from n_corr on comes back zero
    got = _call_match(sg, S, n[0::2], n[1::2], kp[0::2], kp[1::2], ld, strided=True, prefill=float("nan"))
    for k in want:
        np.testing.assert_array_equal(bits(got[k]), bits(want[k]), err_msg=k)
    for b, nc in enumerate(want["n_corr"].tolist()):
        assert (bits(got["pts0"][b, nc:]) == 0).all() and (bits(got["pts1"][b, nc:]) == 0).all()


def test_match_head_fewer_rows_than_matches(match_case):
    sg, S, kp, n, ld, want = match_case
    maxN = 16
    got = _call_match(sg, S, n[0::2], n[1::2], kp[0::2], kp[1::2], maxN, strided=True, prefill=float("nan"))
    nc = want["n_corr"].clamp(max=maxN)
    assert int(want["n_corr"].max()) > maxN
    np.testing.assert_array_equal(got["n_corr"].cpu().numpy(), nc.cpu().numpy())
    np.testing.assert_array_equal(bits(got["matches0"]), bits(want["matches0"]))
    for k in ("pts0", "pts1"):
        np.testing.assert_array_equal(bits(got[k]), bits(want[k][:, :maxN]), err_msg=k)    # the first rows of the full lists; zeros where those had none


def test_whole_matcher_in_place_equals_fallback_route():
    """SuperGluePnPPipeline.match on 2 synthetic pairs at 96 x 72: descriptors sampled into the [x | a] buffer, strided match head and the library's
    default NMS kernel against a separate descriptor tensor, contiguous copies and the tile NMS kernel"""
    from mapfree_reloc_amd.pipeline import SuperGluePnPPipeline
    g = torch.Generator().manual_seed(9)
    ref = F.avg_pool2d(torch.rand(2, 1, 96 + 2, 72 + 2, generator=g), 3, 1)
    qry = torch.roll(ref, (3, -2), (2, 3)) * 0.9 + 0.05
    images = torch.stack([ref, qry], 1).reshape(4, 1, 96, 72).contiguous().to(DEV)
    pipe = SuperGluePnPPipeline(DEV, seed=0)
    a = {k: v.clone() for k, v in pipe.match(images).items()}
    pipe.sg.in_place, pipe.sp.nms_variant = False, 1
    b = pipe.match(images)
    for k in ("pts0", "pts1", "n_corr", "matches0", "matching_scores0", "n_kpts"):
        np.testing.assert_array_equal(bits(a[k]), bits(b[k]), err_msg=k)
    assert int(a["n_kpts"].min()) > 0
