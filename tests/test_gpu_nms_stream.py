"""-m gpu tests of the streaming NMS kernel (csrc/superpoint_post.hip sp_nms_stream_kernel, mfr_sp_nms_candidates_variant 0).

The reference is oracle/nets_ref.simple_nms on the CPU; the tile kernel (variant 1) is a second witness.  Everything here is an equality: the
dense output bit for bit, the candidate keys as a set.  Sizes sit on the kernel's seams (U useful columns per strip, G output rows per segment,
both asked from the library); every size runs a batch of five score fields, each exercising an equality inside simple_nms."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from mapfree_reloc_amd import _lib
from mapfree_reloc_amd.nets import weights as WT
from mapfree_reloc_amd.nets.superpoint import SuperPointHIP
from oracle import nets_ref as NR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEAM_OFFSETS = (0, 4, 5, 8, 9, 12, 20)

# (rows, columns) as functions of (U, G)
SIZES = {
    "1x1": lambda U, G: (1, 1),
    "9x9": lambda U, G: (9, 9),
    "20x21": lambda U, G: (20, 21),
    "41x(U-1)": lambda U, G: (41, U - 1),
    "40xU": lambda U, G: (40, U),
    "45x(U+1)": lambda U, G: (45, U + 1),
    "(G-1)x(2U+1)": lambda U, G: (G - 1, 2 * U + 1),
    "Gx49": lambda U, G: (G, 49),
    "(G+1)x(2U)": lambda U, G: (G + 1, 2 * U),
}


@functools.lru_cache(maxsize=None)
def geometry():
    u, g = ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(_lib.load().mfr_sp_nms_stream_geometry(ctypes.byref(u), ctypes.byref(g)), "mfr_sp_nms_stream_geometry")
    assert u.value > 0 and g.value > 0
    return u.value, g.value


@functools.lru_cache(maxsize=None)
def detector():
    return SuperPointHIP(WT.superpoint_state_dict(1234), DEV)


def seam_field(H, W, U, G):
    """low noise with one maximum exactly on each strip seam and each segment seam and 4, 5, 8, 9, 12 and 20 pixels to either side of it (the
    distances at which a pool, a dilation or the whole halo ends); the peak values repeat, so the peaks tie with each other too"""
    g = torch.Generator().manual_seed(H * 1009 + W)
    s = torch.rand(H, W, generator=g) * 0.0625
    k = 0
    for c in range(0, W + U, U):                                # strip seams (the image's left edge included)
        for d in SEAM_OFFSETS:
            for x in {c - d, c + d}:
                if 0 <= x < W:
                    s[(7 * k + 3) % H, x] = 0.5 + 0.125 * (k % 3); k += 1
    for r in range(0, H + G, G):                                # segment seams
        for d in SEAM_OFFSETS:
            for y in {r - d, r + d}:
                if 0 <= y < H:
                    s[y, (11 * k + 5) % W] = 0.5 + 0.125 * (k % 3); k += 1
    return s


def fields(H, W):
    U, G = geometry()
    g = torch.Generator().manual_seed(H * 7919 + W)
    r = torch.rand(H, W, generator=g)
    r = r * r * r
    sparse = torch.zeros(H, W)
    m = torch.rand(H, W, generator=g) < 0.01
    sparse[m] = (torch.round(torch.rand(H, W, generator=g) * 16) / 16)[m]
    return torch.stack([r, torch.round(r * 64) / 64, torch.full((H, W), 0.25), sparse, seam_field(H, W, U, G)])


def expected_keys(nms, thr, border):
    """the candidate keys of one image from its reference NMS map: score bits << 32 | ~raster index for v > thr inside the border, sorted"""
    H, W = nms.shape
    a = nms.numpy()
    ys, xs = np.nonzero(a > np.float32(thr))
    keep = (xs >= border) & (xs < W - border) & (ys >= border) & (ys < H - border)
    ys, xs = ys[keep], xs[keep]
    bits = a[ys, xs].view(np.uint32).astype(np.uint64)
    idx = (~(ys * W + xs).astype(np.uint32)).astype(np.uint64)
    return np.sort((bits << np.uint64(32)) | idx)


def keys_of(cand, cnt):
    cand, cnt = cand.cpu().numpy().view(np.uint64), cnt.cpu().numpy()
    assert (cnt <= cand.shape[1]).all()
    return [np.sort(cand[b, :cnt[b]]) for b in range(cand.shape[0])], cnt


@functools.lru_cache(maxsize=None)
def run_case(name):
    """one batch of scores through the reference once and through both kernels; shared by the tests below and left unchanged"""
    U, G = geometry()
    if name == "720x536":                                       # the quantised scores of tests/test_gpu_nets_parity.py::test_nms_bit_exact
        g = torch.Generator().manual_seed(1)
        s = torch.rand(2, 720, 536, generator=g)
        s = torch.round(s * s * s * 64) / 64
    else:
        s = fields(*SIZES[name](U, G))
    hip = detector()
    want = NR.simple_nms(s, 4)
    sd = s.to(DEV)
    out = {"scores": s, "want": want, "expect": [expected_keys(want[b], hip.thr, hip.border) for b in range(s.shape[0])]}
    out["stream"] = hip.nms_candidates(sd, want_dense=True, variant=0)
    out["stream_again"] = hip.nms_candidates(sd, want_dense=True, variant=0)
    out["stream_no_dense"] = hip.nms_candidates(sd, want_dense=False, variant=0)
    out["tile"] = hip.nms_candidates(sd, want_dense=True, variant=1)
    torch.cuda.synchronize()
    return out


CASES = list(SIZES) + ["720x536"]


@pytest.mark.parametrize("name", CASES)
def test_dense_output_bit_equal(name):
    c = run_case(name)
    np.testing.assert_array_equal(c["stream"][2].cpu().numpy().view(np.uint32), c["want"].numpy().view(np.uint32))
    np.testing.assert_array_equal(c["tile"][2].cpu().numpy().view(np.uint32), c["want"].numpy().view(np.uint32))


@pytest.mark.parametrize("name", CASES)
def test_candidates_equal_reference_and_tile_kernel(name):
    c = run_case(name)
    ks, cnt_s = keys_of(*c["stream"][:2])
    kt, cnt_t = keys_of(*c["tile"][:2])
    np.testing.assert_array_equal(cnt_s, [len(e) for e in c["expect"]])
    np.testing.assert_array_equal(cnt_s, cnt_t)
    for b, e in enumerate(c["expect"]):
        np.testing.assert_array_equal(ks[b], e)
        np.testing.assert_array_equal(ks[b], kt[b])


@pytest.mark.parametrize("name", CASES)
def test_candidates_repeatable_and_independent_of_dense_output(name):
    c = run_case(name)
    ks, _ = keys_of(*c["stream"][:2])
    assert c["stream_no_dense"][2] is None
    for other in ("stream_again", "stream_no_dense"):
        ko, _ = keys_of(*c[other][:2])
        for a, o in zip(ks, ko):
            np.testing.assert_array_equal(a, o)


def test_candidate_cap_is_respected():
    """cand_cap = 8: the count is the true count, at most 8 keys of the image are stored, nothing is written behind a list"""
    U, G = geometry()
    c = run_case("(G-1)x(2U+1)")
    s = c["scores"][[0, 4]].contiguous()                       # the random field (hundreds of candidates) and the seam field
    expect = [c["expect"][0], c["expect"][4]]
    assert len(expect[0]) > 8
    hip, lib = detector(), _lib.load()
    B, H, W = s.shape
    cap, sentinel = 8, -0x0123456789abcdef
    cand = torch.full((B * cap + 256,), sentinel, dtype=torch.int64, device=DEV)
    cnt = torch.full((B + 16,), -7, dtype=torch.int32, device=DEV)
    _lib.check(lib.mfr_sp_nms_candidates_variant(_lib.ptr(s.to(DEV)), B, H, W, 4, hip.thr, hip.border, None, _lib.ptr(cand), cap, _lib.ptr(cnt), 0,
                                                 _lib.stream_ptr()), "mfr_sp_nms_candidates_variant")
    cand, cnt = cand.cpu(), cnt.cpu()
    assert (cand[B * cap:] == sentinel).all() and (cnt[B:] == -7).all()
    for b in range(B):
        assert int(cnt[b]) == len(expect[b])
        stored = cand[b * cap:(b + 1) * cap].numpy()
        stored = stored[stored != sentinel].view(np.uint64)
        assert len(stored) == min(cap, len(expect[b])) and len(np.unique(stored)) == len(stored)
        assert np.isin(stored, expect[b]).all()
