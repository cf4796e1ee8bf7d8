"""The device JPEG decoder (csrc/jpeg.hip, jpeg_ops.JpegDecoder) against PIL, bit for bit: RGB u8 = Image.open(f).convert("RGB"), gray
plane = datasets.read_gray_plane(f, None).  Inputs are encoded at test time with PIL's encoder."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

import mapfree_reloc_amd  # noqa: F401
from mapfree_reloc_amd import datasets as D, images as IM, jpeg_ops as J

pytestmark = pytest.mark.gpu

H, W = 720, 540


def enc(a, **kw):
    """PIL's encoder with an output block large enough for one pass: with optimize=True libjpeg refuses to suspend (noise at q >= 92)"""
    from PIL import ImageFile
    saved, ImageFile.MAXBLOCK = ImageFile.MAXBLOCK, max(ImageFile.MAXBLOCK, 4 * a.size + (1 << 16))
    try:
        b = io.BytesIO()
        Image.fromarray(a).save(b, "JPEG", **kw)
        return b.getvalue()
    finally:
        ImageFile.MAXBLOCK = saved


def pil_rgb(d):
    return np.asarray(Image.open(io.BytesIO(d)).convert("RGB"))


def pil_gray(d):
    return D.read_gray_plane(io.BytesIO(d), None)


def content(kind, h=H, w=W, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "texture":
        g = (np.clip(IM.synthetic_pair(3 + seed)["img0"], 0, 1) * 255 + 0.5).astype(np.uint8)
        g = np.pad(g, ((0, max(0, h - g.shape[0])), (0, max(0, w - g.shape[1]))), mode="reflect")[:h, :w]
        tint = rng.integers(0, 60, 3).astype(np.int32)
        return np.clip(g[..., None].astype(np.int32) + tint - 30, 0, 255).astype(np.uint8)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    return np.broadcast_to(rng.integers(0, 256, 3).astype(np.uint8), (h, w, 3)).copy()


def check(files, dec=None, **kw):
    dec = dec or J.JpegDecoder("cuda", **kw)
    gray, st, rgb = dec.decode(files, rgb=True)
    torch.cuda.synchronize()
    gray, st, rgb = gray.cpu().numpy(), st.cpu().numpy(), rgb.cpu().numpy()
    for i, f in enumerate(files):
        assert st[i] == 0, (i, st[i])
        assert np.array_equal(rgb[i], pil_rgb(f)), (i, int((rgb[i] != pil_rgb(f)).sum()))
        assert np.array_equal(gray[i, 0], pil_gray(f)), i
    return gray, dec


@pytest.fixture(scope="module")
def sweep():
    files = []
    for sub in (0, 1, 2):
        for q in (50, 92, 100):
            for opt in (False, True):
                for kind in ("texture", "noise", "flat"):
                    files.append(enc(content(kind, seed=len(files)), quality=q, subsampling=sub, optimize=opt))
    return files


def test_sampling_quality_tables_content_sweep_bit_exact(sweep):
    check(sweep)


@pytest.mark.parametrize("hw", [(1, 1), (5, 7), (33, 17), (17, 33), (721, 541)])
def test_odd_sizes_420(hw):
    h, w = hw
    check([enc(content(k, h, w, seed=i), quality=q, subsampling=2) for i, (k, q) in enumerate((("noise", 92), ("texture", 75), ("flat", 100)))])


def test_single_component_files():
    rng = np.random.default_rng(5)
    files = []
    for q in (50, 92, 100):
        b = io.BytesIO()
        Image.fromarray(rng.integers(0, 256, (H, W), dtype=np.uint8), "L").save(b, "JPEG", quality=q)
        files.append(b.getvalue())
    check(files)


@pytest.mark.parametrize("kw", [dict(restart_marker_blocks=1), dict(restart_marker_blocks=4), dict(restart_marker_blocks=7),
                                dict(restart_marker_rows=1), dict(restart_marker_rows=3)])
def test_restart_markers(kw):
    files = [enc(content(k, seed=i), quality=92, subsampling=s, **kw) for i, (k, s) in enumerate((("texture", 2), ("noise", 0), ("flat", 1)))]
    for f in files:
        st, h, _ = J.parse(f)
        assert st == 0 and h.restart_interval > 0 and h.nseg > 1
    check(files)


def test_entropy_routes_agree_and_resynchronisation_runs(sweep):
    files = sweep[::5]
    g_def, _ = check(files)
    dec32 = J.JpegDecoder("cuda", subseq_bits=32)
    g32, _ = check(files, dec32)
    rounds = dec32.rounds.cpu().numpy()
    big = 8 * max(len(f) for f in files) + 64
    g_seq, dseq = check(files, subseq_bits=big)
    assert np.array_equal(g_def, g32) and np.array_equal(g_def, g_seq)
    assert rounds.max() > 1, rounds
    assert dseq.rounds.cpu().numpy().max() == 1


def test_mixed_batch_of_64_equals_single_decodes():
    rng = np.random.default_rng(9)
    files = []
    for i in range(64):
        kind = ("texture", "noise", "flat")[i % 3]
        kw = dict(quality=int(rng.integers(30, 101)), subsampling=int(rng.integers(0, 3)), optimize=bool(i % 2))
        if i % 7 == 0:
            kw["restart_marker_blocks"] = int(rng.integers(1, 9))
        files.append(enc(content(kind, seed=100 + i), **kw))
    b = io.BytesIO()
    Image.fromarray(content("noise", seed=1)[..., 0], "L").save(b, "JPEG", quality=80)
    files[5] = b.getvalue()
    g_all, dec = check(files)
    for i in (0, 5, 13, 63):
        g1, _ = dec.decode([files[i]])
        assert torch.equal(g1[0].cpu(), torch.from_numpy(g_all[i]))


def _entropy_span(d):
    """(first, end) byte range of the entropy-coded data of a single-scan file"""
    i = d.index(b"\xff\xda")
    first = i + 2 + int.from_bytes(d[i + 2:i + 4], "big")
    return first, d.rindex(b"\xff\xd9")


def test_corrupt_streams_flag_their_image_only():
    good = [enc(content(k, seed=20 + i), quality=92, subsampling=2) for i, k in enumerate(("texture", "noise", "texture", "flat"))]
    a, e = _entropy_span(good[1])
    truncated = good[1][:a + (e - a) // 3] + b"\xff\xd9"                    # the segment ends long before its MCU count
    a, e = _entropy_span(good[2])
    mid = a + (e - a) // 2
    bad_code = good[2][:mid] + b"\xff\x00" * 16 + good[2][mid + 32:]       # 128 one-bits: no Huffman code is all ones
    files = [good[0], truncated, bad_code, good[3]]
    for f in files:
        assert J.parse(f)[0] == 0                                           # well-formed at the marker level: the device must catch it
    gray, st = J.JpegDecoder("cuda").decode(files)
    st = st.cpu().numpy()
    assert st[1] & (J.E_TRUNC | J.E_HUFF) and st[2] & (J.E_TRUNC | J.E_HUFF), st
    assert st[0] == 0 and st[3] == 0
    g = gray.cpu().numpy()
    assert np.array_equal(g[0, 0], pil_gray(good[0])) and np.array_equal(g[3, 0], pil_gray(good[3]))


def test_unsupported_files_are_reported_and_left_untouched():
    a = content("texture", seed=4)
    files = [enc(a, quality=90), enc(a, quality=90, progressive=True)]
    out = torch.full((2, 1, H, W), 7.0, device="cuda")
    gray, st = J.JpegDecoder("cuda").decode(files, out=out)
    st = st.cpu().numpy()
    assert st[0] == 0 and st[1] == J.UNSUPPORTED
    assert bool((gray[1] == 7.0).all())
    assert np.array_equal(gray[0, 0].cpu().numpy(), pil_gray(files[0]))
