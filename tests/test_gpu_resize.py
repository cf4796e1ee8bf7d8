"""-m gpu: the device image resize (csrc/resize.hip, mfr_resize_gray_bilinear) equals datasets.gray_plane(rgb, (w, h)) on EVERY element --
integer luma, OpenCV-style bilinear taps of the float plane with each product and sum rounded to float32, / 255 -- and
JpegDecoder.decode(files, resize=(w, h)) equals datasets.read_gray_plane(path, (w, h))."""
import io

import numpy as np
import pytest
import torch

from mapfree_reloc_amd import datasets as D, jpeg_ops as J

pytestmark = pytest.mark.gpu

# (H, W) -> (h, w): down, up, one pixel, odd sizes with separate factors, the identity, ScanNet's ratios (2.0167, 2.025), ScanNet itself
SHAPES = [((5, 7), (3, 4)), ((3, 4), (5, 7)), ((1, 1), (4, 4)), ((33, 17), (16, 9)), ((17, 33), (17, 33)), ((484, 648), (240, 320)),
          ((968, 1296), (480, 640))]


def _batch(H, W, seed):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.integers(0, 256, size=(2, H, W, 3), dtype=np.uint8), np.zeros((1, H, W, 3), np.uint8),
                           np.full((1, H, W, 3), 255, np.uint8)])


@pytest.fixture(scope="module")
def resizer():
    return J.GrayResizer("cuda")


@pytest.mark.parametrize("src,dst", SHAPES, ids=[f"{a[0]}x{a[1]}-{b[0]}x{b[1]}" for a, b in SHAPES])
def test_resize_equals_gray_plane(resizer, src, dst):
    (H, W), (h, w) = src, dst
    rgb = _batch(H, W, 31 * H + W)
    want = torch.from_numpy(np.stack([D.gray_plane(im, (w, h)) for im in rgb]))[:, None]
    out = torch.full((len(rgb), 1, h, w), -1.0, device="cuda")
    resizer(torch.from_numpy(rgb).cuda(), out)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), want)
    assert float(out[2].abs().max()) == 0.0                     # (an all-255 image need not give exactly 1: 255 (1 - f) + 255 f rounds twice, on the host too)
    if src == dst:                                              # the identity reproduces byte / 255
        assert torch.equal(out.cpu()[:, 0], torch.from_numpy(D.luma_u8(rgb).astype(np.float32) / np.float32(255)))


def test_rows_with_a_status_are_left_untouched(resizer):
    rgb = _batch(33, 17, 3)
    out = torch.full((4, 1, 16, 9), -7.0, device="cuda")
    status = torch.tensor([0, 1, 0x20, 0], dtype=torch.int32, device="cuda")
    resizer(torch.from_numpy(rgb).cuda(), out, status)
    torch.cuda.synchronize()
    got = out.cpu()
    assert bool((got[1] == -7.0).all()) and bool((got[2] == -7.0).all())
    for r in (0, 3):
        assert torch.equal(got[r, 0], torch.from_numpy(D.gray_plane(rgb[r], (9, 16))))


def test_bad_sizes_are_refused(resizer):
    from mapfree_reloc_amd import _lib
    lib = _lib.load(require_gpu=True)
    z = torch.zeros(16, dtype=torch.int32, device="cuda")
    f = torch.zeros(16, device="cuda")
    rgb = torch.zeros(1, 2, 2, 3, dtype=torch.uint8, device="cuda")
    for H, W, h, w in ((0, 2, 2, 2), (2, 2, 0, 2), (2, 2, 2, -1)):
        rc = lib.mfr_resize_gray_bilinear(rgb.data_ptr(), 1, H, W, None, z.data_ptr(), z.data_ptr(), f.data_ptr(), z.data_ptr(), z.data_ptr(),
                                          f.data_ptr(), h, w, f.data_ptr(), None)
        assert rc == -1


def _jpeg(H, W, subsampling, seed, tmp_path):
    from PIL import Image
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    im = np.clip(np.stack([3 * xx + yy, 255 - 2 * yy, 2 * xx + 3 * yy], -1) % 256 + rng.integers(-20, 20, (H, W, 3)), 0, 255).astype(np.uint8)
    path = tmp_path / f"f_{H}x{W}_{subsampling}_{seed}.jpg"
    Image.fromarray(im).save(path, format="JPEG", quality=90, subsampling=subsampling)
    return path


@pytest.mark.parametrize("subsampling", [2, 0], ids=["420", "444"])
def test_decoder_resize_equals_read_gray_plane(tmp_path, subsampling):
    H, W, w, h = 97, 131, 64, 47                                # odd file size (partial MCUs), separate factors
    paths = [_jpeg(H, W, subsampling, 1, tmp_path), _jpeg(H, W, subsampling, 2, tmp_path)]
    files = [p.read_bytes() for p in paths]
    dec = J.JpegDecoder("cuda")
    out, status = dec.decode(files, resize=(w, h))
    torch.cuda.synchronize()
    assert out.shape == (2, 1, h, w) and status.tolist() == [0, 0]
    for k, p in enumerate(paths):
        assert torch.equal(out[k, 0].cpu(), torch.from_numpy(D.read_gray_plane(str(p), (w, h))))
    up, st, rgb = dec.decode(files, resize=(2 * W + 1, H), rgb=True)          # an upscale along x only; the RGB stays at the file's size
    assert rgb.shape == (2, H, W, 3) and torch.equal(up[0, 0].cpu(), torch.from_numpy(D.read_gray_plane(str(paths[0]), (2 * W + 1, H))))
    plain, st0 = dec.decode(files)                                            # resize=None: the decoder's plane, as before
    same, _ = dec.decode(files, resize=(W, H))                                # the files' own size is no resize
    assert plain.shape == (2, 1, H, W) and torch.equal(plain, same)
    for k, p in enumerate(paths):
        assert torch.equal(plain[k, 0].cpu(), torch.from_numpy(D.read_gray_plane(str(p), None)))


def test_decoder_resize_skips_files_the_device_does_not_take(tmp_path):
    from PIL import Image
    p0 = _jpeg(40, 56, 2, 5, tmp_path)
    p1 = tmp_path / "progressive.jpg"
    Image.open(p0).save(p1, format="JPEG", progressive=True)
    out = torch.full((2, 1, 20, 30), -3.0, device="cuda")
    _, status = J.JpegDecoder("cuda").decode([p0.read_bytes(), p1.read_bytes()], out=out, resize=(30, 20))
    torch.cuda.synchronize()
    assert status.tolist() == [J.OK, J.UNSUPPORTED] and bool((out[1] == -3.0).all())
    assert torch.equal(out[0, 0].cpu(), torch.from_numpy(D.read_gray_plane(str(p0), (30, 20))))
