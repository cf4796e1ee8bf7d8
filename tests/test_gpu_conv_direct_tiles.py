"""-m gpu: the two pixel tilings of the direct 3x3 convolution (csrc/conv_direct.hip, mfr_conv3x3_direct_f16x2_tiled): tile_mode 1 = the 2-D tile of
8 rows x 32 columns, tile_mode 2 = the LINEAR tile of 256 consecutive units of the image as one padded linear space of pitch Pw >= W + 1.  The K
loop is the same, so every output element sums the same products in the same order: the two outputs must be EQUAL BIT FOR BIT, for every epilogue
(NCHW with / without residual, token-major rows), and the linear tiling must write nothing but the output and raise the range guard for real
pixels only.  Shapes sit where the unit -> pixel mapping can go wrong: one pixel, H Pw = 256 exactly / one more, block boundaries, both plane
strides (448: Pw <= 95, 576: Pw <= 159) and their limits, the 3 x 2 blocking of a 196-channel layer, both pitches of a W % 4 == 0 map."""
import pytest
import torch

from mapfree_reloc_amd import _lib, options
from mapfree_reloc_amd.pipeline import RangeGuard

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E_ARG = -1


def _inputs(B, ci, co, H, W, bias=1, res=0):
    g = torch.Generator().manual_seed(B * 1000 + ci + 7 * H + W)
    x = torch.randn(B, ci, H, W, generator=g).to(DEV)
    w = (torch.randn(co, ci, 3, 3, generator=g) / (3.0 * ci ** 0.5)).to(DEV)
    b = torch.randn(co, generator=g).to(DEV) if bias else None
    r = torch.randn(B, co, H, W, generator=g).to(DEV) if res else None
    return x, w, b, r


def _pack(w):
    lib = _lib.load(require_gpu=True)
    co, ci = int(w.shape[0]), int(w.shape[1])
    u = torch.empty(lib.mfr_conv3x3_direct_f16x2_filter_bytes(ci, co), dtype=torch.uint8, device=w.device)
    _lib.check(lib.mfr_conv3x3_direct_f16x2_filter_pack(_lib.ptr(w), ci, co, _lib.ptr(u), _lib.stream_ptr()), "pack")
    return u


def _launch(x, u, co, b, r, act, y, mode, pitch=0, ldrows=0, pool=0):
    lib = _lib.load(require_gpu=True)
    B, ci, H, W = x.shape
    return lib.mfr_conv3x3_direct_f16x2_tiled(_lib.ptr(x), _lib.ptr(u), _lib.ptr(b), _lib.ptr(r), B, ci, co, H, W, int(act), int(pool), _lib.ptr(y),
                                              int(ldrows), int(mode), int(pitch), _lib.stream_ptr())


def _nchw(x, u, co, b, r, act, mode, pitch=0):
    y = torch.full((x.shape[0], co, x.shape[2], x.shape[3]), float("nan"), dtype=torch.float32, device=DEV)
    _lib.check(_launch(x, u, co, b, r, act, y, mode, pitch), f"tiled mode {mode}")
    return y


@pytest.mark.parametrize("B,ci,co,H,W,act,bias,res,pitch", [
    (1, 16, 128, 1, 1, 0, 1, 0, 0),          # a single pixel
    (2, 8, 128, 5, 2, 1, 1, 0, 0),           # Cin below one K step
    (1, 16, 128, 4, 63, 0, 1, 0, 0),         # H Pw = 256 exactly: one tile
    (1, 16, 128, 5, 63, 1, 1, 1, 0),         # one row more than a tile
    (3, 20, 128, 9, 31, 1, 1, 0, 0),         # block boundaries; B = 3: the number of spatial tiles is no multiple of 8
    (1, 16, 128, 6, 32, 1, 1, 0, 0),
    (1, 16, 128, 6, 33, 0, 1, 1, 0),
    (2, 48, 128, 12, 67, 1, 1, 0, 0),        # three K steps (both stages reused), several tiles
    (1, 64, 128, 5, 135, 1, 1, 0, 0),        # plane stride 576
    (1, 16, 128, 3, 94, 1, 1, 0, 0),         # either side of the 448 limit (Pw = 95 | 96)
    (1, 16, 128, 3, 95, 2, 1, 1, 0),
    (1, 16, 128, 3, 158, 1, 1, 0, 0),        # the widest map
    (1, 16, 160, 9, 33, 1, 1, 0, 0),         # an odd number of 64-channel groups
    (1, 196, 196, 7, 34, 2, 1, 1, 0),        # 3 x 2 blocking of the last channel group, LeakyReLU, residual
    (1, 32, 256, 6, 68, 1, 1, 1, 69),        # W % 4 == 0 at pitch W + 1 (4-byte stores) ...
    (1, 32, 256, 6, 68, 1, 1, 1, 72),        # ... and at W + 4 (rows stay 16-byte aligned: the LDS-exchange store path)
    (2, 128, 256, 90, 67, 1, 1, 0, 0)])      # the bench shape (SuperPoint convPa)
def test_linear_tiling_equals_2d_tiling_bitwise(B, ci, co, H, W, act, bias, res, pitch):
    x, w, b, r = _inputs(B, ci, co, H, W, bias, res)
    u = _pack(w)
    y_rows, y_lin = _nchw(x, u, co, b, r, act, 1), _nchw(x, u, co, b, r, act, 2, pitch)
    assert torch.isfinite(y_rows).all() and torch.isfinite(y_lin).all()          # every element written (the outputs were NaN)
    assert torch.equal(y_rows, y_lin)


@pytest.mark.parametrize("B,ci,co,H,W,act", [(1, 16, 128, 8, 67, 1), (1, 64, 128, 8, 67, 0), (2, 128, 256, 12, 67, 1)])
def test_linear_tiling_rows_output_equals_2d_rows_output_bitwise(B, ci, co, H, W, act):
    """token-major output (convDa's): ld = Cout, and ld > Cout where the columns beyond Cout must stay untouched"""
    x, w, b, _ = _inputs(B, ci, co, H, W)
    u = _pack(w)
    for ld in (co, co + 8):
        ys = []
        for mode in (1, 2):
            y = torch.full((B, H, W, ld), 7.0, dtype=torch.float32, device=DEV)
            y[..., :co] = float("nan")
            _lib.check(_launch(x, u, co, b, None, act, y, mode, 0, ldrows=ld), f"rows mode {mode}")
            ys.append(y)
        assert torch.isfinite(ys[1]).all() and (ys[1][..., co:] == 7.0).all()
        assert torch.equal(ys[0], ys[1])
    assert torch.equal(ys[1][..., :co].permute(0, 3, 1, 2), _nchw(x, u, co, b, None, act, 2))


@pytest.mark.parametrize("B,ci,co,H,W,ld", [(1, 16, 128, 5, 63, 0), (2, 16, 196, 9, 33, 0), (1, 16, 128, 5, 63, 128), (1, 16, 128, 6, 68, 0)])
def test_linear_tiling_writes_nothing_outside_the_output(B, ci, co, H, W, ld):
    """y inside a larger sentinel-filled buffer, one guard band in front and one behind; (1,16,128,5,63): the last tile overhangs the image by 192 of its
    256 units; 196 channels: the last channel group has 60 channels that do not exist"""
    x, w, b, _ = _inputs(B, ci, co, H, W)
    u = _pack(w)
    n, band = B * H * W * (ld or co), 1 << 16
    for mode in (1, 2):
        buf = torch.full((n + 2 * band,), -123.0, dtype=torch.float32, device=DEV)
        y = buf[band:band + n]
        _lib.check(_launch(x, u, co, b, None, 1, y, mode, 0, ldrows=ld), f"mode {mode}")
        assert (buf[:band] == -123.0).all() and (buf[band + n:] == -123.0).all(), mode
        assert (y != -123.0).all(), mode


def test_linear_mode_rejects_what_it_does_not_cover():
    """mode 2 with pooling, with Cout <= 64, beyond the widest instantiation or with a pitch that does not fit: MFR_E_ARG and nothing written"""
    for (ci, co, H, W, pool, pitch) in ((16, 128, 8, 40, 1, 0), (16, 64, 8, 40, 0, 0), (16, 128, 3, 159, 0, 0), (16, 128, 3, 40, 0, 40), (16, 128, 3, 40, 0, 160)):
        x, w, b, _ = _inputs(1, ci, co, H, W)
        u = _pack(w)
        y = torch.full((1, co, H, W), -5.0, dtype=torch.float32, device=DEV)
        assert _launch(x, u, co, b, None, 1, y, 2, pitch, pool=pool) == E_ARG, (ci, co, H, W, pool, pitch)
        torch.cuda.synchronize()
        assert (y == -5.0).all()
    x, w, b, _ = _inputs(1, 16, 128, 8, 40)
    y = torch.empty((1, 128, 8, 40), dtype=torch.float32, device=DEV)
    assert _launch(x, _pack(w), 128, b, None, 1, y, 3) == E_ARG                  # unknown mode
    # the same shapes are fine in the 2-D tiling (and 'auto' never fails where the 2-D tile exists)
    x, w, b, _ = _inputs(1, 16, 128, 3, 159)
    for mode in (0, 1):
        assert torch.isfinite(_nchw(x, _pack(w), 128, b, None, 1, mode)).all()


def test_linear_tiling_range_guard_sees_real_pixels_only():
    """The guard tests ACCUMULATORS (csrc/guard.h).  A discarded position of the linear space (x >= W) sums the right border of row y and the left
    border of row y + 1 -- twice the neighbours any output has on that side.  Every input element's own pixel is a real output, so an out-of-range
    or non-finite ELEMENT raises the flag in either tiling; what only a discarded position could see is a SUM of in-range values, and an fp32
    accumulator cannot overflow from at most 9 Cin products of an f16 value (<= 65504) with an f16 weight term (65504^2 * 9 * 2^16 < 3e15 << 3.4e38).
    So: (i) the largest in-range values on both sides of every discarded column (x = W - 1 and x = 0 of all rows and channels) leave the flag clear,
    the output finite and bitwise the 2-D tiling's; (ii) one out-of-range value at a real pixel -- first, last, next to a discarded column, in the
    last tile -- sets it; with the flag checked through the helper of tests/test_gpu_range_guard.py (pipeline.RangeGuard)."""
    options.reset()
    guard = RangeGuard(torch.device(DEV), lambda: None)
    assert guard.active
    B, ci, co, H, W = 2, 32, 128, 12, 67
    x, w, b, _ = _inputs(B, ci, co, H, W)
    u = _pack(w)

    def fires(xx, mode):
        with guard:
            y = _nchw(xx, u, co, b, None, 1, mode)
        torch.cuda.synchronize()
        return int(guard.flag.item()) != 0, y

    xe = x.clone(); xe[:, :, :, W - 1] = 6.0e4; xe[:, :, :, 0] = -6.0e4; xe[:, ::2, :, 0] = 6.0e4
    (f1, y1), (f2, y2) = fires(xe, 1), fires(xe, 2)
    assert not f1 and not f2 and torch.isfinite(y2).all() and torch.equal(y1, y2)
    for pos in ((0, 0, 0, 0), (B - 1, ci - 1, H - 1, W - 1), (1, 5, 3, W - 1), (0, 7, 4, 0), (1, 0, H - 1, 0)):
        for bad in (7.0e4, float("inf"), float("nan")):
            xb = x.clone(); xb[pos] = bad
            assert fires(xb, 2)[0], (pos, bad)
    assert not fires(x, 2)[0]


def test_conv_tile_option_reaches_the_kernel():
    """HIP.CONV_TILE through nets/conv.py: 'rows' and 'linear' give the bits of 'auto' on a layer with the linear geometry (NCHW and rows output) and on
    one without it (pooled: 'linear' means linear wherever it exists)"""
    from mapfree_reloc_amd.nets.conv import DirectConv3x3
    x, w, b, _ = _inputs(2, 32, 128, 20, 67)
    conv = DirectConv3x3(w, b)
    try:
        want, want_rows, want_pool = conv(x, act=1), conv.rows(x, act=1), conv(x, act=1, pool=True)
        for tile in ("rows", "linear"):
            options.set("CONV_TILE", tile)
            assert torch.equal(conv(x, act=1), want) and torch.equal(conv.rows(x, act=1), want_rows) and torch.equal(conv(x, act=1, pool=True), want_pool)
    finally:
        options.reset()
