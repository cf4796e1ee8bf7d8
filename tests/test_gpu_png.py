"""-m gpu: the device depth PNG decoder (csrc/png.hip, png_ops.DepthPngDecoder) against datasets.read_depth_plane of the same file, bit for bit,
with exact statuses, on files written by tests/png_craft.py: every deflate block type and zlib strategy, tiny dynamic blocks, flushes, split
IDATs, every filter type, far and overlapping matches, every sample value, batches with bad rows, and hand-made malformed streams.  The
shapes are the smallest that reach each mechanism: 37 x 53 (odd, no multiple of 64, one unfilter pass), 300 x 1 (five passes), 128 x 160
(a 32 742-byte match distance)."""
import glob
import io
import os
import sys
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

import mapfree_reloc_amd  # noqa: F401
from mapfree_reloc_amd import datasets as D, png_ops as P

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_craft as PC  # noqa: E402
from png_cases import MODES, VARIANTS, content, malformed_streams, periodic, small_raw, SMALL_H, SMALL_W  # noqa: E402

pytestmark = pytest.mark.gpu

H, W = 37, 53


@pytest.fixture(scope="module")
def dec():
    return P.DepthPngDecoder("cuda")


def ref(f):
    return D.read_depth_plane(io.BytesIO(f))


def check(dec, files):
    """one batch: every status 0 and every plane equal to the host's"""
    out, st = dec.decode(files)
    torch.cuda.synchronize()
    st = st.cpu().numpy()
    assert st.tolist() == [0] * len(files), [hex(int(s)) for s in st]
    o = out.cpu().numpy()
    for i, f in enumerate(files):
        assert np.array_equal(o[i], ref(f)), i
    return o


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_deflate_modes(dec, variant):
    a = content(H, W, 1)
    files = [PC.write_png(a, **dict(MODES[m], **VARIANTS[variant](H * (1 + 2 * W)))) for m in sorted(MODES)]
    assert all(P.parse(f)[0] == P.OK for f in files)
    check(dec, files)


def test_filters(dec):
    a = content(H, W, 2)
    rng = np.random.default_rng(5)
    files = [PC.write_png(a, filters=[t] * H) for t in range(5)]
    files.append(PC.write_png(a, filters=rng.integers(0, 5, H).tolist()))
    edge = a.copy()
    edge[0::3] = 0
    edge[1::3] = 65535                                                   # every predictor wraps around a byte
    files += [PC.write_png(edge, filters=[t] * H) for t in range(5)] + [PC.write_png(edge, filters=rng.integers(0, 5, H).tolist())]
    check(dec, files)


@pytest.mark.parametrize("h,w", [(1, 1), (1, 300), (300, 1)])
def test_sizes(dec, h, w):
    check(dec, [PC.write_png(content(h, w, 3)), PC.write_png(content(h, w, 4), filters=[4 - y % 5 for y in range(h)], level=9)])


def test_every_value(dec):
    a = np.arange(65536, dtype=np.uint16).reshape(256, 256)
    o = check(dec, [PC.write_png(a), PC.write_png(a.T.copy(), level=1)])
    assert np.array_equal(np.sort(o[0].ravel()), D._luts()[1])


def test_window(dec):
    """zlib's own encoder never looks further back than 32 768 - 262 bytes, so it cannot shrink this image (asserted); the stream with the
    32 742-byte distances is written by hand: the first period stored, the rest as matches of up to 258 bytes into it"""
    h, w, period = 128, 160, 102
    rows = np.random.default_rng(7).integers(0, 65536, (period, w), dtype=np.uint16)
    a = rows[np.arange(h) % period]
    raw = PC.filter_rows(a, [0] * h)
    dist = (1 + 2 * w) * period
    assert dist == 32742 and len(PC.deflate(raw, level=9)) > 0.99 * len(raw)
    bw = PC.stored_block(PC.BitWriter(), raw[:dist], final=False)
    rest = len(raw) - dist
    PC.fixed_block(bw, [(min(258, rest - i), dist) for i in range(0, rest, 258)])
    stream = PC.zlib_wrap(bw.bytes(), raw)
    assert zlib.decompress(stream) == raw and len(stream) < 0.9 * len(raw)   # only matches 32 742 bytes back can shrink it
    check(dec, [PC.assemble(w, h, stream), PC.write_png(a, filters=[0] * h, level=9)])


def test_overlapping_copies(dec):
    files = []
    for kw in (dict(strategy=zlib.Z_RLE), dict(level=9)):
        files.append(PC.write_png(np.full((H, W), 0x1234, np.uint16), filters=[0] * H, **kw))
        files += [PC.write_png(periodic(H, W, p), filters=[0] * H, **kw) for p in (2, 3, 7)]
    check(dec, files)


def test_batch_with_bad_rows(dec):
    good = [PC.write_png(content(H, W, 10 + i), level=(0, 1, 6, 9, 6)[i]) for i in range(5)]
    b = io.BytesIO()
    Image.fromarray(np.zeros((H, W), np.uint8)).save(b, format="PNG")
    stream = PC.deflate(PC.filter_rows(content(H, W, 20), [y % 5 for y in range(H)]))
    cut = PC.assemble(W, H, stream[:len(stream) // 3])
    flipped = PC.assemble(W, H, stream[:-2] + bytes([stream[-2] ^ 0x40]) + stream[-1:])
    other = PC.write_png(content(H + 1, W, 21))
    files = [good[0], b.getvalue(), good[1], cut, good[2], flipped, other, good[3], good[4]]
    want = [0, P.UNSUPPORTED, 0, P.E_TRUNC, 0, P.E_CHECK, P.E_SIZE, 0, 0]
    out = torch.full((9, H, W), -7.0, dtype=torch.float32, device="cuda")
    out, st = dec.decode(P.pack(files, H, W), out=out)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == want
    o = out.cpu().numpy()
    for i, f in enumerate(files):
        assert np.array_equal(o[i], ref(f) if want[i] == 0 else np.full((H, W), -7.0, np.float32)), i


def test_hand_made_valid_stream(dec):
    """the bit-writer's own blocks: an empty stored block, a fixed block with an overlapping match, a dynamic block whose match reaches back
    into the block before it"""
    raw, stream = small_raw()
    assert zlib.decompress(stream) == raw
    check(dec, [PC.assemble(SMALL_W, SMALL_H, stream)])


@pytest.mark.parametrize("case", sorted(malformed_streams()))
def test_malformed_stream(dec, case):
    stream, want = malformed_streams()[case]
    good = PC.write_png(content(SMALL_H, SMALL_W, 30))
    files = [PC.assemble(SMALL_W, SMALL_H, stream), good]
    assert P.parse(files[0])[0] == P.OK
    out = torch.full((2, SMALL_H, SMALL_W), -7.0, dtype=torch.float32, device="cuda")
    out, st = dec.decode(files, out=out)
    torch.cuda.synchronize()
    assert [hex(s) for s in st.cpu().tolist()] == [hex(getattr(P, want)), "0x0"]
    o = out.cpu().numpy()
    assert np.all(o[0] == -7.0) and np.array_equal(o[1], ref(good))


def test_workload_shape(dec, tmp_path):
    from tools.bench_fused_split import write_scene
    for s in range(2):
        write_scene((str(tmp_path), s, 3))
    files = [open(p, "rb").read() for p in sorted(glob.glob(os.path.join(str(tmp_path), "test", "*", "*", "*.png")))]
    assert len(files) == 8
    o = check(dec, files)
    assert o.shape == (8, 720, 540)
