"""The depth PNG decoder's shared test cases (tests/test_png_host.py on the CPU, tests/test_gpu_png.py on the device): image content, the
zlib parameter sets, and hand-made deflate streams from tests/png_craft.py -- one valid, and one malformed stream per way RFC 1951 data can be
invalid, each with the status the device must report."""
import zlib

import numpy as np

import png_craft as PC

MODES = {"stored": dict(level=0), "fixed": dict(strategy=zlib.Z_FIXED), "huffman-only": dict(strategy=zlib.Z_HUFFMAN_ONLY),
         "rle": dict(strategy=zlib.Z_RLE), "level9": dict(level=9), "wbits9": dict(wbits=9)}
# raw length -> extra writer arguments
VARIANTS = {"plain": lambda n: {},
            "memlevel1": lambda n: dict(memLevel=1),                     # a new dynamic block every <= 127 symbols
            "flushes": lambda n: dict(flush=[(n // 3, zlib.Z_SYNC_FLUSH), (2 * n // 3, zlib.Z_FULL_FLUSH)]),
            "idat17": lambda n: dict(idat=17)}

SMALL_H, SMALL_W = 2, 3                                                  # the hand-made streams' image: 2 rows of 1 + 6 bytes


def content(h, w, seed):
    """a depth-like plane: a smooth ramp, noise in the low bits, a few rows of 0 and of 65 535"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    a = (900 + 37 * y + 11 * x + rng.integers(0, 6, (h, w))).astype(np.uint16)
    a[rng.random((h, w)) < 0.05] = 0
    if h > 4:
        a[2] = 0
        a[h - 2] = 65535
    return a


def periodic(h, w, p):
    """sample bytes of period p"""
    b = ((np.arange(2 * h * w) % p) * 37 + 1).astype(np.uint8)
    return b.view(">u2").reshape(h, w).astype(np.uint16)


def small_rows(a=0x12, b=0x34):
    return bytes([0, a, b, a, b, a, b] * 2)


# literals 0..253 at 8 bits, 254, 255, end-of-block and length code 257 at 9: a complete code
LL_SMALL = [8] * 254 + [9] * 4


def small_raw():
    """(raw scanlines, zlib stream) of a SMALL_H x SMALL_W image in three blocks: stored and empty; fixed, with a match whose distance (2) is
    below its length (4); dynamic, with one match (length 7, distance 7) that reaches back into the block before it"""
    raw = small_rows()
    bw = PC.BitWriter()
    PC.stored_block(bw, b"", final=False)
    PC.fixed_block(bw, [0, 0x12, 0x34, (4, 2)], final=False)
    PC.dynamic_block(bw, [0] * 256 + [1, 0, 0, 0, 0, 1], [0, 0, 0, 0, 0, 1], [(7, 7)], final=True)
    return raw, PC.zlib_wrap(bw.bytes(), raw)


def malformed_streams():
    """name -> (zlib stream, the png_ops status name the device must give)"""
    raw = small_rows()
    z = lambda bw: PC.zlib_wrap(bw.bytes() + bytes(8), raw)
    B = PC.BitWriter
    cl16 = [4] * 16 + [0, 0, 0]
    c = {}
    c["distance_before_start"] = z(PC.fixed_block(B(), [0, (3, 5)] + list(raw[4:])))
    c["fixed_length_code_286"] = z(PC.fixed_block(B(), [0, ("ll", 286)]))
    c["fixed_distance_code_30"] = z(PC.fixed_block(B(), [0, ("ll", 257), ("d", 30)]))
    c["unassigned_distance_code"] = z(PC.dynamic_block(B(), LL_SMALL, [1], [0, ("ll", 257), ("bits", 1, 1)]))
    c["block_type_3"] = z(B().bits(1, 1).bits(3, 2))
    c["stored_len_nlen"] = z(PC.stored_block(B(), raw, nlen=len(raw)))
    c["hlit_287"] = z(PC.dynamic_header(B(), cl16, [], 287, 1))
    c["hdist_31"] = z(PC.dynamic_header(B(), cl16, [], 257, 31))
    c["repeat_without_predecessor"] = z(PC.dynamic_header(B(), [4] * 15 + [0, 4, 0, 0], [(16, 0)], 257, 1))
    c["repeat_overruns"] = z(PC.dynamic_header(B(), [1] * 1 + [0] * 17 + [1], [(18, 127), (18, 127)], 257, 1))
    c["no_end_of_block_code"] = z(PC.dynamic_block(B(), [8] * 256 + [0], [1], [0], end=False))
    c["oversubscribed"] = z(PC.dynamic_block(B(), [1, 1, 1] + [0] * 253 + [2], [1], [], end=False))
    c["incomplete"] = z(PC.dynamic_block(B(), [0] * 256 + [2, 2], [1], [], end=False))
    c["incomplete_code_length_code"] = z(PC.dynamic_header(B(), [2, 2] + [0] * 17, [(0, 0)] * 258, 257, 1))
    out = {k: (v, "E_DATA") for k, v in c.items()}
    bad_filter = bytes([5]) + raw[1:]
    out["filter_type_5"] = (zlib.compress(bad_filter), "E_DATA")
    out["longer_than_the_image"] = (zlib.compress(raw + b"\0"), "E_SIZE")
    out["shorter_than_the_image"] = (zlib.compress(raw[:-1]), "E_SIZE")
    out["no_adler"] = (zlib.compress(raw)[:-4], "E_TRUNC")
    return out
