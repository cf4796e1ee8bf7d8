"""A PNG writer that takes everything as given, for the depth PNG decoder's tests (png_ops, csrc/png.hip, csrc/host_decode.c): the samples,
the filter type of every row (applied here), the zlib.compressobj parameters, flush points, the IDAT split and extra chunks; plus a small
deflate bit-writer (RFC 1951) for hand-made streams, valid and malformed.  Nothing here reads the code under test."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"


def chunk(ctype, data=b""):
    return struct.pack(">I", len(data)) + ctype + data + struct.pack(">I", zlib.crc32(ctype + data) & 0xFFFFFFFF)


def ihdr(width, height, bit_depth=16, color_type=0, interlace=0):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, bit_depth, color_type, 0, 0, interlace))


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else b if pb <= pc else c


def filter_rows(arr, filters, bpp=2):
    """arr u16 [H, W] (or u8 rows [H, n] with bpp given) -> the filtered scanlines, filter byte first; filters[y] in 0..4"""
    rows = arr.astype(">u2").view(np.uint8).reshape(arr.shape[0], -1) if arr.dtype != np.uint8 else arr
    H, n = rows.shape
    out = bytearray()
    prev = np.zeros(n, np.int32)
    for y in range(H):
        cur = rows[y].astype(np.int32)
        ft = int(filters[y])
        a = np.concatenate([np.zeros(bpp, np.int32), cur[:-bpp]]) if n > bpp else np.zeros(n, np.int32)
        c = np.concatenate([np.zeros(bpp, np.int32), prev[:-bpp]]) if n > bpp else np.zeros(n, np.int32)
        if ft == 0:
            pred = np.zeros(n, np.int32)
        elif ft == 1:
            pred = a
        elif ft == 2:
            pred = prev
        elif ft == 3:
            pred = (a + prev) >> 1
        elif ft == 4:
            pred = np.array([_paeth(int(a[i]), int(prev[i]), int(c[i])) for i in range(n)], np.int32)
        else:
            pred = np.zeros(n, np.int32)                        # an illegal type: the bytes go out as they are
        out.append(ft)
        out += ((cur - pred) & 255).astype(np.uint8).tobytes()
        prev = cur
    return bytes(out)


def deflate(raw, level=6, wbits=15, memLevel=8, strategy=zlib.Z_DEFAULT_STRATEGY, flush=()):
    """zlib stream of raw.  flush: [(byte offset into raw, zlib.Z_SYNC_FLUSH | Z_FULL_FLUSH), ...] in rising order"""
    co = zlib.compressobj(level, zlib.DEFLATED, wbits, memLevel, strategy)
    out, at = b"", 0
    for off, mode in flush:
        out += co.compress(raw[at:off]) + co.flush(mode)
        at = off
    return out + co.compress(raw[at:]) + co.flush()


def assemble(width, height, stream, idat=None, extra=(), bit_depth=16, color_type=0, interlace=0, end=True):
    """the file around a zlib stream.  idat: split size of the IDAT chunks (None: one chunk).  extra: [(where, chunk bytes)], where =
    'head' (after IHDR), 'tail' (after the IDATs) or an int k (between IDAT k - 1 and IDAT k)"""
    parts = [stream] if not idat else [stream[i:i + idat] for i in range(0, max(len(stream), 1), idat)]
    f = SIGNATURE + ihdr(width, height, bit_depth, color_type, interlace)
    f += b"".join(c for w, c in extra if w == "head")
    for k, p in enumerate(parts):
        f += b"".join(c for w, c in extra if w == k and k > 0)
        f += chunk(b"IDAT", p)
    f += b"".join(c for w, c in extra if w == "tail")
    return f + (chunk(b"IEND") if end else b"")


def write_png(arr, filters=None, idat=None, extra=(), **deflate_args):
    """arr u16 [H, W] -> file bytes.  filters: per-row types (default: 0..4 cycling)"""
    arr = np.asarray(arr, dtype=np.uint16)
    H, W = arr.shape
    filters = [y % 5 for y in range(H)] if filters is None else filters
    return assemble(W, H, deflate(filter_rows(arr, filters), **deflate_args), idat, extra)


# --------------------------------------------------------------------------------------------------------------------------------
# deflate by hand

class BitWriter:
    """RFC 1951 bit order: data elements LSB first, Huffman codes MSB first"""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, v, n):
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8
        return self

    def code(self, c, n):
        return self.bits(int(format(c, "0%db" % n)[::-1], 2), n) if n else self

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)
        return self

    def raw(self, b):
        assert self.n == 0
        self.out += b
        return self

    def bytes(self):
        return bytes(self.align().out)


def canonical(lens):
    """code of every symbol with a non-zero length (RFC 1951 3.2.2); over-subscribed sets are numbered all the same"""
    codes, code = {}, 0
    for l in range(1, max(lens) + 1 if max(lens) else 1):
        for s, sl in enumerate(lens):
            if sl == l:
                codes[s] = (code, l)
                code += 1
        code <<= 1
    return codes


FIXED_LL = canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)


def put_match(bw, ll, dd, length, dist):
    ls = max(i for i in range(29) if LEN_BASE[i] <= length and (i < 28 or length == 258))
    bw.code(*ll[257 + ls]).bits(length - LEN_BASE[ls], LEN_EXTRA[ls])
    ds = max(i for i in range(30) if DIST_BASE[i] <= dist)
    bw.code(*dd[ds]).bits(dist - DIST_BASE[ds], DIST_EXTRA[ds])


def fixed_block(bw, items, final=True, end=True):
    """items: ints (literals), (length, dist) matches, or ('ll', symbol) / ('d', code) raw codes"""
    dd = {i: (i, 5) for i in range(32)}
    bw.bits(1 if final else 0, 1).bits(1, 2)
    for it in items:
        if isinstance(it, int):
            bw.code(*FIXED_LL[it])
        elif it[0] == "ll":
            bw.code(*FIXED_LL[it[1]])
        elif it[0] == "d":
            bw.code(*dd[it[1]])
        else:
            put_match(bw, FIXED_LL, dd, *it)
    if end:
        bw.code(*FIXED_LL[256])
    return bw


def dynamic_header(bw, cl_lens, cl_syms, hlit, hdist, final=True, hclen=19):
    """BFINAL, BTYPE 2, HLIT / HDIST / HCLEN as given (the field values: counts minus 257 / 1 / 4 are taken here), the code-length code's
    lengths cl_lens [19] and the sequence cl_syms of (code-length symbol, extra value)"""
    bw.bits(1 if final else 0, 1).bits(2, 2).bits(hlit - 257, 5).bits(hdist - 1, 5).bits(hclen - 4, 4)
    for s in CL_ORDER[:hclen]:
        bw.bits(cl_lens[s], 3)
    cc = canonical(list(cl_lens))
    for s, ex in cl_syms:
        bw.code(*cc[s])
        if s >= 16:
            bw.bits(ex, {16: 2, 17: 3, 18: 7}[s])
    return bw


def dynamic_block(bw, ll_lens, d_lens, items, final=True, end=True):
    """a dynamic block whose code lengths are sent one by one, without repeat codes (the code-length code: symbols 0..15 at 4 bits each);
    items as in fixed_block, plus ('bits', value, n) for raw bits"""
    cl_lens = [4] * 16 + [0, 0, 0]
    dynamic_header(bw, cl_lens, [(l, 0) for l in list(ll_lens) + list(d_lens)], len(ll_lens), len(d_lens), final)
    ll, dd = canonical(list(ll_lens)), canonical(list(d_lens))
    for it in items:
        if isinstance(it, int):
            bw.code(*ll[it])
        elif it[0] == "ll":
            bw.code(*ll[it[1]])
        elif it[0] == "d":
            bw.code(*dd[it[1]])
        elif it[0] == "bits":
            bw.bits(it[1], it[2])
        else:
            put_match(bw, ll, dd, *it)
    if end:
        bw.code(*ll[256])
    return bw


def stored_block(bw, data, final=True, nlen=None):
    bw.bits(1 if final else 0, 1).bits(0, 2).align()
    bw.raw(struct.pack("<HH", len(data), (len(data) ^ 0xFFFF) if nlen is None else nlen) + data)
    return bw


def zlib_wrap(deflate_bytes, raw, cmf=0x78, flg=None):
    """2-byte header + the deflate data + Adler-32 of raw"""
    flg = (31 - (cmf << 8) % 31) % 31 if flg is None else flg
    return bytes([cmf, flg]) + deflate_bytes + struct.pack(">I", zlib.adler32(raw) & 0xFFFFFFFF)
