"""A baseline JPEG writer for the tests, from ITU-T T.81 (B.1-B.2 markers and headers, C canonical Huffman codes, F.1.2 entropy coding).
It takes QUANTISED COEFFICIENTS, not pixels (there is no forward DCT), and every table and marker as the caller gives them, so a test
decides exactly what the decoder sees: tables no encoder library emits (fixed-length codes, codes of 10-16 bits, 16-bit quantisation
tables, ids 2 / 3), any component ids and APPn segments, fill bytes, zero-bit padding, coefficients no pixel block produces.

corpus(height, width) is the set of files the JPEG tests share: each Case carries the class the file belongs to (SUPPORTED: the parse must
take it; UNSUPPORTED: PIL decodes it, the parse must hand it to the host; BROKEN: PIL refuses it, the parse must call it invalid).
Test infrastructure only: plain Python + numpy, slow."""
import collections

import numpy as np

DC_SYMBOLS = list(range(12))                                                     # magnitude categories 0..11 (8-bit precision)
AC_SYMBOLS = [0x00, 0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 11)]
COEF_BOUND = 4096    # sum_k |coef_k q_k| per block up to which the project promises PIL's bits (jpeg_ops.py's docstring)

JFIF = b"\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"


def segment(marker, payload):
    """one marker segment: FF, marker, 16-bit length, payload"""
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def adobe(transform):
    return segment(0xEE, b"Adobe\x00\x64\x00\x00\x00\x00" + bytes([transform]))


# ---- Huffman tables: (BITS[16], HUFFVAL) ----------------------------------------------------------------------------------------------

def table_from_lengths(sym_len):
    """{symbol: code length} -> (BITS, HUFFVAL); the caller keeps sum 2^-length <= 1"""
    bits, vals = [0] * 16, []
    for l in range(1, 17):
        ss = sorted(s for s, ll in sym_len.items() if ll == l)
        bits[l - 1] = len(ss)
        vals += ss
    return bits, vals


def canonical_codes(bits, vals):
    """BITS / HUFFVAL -> {symbol: (code, length)} (T.81 C.2)"""
    out, code, k = {}, 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            out[vals[k]] = (code, l)
            code += 1
            k += 1
        code <<= 1
    return out


def flat_dc():
    """every DC symbol 4 bits: a fixed-length code never resynchronises by itself"""
    return table_from_lengths({s: 4 for s in DC_SYMBOLS})


def flat_ac():
    return table_from_lengths({s: 8 for s in AC_SYMBOLS})


def staircase(symbols, seed, first=1):
    """lengths first, first + 1, ... 16 in a seeded shuffle of `symbols`, each symbol as short as leaves a 16-bit code for every later one,
    the remaining symbols at 16 bits, and the all-ones code of 16 bits free (T.81 C reserves it).  Most of the code space of the long
    lengths stays unused, so a decode from a wrong bit offset meets invalid codes all the time."""
    order = [symbols[i] for i in np.random.default_rng(seed).permutation(len(symbols))]
    budget, lens, l = (1 << 16) - 1, {}, first                                   # in units of 2^-16
    for i, s in enumerate(order):
        later = len(order) - i - 1
        while l < 16 and budget - (1 << (16 - l)) < later:
            l += 1
        lens[s] = l
        budget -= 1 << (16 - l)
        l = min(l + 1, 16)
    assert budget >= 0
    return table_from_lengths(lens)


def fill_code_space(bits, vals):
    """the table with 16-bit codes added (for AC symbols of categories 11-15, which no 8-bit file uses) until none is free: its last
    code is the all-ones code of 16 bits, which libjpeg refuses"""
    free = (1 << 16) - sum(n << (15 - i) for i, n in enumerate(bits))
    spare = [(r << 4) | s for r in range(16) for s in range(11, 16) if (r << 4) | s not in vals]
    assert 0 < free <= len(spare)
    return bits[:15] + [bits[15] + free], vals + spare[:free]


# ---- the writer ---------------------------------------------------------------------------------------------------------------------

class BitWriter:
    """MSB-first bits -> bytes with 0xFF stuffed (F.1.2.3)"""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, code, length):
        self.acc = (self.acc << length) | (code & ((1 << length) - 1))
        self.n += length
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 255
            self.n -= 8
            self.out.append(b)
            if b == 255:
                self.out.append(0)
        self.acc &= (1 << self.n) - 1

    def flush(self, pad_bit=1):
        if self.n:
            k = 8 - self.n
            self.put(((1 << k) - 1) if pad_bit else 0, k)
        o, self.out = bytes(self.out), bytearray()
        return o


def magnitude(v):
    """value -> (category, extra bits) (F.1.2.1)"""
    if v == 0:
        return 0, 0
    s = int(abs(v)).bit_length()
    return s, (v if v > 0 else v + (1 << s) - 1)


def put_block(bw, blk, pred, dc_codes, ac_codes):
    """one block of 64 zig-zag coefficients; returns its DC value (the next prediction)"""
    s, extra = magnitude(int(blk[0]) - pred)
    bw.put(*dc_codes[s])
    bw.put(extra, s)
    nz = [k for k in range(1, 64) if blk[k]]
    run = 0
    for k in range(1, (nz[-1] if nz else 0) + 1):
        if blk[k] == 0:
            run += 1
            continue
        while run > 15:
            bw.put(*ac_codes[0xF0])
            run -= 16
        s, extra = magnitude(int(blk[k]))
        bw.put(*ac_codes[(run << 4) | s])
        bw.put(extra, s)
        run = 0
    if not nz or nz[-1] < 63:
        bw.put(*ac_codes[0x00])
    return int(blk[0])


def block_grids(width, height, comps):
    """[(blocks down, blocks across)] per component, padded to whole MCUs; (MCUs across, MCUs down)"""
    if len(comps) == 1:                                                          # a single-component scan: one block per MCU (A.2.2)
        mx, my = -(-width // 8), -(-height // 8)
        return [(my, mx)], (mx, my)
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    mx, my = -(-width // (8 * hmax)), -(-height // (8 * vmax))
    return [(my * c[2], mx * c[1]) for c in comps], (mx, my)


def craft(width, height, comps, coefs, dqt, dht, restart=0, pad_bit=1, fill=0, tail=b"", before_sof=b"", before_sos=b"", sof=0xC0,
          short_segment=None, raw_scan=None):
    """-> the file's bytes.
    comps       [(id, h, v, tq, td, ta)] in frame order; three components make one interleaved scan, one component one block per MCU
    coefs       per component an int array [blocks down, blocks across, 64] in zig-zag order, padded to whole MCUs (block_grids)
    dqt         DQT segments: [[(id, pq, 64 values in zig-zag order), ...], ...] -- pq 0: 8-bit, 1: 16-bit entries
    dht         DHT segments: [[(0 dc / 1 ac, id, BITS, HUFFVAL), ...], ...]
    restart     restart interval in MCUs (0: no DRI segment)
    pad_bit     the bit that completes the last byte of an entropy-coded segment
    fill        number of 0xFF fill bytes in front of every marker this function writes after SOI (RSTn and EOI included)
    tail        bytes appended after the last MCU of every entropy-coded segment (keep them free of 0xFF)
    before_sof  raw bytes right after SOI (APPn, COM ...); before_sos: raw bytes right before SOS (a DRI 0, a redefined table ...)
    sof         the frame marker, 0xC0 or 0xC1
    short_segment  index of an entropy-coded segment written without its last MCU
    raw_scan    callable(BitWriter, dc codes by table id, ac codes by table id) that writes the scan's bits itself (no restarts)"""
    nc = len(comps)
    ff = b"\xff" * fill
    out = b"\xff\xd8" + before_sof
    for tabs in dqt:
        out += ff + segment(0xDB, b"".join(bytes([(pq << 4) | t]) + (b"".join(int(x).to_bytes(2, "big") for x in q) if pq else
                                                                       bytes(int(x) for x in q)) for t, pq, q in tabs))
    out += ff + segment(sof, bytes([8]) + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([nc]) +
                        b"".join(bytes([c[0], (c[1] << 4) | c[2], c[3]]) for c in comps))
    for tabs in dht:
        out += ff + segment(0xC4, b"".join(bytes([(tc << 4) | t]) + bytes(b) + bytes(v) for tc, t, b, v in tabs))
    if restart:
        out += ff + segment(0xDD, restart.to_bytes(2, "big"))
    out += before_sos
    out += ff + segment(0xDA, bytes([nc]) + b"".join(bytes([c[0], (c[4] << 4) | c[5]]) for c in comps) + bytes([0, 63, 0]))
    dcc = {t: canonical_codes(b, v) for tabs in dht for tc, t, b, v in tabs if tc == 0}
    acc = {t: canonical_codes(b, v) for tabs in dht for tc, t, b, v in tabs if tc == 1}
    bw = BitWriter()
    if raw_scan is not None:
        raw_scan(bw, dcc, acc)
        return out + bw.flush(pad_bit) + tail + ff + b"\xff\xd9"
    grids, (mx, my) = block_grids(width, height, comps)
    for c, g in zip(coefs, grids):
        assert c.shape == g + (64,), (c.shape, g)
    total = mx * my
    nseg = -(-total // restart) if restart else 1
    pred, seg = [0] * nc, 0
    for m in range(total):
        if restart and m and m % restart == 0:
            out += bw.flush(pad_bit) + tail + ff + bytes([0xFF, 0xD0 + (seg & 7)])
            seg += 1
            pred = [0] * nc
        if seg == short_segment and (m + 1 == total or (restart and (m + 1) % restart == 0)):
            continue
        for ci, c in enumerate(comps):
            hh, vv = (1, 1) if nc == 1 else (c[1], c[2])
            for j in range(hh * vv):
                by, bx = (m // mx) * vv + j // hh, (m % mx) * hh + j % hh
                pred[ci] = put_block(bw, coefs[ci][by, bx], pred[ci], dcc[c[4]], acc[c[5]])
    assert seg + 1 == nseg
    return out + bw.flush(pad_bit) + tail + ff + b"\xff\xd9"


# ---- coefficients -------------------------------------------------------------------------------------------------------------------

def block_sums(c, q):
    """sum_k |coef_k q_k| per block"""
    return (np.abs(c) * np.asarray(q).reshape(1, 1, 64)).sum(-1)


def fit_bound(c, q, hi):
    """shrink (towards zero) every block of c whose sum_k |coef_k q_k| exceeds hi"""
    c = c.copy()
    q = np.asarray(q)
    for b in c.reshape(-1, 64):
        s = int((np.abs(b) * q).sum())
        if s > hi:
            b[:] = np.trunc(b * (hi / s)).astype(b.dtype)
    assert block_sums(c, q).max() <= hi
    return c


def random_coefs(rng, grid, q, amp_dc=60, amp_ac=6, density=0.3, hi=2048):
    c = np.zeros(grid + (64,), dtype=np.int64)
    c[..., 0] = rng.integers(-amp_dc, amp_dc + 1, grid)
    m = rng.random(grid + (63,)) < density
    c[..., 1:] = np.where(m, rng.integers(-amp_ac, amp_ac + 1, grid + (63,)), 0)
    return fit_bound(c, q, hi)


def range_limit_coefs(rng, grid, q):
    """blocks with sum_k |coef_k q_k| in (2048, COEF_BOUND]: a few large coefficients of random sign, so that many samples leave [0, 255]"""
    q = np.asarray(q)
    c = np.zeros(grid + (64,), dtype=np.int64)
    for b in c.reshape(-1, 64):
        while not 2048 < int((np.abs(b) * q).sum()) <= COEF_BOUND:                # redraw until the block is inside the interval
            b[:] = 0
            n = int(rng.integers(3, 9))
            idx = rng.choice(64, n, replace=False)
            w = rng.random(n) ** 2 + 0.05
            w = w / w.sum() * rng.uniform(0.6, 1.0) * COEF_BOUND
            b[idx] = np.clip(np.floor(w / q[idx]).astype(np.int64), 0, 1000) * rng.choice([-1, 1], n)
    return c


# ---- the corpus ---------------------------------------------------------------------------------------------------------------------

SUPPORTED, UNSUPPORTED, BROKEN = "supported", "unsupported", "broken"
Case = collections.namedtuple("Case", "name data cls")

SAMPLINGS = {"420": (2, 2), "422": (2, 1), "444": (1, 1), "gray": None}

Q_LUMA = [3 + (7 * k) % 13 for k in range(64)]                                   # zig-zag order; not symmetric, so a transposed or
Q_CHROMA = [2 + (5 * k) % 11 for k in range(64)]                                 # un-zig-zagged table shows
Q_THIRD = [1 + (3 * k) % 7 for k in range(64)]


def _tables(seed):
    return dict(fdc=flat_dc(), fac=flat_ac(), sdc=staircase(DC_SYMBOLS, seed), sac=staircase(AC_SYMBOLS, seed + 1),
                ddc=staircase(DC_SYMBOLS, seed + 2, first=5), sac2=staircase(AC_SYMBOLS, seed + 3, first=2))


def base_file(height, width, sampling, seed=0):
    """the arguments of craft() for the corpus' plain file: luma on a flat DC and a staircase AC table, chroma the other way round"""
    rng = np.random.default_rng([seed, height, width, len(sampling)])
    T = _tables(seed)
    hv = SAMPLINGS[sampling]
    if hv is None:
        comps = [(1, 1, 1, 0, 0, 0)]
    else:
        comps = [(1, hv[0], hv[1], 0, 0, 0), (2, 1, 1, 1, 1, 1), (3, 1, 1, 1, 1, 1)]
    grids, _ = block_grids(width, height, comps)
    qs = [Q_LUMA, Q_CHROMA, Q_CHROMA]
    coefs = [random_coefs(rng, g, qs[i]) for i, g in enumerate(grids)]
    dqt = [[(0, 0, Q_LUMA)], [(1, 0, Q_CHROMA)]]
    dht = [[(0, 0, *T["fdc"])], [(1, 0, *T["sac"])], [(0, 1, *T["sdc"])], [(1, 1, *T["fac"])]]
    return dict(width=width, height=height, comps=comps, coefs=coefs, dqt=dqt, dht=dht, before_sof=JFIF), rng, T, grids


def _retable(comps, tq=None, td=None, ta=None, ids=None, hv=None):
    out = []
    for i, c in enumerate(comps):
        c = list(c)
        if ids is not None:
            c[0] = ids[i]
        if hv is not None:
            c[1], c[2] = hv[i]
        if tq is not None:
            c[3] = tq[i]
        if td is not None:
            c[4] = td[i]
        if ta is not None:
            c[5] = ta[i]
        out.append(tuple(c))
    return out


def overflow_scan(n_blocks):
    """raw_scan for a one-component file on table 0: the first block's run passes coefficient 63 (DC, then four times run 15 + a value:
    k = 16, 32, 48, 64), the rest are plain.  libjpeg stores the last value at index 63 (its natural-order table is padded with 63)."""
    def write(bw, dcc, acc):
        bw.put(*dcc[0][3])
        bw.put(5, 3)
        for _ in range(4):
            bw.put(*acc[0][0xF1])
            bw.put(1, 1)
        for _ in range(n_blocks - 1):
            bw.put(*dcc[0][2])
            bw.put(3, 2)
            bw.put(*acc[0][0x00])
    return write


def no_code_scan(n_blocks):
    """raw_scan on the flat tables: the second block's DC position holds 1111, which the 12-symbol 4-bit table does not assign"""
    def write(bw, dcc, acc):
        bw.put(*dcc[0][2])
        bw.put(3, 2)
        bw.put(*acc[0][0x00])
        bw.put(0xF, 4)
        for _ in range(n_blocks):
            bw.put(*dcc[0][0])
            bw.put(*acc[0][0x00])
    return write


def corpus(height, width, samplings=("420", "422", "444", "gray"), seed=0):
    """-> [Case]: the crafted files of one size.  Every SUPPORTED file keeps sum_k |coef_k q_k| <= COEF_BOUND in every block."""
    cases = []
    for sampling in samplings:
        base, rng, T, grids = base_file(height, width, sampling, seed)
        three = sampling != "gray"
        comps = base["comps"]
        _, (mx, my) = block_grids(width, height, comps)

        def add(name, cls=SUPPORTED, **over):
            kw = {**base, **over}
            if cls == SUPPORTED and "raw_scan" not in kw:
                qv = {t: q for tabs in kw["dqt"] for t, pq, q in tabs}
                for c, co in zip(kw["comps"], kw["coefs"]):
                    assert block_sums(co, qv[c[3]]).max() <= COEF_BOUND, name
            cases.append(Case(f"{sampling}_{height}x{width}_{name}", craft(**kw), cls))

        def all_tables(ldc, lac, cdc, cac):
            return [(0, 0, *T[ldc]), (1, 0, *T[lac]), (0, 1, *T[cdc]), (1, 1, *T[cac])]

        # Huffman tables
        add("base")
        add("flat_everywhere", dht=[[t] for t in all_tables("fdc", "fac", "fdc", "fac")])
        add("staircase_everywhere", dht=[[t] for t in all_tables("sdc", "sac", "ddc", "sac2")])
        add("staircase_luma_flat_chroma", dht=[[t] for t in all_tables("ddc", "sac2", "fdc", "fac")])
        add("flat_luma_staircase_chroma", dht=[[t] for t in all_tables("fdc", "fac", "sdc", "sac")])
        add("four_tables_one_dht", dht=[all_tables("fdc", "sac", "sdc", "fac")])
        add("huff_ids_swapped", comps=_retable(comps, td=[1, 0, 0], ta=[1, 0, 0]))
        add("huff_dc_ac_ids_differ", comps=_retable(comps, td=[0, 1, 0], ta=[1, 0, 1]))
        add("huff_id_2_sof1", UNSUPPORTED, sof=0xC1, comps=_retable(comps, td=[2, 1, 1]), dht=base["dht"] + [[(0, 2, *T["fdc"])]])
        # quantisation tables
        q3 = [[(3, 0, Q_LUMA)], [(2, 0, Q_CHROMA)], [(0, 0, Q_THIRD)]]
        co3 = [random_coefs(rng, g, q) for g, q in zip(grids, (Q_LUMA, Q_CHROMA, Q_THIRD))]
        add("q_ids_3_2_0_three_tables", comps=_retable(comps, tq=[3, 2, 0]), dqt=q3, coefs=co3)
        add("q_16bit_small_values", dqt=[[(0, 1, Q_LUMA)], [(1, 1, Q_CHROMA)]])
        q300 = [300 + 17 * (k % 5) for k in range(64)]
        add("q_16bit_large_values", dqt=[[(0, 1, q300)], [(1, 0, Q_CHROMA)]],
            coefs=[random_coefs(rng, grids[0], q300, amp_dc=3, amp_ac=1, density=0.1)] + base["coefs"][1:])
        add("q_two_tables_one_dqt", dqt=[[(0, 0, Q_LUMA), (1, 1, Q_CHROMA)]])
        # component ids and colour markers
        if three:
            add("ids_0_1_2", comps=_retable(comps, ids=[0, 1, 2]))
            add("ids_10_20_30_no_jfif", comps=_retable(comps, ids=[10, 20, 30]), before_sof=b"")
            add("ids_rgb_full_jfif", comps=_retable(comps, ids=[82, 71, 66]))
            add("ids_rgb_no_jfif", UNSUPPORTED, comps=_retable(comps, ids=[82, 71, 66]), before_sof=b"")
            add("ids_rgb_short_jfif", UNSUPPORTED, comps=_retable(comps, ids=[82, 71, 66]), before_sof=segment(0xE0, b"JFIF\x00\x01\x01"))
            add("adobe_transform_1", before_sof=adobe(1))
            add("adobe_transform_1_ids_rgb", comps=_retable(comps, ids=[82, 71, 66]), before_sof=adobe(1))
            add("adobe_transform_0", UNSUPPORTED, before_sof=adobe(0))
            add("adobe_transform_0_with_jfif", UNSUPPORTED, before_sof=JFIF + adobe(0))
        else:
            add("gray_id_0", comps=_retable(comps, ids=[0]))
            add("gray_sof_says_h2v2", comps=_retable(comps, hv=[(2, 2)]))
        # markers
        add("sof1", sof=0xC1)
        add("dri_0", before_sos=segment(0xDD, b"\x00\x00"))
        unused = segment(0xDB, bytes([2]) + bytes([9] * 64))                      # nothing uses quantisation table 2 ...
        if not three:                                                            # ... and a gray scan no Huffman table 1
            unused += segment(0xC4, bytes([0x01]) + bytes(T["ddc"][0]) + bytes(T["ddc"][1]) + bytes([0x11]) + bytes(T["sac2"][0]) + bytes(T["sac2"][1]))
        add("unused_tables_redefined", before_sos=unused)
        thumb = craft(8, 8, [(1, 1, 1, 0, 0, 0)], [random_coefs(rng, (1, 1), Q_LUMA)], [[(0, 0, Q_LUMA)]], [[(0, 0, *T["fdc"]), (1, 0, *T["fac"])]])
        add("exif_thumbnail_and_com", before_sof=JFIF + segment(0xE1, b"Exif\x00\x00" + b"\x00" * 40 + thumb) +
            segment(0xFE, b"comment \xff\xd9 \xff\xda \xff\xc4 end"))
        # restart intervals, padding, fill bytes
        for ri in (1, 2, 3):
            add(f"restart_{ri}", restart=ri)
        add("restart_mcu_row", restart=mx)
        add("restart_1_zero_padding", restart=1, pad_bit=0)
        add("zero_padding", pad_bit=0)
        add("fill_bytes", fill=3, restart=2)
        add("trailing_bytes", tail=b"\x12\x34\x56")
        add("trailing_bytes_restart", tail=b"\x00\x5a", restart=2)
        # coefficients
        add("dense_no_eob", coefs=[np.where(c == 0, 1, np.sign(c)) for c in base["coefs"]])
        only63 = [np.zeros_like(c) for c in base["coefs"]]
        for c in only63:
            c[..., 63] = 3
            c[..., 0] = 10
        add("only_coefficient_63", coefs=only63)
        one = [[(0, 0, [1] * 64)], [(1, 0, Q_CHROMA)]]
        dc = base["coefs"][0].copy()
        dc[..., 1:] = np.where(rng.random(dc[..., 1:].shape) < 0.05, rng.integers(-3, 4, dc[..., 1:].shape), 0)
        dc[..., 0] = np.where((np.add.outer(np.arange(grids[0][0]), np.arange(grids[0][1])) % 2) == 0, -1000, 1000)
        add("dc_plus_minus_1000", dqt=one, coefs=[dc] + base["coefs"][1:])
        big = np.zeros_like(base["coefs"][0])
        for y in range(grids[0][0]):
            for x in range(grids[0][1]):
                big[y, x, rng.choice(np.arange(1, 64), 2, replace=False)] = rng.integers(512, 1024, 2) * rng.choice([-1, 1], 2)
        big[..., 0] = rng.integers(-100, 101, grids[0])
        add("ac_10_bit_magnitudes", dqt=one, coefs=[big] + base["coefs"][1:])
        add("all_zero_blocks", coefs=[np.zeros_like(c) for c in base["coefs"]])
        # range limit: sum_k |coef_k q_k| in (2048, COEF_BOUND] on every luma block
        for nm, pq, q in (("q1", 0, [1] * 64), ("q7", 0, [7] * 64), ("q300_16bit", 1, [300] * 64)):
            add(f"range_limit_{nm}", dqt=[[(0, pq, q)], [(1, 0, Q_CHROMA)]], coefs=[range_limit_coefs(rng, grids[0], q)] + base["coefs"][1:])
        # Huffman tables libjpeg refuses: the all-ones code of a length assigned; a DC category above 15
        ones = table_from_lengths({s: 4 for s in range(16)})
        add("huff_all_ones_code", BROKEN, dht=[[(0, 0, *ones)]] + base["dht"][1:])
        add("huff_all_ones_code_16_bits", BROKEN, dht=base["dht"][:1] + [[(1, 0, *fill_code_space(*T["sac"]))]] + base["dht"][2:])
        add("huff_dc_category_16", BROKEN, dht=[[(0, 0, *table_from_lengths({**{s: 4 for s in DC_SYMBOLS}, 16: 4}))]] + base["dht"][1:])
        # other samplings PIL decodes and the device does not
        if three and sampling == "444":
            for nm, hv in (("440", [(1, 2), (1, 1), (1, 1)]), ("411", [(4, 1), (1, 1), (1, 1)])):
                cs = _retable(comps, hv=hv)
                g, _ = block_grids(width, height, cs)
                add(f"sampling_{nm}", UNSUPPORTED, comps=cs, coefs=[random_coefs(rng, gg, q) for gg, q in zip(g, (Q_LUMA, Q_CHROMA, Q_CHROMA))], restart=2)
    return cases


def malformed(height=16, width=32):
    """the short fixed list of malformed one-component files the device also sees: [(name, bytes)].  For each the decoder either reports a
    non-zero status or gives PIL's pixels."""
    T = _tables(0)
    comps = [(1, 1, 1, 0, 0, 0)]
    grids, (mx, my) = block_grids(width, height, comps)
    rng = np.random.default_rng(7)
    kw = dict(width=width, height=height, comps=comps, coefs=[random_coefs(rng, grids[0], Q_LUMA)], dqt=[[(0, 0, Q_LUMA)]],
              dht=[[(0, 0, *T["fdc"])], [(1, 0, *T["fac"])]], before_sof=JFIF)
    n = mx * my
    return [("trailing_bytes", craft(**kw, tail=b"\x12\x34\x56\x78\x12")),
            ("run_overflow", craft(**kw, raw_scan=overflow_scan(n))),
            ("segment_one_mcu_short", craft(**kw, restart=mx, short_segment=0)),
            ("code_in_no_table", craft(**kw, raw_scan=no_code_scan(n)))]
