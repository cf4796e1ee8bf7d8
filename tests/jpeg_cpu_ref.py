"""Numpy restatement of the device JPEG decoder's arithmetic (csrc/jpeg.hip; jpeg_ops.py's stage table), for the CPU tests: a sequential
Huffman decode of jpeg_ops.parse()'s record, DC prediction, libjpeg's JDCT_ISLOW inverse DCT, fancy (triangle) upsampling, the fixed-point
YCbCr -> RGB conversion and the loaders' luma.  Restated from ITU-T T.81 and libjpeg's documented behaviour.  Test infrastructure only
(like sift_cpu_ref.py): slow, meant for small images."""
import numpy as np

ZZ = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
               35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


def _huff(t, bits, p):
    """decode one symbol at bit p -> (symbol, length) or (None, 0)"""
    code = 0
    for l in range(1, 17):
        code = (code << 1) | int(bits[p + l - 1]) if p + l - 1 < bits.size else (code << 1) | 1
        if t.maxcode[l] >= 0 and code <= t.maxcode[l]:
            return t.val[code + t.valoff[l]], l
    return None, 0


def coefficients(h, rec):
    """entropy decode + DC prediction -> int32 [blocks, 64] (natural order, MCU block order)"""
    seg = np.frombuffer(rec[:h.seg_table_bytes].tobytes(), dtype=np.uint32).reshape(-1, 2)[:h.nseg]
    data = rec[h.seg_table_bytes:h.seg_table_bytes + h.data_bytes]
    bpm = h.blocks_per_mcu
    coef = np.zeros((h.total_mcus * bpm, 64), dtype=np.int32)
    blk = 0
    for s in range(h.nseg):
        end = seg[s + 1, 0] if s + 1 < h.nseg else h.data_bytes
        bits = np.unpackbits(data[seg[s, 0]:end])
        p, pred = 0, [0, 0, 0, 0]
        for _ in range(int(seg[s, 1])):
            for j in range(bpm):
                c = h.mcu_comp[j]
                sym, l = _huff(h.dc[h.comp_td[c]], bits, p)
                assert sym is not None and p + l + sym <= bits.size, "bad DC code"
                p += l
                v = int("".join(map(str, bits[p:p + sym])) or "0", 2)
                if sym and v < (1 << (sym - 1)):
                    v -= (1 << sym) - 1
                p += sym
                pred[c] += v
                coef[blk, 0] = pred[c]
                k = 1
                while k < 64:
                    rs, l = _huff(h.ac[h.comp_ta[c]], bits, p)
                    assert rs is not None, "bad AC code"
                    p += l
                    r, sz = rs >> 4, rs & 15
                    if sz:
                        k += r
                        assert p + sz <= bits.size, "bad AC code"
                        v = int("".join(map(str, bits[p:p + sz])), 2)
                        if v < (1 << (sz - 1)):
                            v -= (1 << sz) - 1
                        p += sz
                        coef[blk, ZZ[min(k, 63)]] = v
                        k += 1
                    elif r == 15:
                        k += 16
                    else:
                        break
                blk += 1
    return coef


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def idct_islow(coef, q):
    """[N, 64] int coefficients (natural order), [64] quantisation table -> [N, 8, 8] u8 samples (libjpeg JDCT_ISLOW)"""
    C, P = 13, 2
    F = dict(f0298=2446, f0390=3196, f0541=4433, f0765=6270, f0899=7373, f1175=9633, f1501=12299, f1847=15137, f1961=16069,
             f2053=16819, f2562=20995, f3072=25172)

    def one_d(x0, x1, x2, x3, x4, x5, x6, x7, pass1):
        z1 = (x2 + x6) * F["f0541"]
        t2 = z1 - x6 * F["f1847"]
        t3 = z1 + x2 * F["f0765"]
        t0 = (x0 + x4) << C
        t1 = (x0 - x4) << C
        t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
        a0, a1, a2, a3 = x7, x5, x3, x1
        z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
        z5 = (z3 + z4) * F["f1175"]
        a0, a1, a2, a3 = a0 * F["f0298"], a1 * F["f2053"], a2 * F["f3072"], a3 * F["f1501"]
        z1, z2, z3, z4 = -z1 * F["f0899"], -z2 * F["f2562"], -z3 * F["f1961"] + z5, -z4 * F["f0390"] + z5
        a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
        sh = C - P if pass1 else C + P + 3
        return [_descale(v, sh) for v in (t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3)]

    d = coef.astype(np.int64).reshape(-1, 8, 8) * q.astype(np.int64).reshape(1, 8, 8)
    ws = np.stack(one_d(*[d[:, r, :] for r in range(8)], True), axis=1)          # columns: [N, row, col]
    out = np.stack(one_d(*[ws[:, :, c] for c in range(8)], False), axis=2)       # rows
    # libjpeg-turbo's SIMD ISLOW packs the descaled output with signed saturation: a clamp to [-128, 127], then + 128.  (libjpeg's C code
    # looks the output up modulo 1024 in its range-limit table; PIL's decoder runs the SIMD routine.)
    return (np.clip(out, -128, 127) + 128).astype(np.uint8)


def planes(h, coef):
    """u8 component planes padded to whole MCUs"""
    out = []
    bpm = h.blocks_per_mcu
    for c in range(h.ncomp):
        bw, bh = h.comp_bw[c], h.comp_bh[c]
        pl = np.zeros((h.plane_h[c], h.plane_w[c]), dtype=np.uint8)
        q = np.array(h.qt[h.comp_tq[c]], dtype=np.int64)
        for jj in range(bw * bh):
            idx = np.arange(h.total_mcus) * bpm + h.comp_off[c] + jj
            s = idct_islow(coef[idx], q)
            mx, my = np.arange(h.total_mcus) % h.mcus_x, np.arange(h.total_mcus) // h.mcus_x
            for m in range(h.total_mcus):
                by, bx = my[m] * bh + jj // bw, mx[m] * bw + jj % bw
                pl[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = s[m]
        out.append(pl)
    return out


def upsample(pl, dw, dh, hf, vf, W, H):
    """libjpeg fancy upsampling of a [.., >= dw] plane by (hf, vf) in {(1,1), (2,1), (2,2)} -> [H, W] int"""
    a = pl.astype(np.int64)
    if (hf, vf) == (1, 1):
        return a[:H, :W]
    ys = np.arange(H)
    cy = ys // vf
    if vf == 2:
        far = np.clip(np.where(ys % 2 == 0, cy - 1, cy + 1), 0, dh - 1)
        col = 3 * a[cy] + a[far]                                                 # [H, plane_w], x4
        bias_even, bias_odd, sh, mul = 8, 7, 4, 3
    else:
        col = a[cy]
        bias_even, bias_odd, sh, mul = 1, 2, 2, 3
    xs = np.arange(W)
    cx = xs // 2
    this = col[:, cx]
    prev = col[:, np.maximum(cx - 1, 0)]
    nxt = col[:, np.minimum(cx + 1, col.shape[1] - 1)]
    even = np.where(cx == 0, this * 4 if vf == 2 else this, (mul * this + prev + bias_even) >> sh)
    last = cx == dw - 1
    odd = np.where(last, (this * 4 + 7) >> 4 if vf == 2 else this, (mul * this + nxt + bias_odd) >> sh)
    if vf == 2:
        even = np.where(cx == 0, (this * 4 + 8) >> 4, even)
    return np.where(xs % 2 == 0, even, odd)


def fix(x):
    return int(x * 65536 + 0.5)


def ycc_to_rgb(y, cb, cr):
    cb, cr = cb.astype(np.int64) - 128, cr.astype(np.int64) - 128
    r = y + ((fix(1.40200) * cr + 32768) >> 16)
    g = y + ((-fix(0.34414) * cb + 32768 - fix(0.71414) * cr) >> 16)
    b = y + ((fix(1.77200) * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def decode_rgb(h, rec):
    """record -> RGB u8 [H, W, 3] (a gray image: Y replicated)"""
    pl = planes(h, coefficients(h, rec))
    W, H = h.width, h.height
    y = pl[0][:H, :W].astype(np.int64)
    if h.ncomp == 1:
        return np.repeat(y.astype(np.uint8)[..., None], 3, -1)
    hf, vf = h.hmax // h.comp_h[1], h.vmax // h.comp_v[1]
    cb = upsample(pl[1], h.down_w[1], h.down_h[1], hf, vf, W, H)
    cr = upsample(pl[2], h.down_w[2], h.down_h[2], hf, vf, W, H)
    return ycc_to_rgb(y, cb, cr)
