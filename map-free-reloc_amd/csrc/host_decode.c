/* host_decode.c -- libmfr_host.so: the two per-pixel loops of the batched loaders (datasets.py), in C.
 *
 * Reference: the matchers' gray input (etc/feature_matching_baselines/matchers.py:101-104 -> SuperGlue's read_image: an 8-bit grayscale
 * read of the file, / 255 as float32) and lib/datasets/utils.py:77-81 (read_depth_image: uint16 mm / 1000 as float32).  The loaders of
 * the fused path want, per frame, the float32 gray plane  float32(luma_u8(R, G, B)) / 255f  with luma_u8 = (19595 R + 38470 G + 7471 B +
 * 2^15) >> 16 (ITU-R 601-2 rounded to a byte: datasets.luma_u8) and the metric depth float32(v / 1000.0).  Both are table look-ups of
 * the SAME rounded values the numpy expressions produce (the tables are built by numpy in datasets.py); what this file saves is the
 * intermediate arrays and, for the caller, one copy: the results are written straight into the batch slot.  Plain C, no dependencies;
 * not a compute path of the GPU product (that is libmfr_hip.so) -- without this library datasets.py runs the numpy expressions.
 * Since ABI 3 it also holds the host half of the device JPEG decoder (mfr_host_jpeg_parse below; jpeg_ops.py), since ABI 4 that of
 * the device depth PNG decoder (mfr_host_png_parse at the end; png_ops.py).
 */
#include <stddef.h>
#include <stdint.h>

/* rgb: n pixels, 3 bytes each (PIL "RGB" raw order); lut: 256 floats (byte / 255); out: n floats */
void mfr_host_gray_from_rgb(const uint8_t *rgb, size_t n, const float *lut, float *out)
{
    for (size_t i = 0; i < n; ++i)
        out[i] = lut[((uint32_t)rgb[3 * i] * 19595u + (uint32_t)rgb[3 * i + 1] * 38470u + (uint32_t)rgb[3 * i + 2] * 7471u + 0x8000u) >> 16];
}

/* d: n uint16 values; lut: 65536 floats; out: n floats */
void mfr_host_depth_from_u16(const uint16_t *d, size_t n, const float *lut, float *out)
{
    for (size_t i = 0; i < n; ++i) out[i] = lut[d[i]];
}

int mfr_host_abi_version(void) { return 4; }   /* 3: mfr_host_jpeg_parse; 4: mfr_host_png_parse */

/* ---- baseline JPEG: header parse + entropy-segment preparation for the device decoder (csrc/jpeg.hip) ----
 * ITU-T T.81: markers B.1, frame / scan headers B.2, tables B.2.4, restart intervals B.2.4.4 and F.1.2.3, canonical Huffman codes C.
 * Colour interpretation as the JFIF / Adobe APP14 conventions: three components are YCbCr unless an Adobe marker says transform 0, or,
 * with neither a JFIF (APP0 "JFIF\0" of >= 14 bytes) nor an Adobe marker, the component ids spell 'R', 'G', 'B'.  Every read is bounded by n.  Layout: include/mfr_jpeg.h. */
#include <string.h>
#include "mfr_jpeg.h"

static const uint8_t zz_natural[64] = {
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

/* canonical code tables (T.81 C.2 / F.2.2.3) from BITS / HUFFVAL; 0 = ok, -1 = a table libjpeg refuses to decode with ("bogus Huffman
 * table"): BITS over-subscribe the code space, the last code of a length is all ones (T.81 C reserves it), or a DC table holds a
 * category above 15 */
static int huff_build(mfr_jpeg_huff *t, int is_dc)
{
    int code = 0, k = 0;
    memset(t->fast, 0, sizeof(t->fast));
    for (int l = 1; l <= 16; ++l) {
        int nl = t->bits[l - 1];
        t->maxcode[l] = -1;
        t->valoff[l] = 0;
        if (nl) {
            t->valoff[l] = k - code;
            for (int i = 0; i < nl; ++i, ++code, ++k) {
                if (code >= (1 << l)) return -1;
                if (l <= MFR_JPEG_FAST_BITS) {
                    int sh = MFR_JPEG_FAST_BITS - l;
                    for (int f = code << sh; f < ((code + 1) << sh); ++f) t->fast[f] = (uint16_t)((l << 8) | t->val[k]);
                }
            }
            t->maxcode[l] = code - 1;
            if (code >= (1 << l)) return -1;
        }
        code <<= 1;
    }
    if (is_dc)
        for (int i = 0; i < k; ++i)
            if (t->val[i] > 15) return -1;
    return 0;
}

static int rd16(const uint8_t *b, size_t n, size_t i) { return i + 1 < n ? (b[i] << 8) | b[i + 1] : -1; }

/* buf[0..n) -> *h and the record out[0..cap); *rec_bytes = the record's size.  Returns MFR_JPEG_OK / _UNSUPPORTED / _INVALID / _CAPACITY
 * (also in h->status). */
int mfr_host_jpeg_parse(const uint8_t *buf, size_t n, mfr_jpeg_header *h, uint8_t *out, size_t cap, size_t *rec_bytes)
{
    int have_q[4] = {0}, have_dc[2] = {0}, have_ac[2] = {0}, jfif = 0, sof = 0;
    size_t i = 2;
    memset(h, 0, sizeof(*h));
    h->adobe_transform = -1;
    *rec_bytes = 0;
#define FAIL(code) do { h->status = (code); return (code); } while (0)
    if (n < 4 || buf[0] != 0xFF || buf[1] != 0xD8) FAIL(MFR_JPEG_INVALID);
    for (;;) {                                                           /* markers up to SOS */
        if (i >= n || buf[i] != 0xFF) FAIL(MFR_JPEG_INVALID);
        while (i < n && buf[i] == 0xFF) ++i;                             /* fill bytes */
        if (i >= n) FAIL(MFR_JPEG_INVALID);
        int m = buf[i++];
        if (m == 0xD8 || m == 0xD9 || (m >= 0xD0 && m <= 0xD7) || m == 0x01 || m == 0x00) FAIL(MFR_JPEG_INVALID);
        int len = rd16(buf, n, i);
        if (len < 2 || i + (size_t)len > n) FAIL(MFR_JPEG_INVALID);
        const uint8_t *s = buf + i + 2;
        size_t sl = (size_t)len - 2;
        i += (size_t)len;
        if (m == 0xC0 || m == 0xC1) {                                    /* SOF0 / SOF1 */
            if (sof || sl < 6) FAIL(MFR_JPEG_INVALID);
            sof = 1;
            if (s[0] != 8) FAIL(MFR_JPEG_UNSUPPORTED);
            h->height = (s[1] << 8) | s[2];
            h->width = (s[3] << 8) | s[4];
            h->ncomp = s[5];
            if (h->width == 0) FAIL(MFR_JPEG_INVALID);
            if (h->height == 0) FAIL(MFR_JPEG_UNSUPPORTED);              /* height from a DNL marker */
            if (h->ncomp == 0 || sl != 6 + 3 * (size_t)h->ncomp) FAIL(MFR_JPEG_INVALID);
            if (h->ncomp != 1 && h->ncomp != 3) FAIL(MFR_JPEG_UNSUPPORTED);
            for (int c = 0; c < h->ncomp; ++c) {
                h->comp_id[c] = s[6 + 3 * c];
                h->comp_h[c] = s[7 + 3 * c] >> 4;
                h->comp_v[c] = s[7 + 3 * c] & 15;
                h->comp_tq[c] = s[8 + 3 * c];
                if (h->comp_h[c] < 1 || h->comp_h[c] > 4 || h->comp_v[c] < 1 || h->comp_v[c] > 4 || h->comp_tq[c] > 3) FAIL(MFR_JPEG_INVALID);
                for (int d = 0; d < c; ++d)
                    if (h->comp_id[d] == h->comp_id[c]) FAIL(MFR_JPEG_INVALID);
            }
        } else if (m == 0xC4) {                                          /* DHT */
            size_t p = 0;
            while (p < sl) {
                if (p + 17 > sl) FAIL(MFR_JPEG_INVALID);
                int tc = s[p] >> 4, th = s[p] & 15, cnt = 0;
                if (tc > 1 || th > 3) FAIL(MFR_JPEG_INVALID);
                if (th > 1) FAIL(MFR_JPEG_UNSUPPORTED);
                mfr_jpeg_huff *t = tc ? &h->ac[th] : &h->dc[th];
                memset(t, 0, sizeof(*t));
                for (int l = 0; l < 16; ++l) cnt += (t->bits[l] = s[p + 1 + l]);
                if (cnt > 256 || p + 17 + (size_t)cnt > sl) FAIL(MFR_JPEG_INVALID);
                memcpy(t->val, s + p + 17, (size_t)cnt);
                /* as libjpeg, a bogus table only makes the file invalid when the scan uses it (checked below): until then it is undefined */
                if (tc) have_ac[th] = !huff_build(t, 0); else have_dc[th] = !huff_build(t, 1);
                p += 17 + (size_t)cnt;
            }
        } else if (m == 0xDB) {                                          /* DQT */
            size_t p = 0;
            while (p < sl) {
                int pq = s[p] >> 4, tq = s[p] & 15;
                if (pq > 1 || tq > 3 || p + 1 + 64 * (size_t)(pq + 1) > sl) FAIL(MFR_JPEG_INVALID);
                for (int k = 0; k < 64; ++k)
                    h->qt[tq][zz_natural[k]] = (uint16_t)(pq ? (s[p + 1 + 2 * k] << 8) | s[p + 2 + 2 * k] : s[p + 1 + k]);
                have_q[tq] = 1;
                p += 1 + 64 * (size_t)(pq + 1);
            }
        } else if (m == 0xDD) {                                          /* DRI */
            if (sl != 2) FAIL(MFR_JPEG_INVALID);
            h->restart_interval = (s[0] << 8) | s[1];
        } else if (m == 0xE0) {                                          /* APP0 */
            if (sl >= 14 && !memcmp(s, "JFIF\0", 5)) jfif = 1;             /* libjpeg: a shorter payload is not a JFIF header */
        } else if (m == 0xEE) {                                          /* APP14 */
            if (sl >= 12 && !memcmp(s, "Adobe", 5)) h->adobe_transform = s[11];
        } else if (m == 0xDA) {                                          /* SOS */
            if (!sof) FAIL(MFR_JPEG_INVALID);
            if (sl < 1 || sl != 4 + 2 * (size_t)s[0]) FAIL(MFR_JPEG_INVALID);
            int ns = s[0];
            if (ns != h->ncomp) FAIL(MFR_JPEG_UNSUPPORTED);              /* a non-interleaved first scan: multi-scan file */
            for (int q = 0; q < ns; ++q) {
                int c = 0;
                while (c < h->ncomp && h->comp_id[c] != s[1 + 2 * q]) ++c;
                if (c == h->ncomp || c != q) FAIL(MFR_JPEG_INVALID);
                h->comp_td[c] = s[2 + 2 * q] >> 4;
                h->comp_ta[c] = s[2 + 2 * q] & 15;
                if (h->comp_td[c] > 1 || h->comp_ta[c] > 1) FAIL(h->comp_td[c] > 3 || h->comp_ta[c] > 3 ? MFR_JPEG_INVALID : MFR_JPEG_UNSUPPORTED);
            }
            if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) FAIL(MFR_JPEG_INVALID);
            break;
        } else if ((m >= 0xC2 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) || m == 0xCC) {
            FAIL(MFR_JPEG_UNSUPPORTED);                                  /* progressive, lossless, hierarchical, arithmetic */
        } else if (m == 0xDC || m == 0xDE || m == 0xDF) {
            FAIL(MFR_JPEG_UNSUPPORTED);                                  /* DNL / DHP / EXP */
        }                                                                /* other APPn, COM, JPGn: skipped */
    }
    /* colour and sampling */
    if (h->ncomp == 3) {
        if (h->adobe_transform == 0 || h->adobe_transform > 1) FAIL(MFR_JPEG_UNSUPPORTED);
        if (h->adobe_transform < 0 && !jfif && h->comp_id[0] == 'R' && h->comp_id[1] == 'G' && h->comp_id[2] == 'B') FAIL(MFR_JPEG_UNSUPPORTED);
        if (h->comp_h[1] != 1 || h->comp_v[1] != 1 || h->comp_h[2] != 1 || h->comp_v[2] != 1) FAIL(MFR_JPEG_UNSUPPORTED);
        if (!((h->comp_h[0] == 1 && h->comp_v[0] == 1) || (h->comp_h[0] == 2 && h->comp_v[0] == 1) || (h->comp_h[0] == 2 && h->comp_v[0] == 2)))
            FAIL(MFR_JPEG_UNSUPPORTED);
        h->hmax = h->comp_h[0];
        h->vmax = h->comp_v[0];
        h->mcus_x = (h->width + 8 * h->hmax - 1) / (8 * h->hmax);
        h->mcus_y = (h->height + 8 * h->vmax - 1) / (8 * h->vmax);
        int off = 0;
        for (int c = 0; c < 3; ++c) {
            h->comp_bw[c] = h->comp_h[c];
            h->comp_bh[c] = h->comp_v[c];
            h->comp_off[c] = off;
            for (int b = 0; b < h->comp_h[c] * h->comp_v[c]; ++b) h->mcu_comp[off + b] = c;
            off += h->comp_h[c] * h->comp_v[c];
        }
        h->blocks_per_mcu = off;
    } else {                                                             /* one component: a non-interleaved scan, one block per MCU */
        h->hmax = h->comp_h[0];
        h->vmax = h->comp_v[0];
        h->mcus_x = (h->width + 7) / 8;
        h->mcus_y = (h->height + 7) / 8;
        h->comp_bw[0] = h->comp_bh[0] = 1;
        h->blocks_per_mcu = 1;
    }
    int poff = 0;
    for (int c = 0; c < h->ncomp; ++c) {
        if (!have_q[h->comp_tq[c]] || !have_dc[h->comp_td[c]] || !have_ac[h->comp_ta[c]]) FAIL(MFR_JPEG_INVALID);
        h->plane_w[c] = h->mcus_x * h->comp_bw[c] * 8;
        h->plane_h[c] = h->mcus_y * h->comp_bh[c] * 8;
        h->plane_off[c] = poff;
        poff += h->plane_w[c] * h->plane_h[c];
        h->down_w[c] = (int)(((long)h->width * h->comp_h[c] + h->hmax - 1) / h->hmax);
        h->down_h[c] = (int)(((long)h->height * h->comp_v[c] + h->vmax - 1) / h->vmax);
    }
    h->total_mcus = h->mcus_x * h->mcus_y;
    int ri = h->restart_interval;
    int nseg_expect = ri > 0 ? (h->total_mcus + ri - 1) / ri : 1;
    size_t seg_bytes = ((size_t)nseg_expect * 8 + 15) & ~(size_t)15;
    if (cap < seg_bytes + 32) FAIL(MFR_JPEG_CAPACITY);
    /* entropy-coded data: unstuff, split at RSTn */
    uint32_t *seg = (uint32_t *)out;
    uint8_t *d = out + seg_bytes;
    size_t dcap = cap - seg_bytes - 32, o = 0;
    int nseg = 1, done = 0;
    seg[0] = 0;
    while (i < n) {
        uint8_t b = buf[i];
        if (b != 0xFF) {
            if (o >= dcap) FAIL(MFR_JPEG_CAPACITY);
            d[o++] = b;
            ++i;
            continue;
        }
        if (i + 1 >= n) FAIL(MFR_JPEG_INVALID);
        uint8_t m = buf[i + 1];
        if (m == 0x00) {
            if (o >= dcap) FAIL(MFR_JPEG_CAPACITY);
            d[o++] = 0xFF;
            i += 2;
        } else if (m == 0xFF) {
            ++i;                                                         /* fill byte before a marker */
        } else if (m >= 0xD0 && m <= 0xD7) {
            if (ri == 0 || nseg >= nseg_expect || (m & 7) != ((nseg - 1) & 7)) FAIL(MFR_JPEG_INVALID);
            seg[2 * nseg] = (uint32_t)o;
            ++nseg;
            i += 2;
        } else {
            done = 1;
            break;
        }
    }
    if (!done || nseg != nseg_expect) FAIL(MFR_JPEG_INVALID);
    /* after the scan: a second SOS is a multi-scan file; anything but EOI, DNL or skippable segments before it is malformed */
    for (;;) {
        while (i < n && buf[i] == 0xFF) ++i;
        if (i >= n) FAIL(MFR_JPEG_INVALID);
        int m = buf[i++];
        if (m == 0xD9) break;
        if (m == 0xDA || m == 0xDC) FAIL(MFR_JPEG_UNSUPPORTED);
        if ((m >= 0xD0 && m <= 0xD8) || m == 0x00 || m == 0x01) FAIL(MFR_JPEG_INVALID);
        int len = rd16(buf, n, i);
        if (len < 2 || i + (size_t)len > n) FAIL(MFR_JPEG_INVALID);
        i += (size_t)len;
        if (i >= n || buf[i] != 0xFF) FAIL(MFR_JPEG_INVALID);
    }
    for (int k = 0; k < nseg; ++k) {
        uint32_t end = k + 1 < nseg ? seg[2 * k + 2] : (uint32_t)o;
        if (end <= seg[2 * k]) FAIL(MFR_JPEG_INVALID);                   /* an empty restart segment */
        seg[2 * k + 1] = (uint32_t)(k + 1 < nseg || ri == 0 ? (ri ? ri : h->total_mcus) : h->total_mcus - ri * (nseg - 1));
    }
    size_t rec = (seg_bytes + o + 8 + 15) & ~(size_t)15;
    memset(d + o, 0, rec - seg_bytes - o);
    h->nseg = nseg;
    h->seg_table_bytes = (int32_t)seg_bytes;
    h->data_bytes = (int32_t)o;
    h->record_bytes = (int32_t)rec;
    *rec_bytes = rec;
#undef FAIL
    return MFR_JPEG_OK;
}

/* worst-case record size of a file of n bytes with up to nseg restart segments */
size_t mfr_host_jpeg_record_bound(size_t n, int nseg) { return (((size_t)nseg * 8 + 15) & ~(size_t)15) + n + 48; }
size_t mfr_host_jpeg_header_bytes(void) { return sizeof(mfr_jpeg_header); }

/* ---- 16-bit gray PNG: chunk walk + IDAT concatenation for the device decoder (csrc/png.hip) ----
 * PNG 1.2: signature 3.1, chunk layout 3.2, IHDR 4.1.1, IDAT 4.1.3 (consecutive), IEND 4.1.4; the zlib header RFC 1950 2.2.
 * Chunk CRCs are NOT verified (the stream's Adler-32 is, on the device).  Ancillary chunks are skipped; trailing bytes after IEND are
 * ignored.  Every read is bounded by n, every write by cap.  Layout: include/mfr_png.h. */
#include "mfr_png.h"

static uint32_t be32at(const uint8_t *b) { return ((uint32_t)b[0] << 24) | ((uint32_t)b[1] << 16) | ((uint32_t)b[2] << 8) | b[3]; }

/* buf[0..n) -> *h and the record out[0..cap); *rec_bytes = the record's size.  Returns MFR_PNG_OK / _UNSUPPORTED / _INVALID / _CAPACITY
 * (also in h->status).  Two walks over the chunks: the first validates and sizes, the second copies. */
int mfr_host_png_parse(const uint8_t *buf, size_t n, mfr_png_header *h, uint8_t *out, size_t cap, size_t *rec_bytes)
{
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    memset(h, 0, sizeof(*h));
    *rec_bytes = 0;
#define FAIL(code) do { h->status = (code); return (code); } while (0)
    if (n < 8 || memcmp(buf, sig, 8)) FAIL(MFR_PNG_INVALID);
    size_t pos = 8, first_idat = 0, stream = 0;
    int idat = 0, end = 0, first = 1;                                    /* idat: 0 none yet, 1 inside the run, 2 the run is over */
    uint8_t zh[2] = {0, 0};                                              /* the stream's first two bytes (they may lie in two chunks) */
    while (!end) {
        if (n - pos < 12) FAIL(MFR_PNG_INVALID);
        const uint32_t len = be32at(buf + pos);
        const uint8_t *type = buf + pos + 4;
        if (len > 0x7FFFFFFFu || (size_t)len > n - pos - 12) FAIL(MFR_PNG_INVALID);
        const uint8_t *d = buf + pos + 8;
        if (first) {
            if (memcmp(type, "IHDR", 4) || len != 13) FAIL(MFR_PNG_INVALID);
            const uint32_t w = be32at(d), ht = be32at(d + 4);
            if (w == 0 || ht == 0 || w > 0x7FFFFFFFu || ht > 0x7FFFFFFFu) FAIL(MFR_PNG_INVALID);
            const int bd = d[8], ct = d[9];
            const int ok = ct == 0 ? (bd == 1 || bd == 2 || bd == 4 || bd == 8 || bd == 16)
                         : ct == 3 ? (bd == 1 || bd == 2 || bd == 4 || bd == 8)
                         : (ct == 2 || ct == 4 || ct == 6) ? (bd == 8 || bd == 16) : 0;
            if (!ok || d[10] != 0 || d[11] != 0 || d[12] > 1) FAIL(MFR_PNG_INVALID);
            h->width = (int32_t)w; h->height = (int32_t)ht; h->bit_depth = bd; h->color_type = ct; h->interlace = d[12];
            first = 0;
        } else if (!memcmp(type, "IHDR", 4)) {
            FAIL(MFR_PNG_INVALID);
        } else if (!memcmp(type, "IDAT", 4)) {
            if (idat == 2) FAIL(MFR_PNG_INVALID);                        /* another chunk between two IDATs */
            if (idat == 0) first_idat = pos;
            idat = 1;
            for (uint32_t k = 0; k < len && stream + k < 2; ++k) zh[stream + k] = d[k];
            stream += len;
            if (stream > 0x7FFFFFFFu) FAIL(MFR_PNG_INVALID);
        } else if (!memcmp(type, "IEND", 4)) {
            if (idat == 0 || len != 0) FAIL(MFR_PNG_INVALID);
            end = 1;
        } else {
            if (idat == 1) idat = 2;
            if (!(type[0] & 0x20) && memcmp(type, "PLTE", 4)) FAIL(MFR_PNG_INVALID);   /* an unknown critical chunk */
        }
        pos += 12 + (size_t)len;
    }
    if (stream < 2 || (zh[0] & 15) != 8 || ((zh[0] << 8) | zh[1]) % 31 != 0) FAIL(MFR_PNG_INVALID);
    if (h->color_type != 0 || h->bit_depth != 16 || h->interlace != 0) FAIL(MFR_PNG_UNSUPPORTED);
    if ((zh[0] >> 4) > 7 || (zh[1] & 0x20)) FAIL(MFR_PNG_UNSUPPORTED);   /* window above 32 KiB, preset dictionary */
    const size_t rec = (stream + 8 + 15) & ~(size_t)15;
    if (cap < rec) FAIL(MFR_PNG_CAPACITY);
    size_t o = 0;
    for (pos = first_idat; o < stream; ) {                               /* the run was validated above: consecutive, inside [0, n) */
        const uint32_t len = be32at(buf + pos);
        memcpy(out + o, buf + pos + 8, len);
        o += len;
        pos += 12 + (size_t)len;
    }
    memset(out + o, 0, rec - o);
    h->stream_bytes = (int32_t)stream;
    h->record_bytes = (int32_t)rec;
    *rec_bytes = rec;
#undef FAIL
    return MFR_PNG_OK;
}

/* record size of a file of n bytes (always enough: the stream is shorter than the file) */
size_t mfr_host_png_record_bound(size_t n) { return (n + 8 + 15) & ~(size_t)15; }
size_t mfr_host_png_header_bytes(void) { return sizeof(mfr_png_header); }
