// png.hip -- 16-bit gray (millimetre depth) PNG decode on gfx950: the loaders' depth plane of a file, bit for bit what
// datasets.read_depth_plane gives: float32(uint16 / 1000.0).
//
// The host walks the chunks (csrc/host_decode.c mfr_host_png_parse) into a fixed-size header and a record (include/mfr_png.h): the
// zlib stream of the joined IDAT payloads plus >= 8 zero bytes.  One launch covers the n images of a batch, one wavefront (= one
// workgroup) per image, on the caller's stream, no host synchronisation.  Stages (the table is in png_ops.py's docstring):
//   inflate   RFC 1950 / 1951.  The symbol stream is serial, so the wavefront runs it in lock step: every value of the decoder's state
//             (bit buffer, positions, the symbol) is wave-uniform; the lanes share the loads and stores.  The bit buffer is 64 bits,
//             refilled 32 at a time from 64 dwords the lanes hold in registers (one coalesced 256-byte load per 2048 bits).  The
//             literal / length, distance and code-length codes are LDS tables built by the lanes together (one lane per symbol): a look-up of FAST bits
//             -> (length << 9) | symbol, and for longer codes the canonical count / symbol lists.  Literals collect one per lane and
//             leave as one store; an LZ77 match of length L is copied by lanes i < L as out[pos + i] = out[pos - dist + i % dist], which
//             reads only bytes below pos (so distances smaller than the length need no special case).
//   check     the stream must inflate to exactly H (1 + 2 W) bytes; Adler-32 of them as a lane-parallel sum (a = 1 + sum d_i,
//             b = n + sum (n - i) d_i, mod 65521); every row's filter byte <= 4.  Only then is the output plane touched.
//   unfilter  PNG filters 0-4 at 2 bytes per pixel.  Lane l takes row 64 p + l and runs l pixels behind lane l - 1, so the row above's
//             pixel (b) and the one before it (c) are what lane l - 1 produced one and two steps ago: two lane shifts.  Lane 0 reads
//             them from the scratch, where lane 63 of the previous pass wrote its unfiltered row.  The five predictors are computed
//             branch-free and selected on the row's filter byte.  The big-endian sample v leaves as (float)((double)v / 1000.0): the
//             IEEE f64 quotient then one rounding to f32, as numpy's uint16 / 1000.0 then astype(float32).
// Every loop is bounded: a symbol consumes >= 1 bit and the bits consumed are compared with the stream's length after every symbol
// (beyond the stream the reader supplies zeros and never loads); no store goes at or past H (1 + 2 W).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mfr_hip.h"
#include "wave_dev.h"
#include "../../include/mfr_png.h"

#define PNG_LL_FAST 10              // look-up bits of the literal / length code
#define PNG_D_FAST 9                // of the distance code
#define PNG_CL_FAST 7               // of the code-length code (its codes are at most 7 bits: always a hit or an unassigned code)

using mfr::lane_id;

struct PngHuff {                    // one canonical code: fast[low bits of the stream] = (len << 9) | symbol, 0 = longer or unassigned
    uint16_t *fast;
    uint16_t *sym;                  // the symbols ordered by (length, value)
    uint16_t *count;                // [16] number of codes per length
    int fast_bits;
};

struct PngLds {
    uint16_t ll_fast[1 << PNG_LL_FAST], d_fast[1 << PNG_D_FAST], cl_fast[1 << PNG_CL_FAST];
    uint16_t ll_sym[288], d_sym[32], cl_sym[32];
    uint16_t ll_count[16], d_count[16], cl_count[16];
    uint8_t lens[288 + 32];
    uint8_t cl_lens[32];
};

MFR_DEV uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// ---------------------------------------------------------------------------------------------------------------------------
// bit reader: LSB first.  All fields but `chunk` are wave-uniform.
struct PngBits {
    const uint32_t *rec;            // the record, 4-byte aligned
    uint32_t nwords;                // dwords that hold stream bytes; beyond them the reader supplies zeros
    uint32_t total_bits;            // 8 * stream_bytes
    uint32_t chunk;                 // lane l: dword wbase + l
    uint32_t wbase, widx;           // first dword of the chunk, next dword to enter the buffer
    uint64_t buf;
    int cnt;                        // valid bits in buf
    uint32_t used;                  // bits consumed since the stream's start
};

MFR_DEV void bits_load(PngBits &b)
{
    const uint32_t i = b.wbase + (uint32_t)lane_id();
    b.chunk = i < b.nwords ? b.rec[i] : 0u;
}
// at least 33 valid bits afterwards
MFR_DEV void bits_refill(PngBits &b)
{
    if (b.cnt <= 32) {
        if (b.widx - b.wbase >= 64u) { b.wbase = b.widx; bits_load(b); }
        const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)b.chunk, (int)(b.widx - b.wbase));
        b.buf |= (uint64_t)w << b.cnt;
        b.cnt += 32;
        ++b.widx;
    }
}
MFR_DEV void bits_drop(PngBits &b, int n) { b.buf >>= n; b.cnt -= n; b.used += (uint32_t)n; }
MFR_DEV uint32_t bits_take(PngBits &b, int n)               // n <= 16, after a refill
{
    const uint32_t v = (uint32_t)b.buf & ((1u << n) - 1u);
    bits_drop(b, n);
    return v;
}
MFR_DEV void bits_seek(PngBits &b, uint32_t byte)
{
    b.wbase = b.widx = byte >> 2;
    bits_load(b);
    b.buf = 0; b.cnt = 0; b.used = (byte & ~3u) * 8u;
    bits_refill(b);
    bits_drop(b, (int)(byte & 3u) * 8);
}
MFR_DEV bool bits_over(const PngBits &b) { return b.used > b.total_bits; }

// ---------------------------------------------------------------------------------------------------------------------------
// canonical Huffman code from lens[0..n) (LDS), n <= 288.  One lane per symbol, 64 symbols a turn: 15 ballots give lane l the number of
// codes of length l (first pass) and every symbol its rank among those of its length (second pass), so each lane lists its own symbol and
// fills its own look-up entries.  Returns 0, or MFR_PNG_E_DATA for an over-subscribed set or an incomplete one (zlib's rule: an
// incomplete set passes only when no code is longer than 1 bit, and never for the code-length code).  Wave-uniform call.
MFR_DEV int huff_build(const PngHuff &h, const uint8_t *lens, int n, bool may_be_incomplete)
{
    const int lane = lane_id();
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int i = lane; i < (1 << h.fast_bits); i += 64) h.fast[i] = 0;
    int cnt = 0;                                                         // lane l (1..15): codes of length l
    for (int s0 = 0; s0 < n; s0 += 64) {
        const int l = s0 + lane < n ? lens[s0 + lane] : 0;
#pragma unroll
        for (int k = 1; k < 16; ++k) {
            const unsigned long long m = __ballot(l == k);
            if (lane == k) cnt += __popcll(m);
        }
    }
    if (lane < 16) h.count[lane] = (uint16_t)cnt;
    int first = 0, offs = 0, left = 1, my_first = 0, my_offs = 0, longer = 0;
    bool over = false;
#pragma unroll
    for (int l = 1; l < 16; ++l) {
        const int c = __shfl(cnt, l, 64);
        if (lane == l) { my_first = first; my_offs = offs; }
        offs += c;
        first = (first + c) << 1;
        left = (left << 1) - c;
        over |= left < 0;
        if (l > 1) longer += c;
    }
    __syncthreads();                                                     // fast[] zeroed before any entry is written
    if (!over) {
        int run = 0;                                                     // lane l: symbols of length l listed by earlier turns
        for (int s0 = 0; s0 < n; s0 += 64) {
            const int s = s0 + lane;
            const int l = s < n ? lens[s] : 0;
            int rank = 0;
#pragma unroll
            for (int k = 1; k < 16; ++k) {
                const unsigned long long m = __ballot(l == k);
                const int r = __shfl(run, k, 64);
                if (l == k) rank = r + __popcll(m & below);
                if (lane == k) run += __popcll(m);
            }
            const int fl = __shfl(my_first, l, 64), ol = __shfl(my_offs, l, 64);
            if (l) {
                h.sym[ol + rank] = (uint16_t)s;
                if (l <= h.fast_bits) {
                    const uint32_t rev = __brev((uint32_t)(fl + rank)) >> (32 - l);
                    const uint16_t e = (uint16_t)((l << 9) | s);
                    for (uint32_t f = rev; f < (1u << h.fast_bits); f += 1u << l) h.fast[f] = e;
                }
            }
        }
    }
    __syncthreads();
    if (over) return MFR_PNG_E_DATA;
    if (left > 0 && offs > 0 && !(may_be_incomplete && longer == 0)) return MFR_PNG_E_DATA;
    return 0;
}

// one symbol (after a refill: >= 15 valid bits), or -1 for an unassigned code
MFR_DEV int huff_decode(PngBits &b, const PngHuff &h)
{
    const uint32_t e = uni(h.fast[(uint32_t)b.buf & ((1u << h.fast_bits) - 1u)]);
    if (e) {
        bits_drop(b, (int)(e >> 9));
        return (int)(e & 511u);
    }
    int code = 0, first = 0, index = 0;
    for (int len = 1; len < 16; ++len) {
        code |= (int)((b.buf >> (len - 1)) & 1u);
        const int c = (int)uni(h.count[len]);
        if (code - c < first) {
            bits_drop(b, len);
            return (int)uni(h.sym[index + (code - first)]);
        }
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    return -1;
}

// the code lengths of a dynamic block (RFC 1951 3.2.7) and its two codes
MFR_DEV int dynamic_header(PngBits &b, PngLds &S, const PngHuff &ll, const PngHuff &d, const PngHuff &cl)
{
    const int lane = lane_id();
    bits_refill(b);
    const int nlen = (int)bits_take(b, 5) + 257, ndist = (int)bits_take(b, 5) + 1, ncode = (int)bits_take(b, 4) + 4;
    if (nlen > 286 || ndist > 30) return MFR_PNG_E_DATA;
    if (lane < 32) S.cl_lens[lane] = 0;
    __syncthreads();
    // 16 17 18 0 8 7 9 6 10 5 11 4 | 12 3 13 2 14 1 15, 5 bits each
    const uint64_t order_lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 |
                              5ull << 45 | 11ull << 50 | 4ull << 55;
    const uint64_t order_hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    for (int i = 0; i < ncode; ++i) {
        bits_refill(b);
        const uint32_t v = bits_take(b, 3);
        const int o = (int)((i < 12 ? order_lo >> (5 * i) : order_hi >> (5 * (i - 12))) & 31u);
        if (lane == 0) S.cl_lens[o] = (uint8_t)v;
    }
    if (bits_over(b)) return MFR_PNG_E_TRUNC;
    __syncthreads();
    if (huff_build(cl, S.cl_lens, 19, false)) return MFR_PNG_E_DATA;
    int idx = 0, prev = 0;
    const int total = nlen + ndist;
    while (idx < total) {                                                // every turn consumes >= 1 bit or fails
        bits_refill(b);
        const int s = huff_decode(b, cl);
        if (bits_over(b)) return MFR_PNG_E_TRUNC;
        if (s < 0) return MFR_PNG_E_DATA;
        if (s < 16) {
            if (lane == 0) S.lens[idx] = (uint8_t)s;
            prev = s;
            ++idx;
            continue;
        }
        int rep, val = 0;
        if (s == 16) {
            if (idx == 0) return MFR_PNG_E_DATA;
            val = prev;
            rep = 3 + (int)bits_take(b, 2);
        } else if (s == 17) {
            rep = 3 + (int)bits_take(b, 3);
        } else {
            rep = 11 + (int)bits_take(b, 7);
        }
        if (bits_over(b)) return MFR_PNG_E_TRUNC;
        if (idx + rep > total) return MFR_PNG_E_DATA;
        for (int i = lane; i < rep; i += 64) S.lens[idx + i] = (uint8_t)val;
        prev = val;
        idx += rep;
    }
    __syncthreads();
    if (uni(S.lens[256]) == 0) return MFR_PNG_E_DATA;                    // no end-of-block code
    // the distance lengths follow the literal / length ones: the codes read them in place
    if (huff_build(ll, S.lens, nlen, true)) return MFR_PNG_E_DATA;
    if (huff_build(d, S.lens + nlen, ndist, true)) return MFR_PNG_E_DATA;
    return 0;
}

MFR_DEV void fixed_tables(PngLds &S, const PngHuff &ll, const PngHuff &d)
{
    for (int i = lane_id(); i < 288 + 32; i += 64) S.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5);
    __syncthreads();
    huff_build(ll, S.lens, 288, true);
    huff_build(d, S.lens + 288, 30, true);
}

// the pending literals (lane k holds the k-th) leave as one store
MFR_DEV void flush_literals(uint8_t *out, uint32_t &pos, int &npend, uint32_t pend)
{
    if (lane_id() < npend) out[pos + (uint32_t)lane_id()] = (uint8_t)pend;
    pos += (uint32_t)npend;
    npend = 0;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
}

// inflate the record into out[0..total).  Returns 0 or a status; *end_byte = the byte after the final block (where the Adler-32 is)
MFR_DEV int inflate_stream(PngBits &b, PngLds &S, uint8_t *out, uint32_t total, uint32_t stream_bytes, uint32_t *end_byte)
{
    const int lane = lane_id();
    const PngHuff ll = {S.ll_fast, S.ll_sym, S.ll_count, PNG_LL_FAST}, d = {S.d_fast, S.d_sym, S.d_count, PNG_D_FAST},
                  cl = {S.cl_fast, S.cl_sym, S.cl_count, PNG_CL_FAST};
    uint32_t pos = 0;
    bool fixed_ready = false;                                            // the LDS tables hold the fixed codes
    bits_seek(b, 0);
    bits_refill(b);
    const uint32_t cmf = bits_take(b, 8), flg = bits_take(b, 8);
    if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || (flg & 0x20u) || ((cmf << 8) | flg) % 31u != 0u) return MFR_PNG_E_DATA;
    for (;;) {                                                           // blocks: each consumes >= 3 bits
        bits_refill(b);
        const uint32_t bfinal = bits_take(b, 1), btype = bits_take(b, 2);
        if (bits_over(b)) return MFR_PNG_E_TRUNC;
        if (btype == 3u) return MFR_PNG_E_DATA;
        if (btype == 0u) {
            const uint32_t at = (b.used + 7u) >> 3;                      // LEN, NLEN at the next byte boundary
            if (at + 4u > stream_bytes) return MFR_PNG_E_TRUNC;
            bits_seek(b, at);
            bits_refill(b);
            const uint32_t len = bits_take(b, 16);
            bits_refill(b);
            const uint32_t nlen = bits_take(b, 16);
            if ((len ^ 0xFFFFu) != nlen) return MFR_PNG_E_DATA;
            if (at + 4u + len > stream_bytes) return MFR_PNG_E_TRUNC;
            if (len > total - pos) return MFR_PNG_E_SIZE;
            const uint8_t *src = (const uint8_t *)b.rec + at + 4u;
            for (uint32_t i = (uint32_t)lane; i < len; i += 64u) out[pos + i] = src[i];
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            pos += len;
            bits_seek(b, at + 4u + len);
        } else {
            if (btype == 1u) {
                if (!fixed_ready) fixed_tables(S, ll, d);                // (consecutive fixed blocks share one build)
                fixed_ready = true;
            } else {
                fixed_ready = false;
                const int e = dynamic_header(b, S, ll, d, cl);
                if (e) return e;
            }
            int npend = 0;
            uint32_t pend = 0;
            for (;;) {                                                   // symbols: each consumes >= 1 bit
                bits_refill(b);
                const int sym = huff_decode(b, ll);
                if (bits_over(b)) return MFR_PNG_E_TRUNC;
                if (sym < 0) return MFR_PNG_E_DATA;
                if (sym < 256) {
                    if (pos + (uint32_t)npend >= total) return MFR_PNG_E_SIZE;
                    if (lane == npend) pend = (uint32_t)sym;
                    if (++npend == 64) flush_literals(out, pos, npend, pend);
                    continue;
                }
                if (sym == 256) break;
                const int ls = sym - 257;
                if (ls >= 29) return MFR_PNG_E_DATA;
                // length 3.. : codes 257-264 one value each, then groups of four with e extra bits, 285 = 258
                const int le = ls < 8 || ls == 28 ? 0 : (ls - 4) >> 2;
                const uint32_t lbase = ls < 8 ? 3u + (uint32_t)ls : ls == 28 ? 258u : 3u + ((4u + ((uint32_t)ls & 3u)) << le);
                const uint32_t len = lbase + bits_take(b, le);
                bits_refill(b);
                const int ds = huff_decode(b, d);
                if (ds < 0 || ds >= 30) return bits_over(b) ? MFR_PNG_E_TRUNC : MFR_PNG_E_DATA;
                const int de = ds < 4 ? 0 : (ds - 2) >> 1;
                const uint32_t dbase = ds < 4 ? 1u + (uint32_t)ds : 1u + ((2u + ((uint32_t)ds & 1u)) << de);
                const uint32_t dist = dbase + bits_take(b, de);
                if (bits_over(b)) return MFR_PNG_E_TRUNC;
                flush_literals(out, pos, npend, pend);
                if (dist > pos) return MFR_PNG_E_DATA;
                if (len > total - pos) return MFR_PNG_E_SIZE;
                const uint8_t *from = out + (pos - dist);
                for (uint32_t i = (uint32_t)lane; i < len; i += 64u) out[pos + i] = from[i < dist ? i : i % dist];
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                pos += len;
            }
            flush_literals(out, pos, npend, pend);
        }
        if (bfinal) break;
    }
    if (pos != total) return MFR_PNG_E_SIZE;
    *end_byte = (b.used + 7u) >> 3;
    return 0;
}

// Adler-32 of d[0..n), n < 2^31, d 4-byte aligned.  Lane sums in 64 bits, reduced mod 65521 before they can overflow.
MFR_DEV uint32_t adler32_wave(const uint8_t *d, uint32_t n)
{
    const uint32_t lane = (uint32_t)lane_id(), nw = n >> 2;
    const uint32_t *d32 = (const uint32_t *)d;
    uint64_t s1 = 0, s2 = 0;
    uint32_t turns = 0;
    for (uint32_t w = lane; w < nw; w += 64u) {
        const uint32_t v = d32[w];
        const uint32_t b0 = v & 255u, b1 = (v >> 8) & 255u, b2 = (v >> 16) & 255u, b3 = v >> 24;
        const uint64_t k = (uint64_t)(n - 4u * w);                       // weight of byte 4 w
        s1 += b0 + b1 + b2 + b3;
        s2 += k * b0 + (k - 1) * b1 + (k - 2) * b2 + (k - 3) * b3;       // < 2^31 * 1020 < 2^41 per turn
        if (++turns == (1u << 20)) { s2 %= 65521u; turns = 0; }
    }
    const uint32_t i = 4u * nw + lane;
    if (i < n) { s1 += d[i]; s2 += (uint64_t)(n - i) * d[i]; }
    s1 %= 65521u; s2 %= 65521u;
    uint32_t a = (uint32_t)s1, c = (uint32_t)s2;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { a += __shfl_xor(a, off, 64); c += __shfl_xor(c, off, 64); }   // < 64 * 65521
    a = (1u + a) % 65521u;
    c = (n % 65521u + c) % 65521u;
    return (c << 16) | a;
}

MFR_DEV uint32_t paeth(uint32_t a, uint32_t b, uint32_t c)
{
    const int p = (int)a + (int)b - (int)c;
    const int pa = abs(p - (int)a), pb = abs(p - (int)b), pc = abs(p - (int)c);
    return pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
}

// scr: H rows of 1 + 2 W bytes, every filter byte <= 4 -> out [H, W] f32.  See the file's head.
MFR_DEV void unfilter_convert(uint8_t *scr, int H, int W, float *out)
{
    const int lane = lane_id();
    const size_t stride = 1 + 2 * (size_t)W;
    for (int p0 = 0; p0 < H; p0 += 64) {
        const int row = p0 + lane;
        const bool live = row < H;
        const uint8_t *raw = scr + (size_t)(live ? row : 0) * stride;
        const int ft = live ? raw[0] : 0;
        const uint8_t *above = p0 > 0 ? scr + (size_t)(p0 - 1) * stride + 1 : nullptr;    // lane 0's row above (unfiltered by the last pass)
        uint8_t *keep = (lane == 63 && live) ? scr + (size_t)row * stride + 1 : nullptr;  // the next pass's row above
        uint32_t a = 0, pa = 0;                                          // this lane's last two outputs: hi byte | lo byte << 8
        uint32_t b0_prev = 0;                                            // lane 0: the row above's previous pixel
        for (int t = 0; t < W + 63; ++t) {
            const int x = t - lane;
            const bool on = live && x >= 0 && x < W;
            uint32_t b = (uint32_t)__shfl_up((int)a, 1, 64), c = (uint32_t)__shfl_up((int)pa, 1, 64);
            if (lane == 0) {
                c = b0_prev;
                b = (above && x < W) ? (uint32_t)above[2 * x] | (uint32_t)above[2 * x + 1] << 8 : 0u;
                b0_prev = b;
            }
            uint32_t r = 0;
            if (on) r = (uint32_t)raw[1 + 2 * x] | (uint32_t)raw[2 + 2 * x] << 8;
            const uint32_t a0 = a & 255u, a1 = a >> 8, b0 = b & 255u, b1 = b >> 8, c0 = c & 255u, c1 = c >> 8;
            const uint32_t p0v = ft == 1 ? a0 : ft == 2 ? b0 : ft == 3 ? (a0 + b0) >> 1 : ft == 4 ? paeth(a0, b0, c0) : 0u;
            const uint32_t p1v = ft == 1 ? a1 : ft == 2 ? b1 : ft == 3 ? (a1 + b1) >> 1 : ft == 4 ? paeth(a1, b1, c1) : 0u;
            const uint32_t o = (((r & 255u) + p0v) & 255u) | ((((r >> 8) + p1v) & 255u) << 8);
            pa = a;
            a = on ? o : 0u;
            if (on) {
                const uint32_t v = ((o & 255u) << 8) | (o >> 8);
                out[(size_t)row * W + x] = (float)((double)v / 1000.0);
                if (keep) { keep[2 * x] = (uint8_t)(o & 255u); keep[2 * x + 1] = (uint8_t)(o >> 8); }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    }
}

__global__ __launch_bounds__(64) void png_depth_kernel(const mfr_png_header *hdrs, const uint8_t *records, const long long *offsets, int H, int W,
                                                       long long max_record, uint8_t *scratch, size_t scratch_stride, float *out, int *status)
{
    __shared__ PngLds S;
    const int img = blockIdx.x, lane = lane_id();
    const mfr_png_header h = hdrs[img];
    if (h.status != MFR_PNG_OK) {                                        // the host's verdict passes through; the plane stays as it was
        if (lane == 0) status[img] = h.status;
        return;
    }
    const long long o0 = offsets[img], o1 = offsets[img + 1];
    const uint32_t total = (uint32_t)H * (1u + 2u * (uint32_t)W);
    int st = 0;
    if (h.width != W || h.height != H || h.bit_depth != 16 || h.color_type != 0 || h.interlace != 0) st = MFR_PNG_E_SIZE;
    else if (o0 < 0 || (o0 & 15) != 0 || h.stream_bytes < 2 || (long long)h.stream_bytes + 8 > o1 - o0 || (long long)h.stream_bytes > max_record)
        st = MFR_PNG_E_SIZE;
    uint8_t *scr = scratch + (size_t)img * scratch_stride;
    if (!st) {
        PngBits b;
        b.rec = (const uint32_t *)(records + o0);
        b.nwords = ((uint32_t)h.stream_bytes + 3u) >> 2;
        b.total_bits = (uint32_t)h.stream_bytes * 8u;
        uint32_t end_byte = 0;
        st = inflate_stream(b, S, scr, total, (uint32_t)h.stream_bytes, &end_byte);
        if (!st) {
            if (end_byte + 4u > (uint32_t)h.stream_bytes) {
                st = MFR_PNG_E_TRUNC;
            } else {
                const uint8_t *t = records + o0 + end_byte;
                const uint32_t want = (uint32_t)t[0] << 24 | (uint32_t)t[1] << 16 | (uint32_t)t[2] << 8 | (uint32_t)t[3];
                if (adler32_wave(scr, total) != want) st = MFR_PNG_E_CHECK;
            }
        }
        if (!st) {
            bool bad = false;
            for (int r = lane; r < H; r += 64) bad |= scr[(size_t)r * (1 + 2 * (size_t)W)] > 4;
            if (__any(bad)) st = MFR_PNG_E_DATA;
        }
    }
    st = (int)uni((uint32_t)st);
    if (lane == 0) status[img] = st;
    if (st) return;
    unfilter_convert(scr, H, W, out + (size_t)img * H * W);
}

static int png_args(int n, int H, int W, size_t *stride)
{
    if (n <= 0 || H <= 0 || W <= 0 || H > 65535 || W > 65535) return -1;
    const long long total = (long long)H * (1 + 2 * (long long)W);
    if (total >= (1ll << 31)) return -1;
    *stride = mfr::align_up((size_t)total, 256);
    return 0;
}

extern "C" size_t mfr_png_depth_workspace_bytes(int n, int H, int W)
{
    size_t stride;
    if (png_args(n, H, W, &stride) != 0) return 0;
    return stride * (size_t)n;
}

extern "C" int mfr_png_depth_decode(const void *headers, const uint8_t *records, const long long *offsets, int n, int H, int W,
                                    long long max_record_bytes, void *scratch, size_t scratch_bytes, float *out, int *status, void *stream)
{
    size_t stride;
    if (!headers || !records || !offsets || !scratch || !out || !status) return MFR_E_ARG;
    if (png_args(n, H, W, &stride) != 0 || max_record_bytes < 16 || max_record_bytes >= (1ll << 28)) return MFR_E_ARG;
    if (scratch_bytes < stride * (size_t)n) return MFR_E_WORKSPACE;
    hipLaunchKernelGGL(png_depth_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, (const mfr_png_header *)headers, records, offsets, H, W,
                       max_record_bytes, (uint8_t *)scratch, stride, out, status);
    CHECK_LAUNCH();
    return 0;
}
