// jpeg.hip -- baseline (sequential, Huffman, 8-bit) JPEG decode on gfx950: the loaders' gray plane of a file, bit for bit what
// PIL's RGB decode (libjpeg-turbo, libjpeg 6.2 API: JDCT_ISLOW, fancy upsampling) followed by datasets.luma_u8 and / 255f gives.
//
// The host parses the file (csrc/host_decode.c mfr_host_jpeg_parse) into a fixed-size header and a record (include/mfr_jpeg.h):
// the segment table and the unstuffed entropy-coded data.  Stages (every launch covers n images of one size, on the caller's
// stream, no host synchronisation; the stage table with every constant is in jpeg_ops.py's docstring):
//   entropy   one 1024-lane workgroup per image.  Each restart segment is cut into subsequences of S bits; every subsequence
//             is decoded speculatively from a guessed state (bit offset, zig-zag index k, block-in-MCU index j) up to the
//             first symbol that starts past its end, and re-decoded from its predecessor's exit state until no start state
//             changes (Weissenberger & Schmidt, "Massively Parallel Huffman Decoding on GPUs", 2018).  After round r the first
//             r + 1 subsequences of every segment start correctly, so the loop reaches its fixed point in at most nsub rounds
//             and the result does not depend on how fast the code resynchronises.  An exclusive scan of the blocks each
//             subsequence completes places it; a final pass writes the int16 coefficients (DC as differences), stopping at the
//             segment's MCU count.  Then the per-component DC prediction: a segmented prefix sum, reset at restart segments.
//   idct      dequantise + libjpeg's JDCT_ISLOW (CONST_BITS 13, PASS1_BITS 2) + the clamp of its output to [-128, 127], 8 lanes per block
//             (pass 1 one column per lane, pass 2 one row per lane), into u8 component planes padded to whole MCUs
//   colour    one lane per pixel: fancy (triangle) upsampling of the chroma (h2v1, h2v2), fixed-point YCbCr -> RGB, luma
//             (19595 R + 38470 G + 7471 B + 2^15) >> 16, / 255f into the [n,1,H,W] f32 batch (and optionally RGB u8)
// Integer arithmetic throughout (no MFMA): every value equals libjpeg's.  Every loop is bounded; every read of a record is
// bounded by its data length plus the >= 8 zero bytes the parse appends.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mfr_hip.h"
#include "wave_dev.h"
#include "../../include/mfr_jpeg.h"

#define JE_THREADS 1024             // entropy workgroup: one image
#define JE_WAVES (JE_THREADS / 64)
#define JE_SMIN 64                  // default subsequence length: max(JE_SMIN, bits / JE_THREADS rounded up to 32)
#define JE_SENTINEL 0xFFFFFFFFFFFFFFFFull

__constant__ uint8_t c_zz[64] = {
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct JpegLayout {
    long long stride;               // bytes per image
    long long coef, planes, start, exitv, nblk, subseg, changed, segfirst, segdone;   // byte offsets inside an image's area
    int blocks_max, nsub_max, segs_max;
    long long max_record;
};

static long long al256(long long x) { return (x + 255) & ~255ll; }

static int jpeg_layout(int n, int H, int W, long long max_record, int S, JpegLayout *L)
{
    if (n <= 0 || H <= 0 || W <= 0 || H > 65535 || W > 65535 || max_record < 16 || (S != 0 && S < 16)) return -1;
    long long bx8 = (W + 7) / 8, by8 = (H + 7) / 8, bx16 = (W + 15) / 16, by16 = (H + 15) / 16;
    long long b = 3 * bx8 * by8;
    if (4 * bx16 * by8 > b) b = 4 * bx16 * by8;
    if (6 * bx16 * by16 > b) b = 6 * bx16 * by16;
    if (b > (1ll << 26)) return -1;
    long long segs = b;                                        // a segment holds >= 1 MCU
    long long bits = 8 * max_record;
    long long nsub = (S == 0 ? (long long)JE_THREADS : (bits + S - 1) / S) + segs;
    if (nsub > (1ll << 28)) return -1;
    L->blocks_max = (int)b; L->segs_max = (int)segs; L->nsub_max = (int)nsub; L->max_record = max_record;
    long long o = 0;
    L->coef = o; o = al256(o + b * 128);
    L->planes = o; o = al256(o + b * 64);
    L->start = o; o = al256(o + nsub * 8);
    L->exitv = o; o = al256(o + nsub * 8);
    L->nblk = o; o = al256(o + nsub * 4);
    L->subseg = o; o = al256(o + nsub * 4);
    L->changed = o; o = al256(o + nsub);
    L->segfirst = o; o = al256(o + (segs + 1) * 4);
    L->segdone = o; o = al256(o + segs * 4);
    L->stride = o;
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// entropy decode

struct HuffLds {
    uint16_t fast[4][1 << MFR_JPEG_FAST_BITS];   // tables 0, 1: DC; 2, 3: AC
    int maxcode[4][20], valoff[4][20];
    uint8_t val[4][256];
    int blk_dc[MFR_JPEG_MAX_BLOCKS_PER_MCU], blk_ac[MFR_JPEG_MAX_BLOCKS_PER_MCU];
    int scan_v[JE_WAVES], scan_f[JE_WAVES];
    int err, any;
};

// inclusive segmented scan over the workgroup (head flag f starts a new sum); `carry` enters before lane 0 (f = 0 there adds it);
// *next = the value at the last lane (the carry of the following chunk).  Every lane must call it (two barriers).
__device__ int wg_seg_scan(int v, int f, int carry, HuffLds &S, int *next)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int off = 1; off < 64; off <<= 1) {
        int v2 = __shfl_up(v, off, 64), f2 = __shfl_up(f, off, 64);
        if (lane >= off) {
            if (!f) v += v2;
            f |= f2;
        }
    }
    if (lane == 63) { S.scan_v[wave] = v; S.scan_f[wave] = f; }
    __syncthreads();
    int cv = carry;
    for (int w = 0; w < wave; ++w) cv = S.scan_f[w] ? S.scan_v[w] : cv + S.scan_v[w];
    if (!f) v += cv;
    int nc = carry;
    for (int w = 0; w < JE_WAVES; ++w) nc = S.scan_f[w] ? S.scan_v[w] : nc + S.scan_v[w];
    __syncthreads();
    *next = nc;
    return v;
}

__device__ __forceinline__ uint32_t be32(const uint8_t *d, uint32_t w)
{
    return __builtin_bswap32(*(const uint32_t *)(d + 4 * (size_t)w));
}

// 32 bits of the stream starting at bit p (MSB first)
__device__ __forceinline__ uint32_t peek32(const uint8_t *d, uint32_t p)
{
    uint32_t w = p >> 5, sh = p & 31;
    uint32_t hi = be32(d, w);
    return sh ? (hi << sh) | (be32(d, w + 1) >> (32 - sh)) : hi;
}

__device__ __forceinline__ uint64_t pack_state(uint32_t p, int k, int j) { return (uint64_t)p | ((uint64_t)k << 32) | ((uint64_t)j << 40); }

// Decode from state (p, k, j) every symbol that starts before `end`.  seg_end: the segment's bit length (no symbol may cross it).
// write: coefficients of block (blk_base + b) for b in [b0, limit), stopping at limit; *reached = 1 when block `limit` completes.
// Returns 0, MFR_JPEG_E_HUFF or MFR_JPEG_E_TRUNC (then the state is the sentinel).  Bounded: every symbol consumes >= 1 bit.
__device__ int decode_run(const uint8_t *d, const HuffLds &S, int bpm, uint32_t &p, int &k, int &j, uint32_t end, uint32_t seg_end,
                          int &nb, bool write, int16_t *coef, long long blk_base, int b0, int limit, int *reached)
{
    nb = 0;
    while (p < end) {
        if (write && b0 + nb >= limit) break;
        const int t = k == 0 ? S.blk_dc[j] : S.blk_ac[j];
        const uint32_t win = peek32(d, p);
        int len = 0, sym = 0;
        const uint16_t e = S.fast[t][win >> (32 - MFR_JPEG_FAST_BITS)];
        if (e) {
            len = e >> 8;
            sym = e & 255;
        } else {
            for (int l = MFR_JPEG_FAST_BITS + 1; l <= 16; ++l) {
                const int code = (int)(win >> (32 - l));
                if (code <= S.maxcode[t][l]) {
                    len = l;
                    sym = S.val[t][(code + S.valoff[t][l]) & 255];
                    break;
                }
            }
            if (!len) return MFR_JPEG_E_HUFF;
        }
        int r, s;
        if (k == 0) {
            if (sym > 15) return MFR_JPEG_E_HUFF;
            r = 0; s = sym;
        } else {
            r = sym >> 4; s = sym & 15;
        }
        if ((uint64_t)p + len + s > seg_end) return MFR_JPEG_E_TRUNC;
        if (s) {
            int v = (int)((win << len) >> (32 - s));
            if (v < (1 << (s - 1))) v -= (1 << s) - 1;
            k += r;
            if (write) coef[(blk_base + b0 + nb) * 64 + c_zz[k < 63 ? k : 63]] = (int16_t)v;
            k += 1;
        } else if (k == 0) {
            k = 1;                                            // DC difference 0
        } else if (r == 15) {
            k += 16;                                          // ZRL
        } else {
            k = 64;                                           // EOB
        }
        p += len + s;
        if (k >= 64) {
            k = 0;
            j = j + 1 == bpm ? 0 : j + 1;
            ++nb;
            if (write && b0 + nb == limit) *reached = 1;
        }
    }
    return 0;
}

__global__ __launch_bounds__(JE_THREADS) void jpeg_entropy_kernel(const mfr_jpeg_header *hdrs, const uint8_t *recs, const long long *offs,
                                                                  int H, int W, int S_req, JpegLayout L, uint8_t *ws, int *status, int *rounds)
{
    __shared__ HuffLds S;
    const int img = blockIdx.x, tid = threadIdx.x;
    const mfr_jpeg_header *h = hdrs + img;
    const long long off = offs[img], rec_len = offs[img + 1] - off;
    int st = h->status;
    const int bpm = h->blocks_per_mcu, nseg = h->nseg, ri = h->restart_interval;
    const long long nblocks = (long long)h->total_mcus * bpm;
    if (st == 0 && (h->width != W || h->height != H || h->record_bytes > rec_len || rec_len > L.max_record || (off & 15) ||
                    bpm < 1 || bpm > MFR_JPEG_MAX_BLOCKS_PER_MCU || nblocks > L.blocks_max || nseg < 1 || nseg > L.segs_max ||
                    nseg > h->total_mcus || h->seg_table_bytes < 8 * nseg || h->seg_table_bytes + h->data_bytes + 8 > h->record_bytes))
        st = MFR_JPEG_E_SIZE;
    if (st != 0) {
        if (tid == 0) { status[img] = st; if (rounds) rounds[img] = 0; }
        return;
    }
    uint8_t *base = ws + img * L.stride;
    int16_t *coef = (int16_t *)(base + L.coef);
    uint64_t *start = (uint64_t *)(base + L.start), *exitv = (uint64_t *)(base + L.exitv);
    uint32_t *nblk = (uint32_t *)(base + L.nblk), *subseg = (uint32_t *)(base + L.subseg), *segfirst = (uint32_t *)(base + L.segfirst);
    uint32_t *segdone = (uint32_t *)(base + L.segdone);
    uint8_t *changed = base + L.changed;
    const uint8_t *rec = recs + off;
    const uint32_t *segt = (const uint32_t *)rec;
    const uint8_t *d = rec + h->seg_table_bytes;
    const uint32_t data_bits = 8u * (uint32_t)h->data_bytes;

    // tables -> LDS, coefficients -> 0
    for (int i = tid; i < 4 * (1 << MFR_JPEG_FAST_BITS); i += JE_THREADS) {
        const int t = i >> MFR_JPEG_FAST_BITS, f = i & ((1 << MFR_JPEG_FAST_BITS) - 1);
        S.fast[t][f] = (t < 2 ? h->dc[t] : h->ac[t - 2]).fast[f];
    }
    for (int i = tid; i < 4 * 256; i += JE_THREADS) S.val[i >> 8][i & 255] = ((i >> 8) < 2 ? h->dc[i >> 8] : h->ac[(i >> 8) - 2]).val[i & 255];
    if (tid < 80) {
        const int t = tid / 20, l = tid % 20;
        const mfr_jpeg_huff &hu = t < 2 ? h->dc[t] : h->ac[t - 2];
        S.maxcode[t][l] = l >= 1 && l <= 16 ? hu.maxcode[l] : -1;
        S.valoff[t][l] = hu.valoff[l];
    }
    if (tid < bpm) {
        const int c = h->mcu_comp[tid];
        S.blk_dc[tid] = h->comp_td[c] & 1;
        S.blk_ac[tid] = 2 + (h->comp_ta[c] & 1);
    }
    if (tid == 0) S.err = 0;
    {
        int4 *c4 = (int4 *)coef;
        for (long long i = tid; i < nblocks * 8; i += JE_THREADS) c4[i] = make_int4(0, 0, 0, 0);
        for (int s = tid; s < nseg; s += JE_THREADS) segdone[s] = 0;
    }
    const int S_bits = S_req > 0 ? S_req : max(JE_SMIN, (int)(((data_bits + JE_THREADS - 1) / JE_THREADS + 31) & ~31u));

    // subsequences per segment and their exclusive scan
    auto seg_start = [&](int s) -> uint32_t { return 8u * segt[2 * s]; };
    auto seg_endb = [&](int s) -> uint32_t { return s + 1 < nseg ? 8u * segt[2 * s + 2] : data_bits; };
    int carry = 0;
    for (int b = 0; b < nseg; b += JE_THREADS) {
        const int s = b + tid;
        int cnt = 0;
        if (s < nseg) {
            const uint32_t a = seg_start(s), e = seg_endb(s);
            cnt = e > a ? (int)((e - a + S_bits - 1) / S_bits) : 0;
        }
        int nxt;
        const int inc = wg_seg_scan(cnt, 0, carry, S, &nxt);
        if (s < nseg) segfirst[s] = (uint32_t)(inc - cnt);
        carry = nxt;
    }
    const int nsub = carry;
    if (nsub > L.nsub_max || nsub < nseg) {                   // an empty segment, or more subsequences than the workspace holds
        if (tid == 0) { status[img] = nsub < nseg ? MFR_JPEG_INVALID : MFR_JPEG_E_SIZE; if (rounds) rounds[img] = 0; }
        return;
    }
    if (tid == 0) segfirst[nseg] = (uint32_t)nsub;
    __syncthreads();
    for (int s = tid; s < nseg; s += JE_THREADS)
        for (uint32_t q = segfirst[s]; q < segfirst[s + 1]; ++q) subseg[q] = (uint32_t)s;
    __syncthreads();
    for (int q = tid; q < nsub; q += JE_THREADS) {
        const int s = (int)subseg[q];
        start[q] = pack_state(seg_start(s) + (uint32_t)(q - (int)segfirst[s]) * (uint32_t)S_bits, 0, 0);
        changed[q] = 1;
    }
    __syncthreads();

    // the fixed point: at most nsub rounds (after round r the first r + 1 subsequences of every segment start right)
    int nround = 0;
    for (;;) {
        for (int q = tid; q < nsub; q += JE_THREADS) {
            if (!changed[q]) continue;
            changed[q] = 0;
            const uint64_t st0 = start[q];
            const int s = (int)subseg[q];
            const uint32_t a = seg_start(s) + (uint32_t)(q - (int)segfirst[s]) * (uint32_t)S_bits, e = seg_endb(s);
            const uint32_t end = min(e, a + (uint32_t)S_bits);
            uint32_t p = (uint32_t)st0;
            int k = (int)((st0 >> 32) & 0xFF), j = (int)(st0 >> 40), nb = 0, dummy = 0;
            const int rc = decode_run(d, S, bpm, p, k, j, end, e, nb, false, nullptr, 0, 0, 0, &dummy);
            exitv[q] = rc ? JE_SENTINEL : pack_state(p, k, j);
            nblk[q] = (uint32_t)nb;
        }
        __syncthreads();
        int any = 0;
        for (int q = tid; q < nsub; q += JE_THREADS) {
            const int s = (int)subseg[q];
            if (q == (int)segfirst[s]) continue;
            const uint64_t e = exitv[q - 1];
            // a speculative decode that failed (wrong start state) tells nothing: its successor keeps decoding from its own state.
            // The true chain never fails inside a valid segment, so the fixed point is unchanged; on corrupt data the final pass flags it.
            if (e != JE_SENTINEL && e != start[q]) { start[q] = e; changed[q] = 1; any = 1; }
        }
        ++nround;
        if (!__syncthreads_or(any) || nround > nsub) break;
    }

    // blocks before each subsequence inside its segment (exclusive, segmented)
    carry = 0;
    for (int b = 0; b < nsub; b += JE_THREADS) {
        const int q = b + tid;
        int v = 0, f = 0;
        if (q < nsub) { v = (int)nblk[q]; f = q == (int)segfirst[subseg[q]]; }
        int nxt;
        const int inc = wg_seg_scan(v, f, carry, S, &nxt);
        if (q < nsub) nblk[q] = (uint32_t)(inc - v);
        carry = nxt;
    }
    __syncthreads();

    // final pass: coefficients
    int err = 0;
    for (int q = tid; q < nsub; q += JE_THREADS) {
        const uint64_t st0 = start[q];
        const int s = (int)subseg[q];
        const uint32_t a = seg_start(s) + (uint32_t)(q - (int)segfirst[s]) * (uint32_t)S_bits, e = seg_endb(s);
        const uint32_t end = min(e, a + (uint32_t)S_bits);
        const int limit = (int)segt[2 * s + 1] * bpm;
        const int b0 = (int)nblk[q];
        if (b0 >= limit) continue;
        uint32_t p = (uint32_t)st0;
        int k = (int)((st0 >> 32) & 0xFF), j = (int)(st0 >> 40), nb = 0, reached = 0;
        const long long blk_base = (long long)s * (ri > 0 ? ri : 0) * bpm;
        if (blk_base + limit > nblocks) { err |= MFR_JPEG_E_SIZE; continue; }
        err |= decode_run(d, S, bpm, p, k, j, end, e, nb, true, coef, blk_base, b0, limit, &reached);
        if (reached) segdone[s] = 1;
    }
    __syncthreads();
    for (int s = tid; s < nseg; s += JE_THREADS)
        if (!segdone[s]) err |= MFR_JPEG_E_TRUNC;
    if (err) atomicOr(&S.err, err);
    __syncthreads();
    const int e_all = S.err;
    if (tid == 0) { status[img] = e_all; if (rounds) rounds[img] = nround; }
    if (e_all) return;

    // DC prediction: per component, a prefix sum over its blocks in MCU order, restarted at every restart segment
    for (int c = 0; c < h->ncomp; ++c) {
        const int hv = h->comp_bw[c] * h->comp_bh[c], co = h->comp_off[c];
        const long long nc = (long long)h->total_mcus * hv;
        carry = 0;
        for (long long b = 0; b < nc; b += JE_THREADS) {
            const long long i = b + tid;
            int v = 0, f = 0;
            long long blk = 0;
            if (i < nc) {
                const long long m = i / hv;
                const int jj = (int)(i - m * hv);
                blk = m * bpm + co + jj;
                v = coef[blk * 64];
                f = ri > 0 ? (jj == 0 && m % ri == 0) : i == 0;
            }
            int nxt;
            const int inc = wg_seg_scan(v, f, carry, S, &nxt);
            if (i < nc) coef[blk * 64] = (int16_t)inc;
            carry = nxt;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// dequantise + JDCT_ISLOW

#define IDCT_BLOCKS 32              // blocks per 256-lane workgroup

// one 1-D pass; 64-bit products and sums as libjpeg's JLONG, results stored as int (its workspace / DESCALE)
__device__ __forceinline__ void islow_1d(const int x[8], int out[8], int shift)
{
    typedef long long L64;
    const L64 c0298 = 2446, c0390 = 3196, c0541 = 4433, c0765 = 6270, c0899 = 7373, c1175 = 9633, c1501 = 12299, c1847 = 15137,
              c1961 = 16069, c2053 = 16819, c2562 = 20995, c3072 = 25172;
    // even part
    L64 z1 = ((L64)x[2] + x[6]) * c0541;
    const L64 t2 = z1 - (L64)x[6] * c1847, t3 = z1 + (L64)x[2] * c0765;
    const L64 t0 = ((L64)x[0] + x[4]) * 8192, t1 = ((L64)x[0] - x[4]) * 8192;
    const L64 t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    // odd part
    L64 a0 = x[7], a1 = x[5], a2 = x[3], a3 = x[1];
    z1 = a0 + a3;
    L64 z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
    const L64 z5 = (z3 + z4) * c1175;
    a0 *= c0298; a1 *= c2053; a2 *= c3072; a3 *= c1501;
    z1 *= -c0899; z2 *= -c2562; z3 = z3 * -c1961 + z5; z4 = z4 * -c0390 + z5;
    a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4;
    const L64 rnd = 1ll << (shift - 1);
    out[0] = (int)((t10 + a3 + rnd) >> shift); out[7] = (int)((t10 - a3 + rnd) >> shift);
    out[1] = (int)((t11 + a2 + rnd) >> shift); out[6] = (int)((t11 - a2 + rnd) >> shift);
    out[2] = (int)((t12 + a1 + rnd) >> shift); out[5] = (int)((t12 - a1 + rnd) >> shift);
    out[3] = (int)((t13 + a0 + rnd) >> shift); out[4] = (int)((t13 - a0 + rnd) >> shift);
}

__global__ __launch_bounds__(256) void jpeg_idct_kernel(const mfr_jpeg_header *hdrs, JpegLayout L, uint8_t *ws, const int *status)
{
    __shared__ int tile[IDCT_BLOCKS][8][9];
    const int img = blockIdx.y, g = threadIdx.x >> 3, r = threadIdx.x & 7;
    const mfr_jpeg_header *h = hdrs + img;
    if (status[img] != 0) return;                             // uniform over the workgroup
    const int bpm = h->blocks_per_mcu;
    const long long nblocks = (long long)h->total_mcus * bpm;
    const long long b = (long long)blockIdx.x * IDCT_BLOCKS + g;
    const bool live = b < nblocks;
    uint8_t *base = ws + img * L.stride;
    int c = 0, bx = 0, by = 0;
    if (live) {
        const long long m = b / bpm;
        const int jb = (int)(b - m * bpm);
        c = h->mcu_comp[jb];
        const int jj = jb - h->comp_off[c], bw = h->comp_bw[c];
        bx = (int)(m % h->mcus_x) * bw + jj % bw;
        by = (int)(m / h->mcus_x) * h->comp_bh[c] + jj / bw;
        const int4 raw = *(const int4 *)((const int16_t *)(base + L.coef) + b * 64 + r * 8);
        const uint16_t *q = h->qt[h->comp_tq[c] & 3] + r * 8;
        const int16_t *v = (const int16_t *)&raw;
        for (int i = 0; i < 8; ++i) tile[g][r][i] = (int)v[i] * (int)q[i];   // row r, dequantised
    }
    __syncthreads();
    int x[8], o[8];
    if (live) {                                               // pass 1: column r
        for (int i = 0; i < 8; ++i) x[i] = tile[g][i][r];
        islow_1d(x, o, 13 - 2);
    }
    __syncthreads();
    if (live) {
        for (int i = 0; i < 8; ++i) tile[g][i][r] = o[i];
    }
    __syncthreads();
    if (live) {                                               // pass 2: row r
        for (int i = 0; i < 8; ++i) x[i] = tile[g][r][i];
        islow_1d(x, o, 13 + 2 + 3);
        uint32_t w0 = 0, w1 = 0;
        for (int i = 0; i < 8; ++i) {
            // libjpeg-turbo's SIMD ISLOW packs the descaled output with signed saturation: a clamp to [-128, 127], then + 128
            const int s = min(max(o[i], -128), 127) + 128;
            if (i < 4) w0 |= (uint32_t)s << (8 * i); else w1 |= (uint32_t)s << (8 * (i - 4));
        }
        uint8_t *pl = base + L.planes + h->plane_off[c];
        *(uint2 *)(pl + (size_t)(by * 8 + r) * h->plane_w[c] + bx * 8) = make_uint2(w0, w1);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// upsampling + colour + luma

// fancy upsampling of component c at output pixel (x, y): h2v1 and h2v2 triangle filters, edges replicate the last real
// row / column (down_w / down_h), as libjpeg's h2v1_fancy_upsample / h2v2_fancy_upsample
__device__ __forceinline__ int chroma_at(const uint8_t *pl, int pw, int dw, int dh, int hf, int vf, int x, int y)
{
    if (hf == 1) return pl[(size_t)y * pw + x];
    const int cx = x >> 1;
    int row0, row1 = -1;
    if (vf == 2) {
        const int cy = y >> 1;
        row0 = cy;
        row1 = (y & 1) ? min(cy + 1, dh - 1) : max(cy - 1, 0);
    } else {
        row0 = y;
    }
    auto col = [&](int cc) -> int {
        const int a = pl[(size_t)row0 * pw + cc];
        return vf == 2 ? 3 * a + pl[(size_t)row1 * pw + cc] : a;
    };
    const int t = col(cx);
    if (vf == 2) {
        if ((x & 1) == 0) return cx == 0 ? (t * 4 + 8) >> 4 : (3 * t + col(cx - 1) + 8) >> 4;
        return cx == dw - 1 ? (t * 4 + 7) >> 4 : (3 * t + col(cx + 1) + 7) >> 4;
    }
    if ((x & 1) == 0) return cx == 0 ? t : (3 * t + col(cx - 1) + 1) >> 2;
    return cx == dw - 1 ? t : (3 * t + col(cx + 1) + 2) >> 2;
}

__global__ __launch_bounds__(256) void jpeg_colour_kernel(const mfr_jpeg_header *hdrs, JpegLayout L, const uint8_t *ws, const int *status,
                                                          int H, int W, float *gray, uint8_t *rgb)
{
    const int img = blockIdx.y;
    if (status[img] != 0) return;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)H * W) return;
    const int y = (int)(i / W), x = (int)(i - (long long)y * W);
    const mfr_jpeg_header *h = hdrs + img;
    const uint8_t *pl = ws + img * L.stride + L.planes;
    const int Y = pl[h->plane_off[0] + (size_t)y * h->plane_w[0] + x];
    int R = Y, G = Y, B = Y, lum = Y;
    if (h->ncomp == 3) {
        const int hf = h->hmax / h->comp_h[1], vf = h->vmax / h->comp_v[1];
        const int cb = chroma_at(pl + h->plane_off[1], h->plane_w[1], h->down_w[1], h->down_h[1], hf, vf, x, y) - 128;
        const int cr = chroma_at(pl + h->plane_off[2], h->plane_w[2], h->down_w[2], h->down_h[2], hf, vf, x, y) - 128;
        // FIX(1.40200) = 91881, FIX(1.77200) = 116130, FIX(0.71414) = 46802, FIX(0.34414) = 22554, ONE_HALF = 1 << 15
        R = Y + ((91881 * cr + 32768) >> 16);
        G = Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16);
        B = Y + ((116130 * cb + 32768) >> 16);
        R = min(max(R, 0), 255); G = min(max(G, 0), 255); B = min(max(B, 0), 255);
        lum = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
    }
    const size_t o = (size_t)img * H * W + i;
    if (gray) gray[o] = (float)lum / 255.0f;
    if (rgb) {
        rgb[3 * o] = (uint8_t)R; rgb[3 * o + 1] = (uint8_t)G; rgb[3 * o + 2] = (uint8_t)B;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------

extern "C" size_t mfr_jpeg_workspace_bytes(int n, int H, int W, long long max_record_bytes, int subseq_bits)
{
    JpegLayout L;
    if (jpeg_layout(n, H, W, max_record_bytes, subseq_bits, &L) != 0) return 0;
    return (size_t)(L.stride * n);
}

extern "C" int mfr_jpeg_decode(const void *headers, const uint8_t *records, const long long *offsets, int n, int H, int W,
                               long long max_record_bytes, float *gray, uint8_t *rgb, int *status, int *rounds, void *workspace,
                               size_t workspace_bytes, int subseq_bits, void *stream)
{
    JpegLayout L;
    if (!headers || !records || !offsets || (!gray && !rgb) || !status || !workspace) return MFR_E_ARG;
    if (jpeg_layout(n, H, W, max_record_bytes, subseq_bits, &L) != 0) return MFR_E_ARG;
    if (workspace_bytes < (size_t)(L.stride * n)) return MFR_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const mfr_jpeg_header *h = (const mfr_jpeg_header *)headers;
    uint8_t *ws = (uint8_t *)workspace;
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3(n), dim3(JE_THREADS), 0, st, h, records, offsets, H, W, subseq_bits, L, ws, status, rounds);
    CHECK_LAUNCH();
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((L.blocks_max + IDCT_BLOCKS - 1) / IDCT_BLOCKS, n), dim3(256), 0, st, h, L, ws, status);
    CHECK_LAUNCH();
    hipLaunchKernelGGL(jpeg_colour_kernel, dim3((unsigned)(((long long)H * W + 255) / 256), n), dim3(256), 0, st, h, L, ws, status, H, W, gray, rgb);
    CHECK_LAUNCH();
    return 0;
}
