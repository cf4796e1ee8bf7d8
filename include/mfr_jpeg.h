/* mfr_jpeg.h -- the packed per-image header of the baseline JPEG decoder, shared by the host parse (csrc/host_decode.c,
 * libmfr_host.so: mfr_host_jpeg_parse) and the device kernels (csrc/jpeg.hip, libmfr_hip.so: mfr_jpeg_decode).
 *
 * One image = one fixed-size header + one variable-size record.  The record is
 *   [segment table: nseg x {u32 byte offset of the segment in the data, u32 MCU count}, padded to 16 bytes]
 *   [entropy-coded data of the scan, unstuffed (0xFF00 -> 0xFF), RSTn markers removed, segments back to back]
 *   [>= 8 zero bytes, total padded to 16 bytes]
 * Plain C, fixed-width fields only, no implicit padding (every array is a multiple of 16 bytes and starts 16-aligned).
 */
#ifndef MFR_JPEG_H
#define MFR_JPEG_H
#include <stdint.h>

#define MFR_JPEG_OK 0
#define MFR_JPEG_UNSUPPORTED 1      /* valid JPEG the device decoder does not take: progressive, arithmetic, lossless, 12-bit, multi-scan,
                                       > 3 components, RGB / CMYK / YCCK colour, sampling other than 4:4:4, 4:2:2, 4:2:0 or gray,
                                       Huffman table ids 2 / 3 */
#define MFR_JPEG_INVALID 2          /* truncated or malformed input */
#define MFR_JPEG_CAPACITY 3         /* the record buffer is too small */
/* device status bits (mfr_jpeg_decode's per-image status; host parse codes above are passed through unchanged) */
#define MFR_JPEG_E_HUFF 0x10        /* a code with no match within 16 bits */
#define MFR_JPEG_E_TRUNC 0x20       /* a restart segment ended before its MCU count */
#define MFR_JPEG_E_SIZE 0x40        /* the header's size is not the batch's H x W, or the record exceeds its slot */

#define MFR_JPEG_FAST_BITS 9
#define MFR_JPEG_MAX_BLOCKS_PER_MCU 6

typedef struct mfr_jpeg_huff {
    int32_t maxcode[20];            /* [l] largest code of length l (1..16), -1 if none */
    int32_t valoff[20];             /* [l] HUFFVAL index of code c of length l = c + valoff[l] */
    uint16_t fast[1 << MFR_JPEG_FAST_BITS];   /* top 9 bits -> (length << 8) | symbol for codes of <= 9 bits; 0 = longer or no code */
    uint8_t bits[16];               /* BITS: number of codes of length 1..16 */
    uint8_t val[256];               /* HUFFVAL */
} mfr_jpeg_huff;

typedef struct mfr_jpeg_header {
    int32_t status, width, height, ncomp;
    int32_t hmax, vmax, mcus_x, mcus_y;
    int32_t blocks_per_mcu, restart_interval, nseg, total_mcus;
    int32_t seg_table_bytes, data_bytes, record_bytes, adobe_transform;   /* adobe_transform: -1 without an Adobe APP14 marker */
    int32_t comp_id[4], comp_h[4], comp_v[4], comp_tq[4];                 /* as in the frame header */
    int32_t comp_td[4], comp_ta[4];                                       /* DC / AC Huffman table of the scan */
    int32_t comp_bw[4], comp_bh[4];     /* blocks of the component in one MCU across / down (h, v; 1, 1 in a single-component scan) */
    int32_t comp_off[4];                /* first block of the component inside an MCU */
    int32_t plane_w[4], plane_h[4];     /* the component's sample plane padded to whole MCUs, pixels */
    int32_t plane_off[4];               /* byte offset of that plane inside the image's plane area */
    int32_t down_w[4], down_h[4];       /* downsampled_width / height: ceil(W h / hmax), ceil(H v / vmax) */
    int32_t mcu_comp[12];               /* component of block j of an MCU */
    uint16_t qt[4][64];                 /* quantisation tables, natural (row-major) order */
    mfr_jpeg_huff dc[2], ac[2];
} mfr_jpeg_header;

#endif
