/* mfr_png.h -- the packed per-image header of the 16-bit depth PNG decoder, shared by the host parse (csrc/host_decode.c,
 * libmfr_host.so: mfr_host_png_parse) and the device kernel (csrc/png.hip, libmfr_hip.so: mfr_png_depth_decode).
 *
 * One image = one fixed-size header + one variable-size record.  The record is
 *   [the zlib stream (RFC 1950): the payloads of the file's IDAT chunks joined in file order, stream_bytes long]
 *   [>= 8 zero bytes, total padded to 16 bytes]
 * Plain C, fixed-width fields only, no implicit padding.
 */
#ifndef MFR_PNG_H
#define MFR_PNG_H
#include <stdint.h>

#define MFR_PNG_OK 0
#define MFR_PNG_UNSUPPORTED 1       /* a valid PNG the device decoder leaves to the host: anything but colour type 0 at bit depth 16 with
                                       interlace 0; a zlib header with a window above 32 KiB or a preset dictionary */
#define MFR_PNG_INVALID 2           /* truncated or malformed input, zero width or height */
#define MFR_PNG_CAPACITY 3          /* the record buffer is too small for the stream */
/* device status bits (mfr_png_depth_decode's per-image status; host parse codes above are passed through unchanged) */
#define MFR_PNG_E_DATA 0x10         /* invalid deflate data (block type 3, LEN / NLEN, code sets, unassigned code, distance too far) or a
                                       filter type above 4 */
#define MFR_PNG_E_TRUNC 0x20        /* the stream ended before the final block's end or before the Adler-32 */
#define MFR_PNG_E_SIZE 0x40         /* the header's size is not the batch's H x W, the record exceeds its slot, or the stream inflates to
                                       more or fewer than H (1 + 2 W) bytes */
#define MFR_PNG_E_CHECK 0x80        /* Adler-32 mismatch */

typedef struct mfr_png_header {
    int32_t status, width, height, bit_depth;
    int32_t color_type, interlace, stream_bytes, record_bytes;
} mfr_png_header;

#endif
