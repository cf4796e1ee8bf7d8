/* Stand-alone driver of mfr_host_png_parse (csrc/host_decode.c) for the sanitiser pass of tests/test_png_host.py: compiled together with
 * host_decode.c under -fsanitize=address,undefined.  argv[1] is a corpus file of records {u32 little-endian length, bytes}.  Every input is
 * copied into a heap block of exactly its size and parsed into heap records of exactly `cap` bytes, for several caps, so that any read
 * outside [data, data + n) or write outside record[0, cap) is a heap-buffer-overflow report.  Prints "PNG_PARSE_OK <inputs> <ok>". */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mfr_png.h"

int mfr_host_png_parse(const uint8_t *buf, size_t n, mfr_png_header *h, uint8_t *out, size_t cap, size_t *rec_bytes);
size_t mfr_host_png_record_bound(size_t n);

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    long inputs = 0, ok = 0;
    uint8_t lenb[4];
    while (fread(lenb, 1, 4, f) == 4) {
        const size_t n = (size_t)lenb[0] | (size_t)lenb[1] << 8 | (size_t)lenb[2] << 16 | (size_t)lenb[3] << 24;
        uint8_t *data = malloc(n ? n : 1);
        if (!data || fread(data, 1, n, f) != n) return 3;
        uint8_t *exact = malloc(n);                               /* exactly n bytes (malloc(0) is a valid zero-size block) */
        if (n) memcpy(exact, data, n);
        const size_t full = mfr_host_png_record_bound(n);
        size_t want = 0;
        const size_t caps[5] = {full, 0, 16, 0, 0};
        for (int k = 0; k < 5; ++k) {
            size_t cap = caps[k];
            if (k == 3) { if (!want) continue; cap = want; }       /* exactly the record's size */
            if (k == 4) { if (!want) continue; cap = want - 1; }   /* one byte short */
            uint8_t *rec = malloc(cap);
            mfr_png_header h;
            size_t nb = 12345;
            const int st = mfr_host_png_parse(exact, n, &h, rec, cap, &nb);
            if (st < 0 || st > 3 || st != h.status) return 4;
            if (st == MFR_PNG_OK) {
                if (nb > cap || nb != (size_t)h.record_bytes || (size_t)h.stream_bytes + 8 > nb || nb % 16) return 5;
                if (k == 0) { want = nb; ++ok; }
                if (k == 4) return 6;
            } else if (nb != 0) return 7;
            if (k == 3 && st != MFR_PNG_OK) return 8;
            if (k == 4 && st != MFR_PNG_CAPACITY) return 9;
            free(rec);
        }
        free(exact);
        free(data);
        ++inputs;
    }
    fclose(f);
    printf("PNG_PARSE_OK %ld %ld\n", inputs, ok);
    return 0;
}
