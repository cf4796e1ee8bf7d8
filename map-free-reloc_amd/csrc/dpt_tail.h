// dpt_tail.h -- what the depth networks' two ends share (csrc/dpt.hip: DPT-Hybrid, csrc/depth_anything.hip: Depth Anything): torch's bilinear source taps,
// and the tail behind the head's last 1x1 layer -- activation per tap, bilinear resize to the image, metres, millimetres and their rounding.  ONE
// definition: the plain and the row-table entry of each network promise the same bits, and the two networks the same millimetres for the same metres.
#pragma once
#include "wave_dev.h"

namespace mfr {

// torch's source index of upsample_bilinear2d with align_corners=False: scale (dst + 0.5) - 0.5, clamped at 0; the second tap stops at the edge
MFR_DEV void bilinear_taps(int dst, float scale, int n_in, int &i0, int &i1, float &l0, float &l1)
{
    float src = scale * ((float)dst + 0.5f) - 0.5f;
    src = src < 0.f ? 0.f : src;
    i0 = min((int)src, n_in - 1);
    i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
    l1 = src - (float)i0;
    l0 = 1.f - l1;
}

// the four-tap blend with its three fused multiply-adds written out: left to -ffp-contract the compiler fuses them in one kernel and not in its twin
// (packed multiplies, then an add), and the entry points promise the same bits
MFR_DEV float bilinear_blend(float ly0, float ly1, float lx0, float lx1, float v00, float v01, float v10, float v11)
{
    return fmaf(ly0, fmaf(lx0, v00, lx1 * v01), ly1 * fmaf(lx0, v10, lx1 * v11));
}

constexpr int HEAD_MAX_C = 64;

// the 1x1 layer C -> 1 at one position of the head's feature image, then the network's last activation
template <class Act>
MFR_DEV float head_value(const float *__restrict__ f, size_t plane, size_t idx, const float *__restrict__ w, int C, float bias, const Act &act)
{
    float a = bias;
    for (int c = 0; c < C; ++c) a = fmaf(f[c * plane + idx], w[c], a);
    return act(a);
}

// one thread per pixel of the full-resolution map (the body of a kernel of 256-thread workgroups, grid (ceil(Ho Wo / 256), images)): the four taps' head
// values are computed where they are needed (the small input stays in cache).
// ROWS: entry k = blockIdx.y of the tables reads feature image src[k] of the B the caller has and writes plane dst[k] of the D it has; a dst outside
// [0, D) writes nothing, a src outside [0, B) zeroes its plane, and either sets bit 0 of *status.  quantize: the metres written are float32(mm / 1000.0),
// the division in double -- datasets.read_depth_image's value of the 16-bit PNG that holds mm
template <bool ROWS, class Act>
MFR_DEV void depth_tail(const float *__restrict__ f, const float *__restrict__ w, float bias, int C, int Hh, int Wh, const Act &act, int Ho, int Wo, float sy,
                        float sx, float *__restrict__ metres, uint16_t *__restrict__ mm, const int *__restrict__ src, const int *__restrict__ dst, int B, int D,
                        int quantize, int *status)
{
    __shared__ float ws[HEAD_MAX_C];
    if (threadIdx.x < C) ws[threadIdx.x] = w[threadIdx.x];
    __syncthreads();
    int b = blockIdx.y, bo = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Ho * Wo) return;
    if (ROWS) {
        b = src[blockIdx.y];
        bo = dst[blockIdx.y];
        const bool bad_src = b < 0 || b >= B, bad_dst = bo < 0 || bo >= D;
        if (bad_src || bad_dst) {
            if (i == 0) atomicOr(status, 1);
            if (!bad_dst) {
                metres[(size_t)bo * Ho * Wo + i] = 0.f;
                if (mm) mm[(size_t)bo * Ho * Wo + i] = 0;
            }
            return;
        }
    }
    const int y = i / Wo, x = i - y * Wo;
    int y0, y1, x0, x1;
    float ly0, ly1, lx0, lx1;
    bilinear_taps(y, sy, Hh, y0, y1, ly0, ly1);
    bilinear_taps(x, sx, Wh, x0, x1, lx0, lx1);
    const size_t plane = (size_t)Hh * Wh;
    const float *fb = f + (size_t)b * C * plane;
    const float v00 = head_value(fb, plane, (size_t)y0 * Wh + x0, ws, C, bias, act);
    const float v01 = head_value(fb, plane, (size_t)y0 * Wh + x1, ws, C, bias, act);
    const float v10 = head_value(fb, plane, (size_t)y1 * Wh + x0, ws, C, bias, act);
    const float v11 = head_value(fb, plane, (size_t)y1 * Wh + x1, ws, C, bias, act);
    const float v = bilinear_blend(ly0, ly1, lx0, lx1, v00, v01, v10, v11);
    const size_t o = (size_t)bo * Ho * Wo + i;
    if (!ROWS) metres[o] = v;
    if (mm || ROWS) {
        // round-half-even of the EXACT product 1000 v (a 24-bit by a 10-bit factor is exact in double), clamped; NaN -> 0
        const double t = rint((double)v * 1000.0);
        const uint16_t q = (uint16_t)(t >= 65535.0 ? 65535 : (t > 0.0 ? (int)t : 0));
        if (mm) mm[o] = q;
        if (ROWS) metres[o] = quantize ? (float)((double)q / 1000.0) : v;
    }
}

// the size checks of Depth Anything's two tail entries (csrc/dpt.hip's entries keep their own, older copies; the table pointers are checked by the row-table
// entries themselves)
inline bool depth_tail_args_ok(const float *f, const float *w, const float *metres, int B, int C, int Hh, int Wh, int Ho, int Wo)
{
    if (!f || !w || !metres || B < 1 || C < 1 || C > HEAD_MAX_C || Hh < 1 || Wh < 1 || Ho < 1 || Wo < 1) return false;
    return (long long)Hh * Wh * C <= 0x7fffffffLL && (long long)Ho * Wo <= 0x7fffffffLL;
}

}  // namespace mfr
