// Gray plane of a decoded RGB batch at another size (include/mfr_hip.h mfr_resize_gray_bilinear): bit for bit
// datasets.gray_plane(rgb_u8, (w, h)) -- integer luma, that byte as float32, OpenCV-style INTER_LINEAR (half-pixel centres, edge-clamped
// taps, no antialiasing) of the FLOAT plane, / 255f.  The tap tables (i0, i1, f per output row / column) are the caller's: they are
// evaluated in float64 on the host with the very expression of datasets.resize_bilinear_f32 and uploaded once per (n_in, n_out).
//
// Bit equality with numpy needs every product and sum rounded on its own, in numpy's order:
//   top = a00 * (1 - fx) + a01 * fx;  bot = a10 * (1 - fx) + a11 * fx;  out = top * (1 - fy) + bot * fy;  out / 255
// so every operation is an explicitly rounded intrinsic (and this translation unit is built with -ffp-contract=off): one fma breaks it.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mfr_hip.h"

#define CHECK_LAUNCH() do { if (hipGetLastError() != hipSuccess) return MFR_E_LAUNCH; } while (0)

__device__ __forceinline__ float luma_at(const uint8_t *p)
{
    return (float)((19595u * p[0] + 38470u * p[1] + 7471u * p[2] + 32768u) >> 16);
}

__global__ __launch_bounds__(256) void resize_gray_bilinear_kernel(const uint8_t *rgb, const int *status, int H, int W,
                                                                   const int *y0, const int *y1, const float *fy,
                                                                   const int *x0, const int *x1, const float *fx,
                                                                   int h, int w, float *out)
{
    const int img = blockIdx.y;
    if (status && status[img] != 0) return;                   // not decoded (the host's plane, or a failed decode): left as it is
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)h * w) return;
    const int y = (int)(i / w), x = (int)(i - (long long)y * w);
    // the tables hold clamped indices already; clamping again keeps a wrong table from reading outside the image
    const int ya = min(max(y0[y], 0), H - 1), yb = min(max(y1[y], 0), H - 1);
    const int xa = min(max(x0[x], 0), W - 1), xb = min(max(x1[x], 0), W - 1);
    const float wx = fx[x], wy = fy[y];
    const float ux = __fsub_rn(1.0f, wx), uy = __fsub_rn(1.0f, wy);
    const uint8_t *src = rgb + (size_t)img * H * W * 3;
    const uint8_t *ra = src + (size_t)ya * W * 3, *rb = src + (size_t)yb * W * 3;
    const float a00 = luma_at(ra + 3 * (size_t)xa), a01 = luma_at(ra + 3 * (size_t)xb);
    const float a10 = luma_at(rb + 3 * (size_t)xa), a11 = luma_at(rb + 3 * (size_t)xb);
    const float top = __fadd_rn(__fmul_rn(a00, ux), __fmul_rn(a01, wx));
    const float bot = __fadd_rn(__fmul_rn(a10, ux), __fmul_rn(a11, wx));
    const float v = __fadd_rn(__fmul_rn(top, uy), __fmul_rn(bot, wy));
    out[(size_t)img * h * w + i] = __fdiv_rn(v, 255.0f);
}

extern "C" int mfr_resize_gray_bilinear(const uint8_t *rgb, int n, int H, int W, const int32_t *status,
                                        const int32_t *y0, const int32_t *y1, const float *fy,
                                        const int32_t *x0, const int32_t *x1, const float *fx,
                                        int h, int w, float *out, void *stream)
{
    if (n < 0 || H < 1 || W < 1 || h < 1 || w < 1) return MFR_E_ARG;
    if (n == 0) return 0;
    if (!rgb || !y0 || !y1 || !fy || !x0 || !x1 || !fx || !out) return MFR_E_ARG;
    if (n > 65535 || (long long)H * W * 3 > 0x7fffffffLL || (long long)h * w > 0x7fffffffLL) return MFR_E_ARG;
    hipLaunchKernelGGL(resize_gray_bilinear_kernel, dim3((unsigned)(((long long)h * w + 255) / 256), n), dim3(256), 0, (hipStream_t)stream,
                       rgb, status, H, W, y0, y1, fy, x0, x1, fx, h, w, out);
    CHECK_LAUNCH();
    return 0;
}
