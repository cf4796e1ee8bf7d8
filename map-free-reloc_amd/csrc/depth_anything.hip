// Depth Anything V2 (a DINOv2 ViT behind a DPT head): the kernels DPT-Hybrid's (csrc/dpt.hip) do not cover (include/mfr_hip.h mfr_da_*).
//   mfr_da_patch_rows (_tab)   image -> the patch embedding's GEMM operand: bilinear resize (align_corners=False, torch's arithmetic), ImageNet normalisation
//                              and the 14 x 14 unfold in one pass; the 14 x 14 / stride 14 convolution is then ONE linear layer with K = 588
//   mfr_da_tokens              the product's rows + position embeddings -> token rows, the cls row in front
//   mfr_da_head_tail (_rows)   max_depth sigmoid (or ReLU) behind the last 1x1 layer, then dpt_tail.h's resize / millimetres
// fp32 storage and fp32 arithmetic throughout; wave64; every store is a vector (VMEM) store.  Every index is bounded by the launch geometry that the
// entry point derives from its own (checked) arguments; the row tables are range-checked on the device before anything is read through them.
#include "dpt_tail.h"

using namespace mfr;

namespace {

constexpr int PATCH = 14, PATCH_K = 3 * PATCH * PATCH;     // 588 columns of a patch row: (c 14 + i) 14 + j
constexpr int PX = 8;                                      // patches of one band per workgroup: 8 x 588 floats = 18.4 KiB of LDS, eight workgroups per CU

struct Norm3 { float mean[3], std[3]; };

// One workgroup: PX consecutive patches of patch-row blockIdx.y of output image blockIdx.z, i.e. a 14 x (14 PX) band of the network-size image.
// Phase 1: a thread per band pixel, x fastest -- consecutive lanes read consecutive source pixels (u8: 3 adjacent bytes each; f32: three coalesced plane
// reads), every source pixel comes from DRAM once (the 2 x 2 taps of neighbouring outputs hit the cache) -- and writes its three normalised values into LDS
// AT THEIR COLUMN of the patch row: lanes of one patch write consecutive words (conflict-free), a wave spans at most six patches.  The normalised image
// never exists in memory.  Phase 2: the rows leave LDS exactly as they lie there: 16-byte LDS reads (patch stride 2352 bytes = 147 x 16: every read
// aligned, consecutive lanes on consecutive 16-byte slots) and 16-byte global stores, consecutive lanes on consecutive addresses of a row, the
// zero columns 588 .. ldk - 1 in the same stores.
// What should bound it (an expectation from the byte counts; no kernel trace has been taken): the stores.  At 540 x 720 -> 518 x 686 it reads 1.2 MB per image and writes 1813 x ldk x 4 = 4.6 MB (ldk 640), 3.9x the read; the
// arithmetic (two tap computations and nine fused multiply-adds per pixel) is far below either.
// ROWS (mfr_da_patch_rows_tab): output image blockIdx.z is made from image tab[blockIdx.z] of the N the caller has; an index outside [0, N) is never
// dereferenced: that image's rows are zeros and bit 0 of *status is set.  The arithmetic is this one body for both entries
template <bool U8, bool ROWS>
__global__ __launch_bounds__(256) void patch_rows_kernel(const void *__restrict__ img, int H, int W, int gh, int gw, float sy, float sx, Norm3 nrm,
                                                         float *__restrict__ rows, int ldk, const int *__restrict__ tab, int N, int *status)
{
    __shared__ __attribute__((aligned(16))) float band[PX * PATCH_K];
    const int px0 = blockIdx.x * PX, gy = blockIdx.y, j = blockIdx.z;
    const int npx = min(PX, gw - px0);                     // >= 1 by the grid
    const int k4 = ldk >> 2;
    float *out = rows + ((size_t)j * gh + gy) * gw * ldk + (size_t)px0 * ldk;
    int b = j;
    bool zero = false;
    if (ROWS) {
        b = tab[j];
        zero = b < 0 || b >= N;
        if (zero && blockIdx.x == 0 && gy == 0 && threadIdx.x == 0) atomicOr(status, 1);
    }
    if (!zero) {
        const int bw = npx * PATCH;
        for (int e = threadIdx.x; e < PATCH * bw; e += 256) {
            const int i = e / bw, xx = e - i * bw;
            int y0, y1, x0, x1;
            float ly0, ly1, lx0, lx1;
            bilinear_taps(gy * PATCH + i, sy, H, y0, y1, ly0, ly1);
            bilinear_taps(px0 * PATCH + xx, sx, W, x0, x1, lx0, lx1);
            const int p = xx / PATCH, jj = xx - p * PATCH;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float v00, v01, v10, v11;
                if (U8) {
                    const uint8_t *s = (const uint8_t *)img + (size_t)b * H * W * 3 + c;
                    v00 = (float)s[((size_t)y0 * W + x0) * 3] / 255.f; v01 = (float)s[((size_t)y0 * W + x1) * 3] / 255.f;
                    v10 = (float)s[((size_t)y1 * W + x0) * 3] / 255.f; v11 = (float)s[((size_t)y1 * W + x1) * 3] / 255.f;
                } else {
                    const float *s = (const float *)img + ((size_t)b * 3 + c) * H * W;
                    v00 = s[(size_t)y0 * W + x0]; v01 = s[(size_t)y0 * W + x1];
                    v10 = s[(size_t)y1 * W + x0]; v11 = s[(size_t)y1 * W + x1];
                }
                const float v = bilinear_blend(ly0, ly1, lx0, lx1, v00, v01, v10, v11);
                band[p * PATCH_K + (c * PATCH + i) * PATCH + jj] = (v - nrm.mean[c]) / nrm.std[c];
            }
        }
    }
    __syncthreads();
    for (int q = threadIdx.x; q < npx * k4; q += 256) {
        const int p = q / k4, k = (q - p * k4) * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (!zero && k < PATCH_K) v = *(const float4 *)(band + p * PATCH_K + k);       // 588 % 4 == 0: a float4 never straddles the end of the patch
        *(float4 *)(out + (size_t)p * ldk + k) = v;
    }
}

// out[b][0] = cls + pos[0];  out[b][1 + p] = x[b HW + p] + pos[1 + p]: one float4 per thread, 4 (1 + HW) C B bytes written, 4 HW C B read (+ pos, which
// every image reads again from the cache) -- the traffic of an in-place position add, in exchange for ONE embedding product over all images (its output rows
// are evenly spaced; the token blocks, one cls row each, are not)
__global__ __launch_bounds__(256) void da_tokens_kernel(const float *__restrict__ x, int ldx, const float *__restrict__ cls, const float *__restrict__ pos,
                                                        int C, int HW, long long total4, float *__restrict__ out, int ldo)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total4) return;
    const int c4 = C >> 2;
    const int c = (int)(idx % c4) * 4;
    const long long r = idx / c4;
    const int t = (int)(r % (HW + 1));
    const long long b = r / (HW + 1);
    const float4 a = t == 0 ? *(const float4 *)(cls + c) : *(const float4 *)(x + (size_t)(b * HW + t - 1) * ldx + c);
    const float4 p = *(const float4 *)(pos + (size_t)t * C + c);
    *(float4 *)(out + (size_t)r * ldo + c) = make_float4(a.x + p.x, a.y + p.y, a.z + p.z, a.w + p.w);
}

// Depth Anything's last activation: max_depth sigmoid (the metric checkpoints) or ReLU (the relative ones)
struct AnythingAct {
    int metric;
    float max_depth;
    __device__ __forceinline__ float operator()(float a) const { return metric ? max_depth * (1.f / (1.f + expf(-a))) : fmaxf(a, 0.f); }
};

template <bool ROWS>
__global__ __launch_bounds__(256) void da_head_tail_kernel(const float *__restrict__ f, const float *__restrict__ w, float bias, int C, int Hh, int Wh, int metric,
                                                           float max_depth, int Ho, int Wo, float sy, float sx, float *__restrict__ metres,
                                                           uint16_t *__restrict__ mm, const int *__restrict__ src, const int *__restrict__ dst, int B, int D,
                                                           int quantize, int *status)
{
    depth_tail<ROWS>(f, w, bias, C, Hh, Wh, AnythingAct{metric, max_depth}, Ho, Wo, sy, sx, metres, mm, src, dst, B, D, quantize, status);
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
constexpr long long I31 = 0x7fffffffLL;

// shared by the two patch-row entries: sizes, the operand's row length and alignment, the normalisation
bool patch_args_ok(const void *img, const float *rows, int n_out, int H, int W, int gh, int gw, const Norm3 &n, int ldk)
{
    if (!img || !rows || n_out < 1 || n_out > 65535 || H < 1 || W < 1 || gh < 1 || gw < 1 || gh > 65535 || gw > 65535) return false;
    if (ldk < PATCH_K || ldk % 4 || ldk > 4096 || !aligned16(rows)) return false;
    if ((long long)H * W * 3 > I31 || (long long)gh * gw * PATCH * PATCH * 3 > I31) return false;
    for (int c = 0; c < 3; ++c)
        if (!(n.mean[c] == n.mean[c]) || !(n.std[c] > 0.f)) return false;
    return true;
}

}  // namespace

extern "C" int mfr_da_patch_rows(const void *img, int dtype, int B, int H, int W, int gh, int gw, float mean0, float mean1, float mean2, float std0, float std1,
                                 float std2, float *rows, int ldk, void *stream)
{
    const Norm3 n{{mean0, mean1, mean2}, {std0, std1, std2}};
    if ((dtype != 0 && dtype != 1) || !patch_args_ok(img, rows, B, H, W, gh, gw, n, ldk)) return MFR_E_ARG;
    const float sy = (float)H / (float)(gh * PATCH), sx = (float)W / (float)(gw * PATCH);
    const dim3 grid((gw + PX - 1) / PX, gh, B);
    if (dtype == 0) hipLaunchKernelGGL((patch_rows_kernel<true, false>), grid, dim3(256), 0, (hipStream_t)stream, img, H, W, gh, gw, sy, sx, n, rows, ldk, nullptr, 0, nullptr);
    else hipLaunchKernelGGL((patch_rows_kernel<false, false>), grid, dim3(256), 0, (hipStream_t)stream, img, H, W, gh, gw, sy, sx, n, rows, ldk, nullptr, 0, nullptr);
    CHECK_LAUNCH();
    return 0;
}

extern "C" int mfr_da_patch_rows_tab(const uint8_t *img, int N, const int *tab, int m, int H, int W, int gh, int gw, float mean0, float mean1, float mean2,
                                     float std0, float std1, float std2, float *rows, int ldk, int *status, void *stream)
{
    const Norm3 n{{mean0, mean1, mean2}, {std0, std1, std2}};
    if (!tab || !status || N < 1 || !patch_args_ok(img, rows, m, H, W, gh, gw, n, ldk)) return MFR_E_ARG;
    const float sy = (float)H / (float)(gh * PATCH), sx = (float)W / (float)(gw * PATCH);
    hipLaunchKernelGGL((patch_rows_kernel<true, true>), dim3((gw + PX - 1) / PX, gh, m), dim3(256), 0, (hipStream_t)stream, (const void *)img, H, W, gh, gw, sy, sx, n,
                       rows, ldk, tab, N, status);
    CHECK_LAUNCH();
    return 0;
}

extern "C" int mfr_da_tokens(const float *x, int ldx, const float *cls, const float *pos, int B, int C, int HW, float *out, int ldo, void *stream)
{
    if (!x || !cls || !pos || !out || B < 1 || C < 4 || C % 4 || HW < 1 || ldx < C || ldx % 4 || ldo < C || ldo % 4) return MFR_E_ARG;
    if (!aligned16(x) || !aligned16(cls) || !aligned16(pos) || !aligned16(out)) return MFR_E_ARG;
    const long long total4 = (long long)B * (HW + 1) * (C / 4);
    if ((long long)(HW + 1) * C > I31 || total4 > (1LL << 36) || (total4 + 255) / 256 > I31) return MFR_E_ARG;
    hipLaunchKernelGGL(da_tokens_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, ldx, cls, pos, C, HW, total4, out, ldo);
    CHECK_LAUNCH();
    return 0;
}

extern "C" int mfr_da_head_tail(const float *f, const float *w, float bias, int B, int C, int Hh, int Wh, int metric, float max_depth, int Ho, int Wo, float *metres,
                                uint16_t *mm, void *stream)
{
    if (!depth_tail_args_ok(f, w, metres, B, C, Hh, Wh, Ho, Wo) || B > 65535 || (metric != 0 && metric != 1) || (metric && !(max_depth > 0.f))) return MFR_E_ARG;
    const float sy = (float)Hh / (float)Ho, sx = (float)Wh / (float)Wo;
    hipLaunchKernelGGL(da_head_tail_kernel<false>, dim3((unsigned)(((long long)Ho * Wo + 255) / 256), B), dim3(256), 0, (hipStream_t)stream, f, w, bias, C, Hh, Wh, metric,
                       max_depth, Ho, Wo, sy, sx, metres, mm, nullptr, nullptr, B, B, 0, nullptr);
    CHECK_LAUNCH();
    return 0;
}

extern "C" int mfr_da_head_tail_rows(const float *f, const float *w, float bias, int B, int C, int Hh, int Wh, int metric, float max_depth, int Ho, int Wo,
                                     const int *src, const int *dst, int d, float *metres, uint16_t *mm, int D, int quantize, int *status, void *stream)
{
    if (!depth_tail_args_ok(f, w, metres, B, C, Hh, Wh, Ho, Wo) || !src || !dst || !status || D < 1 || d < 1 || d > 65535) return MFR_E_ARG;
    if ((metric != 0 && metric != 1) || (metric && !(max_depth > 0.f)) || (quantize != 0 && quantize != 1)) return MFR_E_ARG;
    const float sy = (float)Hh / (float)Ho, sx = (float)Wh / (float)Wo;
    hipLaunchKernelGGL(da_head_tail_kernel<true>, dim3((unsigned)(((long long)Ho * Wo + 255) / 256), d), dim3(256), 0, (hipStream_t)stream, f, w, bias, C, Hh, Wh, metric,
                       max_depth, Ho, Wo, sy, sx, metres, mm, src, dst, B, D, quantize, status);
    CHECK_LAUNCH();
    return 0;
}
