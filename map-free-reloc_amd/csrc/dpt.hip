// DPT-Hybrid monocular depth (Ranftl et al., ICCV 2021): the kernels between its matrix products (include/mfr_hip.h mfr_dpt_*).  The products themselves
// are the split GEMMs, the implicit-GEMM / direct convolutions and mfr_sg_attention of the other translation units; what is here is the network's glue:
//   mfr_dpt_prep            image -> network input: bilinear resize (align_corners=False, torch's arithmetic) fused with (x - 0.5) / 0.5
//   mfr_dpt_groupnorm       BiT's GroupNorm over NCHW (+ residual) (+ ReLU)
//   mfr_dpt_maxpool3s2      BiT's 3x3 / stride 2 max-pool with an explicit (lo, hi) zero padding per axis
//   mfr_dpt_layernorm       LayerNorm over rows of any C that is a multiple of 64 (+ residual), strided in and out
//   mfr_dpt_bias_gelu       exact (erf) GELU behind fc1
//   mfr_dpt_add_relu        a (+ b) and its ReLU in one pass: the fusion layer's sum and the pre-activation of the residual unit behind it
//   mfr_dpt_tokens          NCHW -> token rows with the cls row and the position embeddings;  mfr_dpt_tokens_inverse: rows -> NCHW (+ per-image bias, GELU)
//   mfr_dpt_shuffle         pixel-shuffle store of ConvTranspose2d(k = s) computed as a GEMM with N = C s^2
//   mfr_dpt_head_tail       1x1 32 -> 1, ReLU, optional 1 / (scale p + shift), bilinear resize to the image, metres f32 (+ u16 millimetres)
// fp32 storage and fp32 arithmetic throughout; wave64; every store is a vector (VMEM) store.  Every index is bounded by the launch geometry that the
// entry point derives from its own (checked) arguments: no kernel trusts a table or a size it was not launched with.
#include "dpt_tail.h"

using namespace mfr;

namespace {

MFR_DEV float gelu_erf(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752440f)); }

// ---------------------------------------------------------------- prep
// ROWS (mfr_dpt_prep_rows): output image blockIdx.y is made from image rows[blockIdx.y] of the N the caller has; an index outside [0, N) is never
// dereferenced: that output image is zeros and bit 0 of *status is set.  The arithmetic is this one body for both entries
template <bool U8, bool ROWS>
__global__ __launch_bounds__(256) void prep_kernel(const void *__restrict__ img, int H, int W, int Hn, int Wn, float sy, float sx, float *__restrict__ out,
                                                   const int *__restrict__ rows, int N, int *status)
{
    const int j = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Hn * Wn) return;
    int b = j;
    if (ROWS) {
        b = rows[j];
        if (b < 0 || b >= N) {
#pragma unroll
            for (int c = 0; c < 3; ++c) out[((size_t)j * 3 + c) * Hn * Wn + i] = 0.f;
            if (i == 0) atomicOr(status, 1);
            return;
        }
    }
    const int y = i / Wn, x = i - y * Wn;
    int y0, y1, x0, x1;
    float ly0, ly1, lx0, lx1;
    bilinear_taps(y, sy, H, y0, y1, ly0, ly1);
    bilinear_taps(x, sx, W, x0, x1, lx0, lx1);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v00, v01, v10, v11;
        if (U8) {
            const uint8_t *p = (const uint8_t *)img + (size_t)b * H * W * 3 + c;
            v00 = (float)p[((size_t)y0 * W + x0) * 3] / 255.f; v01 = (float)p[((size_t)y0 * W + x1) * 3] / 255.f;
            v10 = (float)p[((size_t)y1 * W + x0) * 3] / 255.f; v11 = (float)p[((size_t)y1 * W + x1) * 3] / 255.f;
        } else {
            const float *p = (const float *)img + ((size_t)b * 3 + c) * H * W;
            v00 = p[(size_t)y0 * W + x0]; v01 = p[(size_t)y0 * W + x1];
            v10 = p[(size_t)y1 * W + x0]; v11 = p[(size_t)y1 * W + x1];
        }
        const float v = fmaf(ly0, fmaf(lx0, v00, lx1 * v01), ly1 * fmaf(lx0, v10, lx1 * v11));      // (the fusions written out: see head_tail_kernel)
        out[((size_t)j * 3 + c) * Hn * Wn + i] = (v - 0.5f) / 0.5f;
    }
}

// ---------------------------------------------------------------- GroupNorm
constexpr int GN_THREADS = 512, GN_WAVES = GN_THREADS / 64;

// the workgroup's sum, the same bits in every thread (wave butterfly, then the waves' partials in index order)
MFR_DEV float gn_block_sum(float v, float *sh)
{
    v = wave_sum(v);
    __syncthreads();                                           // the previous round's readers are done with sh
    if (lane_id() == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < GN_WAVES; ++w) t += sh[w];
    return t;
}

// one workgroup per (group, image): the group's (C / G) HW values are contiguous in NCHW.  Two-pass statistics (mean, then centred squares), biased
// variance, rsqrt(var + eps); y = (x - mean) rstd gamma[c] + beta[c] (+ residual) (ReLU); y may be x or residual (each thread reads an element before it writes it, and the
// statistics are complete before the first write: no restrict on the three).  VEC: HW % 4 == 0 and 16-byte aligned planes
template <bool VEC>
__global__ __launch_bounds__(GN_THREADS) void groupnorm_kernel(const float *x, const float *__restrict__ gamma, const float *__restrict__ beta,
                                                               const float *residual, int C, int HW, int G, float eps, int relu, float *y)
{
    __shared__ float sh[GN_WAVES];
    const int g = blockIdx.x, b = blockIdx.y, cg = C / G;
    const size_t base = ((size_t)b * C + (size_t)g * cg) * HW;
    const int n = cg * HW;
    const float *xp = x + base;
    constexpr int STEP = VEC ? 4 : 1;
    float s = 0.f;
    for (int i = threadIdx.x * STEP; i < n; i += GN_THREADS * STEP) {
        if (VEC) { const float4 t = *(const float4 *)(xp + i); s += (t.x + t.y) + (t.z + t.w); }
        else s += xp[i];
    }
    const float mean = gn_block_sum(s, sh) / (float)n;
    float q = 0.f;
    for (int i = threadIdx.x * STEP; i < n; i += GN_THREADS * STEP) {
        if (VEC) {
            const float4 t = *(const float4 *)(xp + i);
            const float d0 = t.x - mean, d1 = t.y - mean, d2 = t.z - mean, d3 = t.w - mean;
            q += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
        } else { const float d = xp[i] - mean; q += d * d; }
    }
    const float rstd = rsqrtf(gn_block_sum(q, sh) / (float)n + eps);
    const float *rp = residual ? residual + base : nullptr;
    float *yp = y + base;
    for (int i = threadIdx.x * STEP; i < n; i += GN_THREADS * STEP) {
        const int c = g * cg + i / HW;                         // VEC: HW % 4 == 0, so the four share a channel
        const float a = gamma[c] * rstd, sft = beta[c] - mean * a;
        if (VEC) {
            const float4 t = *(const float4 *)(xp + i);
            float4 o = make_float4(t.x * a + sft, t.y * a + sft, t.z * a + sft, t.w * a + sft);
            if (rp) { const float4 r = *(const float4 *)(rp + i); o.x += r.x; o.y += r.y; o.z += r.z; o.w += r.w; }
            if (relu) { o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f); }
            *(float4 *)(yp + i) = o;
        } else {
            float o = xp[i] * a + sft;
            if (rp) o += rp[i];
            yp[i] = relu ? fmaxf(o, 0.f) : o;
        }
    }
}

// ---------------------------------------------------------------- max-pool 3x3 / 2, explicit padding with zeros (BiT pads, then pools)
__global__ __launch_bounds__(256) void maxpool3s2_kernel(const float *__restrict__ x, int H, int W, int pt, int pl, int Ho, int Wo, long long total,
                                                         float *__restrict__ y)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int xo = (int)(i % Wo), yo = (int)((i / Wo) % Ho);
    const long long plane = i / ((long long)Wo * Ho);
    const float *p = x + plane * H * W;
    float m = -INFINITY;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const int yy = yo * 2 - pt + dy, xx = xo * 2 - pl + dx;
            const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;
            m = fmaxf(m, in ? p[(size_t)yy * W + xx] : 0.f);
        }
    }
    y[i] = m;
}

// ---------------------------------------------------------------- LayerNorm, one wave per row, the row in registers (C <= 64 * LN_MAXPER)
constexpr int LN_MAXPER = 16;

__global__ __launch_bounds__(256) void layernorm_kernel(const float *x, int ldx, const float *__restrict__ gamma, const float *__restrict__ beta,
                                                        const float *residual, int ldr, long long rows, int C, float eps, float *out, int ldo)
{
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;                                     // no barrier below
    const int lane = lane_id(), per = C >> 6;
    const float *xr = x + r * ldx;
    float v[LN_MAXPER], s = 0.f;
#pragma unroll
    for (int i = 0; i < LN_MAXPER; ++i) { v[i] = i < per ? xr[lane + 64 * i] : 0.f; s += v[i]; }
    const float mean = wave_sum(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < LN_MAXPER; ++i) { const float d = i < per ? v[i] - mean : 0.f; q += d * d; }
    const float rstd = rsqrtf(wave_sum(q) / (float)C + eps);
#pragma unroll
    for (int i = 0; i < LN_MAXPER; ++i) {
        if (i < per) {
            const int c = lane + 64 * i;
            float o = (v[i] - mean) * rstd * gamma[c] + beta[c];
            if (residual) o += residual[r * ldr + c];
            out[r * ldo + c] = o;
        }
    }
}

// ---------------------------------------------------------------- x <- GELU_erf(x + bias), rows of N (N % 4 == 0), in place
__global__ __launch_bounds__(256) void bias_gelu_kernel(float *x, int ld, long long total4, int n4, const float *__restrict__ bias)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    const long long r = i / n4;
    const int c = (int)(i - r * n4) * 4;
    float4 *p = (float4 *)(x + r * ld + c);
    float4 t = *p;
    if (bias) { const float4 bb = *(const float4 *)(bias + c); t.x += bb.x; t.y += bb.y; t.z += bb.z; t.w += bb.w; }
    t.x = gelu_erf(t.x); t.y = gelu_erf(t.y); t.z = gelu_erf(t.z); t.w = gelu_erf(t.w);
    *p = t;
}

// ---------------------------------------------------------------- s = a (+ b);  sum <- s (optional), relu_out <- max(s, 0): the fusion layer's `hidden + residual_layer1(.)`
// together with the pre-activation ReLU of the residual unit that reads it (n % 4 == 0: feature maps of even sizes)
__global__ __launch_bounds__(256) void add_relu_kernel(const float4 *__restrict__ a, const float4 *__restrict__ b, long long n4, float4 *sum, float4 *relu_out)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    float4 s = a[i];
    if (b) { const float4 t = b[i]; s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w; }
    if (sum) sum[i] = s;
    relu_out[i] = make_float4(fmaxf(s.x, 0.f), fmaxf(s.y, 0.f), fmaxf(s.z, 0.f), fmaxf(s.w, 0.f));
}

// ---------------------------------------------------------------- tokens: a 64 (channels) x 64 (positions) tile transposed through LDS
// out[b][1 + p][c] = x[b][c][p] + pos[1 + p][c];  out[b][0][c] = cls[c] + pos[0][c]
__global__ __launch_bounds__(256) void tokens_kernel(const float *__restrict__ x, const float *__restrict__ cls, const float *__restrict__ pos, int C, int HW,
                                                     float *__restrict__ out, int ldo)
{
    __shared__ float tile[64][65];
    const int p0 = blockIdx.x * 64, c0 = blockIdx.y * 64, b = blockIdx.z;
    const int lo = threadIdx.x & 63, hi = threadIdx.x >> 6;
#pragma unroll 4
    for (int k = 0; k < 16; ++k) {
        const int c = k * 4 + hi;
        tile[c][lo] = (c0 + c < C && p0 + lo < HW) ? x[((size_t)b * C + c0 + c) * HW + p0 + lo] : 0.f;
    }
    __syncthreads();
    float *ob = out + (size_t)b * (HW + 1) * ldo;
    if (c0 + lo < C) {
#pragma unroll 4
        for (int k = 0; k < 16; ++k) {
            const int p = k * 4 + hi;
            if (p0 + p < HW) ob[(size_t)(1 + p0 + p) * ldo + c0 + lo] = tile[lo][p] + pos[(size_t)(1 + p0 + p) * C + c0 + lo];
        }
        if (blockIdx.x == 0 && hi == 0) ob[c0 + lo] = cls[c0 + lo] + pos[c0 + lo];
    }
}

// out[b][c][p] = act(rows[b][skip + p][c] + bias_img[b][c])
__global__ __launch_bounds__(256) void tokens_inverse_kernel(const float *__restrict__ rows, int ld, long long img_stride, int skip,
                                                             const float *__restrict__ bias_img, int gelu, int C, int HW, float *__restrict__ out)
{
    __shared__ float tile[64][65];
    const int p0 = blockIdx.x * 64, c0 = blockIdx.y * 64, b = blockIdx.z;
    const int lo = threadIdx.x & 63, hi = threadIdx.x >> 6;
    const float *rb = rows + (size_t)b * img_stride + (size_t)skip * ld;
#pragma unroll 4
    for (int k = 0; k < 16; ++k) {
        const int p = k * 4 + hi;
        tile[p][lo] = (p0 + p < HW && c0 + lo < C) ? rb[(size_t)(p0 + p) * ld + c0 + lo] : 0.f;
    }
    __syncthreads();
    if (p0 + lo >= HW) return;
#pragma unroll 4
    for (int k = 0; k < 16; ++k) {
        const int c = k * 4 + hi;
        if (c0 + c < C) {
            float v = tile[lo][c];
            if (bias_img) v += bias_img[(size_t)b * C + c0 + c];
            out[((size_t)b * C + c0 + c) * HW + p0 + lo] = gelu ? gelu_erf(v) : v;
        }
    }
}

// ---------------------------------------------------------------- pixel shuffle of a transposed convolution with kernel = stride = s
// out[b][co][h s + i][w s + j] = g[(b H + h) W + w][(co s + i) s + j] + bias[co]
__global__ __launch_bounds__(256) void shuffle_kernel(const float *__restrict__ g, int ld, const float *__restrict__ bias, int C, int H, int W, int s,
                                                      long long total, float *__restrict__ out)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int Wo = W * s, Ho = H * s;
    const int xo = (int)(idx % Wo), yo = (int)((idx / Wo) % Ho);
    const long long bc = idx / ((long long)Wo * Ho);
    const int co = (int)(bc % C);
    const long long b = bc / C;
    const int h = yo / s, i = yo - h * s, w = xo / s, j = xo - w * s;
    float v = g[((size_t)(b * H + h) * W + w) * ld + (size_t)(co * s + i) * s + j];
    if (bias) v += bias[co];
    out[idx] = v;
}

// ---------------------------------------------------------------- head tail (the body is dpt_tail.h's depth_tail, shared with csrc/depth_anything.hip)
// DPT-Hybrid's last activation: ReLU, then the optional 1 / (scale p + shift) of the KITTI / NYU checkpoints
struct HybridAct {
    int invert;
    float scale, shift;
    __device__ __forceinline__ float operator()(float a) const
    {
        a = fmaxf(a, 0.f);
        if (invert) a = 1.f / fmaxf(fmaf(scale, a, shift), 1e-8f);
        return a;
    }
};

template <bool ROWS>
__global__ __launch_bounds__(256) void head_tail_kernel(const float *__restrict__ f, const float *__restrict__ w, float bias, int C, int Hh, int Wh, int invert,
                                                        float scale, float shift, int Ho, int Wo, float sy, float sx, float *__restrict__ metres,
                                                        uint16_t *__restrict__ mm, const int *__restrict__ src, const int *__restrict__ dst, int B, int D,
                                                        int quantize, int *status)
{
    depth_tail<ROWS>(f, w, bias, C, Hh, Wh, HybridAct{invert, scale, shift}, Ho, Wo, sy, sx, metres, mm, src, dst, B, D, quantize, status);
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
inline unsigned blocks256(long long n) { return (unsigned)((n + 255) / 256); }
constexpr long long I31 = 0x7fffffffLL;

}  // namespace

extern "C" int mfr_dpt_prep(const void *img, int dtype, int B, int H, int W, float *out, int Hn, int Wn, void *stream)
{
    if (!img || !out || (dtype != 0 && dtype != 1) || B < 1 || B > 65535 || H < 1 || W < 1 || Hn < 32 || Wn < 32 || Hn % 32 || Wn % 32) return MFR_E_ARG;
    if ((long long)H * W * 3 > I31 || (long long)Hn * Wn * 3 > I31) return MFR_E_ARG;
    const float sy = (float)H / (float)Hn, sx = (float)W / (float)Wn;
    const dim3 grid(blocks256((long long)Hn * Wn), B);
    if (dtype == 0) hipLaunchKernelGGL((prep_kernel<true, false>), grid, dim3(256), 0, (hipStream_t)stream, img, H, W, Hn, Wn, sy, sx, out, nullptr, 0, nullptr);
    else hipLaunchKernelGGL((prep_kernel<false, false>), grid, dim3(256), 0, (hipStream_t)stream, img, H, W, Hn, Wn, sy, sx, out, nullptr, 0, nullptr);
    CHECK_LAUNCH();
    return 0;
}

extern "C" int mfr_dpt_groupnorm(const float *x, const float *gamma, const float *beta, const float *residual, int B, int C, int HW, int G, float eps, int relu,
                                 float *y, void *stream)
{
    if (!x || !gamma || !beta || !y || B < 1 || B > 65535 || C < 1 || HW < 1 || G < 1 || G > 65535 || C % G || !(eps >= 0.f) || (relu != 0 && relu != 1))
        return MFR_E_ARG;
    if ((long long)(C / G) * HW > I31 || (long long)B * C * HW > (1LL << 40)) return MFR_E_ARG;
    const bool vec = HW % 4 == 0 && aligned16(x) && aligned16(y) && (!residual || aligned16(residual));
    const dim3 grid(G, B);
    if (vec) hipLaunchKernelGGL(groupnorm_kernel<true>, grid, dim3(GN_THREADS), 0, (hipStream_t)stream, x, gamma, beta, residual, C, HW, G, eps, relu, y);
    else hipLaunchKernelGGL(groupnorm_kernel<false>, grid, dim3(GN_THREADS), 0, (hipStream_t)stream, x, gamma, beta, residual, C, HW, G, eps, relu, y);
    CHECK_LAUNCH();
    return 0;
}

extern "C" int mfr_dpt_maxpool3s2(const float *x, int planes, int H, int W, int pad_top, int pad_bottom, int pad_left, int pad_right, float *y, void *stream)
{
    if (!x || !y || planes < 1 || H < 1 || W < 1) return MFR_E_ARG;
    if (pad_top < 0 || pad_top > 2 || pad_bottom < 0 || pad_bottom > 2 || pad_left < 0 || pad_left > 2 || pad_right < 0 || pad_right > 2) return MFR_E_ARG;
    if (H + pad_top + pad_bottom < 3 || W + pad_left + pad_right < 3) return MFR_E_ARG;
    const int Ho = (H + pad_top + pad_bottom - 3) / 2 + 1, Wo = (W + pad_left + pad_right - 3) / 2 + 1;
    const long long total = (long long)planes * Ho * Wo;
    if ((long long)H * W > I31 || total > (1LL << 36)) return MFR_E_ARG;
    hipLaunchKernelGGL(maxpool3s2_kernel, dim3(blocks256(total)), dim3(256), 0, (hipStream_t)stream, x, H, W, pad_top, pad_left, Ho, Wo, total, y);
    CHECK_LAUNCH();
    return 0;
}

extern "C" int mfr_dpt_layernorm(const float *x, int ldx, const float *gamma, const float *beta, const float *residual, int ldr, long long rows, int C, float eps,
                                 float *out, int ldo, void *stream)
{
    if (!x || !gamma || !beta || !out || rows < 1 || rows > (1LL << 33) || C < 64 || C % 64 || C > 64 * LN_MAXPER || !(eps >= 0.f)) return MFR_E_ARG;
    if (ldx < C || ldo < C || (residual && ldr < C)) return MFR_E_ARG;
    hipLaunchKernelGGL(layernorm_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, ldx, gamma, beta, residual, ldr, rows, C, eps,
                       out, ldo);
    CHECK_LAUNCH();
    return 0;
}

extern "C" int mfr_dpt_bias_gelu(float *x, int ld, long long rows, int N, const float *bias, void *stream)
{
    if (!x || rows < 1 || N < 4 || N % 4 || ld < N || ld % 4 || !aligned16(x) || (bias && !aligned16(bias))) return MFR_E_ARG;
    const long long total4 = rows * (N / 4);
    if (total4 > (1LL << 36)) return MFR_E_ARG;
    hipLaunchKernelGGL(bias_gelu_kernel, dim3(blocks256(total4)), dim3(256), 0, (hipStream_t)stream, x, ld, total4, N / 4, bias);
    CHECK_LAUNCH();
    return 0;
}

extern "C" int mfr_dpt_add_relu(const float *a, const float *b, long long n, float *sum, float *relu_out, void *stream)
{
    if (!a || !relu_out || n < 4 || n % 4 || n > (1LL << 38) || !aligned16(a) || !aligned16(relu_out) || (b && !aligned16(b)) || (sum && !aligned16(sum))) return MFR_E_ARG;
    hipLaunchKernelGGL(add_relu_kernel, dim3(blocks256(n / 4)), dim3(256), 0, (hipStream_t)stream, (const float4 *)a, (const float4 *)b, n / 4, (float4 *)sum,
                       (float4 *)relu_out);
    CHECK_LAUNCH();
    return 0;
}

extern "C" int mfr_dpt_tokens(const float *x, const float *cls, const float *pos, int B, int C, int HW, float *out, int ldo, void *stream)
{
    if (!x || !cls || !pos || !out || B < 1 || B > 65535 || C < 1 || HW < 1 || ldo < C) return MFR_E_ARG;
    if ((C + 63) / 64 > 65535 || (long long)(HW + 1) * ldo > I31 || (long long)C * HW > I31) return MFR_E_ARG;
    hipLaunchKernelGGL(tokens_kernel, dim3((HW + 63) / 64, (C + 63) / 64, B), dim3(256), 0, (hipStream_t)stream, x, cls, pos, C, HW, out, ldo);
    CHECK_LAUNCH();
    return 0;
}

extern "C" int mfr_dpt_tokens_inverse(const float *rows, int ld, long long img_stride, int skip, const float *bias_img, int gelu, int B, int C, int HW, float *out,
                                      void *stream)
{
    if (!rows || !out || B < 1 || B > 65535 || C < 1 || HW < 1 || ld < C || skip < 0 || (gelu != 0 && gelu != 1)) return MFR_E_ARG;
    if (img_stride < (long long)(skip + HW - 1) * ld + C || (C + 63) / 64 > 65535 || (long long)C * HW > I31) return MFR_E_ARG;
    hipLaunchKernelGGL(tokens_inverse_kernel, dim3((HW + 63) / 64, (C + 63) / 64, B), dim3(256), 0, (hipStream_t)stream, rows, ld, img_stride, skip, bias_img, gelu,
                       C, HW, out);
    CHECK_LAUNCH();
    return 0;
}

extern "C" int mfr_dpt_shuffle(const float *g, int ld, const float *bias, int B, int C, int H, int W, int s, float *out, void *stream)
{
    if (!g || !out || B < 1 || C < 1 || H < 1 || W < 1 || (s != 2 && s != 4)) return MFR_E_ARG;
    if ((long long)C * s * s > I31 || ld < C * s * s) return MFR_E_ARG;
    const long long total = (long long)B * C * H * W * s * s;
    if (total > (1LL << 36) || (long long)B * H * W * ld > (1LL << 40)) return MFR_E_ARG;
    hipLaunchKernelGGL(shuffle_kernel, dim3(blocks256(total)), dim3(256), 0, (hipStream_t)stream, g, ld, bias, C, H, W, s, total, out);
    CHECK_LAUNCH();
    return 0;
}

extern "C" int mfr_dpt_head_tail(const float *f, const float *w, float bias, int B, int C, int Hh, int Wh, int invert, float scale, float shift, int Ho, int Wo,
                                 float *metres, uint16_t *mm, void *stream)
{
    if (!f || !w || !metres || B < 1 || B > 65535 || C < 1 || C > HEAD_MAX_C || Hh < 1 || Wh < 1 || Ho < 1 || Wo < 1 || (invert != 0 && invert != 1)) return MFR_E_ARG;
    if ((long long)Hh * Wh * C > I31 || (long long)Ho * Wo > I31 || (invert && !(scale == scale && shift == shift))) return MFR_E_ARG;
    const float sy = (float)Hh / (float)Ho, sx = (float)Wh / (float)Wo;
    hipLaunchKernelGGL(head_tail_kernel<false>, dim3(blocks256((long long)Ho * Wo), B), dim3(256), 0, (hipStream_t)stream, f, w, bias, C, Hh, Wh, invert, scale, shift, Ho,
                       Wo, sy, sx, metres, mm, nullptr, nullptr, B, B, 0, nullptr);
    CHECK_LAUNCH();
    return 0;
}

extern "C" int mfr_dpt_prep_rows(const uint8_t *img, int N, const int *rows, int m, int H, int W, float *out, int Hn, int Wn, int *status, void *stream)
{
    if (!img || !rows || !out || !status || N < 1 || m < 1 || m > 65535 || H < 1 || W < 1 || Hn < 32 || Wn < 32 || Hn % 32 || Wn % 32) return MFR_E_ARG;
    if ((long long)H * W * 3 > I31 || (long long)Hn * Wn * 3 > I31) return MFR_E_ARG;
    const float sy = (float)H / (float)Hn, sx = (float)W / (float)Wn;
    hipLaunchKernelGGL((prep_kernel<true, true>), dim3(blocks256((long long)Hn * Wn), m), dim3(256), 0, (hipStream_t)stream, (const void *)img, H, W, Hn, Wn, sy, sx,
                       out, rows, N, status);
    CHECK_LAUNCH();
    return 0;
}

extern "C" int mfr_dpt_head_tail_rows(const float *f, const float *w, float bias, int B, int C, int Hh, int Wh, int invert, float scale, float shift, int Ho, int Wo,
                                      const int *src, const int *dst, int d, float *metres, uint16_t *mm, int D, int quantize, int *status, void *stream)
{
    if (!f || !w || !metres || !src || !dst || !status || B < 1 || D < 1 || d < 1 || d > 65535 || C < 1 || C > HEAD_MAX_C || Hh < 1 || Wh < 1 || Ho < 1 || Wo < 1)
        return MFR_E_ARG;
    if ((invert != 0 && invert != 1) || (quantize != 0 && quantize != 1)) return MFR_E_ARG;
    if ((long long)Hh * Wh * C > I31 || (long long)Ho * Wo > I31 || (invert && !(scale == scale && shift == shift))) return MFR_E_ARG;
    const float sy = (float)Hh / (float)Ho, sx = (float)Wh / (float)Wo;
    hipLaunchKernelGGL(head_tail_kernel<true>, dim3(blocks256((long long)Ho * Wo), d), dim3(256), 0, (hipStream_t)stream, f, w, bias, C, Hh, Wh, invert, scale, shift,
                       Ho, Wo, sy, sx, metres, mm, src, dst, B, D, quantize, status);
    CHECK_LAUNCH();
    return 0;
}
