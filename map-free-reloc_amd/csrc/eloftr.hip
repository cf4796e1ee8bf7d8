// eloftr.hip -- the kernels of EfficientLoFTR (Wang et al., CVPR 2024; architecture of record: the `transformers` module
// EfficientLoFTRForKeypointMatching) that the project's convolution / GEMM / coarse-matching kernels do not cover (nets/eloftr.py):
//   * the 1 -> Cout stride-2 stem of the folded RepVGG backbone;
//   * the aggregation of the 1/8 token grid (depthwise 4x4/4 convolution for q, 4x4/4 max-pool for k / v, ONE LayerNorm for both);
//   * the rotary encoding in the module's interleaved-pair form, on the whole 256-vector;
//   * softmax attention for short sequences (8 heads x 32, a few hundred keys: a key tile of a head lives in LDS);
//   * the x4 bilinear up-sampling of the message into the right half of the MLP's [x | message] operand, the MLP's leaky ReLU;
//   * the fine pyramid's x2 bilinear up-sampling (align_corners=False) and the token-major -> NCHW hand-over;
//   * the fine windows (8x8 of image 0, padded 10x10 of image 1), read from the half-resolution map with the LAST x2 up-sampling evaluated
//     per window pixel, so that the full-resolution 64-channel map never exists;
//   * the two-stage fine matching, one wavefront per match, everything in LDS;
//   * the final drop of matches outside the unpadded frame, ordered compaction.
// fp32 storage and arithmetic throughout; every argument check returns MFR_E_ARG before any launch.
#include "wave_dev.h"

using namespace mfr;

#define EL_C 256            // hidden size
#define EL_AGG 4            // aggregation kernel = stride
#define EL_HD 32            // head dimension
#define EL_FC 64            // fine channels
#define EL_W0 8             // window of image 0
#define EL_W1 10            // window of image 1 (padding 1)
#define EL_S1 56            // first-stage channels

// ------------------------------------------------------------------------------------------ stem
// y [B,Cout,H/2,W/2] = relu(conv3x3(x [B,1,H,W], stride 2, pad 1) + bias); one thread per output pixel, the filters in LDS
__global__ void __launch_bounds__(256) el_stem_kernel(const float *__restrict__ x, const float *__restrict__ w, const float *__restrict__ bias, int H, int W,
                                                      int Cout, float *__restrict__ y)
{
    __shared__ float sw[64 * 9 + 64];
    for (int e = threadIdx.x; e < Cout * 9; e += 256) sw[e] = w[e];
    for (int e = threadIdx.x; e < Cout; e += 256) sw[64 * 9 + e] = bias ? bias[e] : 0.f;
    __syncthreads();
    const int Ho = H >> 1, Wo = W >> 1, b = blockIdx.y;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= Ho * Wo) return;
    const int oy = p / Wo, ox = p - oy * Wo;
    float t[9];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int iy = 2 * oy - 1 + ky, ix = 2 * ox - 1 + kx;             // <= H - 1, <= W - 1 for even H, W
            t[ky * 3 + kx] = (iy >= 0 && ix >= 0) ? x[((size_t)b * H + iy) * W + ix] : 0.f;
        }
    float *yo = y + (size_t)b * Cout * Ho * Wo + p;
    for (int c = 0; c < Cout; ++c) {
        float s = sw[64 * 9 + c];
#pragma unroll
        for (int k = 0; k < 9; ++k) s += sw[c * 9 + k] * t[k];
        yo[(size_t)c * Ho * Wo] = fmaxf(s, 0.f);
    }
}

// ------------------------------------------------------------------------------------------ aggregation + LayerNorm
// sum of a value over the 256 threads (4 wavefronts) of the block, the same bits in every thread
MFR_DEV float el_block_sum(float v, float *sred)
{
    v = wave_sum(v);
    __syncthreads();                                                          // the previous use of sred has been read
    if ((threadIdx.x & 63) == 0) sred[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sred[0] + sred[1]) + (sred[2] + sred[3]);
}

// one workgroup per aggregated cell, thread = channel: the 16 tokens of the cell are read once (coalesced rows) for both outputs
__global__ void __launch_bounds__(EL_C) el_aggregate_kernel(const float *__restrict__ x, int ldx, long long img_stride, int hc, int wc,
                                                            const float *__restrict__ wq, const float *__restrict__ gamma, const float *__restrict__ beta, float eps,
                                                            float *__restrict__ q_out, float *__restrict__ kv_out)
{
    __shared__ float sred[4];
    const int ha = hc / EL_AGG, wa = wc / EL_AGG;
    const int cell = blockIdx.x % (ha * wa), img = blockIdx.x / (ha * wa);
    const int ay = cell / wa, ax = cell - ay * wa, c = threadIdx.x;
    const float *xi = x + (size_t)img * img_stride;
    float q = 0.f, kv = -INFINITY;
#pragma unroll
    for (int ky = 0; ky < EL_AGG; ++ky)
#pragma unroll
        for (int kx = 0; kx < EL_AGG; ++kx) {
            const float v = xi[((size_t)(ay * EL_AGG + ky) * wc + ax * EL_AGG + kx) * ldx + c];
            q += wq[c * (EL_AGG * EL_AGG) + ky * EL_AGG + kx] * v;
            kv = fmaxf(kv, v);
        }
    const float g = gamma[c], bt = beta[c];
    const size_t o = (size_t)blockIdx.x * EL_C + c;
    // two-pass statistics, biased variance, rsqrt(var + eps): the arithmetic of mfr_layernorm
    if (q_out) {
        const float mean = el_block_sum(q, sred) * (1.f / EL_C);
        const float d = q - mean;
        const float var = el_block_sum(d * d, sred) * (1.f / EL_C);
        q_out[o] = d * rsqrtf(var + eps) * g + bt;
    }
    if (kv_out) {
        const float mean = el_block_sum(kv, sred) * (1.f / EL_C);
        const float d = kv - mean;
        const float var = el_block_sum(d * d, sred) * (1.f / EL_C);
        kv_out[o] = d * rsqrtf(var + eps) * g + bt;
    }
}

// ------------------------------------------------------------------------------------------ rotary
// rows of q (and k) [nb * La, 256], row stride ld; cs [La, 256] = cos [128] | sin [128] of the row's 128 angles; pair (2 i, 2 i + 1) turns by angle i
__global__ void __launch_bounds__(256) el_rotary_kernel(float *__restrict__ q, float *__restrict__ k, int ld, const float *__restrict__ cs, long long rows, int La)
{
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= rows * (EL_C / 2)) return;
    const long long r = e / (EL_C / 2);
    const int i = (int)(e - r * (EL_C / 2)), pos = (int)(r % La);
    const float c = cs[(size_t)pos * EL_C + i], s = cs[(size_t)pos * EL_C + EL_C / 2 + i];
    float2 *pq = (float2 *)(q + (size_t)r * ld) + i;
    const float2 a = *pq;
    *pq = make_float2(a.x * c - a.y * s, a.y * c + a.x * s);
    if (k) {
        float2 *pk = (float2 *)(k + (size_t)r * ld) + i;
        const float2 b = *pk;
        *pk = make_float2(b.x * c - b.y * s, b.y * c + b.x * s);
    }
}

// ------------------------------------------------------------------------------------------ short-sequence softmax attention
// one wavefront per (64 queries, head, image): a lane owns one query (q and the 32 accumulators in registers); keys and values of the head
// pass through LDS in tiles of 64, read as broadcasts (every lane reads the same key).  Online softmax, one rescale per 8 keys.
#define EL_KT 64
__global__ void __launch_bounds__(64) el_attention_kernel(const float *__restrict__ Q, int ldq, const float *__restrict__ K, const float *__restrict__ V, int ldkv,
                                                          int Lq, int Lk, float scale, float *__restrict__ O, int ldo)
{
    __shared__ float4 sk[EL_KT * (EL_HD / 4)], sv[EL_KT * (EL_HD / 4)];
    const int lane = threadIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int qi = blockIdx.x * 64 + lane, qr = qi < Lq ? qi : Lq - 1;             // tail lanes repeat the last query and store nothing
    const float4 *qp = (const float4 *)(Q + ((size_t)b * Lq + qr) * ldq + h * EL_HD);
    float q[EL_HD], acc[EL_HD];
#pragma unroll
    for (int c = 0; c < EL_HD / 4; ++c) {
        const float4 t = qp[c];
        q[4 * c] = t.x; q[4 * c + 1] = t.y; q[4 * c + 2] = t.z; q[4 * c + 3] = t.w;
    }
#pragma unroll
    for (int c = 0; c < EL_HD; ++c) acc[c] = 0.f;
    float m = -INFINITY, l = 0.f;
    const float *Kb = K + (size_t)b * Lk * ldkv + h * EL_HD, *Vb = V + (size_t)b * Lk * ldkv + h * EL_HD;
    for (int k0 = 0; k0 < Lk; k0 += EL_KT) {
        __syncthreads();
        for (int e = lane; e < EL_KT * (EL_HD / 4); e += 64) {
            const int key = e >> 3, piece = e & 7;
            float4 kk = make_float4(0.f, 0.f, 0.f, 0.f), vv = kk;
            if (k0 + key < Lk) {
                kk = ((const float4 *)(Kb + (size_t)(k0 + key) * ldkv))[piece];
                vv = ((const float4 *)(Vb + (size_t)(k0 + key) * ldkv))[piece];
            }
            sk[e] = kk; sv[e] = vv;
        }
        __syncthreads();
        const int nk = Lk - k0 < EL_KT ? Lk - k0 : EL_KT;
        for (int g = 0; g < nk; g += 8) {
            float s[8];
            float gm = m;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float d = 0.f;
#pragma unroll
                for (int c = 0; c < EL_HD / 4; ++c) {
                    const float4 t = sk[(g + j) * (EL_HD / 4) + c];
                    d += q[4 * c] * t.x + q[4 * c + 1] * t.y + q[4 * c + 2] * t.z + q[4 * c + 3] * t.w;
                }
                s[j] = (g + j < nk) ? d * scale : -INFINITY;
                gm = fmaxf(gm, s[j]);
            }
            const float corr = expf(m - gm);                                    // m = -inf the first time: 0 (key 0 always exists, so gm is finite)
            l *= corr;
#pragma unroll
            for (int c = 0; c < EL_HD; ++c) acc[c] *= corr;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float p = expf(s[j] - gm);
                l += p;
#pragma unroll
                for (int c = 0; c < EL_HD / 4; ++c) {
                    const float4 t = sv[(g + j) * (EL_HD / 4) + c];
                    acc[4 * c] += p * t.x; acc[4 * c + 1] += p * t.y; acc[4 * c + 2] += p * t.z; acc[4 * c + 3] += p * t.w;
                }
            }
            m = gm;
        }
    }
    if (qi < Lq) {
        const float inv = 1.f / l;
        float4 *op = (float4 *)(O + ((size_t)b * Lq + qi) * ldo + h * EL_HD);
#pragma unroll
        for (int c = 0; c < EL_HD / 4; ++c) op[c] = make_float4(acc[4 * c] * inv, acc[4 * c + 1] * inv, acc[4 * c + 2] * inv, acc[4 * c + 3] * inv);
    }
}

// ------------------------------------------------------------------------------------------ bilinear up-sampling, align_corners = False
// torch's source index for an output index: max(scale * (dst + 0.5) - 0.5, 0), scale = 1 / factor; the upper neighbour clamps at the edge
MFR_DEV void el_src(int dst, float scale, int n, int &i0, int &i1, float &l0, float &l1)
{
    float s = scale * ((float)dst + 0.5f) - 0.5f;
    if (s < 0.f) s = 0.f;
    i0 = (int)s;
    if (i0 > n - 1) i0 = n - 1;
    i1 = i0 + (i0 < n - 1 ? 1 : 0);
    l1 = s - (float)i0; l0 = 1.f - l1;
}

// msg [nimg, ha * wa, 256] (row stride ldm) -> dst rows of the 4 ha x 4 wa token grid (row stride ldx, image stride img_stride): 256 channels
// per token, the right half of the MLP's operand
__global__ void __launch_bounds__(256) el_up4_kernel(const float *__restrict__ msg, int ldm, int ha, int wa, float *__restrict__ dst, int ldx, long long img_stride,
                                                     long long total)
{
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int c4 = (int)(e & (EL_C / 4 - 1));
    const long long tok = e >> 6;
    const int hc = ha * EL_AGG, wc = wa * EL_AGG;
    const int img = (int)(tok / (hc * wc)), p = (int)(tok - (long long)img * hc * wc);
    const int y = p / wc, x = p - y * wc;
    int y0, y1, x0, x1; float ly0, ly1, lx0, lx1;
    el_src(y, 1.f / EL_AGG, ha, y0, y1, ly0, ly1);
    el_src(x, 1.f / EL_AGG, wa, x0, x1, lx0, lx1);
    const float *mi = msg + (size_t)img * ha * wa * ldm;
    const float4 a = ((const float4 *)(mi + (size_t)(y0 * wa + x0) * ldm))[c4], b = ((const float4 *)(mi + (size_t)(y0 * wa + x1) * ldm))[c4];
    const float4 c = ((const float4 *)(mi + (size_t)(y1 * wa + x0) * ldm))[c4], d = ((const float4 *)(mi + (size_t)(y1 * wa + x1) * ldm))[c4];
    float4 o;
    o.x = ly0 * (lx0 * a.x + lx1 * b.x) + ly1 * (lx0 * c.x + lx1 * d.x);
    o.y = ly0 * (lx0 * a.y + lx1 * b.y) + ly1 * (lx0 * c.y + lx1 * d.y);
    o.z = ly0 * (lx0 * a.z + lx1 * b.z) + ly1 * (lx0 * c.z + lx1 * d.z);
    o.w = ly0 * (lx0 * a.w + lx1 * b.w) + ly1 * (lx0 * c.w + lx1 * d.w);
    ((float4 *)(dst + (size_t)img * img_stride + (size_t)p * ldx))[c4] = o;
}

// out [planes, 2H, 2W] = (add ? add : 0) + up2(in [planes, H, W])
__global__ void __launch_bounds__(256) el_up2_kernel(const float *__restrict__ in, const float *__restrict__ add, float *__restrict__ out, int H, int W, long long total)
{
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int Wo = 2 * W, Ho = 2 * H;
    const long long pl = e / ((long long)Ho * Wo);
    const int p = (int)(e - pl * Ho * Wo), y = p / Wo, x = p - y * Wo;
    int y0, y1, x0, x1; float ly0, ly1, lx0, lx1;
    el_src(y, 0.5f, H, y0, y1, ly0, ly1);
    el_src(x, 0.5f, W, x0, x1, lx0, lx1);
    const float *ip = in + (size_t)pl * H * W;
    const float v = ly0 * (lx0 * ip[y0 * W + x0] + lx1 * ip[y0 * W + x1]) + ly1 * (lx0 * ip[y1 * W + x0] + lx1 * ip[y1 * W + x1]);
    out[e] = add ? add[e] + v : v;
}

__global__ void __launch_bounds__(256) el_leaky_kernel(float *__restrict__ x, int ld, int n4, long long total, float slope)
{
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const long long r = e / n4;
    float4 *p = (float4 *)(x + (size_t)r * ld) + (e - r * n4);
    float4 v = *p;
    v.x = v.x > 0.f ? v.x : v.x * slope; v.y = v.y > 0.f ? v.y : v.y * slope;
    v.z = v.z > 0.f ? v.z : v.z * slope; v.w = v.w > 0.f ? v.w : v.w * slope;
    *p = v;
}

// out [img][c][p] = x[img][p][c] * scale : 32 x 32 tiles through LDS (C % 32 == 0)
__global__ void __launch_bounds__(256) el_rows_to_nchw_kernel(const float *__restrict__ x, int ldx, long long img_stride, int C, int HW, float scale, float *__restrict__ out)
{
    __shared__ float t[32][33];
    const int img = blockIdx.z, p0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8)
        t[r][tx] = (p0 + r < HW) ? x[(size_t)img * img_stride + (size_t)(p0 + r) * ldx + c0 + tx] * scale : 0.f;
    __syncthreads();
    for (int r = ty; r < 32; r += 8)
        if (p0 + tx < HW) out[((size_t)img * C + c0 + r) * HW + p0 + tx] = t[tx][r];
}

// ------------------------------------------------------------------------------------------ fine windows
// feat [nimg, Hh, Wh, 64] NHWC at HALF resolution; a window pixel (Y, X) of the full-resolution frame (2 Hh x 2 Wh) is the x2 bilinear
// up-sampling (align_corners=False) of feat evaluated at that pixel; pixels outside the frame are zero (unfold's padding).
// slot = blockIdx.x = b * maxN + s; slots s >= min(n[b], maxN) are left untouched.  Window origin: cell corner - pad.
__global__ void __launch_bounds__(256) el_gather_kernel(const float *__restrict__ feat, int nimg, int Hh, int Wh, const int *__restrict__ img_ids, const int *__restrict__ cell_ids,
                                                        long long ld_cells, const int *__restrict__ n, int maxN, int wc, int cell_px, int win, int pad,
                                                        float *__restrict__ out)
{
    const int b = blockIdx.x / maxN, s = blockIdx.x - b * maxN;
    const int nb = n[b] < maxN ? n[b] : maxN;
    if (s >= nb) return;
    int img = img_ids[b];
    img = img < 0 ? 0 : (img > nimg - 1 ? nimg - 1 : img);                    // a bad table entry reads the wrong image, never beyond the maps
    const int cell = cell_ids[(size_t)b * ld_cells + s];
    const int Y0 = (cell / wc) * cell_px - pad, X0 = (cell % wc) * cell_px - pad;
    const int total4 = win * win * (EL_FC / 4);
    const float4 *f4 = (const float4 *)(feat + (size_t)img * Hh * Wh * EL_FC);
    float4 *o4 = (float4 *)out + (size_t)blockIdx.x * total4;
    for (int e = threadIdx.x; e < total4; e += 256) {
        const int k = e >> 4, q = e & 15;
        const int ky = k / win, Y = Y0 + ky, X = X0 + (k - ky * win);
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (Y >= 0 && Y < 2 * Hh && X >= 0 && X < 2 * Wh) {
            int y0, y1, x0, x1; float ly0, ly1, lx0, lx1;
            el_src(Y, 0.5f, Hh, y0, y1, ly0, ly1);
            el_src(X, 0.5f, Wh, x0, x1, lx0, lx1);
            const float4 a = f4[((size_t)y0 * Wh + x0) * (EL_FC / 4) + q], bb = f4[((size_t)y0 * Wh + x1) * (EL_FC / 4) + q];
            const float4 c = f4[((size_t)y1 * Wh + x0) * (EL_FC / 4) + q], d = f4[((size_t)y1 * Wh + x1) * (EL_FC / 4) + q];
            o.x = ly0 * (lx0 * a.x + lx1 * bb.x) + ly1 * (lx0 * c.x + lx1 * d.x);
            o.y = ly0 * (lx0 * a.y + lx1 * bb.y) + ly1 * (lx0 * c.y + lx1 * d.y);
            o.z = ly0 * (lx0 * a.z + lx1 * bb.z) + ly1 * (lx0 * c.z + lx1 * d.z);
            o.w = ly0 * (lx0 * a.w + lx1 * bb.w) + ly1 * (lx0 * c.w + lx1 * d.w);
        }
        o4[e] = o;
    }
}

// ------------------------------------------------------------------------------------------ two-stage fine matching
// One wavefront per match.  Lane i owns row i of the 64 x 100 correlation: its window-0 feature in registers, window 1 in LDS (read as
// broadcasts), the correlation in LDS with an odd row pitch (101: the row pass -- lane = row -- and the column pass -- lane = column -- are
// both free of bank conflicts).
//   stage 1: first 56 channels, both sides / sqrt(56); softmax over rows x softmax over columns on the 64 x 100 matrix, THEN the interior 8 x 8
//            of the 10 x 10; arg-max over the flattened 64 x 64 (lowest index on ties); offsets grid - 4 + 0.5 on both sides;
//   stage 2: last 8 channels, window 1 / sqrt(8); the 3 x 3 values of the PADDED 10 x 10 grid at the UNPADDED winner index + {-1, 0, 1} (-1 wraps
//            to 9, as a negative index does in the module); softmax(. / 10), expectation of {-1, 0, 1}^2, added to image 1's point.
#define EL_SP 101
__global__ void __launch_bounds__(64) el_fine_match_kernel(const float *__restrict__ w0, const float *__restrict__ w1, const int *__restrict__ cell_i,
                                                           const int *__restrict__ cell_j, long long ld_cells, const int *__restrict__ n, int maxN, int wc,
                                                           float cell_px, float *__restrict__ pts0, float *__restrict__ pts1, int *__restrict__ arg_out)
{
    __shared__ float4 sb[EL_W1 * EL_W1 * (EL_FC / 4)];
    __shared__ float sS[64 * EL_SP];
    __shared__ float scm[EL_W1 * EL_W1], scs[EL_W1 * EL_W1], sh[9];
    const int b = blockIdx.x / maxN, s = blockIdx.x - b * maxN, lane = threadIdx.x;
    const int nb = n[b] < maxN ? n[b] : maxN;
    if (s >= nb) return;
    const float r56 = sqrtf((float)EL_S1), r8 = sqrtf((float)(EL_FC - EL_S1));
    const float4 *src1 = (const float4 *)w1 + (size_t)blockIdx.x * (EL_W1 * EL_W1 * (EL_FC / 4));
    for (int e = lane; e < EL_W1 * EL_W1 * (EL_FC / 4); e += 64) {
        float4 v = src1[e];
        const float d = (e & 15) < EL_S1 / 4 ? r56 : r8;
        v.x /= d; v.y /= d; v.z /= d; v.w /= d;
        sb[e] = v;
    }
    float a[EL_FC];
    const float4 *src0 = (const float4 *)w0 + ((size_t)blockIdx.x * 64 + lane) * (EL_FC / 4);
#pragma unroll
    for (int c = 0; c < EL_FC / 4; ++c) {
        const float4 t = src0[c];
        a[4 * c] = t.x; a[4 * c + 1] = t.y; a[4 * c + 2] = t.z; a[4 * c + 3] = t.w;
    }
#pragma unroll
    for (int c = 0; c < EL_S1; ++c) a[c] /= r56;
    __syncthreads();
    // stage 1: the lane's row of the correlation, its maximum and its sum of exponentials
    float rm = -INFINITY;
    for (int j = 0; j < EL_W1 * EL_W1; ++j) {
        float d = 0.f;
#pragma unroll
        for (int c = 0; c < EL_S1 / 4; ++c) {
            const float4 t = sb[j * (EL_FC / 4) + c];
            d += a[4 * c] * t.x + a[4 * c + 1] * t.y + a[4 * c + 2] * t.z + a[4 * c + 3] * t.w;
        }
        sS[lane * EL_SP + j] = d;
        rm = fmaxf(rm, d);
    }
    float rs = 0.f;
    for (int j = 0; j < EL_W1 * EL_W1; ++j) rs += expf(sS[lane * EL_SP + j] - rm);
    __syncthreads();
    for (int j = lane; j < EL_W1 * EL_W1; j += 64) {
        float cm = -INFINITY, cs = 0.f;
        for (int i = 0; i < 64; ++i) cm = fmaxf(cm, sS[i * EL_SP + j]);
        for (int i = 0; i < 64; ++i) cs += expf(sS[i * EL_SP + j] - cm);
        scm[j] = cm; scs[j] = cs;
    }
    __syncthreads();
    float best = -1.f; int idx = lane * 64;
    for (int jy = 1; jy <= EL_W0; ++jy)
        for (int jx = 1; jx <= EL_W0; ++jx) {
            const int j = jy * EL_W1 + jx;
            const float v = sS[lane * EL_SP + j];
            const float conf = (expf(v - scm[j]) / scs[j]) * (expf(v - rm) / rs);
            if (conf > best) { best = conf; idx = lane * 64 + (jy - 1) * EL_W0 + (jx - 1); }
        }
    wave_argmax(best, idx);
    const int i1 = idx >> 6, j1 = idx & 63;
    // stage 2: the winner row's last 8 channels, from the lane that holds them
    float ai[EL_FC - EL_S1];
#pragma unroll
    for (int c = 0; c < EL_FC - EL_S1; ++c) ai[c] = __shfl(a[EL_S1 + c], i1, 64);
    if (lane < 9) {
        int rr = j1 / EL_W0 + lane / 3 - 1, cc = j1 % EL_W0 + lane % 3 - 1;
        if (rr < 0) rr += EL_W1;
        if (cc < 0) cc += EL_W1;
        const float4 t0 = sb[(rr * EL_W1 + cc) * (EL_FC / 4) + EL_S1 / 4], t1 = sb[(rr * EL_W1 + cc) * (EL_FC / 4) + EL_S1 / 4 + 1];
        const float d = ai[0] * t0.x + ai[1] * t0.y + ai[2] * t0.z + ai[3] * t0.w + ai[4] * t1.x + ai[5] * t1.y + ai[6] * t1.z + ai[7] * t1.w;
        sh[lane] = d / 10.f;
    }
    __syncthreads();
    if (lane == 0) {
        float hm = sh[0];
        for (int t = 1; t < 9; ++t) hm = fmaxf(hm, sh[t]);
        float e[9], sum = 0.f;
        for (int t = 0; t < 9; ++t) { e[t] = expf(sh[t] - hm); sum += e[t]; }
        float ex = 0.f, ey = 0.f;
        for (int t = 0; t < 9; ++t) { const float p = e[t] / sum; ex += (float)(t % 3 - 1) * p; ey += (float)(t / 3 - 1) * p; }
        const int ci = cell_i[(size_t)b * ld_cells + s], cj = cell_j[(size_t)b * ld_cells + s];
        const float half = (float)(EL_W0 / 2) - 0.5f;
        pts0[2 * (size_t)blockIdx.x] = (float)(ci % wc) * cell_px + ((float)(i1 % EL_W0) - half);
        pts0[2 * (size_t)blockIdx.x + 1] = (float)(ci / wc) * cell_px + ((float)(i1 / EL_W0) - half);
        pts1[2 * (size_t)blockIdx.x] = (float)(cj % wc) * cell_px + ((float)(j1 % EL_W0) - half) + ex;
        pts1[2 * (size_t)blockIdx.x + 1] = (float)(cj / wc) * cell_px + ((float)(j1 / EL_W0) - half) + ey;
        if (arg_out) arg_out[blockIdx.x] = idx;
    }
}

// ------------------------------------------------------------------------------------------ frame test + ordered compaction
// one workgroup per pair: the first min(n[b], maxN) slots in order, those with both endpoints inside the unpadded frame (x < W, y < H) kept
__global__ void __launch_bounds__(256) el_compact_kernel(const float *__restrict__ p0, const float *__restrict__ p1, const float *__restrict__ conf, long long ld_conf,
                                                         const int *__restrict__ n, int maxN, float W, float H, float *__restrict__ o0, float *__restrict__ o1,
                                                         float *__restrict__ oc, int *__restrict__ n_out)
{
    __shared__ Compact256 cs;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int nb = n[b] < maxN ? n[b] : maxN;
    int total = 0;
    for (int start = 0; start < maxN; start += 256) {
        const int s = start + tid;
        bool valid = false;
        float2 a = make_float2(0.f, 0.f), c = a;
        if (s < nb) {
            a = ((const float2 *)p0)[(size_t)b * maxN + s]; c = ((const float2 *)p1)[(size_t)b * maxN + s];
            valid = a.x < W && a.y < H && c.x < W && c.y < H;
        }
        const int o = compact256_slot(cs, valid, total);
        if (valid) {
            ((float2 *)o0)[(size_t)b * maxN + o] = a; ((float2 *)o1)[(size_t)b * maxN + o] = c;
            oc[(size_t)b * maxN + o] = conf[(size_t)b * ld_conf + s];
        }
    }
    for (int s = total + tid; s < maxN; s += 256) {
        ((float2 *)o0)[(size_t)b * maxN + s] = make_float2(0.f, 0.f); ((float2 *)o1)[(size_t)b * maxN + s] = make_float2(0.f, 0.f);
        oc[(size_t)b * maxN + s] = 0.f;
    }
    if (tid == 0) n_out[b] = total;
}

// ------------------------------------------------------------------------------------------ C ABI
static inline bool el_al16(const void *p) { return !((uintptr_t)p & 15); }
static inline unsigned el_blocks(long long total) { return (unsigned)((total + 255) / 256); }

extern "C" {

int mfr_eloftr_stem_s2(const float *x, const float *w, const float *bias, int B, int H, int W, int out_channels, float *y, void *stream)
{
    if (!x || !w || !y || B <= 0 || B > 65535 || H <= 0 || W <= 0 || (H & 1) || (W & 1) || out_channels <= 0 || out_channels > 64) return MFR_E_ARG;
    const long long px = (long long)(H / 2) * (W / 2);
    hipLaunchKernelGGL(el_stem_kernel, dim3(el_blocks(px), B), dim3(256), 0, (hipStream_t)stream, x, w, bias, H, W, out_channels, y);
    CHECK_LAUNCH();
    return 0;
}

int mfr_eloftr_aggregate(const float *x, int ldx, long long img_stride, int nimg, int hc, int wc, const float *wq, const float *gamma, const float *beta, float eps,
                         float *q_out, float *kv_out, void *stream)
{
    if (!x || !wq || !gamma || !beta || (!q_out && !kv_out) || nimg <= 0 || hc <= 0 || wc <= 0 || (hc % EL_AGG) || (wc % EL_AGG) || ldx < EL_C ||
        img_stride < (long long)hc * wc * ldx)
        return MFR_E_ARG;
    const long long blocks = (long long)nimg * (hc / EL_AGG) * (wc / EL_AGG);
    if (blocks > 0x7fffffffLL) return MFR_E_ARG;
    hipLaunchKernelGGL(el_aggregate_kernel, dim3((unsigned)blocks), dim3(EL_C), 0, (hipStream_t)stream, x, ldx, img_stride, hc, wc, wq, gamma, beta, eps, q_out, kv_out);
    CHECK_LAUNCH();
    return 0;
}

int mfr_eloftr_rotary(float *q, float *k, int ld, const float *cos_sin, long long rows, int La, void *stream)
{
    if (!q || !cos_sin || rows <= 0 || La <= 0 || (rows % La) || ld < EL_C || (ld & 1) || ((uintptr_t)q & 7) || ((uintptr_t)k & 7)) return MFR_E_ARG;
    const long long total = rows * (EL_C / 2);
    if ((total + 255) / 256 > 0x7fffffffLL) return MFR_E_ARG;
    hipLaunchKernelGGL(el_rotary_kernel, dim3(el_blocks(total)), dim3(256), 0, (hipStream_t)stream, q, k, ld, cos_sin, rows, La);
    CHECK_LAUNCH();
    return 0;
}

int mfr_eloftr_attention(const float *q, int ldq, const float *k, const float *v, int ldkv, int nb, int Lq, int Lk, int heads, float *out, int ldo, void *stream)
{
    if (!q || !k || !v || !out || nb <= 0 || nb > 65535 || Lq <= 0 || Lk <= 0 || heads <= 0 || heads > 65535 || ldq < heads * EL_HD || ldkv < heads * EL_HD ||
        ldo < heads * EL_HD || (ldq & 3) || (ldkv & 3) || (ldo & 3) || !el_al16(q) || !el_al16(k) || !el_al16(v) || !el_al16(out))
        return MFR_E_ARG;
    hipLaunchKernelGGL(el_attention_kernel, dim3((Lq + 63) / 64, heads, nb), dim3(64), 0, (hipStream_t)stream, q, ldq, k, v, ldkv, Lq, Lk,
                       1.f / sqrtf((float)EL_HD), out, ldo);
    CHECK_LAUNCH();
    return 0;
}

int mfr_eloftr_upsample4_rows(const float *msg, int ldm, int nimg, int ha, int wa, float *dst, int ldx, long long img_stride, void *stream)
{
    if (!msg || !dst || nimg <= 0 || ha <= 0 || wa <= 0 || ldm < EL_C || ldx < EL_C || (ldm & 3) || (ldx & 3) || (img_stride & 3) || !el_al16(msg) || !el_al16(dst) ||
        img_stride < (long long)ha * wa * EL_AGG * EL_AGG * ldx)
        return MFR_E_ARG;
    const long long total = (long long)nimg * ha * wa * EL_AGG * EL_AGG * (EL_C / 4);
    if ((total + 255) / 256 > 0x7fffffffLL) return MFR_E_ARG;
    hipLaunchKernelGGL(el_up4_kernel, dim3(el_blocks(total)), dim3(256), 0, (hipStream_t)stream, msg, ldm, ha, wa, dst, ldx, img_stride, total);
    CHECK_LAUNCH();
    return 0;
}

int mfr_eloftr_upsample2x(const float *in, const float *add, float *out, int planes, int H, int W, void *stream)
{
    if (!in || !out || planes <= 0 || H <= 0 || W <= 0) return MFR_E_ARG;
    const long long total = (long long)planes * H * W * 4;
    if ((long long)H * W * 4 > 0x7fffffffLL || (total + 255) / 256 > 0x7fffffffLL) return MFR_E_ARG;
    hipLaunchKernelGGL(el_up2_kernel, dim3(el_blocks(total)), dim3(256), 0, (hipStream_t)stream, in, add, out, H, W, total);
    CHECK_LAUNCH();
    return 0;
}

int mfr_eloftr_leaky_relu(float *x, int ld, long long rows, int N, float slope, void *stream)
{
    if (!x || rows <= 0 || N <= 0 || (N & 3) || ld < N || (ld & 3) || !el_al16(x)) return MFR_E_ARG;
    const long long total = rows * (N / 4);
    if ((total + 255) / 256 > 0x7fffffffLL) return MFR_E_ARG;
    hipLaunchKernelGGL(el_leaky_kernel, dim3(el_blocks(total)), dim3(256), 0, (hipStream_t)stream, x, ld, N / 4, total, slope);
    CHECK_LAUNCH();
    return 0;
}

int mfr_eloftr_rows_to_nchw(const float *x, int ldx, long long img_stride, int nimg, int C, int HW, float scale, float *out, void *stream)
{
    if (!x || !out || nimg <= 0 || nimg > 65535 || C <= 0 || (C % 32) || C / 32 > 65535 || HW <= 0 || ldx < C || img_stride < (long long)HW * ldx) return MFR_E_ARG;
    hipLaunchKernelGGL(el_rows_to_nchw_kernel, dim3((HW + 31) / 32, C / 32, nimg), dim3(256), 0, (hipStream_t)stream, x, ldx, img_stride, C, HW, scale, out);
    CHECK_LAUNCH();
    return 0;
}

int mfr_eloftr_gather_windows(const float *feat_half, int nimg, int Hh, int Wh, int C, const int32_t *img_ids, const int32_t *cell_ids, long long ld_cells,
                              const int32_t *n, int B, int maxN, int wc, int cell_px, int win, int pad, float *out, void *stream)
{
    if (!feat_half || !img_ids || !cell_ids || !n || !out || nimg <= 0 || Hh <= 0 || Wh <= 0 || C != EL_FC || B <= 0 || maxN <= 0 || ld_cells < maxN || wc <= 0 ||
        cell_px <= 0 || win <= 0 || win > 16 || pad < 0 || !el_al16(feat_half) || !el_al16(out) || (long long)B * maxN > 0x7fffffffLL)
        return MFR_E_ARG;
    hipLaunchKernelGGL(el_gather_kernel, dim3((unsigned)((long long)B * maxN)), dim3(256), 0, (hipStream_t)stream, feat_half, nimg, Hh, Wh, img_ids, cell_ids, ld_cells, n,
                       maxN, wc, cell_px, win, pad, out);
    CHECK_LAUNCH();
    return 0;
}

int mfr_eloftr_fine_match(const float *win0, const float *win1, const int32_t *cell_i, const int32_t *cell_j, long long ld_cells, const int32_t *n, int B, int maxN,
                          int wc, int cell_px, float *pts0, float *pts1, int32_t *stage1_arg, void *stream)
{
    if (!win0 || !win1 || !cell_i || !cell_j || !n || !pts0 || !pts1 || B <= 0 || maxN <= 0 || ld_cells < maxN || wc <= 0 || cell_px <= 0 || !el_al16(win0) ||
        !el_al16(win1) || (long long)B * maxN > 0x7fffffffLL)
        return MFR_E_ARG;
    hipLaunchKernelGGL(el_fine_match_kernel, dim3((unsigned)((long long)B * maxN)), dim3(64), 0, (hipStream_t)stream, win0, win1, cell_i, cell_j, ld_cells, n, maxN, wc,
                       (float)cell_px, pts0, pts1, stage1_arg);
    CHECK_LAUNCH();
    return 0;
}

int mfr_eloftr_compact(const float *pts0, const float *pts1, const float *conf, long long ld_conf, const int32_t *n, int B, int maxN, int W, int H, float *out0,
                       float *out1, float *out_conf, int32_t *n_out, void *stream)
{
    if (!pts0 || !pts1 || !conf || !n || !out0 || !out1 || !out_conf || !n_out || B <= 0 || maxN <= 0 || ld_conf < maxN || W <= 0 || H <= 0 || ((uintptr_t)pts0 & 7) ||
        ((uintptr_t)pts1 & 7) || ((uintptr_t)out0 & 7) || ((uintptr_t)out1 & 7))
        return MFR_E_ARG;
    hipLaunchKernelGGL(el_compact_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, pts0, pts1, conf, ld_conf, n, maxN, (float)W, (float)H, out0, out1, out_conf,
                       n_out);
    CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
