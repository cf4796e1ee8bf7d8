// sift.hip -- SIFT keypoint detection and description (OpenCV 4.8 SIFT_create(nfeatures), default parameters) on gfx950.
//
// Reference call sites: SIFTMatching (lib/models/matching/feature_matching.py:58,82-83: SIFT_create(cfg.SIFT.NUM_FEATURES)
// .detectAndCompute) and SIFT_matcher (etc/feature_matching_baselines/matchers.py:146-147: SIFT_create(2048)).  The semantics,
// step by step with every constant, are tabled in sift_ops.py's docstring; tests/sift_cpu_ref.py restates them in numpy f32
// and the pyramid, keypoints and descriptors here are pinned against it bit for bit (tests/test_gpu_sift.py).  This TU is
// compiled with -ffp-contract=off (EXACT_SRCS): every f32 multiply and add is rounded on its own, in the order written;
// divides, square roots and transcendentals go through binary64 and are rounded once to f32.
//
// Stages (all launches batched over B images of one size, on the caller's stream, no host synchronisation):
//   base      u8 -> f32, 2x bilinear upsample (half-pixel centres, clamped), into level 1 of octave 0 (scratch)
//   blur      separable Gaussian, row pass then column pass, reflect-101, both passes on one LDS tile (halo <= SIFT_MAXR)
//   down      level 0 of octave o = every second pixel of level 3 of octave o-1
//   extrema   one thread per pixel of an octave: DoG formed on the fly from the Gaussian levels (same f32 subtraction),
//             26-neighbour test on DoG layers 1..3, Newton refinement, contrast and edge tests; survivors appended to a
//             per-image candidate buffer (capacity SIFT_CCAP; overflow -> status bit MFR_SIFT_ST_CAND_OVERFLOW)
//   orient    one wavefront per candidate: 36-bin histogram with lane b owning bin b, samples added in OpenCV's row-major
//             order (broadcast by shuffles), [1 4 6 4 1]/16 smoothing, 0.8-peaks -> keypoints (capacity SIFT_KCAP)
//   select    one workgroup per image: bitonic sort of the keypoint indices on (x asc, y asc, size desc, angle asc,
//             response desc, octave desc), duplicate removal, radix select of the nfeatures-th largest response
//             (retainBest keeps every tie), ordered compaction into the caller's arrays
//   desc      one wavefront per keypoint: 4x4x8 histogram over a (d+2)^2 cell grid, lane c owning cell c's 10 bins,
//             samples in OpenCV's row-major order; normalise, clip at 0.2, rescale by 512, saturate to 0..255
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mfr_hip.h"
#include "wave_dev.h"

using namespace mfr;

#define SIFT_LAYERS 3            // nOctaveLayers
#define SIFT_LEVELS 6            // Gaussian images per octave (nOctaveLayers + 3)
#define SIFT_MAXR 16             // largest blur radius the tile supports (the largest used is 13: sigma 3.09, 27 taps)
#define SIFT_BORDER 5            // SIFT_IMG_BORDER
#define SIFT_MAX_OCT 16
#define SIFT_CCAP 16384          // default candidates per image (refined extrema); the caller may ask for fewer
#define SIFT_KCAP 16384          // keypoints per image before selection (power of two: the bitonic sort's width)
#define SIFT_TILE 32

struct SiftKernel { float c[SIFT_MAXR + 1]; int R; };          // c[0] centre tap, c[i] the two taps at distance i
struct SiftCand { int o, layer, r, c; float xc, xr, xi, contr; };
struct SiftKp { float x, y, size, angle, response; int octave; float pad0, pad1; };

__device__ __forceinline__ float div_rn(float a, float b) { return (float)((double)a / (double)b); }
__device__ __forceinline__ float sqrt_rn(float a) { return (float)sqrt((double)a); }
__device__ __forceinline__ float exp_rn(float a) { return (float)exp((double)a); }

__device__ __forceinline__ int refl101(int p, int len)         // cv::borderInterpolate(BORDER_REFLECT_101)
{
    if (len == 1) return 0;
    do {
        if (p < 0) p = -p;
        else p = len - 1 - (p - len) - 1;
    } while ((unsigned)p >= (unsigned)len);
    return p;
}

// cv::fastAtan2 (degrees, [0, 360]): OpenCV's degree-7 polynomial, plain f32 arithmetic
__device__ __forceinline__ float fast_atan2(float y, float x)
{
    const float k = (float)(180.0 / 3.14159265358979323846);
    const float p1 = 0.9997878412794807f * k, p3 = -0.3258083974640975f * k;
    const float p5 = 0.1555786518463281f * k, p7 = -0.04432655554792128f * k;
    const float ax = fabsf(x), ay = fabsf(y);
    float a, c, c2;
    if (ax >= ay) {
        c = div_rn(ay, ax + (float)2.220446049250313e-16);
        c2 = c * c;
        a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    } else {
        c = div_rn(ax, ay + (float)2.220446049250313e-16);
        c2 = c * c;
        a = 90.f - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    }
    if (x < 0) a = 180.f - a;
    if (y < 0) a = 360.f - a;
    return a;
}

// ---- base image: u8 -> f32, 2x bilinear (src = dst/2 - 1/4, clamped); every value is a multiple of 1/16 below 256: exact ----
__global__ void __launch_bounds__(256) sift_base_kernel(const uint8_t *__restrict__ gray, int H, int W, float *__restrict__ dst)
{
    const int W2 = 2 * W, H2 = 2 * H;
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
    if (x >= W2) return;
    const uint8_t *g = gray + (size_t)b * H * W;
    const int xa = (x & 1) ? (x >> 1) : max((x >> 1) - 1, 0), xb = (x & 1) ? min((x >> 1) + 1, W - 1) : (x >> 1);
    const float wxa = (x & 1) ? 0.75f : 0.25f, wxb = (x & 1) ? 0.25f : 0.75f;
    const int ya = (y & 1) ? (y >> 1) : max((y >> 1) - 1, 0), yb = (y & 1) ? min((y >> 1) + 1, H - 1) : (y >> 1);
    const float wya = (y & 1) ? 0.75f : 0.25f, wyb = (y & 1) ? 0.25f : 0.75f;
    const float ha = wxa * (float)g[(size_t)ya * W + xa] + wxb * (float)g[(size_t)ya * W + xb];
    const float hb = wxa * (float)g[(size_t)yb * W + xa] + wxb * (float)g[(size_t)yb * W + xb];
    dst[((size_t)b * H2 + y) * W2 + x] = wya * ha + wyb * hb;
}

// ---- separable Gaussian: acc = c0 p[0] + sum_i c_i (p[-i] + p[+i]), i = 1..R in order; rows first, then columns ----
__global__ void __launch_bounds__(256) sift_blur_kernel(const float *__restrict__ src, float *__restrict__ dst, int H, int W,
                                                        SiftKernel k)
{
    __shared__ float in_s[SIFT_TILE + 2 * SIFT_MAXR][SIFT_TILE + 2 * SIFT_MAXR + 1];
    __shared__ float mid_s[SIFT_TILE + 2 * SIFT_MAXR][SIFT_TILE + 1];
    const int R = k.R, span = SIFT_TILE + 2 * R;
    const int x0 = blockIdx.x * SIFT_TILE, y0 = blockIdx.y * SIFT_TILE, b = blockIdx.z, tid = threadIdx.x;
    const float *s = src + (size_t)b * H * W;
    for (int i = tid; i < span * span; i += 256) {
        const int yy = i / span, xx = i - yy * span;
        in_s[yy][xx] = s[(size_t)refl101(y0 - R + yy, H) * W + refl101(x0 - R + xx, W)];
    }
    __syncthreads();
    for (int i = tid; i < span * SIFT_TILE; i += 256) {
        const int yy = i / SIFT_TILE, xx = i - yy * SIFT_TILE;
        float acc = k.c[0] * in_s[yy][xx + R];
        for (int t = 1; t <= R; ++t) acc = acc + k.c[t] * (in_s[yy][xx + R - t] + in_s[yy][xx + R + t]);
        mid_s[yy][xx] = acc;
    }
    __syncthreads();
    float *d = dst + (size_t)b * H * W;
    for (int i = tid; i < SIFT_TILE * SIFT_TILE; i += 256) {
        const int yy = i / SIFT_TILE, xx = i - yy * SIFT_TILE;
        if (y0 + yy >= H || x0 + xx >= W) continue;
        float acc = k.c[0] * mid_s[yy + R][xx];
        for (int t = 1; t <= R; ++t) acc = acc + k.c[t] * (mid_s[yy + R - t][xx] + mid_s[yy + R + t][xx]);
        d[(size_t)(y0 + yy) * W + x0 + xx] = acc;
    }
}

// ---- next octave: every second pixel (INTER_NEAREST to floor(W/2) x floor(H/2)) ----
__global__ void __launch_bounds__(256) sift_down_kernel(const float *__restrict__ src, int Hs, int Ws, float *__restrict__ dst,
                                                        int H, int W)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
    if (x >= W) return;
    dst[((size_t)b * H + y) * W + x] = src[((size_t)b * Hs + 2 * y) * Ws + 2 * x];
}

struct SiftOctave { const float *g[SIFT_LEVELS]; int H, W, o; };

__device__ __forceinline__ float dog_at(const SiftOctave &O, size_t img, int l, int r, int c)
{
    const size_t p = img + (size_t)r * O.W + c;
    return O.g[l + 1][p] - O.g[l][p];
}

// adjustLocalExtrema: up to 5 Newton steps (3x3 system by Cramer's rule in binary64), contrast and edge tests
__device__ bool sift_refine(const SiftOctave &O, size_t img, int &layer, int &r, int &c, float &xc, float &xr, float &xi, float &contr)
{
    const float img_scale = 1.f / 255.f, deriv_scale = img_scale * 0.5f, second_deriv_scale = img_scale,
                cross_deriv_scale = img_scale * 0.25f;
    int i = 0;
    xi = xr = xc = 0.f;
    for (; i < 5; ++i) {
        const float v = dog_at(O, img, layer, r, c);
        const float dx = (dog_at(O, img, layer, r, c + 1) - dog_at(O, img, layer, r, c - 1)) * deriv_scale;
        const float dy = (dog_at(O, img, layer, r + 1, c) - dog_at(O, img, layer, r - 1, c)) * deriv_scale;
        const float ds = (dog_at(O, img, layer + 1, r, c) - dog_at(O, img, layer - 1, r, c)) * deriv_scale;
        const float v2 = v * 2.f;
        const float dxx = (dog_at(O, img, layer, r, c + 1) + dog_at(O, img, layer, r, c - 1) - v2) * second_deriv_scale;
        const float dyy = (dog_at(O, img, layer, r + 1, c) + dog_at(O, img, layer, r - 1, c) - v2) * second_deriv_scale;
        const float dss = (dog_at(O, img, layer + 1, r, c) + dog_at(O, img, layer - 1, r, c) - v2) * second_deriv_scale;
        const float dxy = (dog_at(O, img, layer, r + 1, c + 1) - dog_at(O, img, layer, r + 1, c - 1) - dog_at(O, img, layer, r - 1, c + 1) +
                           dog_at(O, img, layer, r - 1, c - 1)) * cross_deriv_scale;
        const float dxs = (dog_at(O, img, layer + 1, r, c + 1) - dog_at(O, img, layer + 1, r, c - 1) - dog_at(O, img, layer - 1, r, c + 1) +
                           dog_at(O, img, layer - 1, r, c - 1)) * cross_deriv_scale;
        const float dys = (dog_at(O, img, layer + 1, r + 1, c) - dog_at(O, img, layer + 1, r - 1, c) - dog_at(O, img, layer - 1, r + 1, c) +
                           dog_at(O, img, layer - 1, r - 1, c)) * cross_deriv_scale;
        // H = [dxx dxy dxs; dxy dyy dys; dxs dys dss], X = H^-1 (dx, dy, ds)
        const double a00 = dxx, a01 = dxy, a02 = dxs, a11 = dyy, a12 = dys, a22 = dss, b0 = dx, b1 = dy, b2 = ds;
        const double det = a00 * (a11 * a22 - a12 * a12) - a01 * (a01 * a22 - a02 * a12) + a02 * (a01 * a12 - a02 * a11);
        float X0 = 0.f, X1 = 0.f, X2 = 0.f;
        if (det != 0.0) {
            X0 = (float)((b0 * (a11 * a22 - a12 * a12) - a01 * (b1 * a22 - a12 * b2) + a02 * (b1 * a12 - a11 * b2)) / det);
            X1 = (float)((a00 * (b1 * a22 - a12 * b2) - b0 * (a01 * a22 - a12 * a02) + a02 * (a01 * b2 - b1 * a02)) / det);
            X2 = (float)((a00 * (a11 * b2 - b1 * a12) - a01 * (a01 * b2 - b1 * a02) + b0 * (a01 * a12 - a11 * a02)) / det);
        }
        xi = -X2; xr = -X1; xc = -X0;
        if (fabsf(xi) < 0.5f && fabsf(xr) < 0.5f && fabsf(xc) < 0.5f) break;
        if (fabsf(xi) > (float)(INT_MAX / 3) || fabsf(xr) > (float)(INT_MAX / 3) || fabsf(xc) > (float)(INT_MAX / 3)) return false;
        c += (int)rintf(xc); r += (int)rintf(xr); layer += (int)rintf(xi);
        if (layer < 1 || layer > SIFT_LAYERS || c < SIFT_BORDER || c >= O.W - SIFT_BORDER || r < SIFT_BORDER || r >= O.H - SIFT_BORDER)
            return false;
    }
    if (i >= 5) return false;
    const float v = dog_at(O, img, layer, r, c);
    const float dx = (dog_at(O, img, layer, r, c + 1) - dog_at(O, img, layer, r, c - 1)) * deriv_scale;
    const float dy = (dog_at(O, img, layer, r + 1, c) - dog_at(O, img, layer, r - 1, c)) * deriv_scale;
    const float ds = (dog_at(O, img, layer + 1, r, c) - dog_at(O, img, layer - 1, r, c)) * deriv_scale;
    const float t = dx * xc + dy * xr + ds * xi;
    contr = v * img_scale + t * 0.5f;
    if (fabsf(contr) * (float)SIFT_LAYERS < 0.04f) return false;
    const float v2 = v * 2.f;
    const float dxx = (dog_at(O, img, layer, r, c + 1) + dog_at(O, img, layer, r, c - 1) - v2) * second_deriv_scale;
    const float dyy = (dog_at(O, img, layer, r + 1, c) + dog_at(O, img, layer, r - 1, c) - v2) * second_deriv_scale;
    const float dxy = (dog_at(O, img, layer, r + 1, c + 1) - dog_at(O, img, layer, r + 1, c - 1) - dog_at(O, img, layer, r - 1, c + 1) +
                       dog_at(O, img, layer, r - 1, c - 1)) * cross_deriv_scale;
    const float tr = dxx + dyy, det = dxx * dyy - dxy * dxy;
    if (det <= 0.f || tr * tr * 10.f >= 121.f * det) return false;
    return true;
}

__global__ void __launch_bounds__(256) sift_extrema_kernel(SiftOctave O, SiftCand *__restrict__ cand, int ccap,
                                                           int *__restrict__ ccount, int *__restrict__ status)
{
    const int c = blockIdx.x * 16 + (threadIdx.x & 15), r = blockIdx.y * 16 + (threadIdx.x >> 4), b = blockIdx.z;
    if (r < SIFT_BORDER || r >= O.H - SIFT_BORDER || c < SIFT_BORDER || c >= O.W - SIFT_BORDER) return;
    const size_t img = (size_t)b * O.H * O.W;
    const float threshold = 1.f;                              // cvFloor(0.5 * 0.04 / 3 * 255)
    for (int layer = 1; layer <= SIFT_LAYERS; ++layer) {
        const float val = dog_at(O, img, layer, r, c);
        if (!(fabsf(val) > threshold)) continue;
        bool ext = true;
        for (int l = layer - 1; l <= layer + 1 && ext; ++l)
            for (int dy = -1; dy <= 1 && ext; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    if (l == layer && dy == 0 && dx == 0) continue;
                    const float n = dog_at(O, img, l, r + dy, c + dx);
                    if (val > 0 ? !(val >= n) : !(val <= n)) { ext = false; break; }
                }
        if (!ext) continue;
        int ly = layer, rr = r, cc = c;
        float xc, xr, xi, contr;
        if (!sift_refine(O, img, ly, rr, cc, xc, xr, xi, contr)) continue;
        const int slot = atomicAdd(&ccount[b], 1);
        if (slot < ccap) {
            SiftCand k; k.o = O.o; k.layer = ly; k.r = rr; k.c = cc; k.xc = xc; k.xr = xr; k.xi = xi; k.contr = contr;
            cand[(size_t)b * ccap + slot] = k;
        } else {
            atomicOr(&status[b], MFR_SIFT_ST_CAND_OVERFLOW);
        }
    }
}

struct SiftPyr { const float *g[SIFT_MAX_OCT][SIFT_LEVELS]; int H[SIFT_MAX_OCT], W[SIFT_MAX_OCT]; int n_oct; };

// ---- orientation: one wavefront per candidate; lane j < 36 owns histogram bin j ----
__global__ void __launch_bounds__(256) sift_orient_kernel(SiftPyr P, const SiftCand *__restrict__ cand, int ccap, const int *__restrict__ ccount,
                                                          SiftKp *__restrict__ kps, int *__restrict__ kcount, int *__restrict__ status)
{
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int nc = min(ccount[b], ccap);
    const int nw = gridDim.x * 4;
    for (int ci = blockIdx.x * 4 + (threadIdx.x >> 6); ci < nc; ci += nw) {
        const SiftCand k = cand[(size_t)b * ccap + ci];
        const int o = k.o, H = P.H[o], W = P.W[o];
        const float *img = P.g[o][k.layer] + (size_t)b * H * W;
        const float po = (float)(1 << o);
        const float ptx = ((float)k.c + k.xc) * po, pty = ((float)k.r + k.xr) * po;
        const int octave = o + (k.layer << 8) + ((int)rint(((double)k.xi + 0.5) * 255) << 16);
        const float size = 1.6f * (float)exp2((double)div_rn((float)k.layer + k.xi, (float)SIFT_LAYERS)) * po * 2.f;
        const float response = fabsf(k.contr);
        const float scl_octv = size * 0.5f / po;
        const int radius = (int)rintf(4.5f * scl_octv);
        const float sigma = 1.5f * scl_octv;
        const float expf_scale = div_rn(-1.f, 2.f * sigma * sigma);
        const int side = 2 * radius + 1, len = side * side;
        float h = 0.f;
        for (int p0 = 0; p0 < len; p0 += 64) {
            const int p = p0 + lane;
            const int i = p / side - radius, j = p - (p / side) * side - radius;
            const int y = k.r + i, x = k.c + j;
            int bin = -1;
            float val = 0.f;
            if (p < len && y > 0 && y < H - 1 && x > 0 && x < W - 1) {
                const float dx = img[(size_t)y * W + x + 1] - img[(size_t)y * W + x - 1];
                const float dy = img[(size_t)(y - 1) * W + x] - img[(size_t)(y + 1) * W + x];
                const float w = exp_rn((float)(i * i + j * j) * expf_scale);
                const float ori = fast_atan2(dy, dx);
                const float mag = sqrt_rn(dx * dx + dy * dy);
                bin = (int)rintf((36.f / 360.f) * ori);
                if (bin >= 36) bin -= 36;
                if (bin < 0) bin += 36;
                val = w * mag;
            }
            for (int s = 0; s < 64; ++s) {                    // in sample order: each bin's sum is OpenCV's sequential sum
                const int bs = __shfl(bin, s, 64);
                const float vs = __shfl(val, s, 64);
                if (bs == lane) h = h + vs;
            }
        }
        const int l1 = lane == 0 ? 35 : lane - 1, r1 = lane == 35 ? 0 : lane + 1;
        const int l2 = lane < 2 ? lane + 34 : lane - 2, r2 = lane > 33 ? lane - 34 : lane + 2;
        const float tl1 = __shfl(h, l1, 64), tr1 = __shfl(h, r1, 64), tl2 = __shfl(h, l2, 64), tr2 = __shfl(h, r2, 64);
        const float hist = (tl2 + tr2) * (1.f / 16.f) + (tl1 + tr1) * (4.f / 16.f) + h * (6.f / 16.f);
        const float m = wave_max(lane < 36 ? hist : -INFINITY);
        const float mag_thr = m * 0.8f;
        const float hl = __shfl(hist, l1, 64), hr = __shfl(hist, r1, 64);
        if (lane < 36 && hist > hl && hist > hr && hist >= mag_thr) {
            float bin = (float)lane + div_rn(0.5f * (hl - hr), hl - 2.f * hist + hr);
            bin = bin < 0.f ? 36.f + bin : bin >= 36.f ? bin - 36.f : bin;
            float angle = 360.f - (10.f * bin);
            if (fabsf(angle - 360.f) < 1.1920928955078125e-7f) angle = 0.f;
            const int slot = atomicAdd(&kcount[b], 1);
            if (slot < SIFT_KCAP) {
                SiftKp q;                                     // the input frame (firstOctave = -1): pt, size halved, octave byte - 1
                q.x = ptx * 0.5f; q.y = pty * 0.5f; q.size = size * 0.5f; q.angle = angle; q.response = response;
                q.octave = (octave & ~255) | ((octave - 1) & 255); q.pad0 = q.pad1 = 0.f;
                kps[(size_t)b * SIFT_KCAP + slot] = q;
            } else {
                atomicOr(&status[b], MFR_SIFT_ST_KPT_OVERFLOW);
            }
        }
    }
}

// "a before b" in the order removeDuplicatedSorted leaves (KeyPoint_LessThan); index -1 (padding) sorts last
__device__ __forceinline__ bool kp_before(const SiftKp *__restrict__ kp, int a, int b)
{
    if (a < 0) return false;
    if (b < 0) return true;
    const SiftKp p = kp[a], q = kp[b];
    if (p.x != q.x) return p.x < q.x;
    if (p.y != q.y) return p.y < q.y;
    if (p.size != q.size) return p.size > q.size;
    if (p.angle != q.angle) return p.angle < q.angle;
    if (p.response != q.response) return p.response > q.response;
    if (p.octave != q.octave) return p.octave > q.octave;
    return a < b;
}

__global__ void __launch_bounds__(1024) sift_select_kernel(const SiftKp *__restrict__ kps_all, const int *__restrict__ kcount, int nfeatures,
                                                           int Nmax, float *__restrict__ kpts, float *__restrict__ osize,
                                                           float *__restrict__ oangle, float *__restrict__ oresp, int *__restrict__ ooct,
                                                           int *__restrict__ n_out, int *__restrict__ status)
{
    __shared__ int idx[SIFT_KCAP];
    __shared__ unsigned char keep[SIFT_KCAP];
    __shared__ int hist[256];
    __shared__ int wave_cnt[16];
    __shared__ int sh_prefix, sh_want, sh_base;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const SiftKp *kp = kps_all + (size_t)b * SIFT_KCAP;
    const int M = min(kcount[b], SIFT_KCAP);
    int P = 1;
    while (P < M) P <<= 1;
    for (int i = tid; i < P; i += 1024) idx[i] = i < M ? i : -1;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += 1024) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const int a = idx[i], c = idx[ixj];
                    const bool up = (i & k) == 0;
                    if (up ? kp_before(kp, c, a) : kp_before(kp, a, c)) { idx[i] = c; idx[ixj] = a; }
                }
            }
            __syncthreads();
        }
    // removeDuplicatedSorted: drop a keypoint equal to its predecessor in (x, y, size, angle)
    int nkeep = 0;
    for (int i = tid; i < M; i += 1024) {
        bool kk = true;
        if (i > 0) {
            const SiftKp p = kp[idx[i - 1]], q = kp[idx[i]];
            kk = p.x != q.x || p.y != q.y || p.size != q.size || p.angle != q.angle;
        }
        keep[i] = kk;
        nkeep += kk;
    }
    if (tid == 0) { sh_prefix = 0; sh_want = 0; }
    __syncthreads();
    atomicAdd(&sh_want, nkeep);
    __syncthreads();
    const int K = sh_want;
    __syncthreads();
    unsigned thr_bits = 0u;
    if (nfeatures > 0 && K > nfeatures) {
        // retainBest: keep every keypoint whose response >= the nfeatures-th largest (MSB-first radix select on the f32 bits)
        if (tid == 0) sh_want = nfeatures;
        unsigned mask = 0u;
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (tid < 256) hist[tid] = 0;
            __syncthreads();
            const unsigned prefix = (unsigned)sh_prefix;
            for (int i = tid; i < M; i += 1024) {
                if (!keep[i]) continue;
                const unsigned u = __float_as_uint(kp[idx[i]].response);
                if ((u & mask) == prefix) atomicAdd(&hist[(u >> shift) & 255], 1);
            }
            __syncthreads();
            if (tid == 0) {
                int want = sh_want, acc = 0, d = 255;
                for (; d > 0; --d) {
                    if (acc + hist[d] >= want) break;
                    acc += hist[d];
                }
                sh_want = want - acc;
                sh_prefix = (int)(prefix | ((unsigned)d << shift));
            }
            mask |= 255u << shift;
            __syncthreads();
        }
        thr_bits = (unsigned)sh_prefix;
    }
    // ordered compaction of the kept set
    if (tid == 0) sh_base = 0;
    __syncthreads();
    for (int start = 0; start < M; start += 1024) {
        const int i = start + tid;
        bool sel = false;
        if (i < M && keep[i]) sel = __float_as_uint(kp[idx[i]].response) >= thr_bits;
        const unsigned long long bal = __ballot(sel);
        const int wpre = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wave_cnt[wid] = __popcll(bal);
        __syncthreads();
        int off = sh_base;
        for (int w = 0; w < wid; ++w) off += wave_cnt[w];
        if (sel) {
            const int o = off + wpre;
            if (o < Nmax) {
                const SiftKp q = kp[idx[i]];
                const size_t r = (size_t)b * Nmax + o;
                kpts[2 * r] = q.x; kpts[2 * r + 1] = q.y;
                osize[r] = q.size; oangle[r] = q.angle; oresp[r] = q.response; ooct[r] = q.octave;
            }
        }
        __syncthreads();
        if (tid == 0) {
            int t = 0;
            for (int w = 0; w < 16; ++w) t += wave_cnt[w];
            sh_base += t;
        }
        __syncthreads();
    }
    if (tid == 0) {
        n_out[b] = min(sh_base, Nmax);
        if (sh_base > Nmax) atomicOr(&status[b], MFR_SIFT_ST_OUT_OVERFLOW);
    }
}

// ---- descriptor: one wavefront per keypoint; lane c < 36 owns cell (c / 6, c % 6) of the (d+2) x (d+2) grid, 10 bins each ----
__global__ void __launch_bounds__(256) sift_desc_kernel(SiftPyr P, const float *__restrict__ kpts, const float *__restrict__ ksize,
                                                        const float *__restrict__ kangle, const int *__restrict__ koct,
                                                        const int *__restrict__ n_in, int Nmax, float *__restrict__ desc)
{
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int kid = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (kid >= min(n_in[b], Nmax)) return;
    const size_t row = (size_t)b * Nmax + kid;
    // unpackOctave
    const int ow = koct[row];
    int octave = ow & 255;
    const int layer = (ow >> 8) & 255;
    octave = octave < 128 ? octave : (-128 | octave);
    const float scale = octave >= 0 ? 1.f / (float)(1 << octave) : (float)(1 << -octave);
    const int o = octave + 1;
    if (o < 0 || o >= P.n_oct || layer < 0 || layer >= SIFT_LEVELS) return;
    const int H = P.H[o], W = P.W[o];
    const float *img = P.g[o][layer] + (size_t)b * H * W;
    const float size = ksize[row] * scale;
    const float ptfx = kpts[2 * row] * scale, ptfy = kpts[2 * row + 1] * scale;
    float ori = 360.f - kangle[row];
    if (fabsf(ori - 360.f) < 1.1920928955078125e-7f) ori = 0.f;
    const float scl = size * 0.5f;
    // calcSIFTDescriptor(img, ptf, ori, scl, d = 4, n = 8)
    const int ptx = (int)rintf(ptfx), pty = (int)rintf(ptfy);
    const float arg = ori * (float)(3.14159265358979323846 / 180);
    float cos_t = (float)cos((double)arg), sin_t = (float)sin((double)arg);
    const float bins_per_rad = 8.f / 360.f;
    const float exp_scale = -1.f / (4 * 4 * 0.5f);
    const float hist_width = 3.f * scl;
    int radius = (int)rintf(hist_width * 1.4142135623730951f * (4 + 1) * 0.5f);
    radius = min(radius, (int)sqrt((double)W * W + (double)H * H));
    cos_t = div_rn(cos_t, hist_width);
    sin_t = div_rn(sin_t, hist_width);
    const int side = 2 * radius + 1, len = side * side;
    const int cr = lane / 6, cc = lane - (lane / 6) * 6;
    float h[10];
#pragma unroll
    for (int q = 0; q < 10; ++q) h[q] = 0.f;
    for (int p0 = 0; p0 < len; p0 += 64) {
        const int p = p0 + lane;
        const int i = p / side - radius, j = p - (p / side) * side - radius;
        int code = -1;                                        // r0+1 | (c0+1) << 4 | o0 << 8, or -1
        float rbin = 0.f, cbin = 0.f, obin = 0.f, mag = 0.f;
        if (p < len) {
            const float c_rot = (float)j * cos_t - (float)i * sin_t;
            const float r_rot = (float)j * sin_t + (float)i * cos_t;
            rbin = r_rot + 2.f - 0.5f;
            cbin = c_rot + 2.f - 0.5f;
            const int r = pty + i, c = ptx + j;
            if (rbin > -1.f && rbin < 4.f && cbin > -1.f && cbin < 4.f && r > 0 && r < H - 1 && c > 0 && c < W - 1) {
                const float dx = img[(size_t)r * W + c + 1] - img[(size_t)r * W + c - 1];
                const float dy = img[(size_t)(r - 1) * W + c] - img[(size_t)(r + 1) * W + c];
                const float w = exp_rn((c_rot * c_rot + r_rot * r_rot) * exp_scale);
                const float Ori = fast_atan2(dy, dx);
                const float Mag = sqrt_rn(dx * dx + dy * dy);
                obin = (Ori - ori) * bins_per_rad;
                mag = Mag * w;
                const int r0 = (int)floorf(rbin), c0 = (int)floorf(cbin);
                int o0 = (int)floorf(obin);
                rbin -= (float)r0; cbin -= (float)c0; obin -= (float)o0;
                if (o0 < 0) o0 += 8;
                if (o0 >= 8) o0 -= 8;
                code = (r0 + 1) | ((c0 + 1) << 4) | (o0 << 8);
            }
        }
        for (int s = 0; s < 64; ++s) {
            const int cs = __shfl(code, s, 64);
            if (cs < 0) continue;                             // uniform across the wave
            const float rb = __shfl(rbin, s, 64), cb = __shfl(cbin, s, 64), ob = __shfl(obin, s, 64), mg = __shfl(mag, s, 64);
            const int dr = cr - (cs & 15), dc = cc - ((cs >> 4) & 15), o0 = cs >> 8;
            if (lane < 36 && (unsigned)dr <= 1u && (unsigned)dc <= 1u) {
                const float v_r1 = mg * rb, v_r0 = mg - v_r1;
                const float v_r = dr ? v_r1 : v_r0;
                const float v_rc1 = v_r * cb, v_rc0 = v_r - v_rc1;
                const float v_rc = dc ? v_rc1 : v_rc0;
                const float v1 = v_rc * ob, v0 = v_rc - v1;
#pragma unroll
                for (int q = 0; q < 10; ++q) {
                    if (q == o0) h[q] = h[q] + v0;
                    if (q == o0 + 1) h[q] = h[q] + v1;
                }
            }
        }
    }
    // circular wrap, then the 128 values in (row, col, bin) order: the norms are sequential sums in that order (every lane the same)
    h[0] = h[0] + h[8];
    h[1] = h[1] + h[9];
    float nrm2 = 0.f;
    for (int cell = 0; cell < 16; ++cell) {
        const int src = ((cell >> 2) + 1) * 6 + (cell & 3) + 1;
#pragma unroll
        for (int q = 0; q < 8; ++q) { const float v = __shfl(h[q], src, 64); nrm2 = nrm2 + v * v; }
    }
    const float thr = sqrt_rn(nrm2) * 0.2f;
    float nrm2b = 0.f;
    for (int cell = 0; cell < 16; ++cell) {
        const int src = ((cell >> 2) + 1) * 6 + (cell & 3) + 1;
#pragma unroll
        for (int q = 0; q < 8; ++q) { const float v = fminf(__shfl(h[q], src, 64), thr); nrm2b = nrm2b + v * v; }
    }
    const float fac = div_rn(512.f, fmaxf(sqrt_rn(nrm2b), 1.1920928955078125e-7f));
    if (lane < 36 && cr >= 1 && cr <= 4 && cc >= 1 && cc <= 4) {
        float out[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) out[q] = fminf(fmaxf(rintf(fminf(h[q], thr) * fac), 0.f), 255.f);
        float4 *d = (float4 *)(desc + row * 128 + ((cr - 1) * 4 + (cc - 1)) * 8);
        d[0] = make_float4(out[0], out[1], out[2], out[3]);
        d[1] = make_float4(out[4], out[5], out[6], out[7]);
    }
}

__global__ void sift_clear_kernel(int B, int *__restrict__ ccount, int *__restrict__ kcount, int *__restrict__ status)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B) { ccount[i] = 0; kcount[i] = 0; status[i] = 0; }
}

// ---- host side ----
struct SiftLayout { int n_oct; int H[SIFT_MAX_OCT], W[SIFT_MAX_OCT]; size_t lvl[SIFT_MAX_OCT][SIFT_LEVELS]; size_t cand, kps, ccount, kcount, total; };

static size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

static int sift_layout(int B, int H, int W, int ccap, SiftLayout *L)
{
    if (ccap <= 0 || ccap > SIFT_CCAP || B <= 0 || H < 8 || W < 8 || H > 16384 || W > 16384) return MFR_E_ARG;
    const int H2 = 2 * H, W2 = 2 * W;
    int n = (int)lrint(log((double)(H2 < W2 ? H2 : W2)) / log(2.) - 2) + 1;     // cvRound(log2(min(base)) - 2) - firstOctave
    if (n > SIFT_MAX_OCT) n = SIFT_MAX_OCT;
    if (n < 1) n = 1;
    L->n_oct = n;
    size_t off = 0;
    int h = H2, w = W2;
    for (int o = 0; o < n; ++o) {
        if (h < 1 || w < 1) return MFR_E_ARG;
        L->H[o] = h; L->W[o] = w;
        for (int l = 0; l < SIFT_LEVELS; ++l) { L->lvl[o][l] = off; off = align256(off + (size_t)B * h * w * sizeof(float)); }
        h /= 2; w /= 2;
    }
    L->cand = off; off = align256(off + (size_t)B * ccap * sizeof(SiftCand));
    L->kps = off; off = align256(off + (size_t)B * SIFT_KCAP * sizeof(SiftKp));
    L->ccount = off; off = align256(off + (size_t)B * sizeof(int));
    L->kcount = off; off = align256(off + (size_t)B * sizeof(int));
    L->total = off;
    return 0;
}

// getGaussianKernel(ksize = cvRound(sigma * 8 + 1) | 1, sigma, CV_32F): binary64 taps normalised to sum 1, then rounded to f32
static SiftKernel sift_gauss(double sigma)
{
    SiftKernel k;
    const int n = ((int)lrint(sigma * 8 + 1)) | 1, R = n / 2;
    double cd[2 * SIFT_MAXR + 1], sum = 0.;
    const double scale2X = -0.5 / (sigma * sigma);
    for (int i = 0; i < n; ++i) { const double x = i - (n - 1) * 0.5; cd[i] = exp(scale2X * x * x); sum += cd[i]; }
    sum = 1. / sum;
    for (int i = 0; i <= SIFT_MAXR; ++i) k.c[i] = 0.f;
    for (int i = 0; i <= R; ++i) k.c[i] = (float)(cd[R + i] * sum);
    k.R = R;
    return k;
}

static double sift_level_sigma(int l)
{
    const double sigma = 1.6, k = pow(2., 1. / SIFT_LAYERS);
    if (l == 0) return sqrt(fmax(sigma * sigma - 1.0 * 1.0, 0.01));           // sig_diff of the doubled base: (2 * 0.5)^2
    const double prev = pow(k, (double)(l - 1)) * sigma, tot = prev * k;
    return sqrt(tot * tot - prev * prev);
}

extern "C" {

int mfr_sift_blur_taps(int level, float *taps_host, int *radius_host)
{
    if (level < 0 || level >= SIFT_LEVELS || !taps_host || !radius_host) return MFR_E_ARG;
    const SiftKernel k = sift_gauss(sift_level_sigma(level));
    for (int i = 0; i <= SIFT_MAXR; ++i) taps_host[i] = k.c[i];
    *radius_host = k.R;
    return 0;
}

size_t mfr_sift_workspace_bytes(int B, int H, int W, int cand_cap)
{
    SiftLayout L;
    return sift_layout(B, H, W, cand_cap > 0 ? cand_cap : SIFT_CCAP, &L) == 0 ? L.total : 0;
}

long long mfr_sift_level_offset(int B, int H, int W, int octave, int level, int *Ho_host, int *Wo_host)
{
    SiftLayout L;
    if (sift_layout(B, H, W, SIFT_CCAP, &L) != 0 || octave < 0 || level < 0 || level >= SIFT_LEVELS) return -1;
    if (octave >= L.n_oct) return -1;
    if (Ho_host) *Ho_host = L.H[octave];
    if (Wo_host) *Wo_host = L.W[octave];
    return (long long)L.lvl[octave][level];
}

int mfr_sift_detect(const uint8_t *gray, int B, int H, int W, int nfeatures, int Nmax, int cand_cap, void *workspace, size_t workspace_bytes,
                    float *kpts, float *desc, float *size, float *angle, float *response, int32_t *octave, int32_t *n,
                    int32_t *status, void *stream)
{
    SiftLayout L;
    if (!gray || !workspace || !kpts || !desc || !size || !angle || !response || !octave || !n || !status || Nmax <= 0 || nfeatures < 0)
        return MFR_E_ARG;
    const int ccap = cand_cap > 0 ? cand_cap : SIFT_CCAP;
    if (sift_layout(B, H, W, ccap, &L) != 0) return MFR_E_ARG;
    if (workspace_bytes < L.total) return MFR_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    auto lvl = [&](int o, int l) { return (float *)(ws + L.lvl[o][l]); };
    int *ccount = (int *)(ws + L.ccount), *kcount = (int *)(ws + L.kcount);
    SiftCand *cand = (SiftCand *)(ws + L.cand);
    SiftKp *kps = (SiftKp *)(ws + L.kps);
    hipLaunchKernelGGL(sift_clear_kernel, dim3((B + 255) / 256), dim3(256), 0, st, B, ccount, kcount, status);
    CHECK_LAUNCH();
    // Gaussian pyramid
    SiftKernel kl[SIFT_LEVELS];
    for (int l = 0; l < SIFT_LEVELS; ++l) kl[l] = sift_gauss(sift_level_sigma(l));
    for (int o = 0; o < L.n_oct; ++o) {
        const int h = L.H[o], w = L.W[o];
        const dim3 tiles((w + SIFT_TILE - 1) / SIFT_TILE, (h + SIFT_TILE - 1) / SIFT_TILE, B);
        if (o == 0) {
            hipLaunchKernelGGL(sift_base_kernel, dim3((w + 255) / 256, h, B), dim3(256), 0, st, gray, H, W, lvl(0, 1));
            CHECK_LAUNCH();
            hipLaunchKernelGGL(sift_blur_kernel, tiles, dim3(256), 0, st, (const float *)lvl(0, 1), lvl(0, 0), h, w, kl[0]);
        } else {
            hipLaunchKernelGGL(sift_down_kernel, dim3((w + 255) / 256, h, B), dim3(256), 0, st, (const float *)lvl(o - 1, SIFT_LAYERS),
                               L.H[o - 1], L.W[o - 1], lvl(o, 0), h, w);
        }
        CHECK_LAUNCH();
        for (int l = 1; l < SIFT_LEVELS; ++l) {
            hipLaunchKernelGGL(sift_blur_kernel, tiles, dim3(256), 0, st, (const float *)lvl(o, l - 1), lvl(o, l), h, w, kl[l]);
            CHECK_LAUNCH();
        }
    }
    // extrema + refinement, per octave
    for (int o = 0; o < L.n_oct; ++o) {
        SiftOctave O;
        for (int l = 0; l < SIFT_LEVELS; ++l) O.g[l] = lvl(o, l);
        O.H = L.H[o]; O.W = L.W[o]; O.o = o;
        if (O.H <= 2 * SIFT_BORDER || O.W <= 2 * SIFT_BORDER) continue;
        hipLaunchKernelGGL(sift_extrema_kernel, dim3((O.W + 15) / 16, (O.H + 15) / 16, B), dim3(256), 0, st, O, cand, ccap, ccount, status);
        CHECK_LAUNCH();
    }
    SiftPyr P;
    P.n_oct = L.n_oct;
    for (int o = 0; o < SIFT_MAX_OCT; ++o) {
        P.H[o] = o < L.n_oct ? L.H[o] : 0; P.W[o] = o < L.n_oct ? L.W[o] : 0;
        for (int l = 0; l < SIFT_LEVELS; ++l) P.g[o][l] = o < L.n_oct ? lvl(o, l) : nullptr;
    }
    hipLaunchKernelGGL(sift_orient_kernel, dim3(256, B), dim3(256), 0, st, P, (const SiftCand *)cand, ccap, (const int *)ccount, kps, kcount, status);
    CHECK_LAUNCH();
    hipLaunchKernelGGL(sift_select_kernel, dim3(B), dim3(1024), 0, st, (const SiftKp *)kps, (const int *)kcount, nfeatures, Nmax, kpts, size,
                       angle, response, octave, n, status);
    CHECK_LAUNCH();
    hipLaunchKernelGGL(sift_desc_kernel, dim3((Nmax + 3) / 4, B), dim3(256), 0, st, P, (const float *)kpts, (const float *)size,
                       (const float *)angle, (const int *)octave, (const int *)n, Nmax, desc);
    CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
