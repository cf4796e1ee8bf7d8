// lightglue.hip -- the parts of LightGlue (Lindenberger, Sarlin, Pollefeys, ICCV 2023; SuperPoint features, 9 layers, no adaptive depth / width)
// that the SuperGlue / LoFTR kernels do not already provide.  gfx950, fp32 throughout; built without FMA contraction (csrc/Makefile EXACT_SRCS:
// the precise log-sum-exp of wave_dev.h is only defined for such TUs, and the rotation then is the oracle's two products and one sum).
//
// What runs elsewhere: the q/k/v, MLP and final projections are split GEMMs (gemm_split.hip, both arithmetics, range guard included), the 4 x 64
// softmax attention is mfr_sg_attention as it is (scale 1/8, per-image token counts, cross = 1 for the flipped pair), the similarity matrix is the
// batched split GEMM.  Every kernel here consumes and produces fp32 rows, so none has an f16 range precondition of its own.
//
// Rotary encoding -- ONE choice, stated here: cos / sin are computed once per batch (lg_rotary_table_kernel: 32 angles theta = Wr p per keypoint,
// shared by the 4 heads and by all 9 layers) and applied per layer, in place, to the q and k columns of the self-attention's qkv rows
// (lg_rotary_apply_kernel).  The rotation is NOT fused into the q/k projection's epilogue: that epilogue belongs to the shared split-GEMM template,
// whose 14 instantiations change their register allocation with any code added there (gemm_split.hip, "tile geometry"), and the table costs
// 64 floats per keypoint.  x' = x cos + rot(x) sin with rot (x_2i, x_2i+1) -> (-x_2i+1, x_2i): the interleaved pairing, not Llama's half split.
//
// MLP block  y = x + fc2(GELU(LayerNorm_512(fc1([x | msg])))):  fc1 and fc2 are launches of the shared split GEMM (fc2 with its accumulating epilogue:
// the residual is in place).  The LayerNorm + GELU between them exist in two forms (nets/lightglue.py `mlp`): lg_ln_gelu_kernel here, a pass of its own
// over the hidden rows behind the default fc1 kernel, and fc1's epilogue (gemm_split.hip gemm_ln512_gelu_kernel: a workgroup keeps the four 128-feature
// accumulator blocks of its rows, the pre-norm hidden row is never written).  The pass is the default: measured, the epilogue kernel's one workgroup
// per CU costs more than the pass saves (profiles/lightglue_stage.json).  The one-launch form of the whole block is not built.
//
// Assignment  score_ij = (S_ij - lse_j S_i.) + (S_ij - lse_i S_.j) + logsigmoid(z0_i) + logsigmoid(z1_j)  over the valid n0 x n1 block, then mutual
// row / column arg-max, exp(score) > threshold.  The (N + 1)^2 log-assignment matrix is never written and S is swept TWICE (the shape of
// mfr_loftr_coarse_match): sweep 1 forms complete row log-sum-exps and per-strip column partials, sweep 2 the row arg-max and per-strip column
// arg-max partials; the partials are folded in a fixed order (no float atomics: bit-reproducible).  Ties go to the lowest index.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mfr_hip.h"
#include "wave_dev.h"

using namespace mfr;

// ---- rotary encoding ------------------------------------------------------------------------------------------------------------------------
// cs [M, 64]: cos(theta_i) at column i, sin(theta_i) at 32 + i; one thread per (keypoint, i)
__global__ void __launch_bounds__(256) lg_rotary_table_kernel(const float *__restrict__ kn, const float *__restrict__ wr, long long total, float *__restrict__ cs)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const long long tok = t >> 5;
    const int i = (int)(t & 31);
    const float th = kn[2 * tok] * wr[2 * i] + kn[2 * tok + 1] * wr[2 * i + 1];
    cs[tok * 64 + i] = cosf(th);
    cs[tok * 64 + 32 + i] = sinf(th);
}

// q, k [M, 256] (row stride ld floats, 8-byte aligned pairs): one thread per (row, q | k, head, pair)
__global__ void __launch_bounds__(256) lg_rotary_apply_kernel(float *__restrict__ q, float *__restrict__ k, int ld, long long total, const float *__restrict__ cs)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const long long tok = t >> 8;
    const int rem = (int)(t & 255), which = rem >> 7, h = (rem >> 5) & 3, i = rem & 31;
    float2 *p = (float2 *)((which ? k : q) + (size_t)tok * ld + 64 * h + 2 * i);
    const float c = cs[tok * 64 + i], s = cs[tok * 64 + 32 + i];
    const float2 x = *p;
    *p = make_float2(x.x * c - x.y * s, x.y * c + x.x * s);
}

// ---- LayerNorm_512 + exact GELU, in place: one wavefront per row, 8 values per lane ------------------------------------------------------------
// two-pass statistics (mean, then centred squares), biased variance, rsqrt(var + eps): the arithmetic of mfr_layernorm
__global__ void __launch_bounds__(256) lg_ln_gelu_kernel(float *__restrict__ x, int ld, int M, const float *__restrict__ gamma, const float *__restrict__ beta, float eps)
{
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    float *p = x + (size_t)row * ld;
    float v[8];
    float sum = 0.f;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const float4 t = *(const float4 *)(p + 256 * h + 4 * lane);
        v[4 * h] = t.x; v[4 * h + 1] = t.y; v[4 * h + 2] = t.z; v[4 * h + 3] = t.w;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) sum += v[e];
    const float mean = wave_sum(sum) * (1.0f / 512.0f);
    float sq = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) { v[e] -= mean; sq += v[e] * v[e]; }
    const float rstd = rsqrtf(wave_sum(sq) * (1.0f / 512.0f) + eps);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int c = 256 * h + 4 * lane;
        const float4 g = *(const float4 *)(gamma + c), b = *(const float4 *)(beta + c);
        const float gg[4] = { g.x, g.y, g.z, g.w }, bb[4] = { b.x, b.y, b.z, b.w };
        float y[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float u = v[4 * h + e] * rstd * gg[e] + bb[e];
            y[e] = 0.5f * u * (1.0f + erff(u * 0.70710678118654752440f));
        }
        *(float4 *)(p + c) = make_float4(y[0], y[1], y[2], y[3]);
    }
}

// ---- assignment -------------------------------------------------------------------------------------------------------------------------------
#define LG_STRIP 32          // rows of S per workgroup: 4 wavefronts x 8 rows, wavefront w takes rows w, w + 4, ...
#define LG_CHUNK 1024        // columns per pass of a strip: 16 per lane, kept in registers

MFR_DEV float lg_logsigmoid(float z) { return fminf(z, 0.f) - log1pf(expf(-fabsf(z))); }
MFR_DEV int lg_count(const int *n, int b, int cap) { return min(max(n[b], 0), cap); }

struct LgWs { float *rowmax, *rowterm, *colmax, *colterm, *val0, *part_a, *part_b; int32_t *idx0, *idx1, *part_i; size_t total; };
static LgWs lg_ws_layout(void *base, int B, int N0, int N1)
{
    WsCarver c(base);
    const size_t ns = (size_t)(N0 + LG_STRIP - 1) / LG_STRIP;
    LgWs w;
    // lse_j S_ij = rowmax_i + log(sum_j exp(S_ij - rowmax_i)) is kept as its two parts: S_ij - rowmax_i is exact for the entries that matter (Sterbenz),
    // while S_ij - lse would round at the magnitude of S (1e-4 at |S| ~ 2000) -- the module's log_softmax subtracts the maximum first, too
    w.rowmax = c.take<float>((size_t)B * N0);
    w.rowterm = c.take<float>((size_t)B * N0);            // logsigmoid(z0_i) - log(sum_j exp(S_ij - rowmax_i))
    w.colmax = c.take<float>((size_t)B * N1);
    w.colterm = c.take<float>((size_t)B * N1);            // logsigmoid(z1_j) - log(sum_i exp(S_ij - colmax_j))
    w.val0 = c.take<float>((size_t)B * N0);               // row maximum of the score
    w.idx0 = c.take<int32_t>((size_t)B * N0);             // its column
    w.idx1 = c.take<int32_t>((size_t)B * N1);             // row of the column maximum
    w.part_a = c.take<float>((size_t)B * ns * N1);        // per strip and column: lse maximum (sweep 1) / best score (sweep 2)
    w.part_b = c.take<float>((size_t)B * ns * N1);        // lse sum (sweep 1)
    w.part_i = c.take<int32_t>((size_t)B * ns * N1);      // best row (sweep 2)
    w.total = c.off;
    return w;
}

// One sweep over S for strip blockIdx.x of pair blockIdx.y.  ARGMAX = false: rowterm of the strip's rows, (max, sum) partial of every column over the
// strip's rows.  ARGMAX = true: idx0 / val0 of the strip's rows, (best, row) partial of every column.  Columns in chunks of 1024: a lane owns columns
// c0 + lane + 64 k, k < 16, reads are 256-byte row pieces.
template <bool ARGMAX>
__global__ void __launch_bounds__(256) lg_sweep_kernel(const float *__restrict__ S, int N0, int N1, int ldS, const float *__restrict__ z0,
                                                       const int *__restrict__ n0, const int *__restrict__ n1, LgWs w)
{
    __shared__ float sa[4][LG_CHUNK], sb[4][LG_CHUNK];     // the wavefronts' column partials of one chunk (sb: sum, or the row index as bits)
    __shared__ float ra[4][8], rb[4][8];                    // a wavefront's row state across chunks (only that wavefront touches it)
    const int b = blockIdx.y, strip = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int m = lg_count(n0, b, N0), n = lg_count(n1, b, N1);
    if (n == 0 || strip * LG_STRIP >= m) return;
    const int ns = (N0 + LG_STRIP - 1) / LG_STRIP;
    const float *Sb = S + (size_t)b * N0 * ldS;
    const size_t pbase = ((size_t)b * ns + strip) * N1;
    if (lane < 8) { ra[wid][lane] = -INFINITY; rb[wid][lane] = ARGMAX ? __int_as_float(0x7fffffff) : 0.f; }
    __syncthreads();                                        // the row state is in LDS before lane 0 reads it

    for (int c0 = 0; c0 < n; c0 += LG_CHUNK) {
        float ca[16], cb[16], ct[16], cm[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            ca[k] = -INFINITY; cb[k] = ARGMAX ? __int_as_float(0x7fffffff) : 0.f;
            const int j = c0 + lane + 64 * k;
            ct[k] = (ARGMAX && j < n) ? w.colterm[(size_t)b * N1 + j] : 0.f;
            cm[k] = (ARGMAX && j < n) ? w.colmax[(size_t)b * N1 + j] : 0.f;
        }
        for (int r = 0; r < 8; ++r) {
            const int i = strip * LG_STRIP + wid + 4 * r;       // wave-uniform
            if (i >= m) break;
            const float *row = Sb + (size_t)i * ldS;
            float x[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int j = c0 + lane + 64 * k;
                x[k] = j < n ? row[j] : -INFINITY;
            }
            if (!ARGMAX) {
                // row: the lane's 16 values as (max, sum), merged over the wavefront and into the row's state; column: online update
                float mx = -INFINITY;
#pragma unroll
                for (int k = 0; k < 16; ++k) mx = fmaxf(mx, x[k]);
                LsePrecise a = { mx, 0.f };
                if (mx > -INFINITY) {
#pragma unroll
                    for (int k = 0; k < 16; ++k) a.s += expf(x[k] - mx);          // (x = -inf: 0)
                }
                lse_precise_wave_merge(a);
                if (lane == 0) {
                    LsePrecise st = { ra[wid][r], rb[wid][r] };
                    lse_precise_merge(st, a.m, a.s);
                    ra[wid][r] = st.m; rb[wid][r] = st.s;
                }
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    if (x[k] > -INFINITY) { LsePrecise c = { ca[k], cb[k] }; lse_precise_add(c, x[k]); ca[k] = c.m; cb[k] = c.s; }
                }
            } else {
                const float rt = w.rowterm[(size_t)b * N0 + i], rm = w.rowmax[(size_t)b * N0 + i];
                float best = -INFINITY; int bj = 0x7fffffff;
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const int j = c0 + lane + 64 * k;
                    if (j < n) {
                        const float v = ((x[k] - rm) + rt) + ((x[k] - cm[k]) + ct[k]);
                        if (v > best) { best = v; bj = j; }                          // ascending j within the lane: the lowest index stays
                        if (v > ca[k]) { ca[k] = v; cb[k] = __int_as_float(i); }     // ascending i within the wavefront
                    }
                }
                wave_argmax(best, bj);
                if (lane == 0 && best > ra[wid][r]) { ra[wid][r] = best; rb[wid][r] = __int_as_float(bj); }    // chunks ascend: strict >
            }
        }
        // fold the four wavefronts' column partials (fixed order 0 .. 3) and store the strip's partial of this chunk
#pragma unroll
        for (int k = 0; k < 16; ++k) { sa[wid][lane + 64 * k] = ca[k]; sb[wid][lane + 64 * k] = cb[k]; }
        __syncthreads();
        for (int c = tid; c < LG_CHUNK && c0 + c < n; c += 256) {
            if (!ARGMAX) {
                LsePrecise a = { sa[0][c], sb[0][c] };
                for (int g = 1; g < 4; ++g) lse_precise_merge(a, sa[g][c], sb[g][c]);
                w.part_a[pbase + c0 + c] = a.m; w.part_b[pbase + c0 + c] = a.s;
            } else {
                float best = sa[0][c]; int bi = __float_as_int(sb[0][c]);
                for (int g = 1; g < 4; ++g) {
                    const float ob = sa[g][c]; const int oi = __float_as_int(sb[g][c]);
                    if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
                }
                w.part_a[pbase + c0 + c] = best; w.part_i[pbase + c0 + c] = bi;
            }
        }
        __syncthreads();
    }
    if (lane < 8) {
        const int i = strip * LG_STRIP + wid + 4 * lane;
        if (i < m) {
            if (!ARGMAX) { w.rowmax[(size_t)b * N0 + i] = ra[wid][lane]; w.rowterm[(size_t)b * N0 + i] = lg_logsigmoid(z0[(size_t)b * N0 + i]) - logf(rb[wid][lane]); }
            else { w.val0[(size_t)b * N0 + i] = ra[wid][lane]; w.idx0[(size_t)b * N0 + i] = __float_as_int(rb[wid][lane]); }
        }
    }
}

// colmax_j, colterm_j from the strips' (max, sum) partials (folded in ascending strip order)
__global__ void __launch_bounds__(256) lg_colterm_kernel(int N0, int N1, const float *__restrict__ z1, const int *__restrict__ n0, const int *__restrict__ n1, LgWs w)
{
    const int b = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    const int m = lg_count(n0, b, N0), n = lg_count(n1, b, N1);
    if (j >= n || m == 0) return;
    const int ns = (N0 + LG_STRIP - 1) / LG_STRIP, used = (m + LG_STRIP - 1) / LG_STRIP;
    LsePrecise a = { -INFINITY, 0.f };
    for (int s = 0; s < used; ++s) {
        const size_t o = ((size_t)b * ns + s) * N1 + j;
        lse_precise_merge(a, w.part_a[o], w.part_b[o]);
    }
    w.colmax[(size_t)b * N1 + j] = a.m;
    w.colterm[(size_t)b * N1 + j] = lg_logsigmoid(z1[(size_t)b * N1 + j]) - logf(a.s);
}

// one workgroup per pair: column arg-max over the strips' partials, mutual check + threshold, ordered compaction of the matched keypoints
// (ascending i, as mfr_sg_sinkhorn_match); kpts0 == NULL: no pts0 / pts1 / n_corr
__global__ void __launch_bounds__(256) lg_match_kernel(int N0, int N1, const int *__restrict__ n0, const int *__restrict__ n1, float thr, LgWs w,
                                                       const float *__restrict__ kpts0, const float *__restrict__ kpts1, int K,
                                                       int *matches0, int *__restrict__ matches1, float *ms0, float *__restrict__ ms1,
                                                       float *__restrict__ pts0, float *__restrict__ pts1, int maxN, int *__restrict__ n_corr)
{
    __shared__ Compact256 cs;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int m = lg_count(n0, b, N0), n = lg_count(n1, b, N1);
    const bool any = m > 0 && n > 0;
    const int ns = (N0 + LG_STRIP - 1) / LG_STRIP, used = (m + LG_STRIP - 1) / LG_STRIP;
    int *idx1 = w.idx1 + (size_t)b * N1;
    const int *idx0 = w.idx0 + (size_t)b * N0;
    if (any)
        for (int j = tid; j < n; j += 256) {
            float best = -INFINITY; int bi = 0x7fffffff;
            for (int s = 0; s < used; ++s) {                   // ascending strips hold ascending rows: strict > keeps the lowest
                const size_t o = ((size_t)b * ns + s) * N1 + j;
                const float ob = w.part_a[o];
                if (ob > best) { best = ob; bi = w.part_i[o]; }
            }
            idx1[j] = bi;
        }
    __syncthreads();
    int total = 0;
    for (int start = 0; start < N0; start += 256) {
        const int i = start + tid;
        bool valid = false;
        int j = -1;
        float sc = 0.f;
        if (any && i < m) {
            j = idx0[i];
            const bool mutual = j >= 0 && j < n && idx1[j] == i;      // (a row of NaN scores has no arg-max: its index is out of range)
            sc = mutual ? expf(w.val0[(size_t)b * N0 + i]) : 0.f;
            valid = mutual && sc > thr;
        }
        if (i < N0) {
            matches0[(size_t)b * N0 + i] = valid ? j : -1;
            ms0[(size_t)b * N0 + i] = sc;
        }
        const int o = compact256_slot(cs, valid, total);
        if (valid && kpts0 && o < maxN) {
            pts0[((size_t)b * maxN + o) * 2] = kpts0[((size_t)b * K + i) * 2];
            pts0[((size_t)b * maxN + o) * 2 + 1] = kpts0[((size_t)b * K + i) * 2 + 1];
            pts1[((size_t)b * maxN + o) * 2] = kpts1[((size_t)b * K + j) * 2];
            pts1[((size_t)b * maxN + o) * 2 + 1] = kpts1[((size_t)b * K + j) * 2 + 1];
        }
    }
    if (tid == 0 && n_corr) n_corr[b] = min(total, maxN);
    __syncthreads();                                           // matches0 / ms0 of this pair are complete
    for (int j = tid; j < N1; j += 256) {
        int mi = -1;
        float sc = 0.f;
        if (any && j < n) {
            const int i = idx1[j];
            if (i >= 0 && i < m && idx0[i] == j) {
                sc = ms0[(size_t)b * N0 + i];
                if (matches0[(size_t)b * N0 + i] == j) mi = i;
            }
        }
        matches1[(size_t)b * N1 + j] = mi;
        ms1[(size_t)b * N1 + j] = sc;
    }
}

extern "C" {

int mfr_lg_rotary_table(const float *kpts_norm, const float *wr, int M, float *cs, void *stream)
{
    if (!kpts_norm || !wr || !cs || M <= 0) return MFR_E_ARG;
    const long long total = (long long)M * 32;
    hipLaunchKernelGGL(lg_rotary_table_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, kpts_norm, wr, total, cs);
    CHECK_LAUNCH();
    return 0;
}

int mfr_lg_rotary_apply(float *q, float *k, int ld, int M, const float *cs, void *stream)
{
    if (!q || !k || !cs || M <= 0 || ld < 256 || (ld & 1) || (((uintptr_t)q | (uintptr_t)k) & 7)) return MFR_E_ARG;
    const long long total = (long long)M * 256;
    hipLaunchKernelGGL(lg_rotary_apply_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, q, k, ld, total, cs);
    CHECK_LAUNCH();
    return 0;
}

int mfr_lg_ln_gelu(float *x, int ld, int M, const float *gamma, const float *beta, float eps, void *stream)
{
    if (!x || !gamma || !beta || M <= 0 || ld < 512 || (ld & 3) || !(eps >= 0.f) ||
        (((uintptr_t)x | (uintptr_t)gamma | (uintptr_t)beta) & 15)) return MFR_E_ARG;
    hipLaunchKernelGGL(lg_ln_gelu_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, ld, M, gamma, beta, eps);
    CHECK_LAUNCH();
    return 0;
}

size_t mfr_lg_assign_workspace_bytes(int B, int N0, int N1)
{
    if (B <= 0 || N0 <= 0 || N1 <= 0) return 0;
    return lg_ws_layout(nullptr, B, N0, N1).total;
}

int mfr_lg_assign(const float *S, int B, int N0, int N1, int ldS, const float *z0, const float *z1, const int32_t *n0, const int32_t *n1,
                  float threshold, const float *kpts0, const float *kpts1, int K, void *workspace, size_t workspace_bytes,
                  int32_t *matches0, int32_t *matches1, float *mscores0, float *mscores1, float *pts0, float *pts1, int maxN, int32_t *n_corr,
                  void *stream)
{
    if (!S || !z0 || !z1 || !n0 || !n1 || !workspace || !matches0 || !matches1 || !mscores0 || !mscores1 ||
        B <= 0 || B > 65535 || N0 <= 0 || N1 <= 0 || ldS < N1 || !(threshold >= 0.f)) return MFR_E_ARG;
    const bool want_pts = kpts0 || kpts1 || pts0 || pts1 || n_corr;
    if (want_pts && (!kpts0 || !kpts1 || !pts0 || !pts1 || !n_corr || maxN <= 0 || K < N0 || K < N1)) return MFR_E_ARG;
    const LgWs w = lg_ws_layout(workspace, B, N0, N1);
    if (workspace_bytes < w.total) return MFR_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const dim3 sgrid((N0 + LG_STRIP - 1) / LG_STRIP, B);
    hipLaunchKernelGGL(lg_sweep_kernel<false>, sgrid, dim3(256), 0, s, S, N0, N1, ldS, z0, n0, n1, w);
    hipLaunchKernelGGL(lg_colterm_kernel, dim3((N1 + 255) / 256, B), dim3(256), 0, s, N0, N1, z1, n0, n1, w);
    hipLaunchKernelGGL(lg_sweep_kernel<true>, sgrid, dim3(256), 0, s, S, N0, N1, ldS, z0, n0, n1, w);
    hipLaunchKernelGGL(lg_match_kernel, dim3(B), dim3(256), 0, s, N0, N1, n0, n1, threshold, w, kpts0, kpts1, K, matches0, matches1, mscores0, mscores1,
                       pts0, pts1, want_pts ? maxN : 1, n_corr);
    CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
