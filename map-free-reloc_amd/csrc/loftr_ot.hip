// loftr_ot.hip -- LoFTR coarse matching by optimal transport (Sinkhorn with a dustbin) on gfx950.
//
// Reference call site: LoFTR_matcher (etc/feature_matching_baselines/matchers.py:12-59) loads `*_ot.ckpt`; upstream
// zju3dv/LoFTR CoarseMatching with MATCH_TYPE 'sinkhorn' (un-vendored submodule; arithmetic per SURVEY.md Appendix A.4 and
// SuperGlue's log_optimal_transport):
//
//   Z0 = [[S, a], [a, a]]  (a = bin_score),  norm = -log(m + n),  log_mu = [norm]*m ++ [log n + norm],  log_nu likewise
//   u = v = 0;  iters times:  u = log_mu - logsumexp_j(Z0 + v);  v = log_nu - logsumexp_i(Z0 + u)
//   conf = exp(Z0 + u + v - norm)[:m, :n];  conf > thr, border removal, mutual max  ->  (i, j, conf)
//
// S [B, L0, L1] is read-only and only streamed; the dustbin row / column are the constant a and are never materialised: a row's
// logsumexp gets the one extra term a + v_bin, a column's a + u_bin, and the two dustbin potentials are logsumexps over the u / v
// VECTORS (ot_bin_kernel).  conf exists only as z = (S + u_i) + v_j in the registers of the final sweep: exp is monotonic, so the
// maxima and the mutual test are taken on z and one exp per ROW maximum gives the confidence the threshold looks at.
//
// variant 0 (default): iters + 1 sweeps over S.  A workgroup owns a stripe of rows and ALL columns (a thread holds 4 adjacent
//   columns of each 1024-column block: up to OT_NQMAX blocks = 8192 columns in registers).  Per row: the wavefronts' (max, sum)
//   through LDS give the complete row logsumexp, hence u_i; with the row still in registers S_ij + u_i goes into the thread's
//   per-column online (max, sum).  One partial per (stripe, column); ot_colfold_kernel folds them over the stripes in ascending
//   order (no float atomics: bit-reproducible).  The final sweep has the same shape (row arg-max complete, column maxima folded).
// variant 1 (A/B baseline, cross-check, and what runs for L1 > 8192): a row kernel (one wavefront per row) and a column kernel
//   per iteration, 2 iters + 1 sweeps, precise expf / logf.
//
// Compiled with -ffp-contract=off: z is compared for equality between the row and the column side of the mutual test.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mfr_hip.h"
#include "wave_dev.h"

using namespace mfr;

#define OT_CB 1024          // columns per register block (256 threads x 4)
#define OT_NQMAX 8          // register blocks: variant 0 holds rows of up to 8192 columns
#define OT_RU 2             // rows in flight
#define OT_RSMAX 64         // rows per stripe: 64, 32 or 16 (ot_stripe_rows)

// ---- variant 0: one sweep per iteration -----------------------------------------------------------------------------------
// grid (stripes, B), 256 threads.  v == NULL: the zero potentials of the first iteration (then ubin0 is stored as u_bin).
template <int NQ>
__global__ void __launch_bounds__(256) ot_sweep_kernel(const float *__restrict__ S, int L0, int L1, int rs, const float *__restrict__ v,
                                                       float a, float norm, float ubin0, float *__restrict__ u,
                                                       float *__restrict__ cpm, float *__restrict__ cps)
{
    __shared__ float wm[2][OT_RU][4], wsum[2][OT_RU][4];
    const int st = blockIdx.x, b = blockIdx.y, nst = gridDim.x;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int i0 = st * rs, nrows = min(rs, L0 - i0);
    // 16-byte loads need the row length AND this pair's first row on a 16-byte boundary (the caller's S is only float-aligned by contract)
    const bool vec = (L1 & 3) == 0 && (((uintptr_t)S) & 15) == 0;
    const float *base = S + ((size_t)b * L0 + i0) * L1;
    const float *vb = v ? v + (size_t)b * (L1 + 1) : nullptr;
    int nval[NQ];
    float vv[NQ][4];
    LsePrecise c[NQ][4];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int j0 = q * OT_CB + 4 * tid;
        nval[q] = min(4, max(0, L1 - j0));
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            vv[q][k] = (vb && k < nval[q]) ? vb[j0 + k] : 0.f;
            c[q][k] = { -INFINITY, 0.f };
        }
    }
    const float binterm = a + (vb ? vb[L1] : 0.f);
    if (!v && st == 0 && tid == 0) u[(size_t)b * (L0 + 1) + L0] = ubin0;
    int par = 0;
    for (int r0 = 0; r0 < nrows; r0 += OT_RU, par ^= 1) {
        float x[OT_RU][NQ][4];
#pragma unroll
        for (int r = 0; r < OT_RU; ++r)
#pragma unroll
            for (int q = 0; q < NQ; ++q)
                if (r0 + r < nrows) load4(base + (size_t)(r0 + r) * L1, q * OT_CB + 4 * tid, nval[q], vec, 0.f, x[r][q]);
        // rows: the wavefront's maximum first, one v_exp_f32 per term (an absent column / row is -inf and contributes exp(-inf) = 0)
#pragma unroll
        for (int r = 0; r < OT_RU; ++r) {
            float lm = -INFINITY;
#pragma unroll
            for (int q = 0; q < NQ; ++q)
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (r0 + r < nrows && k < nval[q]) lm = fmaxf(lm, x[r][q][k] + vv[q][k]);
            const float mx = wave_max_dpp(lm);
            const float ms = (mx > -INFINITY) ? mx : 0.f;
            float ls = 0.f;
#pragma unroll
            for (int q = 0; q < NQ; ++q)
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (r0 + r < nrows && k < nval[q]) ls += __expf((x[r][q][k] + vv[q][k]) - ms);
            const float sm = wave_sum_dpp(ls);
            if (lane == 0) { wm[par][r][wid] = mx; wsum[par][r][wid] = sm; }
        }
        __syncthreads();          // (buffers alternate: the next group's writes cannot overtake this group's reads)
        float ui[OT_RU];
#pragma unroll
        for (int r = 0; r < OT_RU; ++r) {
            // the four wavefronts in column order, then the dustbin column's term: every thread evaluates the same expression
            float M = binterm;
#pragma unroll
            for (int w = 0; w < 4; ++w) M = fmaxf(M, wm[par][r][w]);
            float s = 0.f;
#pragma unroll
            for (int w = 0; w < 4; ++w) s += wsum[par][r][w] * __expf(wm[par][r][w] - M);
            s += __expf(binterm - M);
            ui[r] = norm - (M + logf(s));
            if (tid == 0 && r0 + r < nrows) u[(size_t)b * (L0 + 1) + i0 + r0 + r] = ui[r];
        }
        // columns: the rows in flight at once (row r0 exists; an absent row is -inf)
#pragma unroll
        for (int q = 0; q < NQ; ++q)
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < nval[q]) {
                    const float t0 = x[0][q][k] + ui[0];
                    const float t1 = (r0 + 1 < nrows) ? x[1][q][k] + ui[1] : -INFINITY;
                    const float bm = fmaxf(t0, t1);
                    const float bs = __expf(t0 - bm) + __expf(t1 - bm);
                    const float nm = fmaxf(c[q][k].m, bm);
                    c[q][k].s = c[q][k].s * __expf(c[q][k].m - nm) + bs * __expf(bm - nm);
                    c[q][k].m = nm;
                }
    }
    float *pm = cpm + ((size_t)b * nst + st) * L1, *ps = cps + ((size_t)b * nst + st) * L1;
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < nval[q]) { pm[q * OT_CB + 4 * tid + k] = c[q][k].m; ps[q * OT_CB + 4 * tid + k] = c[q][k].s; }
}

// v_j = log_nu - logsumexp_i(S_ij + u_i, a + u_bin): the stripes' partials in ascending order, then the dustbin row's term
__global__ void __launch_bounds__(256) ot_colfold_kernel(int L0, int L1, int nst, const float *__restrict__ cpm, const float *__restrict__ cps,
                                                         const float *__restrict__ u, float a, float norm, float *__restrict__ v)
{
    const int b = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= L1) return;
    LsePrecise acc = { -INFINITY, 0.f };
    for (int k = 0; k < nst; ++k) lse_precise_merge(acc, cpm[((size_t)b * nst + k) * L1 + j], cps[((size_t)b * nst + k) * L1 + j]);
    lse_precise_merge(acc, a + u[(size_t)b * (L0 + 1) + L0], 1.f);
    v[(size_t)b * (L1 + 1) + j] = norm - (acc.m + logf(acc.s));
}

// logsumexp of x[0 .. n) by one workgroup of 256 threads, fixed order; every thread returns the value
static __device__ float ot_block_lse(const float *x, int n, float *red)
{
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    float m = -INFINITY;
    for (int i = tid; i < n; i += 256) m = fmaxf(m, x[i]);
    m = wave_max(m);
    __syncthreads();
    if (lane == 0) red[wid] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float s = 0.f;
    for (int i = tid; i < n; i += 256) s += expf(x[i] - m);
    s = wave_sum(s);
    __syncthreads();
    if (lane == 0) red[wid] = s;
    __syncthreads();
    s = ((red[0] + red[1]) + red[2]) + red[3];
    return m + logf(s);
}

// the dustbin potentials, one workgroup per pair: v_bin from the u vector; then (unless this was the last iteration) the NEXT
// iteration's u_bin from the completed v vector.  Row / column L of the augmented matrix is the constant a.
__global__ void __launch_bounds__(256) ot_bin_kernel(int L0, int L1, float a, float lmu_bin, float lnu_bin, int last,
                                                     float *u, float *v)
{
    __shared__ float red[4];
    const int b = blockIdx.x;
    float *ub = u + (size_t)b * (L0 + 1), *vb = v + (size_t)b * (L1 + 1);
    const float lu = ot_block_lse(ub, L0 + 1, red);
    if (threadIdx.x == 0) vb[L1] = lnu_bin - (a + lu);
    if (last) return;
    __threadfence_block();
    __syncthreads();
    const float lv = ot_block_lse(vb, L1 + 1, red);
    if (threadIdx.x == 0) ub[L0] = lmu_bin - (a + lv);
}

// final sweep: z = (S_ij + u_i) + v_j; complete row maximum / arg-max (lowest j on a tie), column maxima per stripe
template <int NQ>
__global__ void __launch_bounds__(256) ot_best_kernel(const float *__restrict__ S, int L0, int L1, int rs, const float *__restrict__ u,
                                                      const float *__restrict__ v, float *__restrict__ rbest, int *__restrict__ rarg,
                                                      float *__restrict__ cbp)
{
    __shared__ float wb[OT_RSMAX][4];
    __shared__ int wj[OT_RSMAX][4];
    const int st = blockIdx.x, b = blockIdx.y, nst = gridDim.x;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int i0 = st * rs, nrows = min(rs, L0 - i0);
    const bool vec = (L1 & 3) == 0 && (((uintptr_t)S) & 15) == 0;
    const float *base = S + ((size_t)b * L0 + i0) * L1;
    const float *ub = u + (size_t)b * (L0 + 1) + i0, *vb = v + (size_t)b * (L1 + 1);
    int nval[NQ];
    float vv[NQ][4], cb[NQ][4];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int j0 = q * OT_CB + 4 * tid;
        nval[q] = min(4, max(0, L1 - j0));
#pragma unroll
        for (int k = 0; k < 4; ++k) { vv[q][k] = k < nval[q] ? vb[j0 + k] : 0.f; cb[q][k] = -INFINITY; }
    }
    for (int r0 = 0; r0 < nrows; r0 += OT_RU) {
        float x[OT_RU][NQ][4];
#pragma unroll
        for (int r = 0; r < OT_RU; ++r)
#pragma unroll
            for (int q = 0; q < NQ; ++q)
                if (r0 + r < nrows) load4(base + (size_t)(r0 + r) * L1, q * OT_CB + 4 * tid, nval[q], vec, 0.f, x[r][q]);
        float best[OT_RU]; int bj[OT_RU];
#pragma unroll
        for (int r = 0; r < OT_RU; ++r) {
            best[r] = -INFINITY; bj[r] = 0x7fffffff;
            if (r0 + r < nrows) {
                const float ui = ub[r0 + r];
#pragma unroll
                for (int q = 0; q < NQ; ++q)
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (k < nval[q]) {
                            const float z = (x[r][q][k] + ui) + vv[q][k];
                            if (z > best[r]) { best[r] = z; bj[r] = q * OT_CB + 4 * tid + k; }
                            if (z > cb[q][k]) cb[q][k] = z;
                        }
            }
        }
        // (wave_argmax of the rows in flight, interleaved by hand as in loftr.hip's dsm_best_tile_kernel)
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
            for (int r = 0; r < OT_RU; ++r) {
                const float ob = __shfl_xor(best[r], off, 64); const int oj = __shfl_xor(bj[r], off, 64);
                if (ob > best[r] || (ob == best[r] && oj < bj[r])) { best[r] = ob; bj[r] = oj; }
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int r = 0; r < OT_RU; ++r)
                if (r0 + r < nrows) { wb[r0 + r][wid] = best[r]; wj[r0 + r][wid] = bj[r]; }
        }
    }
    __syncthreads();
    if (tid < nrows) {
        float best = wb[tid][0]; int bj = wj[tid][0];
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (wb[tid][w] > best || (wb[tid][w] == best && wj[tid][w] < bj)) { best = wb[tid][w]; bj = wj[tid][w]; }
        rbest[(size_t)b * L0 + i0 + tid] = best; rarg[(size_t)b * L0 + i0 + tid] = bj;
    }
    float *pc = cbp + ((size_t)b * nst + st) * L1;
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < nval[q]) pc[q * OT_CB + 4 * tid + k] = cb[q][k];
}

__global__ void __launch_bounds__(256) ot_bestfold_kernel(int L1, int nst, const float *__restrict__ cbp, float *__restrict__ cbest)
{
    const int b = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= L1) return;
    float best = -INFINITY;
    for (int k = 0; k < nst; ++k) best = fmaxf(best, cbp[((size_t)b * nst + k) * L1 + j]);
    cbest[(size_t)b * L1 + j] = best;
}

// ---- variant 1: the plain form, a row kernel and a column kernel per iteration ---------------------------------------------
__global__ void __launch_bounds__(256) ot_row_kernel(const float *__restrict__ S, int L0, int L1, const float *__restrict__ v, float a,
                                                     float norm, float ubin0, float *__restrict__ u)
{
    const int b = blockIdx.y, lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (!v && blockIdx.x == 0 && threadIdx.x == 0) u[(size_t)b * (L0 + 1) + L0] = ubin0;
    if (i >= L0) return;
    const float *row = S + ((size_t)b * L0 + i) * L1;
    const float *vb = v ? v + (size_t)b * (L1 + 1) : nullptr;
    LsePrecise acc = { -INFINITY, 0.f };
    for (int j = lane; j < L1; j += 64) lse_precise_add(acc, row[j] + (vb ? vb[j] : 0.f));
    lse_precise_wave_merge(acc);
    if (lane == 0) {
        lse_precise_merge(acc, a + (vb ? vb[L1] : 0.f), 1.f);
        u[(size_t)b * (L0 + 1) + i] = norm - (acc.m + logf(acc.s));
    }
}

__global__ void __launch_bounds__(1024) ot_col_kernel(const float *__restrict__ S, int L0, int L1, const float *__restrict__ u, float a,
                                                      float norm, float *__restrict__ v)
{
    __shared__ float sm[16][64], ss[16][64];
    const int b = blockIdx.y, lane = threadIdx.x & 63, g = threadIdx.x >> 6, j = blockIdx.x * 64 + lane;
    const float *ub = u + (size_t)b * (L0 + 1);
    LsePrecise acc = { -INFINITY, 0.f };
    if (j < L1) {
        const float *colp = S + (size_t)b * L0 * L1 + j;
        for (int i = g; i < L0; i += 16) lse_precise_add(acc, colp[(size_t)i * L1] + ub[i]);
    }
    sm[g][lane] = acc.m; ss[g][lane] = acc.s;
    __syncthreads();
    if (g == 0 && j < L1) {
        for (int k = 1; k < 16; ++k) lse_precise_merge(acc, sm[k][lane], ss[k][lane]);
        lse_precise_merge(acc, a + ub[L0], 1.f);
        v[(size_t)b * (L1 + 1) + j] = norm - (acc.m + logf(acc.s));
    }
}

__global__ void __launch_bounds__(256) ot_rowbest_kernel(const float *__restrict__ S, int L0, int L1, const float *__restrict__ u,
                                                         const float *__restrict__ v, float *__restrict__ rbest, int *__restrict__ rarg)
{
    const int b = blockIdx.y, lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= L0) return;
    const float *row = S + ((size_t)b * L0 + i) * L1;
    const float *vb = v + (size_t)b * (L1 + 1);
    const float ui = u[(size_t)b * (L0 + 1) + i];
    float best = -INFINITY; int bj = 0x7fffffff;
    for (int j = lane; j < L1; j += 64) {
        const float z = (row[j] + ui) + vb[j];
        if (z > best) { best = z; bj = j; }
    }
    wave_argmax(best, bj);
    if (lane == 0) { rbest[(size_t)b * L0 + i] = best; rarg[(size_t)b * L0 + i] = bj; }
}

__global__ void __launch_bounds__(1024) ot_colbest_kernel(const float *__restrict__ S, int L0, int L1, const float *__restrict__ u,
                                                          const float *__restrict__ v, float *__restrict__ cbest)
{
    __shared__ float sb[16][64];
    const int b = blockIdx.y, lane = threadIdx.x & 63, g = threadIdx.x >> 6, j = blockIdx.x * 64 + lane;
    const float *ub = u + (size_t)b * (L0 + 1);
    float best = -INFINITY;
    if (j < L1) {
        const float *colp = S + (size_t)b * L0 * L1 + j;
        const float vj = v[(size_t)b * (L1 + 1) + j];
        for (int i = g; i < L0; i += 16) best = fmaxf(best, (colp[(size_t)i * L1] + ub[i]) + vj);
    }
    sb[g][lane] = best;
    __syncthreads();
    if (g == 0 && j < L1) {
        for (int k = 1; k < 16; ++k) best = fmaxf(best, sb[k][lane]);
        cbest[(size_t)b * L1 + j] = best;
    }
}

// ---- both variants: threshold, border, mutual maximum, ordered compaction (upstream get_coarse_match), one workgroup per pair ----
// rbest / cbest hold z = log(conf) + norm; conf = exp(z - norm) is formed once per row
__global__ void __launch_bounds__(256) ot_match_kernel(int L0, int L1, int h0, int w0, int h1, int w1, float thr, int border, float norm,
                                                       const float *__restrict__ rbest, const int *__restrict__ rarg,
                                                       const float *__restrict__ cbest, int *__restrict__ i_ids,
                                                       int *__restrict__ j_ids, float *__restrict__ mconf, int *__restrict__ n_match)
{
    __shared__ Compact256 cs;
    const int b = blockIdx.x, tid = threadIdx.x;
    int total = 0;
    for (int start = 0; start < L0; start += 256) {
        const int i = start + tid;
        bool valid = false; int j = 0; float c = 0.f;
        if (i < L0) {
            const float z = rbest[(size_t)b * L0 + i];
            j = rarg[(size_t)b * L0 + i];
            if (j >= 0 && j < L1) {                       // (a row of NaNs has no arg-max)
                c = expf(z - norm);
                const int y0 = i / w0, x0 = i - y0 * w0, y1 = j / w1, x1 = j - y1 * w1;
                const bool inb = y0 >= border && y0 < h0 - border && x0 >= border && x0 < w0 - border &&
                                 y1 >= border && y1 < h1 - border && x1 >= border && x1 < w1 - border;
                valid = (c > thr) && inb && (z == cbest[(size_t)b * L1 + j]);
            }
        }
        const int o = compact256_slot(cs, valid, total);
        if (valid) {
            i_ids[(size_t)b * L0 + o] = i; j_ids[(size_t)b * L0 + o] = j; mconf[(size_t)b * L0 + o] = c;
        }
    }
    if (tid == 0) n_match[b] = total;
}

// rows per stripe of variant 0: 64 when that already gives every CU two workgroups, else 32 / 16 (a pure function of the shape: the fold order,
// hence the result's bits, depends on B and L0 only)
static inline int ot_stripe_rows(int B, int L0)
{
    for (int rs = OT_RSMAX; rs > 16; rs >>= 1)
        if ((size_t)B * ((L0 + rs - 1) / rs) >= 512) return rs;
    return 16;
}

#define OT_LAUNCH_NQ(KERNEL, NQv, ...)                                                                                       \
    switch (NQv) {                                                                                                            \
    case 1: hipLaunchKernelGGL(KERNEL<1>, __VA_ARGS__); break;                                                                \
    case 2: hipLaunchKernelGGL(KERNEL<2>, __VA_ARGS__); break;                                                                \
    case 3: hipLaunchKernelGGL(KERNEL<3>, __VA_ARGS__); break;                                                                \
    case 4: hipLaunchKernelGGL(KERNEL<4>, __VA_ARGS__); break;                                                                \
    case 5: hipLaunchKernelGGL(KERNEL<5>, __VA_ARGS__); break;                                                                \
    case 6: hipLaunchKernelGGL(KERNEL<6>, __VA_ARGS__); break;                                                                \
    case 7: hipLaunchKernelGGL(KERNEL<7>, __VA_ARGS__); break;                                                                \
    default: hipLaunchKernelGGL(KERNEL<8>, __VA_ARGS__); break;                                                               \
    }

extern "C" {

size_t mfr_loftr_ot_match_workspace_bytes(int B, int L0, int L1)
{
    if (B <= 0 || L0 <= 0 || L1 <= 0) return 0;
    const int rs = ot_stripe_rows(B, L0);
    const size_t nst = (size_t)(L0 + rs - 1) / rs;
    return align_up((size_t)B * (L0 + 1) * 4, 256) + align_up((size_t)B * (L1 + 1) * 4, 256) + 2 * align_up((size_t)B * L0 * 4, 256) +
           align_up((size_t)B * L1 * 4, 256) + 2 * align_up((size_t)B * nst * L1 * 4, 256);
}

int mfr_loftr_ot_match(const float *S, int B, int h0, int w0, int h1, int w1, float bin_score, int iters, float thr, int border,
                       void *workspace, size_t workspace_bytes, int32_t *i_ids, int32_t *j_ids, float *mconf, int32_t *n_match,
                       float *u_out, float *v_out, int variant, void *stream)
{
    if (!S || !workspace || !i_ids || !j_ids || !mconf || !n_match || B <= 0 || B > 65535 || h0 <= 0 || w0 <= 0 || h1 <= 0 || w1 <= 0 ||
        iters < 1 || border < 0 || (variant != 0 && variant != 1) || !(bin_score == bin_score) || !(thr == thr))
        return MFR_E_ARG;
    if ((long long)h0 * w0 > 0x7fffff00ll || (long long)h1 * w1 > 0x7fffff00ll) return MFR_E_ARG;
    const int L0 = h0 * w0, L1 = h1 * w1;
    if (workspace_bytes < mfr_loftr_ot_match_workspace_bytes(B, L0, L1)) return MFR_E_WORKSPACE;
    const int rs = ot_stripe_rows(B, L0), nst = (L0 + rs - 1) / rs;
    char *ws = (char *)workspace;
    const size_t au = align_up((size_t)B * (L0 + 1) * 4, 256), av = align_up((size_t)B * (L1 + 1) * 4, 256);
    const size_t a0 = align_up((size_t)B * L0 * 4, 256), a1 = align_up((size_t)B * L1 * 4, 256);
    const size_t ap = align_up((size_t)B * nst * L1 * 4, 256);
    float *u = u_out ? u_out : (float *)ws, *v = v_out ? v_out : (float *)(ws + au);
    float *rbest = (float *)(ws + au + av);
    int *rarg = (int *)(ws + au + av + a0);
    float *cbest = (float *)(ws + au + av + 2 * a0);
    float *cpm = (float *)(ws + au + av + 2 * a0 + a1), *cps = (float *)(ws + au + av + 2 * a0 + a1 + ap);
    hipStream_t s = (hipStream_t)stream;
    // the marginals in fp32, as the reference forms them: norm = -log(m + n), the dustbins' log n + norm / log m + norm
    const float norm = -logf((float)L0 + (float)L1);
    const float lmu_bin = logf((float)L1) + norm, lnu_bin = logf((float)L0) + norm;
    const float a = bin_score;
    // first iteration, v = 0: u_bin = log_mu_bin - logsumexp of n + 1 terms a
    const float ubin0 = lmu_bin - (a + logf((float)L1 + 1.0f));
    const int nq = (L1 + OT_CB - 1) / OT_CB;
    const bool tiled = variant == 0 && nq <= OT_NQMAX;
    for (int it = 0; it < iters; ++it) {
        const float *vin = it == 0 ? nullptr : v;
        if (tiled) {
            OT_LAUNCH_NQ(ot_sweep_kernel, nq, dim3(nst, B), dim3(256), 0, s, S, L0, L1, rs, vin, a, norm, ubin0, u, cpm, cps);
            CHECK_LAUNCH();
            hipLaunchKernelGGL(ot_colfold_kernel, dim3((L1 + 255) / 256, B), dim3(256), 0, s, L0, L1, nst, cpm, cps, u, a, norm, v);
        } else {
            hipLaunchKernelGGL(ot_row_kernel, dim3((L0 + 3) / 4, B), dim3(256), 0, s, S, L0, L1, vin, a, norm, ubin0, u);
            CHECK_LAUNCH();
            hipLaunchKernelGGL(ot_col_kernel, dim3((L1 + 63) / 64, B), dim3(1024), 0, s, S, L0, L1, u, a, norm, v);
        }
        CHECK_LAUNCH();
        hipLaunchKernelGGL(ot_bin_kernel, dim3(B), dim3(256), 0, s, L0, L1, a, lmu_bin, lnu_bin, it == iters - 1 ? 1 : 0, u, v);
        CHECK_LAUNCH();
    }
    if (tiled) {
        OT_LAUNCH_NQ(ot_best_kernel, nq, dim3(nst, B), dim3(256), 0, s, S, L0, L1, rs, u, v, rbest, rarg, cpm);
        CHECK_LAUNCH();
        hipLaunchKernelGGL(ot_bestfold_kernel, dim3((L1 + 255) / 256, B), dim3(256), 0, s, L1, nst, cpm, cbest);
    } else {
        hipLaunchKernelGGL(ot_rowbest_kernel, dim3((L0 + 3) / 4, B), dim3(256), 0, s, S, L0, L1, u, v, rbest, rarg);
        CHECK_LAUNCH();
        hipLaunchKernelGGL(ot_colbest_kernel, dim3((L1 + 63) / 64, B), dim3(1024), 0, s, S, L0, L1, u, v, cbest);
    }
    CHECK_LAUNCH();
    hipLaunchKernelGGL(ot_match_kernel, dim3(B), dim3(256), 0, s, L0, L1, h0, w0, h1, w1, thr, border, norm, rbest, rarg, cbest, i_ids,
                       j_ids, mconf, n_match);
    CHECK_LAUNCH();
    return 0;
}

}   // extern "C"
