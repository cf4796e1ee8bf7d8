// emat_lds.h -- Nister's 5-point solver on the LDS (gfx950): the front end of a minimal solve (one lane each, working set in
// LDS) and the root stage (eight lanes each), joined by the record below.
//
// Restated cv.findEssentialMat minimal solver (lib/models/matching/pose_solver.py:46-48).  The reference of the arithmetic is
// oracle/mfr_oracle_emat.c (mfr_ref_fivept, mfr_ref_poly_real_roots): tests/test_gpu_emat_parity.py pins the counts and losses
// of every RANSAC iteration, the selected iteration, masks and poses to it bit for bit.
//
// Front end: every array that is indexed at run time (Gauss-Jordan pivoting, the monomial index tables) lives in LDS instead of
// the per-lane private segment.  emat_hyp_kernel ran one solve per lane with 5984 bytes of scratch per lane: every array access
// was a trip to the memory hierarchy and a launch of 16 k solves took 9.9 ms whatever the batch (pure latency, one wavefront per
// CU).  Layout: element e of lane l at word e * 64 + l (conflict-free ds_read/write_b64); 290 doubles per lane = 145 KB per
// 64-lane workgroup, by re-using dead regions:
//     [0, 36)    Ep[9][4]        null-space basis (live to the end)
//     [36, 236)  A[5][9] then M[10][20] (built directly in its column-permuted order), then P / c0 / c1 / c2 once Bx / By / B1
//                have been extracted
//     [236, 290) m[10], neg[4], one row of EEt[3][10], tr[10]; later Bx[3][4], By[3][4], B1[3][5]
// The trace-free part of E E^T is formed one row of blocks at a time (the diagonal blocks are evaluated twice, identically),
// which keeps the order of every floating-point operation of the oracle.
#pragma once
#include "emat_dev.h"

namespace mfr {

#define FP_LDS_DOUBLES 290

// The front end's record of one hypothesis, in the hypothesis' slot of Es: Ep[9][4] | Bx[3][4] | By[3][4] | B1[3][5] | P[11].
// fivept_front_lds writes it and returns FP_NSOL_PENDING for the hypothesis' nsol; fp_roots_group replaces the record by the
// hypothesis' <= 10 essential matrices (9 doubles each) and nsol by their number.
#define FP_REC_EP 0
#define FP_REC_BX 36
#define FP_REC_BY 48
#define FP_REC_B1 60
#define FP_REC_P 75
#define FP_REC_DOUBLES 86
#define FP_SLOT_DOUBLES 90          // 10 x 9: a hypothesis' slot of Es
#define FP_NSOL_PENDING (-1)        // front end done, roots pending

// the monomial index tables as compile-time constants: with the loops fully unrolled every LDS offset is an immediate (tables
// in memory cost a scalar load per multiply-add)
struct FpTables {
    int idx11[4][4] = { {0, 1, 2, 6}, {1, 3, 4, 7}, {2, 4, 5, 8}, {6, 7, 8, 9} };
    int idx21[10][4] = { {0, 1, 2, 10}, {1, 3, 4, 11}, {2, 4, 5, 12}, {3, 6, 7, 13}, {4, 7, 8, 14}, {5, 8, 9, 15}, {10, 11, 12, 16},
                         {11, 13, 14, 17}, {12, 14, 15, 18}, {16, 17, 18, 19} };
    // inverse of the oracle's column order perm of the 20 monomials: M[r][c] = C[r][perm[c]]  <=>  C[r][k] = M[r][nperm_inv[k]]
    int nperm_inv[20] = { 0, 2, 4, 3, 8, 10, 1, 6, 13, 16, 5, 9, 11, 7, 14, 17, 12, 15, 18, 19 };
};

struct LdsArr {
    double *p;                                        // lane's element 0
    __device__ __forceinline__ double &operator[](int i) const { return p[i * 64]; }
    __device__ __forceinline__ LdsArr at(int off) const { return LdsArr{ p + off * 64 }; }
};

// Horner on a register-resident, zero-padded coefficient vector.  Padding is exact: with c[k] = 0 for k > deg the first steps
// compute (+-0) * x + c[deg] = c[deg] bit for bit (x finite, c[deg] != 0), after which the recurrence is the original one.  The
// coefficients of a derivative level are loaded from LDS ONCE per level instead of once per Horner step: with one wavefront
// per CU a dependent LDS load per step (~100 cycles, 20 steps per Newton iteration, ~60 iterations x ~65 brackets, every lane
// waiting for the slowest) was >90 % of the solve.
template <int N>
MFR_DEV double horner_reg(const double (&c)[N], double x)
{
    double y = c[N - 1];
#pragma unroll
    for (int i = N - 2; i >= 0; --i) y = y * x + c[i];
    return y;
}

MFR_DEV void lds_mul11(LdsArr a, LdsArr b, LdsArr o)
{
    constexpr FpTables T{};
    double av[4], bv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { av[i] = a[i]; bv[i] = b[i]; }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) o[T.idx11[i][j]] = o[T.idx11[i][j]] + av[i] * bv[j];
}
// o is a row of the (column-permuted) M: monomial k lands in column nperm_inv[k]
MFR_DEV void lds_mul21_perm(LdsArr a, LdsArr b, LdsArr o)
{
    constexpr FpTables T{};
    double av[10], bv[4];
#pragma unroll
    for (int i = 0; i < 10; ++i) av[i] = a[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) bv[j] = b[j];
#pragma unroll
    for (int i = 0; i < 10; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) { const int c = T.nperm_inv[T.idx21[i][j]]; o[c] = o[c] + av[i] * bv[j]; }
}

// Front end of one minimal solve: null space, 10x20 constraint matrix, Gauss-Jordan, degree-10 polynomial.
// x0, x1: 5 normalised points each (registers); rec: the hypothesis' slot in GLOBAL memory, receives the record.
// S = this lane's LDS window (FP_LDS_DOUBLES doubles, stride 64), colp = this lane's int window (9 ints, stride 64).
// Returns FP_NSOL_PENDING (the root stage then runs in emat_roots_kernel with 8 lanes per hypothesis), or 0 on a degenerate
// pivot (no record).
MFR_DEV int fivept_front_lds(const double *x0, const double *x1, double *rec, double *lds_lane, int *colp_lane)
{
    const LdsArr S{ lds_lane };
    const LdsArr Ep = S, A = S.at(36), M = S.at(36), m = S.at(236), neg = S.at(246), EE = S.at(250), tr = S.at(280);
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const double a = x0[2 * i], b = x0[2 * i + 1], c = x1[2 * i], d = x1[2 * i + 1];
        const LdsArr Ai = A.at(9 * i);
        Ai[0] = c * a; Ai[1] = c * b; Ai[2] = c; Ai[3] = d * a; Ai[4] = d * b; Ai[5] = d;
        Ai[6] = a; Ai[7] = b; Ai[8] = 1.0;
    }
    for (int j = 0; j < 9; ++j) colp_lane[j * 64] = j;
    for (int r = 0; r < 5; ++r) {
        int pr = r, pc = r;
        double best = -1.0;
        for (int i = r; i < 5; ++i)
            for (int j = r; j < 9; ++j) {
                const double e = A[9 * i + j];
                const double v = e < 0.0 ? -e : e;
                if (v > best) { best = v; pr = i; pc = j; }
            }
        if (!(best > 1e-300)) return 0;
        if (pr != r)
            for (int j = 0; j < 9; ++j) { const double tmp = A[9 * r + j]; A[9 * r + j] = A[9 * pr + j]; A[9 * pr + j] = tmp; }
        if (pc != r) {
            for (int i = 0; i < 5; ++i) { const double tmp = A[9 * i + r]; A[9 * i + r] = A[9 * i + pc]; A[9 * i + pc] = tmp; }
            const int ti = colp_lane[r * 64]; colp_lane[r * 64] = colp_lane[pc * 64]; colp_lane[pc * 64] = ti;
        }
        const double inv = 1.0 / A[9 * r + r];
        double rr[9];                                     // pivot row staged in registers: batched LDS traffic, same arithmetic
#pragma unroll
        for (int j = 0; j < 9; ++j) rr[j] = A[9 * r + j];
#pragma unroll
        for (int j = 0; j < 9; ++j) { rr[j] = rr[j] * inv; A[9 * r + j] = rr[j]; }
        for (int i = 0; i < 5; ++i)
            if (i != r) {
                const double f = A[9 * i + r];
                double ri[9];
#pragma unroll
                for (int j = 0; j < 9; ++j) ri[j] = A[9 * i + j];
#pragma unroll
                for (int j = 0; j < 9; ++j) A[9 * i + j] = ri[j] - f * rr[j];
            }
    }
    for (int k = 0; k < 4; ++k) {
        // v[j] = 0 except v[5 + k] = 1 and v[r] = -A[r][5 + k] (r < 5); Ep[colp[j]][k] = v[j]
        for (int j = 0; j < 9; ++j) {
            double v = 0.0;
            if (j == 5 + k) v = 1.0;
            if (j < 5) v = -A[9 * j + 5 + k];
            Ep[colp_lane[j * 64] * 4 + k] = v;
        }
    }
    // ---- constraint matrix, built directly as M (A's region is dead now)
    for (int q = 0; q < 200; ++q) M[q] = 0.0;
#define MFR_MINOR_L(a, b, c, d)                                       \
    do {                                                              \
        for (int q = 0; q < 10; ++q) m[q] = 0.0;                      \
        lds_mul11(Ep.at(4 * (a)), Ep.at(4 * (b)), m);               \
        for (int q = 0; q < 4; ++q) neg[q] = -Ep[4 * (c) + q];        \
        lds_mul11(neg, Ep.at(4 * (d)), m);                          \
    } while (0)
    MFR_MINOR_L(4, 8, 5, 7); lds_mul21_perm(m, Ep.at(0), M);
    MFR_MINOR_L(5, 6, 3, 8); lds_mul21_perm(m, Ep.at(4), M);
    MFR_MINOR_L(3, 7, 4, 6); lds_mul21_perm(m, Ep.at(8), M);
#undef MFR_MINOR_L
    // trace of E E^T from its three diagonal blocks
    for (int i = 0; i < 3; ++i) {
        const LdsArr Eii = EE.at(10 * i);
        for (int q = 0; q < 10; ++q) Eii[q] = 0.0;
        for (int k = 0; k < 3; ++k) lds_mul11(Ep.at(4 * (3 * i + k)), Ep.at(4 * (3 * i + k)), Eii);
    }
    for (int q = 0; q < 10; ++q) tr[q] = (EE[q] + EE[10 + q]) + EE[20 + q];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) {
            const LdsArr Eij = EE.at(10 * j);
            for (int q = 0; q < 10; ++q) Eij[q] = 0.0;
            for (int k = 0; k < 3; ++k) lds_mul11(Ep.at(4 * (3 * i + k)), Ep.at(4 * (3 * j + k)), Eij);
        }
        for (int q = 0; q < 10; ++q) EE[10 * i + q] = EE[10 * i + q] - 0.5 * tr[q];
        for (int j = 0; j < 3; ++j)
            for (int k = 0; k < 3; ++k) lds_mul21_perm(EE.at(10 * k), Ep.at(4 * (3 * k + j)), M.at(20 * (1 + 3 * i + j)));
    }
    for (int c = 0; c < 10; ++c) {
        int pr = c;
        double best = -1.0;
        for (int i = c; i < 10; ++i) {
            const double e = M[20 * i + c];
            const double v = e < 0.0 ? -e : e;
            if (v > best) { best = v; pr = i; }
        }
        if (!(best > 1e-300)) return 0;
        if (pr != c)
            for (int j = 0; j < 20; ++j) { const double tmp = M[20 * c + j]; M[20 * c + j] = M[20 * pr + j]; M[20 * pr + j] = tmp; }
        const double inv = 1.0 / M[20 * c + c];
        double rc[20];
#pragma unroll
        for (int j = 0; j < 20; ++j) rc[j] = M[20 * c + j];
#pragma unroll
        for (int j = 0; j < 20; ++j) { rc[j] = rc[j] * inv; M[20 * c + j] = rc[j]; }
        for (int i = 0; i < 10; ++i)
            if (i != c) {
                const double f = M[20 * i + c];
                double ri[20];
#pragma unroll
                for (int j = 0; j < 20; ++j) ri[j] = M[20 * i + j];
#pragma unroll
                for (int j = 0; j < 20; ++j) M[20 * i + j] = ri[j] - f * rc[j];
            }
    }
    // [3][4], [3][4], [3][5] over the dead m / neg / EE / tr region, spaced as in the record
    const LdsArr Bx = S.at(236), By = Bx.at(FP_REC_BY - FP_REC_BX), B1 = Bx.at(FP_REC_B1 - FP_REC_BX);
    for (int r = 0; r < 3; ++r) {
        const LdsArr e = M.at(20 * (4 + 2 * r)), f = M.at(20 * (5 + 2 * r));
        Bx[4 * r] = e[12]; Bx[4 * r + 1] = e[11] - f[12]; Bx[4 * r + 2] = e[10] - f[11]; Bx[4 * r + 3] = -f[10];
        By[4 * r] = e[15]; By[4 * r + 1] = e[14] - f[15]; By[4 * r + 2] = e[13] - f[14]; By[4 * r + 3] = -f[13];
        B1[5 * r] = e[19]; B1[5 * r + 1] = e[18] - f[19]; B1[5 * r + 2] = e[17] - f[18]; B1[5 * r + 3] = e[16] - f[17]; B1[5 * r + 4] = -f[16];
    }
    // M's region is dead: P[11] | c0[8] | c1[8] | c2[7]
    const LdsArr P = S.at(36), c0 = S.at(47), c1 = S.at(55), c2 = S.at(63);
    for (int q = 0; q < 11; ++q) P[q] = 0.0;
    for (int q = 0; q < 8; ++q) { c0[q] = 0.0; c1[q] = 0.0; }
    for (int q = 0; q < 7; ++q) c2[q] = 0.0;
    for (int a = 0; a < 4; ++a)
        for (int b = 0; b < 5; ++b) {
            c0[a + b] = c0[a + b] + (By[4 + a] * B1[10 + b] - B1[5 + b] * By[8 + a]);
            c1[a + b] = c1[a + b] + (Bx[4 + a] * B1[10 + b] - B1[5 + b] * Bx[8 + a]);
        }
    for (int a = 0; a < 4; ++a)
        for (int b = 0; b < 4; ++b) c2[a + b] = c2[a + b] + (Bx[4 + a] * By[8 + b] - By[4 + a] * Bx[8 + b]);
    for (int a = 0; a < 4; ++a)
        for (int b = 0; b < 8; ++b) P[a + b] = P[a + b] + (Bx[a] * c0[b] - By[a] * c1[b]);
    for (int a = 0; a < 5; ++a)
        for (int b = 0; b < 7; ++b) P[a + b] = P[a + b] + B1[a] * c2[b];
    for (int q = 0; q < FP_REC_BX - FP_REC_EP; ++q) rec[FP_REC_EP + q] = Ep[q];
    for (int q = 0; q < FP_REC_P - FP_REC_BX; ++q) rec[FP_REC_BX + q] = Bx[q];      // Bx | By | B1 are contiguous, here as in the record
    for (int q = 0; q < FP_REC_DOUBLES - FP_REC_P; ++q) rec[FP_REC_P + q] = P[q];
    return FP_NSOL_PENDING;
}

// ---------------------------------------------------------------------------------------------------------------------
// Root stage with EIGHT lanes per hypothesis (emat_roots_kernel).  The derivative-isolation root finder is sequential across
// derivative levels but the brackets of one level are independent: the lanes of a group evaluate the bracket ends in parallel
// and refine the sign-change brackets in parallel, so a level costs the iterations of its slowest bracket instead of their
// sum, and 16 k hypotheses become 2000 wavefronts instead of 250 (one latency-bound wavefront per CU before).  Every
// bracket's rtsafe iteration, every Horner evaluation and every derivative coefficient ((c[i+L] * (i+L)) * (i+L-1) ... * (i+1),
// the multiplication order of the derivative tower) is the arithmetic of poly_real_roots (geom_dev.h; the oracle's
// mfr_ref_poly_real_roots): bit-identical roots.
// ---------------------------------------------------------------------------------------------------------------------
MFR_DEV double fp_dcoef(const double (&c)[11], int L, int i)      // coefficient i of the L-th derivative
{
    double v = 0.0;
#pragma unroll
    for (int k = 0; k < 11; ++k) if (k == i + L) v = c[k];
    for (int k = L; k >= 1; --k) v = v * (double)(i + k);
    return v;
}

#define FPR_GROUP 8
#define FPR_HYP_PER_WG 32
struct FprShared {                                  // per hypothesis
    double in[FP_REC_P];                            // the record up to P: Ep[36] | Bx[12] | By[12] | B1[15]
    double ends[12], fe[12], rr[12], crit[12];
    int ne, nc;
};

MFR_DEV void fp_roots_group(double *slot, int32_t *nsol_out, volatile FprShared *sh, int sub, bool active)
{
    double c[11];
#pragma unroll
    for (int k = 0; k < 11; ++k) c[k] = active ? slot[FP_REC_P + k] : 0.0;
    if (active) {
        for (int q = sub; q < FP_REC_P; q += FPR_GROUP) sh->in[q] = slot[q];
    }
    int deg = 10;                                   // while (deg > 0 && c[deg] == 0) --deg, with static register indices
#pragma unroll
    for (int k = 10; k >= 1; --k) if (deg == k && c[k] == 0.0) deg = k - 1;
    double bound = 0.0, cdeg = 0.0;
#pragma unroll
    for (int k = 0; k < 11; ++k) if (k == deg) cdeg = c[k];
    bool live = active && deg > 0;
    if (live) {
        for (int i = 0; i < deg; ++i) {
            double ci = 0.0;
#pragma unroll
            for (int k = 0; k < 11; ++k) if (k == i) ci = c[k];
            double r = ci / cdeg;
            if (r < 0.0) r = -r;
            if (r > bound) bound = r;
        }
        bound = bound + 1.0;
        if (!(bound < 1e300)) live = false;
    }
    int nc = 0;
    if (live) {
        nc = 1;
        if (sub == 0) sh->crit[0] = -fp_dcoef(c, deg - 1, 0) / fp_dcoef(c, deg - 1, 1);
    }
    int L = live ? deg - 2 : -1;
    while (__ballot(L >= 0)) {
        const bool lv = L >= 0;
        double pc[11], dpc[10];
        const int m = deg - L;
#pragma unroll
        for (int k = 0; k < 11; ++k) pc[k] = (lv && k <= m) ? fp_dcoef(c, L, k) : 0.0;
#pragma unroll
        for (int k = 0; k < 10; ++k) dpc[k] = (lv && k <= m - 1) ? fp_dcoef(c, L + 1, k) : 0.0;
        // bracket ends: -bound, the increasing critical points of the level above, +bound (the scan's `continue` rule)
        if (lv && sub == 0) {
            int ne = 0;
            double last = -bound;
            sh->ends[ne++] = last;
            for (int i = 0; i <= nc; ++i) {
                const double xh = (i < nc) ? sh->crit[i] : bound;
                if (i < nc && !(xh > last)) continue;
                sh->ends[ne++] = xh; last = xh;
            }
            sh->ne = ne;
        }
        const int ne = lv ? sh->ne : 0;
        for (int j = sub; j < ne; j += FPR_GROUP) sh->fe[j] = horner_reg(pc, sh->ends[j]);
        for (int j0 = 0; j0 < 12; j0 += FPR_GROUP) {                   // refinements of the sign-change brackets, one per lane
            const int j = j0 + sub;
            bool work = false;
            double lo = 0.0, hi = 0.0, flo = 0.0;
            if (lv && j + 1 < ne) {
                const double fl = sh->fe[j], fh = sh->fe[j + 1];
                if (fl != 0.0 && fh != 0.0 && ((fl < 0.0) != (fh < 0.0))) { work = true; lo = sh->ends[j]; hi = sh->ends[j + 1]; flo = fl; }
            }
            if (!__ballot(work)) continue;
            // refine_root of geom_dev.h (safeguarded Newton, rtsafe), run in lock step by the lanes that have a bracket: each lane
            // executes that loop's statements on its own bracket
            double x = 0.5 * (lo + hi), dxold = hi - lo, dx = dxold;
            double fx = work ? horner_reg(pc, x) : 0.0, dfx = work ? horner_reg(dpc, x) : 1.0;
            int it = 0;
            bool run = work;
            while (__ballot(run)) {
                if (run) {
                    if (it >= 200 || fx == 0.0) run = false;
                    else {
                        if ((fx < 0.0) == (flo < 0.0)) lo = x; else hi = x;
                        const double a = (x - hi) * dfx - fx, b = (x - lo) * dfx - fx;
                        double tf = 2.0 * fx;
                        if (tf < 0.0) tf = -tf;
                        double td = dxold * dfx;
                        if (td < 0.0) td = -td;
                        const bool newton = ((a < 0.0) != (b < 0.0)) && (tf <= td);
                        double xn;
                        dxold = dx;
                        if (newton) { dx = fx / dfx; xn = x - dx; }
                        else { dx = 0.5 * (hi - lo); xn = lo + dx; }
                        if (!(xn > lo && xn < hi)) { dx = 0.5 * (hi - lo); xn = lo + dx; }
                        if (xn == x) run = false;
                        else {
                            const double adx = dx < 0.0 ? -dx : dx, ax = xn < 0.0 ? -xn : xn;
                            x = xn;
                            if (adx <= 2e-16 * ax || adx < 1e-300) run = false;
                            else { fx = horner_reg(pc, x); dfx = horner_reg(dpc, x); ++it; }
                        }
                    }
                }
            }
            if (work) sh->rr[j] = x;
        }
        // the scan's bookkeeping, in bracket order (one lane; the refined roots are ready)
        if (lv && sub == 0) {
            int nr = 0;
            double prev = 0.0;
            for (int j = 0; j + 1 < ne; ++j) {
                const double xl = sh->ends[j], fl = sh->fe[j], fh = sh->fe[j + 1];
                if (fl == 0.0) { if (nr == 0 || prev != xl) { sh->crit[nr++] = xl; prev = xl; } }
                else if (fh != 0.0 && ((fl < 0.0) != (fh < 0.0))) { prev = sh->rr[j]; sh->crit[nr++] = prev; }
            }
            const double xl = sh->ends[ne - 1], fl = sh->fe[ne - 1];
            if (fl == 0.0 && (nr == 0 || prev != xl)) sh->crit[nr++] = xl;
            sh->nc = nr;
        }
        if (lv) { nc = sh->nc; --L; }
    }
    // one E per real root (the tail of the oracle's mfr_ref_fivept), roots handled in parallel, compacted in root order
    int ns = 0;
    for (int r0 = 0; r0 < 16; r0 += FPR_GROUP) {
        const int r = r0 + sub;
        bool ok = false;
        double ev[9];
        if (live && r < nc) {
            const double z = sh->crit[r];
            const volatile double *Ep = sh->in + FP_REC_EP, *Bx = sh->in + FP_REC_BX, *By = sh->in + FP_REC_BY, *B1 = sh->in + FP_REC_B1;
            double bx[3], by[3], b1[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                bx[k] = ((Bx[4 * k + 3] * z + Bx[4 * k + 2]) * z + Bx[4 * k + 1]) * z + Bx[4 * k];
                by[k] = ((By[4 * k + 3] * z + By[4 * k + 2]) * z + By[4 * k + 1]) * z + By[4 * k];
                b1[k] = (((B1[5 * k + 4] * z + B1[5 * k + 3]) * z + B1[5 * k + 2]) * z + B1[5 * k + 1]) * z + B1[5 * k];
            }
            double v0 = 0.0, v1 = 0.0, v2 = 0.0, bestw = -1.0;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const int p = a, q = (a + 1) % 3;
                const double w0 = by[p] * b1[q] - b1[p] * by[q];
                const double w1 = b1[p] * bx[q] - bx[p] * b1[q];
                const double w2 = bx[p] * by[q] - by[p] * bx[q];
                const double aw = w2 < 0.0 ? -w2 : w2;
                if (aw > bestw) { bestw = aw; v0 = w0; v1 = w1; v2 = w2; }
            }
            if (bestw > 0.0) {
                const double x = v0 / v2, y = v1 / v2;
                double nn = 0.0;
#pragma unroll
                for (int e = 0; e < 9; ++e) {
                    ev[e] = ((x * Ep[4 * e] + y * Ep[4 * e + 1]) + z * Ep[4 * e + 2]) + Ep[4 * e + 3];
                    nn = nn + ev[e] * ev[e];
                }
                if ((nn > 0.0) && (nn < 1e300)) {
                    const double s = 1.0 / sqrt(nn);
#pragma unroll
                    for (int e = 0; e < 9; ++e) ev[e] = ev[e] * s;
                    ok = true;
                }
            }
        }
        const unsigned long long bal = __ballot(ok);
        const int lane = (int)(threadIdx.x & 63), gbase = lane & ~(FPR_GROUP - 1);
        const unsigned seg = (unsigned)((bal >> gbase) & 0xffull);
        if (ok) {
            double *E = slot + 9 * (ns + __popc(seg & ((1u << sub) - 1u)));
#pragma unroll
            for (int e = 0; e < 9; ++e) E[e] = ev[e];
        }
        ns += __popc(seg);
    }
    if (active && sub == 0) *nsol_out = ns;
}

}  // namespace mfr
