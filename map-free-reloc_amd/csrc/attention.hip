// attention.hip -- SuperGlue multi-head softmax attention (self and cross) on gfx950: the exact-fp32 kernel (rounds 1-2, kept for A/B and parity),
// and ONE software-pipelined kernel body on the 16-bit matrix cores at fp32 accuracy by operand splitting, instantiated for two arithmetics
// (AtF16x2: round 5, the default; AtBf16x3: rounds 3-4, what an out-of-range scene is re-run on).  The split body's online softmax keeps a STALE
// per-query reference that moves only when a tile's maximum outgrows it by 2^AT_TAU (the exact-fp32 kernel keeps the running maximum).
//
// Reference call site: SuperGlue_matcher (etc/feature_matching_baselines/matchers.py:62-120) ->
// upstream AttentionalGNN / MultiHeadedAttention (un-vendored):
//     prob = softmax(q^T k / sqrt(64)) ; message = prob v        4 heads x 64, N <= 1024 keypoints,
// applied 18 x 2 times per image pair.  Upstream materialises the [4, N, N] score tensor
// (16.8 MB fp32 per application); here it never leaves registers (flash-style online softmax).
//
// Mapping to CDNA4: one wavefront owns 32 queries.  Both contractions run on the exact-fp32
// matrix cores (v_mfma_f32_32x32x2_f32: bit-identical to an fmaf chain, so no precision is traded
// against the fp32 reference):
//   S^T[key, q] = sum_d K[key,d] Q[q,d]   A = K tile (LDS, 16-B reads, row stride 68 floats:
//                                         conflict-free), B = Q^T held in 32 VGPRs for the whole loop
//   O^T[d, q]   = sum_key V[key,d] P[key,q]  A = V tile (LDS), B = P -- the probabilities are consumed
//                                         as the B operand IN the accumulator layout S^T was produced
//                                         in (row<->key pairing chosen to match), so P never moves.
// Softmax statistics are per query = per lane column: the row reduction is 16 in-register maxes /
// adds plus ONE cross-half exchange (lane ^ 32).  K/V tiles (32 keys) are prefetched into
// registers while the previous tile is being multiplied and double-buffered in LDS (one barrier
// per tile).  Keys >= n_tok[image] are masked; cross attention just reads the partner image's K/V
// (image b ^ 1), no copy.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mfr_hip.h"
#include "wave_dev.h"
#include "split_f16.h"
#include "guard.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

#define AT_D 64
#define AT_KT 32            // keys per tile
#define AT_KS 68            // K tile row stride (floats): 272 B -> conflict-free ds_read_b128
#define AT_QW 32            // queries per wavefront
// The split kernels' softmax reference moves only when a tile's maximum exceeds it by more than AT_TAU (in log2 units), so 0 < p <= 2^AT_TAU.
// Derived, not tuned: f16x2 needs p <= 65504, and its low term is (p - ph) 2^11 <= 2^(AT_TAU - 11) 2^11 = 2^AT_TAU <= 65504, i.e. AT_TAU <= 15 by
// range; 14 leaves a factor of two for the rounding of exp2 and of the comparison.  bf16x3 has no range limit and shares the body and the constant.
constexpr float AT_TAU = 14.0f;
#define AT_WAVES 4

// The two stores every kernel here ends in; lane (q, half) of a wavefront owns query row q.
// rows >= n_tok are defined to be zero: row = the lane's 32 channels (32 half ..) of its head
__device__ __forceinline__ void at_store_zero_row(float *row)
{
#pragma unroll
    for (int g = 0; g < 8; ++g) ((float4 *)row)[g] = make_float4(0.f, 0.f, 0.f, 0.f);
}
// O^T accumulators of channels 0-31 (o0) / 32-63 (o1): rows (r&3) + 8(r>>2) + 4 half, r = 4g..4g+3 -> 4 consecutive d starting at 8g + 4 half (op points at d = 4 half)
__device__ __forceinline__ void at_store_normalised(float *op, f32x16 o0, f32x16 o1, float inv)
{
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        *(float4 *)(op + 8 * g) = make_float4(o0[4 * g] * inv, o0[4 * g + 1] * inv, o0[4 * g + 2] * inv, o0[4 * g + 3] * inv);
        *(float4 *)(op + 32 + 8 * g) = make_float4(o1[4 * g] * inv, o1[4 * g + 1] * inv, o1[4 * g + 2] * inv, o1[4 * g + 3] * inv);
    }
}

__global__ void __launch_bounds__(256, 2) sg_attention_kernel(
    const float *__restrict__ Q, const float *__restrict__ Kp, const float *__restrict__ Vp, int ld,
    int N, int heads, int B2, const int *__restrict__ n_tok, int cross, float scale_log2e, float *__restrict__ O, int ldo)
{
    __shared__ __attribute__((aligned(16))) float Ks[2][AT_KT][AT_KS];
    __shared__ __attribute__((aligned(16))) float Vs[2][AT_KT][AT_D];
    // 1-D grid, (image, head) fastest: workgroup L runs on XCD L % 8 (observed dispatch), so with
    // heads*B2 a multiple of 8 all query blocks of one (image, head) share an XCD and its K/V tiles are
    // fetched into that XCD's L2 once instead of once per query block (PMC: 5.6x the algorithmic reads
    // with the query block as the fastest index)
    const int nbh = heads * B2;
    const int bh = blockIdx.x % nbh, qb = blockIdx.x / nbh;
    const int b = bh / heads, h = bh - b * heads;
    const int bk = cross ? (b ^ 1) : b;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int ql = lane & 31, half = lane >> 5;
    const int nq = n_tok[b], nk = n_tok[bk];
    const int q0 = qb * (AT_QW * AT_WAVES);
    const int q = q0 + wid * AT_QW + ql;
    if (q0 >= nq) {                                         // whole workgroup beyond this image's keypoints
        if (q < N) at_store_zero_row(O + ((size_t)b * N + q) * ldo + h * AT_D + 32 * half);
        return;
    }

    // Q^T operand: lane (q, half) keeps Q[q][half*32 + s], s = 0..31, pre-scaled by log2(e)/sqrt(64)
    float qreg[32];
    {
        const bool ok = q < N;
        const float4 *qp = (const float4 *)(Q + ((size_t)b * N + (ok ? q : 0)) * ld + h * AT_D + half * 32);
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            float4 t = ok ? qp[g] : make_float4(0.f, 0.f, 0.f, 0.f);
            qreg[4 * g] = t.x * scale_log2e; qreg[4 * g + 1] = t.y * scale_log2e;
            qreg[4 * g + 2] = t.z * scale_log2e; qreg[4 * g + 3] = t.w * scale_log2e;
        }
    }
    f32x16 o0, o1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { o0[r] = 0.f; o1[r] = 0.f; }
    float m_run = -INFINITY, l_run = 0.f;

    // staging assignment: thread -> (row r and r+16, 4 floats at column c4*4)
    const int sr = tid >> 4, sc = (tid & 15) * 4;
    const float *kbase = Kp + (size_t)bk * N * ld + h * AT_D + sc;
    const float *vbase = Vp + (size_t)bk * N * ld + h * AT_D + sc;
    const int ntiles = (nk + AT_KT - 1) / AT_KT;
    float4 kr0, kr1, vr0, vr1;
    auto gload = [&](int t) {
        const int k0 = t * AT_KT + sr, k1 = k0 + 16;
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        kr0 = (k0 < nk) ? *(const float4 *)(kbase + (size_t)k0 * ld) : z;
        kr1 = (k1 < nk) ? *(const float4 *)(kbase + (size_t)k1 * ld) : z;
        vr0 = (k0 < nk) ? *(const float4 *)(vbase + (size_t)k0 * ld) : z;
        vr1 = (k1 < nk) ? *(const float4 *)(vbase + (size_t)k1 * ld) : z;
    };
    auto lstore = [&](int buf) {
        *(float4 *)&Ks[buf][sr][sc] = kr0; *(float4 *)&Ks[buf][sr + 16][sc] = kr1;
        *(float4 *)&Vs[buf][sr][sc] = vr0; *(float4 *)&Vs[buf][sr + 16][sc] = vr1;
    };
    if (ntiles > 0) { gload(0); lstore(0); }
    __syncthreads();

    for (int t = 0; t < ntiles; ++t) {
        const int buf = t & 1;
        if (t + 1 < ntiles) gload(t + 1);                   // in flight during the MFMAs below

        // ---- S^T = K Q^T (32 keys x 32 queries, contraction 64 as 32 steps of 2)
        f32x16 s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.f;
        const float *krow = &Ks[buf][ql][half * 32];
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            const float4 a = *(const float4 *)(krow + 4 * g);
            s = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, qreg[4 * g], s, 0, 0, 0);
            s = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, qreg[4 * g + 1], s, 0, 0, 0);
            s = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, qreg[4 * g + 2], s, 0, 0, 0);
            s = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, qreg[4 * g + 3], s, 0, 0, 0);
        }
        // ---- online softmax over this tile's keys (rows of S^T); key = (r&3) + 8(r>>2) + 4 half
        const int kb = t * AT_KT + 4 * half;
        float mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = kb + (r & 3) + 8 * (r >> 2);
            if (key >= nk) s[r] = -INFINITY;
            mx = fmaxf(mx, s[r]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);               // finite: tile 0 always holds key 0
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
        float rs = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) { s[r] = __builtin_amdgcn_exp2f(s[r] - m_new); rs += s[r]; }
        rs += __shfl_xor(rs, 32, 64);
        l_run = l_run * alpha + rs;
        m_run = m_new;
#pragma unroll
        for (int r = 0; r < 16; ++r) { o0[r] *= alpha; o1[r] *= alpha; }
        // ---- O^T += V^T P   (A = V[key(r,half)][d], B = p[r])
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = 4 * half + (r & 3) + 8 * (r >> 2);
            const float a0 = Vs[buf][key][ql], a1 = Vs[buf][key][32 + ql];
            o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, s[r], o0, 0, 0, 0);
            o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, s[r], o1, 0, 0, 0);
        }
        if (t + 1 < ntiles) lstore(buf ^ 1);
        __syncthreads();
    }

    if (q < N) {
        const float inv = (l_run > 0.f && q < nq) ? 1.f / l_run : 0.f;
        at_store_normalised(O + ((size_t)b * N + q) * ldo + h * AT_D + 4 * half, o0, o1, inv);
    }
}


// ------------------------------------------------------------------------------------------------------------------
// The same attention on the 16-bit matrix cores at fp32 accuracy: every fp32 operand is split into NT 16-bit terms and a product is
// evaluated as a few partial products accumulated in fp32.  An arithmetic (AtBf16x3 / AtF16x2 below) is: NT operand terms = LDS term images,
// NO accumulator sets of O^T, the split of a value pair (split2), the MFMAs of one S^T step and of 16 keys of O^T (AT_*_QK / AT_*_PV), how two
// accumulators fold into one value (fold), and three switches (WEAVE, GUARD, P_COPY).  Everything else -- decomposition, staging, pipeline,
// mask, softmax, store -- is sg_attention_split_p.
// Structure as above (one wavefront = 32 queries, 32-key tiles, online softmax in the accumulator layout, P never moves):
//   S^T = K Q^T   A = K tile split in LDS (row stride 72 halfwords: conflict-free 16-B reads), B = Q^T split once into 16 NT VGPRs
//   O^T = V^T P   A = V^T tile split in LDS, keys stored in the order the S^T accumulator hands them out (position
//                 16s + 8h + 4g + j for key 16s + 8g + 4h + j), so a lane's eight contraction slots are one 16-B read;
//                 B = P split in registers (16 values per lane per tile)
// The K / V tiles are split once per workgroup by the staging threads (V is fetched d-per-lane so that its transpose
// is two 8-byte LDS stores per term).
typedef short bf16x8 __attribute__((ext_vector_type(8)));

#define AB_KS 72            // K tile row stride (halfwords): 144 B
#define AB_VS 40            // V^T tile row stride (halfwords): 80 B
#define AB_WAVES 8

typedef float at_f2 __attribute__((ext_vector_type(2)));
union Frag8 { bf16x8 v; unsigned u[4]; uint4 q; };

// ---- "bf16x3" (variant 2; what the range guard re-runs a scene on): every fp32 operand x is split EXACTLY into three bf16 terms x = h + m + l
// (truncation: 8 + 8 + 8 significand bits), and a product a.b is evaluated as the six partial products hh + hm + mh + hl + lh + mm (each exact in
// fp32) accumulated in fp32 by v_mfma_f32_32x32x16_bf16 -- the dropped terms (ml, lm, ll) are below 2^-26 |a||b|.  Measured against an fp64
// product (tools/ubench/bf16x3_probe.hip, profiles/r03_bf16x3_probe.jsonl; K = 64 .. 2304): rms / max error 2.4e-8 / 2.3e-7 of sum|a||b|, vs
// 2.8e-8 / 2.6e-7 for the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32) on the same data -- the same error class, at 16/6 = 2.7x the matrix rate.
// Two accumulator chains per product (s / s2) that simply add; no range precondition, hence no guard.  Its 24 + 24 MFMAs per tile are woven
// with the VALU work by sched_group_barrier (one MFMA, then up to nv VALU).  P_COPY: the probabilities reach split2 through a copy of eight; without
// it hipcc's SLP pass emits the split of P ahead of the O^T MFMAs and two packed adds of the loop fall apart into four scalar ones (f16x2: the
// reverse, two more waits with the copy).
// (The MFMA groups are macros on the kernel's own accumulator variables: handed to a function by reference, the accumulators are promoted to
// registers only after inlining, the loop's phi order changes and eight 64-bit register copies appear in front of the loop.)
#define MFMA_BF16(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16((a).v, (b).v, (c), 0, 0, 0)
// kf / qf: [h, m, l] of 16 contraction slots
#define AT_BF16X3_QK(kf, qf, s, s2) do { \
        s2 = MFMA_BF16(kf[1], qf[1], s2); s = MFMA_BF16(kf[0], qf[2], s); s2 = MFMA_BF16(kf[2], qf[0], s2); \
        s = MFMA_BF16(kf[0], qf[1], s); s2 = MFMA_BF16(kf[1], qf[0], s2); s = MFMA_BF16(kf[0], qf[0], s); } while (0)
// vf: 0 / 1 = h term of channels 0-31 / 32-63, 2 / 3 = m, 4 / 5 = l
#define AT_BF16X3_PV(vf, pf, o0, o1) do { \
        o0 = MFMA_BF16(vf[2], pf[1], o0); o1 = MFMA_BF16(vf[3], pf[1], o1); o0 = MFMA_BF16(vf[0], pf[2], o0); o1 = MFMA_BF16(vf[1], pf[2], o1); \
        o0 = MFMA_BF16(vf[4], pf[0], o0); o1 = MFMA_BF16(vf[5], pf[0], o1); o0 = MFMA_BF16(vf[0], pf[1], o0); o1 = MFMA_BF16(vf[1], pf[1], o1); \
        o0 = MFMA_BF16(vf[2], pf[0], o0); o1 = MFMA_BF16(vf[3], pf[0], o1); o0 = MFMA_BF16(vf[0], pf[0], o0); o1 = MFMA_BF16(vf[1], pf[0], o1); } while (0)
struct AtBf16x3 {
    static constexpr int NT = 3, NO = 1;
    static constexpr bool WEAVE = true, GUARD = false, P_COPY = true;
    // two values at a time: the subtractions are packed fp32 instructions (v_pk_add_f32 with a negated operand, one issue slot for two lanes of data);
    // word(k) = where term k's packed pair goes (written in place: through a temporary the fragment words are assembled after all three terms)
    template <class W> static __device__ __forceinline__ void split2(float x0f, float x1f, W &&word)
    {
        at_f2 x; x.x = x0f; x.y = x1f;
        const unsigned x0 = __float_as_uint(x.x), x1 = __float_as_uint(x.y);
        at_f2 h; h.x = __uint_as_float(x0 & 0xffff0000u); h.y = __uint_as_float(x1 & 0xffff0000u);
        const at_f2 r = x - h;
        const unsigned r0 = __float_as_uint(r.x), r1 = __float_as_uint(r.y);
        at_f2 m; m.x = __uint_as_float(r0 & 0xffff0000u); m.y = __uint_as_float(r1 & 0xffff0000u);
        const at_f2 l = r - m;
        word(0) = bf_pack_hi16(x0, x1); word(1) = bf_pack_hi16(r0, r1); word(2) = bf_pack_hi16(__float_as_uint(l.x), __float_as_uint(l.y));
    }
    static __device__ __forceinline__ float fold(float main, float second) { return main + second; }
};

// ---- "f16x2" (variant 0, the default; split_f16.h): both operands of both contractions are activations, so there is no packed weight to carry
// the 2^-11: every operand is split the activation way, x -> xh = rne_f16(x), xl = rne_f16((x - xh) 2^11), and a contraction keeps TWO accumulators,
//     main += ah bh          corr += ah bl + al bh          result = main + 2^-11 corr          (dropped: al bl 2^-22, below 2^-24 |a||b|)
// i.e. THREE v_mfma_f32_32x32x16_f16 per block instead of six bf16 ones, 2.5 instead of 5.5 VALU per split element (K, V: once per 256 queries
// at staging; P: per tile in registers), two instead of three term images of K / V in LDS and 32 instead of 48 registers of Q.  The S^T tile
// has two accumulator chains anyway (s, s2), so the fold is one fma per score; O^T carries a correction pair (32 registers).  Every operand
// term is good to 2^-24 relative for |x| >= 2^-12 and to an absolute 2^-36 below (P <= 1: its tiny entries are exact to 2^-36).  The f16 terms
// overflow beyond 65504: the kernel carries the range guard (guard.h).
#define MFMA_F16(a, b, c) SF_MFMA((a).q, (b).q, (c))
// kf / qf: [h, l]; corr += kh ql + kl qh (s2), main += kh qh (s)
#define AT_F16X2_QK(kf, qf, s, s2) do { s2 = MFMA_F16(kf[0], qf[1], s2); s = MFMA_F16(kf[0], qf[0], s); s2 = MFMA_F16(kf[1], qf[0], s2); } while (0)
// vf: 0 / 1 = h term of channels 0-31 / 32-63, 2 / 3 = l term; o0 / o1 = main, c0 / c1 = correction
#define AT_F16X2_PV(vf, pf, o0, o1, c0, c1) do { \
        c0 = MFMA_F16(vf[0], pf[1], c0); c1 = MFMA_F16(vf[1], pf[1], c1); o0 = MFMA_F16(vf[0], pf[0], o0); o1 = MFMA_F16(vf[1], pf[0], o1); \
        c0 = MFMA_F16(vf[2], pf[0], c0); c1 = MFMA_F16(vf[3], pf[0], c1); } while (0)
struct AtF16x2 {
    static constexpr int NT = 2, NO = 2;
    static constexpr bool WEAVE = false, GUARD = true, P_COPY = false;
    template <class W> static __device__ __forceinline__ void split2(float x0, float x1, W &&word) { sf_split2(x0, x1, SF_LOW_SCALE, word(0), word(1)); }
    static __device__ __forceinline__ float fold(float main, float second) { return __builtin_fmaf(second, 1.0f / SF_LOW_SCALE, main); }
};

// Measurement build only (tools/attention_rescale_count.py compiles THIS file a second time with -DAT_PROF into tools/ubench/libmfr_hip_att_prof.so; the
// product library never defines it): per launch (slot = launch number mod AT_PROF_SLOTS) the tiles executed, the tiles whose rescale branch was
// taken, and the tiles in which the branch of a reference that follows the running maximum (m_true, what the kernel did before AT_TAU) would have
// been taken; counted per wavefront in scalars, one atomicAdd per counter and wavefront at exit.
#ifdef AT_PROF
#define AT_PROF_SLOTS 64
__device__ unsigned at_prof[AT_PROF_SLOTS][3];
static int at_prof_launches = 0;
#define AT_PROF_DECL , int prof_slot
#define AT_PROF_PASS , prof_slot
#define AT_PROF_NEXT , (at_prof_launches++ % AT_PROF_SLOTS)
#define AT_PROF_INIT() float m_true = -INFINITY; unsigned prof_resc = 0, prof_run = 0
#define AT_PROF_TILE(mx) do { const float mt_ = fmaxf(m_true, (mx)); prof_run += __ballot(mt_ != m_true) != 0ull; m_true = mt_; } while (0)
#define AT_PROF_RESCALED() (++prof_resc)
#define AT_PROF_COMMIT(ntiles) do { if (lane == 0) { atomicAdd(&at_prof[prof_slot][0], (unsigned)(ntiles)); atomicAdd(&at_prof[prof_slot][1], prof_resc); \
        atomicAdd(&at_prof[prof_slot][2], prof_run); } } while (0)
#else
#define AT_PROF_DECL
#define AT_PROF_PASS
#define AT_PROF_NEXT
#define AT_PROF_INIT() do { } while (0)
#define AT_PROF_TILE(mx) do { } while (0)
#define AT_PROF_RESCALED() do { } while (0)
#define AT_PROF_COMMIT(ntiles) do { } while (0)
#endif

// ---- the pipelined kernel: eight wavefronts (256 queries) per workgroup -------------------------------------------------------------------------
// K / V rows are read through buffer descriptors that end at row nk: the row offset of a tile is a SCALAR (no address VALU), rows beyond nk
// read as zero in hardware (no clamp, no select); a K / V tile is split once per 256 queries.  (Round 3's 128-query kernel and the
// non-pipelined eight-wavefront kernel computed the same bits and left the library in round 5: profiles/r04_bench_attention.json.)
// Without pipelining a wavefront's tile is [S^T MFMAs] -> [softmax: ~120 VALU slots, no MFMA] -> [O^T MFMAs, with the split of P];
// the barrier per tile keeps all wavefronts of the CU in the same phase, so the matrix core idles through every softmax (measured on bf16x3: a
// tile costs a SIMD the SUM of its two wavefronts' MFMA and VALU time, 5400 cycles for 3072 of MFMA).  Here the score product runs one tile ahead:
// iteration t issues S^T(t+1) = K(t+1) Q^T in four steps, and between them the softmax of tile t (whose scores were finished an
// iteration ago) -- independent instruction streams that one wavefront overlaps by itself; then O^T += V(t)^T P(t).  K is therefore staged one
// tile further ahead than V (K(t+2) and V(t+1) are written during iteration t; two LDS stages each).  Per query the same
// arithmetic in the same order as a non-pipelined loop.  The two __global__ kernels below are this body with an arithmetic.
// The softmax reference is STALE: flash-style softmax is exact for any per-query reference m_ref (p = exp2(s - m_ref); the final division by l_run
// cancels it), so m_ref follows the running maximum only when a tile's maximum exceeds it by more than AT_TAU.  Rescaling the accumulator sets and
// l_run -- one exp2 and 33 (packed) multiplies that no MFMA overlaps -- thereby becomes a cold, wave-uniform branch instead of one taken whenever
// any of the wavefront's 32 queries saw a new maximum (share of tiles, before -> after: profiles/attention_rescale_ab.json).  Invariants:
//   m_ref <= the true running maximum <= m_ref + AT_TAU   (m_ref is a tile maximum once set; a tile that exceeds m_ref + AT_TAU moves it)
//   hence 0 < p <= 2^AT_TAU, inside the f16 operand range with its low term (AT_TAU), and l_run >= 1 from the tile that set m_ref on;
//   small probabilities are no less precise than with the running maximum as reference: against a stale reference they are LARGER.
// A NaN tile maximum (an out-of-range q row: every score NaN) never moves the reference (the comparison is false); p = exp2(NaN - m_ref) is NaN all
// the same, so the accumulators the range guard tests still turn NaN.
template <class AR>
__device__ __forceinline__ void sg_attention_split_p(
    const float *Q, const float *Kp, const float *Vp, int ld, int N, int heads, int B2, const int *n_tok, int cross, float scale_log2e, float *O, int ldo, int *guard AT_PROF_DECL)
{
    constexpr int NT = AR::NT, NO = AR::NO;
    __shared__ __attribute__((aligned(16))) unsigned short Ks[2][NT][AT_KT][AB_KS];
    __shared__ __attribute__((aligned(16))) unsigned short Vt[2][NT][AT_D][AB_VS];
    const int nbh = heads * B2;
    const int bh = blockIdx.x % nbh, qb = blockIdx.x / nbh;
    const int b = bh / heads, h = bh - b * heads;
    const int bk = cross ? (b ^ 1) : b;
    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ql = lane & 31, half = lane >> 5;
    const int nq = n_tok[b], nk = n_tok[bk];
    const int q0 = qb * (AT_QW * AB_WAVES);
    const int q = q0 + wid * AT_QW + ql;
    if (q0 >= nq) {
        if (q < N) at_store_zero_row(O + ((size_t)b * N + q) * ldo + h * AT_D + 32 * half);
        return;
    }

    Frag8 qf[4][NT];                                        // [step][term]
    {
        const bool ok = q < N;
        const float *qp = Q + ((size_t)b * N + (ok ? q : 0)) * ld + h * AT_D + half * 8;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            float4 t0 = *(const float4 *)(qp + 16 * s), t1 = *(const float4 *)(qp + 16 * s + 4);
            if (!ok) { t0 = make_float4(0.f, 0.f, 0.f, 0.f); t1 = t0; }
            AR::split2(t0.x * scale_log2e, t0.y * scale_log2e, [&](int k) -> unsigned & { return qf[s][k].u[0]; });
            AR::split2(t0.z * scale_log2e, t0.w * scale_log2e, [&](int k) -> unsigned & { return qf[s][k].u[1]; });
            AR::split2(t1.x * scale_log2e, t1.y * scale_log2e, [&](int k) -> unsigned & { return qf[s][k].u[2]; });
            AR::split2(t1.z * scale_log2e, t1.w * scale_log2e, [&](int k) -> unsigned & { return qf[s][k].u[3]; });
        }
    }
    f32x16 o0, o1, c0, c1;                                  // O^T of channels 0-31 / 32-63: main and (NO = 2) correction accumulators
#pragma unroll
    for (int r = 0; r < 16; ++r) { o0[r] = 0.f; o1[r] = 0.f; c0[r] = 0.f; c1[r] = 0.f; }
    float m_ref = -INFINITY, m_thr = -INFINITY, l_run = 0.f;    // m_thr = m_ref + AT_TAU, kept so that the sum is formed where m_ref moves (the cold branch)
    AT_PROF_INIT();

    const int sr = tid >> 4, sc4 = (tid & 15) * 4;
    const unsigned rowb = (unsigned)ld * 4u;
    const unsigned span = nk > 0 ? (unsigned)(nk - 1) * rowb + AT_D * 4u : 0u;
    const __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc((void *)(Kp + (size_t)bk * N * ld + h * AT_D), 0, (int)span, MFR_RSRC_FLAGS);
    const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc((void *)(Vp + (size_t)bk * N * ld + h * AT_D), 0, (int)span, MFR_RSRC_FLAGS);
    const unsigned koff = (unsigned)sr * rowb + 4u * (unsigned)sc4, voff = 4u * (unsigned)lane;
    const int ntiles = (nk + AT_KT - 1) / AT_KT;
    float4 kr;
    float v0, v1, v2, v3;
    auto gload_k = [&](int t) { kr = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rk, koff, (unsigned)(t * AT_KT) * rowb, 0)); };
    auto gload_v = [&](int t) {
        const unsigned sv = (unsigned)(t * AT_KT + 4 * wid) * rowb;
        v0 = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rv, voff, sv, 0));
        v1 = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rv, voff, sv + rowb, 0));
        v2 = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rv, voff, sv + 2u * rowb, 0));
        v3 = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rv, voff, sv + 3u * rowb, 0));
    };
    auto lstore_k = [&](int buf) {
        unsigned w[NT][2];
        AR::split2(kr.x, kr.y, [&](int k) -> unsigned & { return w[k][0]; }); AR::split2(kr.z, kr.w, [&](int k) -> unsigned & { return w[k][1]; });
        *(uint2 *)&Ks[buf][0][sr][sc4] = make_uint2(w[0][0], w[0][1]); *(uint2 *)&Ks[buf][1][sr][sc4] = make_uint2(w[1][0], w[1][1]);
        if constexpr (NT == 3) *(uint2 *)&Ks[buf][2][sr][sc4] = make_uint2(w[2][0], w[2][1]);
    };
    auto lstore_v = [&](int buf) {
        unsigned w[NT][2];
        AR::split2(v0, v1, [&](int k) -> unsigned & { return w[k][0]; }); AR::split2(v2, v3, [&](int k) -> unsigned & { return w[k][1]; });
        const int p0 = 16 * (wid >> 2) + 8 * (wid & 1) + 4 * ((wid >> 1) & 1);
        *(uint2 *)&Vt[buf][0][lane][p0] = make_uint2(w[0][0], w[0][1]); *(uint2 *)&Vt[buf][1][lane][p0] = make_uint2(w[1][0], w[1][1]);
        if constexpr (NT == 3) *(uint2 *)&Vt[buf][2][lane][p0] = make_uint2(w[2][0], w[2][1]);
    };
    const unsigned short *kq0 = &Ks[0][0][ql][8 * half], *vq0 = &Vt[0][0][ql][8 * half];
    // the NT term fragments of S^T's step st from the K stage at kq / the 2 NT fragments of 16 keys of V^T (term k: f[2k] / f[2k+1] = channels 0-31 / 32-63).
    // Written out per term, as the LDS stores above: a loop over k < NT is unrolled only after the addresses were formed, and the stores lose their alignment.
#define AT_KLOAD(f, kq, st) do { f[0].q = *(const uint4 *)((kq) + 16 * (st)); f[1].q = *(const uint4 *)((kq) + AT_KT * AB_KS + 16 * (st)); \
        if constexpr (NT == 3) f[2].q = *(const uint4 *)((kq) + 2 * AT_KT * AB_KS + 16 * (st)); } while (0)
#define AT_VLOAD(f, vq, st) do { \
        f[0].q = *(const uint4 *)((vq) + 16 * (st)); f[1].q = *(const uint4 *)((vq) + 32 * AB_VS + 16 * (st)); \
        f[2].q = *(const uint4 *)((vq) + AT_D * AB_VS + 16 * (st)); f[3].q = *(const uint4 *)((vq) + AT_D * AB_VS + 32 * AB_VS + 16 * (st)); \
        if constexpr (NT == 3) { f[4].q = *(const uint4 *)((vq) + 2 * AT_D * AB_VS + 16 * (st)); f[5].q = *(const uint4 *)((vq) + 2 * AT_D * AB_VS + 32 * AB_VS + 16 * (st)); } } while (0)
    // one MFMA, then up to nv VALU, nm times (sched_group_barrier); only where the arithmetic asks for it
#define AT_WEAVE(nm, nv) do { if constexpr (AR::WEAVE) { _Pragma("unroll") for (int w_ = 0; w_ < (nm); ++w_) { \
        __builtin_amdgcn_sched_group_barrier(0x8, 1, 0); __builtin_amdgcn_sched_group_barrier(0x2, (nv), 0); } } } while (0)
#define AT_QK(kf, qf, s, s2) do { if constexpr (NT == 3) AT_BF16X3_QK(kf, qf, s, s2); else AT_F16X2_QK(kf, qf, s, s2); } while (0)
#define AT_PV(vf, pf) do { if constexpr (NT == 3) AT_BF16X3_PV(vf, pf, o0, o1); else AT_F16X2_PV(vf, pf, o0, o1, c0, c1); } while (0)
    // eight probabilities p[o .. o+7] -> word j of each term's fragment = the pair (2j, 2j+1); AR::P_COPY: see AtBf16x3
#define AT_SPLIT_P(pf, o) do { if constexpr (AR::P_COPY) { \
            float pp_[8]; \
            _Pragma("unroll") for (int j_ = 0; j_ < 8; ++j_) pp_[j_] = p[(o) + j_]; \
            _Pragma("unroll") for (int j_ = 0; j_ < 4; ++j_) AR::split2(pp_[2 * j_], pp_[2 * j_ + 1], [&](int k) -> unsigned & { return pf[k].u[j_]; }); \
        } else { \
            _Pragma("unroll") for (int j_ = 0; j_ < 4; ++j_) AR::split2(p[(o) + 2 * j_], p[(o) + 2 * j_ + 1], [&](int k) -> unsigned & { return pf[k].u[j_]; }); \
        } } while (0)
#define AT_FOLD_SCORES(sc, s, s2) do { _Pragma("unroll") for (int r_ = 0; r_ < 16; ++r_) sc[r_] = AR::fold(s[r_], s2[r_]); } while (0)

    f32x16 sc;                                              // the scores of the tile whose softmax is due
    gload_k(0); gload_v(0); lstore_k(0); lstore_v(0);       // (tiles beyond nk: zeros)
    gload_k(1); lstore_k(1);
    gload_k(2); gload_v(1);                                 // staged during iteration 0
    __syncthreads();
    {
        f32x16 s, s2;
#pragma unroll
        for (int r = 0; r < 16; ++r) { s[r] = 0.f; s2[r] = 0.f; }
        if (ntiles > 0) {
#pragma unroll
            for (int st = 0; st < 4; ++st) { Frag8 kf[NT]; AT_KLOAD(kf, kq0, st); AT_QK(kf, qf[st], s, s2); }
        }
        AT_FOLD_SCORES(sc, s, s2);
    }
    __syncthreads();                                        // K stage 0 is rewritten during iteration 0

    // The last iteration multiplies a K stage of zeros (tile ntiles does not exist) and stages tiles that are never used: one basic block per
    // chunk, so that the MFMAs and the VALU work can be woven together, is worth more than the MFMAs it wastes.
    for (int t = 0; t < ntiles; ++t) {
        const int buf = t & 1;
        const unsigned short *kq = kq0 + (buf ^ 1) * (NT * AT_KT * AB_KS);
        const unsigned short *vq = vq0 + buf * (NT * AT_D * AB_VS);
        f32x16 s, s2;
#pragma unroll
        for (int r = 0; r < 16; ++r) { s[r] = 0.f; s2[r] = 0.f; }
        Frag8 ka[NT], kb2[NT];
        AT_KLOAD(ka, kq, 0);
        AT_KLOAD(kb2, kq, 1);
        const int kb = t * AT_KT + 4 * half;
        if ((t + 1) * AT_KT > nk) {                         // only the last tile can hold keys >= nk (wave-uniform branch)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (kb + (r & 3) + 8 * (r >> 2) >= nk) sc[r] = -INFINITY;
        }
        // ---- S^T(t+1), step 0  ||  softmax(t): row maximum
        AT_QK(ka, qf[0], s, s2);
        AT_KLOAD(ka, kq, 2);
        float mx = sc[0];
#pragma unroll
        for (int r = 1; r < 15; r += 2) mx = fmaxf(fmaxf(mx, sc[r]), sc[r + 1]);
        mx = fmaxf(mx, sc[15]);
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const bool need = mx > m_thr;                       // (tile 0: m_thr = -inf, true wherever mx is finite; a NaN mx: false, and p below is NaN)
        const float m_use = need ? mx : m_ref;
        AT_PROF_TILE(mx);
        AT_WEAVE(6, 2);
        __builtin_amdgcn_sched_barrier(0);
        // ---- step 1  ||  exponentials of keys 0 .. 7
        AT_QK(kb2, qf[1], s, s2);
        AT_KLOAD(kb2, kq, 3);
        float p[16];
        at_f2 rs2; rs2.x = 0.f; rs2.y = 0.f;
        at_f2 mm; mm.x = m_use; mm.y = m_use;
#pragma unroll
        for (int r = 0; r < 8; r += 2) {
            at_f2 d; d.x = sc[r]; d.y = sc[r + 1];
            d = d - mm;
            at_f2 e; e.x = __builtin_amdgcn_exp2f(d.x); e.y = __builtin_amdgcn_exp2f(d.y);
            rs2 += e;
            p[r] = e.x; p[r + 1] = e.y;
        }
        AT_WEAVE(6, 3);
        __builtin_amdgcn_sched_barrier(0);
        // ---- step 2  ||  exponentials of keys 8 .. 15
        AT_QK(ka, qf[2], s, s2);
#pragma unroll
        for (int r = 8; r < 16; r += 2) {
            at_f2 d; d.x = sc[r]; d.y = sc[r + 1];
            d = d - mm;
            at_f2 e; e.x = __builtin_amdgcn_exp2f(d.x); e.y = __builtin_amdgcn_exp2f(d.y);
            rs2 += e;
            p[r] = e.x; p[r + 1] = e.y;
        }
        float rs = rs2.x + rs2.y;
        rs += __shfl_xor(rs, 32, 64);
        AT_WEAVE(6, 3);
        __builtin_amdgcn_sched_barrier(0);
        if (__ballot(need) != 0ull) {                       // the reference moved for some query of this wavefront (cold): rescale; alpha = 1 in the other lanes
            const float alpha = __builtin_amdgcn_exp2f(m_ref - m_use);
            m_thr = m_use + AT_TAU;
            AT_PROF_RESCALED();
            l_run *= alpha;
#pragma unroll
            for (int r = 0; r < 16; ++r) { o0[r] *= alpha; o1[r] *= alpha; c0[r] *= alpha; c1[r] *= alpha; }
        }
        l_run += rs;
        m_ref = m_use;
        // ---- step 3  ||  split of P (first 16 keys), staging of K(t+2) / V(t+1)
        AT_QK(kb2, qf[3], s, s2);
        Frag8 va[2 * NT];
        AT_VLOAD(va, vq, 0);
        Frag8 pf0[NT];
        AT_SPLIT_P(pf0, 0);
        lstore_k(buf); lstore_v(buf ^ 1);
        gload_k(t + 3); gload_v(t + 2);
        AT_WEAVE(6, 14);
        __builtin_amdgcn_sched_barrier(0);
        // ---- O^T += V^T P: keys 0 .. 15  ||  split of P (last 16 keys); then keys 16 .. 31
        AT_PV(va, pf0);
        Frag8 vb[2 * NT];
        AT_VLOAD(vb, vq, 1);
        Frag8 pf1[NT];
        AT_SPLIT_P(pf1, 8);
        AT_WEAVE(12, 4);
        __builtin_amdgcn_sched_barrier(0);
        AT_PV(vb, pf1);
        AT_FOLD_SCORES(sc, s, s2);
        __syncthreads();
    }
#undef AT_FOLD_SCORES
#undef AT_SPLIT_P
#undef AT_PV
#undef AT_QK
#undef AT_WEAVE
#undef AT_VLOAD
#undef AT_KLOAD
    AT_PROF_COMMIT(ntiles);

    if (q < N) {
        const float inv = (l_run > 0.f && q < nq) ? 1.f / l_run : 0.f;
        float *op = O + ((size_t)b * N + q) * ldo + h * AT_D + 4 * half;
        if constexpr (AR::GUARD) {
            if (guard) {
                // range guard (guard.h): an out-of-range q / k row turns the row's scores, hence its probabilities and its whole output row, into NaN; an
                // out-of-range v[n, d] turns column d of every row into NaN -- so every accumulator is tested, before the normalisation (inv = 0 for a NaN sum)
                float chk = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) { MFR_GUARD_ACC(chk, o0[r]); MFR_GUARD_ACC(chk, c0[r]); MFR_GUARD_ACC(chk, o1[r]); MFR_GUARD_ACC(chk, c1[r]); }
                MFR_GUARD_ACC(chk, l_run);
                if (chk != chk) atomicOr(guard, 1);        // (rows >= N of the last block do not reach this point: per-lane test)
            }
        }
        if constexpr (NO == 2) {
#pragma unroll
            for (int r = 0; r < 16; ++r) { o0[r] = AR::fold(o0[r], c0[r]); o1[r] = AR::fold(o1[r], c1[r]); }
        }
        at_store_normalised(op, o0, o1, inv);
    }
}

__global__ void __launch_bounds__(512, 1) sg_attention_bf16x3_p_kernel(
    const float *__restrict__ Q, const float *__restrict__ Kp, const float *__restrict__ Vp, int ld,
    int N, int heads, int B2, const int *__restrict__ n_tok, int cross, float scale_log2e, float *__restrict__ O, int ldo AT_PROF_DECL)
{
    sg_attention_split_p<AtBf16x3>(Q, Kp, Vp, ld, N, heads, B2, n_tok, cross, scale_log2e, O, ldo, nullptr AT_PROF_PASS);
}

__global__ void __launch_bounds__(512, 1) sg_attention_f16x2_p_kernel(
    const float *__restrict__ Q, const float *__restrict__ Kp, const float *__restrict__ Vp, int ld,
    int N, int heads, int B2, const int *__restrict__ n_tok, int cross, float scale_log2e, float *__restrict__ O, int ldo, int *guard AT_PROF_DECL)
{
    sg_attention_split_p<AtF16x2>(Q, Kp, Vp, ld, N, heads, B2, n_tok, cross, scale_log2e, O, ldo, guard AT_PROF_PASS);
}

extern "C" {

#ifdef AT_PROF
// the counters of the launches since the last call, [AT_PROF_SLOTS][3] = (tiles, rescaled, rescaled with a running-maximum reference), and their number; clears both
int mfr_sg_attention_profile(unsigned *out_host, int *launches)
{
    static const unsigned zero[AT_PROF_SLOTS][3] = {};
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpyFromSymbol(out_host, HIP_SYMBOL(at_prof), sizeof(zero), 0, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpyToSymbol(HIP_SYMBOL(at_prof), zero, sizeof(zero), 0, hipMemcpyHostToDevice) != hipSuccess) return MFR_E_LAUNCH;
    *launches = at_prof_launches;
    at_prof_launches = 0;
    return 0;
}
#endif

// q,k,v: [B2, N, ld] fp32 (row = keypoint; channels of head h at [h*64, h*64+64) from the given base
// pointers, so a fused [.., 768] qkv buffer is passed as base, base+256, base+512 with ld = 768).
// out: [B2, N, ldo].  cross != 0: image b attends to image b^1 (the other image of its pair).
// variant: 0 = f16x2, 256 queries per workgroup, score product one tile ahead of the softmax (default); 1 = exact-fp32 matrix instruction
// (128 queries per workgroup); 2 = bf16x3, otherwise as 0
int mfr_sg_attention_variant(const float *q, const float *k, const float *v, int ld, int B2, int N, int heads,
                             const int32_t *n_tok, int cross, float *out, int ldo, int variant, void *stream)
{
    if (!q || !k || !v || !n_tok || !out || B2 <= 0 || N <= 0 || heads <= 0 || (ld & 3) || (ldo & 3)) return MFR_E_ARG;
    if (cross && (B2 & 1)) return MFR_E_ARG;
    if (variant < 0 || variant > 2) return MFR_E_ARG;
    // the buffer descriptors of variants 0 / 2 address an (image, head)'s rows with 32-bit offsets
    if (variant != 1 && (size_t)N * ld * 4 >= 0x7fffffffull) variant = 1;
    const float scale_log2e = 1.4426950408889634f / 8.0f;          // log2(e) / sqrt(64)
    if (variant != 1) {
        const int nqb = (N + AT_QW * AB_WAVES - 1) / (AT_QW * AB_WAVES);
        if (variant == 0)
            hipLaunchKernelGGL(sg_attention_f16x2_p_kernel, dim3(nqb * heads * B2), dim3(512), 0, (hipStream_t)stream, q, k, v, ld, N, heads, B2, n_tok, cross,
                               scale_log2e, out, ldo, mfr_guard_current() AT_PROF_NEXT);
        else
            hipLaunchKernelGGL(sg_attention_bf16x3_p_kernel, dim3(nqb * heads * B2), dim3(512), 0, (hipStream_t)stream, q, k, v, ld, N, heads, B2, n_tok, cross,
                               scale_log2e, out, ldo AT_PROF_NEXT);
    } else {
        const int nqb = (N + AT_QW * AT_WAVES - 1) / (AT_QW * AT_WAVES);
        hipLaunchKernelGGL(sg_attention_kernel, dim3(nqb * heads * B2), dim3(256), 0, (hipStream_t)stream, q, k, v, ld, N, heads, B2, n_tok, cross,
                           scale_log2e, out, ldo);
    }
    CHECK_LAUNCH();
    return 0;
}

int mfr_sg_attention(const float *q, const float *k, const float *v, int ld, int B2, int N, int heads,
                     const int32_t *n_tok, int cross, float *out, int ldo, void *stream)
{
    return mfr_sg_attention_variant(q, k, v, ld, B2, N, heads, n_tok, cross, out, ldo, 0, stream);
}

}  // extern "C"
