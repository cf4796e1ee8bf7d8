// wave_dev.h -- the wavefront (64 lanes) and workgroup primitives the kernels share, plus the host-side pieces every TU needs
// (CHECK_LAUNCH, align_up and the workspace carver, the raw-buffer descriptor word).  gfx950.
//
// ONE definition of each: the solvers equal the CPU oracle bit for bit and the matchers compare values for equality between their row and
// their column side, so two copies of a reduction that drift apart are a wrong result, not a style problem.
//
// Floating-point contract: an inline function takes the -ffp-contract mode of the TU that includes it (csrc/Makefile: solver and matcher
// TUs off, NN-kernel TUs fast).  The reductions, the compaction and load4 hold no a * b + c, so they mean the same in both; the precise
// log-sum-exp does (see there).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/mfr_hip.h"

#define MFR_DEV static __device__ __forceinline__
#define MFR_DEV_NOINLINE static __device__ __noinline__

// ---------------------------------------------------------------- host side
#define CHECK_LAUNCH() do { if (hipGetLastError() != hipSuccess) return MFR_E_LAUNCH; } while (0)
// dword 3 of a raw buffer descriptor on gfx9-family CDNA (32-bit data format): out-of-range reads return 0 (how the convolutions produce
// their zero padding: padded taps get an offset beyond the buffer) and out-of-range writes are dropped
#define MFR_RSRC_FLAGS 0x00020000

namespace mfr {

static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// a workspace as consecutive 256-byte-aligned arrays.  A solver states its layout ONCE, as the takes of one function: run on a null
// base it sizes the workspace (`off` after the last take), run on the caller's buffer it hands out the same pointers
struct WsCarver {
    char *base;
    size_t off = 0;
    explicit WsCarver(void *b) : base((char *)b) {}
    template <class T> T *take(size_t count)
    {
        T *p = base ? (T *)(base + off) : nullptr;
        off = align_up(off + sizeof(T) * count, 256);
        return p;
    }
};

MFR_DEV int lane_id() { return (int)(threadIdx.x & 63); }

// ---------------------------------------------------------------- xor butterfly 32, 16, 8, 4, 2, 1
// every lane ends with the same bits (a + b == b + a, max likewise).  wave_sum(double) is the order the CPU oracle restates for the
// solvers' sums over points: do not reorder.
MFR_DEV double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
    return v;
}
MFR_DEV float wave_sum(float v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
    return v;
}
MFR_DEV float wave_max(float v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}
// comparisons only (`if (o < v) v = o`, no fminf): the same value in every lane; a NaN never passes the test, so it is skipped like in the
// sequential loop, unless it is the lane's own start value
MFR_DEV float wave_min(float v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float o = __shfl_xor(v, off, 64);
        if (o < v) v = o;
    }
    return v;
}

// arg-max over the wavefront: the larger value wins, equal values give the LOWER index (comparisons only: the same answer in every lane
// whatever the pairing order).  `best` is not NaN: the callers build it with `x > best` from -inf / -1, which a NaN never passes
MFR_DEV void wave_argmax(float &best, int &idx)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float ob = __shfl_xor(best, off, 64); const int oi = __shfl_xor(idx, off, 64);
        if (ob > best || (ob == best && oi < idx)) { best = ob; idx = oi; }
    }
}

// ---------------------------------------------------------------- DPP / permlane max and sum
// wavefront-wide max / sum that leave the SAME bits in all 64 lanes (every step pairs two groups and a + b == b + a): DPP inside a row of
// 16 lanes (quad_perm xor 1, xor 2, row_half_mirror, row_mirror), then gfx950's v_permlane16_swap / v_permlane32_swap across rows and halves
// (two copies of x go in; one comes back holding the even rows' / lower half's values everywhere, the other the odd rows' / upper half's) --
// no LDS round trip.  Inline asm: the builtin, given the same value twice, was compiled to x + x (hipcc 7.2).
// The lanes are paired in another order than in the butterfly above, so wave_sum_dpp(x) and wave_sum(x) may differ in the last bits: a
// kernel family picks one and keeps it.
MFR_DEV void wave_swap16(float &a, float &b) { asm("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b)); }
MFR_DEV void wave_swap32(float &a, float &b) { asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b)); }
template <int CTRL> MFR_DEV float wave_dpp(float x)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xf, 0xf, false));
}
MFR_DEV float wave_max_dpp(float x)
{
    x = fmaxf(x, wave_dpp<0xB1>(x)); x = fmaxf(x, wave_dpp<0x4E>(x)); x = fmaxf(x, wave_dpp<0x141>(x)); x = fmaxf(x, wave_dpp<0x140>(x));
    float y = x; wave_swap16(x, y); x = fmaxf(x, y);
    y = x; wave_swap32(x, y); x = fmaxf(x, y);
    return x;
}
MFR_DEV float wave_sum_dpp(float x)
{
    x += wave_dpp<0xB1>(x); x += wave_dpp<0x4E>(x); x += wave_dpp<0x141>(x); x += wave_dpp<0x140>(x);
    float y = x; wave_swap16(x, y); x += y;
    y = x; wave_swap32(x, y); x += y;
    return x;
}

// ---------------------------------------------------------------- ordered compaction, one workgroup of 256 threads
// compact256_slot gives every thread whose `valid` is set its output slot: slots follow thread order within a call and call order across
// calls, i.e. the order of a sequential `if (valid) out[n++] = ..`.  `total` is the thread's running count (start it at 0): on return it
// includes this call's survivors, in EVERY thread.  All 256 threads (4 wavefronts, 1-D block) must make the call together; two barriers
// per call (the counts are read between them, so the next call may overwrite them).
//     __shared__ Compact256 cs;  int total = 0;
//     for (start = 0; start < n; start += 256) { valid = ..; const int o = compact256_slot(cs, valid, total); if (valid) out[o] = ..; }
//     if (threadIdx.x == 0) n_out[b] = total;
struct Compact256 { int wave_cnt[4]; };
MFR_DEV int compact256_slot(Compact256 &c, bool valid, int &total)
{
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(valid);
    if (lane == 0) c.wave_cnt[wid] = __popcll(bal);
    __syncthreads();
    int slot = total + __popcll(bal & ((1ull << lane) - 1ull));
    for (int w = 0; w < wid; ++w) slot += c.wave_cnt[w];
    total += c.wave_cnt[0] + c.wave_cnt[1] + c.wave_cnt[2] + c.wave_cnt[3];
    __syncthreads();
    return slot;
}

// one wavefront's step of a sequential `if (in) idx[m++] = i`: the lanes whose `in` is set append their `i` in lane order; `m` (wave-uniform)
// advances by their number.  A later read of idx[] by other lanes needs a __threadfence() first.
MFR_DEV void wave_compact_append(bool in, int i, int32_t *__restrict__ idx, int &m)
{
    const unsigned long long bal = __ballot(in);
    if (in) idx[m + __popcll(bal & ((1ull << lane_id()) - 1ull))] = i;
    m += __popcll(bal);
}

// ---------------------------------------------------------------- precise online log-sum-exp
// (max, sum of exp(x - max)) with libm's expf, the textbook two-case update; an empty partial (m = -inf) merges to nothing.
// a.s * expf(..) + s CAN contract into an fma: every user today (loftr.hip, loftr_ot.hip) is built with -ffp-contract=off, and their
// four-sweep and tiled variants are compared against each other, so a TU built with contraction must not start using these.
// (superglue_match.hip keeps its own branch-free __expf / fmaf form: different arithmetic, different name.)
struct LsePrecise { float m, s; };
MFR_DEV void lse_precise_add(LsePrecise &a, float x)
{
    if (x > a.m) { a.s = a.s * expf(a.m - x) + 1.f; a.m = x; }
    else a.s = a.s + expf(x - a.m);
}
MFR_DEV void lse_precise_merge(LsePrecise &a, float m, float s)
{
    if (m == -INFINITY) return;
    if (m > a.m) { a.s = a.s * expf(a.m - m) + s; a.m = m; }
    else a.s = a.s + s * expf(m - a.m);
}
// the 64 lanes' partials merged in the xor butterfly: every lane ends with the wavefront's (m, s)
MFR_DEV void lse_precise_wave_merge(LsePrecise &a)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float om = __shfl_xor(a.m, off, 64), os = __shfl_xor(a.s, off, 64);
        lse_precise_merge(a, om, os);
    }
}

// ---------------------------------------------------------------- 4 adjacent row elements
// x[k] = p[j0 + k] for k < nval, `fill` beyond; one 16-byte load when all four exist and the caller vouches for the alignment (vec)
MFR_DEV void load4(const float *__restrict__ p, int j0, int nval, bool vec, float fill, float x[4])
{
    if (nval == 4 && vec) {
        const float4 t = *(const float4 *)(p + j0);
        x[0] = t.x; x[1] = t.y; x[2] = t.z; x[3] = t.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = k < nval ? p[j0 + k] : fill;
    }
}

}  // namespace mfr
