"""-m gpu: the split attention kernels' STALE softmax reference (csrc/attention.hip, AT_TAU): the accumulators are rescaled only when a tile's maximum
exceeds the per-query reference by more than TAU = 14 (log2 units), so the probabilities reach 2^TAU instead of 1.  Random inputs hardly ever take
that branch after the first tiles and never come near 2^TAU, so the scores here are BUILT: q and k carry one non-zero channel per head,

    q[i, h, ch_h] = u_i * 8 / log2(e),  k[j, h, ch_h] = c_j     ->     s_ij * log2(e) / 8 = u_i * c_j   (the kernel's exponent, in log2 units),

and every case first checks on the CPU, in float64 and from the float32 tensors the device gets, that the scores are what the case needs.
Bars, the same for every case (tests/test_gpu_nets_parity.py): a float64 softmax at rtol 1e-4 / atol 2e-5, and the split kernel's error (max and
rms) <= 1.5 x the exact-fp32 kernel's (variant 1, which keeps the running maximum as its reference) on the same input; B2 = 2, 4 heads, variants 0
(f16x2) and 2 (bf16x3), self and cross.  The staircases END near 0: the keys that carry the softmax then have small scores, so the error measured
is the kernels' and not the fp32 rounding of a score of 64."""
import numpy as np
import pytest
import torch

from mapfree_reloc_amd import _lib, options
from mapfree_reloc_amd.pipeline import RangeGuard

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAU = 14.0                      # csrc/attention.hip AT_TAU
LOG2E = 1.4426950408889634
B2, HEADS = 2, 4
_CH = [(5 + 17 * h) % 64 for h in range(HEADS)]          # the non-zero channel of head h


def _build(u, c, v):
    """u [B2, K] query factors, c [B2, HEADS, K] key values, v [B2, K, 256] -> qkv [B2, K, 768] float32"""
    K = u.shape[1]
    qkv = torch.zeros(B2, K, 768, dtype=torch.float64)
    for h in range(HEADS):
        qkv[:, :, 64 * h + _CH[h]] = u * (8.0 / LOG2E)
        qkv[:, :, 256 + 64 * h + _CH[h]] = c[:, h]
    qkv[:, :, 512:] = v
    return qkv.float()


def _scores_log2(qkv, b, bk):
    """[HEADS, K, K] float64: the exponents the kernel forms for image b attending to image bk"""
    K = qkv.shape[1]
    q, k = qkv[b, :, :256].double().view(K, HEADS, 64), qkv[bk, :, 256:512].double().view(K, HEADS, 64)
    return torch.einsum("nhd,mhd->hnm", q, k) * (LOG2E / 8.0)


def _tile_max(s, nk):
    """[HEADS, K, ntiles]: maximum of every 32-key tile over the keys < nk"""
    return torch.stack([s[:, :, t:min(t + 32, nk)].max(-1).values for t in range(0, nk, 32)], -1)


def _reference(qkv, n, cross):
    """float64 softmax per image: [nq, 256], zeros where the key image is empty"""
    K = qkv.shape[1]
    q, k, v = [t.double().view(B2, K, HEADS, 64) for t in qkv.split(256, -1)]
    want = []
    for b in range(B2):
        bk = b ^ 1 if cross else b
        nq, nk = n[b], n[bk]
        s = torch.einsum("nhd,mhd->hnm", q[b, :nq], k[bk, :nk]) / 8.0
        want.append(torch.einsum("hnm,mhd->nhd", s.softmax(-1), v[bk, :nk]).reshape(nq, 256))
    return want


def _rows(K, spread=0.01):
    """query factors 1 .. 1 + spread: every query meets the same staircase, stretched a little, so that the rows are not copies of each other"""
    i = torch.arange(K, dtype=torch.float64)
    return torch.stack([1.0 + spread * ((i + 3 * b) % 8) / 7.0 for b in range(B2)])


def _staircase(K, step, peak_first, n=(None, None)):
    """c [B2, HEADS, K]: tile t's maximum is step * (t - last tile) + 0.25 h, at key 0 of the tile (peak_first) or at key (7 t + 3) % 32; the other
    keys of a tile lie 1/8 .. 3 below it, in a seeded pattern that differs per image and head.  `last tile` is the last one that holds a key < n[b] of
    ITS image (the keys that carry the softmax have small scores whatever the count); the keys beyond n[b] climb on: a mask that let one through
    would hand it the whole softmax"""
    g = torch.Generator().manual_seed(int(step * 100) + K)
    c = torch.empty(B2, HEADS, K, dtype=torch.float64)
    for b in range(B2):
        nt = ((n[b] or K) + 31) // 32
        for h in range(HEADS):
            below = torch.randint(1, 25, (K,), generator=g).double() / 8.0
            for t in range((K + 31) // 32):
                below[min(32 * t + (0 if peak_first else (7 * t + 3) % 32), K - 1)] = 0.0
            c[b, h] = step * (torch.arange(K) // 32 - (nt - 1)).double() + 0.25 * h - below
    return c


def _values(K, seed, bits=24):
    """v ~ N(0, 1); bits < 24: significands cut to `bits` bits"""
    v = torch.randn(B2, K, 256, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).float()
    return (v.view(torch.int32) & (-1 << (24 - bits))).view(torch.float32).double()


def _case_stairs_over(cross):
    """five tiles, every tile's maximum TAU + 2 above the previous one (x the query factor): the reference moves in every tile"""
    K = 160
    qkv = _build(_rows(K), _staircase(K, TAU + 2.0, False), _values(K, 1))
    for b in range(B2):
        tm = _tile_max(_scores_log2(qkv, b, b ^ 1 if cross else b), K)
        assert tm.shape[-1] == 5 and ((tm[..., 1:] - tm[..., :-1]) > TAU + 1.9).all()
    return qkv, [K, K]


def _case_stairs_under(cross):
    """five tiles, every tile's maximum TAU - 0.25 above the previous one: no tile exceeds its predecessor by TAU, yet the true maximum ends
    4 (TAU - 0.25) above tile 0's -- a reference compared tile against tile would never move and p would reach 2^55; the reference has to move when the
    CUMULATIVE gap passes TAU (tiles 2 and 4).  Query factors 1 .. 1.01: the largest step is 13.89 < TAU"""
    K = 160
    qkv = _build(_rows(K), _staircase(K, TAU - 0.25, False), _values(K, 2))
    for b in range(B2):
        tm = _tile_max(_scores_log2(qkv, b, b ^ 1 if cross else b), K)
        d = tm[..., 1:] - tm[..., :-1]
        assert (d < TAU - 0.1).all() and (d > TAU - 0.3).all() and ((tm[..., 2] - tm[..., 0]) > TAU + 13.0).all() and ((tm[..., 4] - tm[..., 0]) > 4 * (TAU - 0.26)).all()
    return qkv, [K, K]


def _case_largest_p(cross):
    """tile 0's maximum is exactly 0 (a key with c = 0), every other key lies 1/8 .. 3 below 0, and ONE key of tile 1 sits at TAU - 0.01 for the largest
    query factor (13.85 .. 13.99 over the rows): the reference stays at 0, that key's p is 2^13.99 ~ 16270 -- f16x2's high term near 2^14 and its low
    term (p - ph) 2^11 -- and its row of v holds +-5.7e4 .. 6.3e4 (|v| <= 65504 is f16x2's range, 6e4 the largest decade inside it)"""
    K = 64
    g = torch.Generator().manual_seed(3)
    u = _rows(K)
    c = -torch.randint(1, 25, (B2, HEADS, K), generator=g).double() / 8.0
    v = _values(K, 3)
    for b in range(B2):
        for h in range(HEADS):
            c[b, h, (5 * h + b) % 32] = 0.0
            c[b, h, 40 + h] = (TAU - 0.01) / float(u.max())
        for h in range(HEADS):
            big = 6.0e4 * (1.0 + 0.09 * (torch.rand(64, generator=g, dtype=torch.float64) - 0.5))
            v[b, 40 + h, 64 * h:64 * h + 64] = big * (1.0 - 2.0 * torch.randint(0, 2, (64,), generator=g).double())
    qkv = _build(u, c, v)
    for b in range(B2):
        s = _scores_log2(qkv, b, b ^ 1 if cross else b)
        assert (_tile_max(s, K)[..., 0] == 0).all()
        for h in range(HEADS):
            top = s[h, :, 40 + h]
            assert (top < TAU - 0.009).all() and (top > TAU - 0.16).all() and float(top.max()) > TAU - 0.0101
            assert (s[h, :, 32:].max(-1).values == top).all()
    assert float(qkv[..., 512:].abs().max()) < 65504.0
    return qkv, [K, K]


def _case_one_lane(cross):
    """wavefront 1 (queries 32 .. 63): one query per head has factor 1, every other query of the image 0 -- flat scores, a uniform softmax.  All keys are
    0 except three keys of tile 2 at TAU + 3: that one lane's reference moves in tile 2 (the wavefront takes the branch), its 31 neighbours' alpha is 1"""
    K = 160
    u = torch.zeros(B2, K, dtype=torch.float64)
    c = torch.zeros(B2, HEADS, K, dtype=torch.float64)
    for b in range(B2):
        u[b, 37 + 9 * b] = 1.0
        for h in range(HEADS):
            c[b, h, [64 + h, 75 + b, 95 - 2 * h]] = TAU + 3.0
    qkv = _build(u, c, _values(K, 4))
    for b in range(B2):
        tm = _tile_max(_scores_log2(qkv, b, b ^ 1 if cross else b), K)
        jump = tm[..., 2] - tm[..., :2].max(-1).values
        hot = torch.zeros(K, dtype=torch.bool); hot[37 + 9 * b] = True
        assert (jump[:, hot] > TAU + 2.99).all() and (tm[:, ~hot] == 0).all() and (tm[:, hot][..., [0, 1, 3, 4]] == 0).all()
    return qkv, [K, K]


def _case_counts(K, n):
    def make(cross):
        """the staircase with a step above TAU and each tile's maximum at the tile's first key, so that a last tile of one key (33, 65) still moves the
        reference while its other 31 keys are masked.  A row with one key (n_tok = 1), or with a last tile of one key a step above the rest, is
        one-hot: the exact-fp32 kernel returns that key's v with NO error, a split kernel v as its operand terms hold it -- f16x2: 22 bits, half an
        ulp short (split_f16.h), a figure the cases above measure on spread rows -- and 1.5 x 0 bounds nothing.  So v has 16-bit significands here,
        exact in both splits, and the ratio compares what these cases are about: the mask and the moving reference"""
        qkv = _build(_rows(K), _staircase(K, TAU + 2.0, True, n), _values(K, 5, bits=16))
        for b in range(B2):
            nk = n[b ^ 1 if cross else b]
            tm = _tile_max(_scores_log2(qkv, b, b ^ 1 if cross else b), nk)
            assert tm.shape[-1] == (nk + 31) // 32 and ((tm[..., 1:] - tm[..., :-1]) > TAU + 1.9).all()
        return qkv, list(n)
    return make


_CASES = {"stairs_over": _case_stairs_over, "stairs_under": _case_stairs_under, "largest_p": _case_largest_p, "one_lane": _case_one_lane}
for _K in (33, 65):
    for _n in ((1, 32), (32, 33), (33, _K)):
        _CASES[f"counts_K{_K}_n{_n[0]}_{_n[1]}"] = _case_counts(_K, _n)
_cache = {}


def _run(qkv, n_tok, cross, variant):
    lib = _lib.load()
    K = qkv.shape[1]
    out = torch.full((B2, K, 256), float("nan"), device=DEV)          # every row must be written
    base = qkv.data_ptr()
    _lib.check(lib.mfr_sg_attention_variant(base, base + 256 * 4, base + 512 * 4, 768, B2, K, HEADS, n_tok.data_ptr(), 1 if cross else 0,
                                            out.data_ptr(), 256, variant, _lib.stream_ptr()), "mfr_sg_attention")
    return out


def _error(got, want, n):
    e = torch.cat([got[b, :n[b]].double() - want[b] for b in range(B2)])
    return float(e.abs().max()), float(e.pow(2).mean().sqrt())


def _case(name, cross):
    """inputs, the float64 reference and the exact-fp32 kernel's error of one case: built once, shared by both split variants, never modified"""
    if (name, cross) not in _cache:
        qkv, n = _CASES[name](cross)
        want = _reference(qkv, n, cross)
        qd, nd = qkv.to(DEV), torch.tensor(n, dtype=torch.int32, device=DEV)
        _cache[name, cross] = (qd, nd, n, want, _error(_run(qd, nd, cross, 1).cpu(), want, n))
    return _cache[name, cross]


@pytest.mark.parametrize("variant", [0, 2])
@pytest.mark.parametrize("cross", [False, True])
@pytest.mark.parametrize("name", list(_CASES))
def test_attention_stale_reference(name, cross, variant):
    qd, nd, n, want, err_fp32 = _case(name, cross)
    options.reset()
    guard = RangeGuard(torch.device(DEV), lambda: None)
    assert guard.active
    with guard:
        got = _run(qd, nd, cross, variant)
    torch.cuda.synchronize()
    assert int(guard.flag.item()) == 0                                 # every operand in range, p <= 2^TAU included
    got = got.cpu()
    assert torch.isfinite(got).all()
    err = _error(got, want, n)
    print(f"{name} cross={cross} variant={variant}: max / rms error {err[0]:.3e} / {err[1]:.3e}, exact-fp32 kernel {err_fp32[0]:.3e} / {err_fp32[1]:.3e}")
    for b in range(B2):
        np.testing.assert_allclose(got[b, :n[b]].numpy(), want[b].float().numpy(), rtol=1e-4, atol=2e-5)
        assert (got[b, n[b]:] == 0).all()
    assert err[0] <= 1.5 * err_fp32[0] + 1e-9 and err[1] <= 1.5 * err_fp32[1] + 1e-10, (err, err_fp32)
