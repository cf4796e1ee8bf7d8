"""-m gpu: every mfr_eloftr_* entry of csrc/eloftr.hip called DIRECTLY, against float64, at the sizes where its loops run more than once.

tests/test_gpu_eloftr.py runs the stages at 96 x 128 and 160 x 96: 12 and 15 aggregated tokens, so the attention kernel's key-tile loop (tiles of 64)
runs once, there is one query block, no partial tile behind a full one and never Lq != Lk; the compaction only sees maxN = 320, the up-samplings
never an axis of length 1, the rotary entry never k == NULL, and no argument check is ever exercised.  Here:

  * outputs are pre-filled with NaN, so an element the kernel does not write shows;
  * where the output sits in a wider buffer (ld > N, a guard row behind the last one) the guard holds a sentinel that must come back bit-identical;
  * inputs the call has no business reading (guard columns, rows behind a count) hold NaN or plausible values, whichever makes a wrong read visible;
  * continuous results meet the file's bar, eloftr_ref.check: err(device) <= 10 x err(float32 partner), max and rms, against float64 on the same
    float32 inputs, the partner being the same formula in float32 on the CPU; copies, selections and exact scalings are compared bit for bit.

Argument checks: one table per entry; every case differs from a valid call (asserted to return 0) in ONE argument, must return MFR_E_ARG and leave the
NaN-filled outputs untouched (the two in-place entries, _rotary and _leaky_relu, get -2 instead: a NaN stays a NaN under either, so it could not show a write).  Every case stays memory-safe if its check were missing (in-range sizes, 1 MB behind every pointer), so a lost check
shows as a wrong return code and not as a fault.  For that reason the checks that guard against a NULL pointer, a grid dimension above 65535, an
index beyond 2^31 and La <= 0 (a division by zero on the device) are NOT in the tables; the one NULL case is _aggregate with both outputs NULL, which
writes nothing."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import eloftr_ref as R
from mapfree_reloc_amd import _lib
from mapfree_reloc_amd.nets import eloftr as EL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAYER = 1
NAN = float("nan")
SENTINEL = -1.2345678e30
E_ARG = -1                                   # MFR_E_ARG (include/mfr_hip.h)


def _lib_():
    return _lib.load(require_gpu=True)


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _full(shape, value):
    return torch.full(shape, value, dtype=torch.float32, device=DEV)


def _randn(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


@pytest.fixture(scope="module")
def net():
    """the device module, built once per file: the aggregation's weights and the allocation-only wrappers"""
    return EL.EfficientLoFTRHIP(R.weights("perturbed"), DEV)


# ====================================================================================================================== attention
ATT_NB = 3
SQUARE = (7, 8, 9, 63, 64, 65, 72, 129, 391)
RECT = ((1, 391), (65, 7), (130, 64), (391, 65), (63, 129))
SPIKE_AT = (0, 7, 8, 63, 64, -1)
SCORE_SHAPES = ["rising", "falling"] + [f"spike{p}" for p in SPIKE_AT]


def attention_ref(q, k, v):
    """softmax(q k^T / sqrt(32)) v per image and head in the dtype of the inputs: q [nb, Lq, heads, 32], k, v [nb, Lk, heads, 32]"""
    s = torch.einsum("bihc,bjhc->bhij", q, k) / math.sqrt(EL.HIDDEN // EL.HEADS)
    return torch.einsum("bhij,bjhc->bihc", torch.softmax(s, -1), v)


def plain_case(Lq, Lk, heads, seed):
    """randn x 1.5 inputs (the scale of tests' other attention inputs): scaled scores of about +-3"""
    return tuple(_randn((ATT_NB, L, heads, 32), seed + i, 1.5) for i, L in enumerate((Lq, Lk, Lk)))


def shaped_case(Lk, shape, heads=EL.HEADS, seed=40):
    """q and k whose scaled score of query i against key j is f(j) + noise(i, j), noise of about +-0.2, per head: channel 0 of a head carries f (q has
    sqrt(32) there, k has f(j)), the other 31 channels carry the noise.  f: 'rising' 0.5 j (the running maximum moves in every group of 8 keys and ends
    on the last key of the partial tile), 'falling' -0.5 j (it never moves after key 0), 'spikeP' +12 at key P alone (P = -1: the last key).  +12 and no
    more: the other keys keep a weight of e^-12 = 6e-6, above fp32 resolution, so the float32 partner's error stays a round-off figure."""
    j = torch.arange(Lk, dtype=torch.float32)
    if shape == "rising":
        f = 0.5 * j
    elif shape == "falling":
        f = -0.5 * j
    else:
        p = int(shape[len("spike"):])
        f = torch.zeros(Lk)
        f[p] = 12.0
    q = _randn((ATT_NB, Lk, heads, 32), seed, 0.1 * math.sqrt(32.0))
    k = _randn((ATT_NB, Lk, heads, 32), seed + 1, 0.35)
    q[..., 0] = math.sqrt(32.0)
    k[..., 0] = f[None, :, None]
    return q, k, _randn((ATT_NB, Lk, heads, 32), seed + 2, 1.5)


def partner_and_reference(q, k, v):
    """(float32 partner, float64 reference), with the condition on the CASE asserted: the partner's relative max error is a round-off figure (>= 1e-8),
    not one a collapsed softmax makes meaningless as a yardstick"""
    f32, f64 = attention_ref(q, k, v), attention_ref(q.double(), k.double(), v.double())
    assert R.err(f32, f64)[0] >= 1e-8, R.err(f32, f64)
    return f32, f64


def run_attention_packed(q, k, v):
    """q | k | v packed as the stage packs them (ld = 768, 8 heads), out with ldo = 256 and one guard row behind it; rows the call does not own are NaN"""
    nb, Lq, heads, _ = q.shape
    Lk = k.shape[1]
    assert heads == EL.HEADS
    buf = _full((nb * max(Lq, Lk), 768), NAN)
    buf[:nb * Lq, :256] = q.reshape(nb * Lq, 256).to(DEV)
    buf[:nb * Lk, 256:512] = k.reshape(nb * Lk, 256).to(DEV)
    buf[:nb * Lk, 512:] = v.reshape(nb * Lk, 256).to(DEV)
    out = _full((nb * Lq + 1, 256), NAN)
    out[-1] = SENTINEL
    base = buf.data_ptr()
    _lib.check(_lib_().mfr_eloftr_attention(base, 768, base + 1024, base + 2048, 768, nb, Lq, Lk, heads, _lib.ptr(out), 256, _lib.stream_ptr()), "mfr_eloftr_attention")
    assert _same_bits(out[-1], _full((256,), SENTINEL))
    return out[:-1].reshape(nb, Lq, heads, 32).cpu()


def run_attention_separate(q, k, v, ldq=100, ldkv=112, ldo=104):
    """three buffers, every stride different and wider than heads x 32; input guard columns NaN, output guard columns a sentinel"""
    nb, Lq, heads, _ = q.shape
    Lk, n = k.shape[1], heads * 32
    bq, bk, bv = _full((nb * Lq, ldq), NAN), _full((nb * Lk, ldkv), NAN), _full((nb * Lk, ldkv), NAN)
    bq[:, :n], bk[:, :n], bv[:, :n] = q.reshape(-1, n).to(DEV), k.reshape(-1, n).to(DEV), v.reshape(-1, n).to(DEV)
    out = _full((nb * Lq, ldo), SENTINEL)
    out[:, :n] = NAN
    _lib.check(_lib_().mfr_eloftr_attention(_lib.ptr(bq), ldq, _lib.ptr(bk), _lib.ptr(bv), ldkv, nb, Lq, Lk, heads, _lib.ptr(out), ldo, _lib.stream_ptr()),
               "mfr_eloftr_attention")
    assert _same_bits(out[:, n:], _full((nb * Lq, ldo - n), SENTINEL))
    return out[:, :n].reshape(nb, Lq, heads, 32).cpu()


@pytest.mark.parametrize("Lq,Lk", [(L, L) for L in SQUARE] + list(RECT))
def test_attention_vs_float64(Lq, Lk):
    """one to seven key tiles, a partial tile behind full ones, one to seven query blocks with a partial last one, Lq != Lk both ways"""
    q, k, v = plain_case(Lq, Lk, EL.HEADS, 100 + Lq + 7 * Lk)
    f32, f64 = partner_and_reference(q, k, v)
    R.check(f"attention Lq {Lq} Lk {Lk}", run_attention_packed(q, k, v), f32, f64)


@pytest.mark.parametrize("Lq,Lk", [(9, 9), (65, 129), (130, 64)])
def test_attention_three_heads_separate_buffers(Lq, Lk):
    q, k, v = plain_case(Lq, Lk, 3, 300 + Lq)
    f32, f64 = partner_and_reference(q, k, v)
    R.check(f"attention 3 heads, ldq 100 ldkv 112 ldo 104, Lq {Lq} Lk {Lk}", run_attention_separate(q, k, v), f32, f64)


@pytest.mark.parametrize("shape", SCORE_SHAPES)
@pytest.mark.parametrize("Lk", [391, 72])
def test_attention_score_shapes(Lk, shape):
    """where the running maximum moves: in every group of 8 up to the last key of the partial tile, never after key 0, once at a chosen key (first and
    last key of a group of 8, of a tile, of the sequence)"""
    q, k, v = shaped_case(Lk, shape)
    s = torch.einsum("bihc,bjhc->bhij", q.double(), k.double()) / math.sqrt(32.0)
    if shape == "rising":
        g = s[..., :Lk // 8 * 8].reshape(*s.shape[:-1], Lk // 8, 8).amax(-1)
        assert bool((s.argmax(-1) >= Lk - 5).all()) and bool((g[..., 1:] > g[..., :-1]).all())
    elif shape == "falling":
        assert bool((s.argmax(-1) <= 4).all())
    else:
        p = int(shape[len("spike"):]) % Lk
        assert bool((s.argmax(-1) == p).all()) and float(s[..., p].min()) > 10.5 and float(s.abs().amax(-1).max()) < 13.5
    f32, f64 = partner_and_reference(q, k, v)
    R.check(f"attention Lk {Lk} scores {shape}", run_attention_packed(q, k, v), f32, f64)


@pytest.mark.parametrize("Lq", [1, 65])
def test_attention_one_key_returns_v(Lq):
    """Lk = 1: the weight is exp(0) / 1, so the output IS v, bit for bit (check does not apply: the partner's error is zero)"""
    q, k, v = plain_case(Lq, 1, EL.HEADS, 500 + Lq)
    got = run_attention_packed(q, k, v)
    assert _same_bits(got, v.expand(-1, Lq, -1, -1).contiguous())
    q, k, v = plain_case(Lq, 1, 3, 510 + Lq)
    assert _same_bits(run_attention_separate(q, k, v), v.expand(-1, Lq, -1, -1).contiguous())


# ====================================================================================================================== up-sampling, hand-over, activation
@pytest.mark.parametrize("ha,wa", [(1, 1), (1, 5), (6, 1), (3, 7)])
def test_upsample4_rows_vs_float64(ha, wa):
    """an axis of length 1 (both neighbours clamp) and odd grids; dst = the right half of a 512-wide buffer whose images lie 3 rows further apart than
    they must: the left half and the gap rows come back bit-identical"""
    nimg, ldm, gap = 3, 260, 3
    L = 16 * ha * wa
    msg = _randn((nimg, ha * wa, 256), 60 + ha * 8 + wa)
    bm = _full((nimg * ha * wa, ldm), NAN)
    bm[:, :256] = msg.reshape(-1, 256).to(DEV)
    before = _full((nimg * (L + gap), 512), SENTINEL)
    buf = before.clone()
    rows = torch.cat([torch.arange(L) + i * (L + gap) for i in range(nimg)]).to(DEV)
    buf[rows, 256:] = NAN
    _lib.check(_lib_().mfr_eloftr_upsample4_rows(_lib.ptr(bm), ldm, nimg, ha, wa, buf.data_ptr() + 1024, 512, (L + gap) * 512, _lib.stream_ptr()), "mfr_eloftr_upsample4_rows")
    got = buf[rows, 256:].reshape(nimg, 4 * ha, 4 * wa, 256).cpu()
    buf[rows, 256:] = SENTINEL
    assert _same_bits(buf, before)
    up = lambda t: F.interpolate(t.reshape(nimg, ha, wa, 256).permute(0, 3, 1, 2), scale_factor=4, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    R.check(f"upsample4_rows {ha} x {wa}", got, up(msg), up(msg.double()))


@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("H,W", [(1, 1), (1, 9), (7, 1), (5, 6)])
def test_upsample2x_vs_float64(H, W, with_add):
    planes = 5
    x, add = _randn((1, planes, H, W), 70 + H * 16 + W), _randn((1, planes, 2 * H, 2 * W), 71 + H * 16 + W)
    out = _full((planes * 4 * H * W + 8,), NAN)
    out[-8:] = SENTINEL
    dx, a = x.to(DEV), add.to(DEV) if with_add else None
    _lib.check(_lib_().mfr_eloftr_upsample2x(_lib.ptr(dx), _lib.ptr(a), _lib.ptr(out), planes, H, W, _lib.stream_ptr()), "mfr_eloftr_upsample2x")
    assert _same_bits(out[-8:], _full((8,), SENTINEL))
    up = lambda t, s: F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=False) + (s if with_add else 0)
    got, f32, f64 = out[:-8].reshape(1, planes, 2 * H, 2 * W).cpu(), up(x, add), up(x.double(), add.double())
    if (H, W) == (1, 1) and not with_add:
        # every output IS the plane's one input value and torch's float32 returns it exactly: a partner without error is no yardstick.  The kernel
        # evaluates l0 (lx0 a + lx1 a) + l1 (...) with exact weights (0.25 / 0.75): two rounded products and a rounded sum per axis pair, each half an
        # ulp of a value no larger than |a| -- 4 ulp of |a| bounds it
        e = float(((got.double() - f64).abs() / f64.abs()).max())
        print(f"[eloftr] upsample2x 1 x 1: device max relative error {e:.3e} (float32 partner: exact)")
        assert float((f32.double() - f64).abs().max()) == 0 and e <= 4 * 2.0 ** -24
    else:
        R.check(f"upsample2x {H} x {W} add {with_add}", got, f32, f64)


@pytest.mark.parametrize("C", [32, 256])
@pytest.mark.parametrize("HW", [1, 31, 32, 33, 240])
def test_rows_to_nchw_is_the_scaled_permutation(HW, C):
    """below, on and above the 32-token tile; 1 / 16 is a power of two, so out == permute(x) / 16 bit for bit.  Columns beyond C and the gap rows are NaN"""
    nimg, gap = 3, 2
    x = _randn((nimg, HW, C), 80 + HW + C)
    buf = _full((nimg, HW + gap, 512), NAN)
    buf[:, :HW, :C] = x.to(DEV)
    out = _full((nimg * C * HW + 8,), NAN)
    out[-8:] = SENTINEL
    _lib.check(_lib_().mfr_eloftr_rows_to_nchw(_lib.ptr(buf), 512, (HW + gap) * 512, nimg, C, HW, 1.0 / 16.0, _lib.ptr(out), _lib.stream_ptr()), "mfr_eloftr_rows_to_nchw")
    assert _same_bits(out[-8:], _full((8,), SENTINEL))
    assert _same_bits(out[:-8].reshape(nimg, C, HW).cpu(), (x.permute(0, 2, 1) * (1.0 / 16.0)).contiguous())


@pytest.mark.parametrize("rows", [1, 1031])
def test_leaky_relu_in_place_with_guard_columns(rows):
    """N = 20 of ld = 28: one fp32 multiply, so equal to F.leaky_relu on the device bit for bit; the 8 guard columns untouched"""
    N, ld = 20, 28
    x = _randn((rows, N), 90 + rows)
    x[0, :4] = torch.tensor([0.0, 1e-30, -1e-30, -3.0e38])
    buf = _full((rows, ld), SENTINEL)
    buf[:, :N] = x.to(DEV)
    want = F.leaky_relu(x.to(DEV), 0.01)
    _lib.check(_lib_().mfr_eloftr_leaky_relu(_lib.ptr(buf), ld, rows, N, 0.01, _lib.stream_ptr()), "mfr_eloftr_leaky_relu")
    assert _same_bits(buf[:, N:], _full((rows, ld - N), SENTINEL))
    assert _same_bits(buf[:, :N], want) and bool((want < 0).any())


def _module_rotation(m, q, k, hw):
    """eloftr_ref.rotary_qk's rotation alone (the module's tables and apply_rotary_pos_emb) on GIVEN q, k [n, La, 256]"""
    from transformers.models.efficientloftr.modeling_efficientloftr import apply_rotary_pos_emb
    n, La, _ = q.shape
    cos, sin = R.position_embeddings(m, torch.zeros(n, 256, hw[0], hw[1], dtype=q.dtype))
    a, b = apply_rotary_pos_emb(q.view(n, La, 1, 256), k.view(n, La, 1, 256), cos, sin, unsqueeze_dim=2)
    return a.reshape(n, La, 256).to(q.dtype), b.reshape(n, La, 256).to(q.dtype)


@pytest.mark.parametrize("with_k", [False, True])
def test_rotary_on_given_q_and_k(with_k):
    """rows = 3 x 15 (aggregated grid 3 x 5) in the stage's q | k | v buffer; k == NULL rotates q alone and leaves the k (and v) columns untouched"""
    n, hw_agg = 3, (3, 5)
    La = hw_agg[0] * hw_agg[1]
    q, k = _randn((n, La, 256), 95), _randn((n, La, 256), 96)
    buf = _full((n * La, 768), SENTINEL)
    buf[:, :256], buf[:, 256:512] = q.reshape(-1, 256).to(DEV), k.reshape(-1, 256).to(DEV)
    before = buf.clone()
    cs = EL.rotary_table(hw_agg[0], hw_agg[1], DEV)
    _lib.check(_lib_().mfr_eloftr_rotary(buf.data_ptr(), buf.data_ptr() + 1024 if with_k else None, 768, _lib.ptr(cs), n * La, La, _lib.stream_ptr()), "mfr_eloftr_rotary")
    m32, m64 = R.modules("perturbed")
    hw = (EL.AGG * hw_agg[0], EL.AGG * hw_agg[1])                                                     # the 1/8 grid the module aggregates by 4
    with torch.no_grad():
        f32, f64 = _module_rotation(m32, q, k, hw), _module_rotation(m64, q.double(), k.double(), hw)
    R.check(f"rotary q (k {'given' if with_k else 'NULL'})", buf[:, :256].reshape(n, La, 256).cpu(), f32[0], f64[0])
    if with_k:
        R.check("rotary k", buf[:, 256:512].reshape(n, La, 256).cpu(), f32[1], f64[1])
        assert _same_bits(buf[:, 512:], before[:, 512:])
    else:
        assert _same_bits(buf[:, 256:], before[:, 256:])


# ====================================================================================================================== aggregation, stem, compaction
@pytest.mark.parametrize("hc,wc", [(4, 4), (8, 4)])
def test_aggregate_outputs_separately_and_together(net, hc, wc):
    """one and two aggregated cells per image; the single-output calls (cross attention) equal the matching half of the two-output call bit for bit"""
    nimg, gap = 3, 2
    L, La = hc * wc, (hc // 4) * (wc // 4)
    x = _randn((nimg, 256, hc, wc), 110 + hc)
    buf = _full((nimg, L + gap, 512), NAN)
    buf[:, :L, :256] = x.permute(0, 2, 3, 1).reshape(nimg, L, 256).to(DEV)
    blk = net.layers[LAYER]["self"]

    def run(want_q, want_kv):
        q, kv = (_full((nimg * La + 1, 256), NAN) if w else None for w in (want_q, want_kv))
        for t in (q, kv):
            if t is not None:
                t[-1] = SENTINEL
        _lib.check(_lib_().mfr_eloftr_aggregate(_lib.ptr(buf), 512, (L + gap) * 512, nimg, hc, wc, _lib.ptr(blk["wagg"]), _lib.ptr(blk["ln"][0]), _lib.ptr(blk["ln"][1]),
                                                1e-5, _lib.ptr(q), _lib.ptr(kv), _lib.stream_ptr()), "mfr_eloftr_aggregate")
        for t in (q, kv):
            assert t is None or _same_bits(t[-1], _full((256,), SENTINEL))
        return (None if q is None else q[:-1]), (None if kv is None else kv[:-1])
    q, kv = run(True, True)
    assert _same_bits(run(True, False)[0], q) and _same_bits(run(False, True)[1], kv)
    m32, m64 = R.modules("perturbed")
    with torch.no_grad():
        a32, a64 = R.aggregation(m32, LAYER, "self", x), R.aggregation(m64, LAYER, "self", x.double())
    R.check(f"aggregate q {hc} x {wc}", q.reshape(nimg, La, 256).cpu(), a32[0], a64[0])
    R.check(f"aggregate kv {hc} x {wc}", kv.reshape(nimg, La, 256).cpu(), a32[1], a64[1])


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("H,W", [(2, 2), (6, 34)])
@pytest.mark.parametrize("Cout", [5, 64])
def test_stem_s2_vs_float64_convolution(Cout, H, W, with_bias):
    """one output pixel per image (every tap but the centre 2 x 2 is padding) and 3 x 17; a filter count below the LDS table's 64 and at it; bias NULL"""
    B = 3
    x, w, b = torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(120 + H)), _randn((Cout, 1, 3, 3), 121 + Cout, 0.5), _randn((Cout,), 122 + Cout, 0.2)
    n = B * Cout * (H // 2) * (W // 2)
    y = _full((n + 8,), NAN)
    y[-8:] = SENTINEL
    dx, dw, db = x.to(DEV), w.to(DEV), b.to(DEV)
    _lib.check(_lib_().mfr_eloftr_stem_s2(_lib.ptr(dx), _lib.ptr(dw), _lib.ptr(db) if with_bias else None, B, H, W, Cout, _lib.ptr(y), _lib.stream_ptr()), "mfr_eloftr_stem_s2")
    assert _same_bits(y[-8:], _full((8,), SENTINEL))
    want = torch.relu(F.conv2d(x.double(), w.double(), b.double() if with_bias else None, stride=2, padding=1))
    got = y[:-8].reshape(want.shape).cpu()
    e = float((got.double() - want).abs().max())
    print(f"[eloftr] stem_s2 Cout {Cout} {H} x {W} bias {with_bias}: max error {e:.3e}, scale {float(want.abs().max()):.3e}")
    assert float(want.abs().max()) > 0.1 and e <= 2e-5 * float(want.abs().max())


def compact_case(maxN, W=100, H=80, seed=130):
    """B = 3 pairs with n = [maxN, maxN // 2, 0].  EVERY slot holds points, also behind n[b] (most of them inside the frame: a kernel that ignores the
    count keeps them).  Each of a slot's 4 coordinates lies outside with probability 0.1, so about a third of the slots fail; slots around 255 / 256 and
    511 / 512 (the 256-slot passes of the kernel) are forced: fail at 253, 255, 256, 258, 509, 511, 512, 514, keep at 254, 257, 510, 513.  Slots 3 k + 1
    of the failing ones have a coordinate EXACTLY on the edge (x == W or y == H): dropped, the test is strict."""
    g = torch.Generator().manual_seed(seed + maxN)
    B = 3
    bound = torch.tensor([W, H], dtype=torch.float32)
    pts = torch.rand(B, 2, maxN, 2, generator=g) * bound * 0.98                                      # [pair, side, slot, xy], all inside
    out = torch.rand(B, 2, maxN, 2, generator=g) < 0.1
    for s in (253, 255, 256, 258, 509, 511, 512, 514):
        if s < maxN:
            out[:, :, s] = False
            out[:, s % 2, s, (s // 2) % 2] = True
    for s in (254, 257, 510, 513):
        if s < maxN:
            out[:, :, s] = False
    if maxN == 1:
        out[0], out[1] = False, False
        out[1, 1, 0, 1] = True                                                                       # pair 0 keeps its slot (pair 1 has n = 0 anyway)
    beyond = bound * (1.0 + 0.2 * torch.rand(B, 2, maxN, 2, generator=g))
    fail = torch.nonzero(out.any(1).any(-1))
    pts = torch.where(out, beyond, pts)
    for b, s in fail[1::3].tolist():                                                                 # exactly on the edge
        side, xy = torch.nonzero(out[b, :, s])[0].tolist()
        pts[b, side, s, xy] = bound[xy]
    conf = torch.rand(B, maxN + 3, generator=g)
    n = torch.tensor([maxN, maxN // 2, 0], dtype=torch.int32)
    return pts[:, 0].contiguous(), pts[:, 1].contiguous(), conf, n


@pytest.mark.parametrize("maxN", [1, 255, 256, 257, 600])
def test_compact_against_a_boolean_mask(maxN):
    W, H, B = 100, 80, 3
    p0, p1, conf, n = compact_case(maxN, W, H)
    o0, o1, oc = _full((B, maxN, 2), NAN), _full((B, maxN, 2), NAN), _full((B, maxN), NAN)
    n_out = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    d0, d1, dc, dn = p0.to(DEV), p1.to(DEV), conf.to(DEV), n.to(DEV)
    _lib.check(_lib_().mfr_eloftr_compact(_lib.ptr(d0), _lib.ptr(d1), _lib.ptr(dc), maxN + 3, _lib.ptr(dn), B, maxN, W, H, _lib.ptr(o0), _lib.ptr(o1), _lib.ptr(oc),
                                          _lib.ptr(n_out), _lib.stream_ptr()), "mfr_eloftr_compact")
    a, c, cf = p0.numpy(), p1.numpy(), conf.numpy()
    w0, w1, wc, wn = np.zeros((B, maxN, 2), np.float32), np.zeros((B, maxN, 2), np.float32), np.zeros((B, maxN), np.float32), np.zeros(B, np.int32)
    edge = 0
    for b in range(B):
        live = np.arange(maxN) < int(n[b])
        keep = live & (a[b, :, 0] < np.float32(W)) & (a[b, :, 1] < np.float32(H)) & (c[b, :, 0] < np.float32(W)) & (c[b, :, 1] < np.float32(H))
        edge += int((live & ((a[b, :, 0] == W) | (a[b, :, 1] == H) | (c[b, :, 0] == W) | (c[b, :, 1] == H))).sum())
        wn[b] = keep.sum()
        w0[b, :wn[b]], w1[b, :wn[b]], wc[b, :wn[b]] = a[b][keep], c[b][keep], cf[b, :maxN][keep]
    print(f"[eloftr] compact maxN {maxN}: n {n.tolist()} -> {wn.tolist()}, {edge} live slots exactly on the edge")
    if maxN >= 255:
        assert 0.2 * maxN < maxN - wn[0] < 0.5 * maxN and edge > 0
    assert np.array_equal(n_out.cpu().numpy(), wn)
    for got, want in ((o0, w0), (o1, w1), (oc, wc)):
        assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))


# ====================================================================================================================== argument checks
POOL = 1 << 18                                # floats behind every pointer (1 MB): every case below stays inside if its check were missing


class _Pool:
    def __init__(self):
        self.i = [_full((POOL,), 0.5) for _ in range(4)]                                             # inputs
        self.o = [_full((POOL,), NAN) for _ in range(4)]                                             # outputs
        self.n = torch.ones(POOL, dtype=torch.int32, device=DEV)                                     # counts (1 live slot per pair)
        self.z = torch.zeros(POOL, dtype=torch.int32, device=DEV)                                    # cell and image indices
        self.oi = torch.full((POOL,), -1, dtype=torch.int32, device=DEV)                             # integer outputs

    def reset(self, fill=NAN):
        """NaN into every output; -2 for the two entries that work in place (a NaN stays a NaN under a rotation or a leaky ReLU: it could not show a write)"""
        self.fill = fill
        for t in self.o:
            t.fill_(fill)
        self.oi.fill_(-1)

    def untouched(self):
        same = (lambda t: bool(torch.isnan(t).all())) if self.fill != self.fill else (lambda t: bool((t == self.fill).all()))
        return all(same(t) for t in self.o) and bool((self.oi == -1).all())


@pytest.fixture(scope="module")
def pool():
    return _Pool()


def _entries(p):
    """entry -> (its valid arguments by name, in the order of the C declaration)"""
    I, O = [t.data_ptr() for t in p.i], [t.data_ptr() for t in p.o]
    return {
        "stem_s2": dict(x=I[0], w=I[1], bias=I[2], B=2, H=4, W=6, Cout=5, y=O[0]),
        "aggregate": dict(x=I[0], ldx=256, img_stride=16 * 256, nimg=2, hc=4, wc=4, wq=I[1], gamma=I[2], beta=I[3], eps=1e-5, q_out=O[0], kv_out=O[1]),
        "rotary": dict(q=O[0], k=O[1], ld=256, cos_sin=I[0], rows=30, La=15),
        "attention": dict(q=I[0], ldq=256, k=I[1], v=I[2], ldkv=256, nb=2, Lq=9, Lk=9, heads=8, out=O[0], ldo=256),
        "upsample4_rows": dict(msg=I[0], ldm=256, nimg=2, ha=1, wa=2, dst=O[0], ldx=256, img_stride=32 * 256),
        "upsample2x": dict(inp=I[0], add=I[1], out=O[0], planes=2, H=3, W=4),
        "leaky_relu": dict(x=O[0], ld=32, rows=5, N=24, slope=0.01),
        "rows_to_nchw": dict(x=I[0], ldx=64, img_stride=40 * 64, nimg=2, C=64, HW=40, scale=0.5, out=O[0]),
        "gather_windows": dict(feat=I[0], nimg=2, Hh=8, Wh=8, C=64, img_ids=p.z.data_ptr(), cell_ids=p.z.data_ptr(), ld_cells=4, n=p.n.data_ptr(), B=2, maxN=2, wc=2,
                               cell_px=8, win=8, pad=0, out=O[0]),
        "fine_match": dict(win0=I[0], win1=I[1], cell_i=p.z.data_ptr(), cell_j=p.z.data_ptr(), ld_cells=4, n=p.n.data_ptr(), B=2, maxN=2, wc=2, cell_px=8, pts0=O[0],
                           pts1=O[1], arg=p.oi.data_ptr()),
        "compact": dict(pts0=I[0], pts1=I[1], conf=I[2], ld_conf=8, n=p.n.data_ptr(), B=2, maxN=4, W=100, H=80, out0=O[0], out1=O[1], out_conf=O[2], n_out=p.oi.data_ptr()),
    }


# entry -> the cases: (id, the ONE argument that differs; an int for a pointer is a byte offset added to it)
_OFF = ("x", "q", "k", "v", "out", "msg", "dst", "feat", "win0", "win1", "pts0", "pts1", "out0", "out1")
ARG_CASES = {
    "stem_s2": [("B0", dict(B=0)), ("H0", dict(H=0)), ("W0", dict(W=0)), ("H_odd", dict(H=5)), ("W_odd", dict(W=7)), ("Cout0", dict(Cout=0)), ("Cout65", dict(Cout=65))],
    "aggregate": [("no_output", dict(q_out=None, kv_out=None)), ("nimg0", dict(nimg=0)), ("hc0", dict(hc=0)), ("wc0", dict(wc=0)), ("hc_not_x4", dict(hc=6)),
                  ("wc_not_x4", dict(wc=6)), ("ldx_below_256", dict(ldx=252)), ("img_stride_short", dict(img_stride=16 * 256 - 1))],
    "rotary": [("rows0", dict(rows=0)), ("rows_not_xLa", dict(rows=29)), ("ld_below_256", dict(ld=254)), ("ld_odd", dict(ld=257)), ("q_off_4", dict(q=4)), ("k_off_4", dict(k=4))],
    "attention": [("nb0", dict(nb=0)), ("Lq0", dict(Lq=0)), ("Lk0", dict(Lk=0)), ("heads0", dict(heads=0)), ("ldq_short", dict(ldq=252)), ("ldkv_short", dict(ldkv=252)),
                  ("ldo_short", dict(ldo=252)), ("ldq_not_x4", dict(ldq=258)), ("ldkv_not_x4", dict(ldkv=258)), ("ldo_not_x4", dict(ldo=258)), ("q_off_8", dict(q=8)),
                  ("k_off_8", dict(k=8)), ("v_off_8", dict(v=8)), ("out_off_8", dict(out=8))],
    "upsample4_rows": [("nimg0", dict(nimg=0)), ("ha0", dict(ha=0)), ("wa0", dict(wa=0)), ("ldm_short", dict(ldm=252)), ("ldx_short", dict(ldx=252)),
                       ("ldm_not_x4", dict(ldm=258)), ("ldx_not_x4", dict(ldx=258, img_stride=32 * 258)), ("img_stride_not_x4", dict(img_stride=32 * 256 + 2)),
                       ("img_stride_short", dict(img_stride=32 * 256 - 4)), ("msg_off_8", dict(msg=8)), ("dst_off_8", dict(dst=8))],
    "upsample2x": [("planes0", dict(planes=0)), ("H0", dict(H=0)), ("W0", dict(W=0))],
    "leaky_relu": [("rows0", dict(rows=0)), ("N0", dict(N=0)), ("N_not_x4", dict(N=22)), ("ld_below_N", dict(ld=20)), ("ld_not_x4", dict(ld=30)), ("x_off_8", dict(x=8))],
    "rows_to_nchw": [("nimg0", dict(nimg=0)), ("C0", dict(C=0)), ("C_not_x32", dict(C=48)), ("HW0", dict(HW=0)), ("ldx_below_C", dict(ldx=60)),
                     ("img_stride_short", dict(img_stride=40 * 64 - 1))],
    "gather_windows": [("nimg0", dict(nimg=0)), ("Hh0", dict(Hh=0)), ("Wh0", dict(Wh=0)), ("C_not_64", dict(C=32)), ("B0", dict(B=0)), ("maxN0", dict(maxN=0)),
                       ("ld_cells_below_maxN", dict(ld_cells=1)), ("wc0", dict(wc=0)), ("cell_px0", dict(cell_px=0)), ("win0", dict(win=0)), ("win17", dict(win=17)),
                       ("pad_negative", dict(pad=-1)), ("feat_off_8", dict(feat=8)), ("out_off_8", dict(out=8))],
    "fine_match": [("B0", dict(B=0)), ("maxN0", dict(maxN=0)), ("ld_cells_below_maxN", dict(ld_cells=1)), ("wc0", dict(wc=0)), ("cell_px0", dict(cell_px=0)),
                   ("win0_off_8", dict(win0=8)), ("win1_off_8", dict(win1=8))],
    "compact": [("B0", dict(B=0)), ("maxN0", dict(maxN=0)), ("ld_conf_below_maxN", dict(ld_conf=3)), ("W0", dict(W=0)), ("H0", dict(H=0)), ("pts0_off_4", dict(pts0=4)),
                ("pts1_off_4", dict(pts1=4)), ("out0_off_4", dict(out0=4)), ("out1_off_4", dict(out1=4))],
}


IN_PLACE = ("rotary", "leaky_relu")


def _call(entry, p, change):
    p.reset(-2.0 if entry in IN_PLACE else NAN)
    args = _entries(p)[entry]
    for k, v in change.items():
        assert k in args, (entry, k)
        args[k] = args[k] + v if (k in _OFF and v is not None) else v
    return getattr(_lib_(), f"mfr_eloftr_{entry}")(*args.values(), _lib.stream_ptr())


@pytest.mark.parametrize("entry", list(ARG_CASES))
def test_argument_tables_start_from_a_valid_call(pool, entry):
    assert _call(entry, pool, {}) == 0
    torch.cuda.synchronize()
    assert not pool.untouched()                                                                      # the valid call does write: `untouched` can tell


@pytest.mark.parametrize("entry,case,change", [(e, c, ch) for e, cases in ARG_CASES.items() for c, ch in cases], ids=[f"{e}-{c}" for e, cases in ARG_CASES.items() for c, _ in cases])
def test_argument_check_returns_e_arg_and_writes_nothing(pool, entry, case, change):
    rc = _call(entry, pool, change)
    torch.cuda.synchronize()
    assert rc == E_ARG, (entry, case, rc)
    assert pool.untouched(), (entry, case)
