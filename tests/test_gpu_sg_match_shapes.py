"""-m gpu tests of SuperGlue's match head (csrc/superglue_match.hip) OFF the 1024 x 1024 problem every other comparison with a reference runs at: row
pitches that are no multiple of 4 or of 64, fewer than 16 rows, fewer than 64 columns, ldS > 1024, other iteration counts, bin scores and thresholds,
exact ties, a non-finite score and a score block that is not 16-byte aligned.

Reference: oracle.nets_ref.log_optimal_transport on the valid block in FLOAT64, then row / column arg-max, mutual check, exp(score) > thr and ordered
compaction -- the code of tests/test_gpu_nets_parity.py::test_sinkhorn_match_vs_oracle, with that test's bars: matches exact outside a band of 1e-3
around the threshold (the band's rows are counted and printed, at most max(2, m // 100) of them), scores within rtol 2e-4 / atol 2e-5.  A row is in
the band if it IS a mutual arg-max and its score is within 1e-3 of the threshold: the row of another kind scores exactly 0 on both sides whatever the
threshold, so at thr = 0 it is not a threshold decision (for every thr > 1e-3 this is that test's `abs(ms0 - thr) <= 1e-3`, to the row).

Every launch goes through the C entry point on buffers of the test's own: outputs pre-filled with NaN / -7, one guard row behind each, the workspace
sized exactly by mfr_sg_match_workspace_bytes and filled with 0xFF."""
import numpy as np
import pytest
import torch

from mapfree_reloc_amd import _lib
from oracle import nets_ref as NR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAND = 1e-3

# ldS -> (m list, n list): the pairs of one launch
SHAPES = {
    4: ([4, 1, 3], [4, 4, 2]),                      # sweep kernel, one float4 per row, 13+ row groups without a row
    37: ([37, 1, 20], [30, 37, 37]),                # general row path, n < 64: lanes without a column in the butterfly
    70: ([70, 33, 64], [65, 70, 1]),                # general path, two column blocks; a single column
    512: ([512, 300, 17], [512, 511, 400]),         # sweep kernel, half its float4 indices clamped; n == ldS
    1000: ([1000, 999, 611], [1000, 640, 1000]),    # sweep kernel, last float4 index 249
    1002: ([1002, 1001, 40], [1002, 777, 1002]),    # general path just below 1024
    1100: ([1100, 1030], [1050, 1100]),             # ldS > 1024
}
# variant 0 == variant 1: ragged, m < 16, n % 4 != 0, n == ldS, an empty side
RAGGED = {
    4: ([4, 1, 3, 0, 4, 2], [4, 4, 2, 3, 0, 3]),
    512: ([512, 300, 17, 1, 0, 15, 511, 64, 49], [512, 511, 400, 5, 12, 512, 3, 0, 48]),
    1000: ([1000, 999, 611, 40, 1, 0, 16, 49, 777], [1000, 640, 1000, 17, 5, 12, 999, 998, 0]),
    1020: ([1020, 611, 40, 1, 1000, 65, 0, 777, 16, 49], [1020, 1000, 17, 5, 3, 64, 12, 778, 1019, 48]),
}


def f32(x):
    """the value the C entry point receives for a `float` parameter"""
    return float(np.float32(x))


def structured_scores(g, B, m_list, n_list, ld):
    """tests/test_gpu_nets_parity.py::_structured_scores"""
    S = torch.randn(B, ld, ld, generator=g) * 0.5
    for b in range(B):
        k = min(m_list[b], n_list[b])
        perm = torch.randperm(n_list[b], generator=g)[:k]
        S[b, torch.arange(k), perm] += torch.rand(k, generator=g) * 12
    return S


_inputs, _couplings = {}, {}


def inputs(ld, lists=None):
    """(S, k0, k1, m list, n list) on the host, seed 600 + ldS; computed once and never written"""
    key = (ld, lists is None)
    if key not in _inputs:
        m_list, n_list = lists or SHAPES[ld]
        g = torch.Generator().manual_seed(600 + ld)
        S = structured_scores(g, len(m_list), [max(m, 1) for m in m_list], [max(n, 1) for n in n_list], ld)
        k0 = torch.rand(len(m_list), ld, 2, generator=g) * 500
        k1 = torch.rand(len(m_list), ld, 2, generator=g) * 500
        _inputs[key] = (S, k0, k1, m_list, n_list)
    return _inputs[key]


def reference(S, m, n, bin_score, iters, thr, key=None):
    """float64 -> (matches0 [m] (-1 = none), mscores0 [m], mutual [m]) of one pair; the couplings are kept per `key` (they do not depend on thr)"""
    if m == 0 or n == 0:
        return torch.full((m,), -1, dtype=torch.long), torch.zeros(m, dtype=torch.float64), torch.zeros(m, dtype=torch.bool)
    if key is None or key not in _couplings:
        Z = NR.log_optimal_transport(S[None, :m, :n].double(), torch.tensor(f32(bin_score), dtype=torch.float64), iters)[0, :-1, :-1]
        max0, max1 = Z.max(1), Z.max(0)
        if key is not None:
            _couplings[key] = (max0, max1)
    else:
        max0, max1 = _couplings[key]
    i0, i1 = max0.indices, max1.indices
    mutual = torch.arange(m) == i1[i0]
    ms0 = torch.where(mutual, max0.values.exp(), torch.zeros((), dtype=torch.float64))
    valid = mutual & (ms0 > f32(thr))
    return torch.where(valid, i0, torch.tensor(-1)), ms0, mutual


def band_of(ms0, mutual, thr):
    return mutual & ((ms0 - f32(thr)).abs() <= BAND)


def launch(S, m_list, n_list, k0, k1, bin_score, iters, thr, variant, maxN=None):
    """mfr_sg_sinkhorn_match_variant on S [B, ld, ld] (a device tensor, used where it lies); -> the outputs on the host, the guard row of each as its
    last row.  Checks the guard rows."""
    lib = _lib.load()
    B, ld, _ = S.shape
    maxN = maxN or ld
    n0 = torch.tensor(m_list, dtype=torch.int32, device=DEV); n1 = torch.tensor(n_list, dtype=torch.int32, device=DEV)
    k0, k1 = k0.to(DEV), k1.to(DEV)
    ws = torch.full((lib.mfr_sg_match_workspace_bytes(B, ld),), 0xFF, dtype=torch.uint8, device=DEV)
    o = dict(matches0=torch.full((B + 1, ld), -7, dtype=torch.int32, device=DEV), matching_scores0=torch.full((B + 1, ld), float("nan"), device=DEV),
             pts0=torch.full((B + 1, maxN, 2), float("nan"), device=DEV), pts1=torch.full((B + 1, maxN, 2), float("nan"), device=DEV),
             n_corr=torch.full((B + 1,), -7, dtype=torch.int32, device=DEV))
    _lib.check(lib.mfr_sg_sinkhorn_match_variant(_lib.ptr(S), B, ld, _lib.ptr(n0), _lib.ptr(n1), float(bin_score), int(iters), float(thr),
                                                 _lib.ptr(k0), _lib.ptr(k1), k0.shape[1], _lib.ptr(ws), ws.numel(),
                                                 _lib.ptr(o["matches0"]), _lib.ptr(o["matching_scores0"]), _lib.ptr(o["pts0"]), _lib.ptr(o["pts1"]), maxN,
                                                 _lib.ptr(o["n_corr"]), int(variant), _lib.stream_ptr()), "mfr_sg_sinkhorn_match_variant")
    torch.cuda.synchronize()
    o = {k: v.cpu() for k, v in o.items()}
    assert (o["matches0"][B] == -7).all() and int(o["n_corr"][B]) == -7, "guard row written"
    for k in ("matching_scores0", "pts0", "pts1"):
        assert torch.isnan(o[k][B]).all(), f"guard row of {k} written"
    return o


def bits(t):
    return t.contiguous().numpy().view(np.int32)


def check_against_reference(o, S, k0, k1, m_list, n_list, bin_score, iters, thr, tag, min_frac=False):
    """the assertions of test_sinkhorn_match_vs_oracle for every pair of a launch; -> the reference's number of matches in the batch"""
    ld = S.shape[1]
    n_ref = 0
    for b, (m, n) in enumerate(zip(m_list, n_list)):
        want, ms0, mutual = reference(S[b], m, n, bin_score, iters, thr, key=(ld, b, m, n, f32(bin_score), iters))
        band = band_of(ms0, mutual, thr)
        safe = ~band
        got = o["matches0"][b, :m].long()
        gs = o["matching_scores0"][b, :m]
        n_band, cap = int(band.sum()), max(2, m // 100)
        n_flip = int((got[band] != want[band]).sum())
        n_ref += int((want > -1).sum())
        print(f"{tag} pair {b} ({m} x {n}): {n_band} of {m} rows within {BAND} of the {thr} threshold (cap {cap}), {n_flip} of them decided differently; "
              f"{int((want > -1).sum())} reference matches, {int((got > -1).sum())} here")
        assert n_band <= cap
        np.testing.assert_array_equal(got[safe].numpy(), want[safe].numpy())
        np.testing.assert_allclose(gs[safe].double().numpy(), ms0[safe].numpy(), rtol=2e-4, atol=2e-5)
        nv = int((got > -1).sum())
        assert int(o["n_corr"][b]) == nv
        if min_frac and min(m, n) >= 4:
            assert nv > min(m, n) // 4
        sel = torch.nonzero(got > -1)[:, 0]
        np.testing.assert_array_equal(o["pts0"][b, :nv].numpy(), k0[b, sel].numpy())
        np.testing.assert_array_equal(o["pts1"][b, :nv].numpy(), k1[b, got[sel]].numpy())
        assert (bits(o["pts0"][b, nv:]) == 0).all() and (bits(o["pts1"][b, nv:]) == 0).all()
        assert (o["matches0"][b, m:] == -1).all() and (bits(o["matching_scores0"][b, m:]) == 0).all()
    return n_ref


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("bin_score", [1.0, 2.37])
@pytest.mark.parametrize("ld", sorted(SHAPES))
def test_match_head_vs_float64_oracle(ld, bin_score, variant):
    S, k0, k1, m_list, n_list = inputs(ld)
    o = launch(S.to(DEV), m_list, n_list, k0, k1, bin_score, 20, 0.2, variant)
    check_against_reference(o, S, k0, k1, m_list, n_list, bin_score, 20, 0.2, f"ldS {ld} bin {bin_score} variant {variant}", min_frac=True)


@pytest.mark.parametrize("ld", sorted(RAGGED))
def test_one_sweep_equals_two_pass_bitwise_off_1024(ld):
    """tests/test_gpu_nets_parity.py::test_sinkhorn_one_sweep_equals_two_pass_bitwise at other row pitches"""
    S, k0, k1, m_list, n_list = inputs(ld, RAGGED[ld])
    Sd = S.to(DEV)
    a = launch(Sd, m_list, n_list, k0, k1, 2.37, 20, 0.2, 0)
    b = launch(Sd, m_list, n_list, k0, k1, 2.37, 20, 0.2, 1)
    for k in a:
        np.testing.assert_array_equal(bits(a[k]), bits(b[k]), err_msg=k)
    B = len(m_list)
    total = int(a["n_corr"][:B].sum())
    print(f"ldS {ld}: {total} matches in {B} pairs, the same bits from both variants")
    assert total > sum(min(m, n) for m, n in zip(m_list, n_list)) // 4          # the planted peaks: what every pair of the oracle test exceeds
    for i, (m, n) in enumerate(zip(m_list, n_list)):
        if m == 0 or n == 0:
            assert int(a["n_corr"][i]) == 0 and (a["matches0"][i] == -1).all() and (bits(a["matching_scores0"][i]) == 0).all()
            assert (bits(a["pts0"][i]) == 0).all() and (bits(a["pts1"][i]) == 0).all()


PARAMS = [dict(iters=0), dict(iters=1), dict(iters=3), dict(iters=100), dict(bin_score=-5.0), dict(bin_score=8.0), dict(thr=0.0), dict(thr=0.9)]


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("par", PARAMS, ids=lambda p: "-".join(f"{k}{v}" for k, v in p.items()))
@pytest.mark.parametrize("ld", [70, 512])
def test_match_head_parameters_vs_float64_oracle(ld, par, variant):
    """one parameter at a time away from (bin_score 1, 20 iterations, threshold 0.2).  At 0 iterations the scores reach ~4e8 (rtol covers them)."""
    p = dict(bin_score=1.0, iters=20, thr=0.2); p.update(par)
    S, k0, k1, m_list, n_list = inputs(ld)
    o = launch(S.to(DEV), m_list, n_list, k0, k1, p["bin_score"], p["iters"], p["thr"], variant)
    n_ref = check_against_reference(o, S, k0, k1, m_list, n_list, p["bin_score"], p["iters"], p["thr"], f"ldS {ld} {par} variant {variant}")
    assert n_ref >= 1, "the reference itself has no match: the case compares nothing"


@pytest.mark.parametrize("ld", [8, 9])
def test_ties_go_to_the_lowest_index(ld):
    """S = 0 on 8 x 8: every entry of the coupling ties.  Row 0 and column 0 pick each other (the lowest index on both sides), every other row picks
    column 0 and is not mutual.  ldS 8: the sweep kernel; ldS 9 with counts 8: the general path (the 9th row and column hold 5, and are never read)"""
    S = torch.full((1, ld, ld), 5.0)
    S[:, :8, :8] = 0
    k0 = torch.arange(ld * 2, dtype=torch.float32).reshape(1, ld, 2) + 1; k1 = k0 + 100
    Z = NR.log_optimal_transport(torch.zeros(1, 8, 8, dtype=torch.float64), torch.tensor(1.0, dtype=torch.float64), 20)
    want = float(Z[0, 0, 0].exp())
    assert abs(want - 0.0471926) < 1e-6 and want > 0.01 + BAND
    for variant in (0, 1):
        o = launch(S.to(DEV), [8], [8], k0, k1, 1.0, 20, 0.01, variant)
        print(f"ties ldS {ld} variant {variant}: matches0 {o['matches0'][0].tolist()}, mscores0[0] {float(o['matching_scores0'][0, 0]):.7f} (float64: {want:.7f})")
        assert o["matches0"][0].tolist() == [0] + [-1] * (ld - 1)
        np.testing.assert_allclose(float(o["matching_scores0"][0, 0]), want, rtol=2e-4, atol=2e-5)
        assert (bits(o["matching_scores0"][0, 1:]) == 0).all()
        assert int(o["n_corr"][0]) == 1
        np.testing.assert_array_equal(o["pts0"][0, 0].numpy(), k0[0, 0].numpy()); np.testing.assert_array_equal(o["pts1"][0, 0].numpy(), k1[0, 0].numpy())
        assert (bits(o["pts0"][0, 1:]) == 0).all() and (bits(o["pts1"][0, 1:]) == 0).all()


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("ld", [70, 512])
def test_non_finite_score_empties_its_pair_only(ld, bad, variant):
    """one NaN / +inf inside pair 1's valid block: that pair has no arg-max anywhere and returns nothing (the row's index sentinel is not an address);
    pairs 0 and 2 are the bits of a launch without pair 1"""
    S, k0, k1, m_list, n_list = inputs(ld)
    S = S.clone()
    S[1, m_list[1] // 2, n_list[1] // 3] = bad
    o = launch(S.to(DEV), m_list, n_list, k0, k1, 1.0, 20, 0.2, variant)
    assert int(o["n_corr"][1]) == 0 and (o["matches0"][1] == -1).all() and (bits(o["matching_scores0"][1]) == 0).all()
    assert (bits(o["pts0"][1]) == 0).all() and (bits(o["pts1"][1]) == 0).all()
    keep = [0, 2]
    alone = launch(S[keep].to(DEV), [m_list[b] for b in keep], [n_list[b] for b in keep], k0[keep], k1[keep], 1.0, 20, 0.2, variant)
    for k in o:
        np.testing.assert_array_equal(bits(o[k][keep]), bits(alone[k][:2]), err_msg=k)
    assert int(alone["n_corr"][0]) > min(m_list[0], n_list[0]) // 4


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("offset", [1, 2])
def test_misaligned_scores_same_bits(offset, variant):
    """the 512 case with S one / two floats off a 16-byte boundary: no 16-byte load of S, and every output the bits of the aligned copy"""
    ld = 512
    S, k0, k1, m_list, n_list = inputs(ld)
    Sd = S.to(DEV)
    store = torch.empty(S.numel() + 4, device=DEV)
    Sm = store[offset:offset + S.numel()].view(S.shape)
    Sm.copy_(Sd)
    assert Sd.data_ptr() % 16 == 0 and Sm.data_ptr() % 16 == 4 * offset and Sm.is_contiguous()
    want = launch(Sd, m_list, n_list, k0, k1, 2.37, 20, 0.2, variant)
    got = launch(Sm, m_list, n_list, k0, k1, 2.37, 20, 0.2, variant)
    for k in want:
        np.testing.assert_array_equal(bits(got[k]), bits(want[k]), err_msg=k)
    assert int(want["n_corr"][0]) > 128
