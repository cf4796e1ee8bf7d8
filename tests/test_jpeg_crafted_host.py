"""The host half of the device JPEG decoder and the numpy restatement of its arithmetic (tests/jpeg_cpu_ref.py) against PIL on files PIL's
own encoder never writes (tests/jpeg_craft.py): fixed-length and 16-bit Huffman codes, 16-bit and re-numbered quantisation tables, any
component ids and colour markers, fill bytes, zero padding, restart intervals down to one MCU, coefficients that leave the sample range.
Three invariants hold for the whole corpus:
  A  the parse says OK  =>  PIL opens the file without a warning and the restatement equals PIL in every byte (RGB and the gray plane);
  B  the file is in the supported class  =>  the parse says OK;
  C  PIL decodes the file but it is outside that class  =>  UNSUPPORTED (never OK, never INVALID);
and a file PIL refuses (a Huffman table libjpeg calls bogus) is INVALID.  No comparison has a tolerance."""
import io
import os
import sys
import warnings

import numpy as np
import pytest
from PIL import Image

import mapfree_reloc_amd  # noqa: F401
from mapfree_reloc_amd import datasets as D, jpeg_ops as J

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_cpu_ref as R  # noqa: E402
import jpeg_craft as JC  # noqa: E402

SIZES = [(48, 64), (37, 29), (1, 1), (17, 33)]                                   # (height, width)


def pil_rgb(d):
    """PIL's RGB decode with every warning an error -> array, or the exception"""
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        try:
            return np.asarray(Image.open(io.BytesIO(d)).convert("RGB"))
        except Exception as e:                                                   # noqa: BLE001 (whatever PIL raises is the answer)
            return e


def violations(case):
    """the invariants one file breaks, as strings"""
    ref = pil_rgb(case.data)
    st, h, rec = J.parse(case.data)
    bad = []
    if st == J.OK:                                                               # A
        if isinstance(ref, Exception):
            bad.append(f"A: parse OK, PIL raises {type(ref).__name__}: {ref}")
        else:
            got = R.decode_rgb(h, rec)
            if not np.array_equal(got, ref):
                bad.append(f"A: {int((got != ref).any(-1).sum())} of {ref.shape[0] * ref.shape[1]} pixels differ from PIL, max "
                           f"{int(np.abs(got.astype(int) - ref.astype(int)).max())}")
            elif not np.array_equal(D.gray_plane(got), D.read_gray_plane(io.BytesIO(case.data), None)):
                bad.append("A: gray plane differs")
    if case.cls == JC.SUPPORTED and st != J.OK:                                  # B
        bad.append(f"B: supported file, parse status {st}")
    if case.cls == JC.UNSUPPORTED:                                               # C
        if isinstance(ref, Exception):
            bad.append(f"C: the test expects PIL to decode this file: {ref}")
        if st != J.UNSUPPORTED:
            bad.append(f"C: PIL decodes it, outside the supported class, parse status {st}")
    if case.cls == JC.BROKEN:
        if not isinstance(ref, Exception):
            bad.append("the test expects PIL to refuse this file")
        if st != J.INVALID:
            bad.append(f"PIL refuses it, parse status {st}")
    return bad


@pytest.mark.parametrize("sampling", list(JC.SAMPLINGS))
@pytest.mark.parametrize("hw", SIZES)
def test_crafted_corpus_invariants(hw, sampling):
    cases = JC.corpus(hw[0], hw[1], samplings=(sampling,))
    assert len(cases) >= 35
    failed = {c.name: v for c in cases for v in [violations(c)] if v}
    assert not failed, "\n".join(f"{k}: {v}" for k, v in failed.items())


def test_corpus_holds_every_class_and_every_feature():
    cases = JC.corpus(37, 29)
    assert {c.cls for c in cases} == {JC.SUPPORTED, JC.UNSUPPORTED, JC.BROKEN}
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    ok = [c for c in cases if c.cls == JC.SUPPORTED]
    heads = [J.parse(c.data)[1] for c in ok]
    assert any(max(h.comp_tq[:h.ncomp]) == 3 for h in heads) and any(np.asarray(h.qt).max() > 255 for h in heads)
    assert any(any(h.ac[t].bits[15] for t in (0, 1)) for h in heads) and any(any(h.dc[t].bits[9:] for t in (0, 1)) for h in heads)
    assert any(h.nseg > 8 for h in heads)                                        # RST7 -> RST0
    assert any(h.comp_td[0] != h.comp_ta[0] for h in heads) and any(h.comp_td[0] == 1 for h in heads)


@pytest.mark.parametrize("sampling", ["420", "gray"])
def test_range_limit_files_saturate_inside_the_coefficient_bound(sampling):
    """blocks with sum_k |coef_k q_k| in (2048, 4096]: PIL clamps what leaves [0, 255] (its SIMD inverse DCT packs with signed saturation;
    libjpeg's C code wraps modulo 1024 in its range-limit table), and at least a tenth of the pixels sit at 0 or 255"""
    cases = [c for c in JC.corpus(48, 64, samplings=(sampling,)) if "range_limit" in c.name]
    assert len(cases) == 3
    for c in cases:
        st, h, rec = J.parse(c.data)
        assert st == J.OK
        coef = R.coefficients(h, rec)
        luma = coef.reshape(h.total_mcus, h.blocks_per_mcu, 64)[:, :h.comp_bw[0] * h.comp_bh[0]].reshape(-1, 64)   # natural order, as qt
        sums = (np.abs(luma) * np.asarray(h.qt[h.comp_tq[0]], dtype=np.int64)).sum(-1)
        assert sums.min() > 2048 and sums.max() <= JC.COEF_BOUND, (c.name, sums.min(), sums.max())
        assert np.array_equal(R.decode_rgb(h, rec), pil_rgb(c.data)), c.name
        y = R.planes(h, coef)[0][:h.height, :h.width]
        sat = float(((y == 0) | (y == 255)).mean())
        print(f"{c.name}: {sat:.3f} of the luma samples at 0 or 255")
        assert sat >= 0.1, (c.name, sat)


def test_pil_clamps_out_of_range_samples():
    """one block, DC only, dequantised 8 * 700: the sample is 700 + 128.  The SIMD inverse DCT of libjpeg-turbo saturates it to 255; the C
    inverse DCT looks ((700 + 128) mod 1024) up in the range-limit table and gives 0 there.  The project restates the first."""
    c = np.zeros((1, 1, 64), dtype=np.int64)
    for dc, want in ((700, 255), (-700, 0)):
        c[0, 0, 0] = dc
        d = JC.craft(8, 8, [(1, 1, 1, 0, 0, 0)], [c], [[(0, 0, [8] * 64)]], [[(0, 0, *JC.flat_dc()), (1, 0, *JC.flat_ac())]])
        got = np.unique(np.asarray(Image.open(io.BytesIO(d))))
        assert got.tolist() == [want], \
            f"PIL decodes an out-of-range sample ({dc * 8} + 128) to {got.tolist()}, not {want}: this PIL's libjpeg runs without the SIMD " \
            f"inverse DCT (saturating pack), which the device decoder and tests/jpeg_cpu_ref.py restate"
        st, h, rec = J.parse(d)
        assert st == J.OK and np.unique(R.decode_rgb(h, rec)).tolist() == [want]


def test_short_jfif_payload_does_not_count_as_jfif():
    """libjpeg takes an APP0 as JFIF only with >= 14 bytes of payload: ids 'R','G','B' behind a 7-byte JFIF payload are RGB to PIL"""
    cases = {c.name.split("_", 2)[2]: c for c in JC.corpus(37, 29, samplings=("444",))}
    assert J.parse(cases["ids_rgb_short_jfif"].data)[0] == J.UNSUPPORTED
    assert J.parse(cases["ids_rgb_full_jfif"].data)[0] == J.OK
    assert J.parse(cases["ids_rgb_no_jfif"].data)[0] == J.UNSUPPORTED


def test_huffman_tables_libjpeg_refuses_are_invalid_only_when_a_scan_uses_them():
    cases = {c.name.split("_", 2)[2]: c for c in JC.corpus(17, 33, samplings=("gray",))}
    for name in ("huff_all_ones_code", "huff_all_ones_code_16_bits", "huff_dc_category_16"):
        assert isinstance(pil_rgb(cases[name].data), Exception), name
        assert J.parse(cases[name].data)[0] == J.INVALID, name
    # the same bogus table under id 1, which a gray scan does not use: PIL decodes the file, and so does the parse
    base, _, T, _ = JC.base_file(17, 33, "gray")
    ones = JC.table_from_lengths({s: 4 for s in range(16)})
    d = JC.craft(**{**base, "dht": base["dht"][:2] + [[(0, 1, *ones)], base["dht"][3]]})
    assert not violations(JC.Case("unused_bogus_table", d, JC.SUPPORTED))


def test_malformed_files_keep_every_index_in_range():
    """the files the GPU test also decodes, first through the restatement: it either refuses the stream (an assertion on a bad code or a
    short segment) or decodes it with every index in range (numpy raises IndexError otherwise) to PIL's pixels"""
    seen = {}
    for name, d in JC.malformed():
        st, h, rec = J.parse(d)
        assert st == J.OK, name                                                  # well-formed at the marker level
        try:
            got = R.decode_rgb(h, rec)
        except AssertionError as e:
            seen[name] = str(e)
            continue
        seen[name] = "decoded"
        ref = pil_rgb(d)                                                         # PIL decodes these without a warning
        assert not isinstance(ref, Exception) and np.array_equal(got, ref), (name, ref)
    assert seen["trailing_bytes"] == "decoded" and seen["run_overflow"] == "decoded", seen
    assert seen["segment_one_mcu_short"] != "decoded" and seen["code_in_no_table"] != "decoded", seen
