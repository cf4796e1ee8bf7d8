"""The device JPEG decoder (csrc/jpeg.hip, jpeg_ops.JpegDecoder) against PIL, bit for bit, on files PIL's encoder never writes
(tests/jpeg_craft.py; the same corpus tests/test_jpeg_crafted_host.py holds the parse and the numpy restatement to): fixed-length Huffman
codes, which never resynchronise, and staircase tables with codes of 10-16 bits and most of the code space unused, which make speculative
decodes fail all the time; 16-bit and re-numbered quantisation tables; Huffman ids swapped between the components; restart intervals of
one MCU; coefficients whose samples leave [0, 255].  RGB u8 = Image.open(f).convert("RGB"), gray plane = datasets.read_gray_plane(f, None);
every comparison is array_equal and every status an exact value."""
import io
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import mapfree_reloc_amd  # noqa: F401
from mapfree_reloc_amd import datasets as D, jpeg_ops as J

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_craft as JC  # noqa: E402

pytestmark = pytest.mark.gpu

H, W = 720, 540
SIZES = [(48, 64), (37, 29), (1, 1), (17, 33)]


def pil_rgb(d):
    return np.asarray(Image.open(io.BytesIO(d)).convert("RGB"))


def pil_gray(d):
    return D.read_gray_plane(io.BytesIO(d), None)


def check(files, dec=None, **kw):
    """decode one batch; every file: status 0, RGB and gray plane equal to PIL's -> (gray, rgb, decoder)"""
    dec = dec or J.JpegDecoder("cuda", **kw)
    gray, st, rgb = dec.decode(files, rgb=True)
    torch.cuda.synchronize()
    gray, st, rgb = gray.cpu().numpy(), st.cpu().numpy(), rgb.cpu().numpy()
    for i, f in enumerate(files):
        assert st[i] == 0, (i, st[i])
        ref = pil_rgb(f)
        assert np.array_equal(rgb[i], ref), (i, int((rgb[i] != ref).any(-1).sum()))
        assert np.array_equal(gray[i, 0], pil_gray(f)), i
    return gray, rgb, dec


def supported(hw, **kw):
    return [c for c in JC.corpus(hw[0], hw[1], **kw) if c.cls == JC.SUPPORTED]


def large(sampling, tables, restart=0, coefs=None, seed=3):
    """a 720 x 540 file: tables 'flat' or 'staircase' on every component"""
    base, rng, T, grids = JC.base_file(H, W, sampling, seed)
    names = ("fdc", "fac", "fdc", "fac") if tables == "flat" else ("sdc", "sac", "ddc", "sac2")
    base["dht"] = [[(i & 1, i >> 1, *T[n])] for i, n in enumerate(names)]
    if coefs == "range_limit":
        q = [300] * 64
        base["dqt"] = [[(0, 1, q)], [(1, 0, JC.Q_CHROMA)]]
        base["coefs"] = [JC.range_limit_coefs(rng, grids[0], q)] + base["coefs"][1:]
    return JC.craft(**base, restart=restart)


@pytest.mark.parametrize("hw", SIZES)
def test_corpus_of_one_size_on_every_entropy_route(hw):
    """the whole supported corpus as one mixed batch: the default subsequence length, 32-bit subsequences (every code of the staircase
    tables crosses subsequences; the flat tables take many rounds) and the sequential route equal PIL and each other"""
    files = [c.data for c in supported(hw)]
    assert len(files) > 100
    g_def, r_def, _ = check(files)
    g32, r32, dec32 = check(files, subseq_bits=32)
    g_seq, r_seq, dseq = check(files, subseq_bits=8 * max(len(f) for f in files) + 64)
    assert np.array_equal(g_def, g32) and np.array_equal(g_def, g_seq) and np.array_equal(r_def, r32) and np.array_equal(r_def, r_seq)
    assert dseq.rounds.cpu().numpy().max() == 1
    if hw != (1, 1):
        assert dec32.rounds.cpu().numpy().max() > 1


def test_map_free_size_flat_and_staircase_tables_and_restart_interval_one():
    """720 x 540: streams that never resynchronise (flat tables), streams whose wrong-state decodes hit unassigned codes all the time
    (staircase tables: a failed speculative decode leaves its successor's guess), and up to 6120 restart segments"""
    files = [large("420", "flat"), large("420", "staircase"), large("444", "flat", restart=1), large("444", "staircase", restart=1),
             large("gray", "flat", restart=1), large("422", "staircase"), large("422", "flat", restart=7)]
    heads = [J.parse(f)[1] for f in files]
    assert max(h.nseg for h in heads) == 6120 and heads[0].nseg == 1
    _, _, dec = check(files)
    rounds = dec.rounds.cpu().numpy()
    print("rounds at the default subsequence length (flat 4:2:0, staircase 4:2:0, ...):", rounds.tolist())
    assert rounds[0] > 1, rounds                                                 # the flat-table stream needed the fixed point
    for i in (0, 1, 5):                                                          # one at a time: the same planes
        g1, _ = J.JpegDecoder("cuda").decode([files[i]])
        assert np.array_equal(g1[0, 0].cpu().numpy(), pil_gray(files[i]))


def test_staircase_tables_with_short_subsequences():
    """codes of up to 16 bits against 32-bit subsequences: almost every speculative start is wrong and most of them meet a code no table
    assigns; the image still comes out with status 0 and PIL's pixels"""
    files = [c.data for hw in ((48, 64),) for c in supported(hw) if "staircase" in c.name or "four_tables" in c.name]
    assert len(files) >= 8
    _, _, dec = check(files, subseq_bits=32)
    assert dec.rounds.cpu().numpy().min() > 1
    check(files, subseq_bits=16)


def test_range_limit_and_16_bit_quantisation_tables():
    """the IDCT kernel: samples far outside [0, 255] are clamped as PIL's SIMD inverse DCT clamps them, 16-bit table entries multiply
    without truncation; one 720 x 540 file so that the blocks spread over many workgroups"""
    files = [c.data for c in supported((48, 64)) if "range_limit" in c.name or "q_16bit" in c.name or "dc_plus_minus" in c.name or
             "ac_10_bit" in c.name]
    assert len(files) == 4 * 7
    check(files)
    _, rgb, _ = check([large("420", "flat", coefs="range_limit"), large("gray", "staircase", coefs="range_limit")])
    assert float(((rgb[1] == 0) | (rgb[1] == 255)).mean()) >= 0.1                # the gray file: a tenth of the samples at the limits


def test_table_id_permutations_select_the_right_tables():
    """blk_dc / blk_ac in LDS and comp_tq & 3: luma on Huffman tables 1, DC and AC ids differing inside a component, quantisation ids 3 / 2 / 0"""
    files = [c.data for hw in ((48, 64), (37, 29)) for c in supported(hw) if "huff_ids" in c.name or "huff_dc_ac" in c.name or "q_ids" in c.name
             or "q_two" in c.name or "unused_tables" in c.name]
    assert len(files) == 2 * 4 * 5
    same = {}
    for f in files:
        same.setdefault((J.parse(f)[1].height, J.parse(f)[1].width), []).append(f)
    for batch in same.values():
        check(batch)


def test_batch_of_64_crafted_and_pil_files_equals_single_decodes():
    rng = np.random.default_rng(11)
    crafted = [c.data for c in supported((48, 64))]
    files = crafted[::max(1, len(crafted) // 40)][:40]
    for i in range(64 - len(files)):
        b = io.BytesIO()
        a = rng.integers(0, 256, (48, 64, 3), dtype=np.uint8)
        if i % 7 == 3:
            Image.fromarray(a[..., 0]).save(b, "JPEG", quality=80)
        else:
            kw = dict(quality=int(rng.integers(30, 101)), subsampling=i % 3, optimize=bool(i % 2))
            if i % 5 == 0:
                kw["restart_marker_blocks"] = 1 + i % 4
            Image.fromarray(a).save(b, "JPEG", **kw)
        files.append(b.getvalue())
    order = rng.permutation(64)
    files = [files[i] for i in order]
    assert len(files) == 64
    g_all, r_all, dec = check(files)
    for i, f in enumerate(files):
        g1, st1, r1 = dec.decode([f], rgb=True)
        assert int(st1[0]) == 0 and np.array_equal(g1[0].cpu().numpy(), g_all[i]) and np.array_equal(r1[0].cpu().numpy(), r_all[i]), i


def test_status_classes_in_one_batch():
    """one file of every kind PIL decodes and the device does not (UNSUPPORTED: plane untouched) and of every kind PIL refuses (INVALID),
    each between good files that still equal PIL"""
    cases = JC.corpus(37, 29)
    odd = [c for c in cases if c.cls != JC.SUPPORTED and (c.name.startswith("444") or c.name.startswith("gray"))]
    assert {c.cls for c in odd} == {JC.UNSUPPORTED, JC.BROKEN} and len(odd) >= 12
    good = [c.data for c in cases if c.cls == JC.SUPPORTED][:len(odd) + 1]
    files, want = [good[0]], [J.OK]
    for c, g in zip(odd, good[1:]):
        files += [c.data, g]
        want += [J.UNSUPPORTED if c.cls == JC.UNSUPPORTED else J.INVALID, J.OK]
    out = torch.full((len(files), 1, 37, 29), 7.0, device="cuda")
    gray, st = J.JpegDecoder("cuda").decode(J.pack(files, 37, 29), out=out)
    assert st.cpu().numpy().tolist() == want
    g = gray.cpu().numpy()
    for i, f in enumerate(files):
        if want[i] == J.OK:
            assert np.array_equal(g[i, 0], pil_gray(f)), i
        else:
            assert (g[i] == 7.0).all(), i


def test_file_of_another_size_gets_e_size_alone():
    a, b = supported((48, 64), samplings=("420",)), supported((37, 29), samplings=("420",))
    files = [a[0].data, a[1].data, b[0].data, a[2].data]
    out = torch.full((4, 1, 48, 64), 7.0, device="cuda")
    gray, st = J.JpegDecoder("cuda").decode(files, out=out)
    assert st.cpu().numpy().tolist() == [0, 0, J.E_SIZE, 0]
    g = gray.cpu().numpy()
    assert (g[2] == 7.0).all()
    for i in (0, 1, 3):
        assert np.array_equal(g[i, 0], pil_gray(files[i]))


def test_malformed_streams():
    """the fixed list tests/test_jpeg_crafted_host.py first runs through the restatement (every index in range): a non-zero status, or
    PIL's pixels.  Trailing bytes and a run past coefficient 63 decode as PIL decodes them; a segment one MCU short is E_TRUNC, a code no
    table assigns E_HUFF; the good files around them are untouched by it."""
    bad = dict(JC.malformed())
    good = [c.data for c in supported((16, 32), samplings=("gray",))[:3]]
    names = list(bad)
    files = [good[0]] + [x for n, g in zip(names, good[1:] + good[:2]) for x in (bad[n], g)]
    for f in files:
        assert J.parse(f)[0] == 0                                                # well-formed at the marker level: the device must catch it
    for kw in (dict(), dict(subseq_bits=32), dict(subseq_bits=1 << 16)):
        gray, st, rgb = J.JpegDecoder("cuda", **kw).decode(files, rgb=True)
        st, rgb = st.cpu().numpy(), rgb.cpu().numpy()
        for i, f in enumerate(files):
            if i % 2 == 0:
                assert st[i] == 0 and np.array_equal(rgb[i], pil_rgb(f)), (kw, i)
                continue
            name = names[i // 2]
            assert st[i] != 0 or np.array_equal(rgb[i], pil_rgb(f)), (kw, name)
            if name == "segment_one_mcu_short":
                assert st[i] & J.E_TRUNC and not st[i] & ~(J.E_TRUNC | J.E_HUFF), (kw, name, st[i])
            if name == "code_in_no_table":
                assert st[i] & J.E_HUFF and not st[i] & ~(J.E_TRUNC | J.E_HUFF), (kw, name, st[i])
            if name in ("trailing_bytes", "run_overflow"):
                assert st[i] == 0, (kw, name, st[i])
