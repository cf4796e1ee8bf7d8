"""The host half of the device JPEG decoder (csrc/host_decode.c mfr_host_jpeg_parse, jpeg_ops.parse) against PIL on files PIL encodes,
its classification of unsupported / invalid input (also under AddressSanitizer + UndefinedBehaviorSanitizer), and the numpy restatement of
the device arithmetic (tests/jpeg_cpu_ref.py) against PIL's decode, bit for bit."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

import mapfree_reloc_amd  # noqa: F401
from mapfree_reloc_amd import jpeg_ops as J

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_cpu_ref as R  # noqa: E402
import jpeg_craft as JC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def enc(a, mode=None, **kw):
    b = io.BytesIO()
    Image.fromarray(a, mode).save(b, "JPEG", **kw)
    return b.getvalue()


def img(h, w, seed=0, smooth=False):
    rng = np.random.default_rng(seed)
    if smooth:
        y, x = np.mgrid[0:h, 0:w]
        return np.stack([(x * 5 + y) % 256, (y * 3) % 256, (x * y) % 256], -1).astype(np.uint8)
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def marker_segments(d):
    """(marker, start) of every marker outside the entropy-coded data, in file order"""
    out, i = [], 2
    while i < len(d):
        assert d[i] == 0xFF
        m = d[i + 1]
        out.append((m, i))
        if m == 0xD9:
            break
        n = int.from_bytes(d[i + 2:i + 4], "big")
        i += 2 + n
        if m == 0xDA:                                            # skip the entropy-coded data
            while not (d[i] == 0xFF and d[i + 1] not in (0x00,) and not 0xD0 <= d[i + 1] <= 0xD7):
                i += 1
    return out


def restuffed(h, rec):
    """the record's data stuffed again (0xFF -> 0xFF00) with RST0..7 between the segments"""
    seg = np.frombuffer(rec[:h.seg_table_bytes].tobytes(), dtype=np.uint32).reshape(-1, 2)[:h.nseg]
    data = rec[h.seg_table_bytes:h.seg_table_bytes + h.data_bytes].tobytes()
    out = b""
    for s in range(h.nseg):
        end = int(seg[s + 1, 0]) if s + 1 < h.nseg else h.data_bytes
        if s:
            out += bytes([0xFF, 0xD0 + (s - 1) % 8])
        out += data[int(seg[s, 0]):end].replace(b"\xff", b"\xff\x00")
    return out


CASES = [dict(quality=q, subsampling=s, optimize=o) for q in (50, 92, 100) for s in (0, 1, 2) for o in (False, True)] + \
        [dict(quality=85, subsampling=2, restart_marker_blocks=b) for b in (1, 4, 7)] + \
        [dict(quality=85, subsampling=1, restart_marker_rows=r) for r in (1, 3)]


@pytest.mark.parametrize("kw", CASES)
def test_parse_matches_pil(kw):
    for (h, w) in ((48, 64), (37, 29)):
        d = enc(img(h, w, seed=h), **kw)
        st, hd, rec = J.parse(d)
        assert st == J.OK
        pim = Image.open(io.BytesIO(d))
        assert (hd.width, hd.height) == pim.size
        assert [(hd.comp_id[c], hd.comp_h[c], hd.comp_v[c], hd.comp_tq[c]) for c in range(hd.ncomp)] == [tuple(x) for x in pim.layer]
        for t, q in pim.quantization.items():
            assert list(hd.qt[t]) == list(q)
        mx = hd.mcus_x
        ri = kw.get("restart_marker_blocks", kw.get("restart_marker_rows", 0) * mx)
        assert hd.restart_interval == ri
        n_rst = sum(1 for i in range(len(d) - 1) if d[i] == 0xFF and 0xD0 <= d[i + 1] <= 0xD7)
        assert hd.nseg == n_rst + 1
        sos = [s for m, s in marker_segments(d) if m == 0xDA][0]
        first = sos + 2 + int.from_bytes(d[sos + 2:sos + 4], "big")
        assert restuffed(hd, rec) == d[first:d.rindex(b"\xff\xd9")]     # unstuffed exactly: no 0xFF00 pair and no RSTn left over
        assert rec.size % 16 == 0 and not rec[hd.seg_table_bytes + hd.data_bytes:].any()


def test_gray_and_golden_files():
    d = enc(img(21, 30)[..., 0], "L", quality=80)
    st, hd, _ = J.parse(d)
    assert st == J.OK and hd.ncomp == 1 and hd.blocks_per_mcu == 1 and (hd.mcus_x, hd.mcus_y) == (4, 3)
    for name in sorted(os.listdir(os.path.join(ROOT, "tests", "golden"))):
        if name.startswith("gray_src_") and name.endswith(".jpg"):
            d = open(os.path.join(ROOT, "tests", "golden", name), "rb").read()
            st, hd, _ = J.parse(d)
            assert st in (J.OK, J.UNSUPPORTED)
            assert (hd.width, hd.height) == Image.open(io.BytesIO(d)).size or st == J.UNSUPPORTED


def bad_inputs():
    """(name, bytes, expected status)"""
    a = img(40, 56, seed=3)
    base = enc(a, quality=90, subsampling=2, restart_marker_blocks=3)
    out = [("progressive", enc(a, quality=90, progressive=True), J.UNSUPPORTED)]
    b = io.BytesIO()
    Image.fromarray(a).convert("CMYK").save(b, "JPEG", quality=90)
    out.append(("cmyk", b.getvalue(), J.UNSUPPORTED))
    b = io.BytesIO()
    Image.fromarray(a).save(b, "PNG")
    out.append(("png", b.getvalue(), J.INVALID))
    rng = np.random.default_rng(0)
    for k in range(20):
        out.append((f"random{k}", rng.integers(0, 256, int(rng.integers(0, 4000)), dtype=np.uint8).tobytes(), J.INVALID))
    out.append(("soi_random", b"\xff\xd8" + rng.integers(0, 256, 3000, dtype=np.uint8).tobytes(), J.INVALID))
    for m, s in marker_segments(base):
        for cut in (s, s + 1, s + 3, s + 5):
            if cut < len(base):
                out.append((f"cut_{m:02x}_{cut}", base[:cut], J.INVALID))
    a0, e0 = [s for m, s in marker_segments(base) if m == 0xDA][0], base.rindex(b"\xff\xd9")
    for f in (0.1, 0.5, 0.9):
        out.append((f"cut_data_{f}", base[:a0 + int(f * (e0 - a0))], J.INVALID))
    return out


def test_classification_unsupported_and_invalid():
    for name, d, want in bad_inputs():
        st, _, rec = J.parse(d)
        assert st == want, name
        assert rec is None
    d = enc(img(40, 56), quality=90)
    st, _, _ = J.parse(d, cap=64)
    assert st == J.CAPACITY


DRIVER = r'''
import ctypes, os, sys
lib = ctypes.CDLL(sys.argv[1])
vp, sz = ctypes.c_void_p, ctypes.c_size_t
lib.mfr_host_jpeg_parse.argtypes = [ctypes.c_char_p, sz, vp, vp, sz, vp]
lib.mfr_host_jpeg_header_bytes.restype = sz
hb = lib.mfr_host_jpeg_header_bytes()
n = 0
for name in sorted(os.listdir(sys.argv[2])):
    d = open(os.path.join(sys.argv[2], name), "rb").read()
    want = int(name.split("_")[0])
    for cap in (len(d) * 2 + 4096, 48):
        h = ctypes.create_string_buffer(hb)
        rec = ctypes.create_string_buffer(cap)
        nb = sz(0)
        st = lib.mfr_host_jpeg_parse(d, len(d), h, rec, cap, ctypes.byref(nb))
        assert st == want or (cap == 48 and st == 3), (name, st, want)
        n += 1
print("SANITIZED_OK", n)

# the crafted corpus (tests/jpeg_craft.py), every file whole, cut at each of its markers, and with each single byte of its SOF / SOS /
# DHT / DQT / DRI segments set to 0x00 and to 0xFF: the sanitised parse returns what the plain build (argv[4]) returns
plain = ctypes.CDLL(sys.argv[4])
plain.mfr_host_jpeg_parse.argtypes = lib.mfr_host_jpeg_parse.argtypes

def status(l, d, cap):
    h = ctypes.create_string_buffer(hb)
    rec = ctypes.create_string_buffer(cap)
    nb = sz(0)
    return l.mfr_host_jpeg_parse(d, len(d), h, rec, cap, ctypes.byref(nb))

def markers(d):
    # (marker, offset of the FF right before it, end of its segment) for every marker of a single-scan file
    out, i = [], 2
    while i + 1 < len(d):
        while d[i + 1] == 0xFF:
            i += 1
        m = d[i + 1]
        if m == 0xD9 or 0xD0 <= m <= 0xD7:
            out.append((m, i, i + 2))
            if m == 0xD9:
                break
            i += 2
        else:
            end = i + 2 + int.from_bytes(d[i + 2:i + 4], "big")
            out.append((m, i, end))
            i = end
        if m == 0xDA or 0xD0 <= m <= 0xD7:                      # entropy-coded data up to the next marker
            while not (d[i] == 0xFF and d[i + 1] != 0x00):
                i += 1
    return out

m = 0
for name in sorted(os.listdir(sys.argv[3])):
    d = open(os.path.join(sys.argv[3], name), "rb").read()
    cap = len(d) * 2 + 4096
    variants = [d]
    for mk, a, e in markers(d):
        variants.append(d[:a])
        variants.append(d[:a + 1])
        if mk in (0xC0, 0xC1, 0xDA, 0xC4, 0xDB, 0xDD):
            for i in range(a + 2, e):
                for v in (0x00, 0xFF):
                    if d[i] != v:
                        variants.append(d[:i] + bytes([v]) + d[i + 1:])
    for v in variants:
        st = status(lib, v, cap)
        assert st == status(plain, v, cap), (name, st)
        m += 1
    assert status(lib, d, 48) in (status(plain, d, cap), 3), name
print("CRAFTED_OK", m)
'''


def test_parse_under_asan_ubsan(tmp_path):
    so = str(tmp_path / "libmfr_host_asan.so")
    src = os.path.join(ROOT, "map-free-reloc_amd", "csrc", "host_decode.c")
    r = subprocess.run(["gcc", "-O1", "-g", "-fPIC", "-shared", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                        "-I" + os.path.join(ROOT, "include"), "-o", so, src], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("sanitizer build unavailable here: " + r.stderr[-200:])
    libasan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(libasan) or not os.path.exists(libasan):
        pytest.skip("libasan.so not found")
    inputs = tmp_path / "inputs"
    inputs.mkdir()
    good = [enc(img(48, 64, seed=s), quality=q, subsampling=sub, **kw) for s, (q, sub, kw) in
            enumerate(((92, 2, {}), (50, 0, dict(restart_marker_blocks=1)), (100, 1, dict(optimize=True))))]
    for k, d in enumerate(good):
        (inputs / f"0_good{k}").write_bytes(d)
    for k, (name, d, want) in enumerate(bad_inputs()):
        (inputs / f"{want}_{k}_{name}").write_bytes(d)
    crafted = tmp_path / "crafted"
    crafted.mkdir()
    n_crafted = 0
    for hw in ((48, 64), (37, 29), (1, 1), (17, 33)):
        for c in JC.corpus(*hw):
            (crafted / c.name).write_bytes(c.data)
            n_crafted += 1
    for name, d in JC.malformed():
        (crafted / f"malformed_{name}").write_bytes(d)
    from mapfree_reloc_amd import datasets
    plain = datasets._host_lib()._name
    env = dict(os.environ, LD_PRELOAD=libasan, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([sys.executable, "-c", DRIVER, so, str(inputs), str(crafted), plain], capture_output=True, text=True, env=env, timeout=1500)
    assert p.returncode == 0 and "SANITIZED_OK" in p.stdout, (p.stdout[-500:], p.stderr[-3000:])
    assert "CRAFTED_OK" in p.stdout and int(p.stdout.split("CRAFTED_OK")[1]) > 100 * n_crafted, p.stdout[-500:]


@pytest.mark.parametrize("sub", [0, 1, 2])
def test_cpu_restatement_equals_pil(sub):
    for k, (h, w) in enumerate(((16, 16), (5, 7), (33, 17), (17, 33), (1, 1), (2, 2), (40, 56))):
        for q in (50, 100):
            d = enc(img(h, w, seed=k, smooth=bool(k % 2)), quality=q, subsampling=sub, restart_marker_blocks=2 if q == 50 else 0)
            st, hd, rec = J.parse(d)
            assert st == J.OK
            assert np.array_equal(R.decode_rgb(hd, rec), np.asarray(Image.open(io.BytesIO(d)).convert("RGB"))), (h, w, q)
    d = enc(img(20, 30)[..., 0], "L", quality=80)
    st, hd, rec = J.parse(d)
    assert np.array_equal(R.decode_rgb(hd, rec)[..., 0], np.asarray(Image.open(io.BytesIO(d))))


def test_jpeg_decode_key_defaults_to_host_and_rejects_unknown_values():
    from mapfree_reloc_amd import datasets as D
    from mapfree_reloc_amd.config import get_cfg_defaults
    assert get_cfg_defaults().HIP.JPEG_DECODE == "host"
    assert D.check_jpeg_decode("device") == "device"
    with pytest.raises(ValueError):
        D.check_jpeg_decode("gpu")
    with pytest.raises(ValueError):
        D.PairBatchLoader([], 4, jpeg_decode="nvjpeg")
    assert D.PairBatchLoader([], 4).jpeg_decode == "host"


def test_pack_of_only_unsupported_files_reports_each_status():
    a = img(24, 32)
    pb = J.pack([enc(a, quality=90, progressive=True), b"not a jpeg"])
    assert list(pb.status) == [J.UNSUPPORTED, J.INVALID] and (pb.H, pb.W) == (0, 0)
