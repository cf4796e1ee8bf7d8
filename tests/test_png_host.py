"""CPU: the host half of the device depth PNG decoder (csrc/host_decode.c mfr_host_png_parse, png_ops.parse) -- classification, the record,
the header mirror, the configuration key, the loader's refusal to decode silently on the host without a GPU -- and the test writer itself
(tests/png_craft.py, tests/png_cases.py) against PIL and zlib.  The parse also runs under AddressSanitizer / UBSan as a stand-alone C program
(tests/png_parse_main.c) over the crafted corpus with its single-byte and truncation mutations."""
import io
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest
from PIL import Image

import mapfree_reloc_amd  # noqa: F401
from mapfree_reloc_amd import datasets as D, png_ops as P
from mapfree_reloc_amd.config import get_cfg_defaults

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_craft as PC  # noqa: E402
from png_cases import MODES, VARIANTS, content, malformed_streams, small_raw, small_rows, SMALL_H, SMALL_W  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 37, 53


def crafted():
    a = content(H, W, 1)
    n = H * (1 + 2 * W)
    return {f"{m}-{v}": (a, PC.write_png(a, **dict(MODES[m], **VARIANTS[v](n)))) for m in sorted(MODES) for v in sorted(VARIANTS)}


def idat_payload(f):
    out, pos = b"", 8
    while pos < len(f):
        n, t = struct.unpack(">I4s", f[pos:pos + 8])
        if t == b"IDAT":
            out += f[pos + 8:pos + 8 + n]
        pos += 12 + n
    return out


def pil_png(arr, **kw):
    b = io.BytesIO()
    Image.fromarray(arr).save(b, format="PNG", **kw)
    return b.getvalue()


def test_writer_against_pil_and_zlib():
    for name, (a, f) in crafted().items():
        im = Image.open(io.BytesIO(f))
        assert im.mode == "I;16" and np.array_equal(np.asarray(im, dtype=np.uint16), a), name
    raw, stream = small_raw()
    assert zlib.decompress(stream) == raw == small_rows()
    im = Image.open(io.BytesIO(PC.assemble(SMALL_W, SMALL_H, stream)))
    assert np.array_equal(np.asarray(im, dtype=np.uint16), np.full((SMALL_H, SMALL_W), 0x1234, np.uint16))
    for name, (s, want) in malformed_streams().items():           # zlib refuses every one of them too (or stops short of the image)
        d = zlib.decompressobj()
        try:
            got = d.decompress(s)
            assert not d.eof or got != raw or name == "filter_type_5", name
        except zlib.error:
            pass


def test_ok_files_record_and_header():
    for name, (a, f) in crafted().items():
        st, h, rec = P.parse(f)
        payload = idat_payload(f)
        assert st == P.OK == h.status, name
        assert (h.width, h.height, h.bit_depth, h.color_type, h.interlace, h.stream_bytes) == (W, H, 16, 0, 0, len(payload)), name
        assert rec.size == h.record_bytes == (len(payload) + 8 + 15) // 16 * 16
        assert rec[:len(payload)].tobytes() == payload and not rec[len(payload):].any(), name
        assert zlib.decompress(payload) == PC.filter_rows(a, [y % 5 for y in range(H)])
    # ancillary chunks before, after and around the run are skipped; bytes after IEND are ignored
    a = content(H, W, 2)
    txt = PC.chunk(b"tEXt", b"k\0v")
    f = PC.write_png(a, idat=40, extra=[("head", txt), ("tail", txt), ("tail", PC.chunk(b"tIME", bytes(7)))]) + b"trailing"
    st, h, rec = P.parse(f)
    assert st == P.OK and rec[:h.stream_bytes].tobytes() == idat_payload(f[:-8])


def test_unsupported():
    g8 = np.arange(H * W, dtype=np.uint8).reshape(H, W)
    files = {"gray8": pil_png(g8), "rgb": pil_png(np.stack([g8] * 3, -1)), "adam7": PC.assemble(W, H, zlib.compress(bytes(8 * H * W)), interlace=1)}
    b = io.BytesIO()
    Image.fromarray(g8).convert("P").save(b, format="PNG")
    files["palette"] = b.getvalue()
    raw = PC.filter_rows(content(H, W, 3), [0] * H)
    co = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_DEFAULT_STRATEGY, b"dictionary")
    files["preset_dictionary"] = PC.assemble(W, H, co.compress(raw) + co.flush())
    files["window_64k"] = PC.assemble(W, H, bytes([0x88, 0x1C]) + zlib.compress(raw)[2:])
    for name, f in files.items():
        st, h, rec = P.parse(f)
        assert st == P.UNSUPPORTED == h.status and rec is None, name
    assert (0x88 * 256 + 0x1C) % 31 == 0


def test_invalid():
    a = content(3, 5, 4)
    f = PC.write_png(a, idat=9)
    stream = idat_payload(f)
    txt = PC.chunk(b"tEXt", b"k\0v")
    bad = {"signature": b"\x89PNX" + f[4:],
           "no_ihdr": PC.SIGNATURE + f[8 + 25:],
           "ihdr_second": PC.SIGNATURE + txt + f[8:],
           "no_idat": PC.SIGNATURE + PC.ihdr(5, 3) + PC.chunk(b"IEND"),
           "no_iend": PC.assemble(5, 3, stream, end=False),
           "split_run": PC.assemble(5, 3, stream, idat=9, extra=[(1, txt)]),
           "length_past_end": f[:8 + 25] + struct.pack(">I", len(f)) + f[8 + 25 + 4:],
           "length_2_31": f[:8 + 25] + struct.pack(">I", 0x80000000) + f[8 + 25 + 4:],
           "zero_width": PC.assemble(0, 3, stream), "zero_height": PC.assemble(5, 0, stream),
           "bit_depth_3": PC.assemble(5, 3, stream, bit_depth=3),
           "unknown_critical": PC.assemble(5, 3, stream, extra=[("head", PC.chunk(b"ABCD", b"x"))]),
           "stream_of_one_byte": PC.assemble(5, 3, stream[:1]),
           "zlib_method": PC.assemble(5, 3, bytes([0x77, 0x01]) + stream[2:]),
           "empty": b"", "signature_only": PC.SIGNATURE}
    for name, d in bad.items():
        assert P.parse(d)[0] == P.INVALID, name
    assert P.parse(f)[0] == P.OK
    end = len(f) - 12                                               # everything short of the whole IEND chunk is invalid
    for n in range(len(f)):
        assert P.parse(f[:n])[0] == P.INVALID, n
    assert end > 0


def test_capacity():
    f = PC.write_png(content(H, W, 5))
    st, h, rec = P.parse(f)
    need = h.record_bytes
    assert P.parse(f, cap=need)[0] == P.OK and np.array_equal(P.parse(f, cap=need)[2], rec)
    st, h2, r2 = P.parse(f, cap=need - 1)
    assert st == P.CAPACITY == h2.status and r2 is None
    hdr = np.zeros(P.HEADER_BYTES, np.uint8)
    slot = np.full(need + 32, 0xAA, np.uint8)
    st, nb = P.parse_into(f, hdr, slot[:need])
    assert st == P.OK and nb == need and (slot[need:] == 0xAA).all() and np.array_equal(slot[:need], rec)


def test_header_mirror_and_abi():
    lib = D._host_lib()
    assert lib is not None and lib.mfr_host_abi_version() == 4
    assert lib.mfr_host_png_header_bytes() == P.HEADER_BYTES == 32
    assert (P.OK, P.UNSUPPORTED, P.INVALID, P.CAPACITY, P.E_DATA, P.E_TRUNC, P.E_SIZE, P.E_CHECK) == (0, 1, 2, 3, 0x10, 0x20, 0x40, 0x80)
    hdr = open(os.path.join(ROOT, "include", "mfr_png.h")).read()
    for name in ("OK", "UNSUPPORTED", "INVALID", "CAPACITY", "E_DATA", "E_TRUNC", "E_SIZE", "E_CHECK"):
        v = getattr(P, name)
        assert f"#define MFR_PNG_{name} {v if v < 16 else hex(v)} " in hdr or f"#define MFR_PNG_{name} {v}\n" in hdr, name


def test_config_key_and_validator():
    assert get_cfg_defaults().HIP.DEPTH_DECODE == "host"
    assert D.check_depth_decode("host") == "host" and D.check_depth_decode("device") == "device"
    for v in ("gpu", "", None, "Device"):
        with pytest.raises(ValueError):
            D.check_depth_decode(v)
    with pytest.raises(ValueError):
        D.PairBatchLoader([], depth_decode="gpu")


@pytest.mark.parametrize("decode", ["thread", "process"])
def test_loader_device_route_refuses_without_gpu(tmp_path, decode):
    from mapfree_reloc_amd._lib import MfrLibraryError
    from tools.bench_fused_split import write_scene
    write_scene((str(tmp_path), 0, 2))
    cfg = get_cfg_defaults()
    cfg.DATASET.DATA_ROOT = str(tmp_path); cfg.DATASET.WIDTH = 540; cfg.DATASET.HEIGHT = 720; cfg.DATASET.ESTIMATED_DEPTH = "dptkitti"
    loader = D.PairBatchLoader(D.list_scenes(cfg, "test"), 2, prefetch=1, pin=False, workers=2, decode=decode, depth_decode="device")
    try:
        with pytest.raises(MfrLibraryError):
            for _ in D.DevicePrefetcher(loader, "cpu"):
                pass
    finally:
        loader.close()


def mutations(files):
    """every truncation and three single-byte changes per position"""
    for f in files:
        yield f
        for n in range(len(f)):
            yield f[:n]
        for i in range(len(f)):
            for v in (f[i] ^ 0xFF, f[i] ^ 0x01, 0):
                if v != f[i]:
                    yield f[:i] + bytes([v]) + f[i + 1:]


def test_parse_under_asan_ubsan_standalone(tmp_path):
    exe = str(tmp_path / "png_parse_main")
    # the sanitiser runtimes linked statically: the program needs nothing preloaded and runs in whatever environment the suite has
    r = subprocess.run(["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer",
                        "-fno-sanitize-recover=all",
                        "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "png_parse_main.c"),
                        os.path.join(ROOT, "map-free-reloc_amd", "csrc", "host_decode.c")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    a = content(SMALL_H, SMALL_W, 6)
    txt = PC.chunk(b"tEXt", b"k\0v")
    small = [PC.write_png(a), PC.write_png(a, idat=5, level=0), PC.write_png(a, idat=7, extra=[("head", txt), ("tail", txt)]),
             PC.assemble(SMALL_W, SMALL_H, small_raw()[1]), PC.assemble(SMALL_W, SMALL_H, small_raw()[1], idat=1),
             pil_png(np.zeros((2, 3), np.uint8)), PC.assemble(SMALL_W, SMALL_H, zlib.compress(bytes(64)), interlace=1)]
    whole = [f for _, f in crafted().values()] + [PC.assemble(SMALL_W, SMALL_H, s) for s, _ in malformed_streams().values()]
    corpus = tmp_path / "corpus.bin"
    n = 0
    with open(corpus, "wb") as out:
        for d in list(mutations(small)) + whole:
            out.write(struct.pack("<I", len(d)) + d)
            n += 1
    p = subprocess.run([exe, str(corpus)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and p.stdout.startswith("PNG_PARSE_OK"), (p.returncode, p.stdout[-300:], p.stderr[-3000:])
    inputs, ok = (int(v) for v in p.stdout.split()[1:3])
    assert inputs == n > 2000 and ok >= len(small) - 2 + len(whole)
