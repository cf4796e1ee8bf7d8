"""Baseline JPEG decode on the GPU (csrc/jpeg.hip, include/mfr_hip.h mfr_jpeg_*), with the header parse on the host (csrc/host_decode.c,
libmfr_host.so mfr_host_jpeg_parse; layout in include/mfr_jpeg.h).  The result is the loaders' gray plane of the file,
datasets.read_gray_plane(path, None), bit for bit: PIL's RGB decode (libjpeg-turbo, libjpeg 6.2 API: JDCT_ISLOW, fancy upsampling,
no DCT scaling), then datasets.luma_u8, then / 255 in float32.  Torch only provides memory and the stream.

| stage | what | where |
|---|---|---|
| parse | SOI / APPn / DQT / SOF0-1 (8-bit) / DHT / DRI / SOS / EOI; quantisation tables in natural order; canonical Huffman tables (T.81 C.2) as a 9-bit look-up plus maxcode per length; entropy data unstuffed, RSTn removed, one {byte offset, MCU count} per restart segment | host, plain C |
| entropy | per restart segment, subsequences of S bits decoded speculatively from a guessed state (bit offset, zig-zag index, block in MCU) and re-decoded from their predecessor's exit state until nothing changes (Weissenberger & Schmidt 2018); exclusive scan of the blocks each subsequence completes; a final pass writes int16 coefficients, DC as differences | one workgroup per image |
| DC | per-component prefix sum of the DC differences, reset at every restart segment | same workgroup |
| IDCT | dequantise, libjpeg's JDCT_ISLOW integer inverse DCT (13-bit constants, 2 fractional bits between the passes), its output clamped to [-128, 127] then + 128 (the signed-saturating pack of libjpeg-turbo's SIMD routine, which PIL runs; not the modulo-1024 range-limit table of libjpeg's C code) into u8 planes padded to whole MCUs | 8 lanes per block |
| colour | libjpeg's fancy (triangle) upsampling for h2v1 / h2v2 (edges replicate the last real row / column), fixed-point YCbCr -> RGB (16-bit tables, ONE_HALF rounding), luma (19595 R + 38470 G + 7471 B + 2^15) >> 16, / 255f | one lane per pixel |

Files the parse calls unsupported (progressive, arithmetic, 12-bit, multi-scan, CMYK / RGB colour, other sampling, Huffman table ids 2 / 3,
which only an extended-sequential SOF1 file may use) are the caller's to decode on the host; `decode` reports them per image in `status` (1)
and leaves their planes untouched.  The parse takes: SOF0 / SOF1 at 8 bits, one interleaved scan (or one component), gray or YCbCr at
4:4:4 / 4:2:2 / 4:2:0, quantisation table ids 0-3 with 8- or 16-bit entries, Huffman table ids 0 / 1, any component ids.  Three components
are YCbCr unless an Adobe APP14 marker says transform 0, or, with neither an Adobe marker nor a JFIF APP0 (payload >= 14 bytes, as libjpeg
asks), the ids spell 'R', 'G', 'B'.  A Huffman table libjpeg refuses ("bogus Huffman table": the all-ones code of a length assigned, the
code space over-subscribed, a DC category above 15) makes the file invalid when the scan uses it.

Bit-exactness with PIL is promised for files in which every block has sum_k |coef_k q_k| <= 4096 (quantised coefficient times its table
entry), which every encoder working from 8-bit pixels satisfies: the first IDCT pass scales a term by at most ~1.39 * 4, so its outputs
stay below 2^15 and the 16-bit intermediates of libjpeg-turbo's SIMD IDCT cannot saturate.  Beyond that bound PIL's result depends on
that saturation, which is not restated here.  tests/jpeg_craft.py writes files up to the bound; tests/test_jpeg_crafted_host.py and
tests/test_gpu_jpeg_crafted.py compare them with PIL.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib

OK, UNSUPPORTED, INVALID, CAPACITY = 0, 1, 2, 3
E_HUFF, E_TRUNC, E_SIZE = 0x10, 0x20, 0x40


class Huff(C.Structure):
    _fields_ = [("maxcode", C.c_int32 * 20), ("valoff", C.c_int32 * 20), ("fast", C.c_uint16 * 512), ("bits", C.c_uint8 * 16),
                ("val", C.c_uint8 * 256)]


class Header(C.Structure):
    """include/mfr_jpeg.h mfr_jpeg_header"""
    _fields_ = [(f, C.c_int32) for f in ("status", "width", "height", "ncomp", "hmax", "vmax", "mcus_x", "mcus_y", "blocks_per_mcu",
                                         "restart_interval", "nseg", "total_mcus", "seg_table_bytes", "data_bytes", "record_bytes",
                                         "adobe_transform")] + \
               [(f, C.c_int32 * 4) for f in ("comp_id", "comp_h", "comp_v", "comp_tq", "comp_td", "comp_ta", "comp_bw", "comp_bh",
                                             "comp_off", "plane_w", "plane_h", "plane_off", "down_w", "down_h")] + \
               [("mcu_comp", C.c_int32 * 12), ("qt", (C.c_uint16 * 64) * 4), ("dc", Huff * 2), ("ac", Huff * 2)]


HEADER_BYTES = C.sizeof(Header)


def _host():
    from . import datasets
    lib = datasets._host_lib()
    if lib is None:
        raise _lib.MfrLibraryError("csrc/libmfr_host.so (ABI 4) not found: build it with __graft_entry__.build()")
    assert lib.mfr_host_jpeg_header_bytes() == HEADER_BYTES, "jpeg_ops.Header does not mirror include/mfr_jpeg.h"
    return lib


def record_bound(nbytes, nseg=1):
    """bytes a file of `nbytes` needs as a record when it has at most `nseg` restart segments (always enough: nseg <= nbytes)"""
    return int(_host().mfr_host_jpeg_record_bound(int(nbytes), int(nseg)))


def parse(data, cap=None):
    """one file's bytes -> (status, Header, record u8 array or None).  cap: record buffer size (default: always enough)"""
    lib = _host()
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    cap = record_bound(buf.size, buf.size // 3 + 1) if cap is None else int(cap)        # a segment takes >= 1 byte + its RSTn
    rec = np.zeros(max(cap, 16), dtype=np.uint8)
    h = Header()
    nb = C.c_size_t(0)
    st = lib.mfr_host_jpeg_parse(buf.ctypes.data, buf.size, C.byref(h), rec.ctypes.data, cap, C.byref(nb))
    return st, h, (rec[:nb.value] if st == OK else None)


def parse_into(data, header_row, slot):
    """parse straight into a batch: header_row = u8 [HEADER_BYTES] view, slot = u8 view (16-aligned) -> (status, record bytes)"""
    lib = _host()
    buf = np.frombuffer(data, dtype=np.uint8)
    nb = C.c_size_t(0)
    st = lib.mfr_host_jpeg_parse(buf.ctypes.data, buf.size, header_row.ctypes.data, slot.ctypes.data, slot.size, C.byref(nb))
    return st, nb.value


class PackedBatch:
    """a batch for the device: headers u8 [n, HEADER_BYTES], records u8 [sum] (each 16-aligned), offsets i64 [n + 1], parse status i32 [n]"""

    def __init__(self, headers, records, offsets, status, H, W):
        self.headers, self.records, self.offsets, self.status, self.H, self.W = headers, records, offsets, status, H, W

    @property
    def n(self):
        return len(self.status)


def pack(files, H=None, W=None):
    """list of file bytes -> PackedBatch.  H, W: the batch's size (default: the first parsed file's; 0 x 0 when none parses)"""
    heads, recs, status = [], [], []
    for f in files:
        st, h, rec = parse(f)
        if st == OK and H is None:
            H, W = h.height, h.width
        heads.append(np.frombuffer(bytes(h), dtype=np.uint8))
        recs.append(rec if rec is not None else np.zeros(0, np.uint8))
        status.append(st)
    offsets = np.zeros(len(files) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([r.size for r in recs])
    return PackedBatch(np.stack(heads) if heads else np.zeros((0, HEADER_BYTES), np.uint8),
                       np.concatenate(recs + [np.zeros(16, np.uint8)]), offsets, np.asarray(status, np.int32), H or 0, W or 0)


class JpegDecoder:
    """JpegDecoder(device).decode(files: list[bytes] | PackedBatch, out=None, rgb=False, resize=None) -> (gray [n,1,H,W] f32, status [n] i32)
    on the device (plus rgb [n,H,W,3] u8 with rgb=True; resize=(w, h): gray [n,1,h,w], resized on the device).  status: 0 ok, 1 unsupported (host's to decode: its plane is left as it was), 2 / 3
    invalid / capacity at the parse, E_HUFF / E_TRUNC / E_SIZE bits from the device.  subseq_bits: test-only subsequence length (0 =
    default).  No CPU fallback: without libmfr_hip.so or a GPU it raises MfrLibraryError."""

    def __init__(self, device="cuda", subseq_bits=0):
        self.device = torch.device(device)
        self.subseq_bits = int(subseq_bits)
        self._ws = None
        self._resizer = None
        self.rounds = None

    def workspace(self, n, H, W, max_record):
        lib = _lib.load(require_gpu=True)
        nb = lib.mfr_jpeg_workspace_bytes(n, H, W, int(max_record), self.subseq_bits)
        if nb == 0:
            raise ValueError(f"JPEG: unsupported batch {n}x{H}x{W}, record {max_record} B, S {self.subseq_bits}")
        if self._ws is None or self._ws.numel() < nb:
            self._ws = torch.empty(nb, dtype=torch.uint8, device=self.device)
        return self._ws

    def decode_device(self, headers, records, offsets, n, H, W, max_record, out, status, rgb=None):
        """the device half on tensors already on the device (headers u8 [n, HEADER_BYTES], records u8, offsets i64 [n + 1]), launched on
        torch's current stream; the workspace and the round counters are marked as used by that stream (the caching allocator then does
        not hand them to other work before these launches are done, whichever stream allocated them)"""
        _lib.load(require_gpu=True)
        ws = self.workspace(n, H, W, max_record)
        self.rounds = torch.zeros(max(n, 1), dtype=torch.int32, device=self.device)
        cur = torch.cuda.current_stream(self.device)
        _lib.call("mfr_jpeg_decode", headers, records, offsets, n, H, W, int(max_record), out, rgb, status, self.rounds, ws, ws.numel(), self.subseq_bits,
                  stream=cur.cuda_stream)
        ws.record_stream(cur)
        self.rounds.record_stream(cur)

    def decode(self, files, out=None, rgb=False, resize=None):
        """resize = (w, h): the planes are datasets.read_gray_plane(path, (w, h)) -- the files are decoded at their own size into RGB scratch
        and resized on the device (GrayResizer, csrc/resize.hip); `out` is then [n,1,h,w] and the RGB returned with rgb=True stays at the
        files' size.  resize None (or the files' own size): the decoder's gray plane, as before."""
        _lib.load(require_gpu=True)
        pb = files if isinstance(files, PackedBatch) else pack(files)
        n, H, W = pb.n, pb.H, pb.W
        dev = self.device
        resized = resize is not None and (int(resize[0]), int(resize[1])) != (W, H)
        oh, ow = (int(resize[1]), int(resize[0])) if resized else (H, W)
        if out is None:
            out = torch.zeros(n, 1, oh, ow, dtype=torch.float32, device=dev)
        assert out.shape == (n, 1, oh, ow) and out.dtype == torch.float32 and out.is_contiguous()
        rgb_t = torch.zeros(n, H, W, 3, dtype=torch.uint8, device=dev) if (rgb or resized) else None
        status = torch.from_numpy(pb.status.copy()).to(dev)
        if n and bool((pb.status == OK).any()):                # nothing the device takes (e.g. only progressive files): statuses only
            max_rec = max(16, int(np.max(np.diff(pb.offsets))))
            self.decode_device(torch.from_numpy(pb.headers).to(dev), torch.from_numpy(pb.records).to(dev),
                               torch.from_numpy(pb.offsets).to(dev), n, H, W, max_rec, None if resized else out, status, rgb_t)
            if resized:
                if self._resizer is None:
                    self._resizer = GrayResizer(dev)
                self._resizer(rgb_t, out, status)
        return (out, status, rgb_t) if rgb else (out, status)


def resize_taps(n_out, n_in):
    """(i0, i1 int32 [n_out], f float32 [n_out]): the bilinear taps of datasets.resize_bilinear_f32 along one axis (the same float64
    expression, datasets.bilinear_taps), in the types csrc/resize.hip reads"""
    from .datasets import bilinear_taps
    i0, i1, f = bilinear_taps(n_out, n_in)
    return i0.astype(np.int32), i1.astype(np.int32), f


class GrayResizer:
    """GrayResizer(device)(rgb [n,H,W,3] u8, out [n,1,h,w] f32, status=None): datasets.gray_plane(rgb[i], (w, h)) of every row whose status
    is 0 (all rows without a status), on torch's current stream (include/mfr_hip.h mfr_resize_gray_bilinear).  The tap tables of a size pair
    are computed on the host once and kept on the device."""

    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        self._taps = {}

    def taps(self, n_out, n_in):
        key = (int(n_out), int(n_in))
        t = self._taps.get(key)
        if t is None:
            t = self._taps[key] = tuple(torch.from_numpy(a).to(self.device) for a in resize_taps(*key))
        return t

    def __call__(self, rgb, out, status=None):
        _lib.load(require_gpu=True)
        n, H, W, c = rgb.shape
        h, w = out.shape[-2:]
        assert c == 3 and rgb.dtype == torch.uint8 and out.dtype == torch.float32 and out.shape == (n, 1, h, w)
        assert status is None or (status.dtype == torch.int32 and status.numel() == n)
        y0, y1, fy = self.taps(h, H)
        x0, x1, fx = self.taps(w, W)
        cur = torch.cuda.current_stream(self.device)
        _lib.call("mfr_resize_gray_bilinear", rgb, n, H, W, status, y0, y1, fy, x0, x1, fx, h, w, out, stream=cur.cuda_stream)
        for t in (y0, y1, fy, x0, x1, fx):
            t.record_stream(cur)
        return out
