"""16-bit gray (millimetre depth) PNG decode on the GPU (csrc/png.hip, include/mfr_hip.h mfr_png_depth_*), with the chunk walk on the host
(csrc/host_decode.c, libmfr_host.so mfr_host_png_parse; layout in include/mfr_png.h).  The result is the loaders' depth plane of the file,
datasets.read_depth_plane(path), bit for bit: float32(uint16 / 1000.0).  Torch only provides memory and the stream.

| stage | what | where |
|---|---|---|
| parse | signature, IHDR first (13 bytes, a legal colour type / bit depth pair, non-zero size), every chunk length against the file's, IDAT chunks consecutive, IEND; ancillary chunks skipped; the IDAT payloads joined into the record (the zlib stream) + >= 8 zero bytes; zlib header: method 8, FCHECK | host, plain C |
| inflate | RFC 1950 / 1951: stored, fixed and dynamic blocks, any number of them, distances up to 32 768; wave-uniform symbol decode from a 64-bit bit buffer fed by 256-byte coalesced loads; code tables in LDS (10 / 9 / 7-bit look-ups + canonical lists) built by the lanes together; literals stored 64 at a time, matches copied by the lanes (out[pos + i] = out[pos - dist + i % dist]) | one wavefront per image |
| check | inflated size == H (1 + 2 W); Adler-32 as a lane-parallel sum; filter bytes <= 4 | same wavefront |
| unfilter | filters 0-4 at 2 bytes per pixel, lane l on row 64 p + l running l pixels behind lane l - 1 (the row above arrives by a lane shift), five predictors branch-free, selected on the filter byte | same wavefront |
| convert | big-endian sample v -> (float)((double) v / 1000.0) | same wavefront |

Chunk CRCs are NOT verified (neither on the host nor on the device); the stream's Adler-32 is, on the device.  Files the parse calls
unsupported (any colour type / bit depth but gray 16, Adam7, a zlib window above 32 KiB, a preset dictionary) are the caller's to decode on
the host; `decode` reports them per image in `status` (1) and leaves their planes untouched, as it does for every row with an error
status.  No CPU fallback: without libmfr_hip.so or a GPU it raises MfrLibraryError.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib

OK, UNSUPPORTED, INVALID, CAPACITY = 0, 1, 2, 3
E_DATA, E_TRUNC, E_SIZE, E_CHECK = 0x10, 0x20, 0x40, 0x80


class Header(C.Structure):
    """include/mfr_png.h mfr_png_header"""
    _fields_ = [(f, C.c_int32) for f in ("status", "width", "height", "bit_depth", "color_type", "interlace", "stream_bytes", "record_bytes")]


HEADER_BYTES = C.sizeof(Header)


def _host():
    from . import datasets
    lib = datasets._host_lib()
    if lib is None:
        raise _lib.MfrLibraryError("csrc/libmfr_host.so (ABI 4) not found: build it with __graft_entry__.build()")
    assert lib.mfr_host_png_header_bytes() == HEADER_BYTES, "png_ops.Header does not mirror include/mfr_png.h"
    return lib


def record_bound(nbytes):
    """bytes a file of `nbytes` needs as a record (always enough)"""
    return int(_host().mfr_host_png_record_bound(int(nbytes)))


def parse(data, cap=None):
    """one file's bytes -> (status, Header, record u8 array or None).  cap: record buffer size (default: always enough)"""
    lib = _host()
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    cap = record_bound(buf.size) if cap is None else int(cap)
    rec = np.zeros(max(cap, 16), dtype=np.uint8)
    h = Header()
    nb = C.c_size_t(0)
    st = lib.mfr_host_png_parse(buf.ctypes.data, buf.size, C.byref(h), rec.ctypes.data, cap, C.byref(nb))
    return st, h, (rec[:nb.value] if st == OK else None)


def parse_into(data, header_row, slot):
    """parse straight into a batch: header_row = u8 [HEADER_BYTES] view, slot = u8 view (16-aligned) -> (status, record bytes)"""
    lib = _host()
    buf = np.frombuffer(data, dtype=np.uint8)
    nb = C.c_size_t(0)
    st = lib.mfr_host_png_parse(buf.ctypes.data, buf.size, header_row.ctypes.data, slot.ctypes.data, slot.size, C.byref(nb))
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


class DepthPngDecoder:
    """DepthPngDecoder(device).decode(files: list[bytes] | PackedBatch, out=None) -> (depth [n,H,W] f32, status [n] i32) on the device.
    status: 0 ok, 1 unsupported (host's to decode), 2 / 3 invalid / capacity at the parse, E_DATA / E_TRUNC / E_SIZE / E_CHECK from the
    device; a row whose status is not 0 keeps its plane of `out` as it was.  No CPU fallback: without libmfr_hip.so or a GPU it raises
    MfrLibraryError."""

    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        self._scratch = None

    def scratch(self, n, H, W):
        lib = _lib.load(require_gpu=True)
        nb = lib.mfr_png_depth_workspace_bytes(n, H, W)
        if nb == 0:
            raise ValueError(f"PNG: unsupported batch {n}x{H}x{W}")
        if self._scratch is None or self._scratch.numel() < nb:
            self._scratch = torch.empty(nb, dtype=torch.uint8, device=self.device)
        return self._scratch

    def decode_device(self, headers, records, offsets, n, H, W, max_record, out, status):
        """the device half on tensors already on the device (headers u8 [n, HEADER_BYTES], records u8, offsets i64 [n + 1]), launched on
        torch's current stream; the scratch is marked as used by that stream"""
        _lib.load(require_gpu=True)
        sc = self.scratch(n, H, W)
        cur = torch.cuda.current_stream(self.device)
        _lib.call("mfr_png_depth_decode", headers, records, offsets, n, H, W, int(max_record), sc, sc.numel(), out, status, stream=cur.cuda_stream)
        sc.record_stream(cur)

    def decode(self, files, out=None):
        _lib.load(require_gpu=True)
        pb = files if isinstance(files, PackedBatch) else pack(files)
        n, H, W = pb.n, pb.H, pb.W
        dev = self.device
        if out is None:
            out = torch.zeros(n, H, W, dtype=torch.float32, device=dev)
        assert out.shape == (n, H, W) and out.dtype == torch.float32 and out.is_contiguous()
        status = torch.from_numpy(pb.status.copy()).to(dev)
        if n and bool((pb.status == OK).any()):                # nothing the device takes: the parse's statuses only
            max_rec = max(16, int(np.max(np.diff(pb.offsets))))
            self.decode_device(torch.from_numpy(pb.headers).to(dev), torch.from_numpy(pb.records).to(dev),
                               torch.from_numpy(pb.offsets).to(dev), n, H, W, max_rec, out, status)
        return out, status
