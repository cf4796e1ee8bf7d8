"""Baseline JPEG decode on the GPU (csrc/jpeg.hip, jpeg_ops.JpegDecoder) vs the host route, per frame, on 540x720 frames encoded like the
bench tree's (tools/bench_fused_split.write_scene: PIL quality 92, 4:2:0, the synthetic_pair texture as RGB gray).
  device   ms per batch of B frames for the three launches (entropy, IDCT, colour), headers + records already on the device;
           the bytes and blocks the batch holds
  host     per frame on one CPU: file read + C parse into a record (the device route's host work), PIL's JPEG decode + luma + / 255
           (datasets.read_gray_plane, today's host route) and the 16-bit depth PNG read (datasets.read_depth_plane, both routes)
Prints one JSON line; --out writes it to a file as well.
Usage: python tools/bench_jpeg.py [--batch 64] [--reps 20] [--out profiles/jpeg_bench_b64.json]"""
import argparse
import io
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mapfree_reloc_amd import datasets as D, images as IM, jpeg_ops as J  # noqa: E402


def frames(B):
    from PIL import Image
    out, dpt = [], []
    for k in range(B):
        p = IM.synthetic_pair(100 + k // 4)
        im = np.roll(p["img1" if k % 2 else "img0"], 8 * (k % 5), axis=0)
        rgb = np.repeat((np.clip(im, 0, 1) * 255 + 0.5).astype(np.uint8)[..., None], 3, 2)
        b = io.BytesIO(); Image.fromarray(rgb).save(b, "JPEG", quality=92); out.append(b.getvalue())
        b = io.BytesIO(); Image.fromarray((np.clip(p["depth0"], 0, 65.0) * 1000 + 0.5).astype(np.uint16)).save(b, "PNG"); dpt.append(b.getvalue())
    return out, dpt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    files, pngs = frames(a.batch)
    tmp = tempfile.mkdtemp()
    paths = []
    for k, (f, p) in enumerate(zip(files, pngs)):
        open(os.path.join(tmp, f"{k}.jpg"), "wb").write(f); open(os.path.join(tmp, f"{k}.png"), "wb").write(p)
        paths.append(os.path.join(tmp, f"{k}"))
    # host work per frame
    def per_frame(fn):
        fn(0)
        t0 = time.perf_counter()
        for k in range(len(paths)):
            fn(k)
        return 1e3 * (time.perf_counter() - t0) / len(paths)
    t_parse = per_frame(lambda k: J.parse(open(paths[k] + ".jpg", "rb").read()))
    t_pil = per_frame(lambda k: D.read_gray_plane(paths[k] + ".jpg", None))
    t_png = per_frame(lambda k: D.read_depth_plane(paths[k] + ".png"))
    # device
    pb = J.pack(files)
    dev = "cuda"
    hd, rec, off = (torch.from_numpy(x).to(dev) for x in (pb.headers, pb.records, pb.offsets))
    n, H, W = pb.n, pb.H, pb.W
    out = torch.empty(n, 1, H, W, device=dev)
    st = torch.from_numpy(pb.status.copy()).to(dev)
    dec = J.JpegDecoder(dev)
    max_rec = int(np.max(np.diff(pb.offsets)))
    run = lambda: dec.decode_device(hd, rec, off, n, H, W, max_rec, out, st)
    run(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        run()
    e1.record(); torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.reps
    ok = all(np.array_equal(out[i, 0].cpu().numpy(), D.read_gray_plane(paths[i] + ".jpg", None)) for i in range(0, n, 7))
    heads = [J.parse(f)[1] for f in files]
    r = dict(metric="jpeg_decode", batch=n, H=H, W=W, quality=92, sampling="4:2:0", device_ms_per_batch=round(ms, 4),
             device_ms_per_frame=round(ms / n, 5), device_frames_per_s=round(1e3 * n / ms, 1),
             file_bytes_mean=int(np.mean([len(f) for f in files])), record_bytes_total=int(pb.offsets[-1]),
             entropy_bytes_total=int(sum(h.data_bytes for h in heads)), blocks_total=int(sum(h.total_mcus * h.blocks_per_mcu for h in heads)),
             rounds_max=int(dec.rounds.max()), host_ms_per_frame=dict(read_and_parse=round(t_parse, 4), pil_gray_plane=round(t_pil, 4),
                                                                   png_depth=round(t_png, 4)),
             bit_exact_vs_read_gray_plane=bool(ok), device=torch.cuda.get_device_name(0))
    s = json.dumps(r)
    print(s)
    if a.out:
        open(a.out, "w").write(s + "\n")


if __name__ == "__main__":
    main()
