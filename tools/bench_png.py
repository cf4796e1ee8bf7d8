"""16-bit depth PNG decode on the GPU (csrc/png.hip, png_ops.DepthPngDecoder) vs the host route, on the 540x720 depth maps of a tree that
tools/bench_fused_split.write_scene writes (the same files the loader legs of that tool read).
  device   ms per batch of B maps for the one launch (inflate, Adler-32, unfilter, convert), headers + records already on the device;
           the stream bytes the batch holds
  host     per map on one CPU: file read + C parse into a record (the device route's host work) and the PNG read + table look-up
           (datasets.read_depth_plane, today's host route)
write_scene's depth is piecewise smooth: PIL's encoder deflates a map to about 2.2 KB of stream (long matches, few symbols), not the few
hundred KB a sensor's or a network's depth map takes; the stream sizes measured are part of the record.
Prints one JSON line; --out writes it to a file as well.
Usage: python tools/bench_png.py [--batch 64] [--reps 20] [--out profiles/png_bench_b64.json]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mapfree_reloc_amd import datasets as D, png_ops as P  # noqa: E402


def scene_files(B):
    """the bytes of B depth PNGs out of scenes written by write_scene (7 query frames each: 8 depth maps per scene), in path order"""
    import glob
    from tools.bench_fused_split import write_scene
    root = tempfile.mkdtemp()
    for s in range((B + 7) // 8):
        write_scene((root, s, 7))
    paths = sorted(glob.glob(os.path.join(root, "test", "*", "*", "*.png")))[:B]
    assert len(paths) == B
    return [open(p, "rb").read() for p in paths]


def measure(files, reps):
    tmp = tempfile.mkdtemp()
    paths = []
    for k, f in enumerate(files):
        paths.append(os.path.join(tmp, f"{k}.png"))
        open(paths[-1], "wb").write(f)

    def per_frame(fn):
        fn(0)
        t0 = time.perf_counter()
        for k in range(len(paths)):
            fn(k)
        return 1e3 * (time.perf_counter() - t0) / len(paths)
    t_parse = per_frame(lambda k: P.parse(open(paths[k], "rb").read()))
    t_png = per_frame(lambda k: D.read_depth_plane(paths[k]))
    pb = P.pack(files)
    dev = "cuda"
    hd, rec, off = (torch.from_numpy(x).to(dev) for x in (pb.headers, pb.records, pb.offsets))
    n, H, W = pb.n, pb.H, pb.W
    out = torch.empty(n, H, W, device=dev)
    st = torch.from_numpy(pb.status.copy()).to(dev)
    dec = P.DepthPngDecoder(dev)
    max_rec = int(np.max(np.diff(pb.offsets)))
    run = lambda: dec.decode_device(hd, rec, off, n, H, W, max_rec, out, st)
    run(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        run()
    e1.record(); torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    ok = int(st.abs().max()) == 0 and all(np.array_equal(out[i].cpu().numpy(), D.read_depth_plane(paths[i])) for i in range(n))
    heads = [P.parse(f)[1] for f in files]
    return dict(batch=n, H=H, W=W, device_ms_per_batch=round(ms, 4), device_ms_per_map=round(ms / n, 5), device_maps_per_s=round(1e3 * n / ms, 1),
                file_bytes_mean=int(np.mean([len(f) for f in files])), stream_bytes_total=int(sum(h.stream_bytes for h in heads)),
                stream_bytes_max=int(max(h.stream_bytes for h in heads)), inflated_bytes_per_map=H * (1 + 2 * W),
                host_ms_per_frame=dict(read_and_parse=round(t_parse, 4), png_depth=round(t_png, 4)), bit_exact_vs_read_depth_plane=bool(ok))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    r = dict(metric="png_depth_decode", files="tools/bench_fused_split.write_scene", **measure(scene_files(a.batch), a.reps),
             device=torch.cuda.get_device_name(0))
    s = json.dumps(r)
    print(s)
    if a.out:
        open(a.out, "w").write(s + "\n")


if __name__ == "__main__":
    main()
