"""A/B record: the two pixel tilings of the direct f16x2 3x3 convolution (csrc/conv_direct.hip, mfr_conv3x3_direct_f16x2_tiled) -- tile_mode 1, the 2-D
tile of 8 rows x 32 columns, against tile_mode 2, the linear tile of 256 units of the padded linear pixel space -- on every stride-1, un-pooled layer
shape of the two backbones that the linear geometry covers (Cout > 64, W <= 158), at the bench batches (64 SuperPoint images of 720 x 540, 32 LoFTR
images of 720 x 544), same inputs, and pitch W + 1 against W + 4 where W % 4 == 0.

Per shape: REPS repetitions of [2-D, linear (, linear at W + 4)], each the median of N single-launch event timings after a warm-up; the record keeps
every repetition's medians, their medians, the SPREAD (max - min) of the 2-D median over the repetitions, computed positions per image of both
tilings, and torch.equal of the outputs.  `linear_faster` is the rule `auto` is filled by: median(linear) < median(2-D) - spread(2-D).
python tools/ab_direct_tiles.py [out.json] [layer-name-substring]"""
import json
import os
import statistics
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import mapfree_reloc_amd  # noqa: F401
from mapfree_reloc_amd import _lib

dev = "cuda:0"
N, WARM, REPS = 60, 10, 3
# name, images, Cin, Cout, H, W, residual, rows output
LAYERS = [("sp.conv3a 64->128 @180x135", 64, 64, 128, 180, 135, 0, 0), ("sp.conv4a 128->128 @90x67", 64, 128, 128, 90, 67, 0, 0),
          ("sp.convPa 128->256 @90x67", 64, 128, 256, 90, 67, 0, 0), ("sp.convDa 128->256 @90x67 rows", 64, 128, 256, 90, 67, 0, 1),
          ("loftr.layer2 196->196 @180x136 res", 32, 196, 196, 180, 136, 1, 0), ("loftr.layer3 256->256 @90x68 res", 32, 256, 256, 90, 68, 1, 0),
          ("loftr.l2out2.0 256->256 @180x136", 32, 256, 256, 180, 136, 0, 0),
          ("loftr.l2out2.1 256->196 @180x136", 32, 256, 196, 180, 136, 0, 0)]


def median_ms(fn):
    for _ in range(WARM):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(N)]
    for e0, e1 in ev:
        e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return statistics.median(e0.elapsed_time(e1) for e0, e1 in ev)


def main():
    lib = _lib.load(require_gpu=True)
    sel = sys.argv[2] if len(sys.argv) > 2 else ""
    res = {}
    for name, n, ci, co, H, W, has_res, rows in LAYERS:
        if sel not in name:
            continue
        g = torch.Generator().manual_seed(ci + H)
        x = torch.randn(n, ci, H, W, generator=g).to(dev)
        w = (torch.randn(co, ci, 3, 3, generator=g) / (3.0 * ci ** 0.5)).to(dev)
        b = torch.randn(co, generator=g).to(dev)
        r = torch.randn(n, co, H, W, generator=g).to(dev) if has_res else None
        u = torch.empty(lib.mfr_conv3x3_direct_f16x2_filter_bytes(ci, co), dtype=torch.uint8, device=dev)
        _lib.check(lib.mfr_conv3x3_direct_f16x2_filter_pack(_lib.ptr(w), ci, co, _lib.ptr(u), _lib.stream_ptr()), "pack")
        variants = {"rows2d": (1, 0), "linear_w1": (2, W + 1)}
        if W % 4 == 0:
            variants["linear_w4"] = (2, W + 4)
        ys = {k: torch.full((n, H, W, co) if rows else (n, co, H, W), float("nan"), dtype=torch.float32, device=dev) for k in variants}

        def launch(k):
            mode, pitch = variants[k]
            _lib.check(lib.mfr_conv3x3_direct_f16x2_tiled(_lib.ptr(x), _lib.ptr(u), _lib.ptr(b), _lib.ptr(r), n, ci, co, H, W, 1, 0, _lib.ptr(ys[k]),
                                                          co if rows else 0, mode, pitch, _lib.stream_ptr()), k)
        reps = {k: [] for k in variants}
        for _ in range(REPS):
            for k in variants:
                reps[k].append(round(median_ms(lambda: launch(k)), 4))
        torch.cuda.synchronize()
        med = {k: statistics.median(v) for k, v in reps.items()}
        spread = max(reps["rows2d"]) - min(reps["rows2d"])
        best = min((k for k in variants if k != "rows2d"), key=lambda k: med[k])
        res[name] = dict(images=n, launches_per_median=N, repetitions=reps, median_ms=med, rows2d_spread_ms=round(spread, 4),
                         positions_per_image=dict(real=H * W, rows2d=-(-W // 32) * 32 * -(-H // 8) * 8,
                                                  **{k: -(-H * p // 256) * 256 for k, (m, p) in variants.items() if m == 2}),
                         equal_to_rows2d={k: bool(torch.equal(ys[k], ys["rows2d"])) and bool(torch.isfinite(ys[k]).all()) for k in variants if k != "rows2d"},
                         best_linear=best, linear_over_rows2d=round(med[best] / med["rows2d"], 4), linear_faster=bool(med[best] < med["rows2d"] - spread))
        print(name, json.dumps(res[name]), flush=True)
        del x, w, b, r, u, ys
    if len(sys.argv) > 1 and sys.argv[1]:
        os.makedirs(os.path.dirname(sys.argv[1]) or ".", exist_ok=True)
        json.dump(res, open(sys.argv[1], "w"), indent=1)


if __name__ == "__main__":
    main()
