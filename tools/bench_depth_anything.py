"""Depth Anything V2 depth stage on the GPU: median ms per frame and per stage for ViT-S / B / L at the production size (686 x 518 network input, 1814 tokens,
from 720 x 540 frames) in batches of 16, and DPT-Hybrid at its 384 x 512 through the same timer in the same run.

    python tools/bench_depth_anything.py --out profiles/depth_anything_stage.json [--encoders vits vitb vitl] [--batch 16] [--net 686 518] [--image 720 540]
                                         [--iters 5] [--repeats 5] [--warmup 2] [--min-window-ms 50]

HIP events around a window of passes that ends in a synchronise, `repeats` such windows after `warmup` passes; a window holds at least `iters` passes and at
least --min-window-ms of GPU time (the small stages run hundreds of calls per window; `iters` in the record is the count used).  The record holds the median
window and, beside it, the fastest and the slowest (the spread).  A stage's figure is events around its Python calls: it includes the output allocation and the
gaps between its launches, so for the stages of a few microseconds it is an upper bound on the kernel time; no kernel trace is taken here.  Seeded synthetic
weights, random image bytes, f16x2 arithmetic (bf16x3 with --splits).  Each stage is timed alone on its real input, so the stages' sum is close to, not equal
to, the whole pass.  No target is attached: this is the first measurement of this network here."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mapfree_reloc_amd import options  # noqa: E402
from mapfree_reloc_amd.config.depth_anything_arch import PRESETS  # noqa: E402
from mapfree_reloc_amd.nets import depth_anything as DA, dpt, weights as WT  # noqa: E402


def timed(fn, iters, repeats, warmup, min_window_ms):
    """-> dict(median, min, max, iters) in ms per call of fn.  A window holds at least `iters` calls and at least `min_window_ms` of GPU time (one probe window
    of `iters` calls sizes it): a window of a fraction of a millisecond would measure the gaps between launches as much as the kernels"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    per_call = max(a.elapsed_time(b) / iters, 1e-4)
    iters = max(iters, int(min_window_ms / per_call) + 1)
    runs = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        runs.append(a.elapsed_time(b) / iters)
    runs.sort()
    return dict(median=round(runs[len(runs) // 2], 4), min=round(runs[0], 4), max=round(runs[-1], 4), iters=iters)


def per_frame(t, B):
    return dict(ms_per_batch=t, ms_per_frame=round(t["median"] / B, 4), spread_ms_per_frame=[round(t["min"] / B, 4), round(t["max"] / B, 4)])


def flops(a, B, gh, gw):
    """multiply-adds x 2 of one pass (products and convolutions only), by stage"""
    conv = lambda ci, co, k, h, w: 2.0 * ci * co * k * k * h * w
    d, T, hw = a["VIT_WIDTH"], 1 + gh * gw, gh * gw
    n_layers = max(a["TAPS"]) + 1
    ns, F = a["NECK_SIZES"], a["FUSION_WIDTH"]
    sizes = [(4 * gh, 4 * gw), (2 * gh, 2 * gw), (gh, gw), ((gh - 1) // 2 + 1, (gw - 1) // 2 + 1)]
    out = dict(embedding=2.0 * hw * DA.PATCH_K * d, encoder_linear=n_layers * 2.0 * T * (4 * d * d + 2 * d * a["VIT_MLP"]), encoder_attention=n_layers * 4.0 * T * T * d)
    out["reassemble"] = sum(2.0 * T * d * ns[i] for i in range(4)) + 2.0 * T * ns[0] * ns[0] * 16 + 2.0 * T * ns[1] * ns[1] * 4 + conv(ns[3], ns[3], 3, *sizes[3])
    neck = sum(conv(ns[i], F, 3, *sizes[i]) for i in range(4))
    up = [sizes[2], sizes[1], sizes[0], (8 * gh, 8 * gw)]
    for i, (hh, ww) in enumerate(reversed(sizes)):
        neck += (2 if i == 0 else 4) * conv(F, F, 3, hh, ww) + conv(F, F, 1, *up[i])
    out["neck"] = neck
    out["head"] = conv(F, F // 2, 3, 8 * gh, 8 * gw) + conv(F // 2, a["HEAD_WIDTH"], 3, 14 * gh, 14 * gw) + conv(a["HEAD_WIDTH"], 1, 1, 14 * gh, 14 * gw)
    out = {k: v * B for k, v in out.items()}
    out["total"] = sum(out.values())
    return out


def bench_da(name, split, B, net_hw, image_hw, T):
    arch = dict(PRESETS[name])
    with options.override(SPLIT=split):
        net = DA.DepthAnythingHIP(WT.depth_anything_state_dict(arch=arch), "cuda", arch=arch)
    gh, gw = net_hw[0] // DA.PATCH, net_hw[1] // DA.PATCH
    img = torch.randint(0, 256, (B, image_hw[0], image_hw[1], 3), generator=torch.Generator().manual_seed(B), dtype=torch.uint8).cuda()
    whole = timed(lambda: net(img, net_hw, millimetres=True), **T)
    metres, _ = net(img, net_hw, millimetres=True)
    assert bool(torch.isfinite(metres).all()), "bench_depth_anything: the pass produced non-finite depth"
    rows = net.prep(img, net_hw)
    emb = net.embed(rows)
    tok = DA.tokens(emb, net.cls, net.position_embeddings(gh, gw), B)
    h, Tn = arch["VIT_WIDTH"], 1 + gh * gw
    last = max(arch["TAPS"])

    def layers():
        x, states = tok.reshape(B * Tn, h).clone(), {}
        for l, L in enumerate(net.layers[:last + 1]):
            net.vit_layer(L, x, B, Tn)
            if l in arch["TAPS"]:
                states[l] = x.clone().view(B, Tn, h)
        return [states[l] for l in arch["TAPS"]]
    states = layers()
    taps_reassemble = lambda: [net.reassemble(i, net.tap(s), gh, gw) for i, s in enumerate(states)]
    feats = taps_reassemble()
    fused = net.neck(feats)
    feat = net.head_features(fused, gh, gw)
    stages = {
        "patch_rows": lambda: net.prep(img, net_hw),
        "embedding_product": lambda: net.embed(rows),
        "token_assembly": lambda: DA.tokens(emb, net.cls, net.position_embeddings(gh, gw), B),
        "encoder": layers,
        "taps_and_reassemble": taps_reassemble,
        "neck": lambda: net.neck(feats),
        "head_at_14g": lambda: net.head_features(fused, gh, gw),
        "tail": lambda: net.tail(feat, image_hw, millimetres=True),
    }
    split_ms = {k: per_frame(timed(fn, **T), B) for k, fn in stages.items()}
    fl = flops(arch, B, gh, gw)
    rec = dict(encoder=name, arithmetic=split, batch=B, tokens=Tn, whole_pass=per_frame(whole, B), stages=split_ms,
               stages_sum_ms_per_frame=round(sum(v["ms_per_frame"] for v in split_ms.values()), 4), flop=fl,
               tflops_whole_pass=round(fl["total"] / (whole["median"] * 1e-3) / 1e12, 3),
               head_map_bytes_per_frame=dict(note="the 14 g map of FUSION_WIDTH / 2 channels: written once by the resize, read once by conv2",
                                             bytes=4 * (arch["FUSION_WIDTH"] // 2) * net_hw[0] * net_hw[1]),
               metres_range=[round(float(metres.min()), 4), round(float(metres.max()), 4)])
    del net
    torch.cuda.empty_cache()
    return rec


def bench_hybrid(split, B, image_hw, T, net_hw=(384, 512)):
    with options.override(SPLIT=split):
        net = dpt.DPTHIP(WT.dpt_state_dict(), "cuda")
    img = torch.randint(0, 256, (B, image_hw[0], image_hw[1], 3), generator=torch.Generator().manual_seed(B), dtype=torch.uint8).cuda()
    whole = timed(lambda: net(img, net_hw, millimetres=True), **T)
    del net
    torch.cuda.empty_cache()
    return dict(network="DPT-Hybrid", arithmetic=split, batch=B, net_hw=list(net_hw), tokens=1 + (net_hw[0] // 16) * (net_hw[1] // 16), whole_pass=per_frame(whole, B))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--encoders", nargs="*", default=["vits", "vitb", "vitl"])
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--net", type=int, nargs=2, default=[686, 518])
    ap.add_argument("--image", type=int, nargs=2, default=[720, 540])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--min-window-ms", type=float, default=50.0)
    ap.add_argument("--splits", nargs="*", default=["f16x2"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_depth_anything: no GPU visible; this measurement has no CPU form")
    T = dict(iters=args.iters, repeats=args.repeats, warmup=args.warmup, min_window_ms=args.min_window_ms)
    res = dict(workload=dict(net_hw=args.net, image_hw=args.image, batch=args.batch, **T), device=torch.cuda.get_device_name(0),
               note="whole pass = image bytes -> metres + millimetres at the image size; HIP events around windows of at least `iters` passes and `min_window_ms` of GPU "
                    "time, `repeats` windows after `warmup` passes: median window, fastest and slowest beside it; stage figures include allocation and launch gaps "
                    "(upper bounds on kernel time for the microsecond stages; no kernel trace); seeded synthetic weights, random images; each stage is timed alone on its real input (the sum "
                    "is not the whole pass); first measurement of this network on this chip: no target, no earlier number",
               depth_anything=[], dpt_hybrid=[])
    with torch.no_grad():
        for split in args.splits:
            for name in args.encoders:
                res["depth_anything"].append(bench_da(name, split, args.batch, tuple(args.net), tuple(args.image), T))
                print(json.dumps({k: res["depth_anything"][-1][k] for k in ("encoder", "arithmetic", "whole_pass", "stages_sum_ms_per_frame")}), flush=True)
            res["dpt_hybrid"].append(bench_hybrid(split, args.batch, tuple(args.image), T))
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
