"""DPT-Hybrid depth stage on the GPU: ms per image at the network size for a few batch sizes, the split over the network's stages, and the FLOP count of
the configuration beside it (so a rate can be read off).  HIP events around work that ends in a synchronise; warm-up first; seeded synthetic weights.

    python tools/bench_dpt.py --out profiles/dpt_stage.json [--batches 2 16] [--net 384 512] [--image 540 720] [--iters 40] [--warmup 5]

The stage split times each stage of nets/dpt.DPTHIP on its own (events around the stage's launches, the stage's real input): the sum is close to, not
equal to, the whole pass.  The per-KERNEL split comes from a profiler run of its own (tracing slows the host, so no end-to-end number is taken from it):

    rocprofv3 --kernel-trace --output-format csv -d TRACE_DIR -- python tools/bench_dpt.py --trace-passes 10 --batches 16
    python tools/bench_dpt.py --merge-kernel-trace TRACE_DIR --trace-passes 10 --batches 16 --out profiles/dpt_stage.json

The first runs `warmup + 10` identical passes of one batch size in the f16x2 arithmetic and nothing else; the second (no GPU needed) sums the trace per kernel name,
divides by the number of passes and writes `kernel_split` into the record (kernels of the one-off weight packing show as fractions of a launch per pass)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mapfree_reloc_amd import options  # noqa: E402
from mapfree_reloc_amd.nets import dpt, weights as WT  # noqa: E402


def flops(arch, B, Hn, Wn):
    """multiply-adds x 2 of one pass over B images at Hn x Wn, by stage (convolutions, linear layers and the two attention products; norms and glue not counted)"""
    conv = lambda ci, co, k, h, w: 2.0 * ci * co * k * k * h * w
    out = {}
    E = arch["BIT_EMBEDDING_SIZE"]
    out["stem"] = conv(3, E, 7, Hn // 2, Wn // 2)
    f, prev, h, w = 0.0, E, Hn // 4, Wn // 4
    for s, (depth, c) in enumerate(zip(arch["BIT_DEPTHS"], arch["BIT_HIDDEN_SIZES"])):
        mid = c // 4
        for l in range(depth):
            stride = 2 if (l == 0 and s > 0) else 1
            ho, wo = h // stride, w // stride
            f += conv(prev, mid, 1, h, w) + conv(mid, mid, 3, ho, wo) + conv(mid, c, 1, ho, wo) + (conv(prev, c, 1, ho, wo) if l == 0 else 0.0)
            prev, h, w = c, ho, wo
    out["bottlenecks"] = f
    d, T = arch["VIT_WIDTH"], 1 + h * w
    out["patch_projection"] = conv(prev, d, 1, h, w)
    n_layers = max(arch["TAPS"][2:]) + 1
    out["vit_linear"] = n_layers * 2.0 * T * (3 * d * d + d * d + 2 * d * arch["VIT_MLP"])
    out["vit_attention"] = n_layers * 4.0 * T * T * d
    ns, F = arch["NECK_SIZES"], arch["FUSION_WIDTH"]
    out["reassemble"] = 2 * (2.0 * T * d * d) + conv(d, ns[2], 1, h, w) + conv(d, ns[3], 1, h, w) + conv(ns[3], ns[3], 3, h // 2, w // 2)
    sizes = [(Hn // 4, Wn // 4), (Hn // 8, Wn // 8), (h, w), (h // 2, w // 2)]
    neck = sum(conv(ns[i], F, 3, *sizes[i]) for i in range(4))
    for i, (hh, ww) in enumerate(reversed(sizes)):
        neck += (2 if i == 0 else 4) * conv(F, F, 3, hh, ww) + conv(F, F, 1, 2 * hh, 2 * ww)
    out["neck"] = neck
    out["head"] = conv(F, F // 2, 3, Hn // 2, Wn // 2) + conv(F // 2, 32, 3, Hn, Wn) + conv(32, 1, 1, Hn, Wn)
    out = {k: v * B for k, v in out.items()}
    out["total"] = sum(out.values())
    return out


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    runs = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        runs.append(a.elapsed_time(b) / iters)
    return sorted(runs)[1], runs


def bench(net, B, net_hw, image_hw, iters, warmup):
    g = torch.Generator().manual_seed(B)
    img = torch.randint(0, 256, (B, image_hw[0], image_hw[1], 3), generator=g, dtype=torch.uint8).cuda()
    whole, runs = timed(lambda: net(img, net_hw, millimetres=True), iters, warmup)
    metres, mm = net(img, net_hw, millimetres=True)
    assert bool(torch.isfinite(metres).all()), "bench_dpt: the pass produced non-finite depth"
    x = dpt.prep(img, *net_hw)
    s1, s2, s3 = net.backbone(x)
    gh, gw = s3.shape[2:]
    tok = net.tokenize(s3)
    t2, t3 = net.encoder(tok)
    r2, r3 = net.reassemble(2, t2, gh, gw), net.reassemble(3, t3, gh, gw)
    fused = net.neck([s1, s2, r2, r3])
    feat = net.head_features(fused)
    stages = {
        "prep": lambda: dpt.prep(img, *net_hw),
        "bit_backbone": lambda: net.backbone(x),
        "tokenize": lambda: net.tokenize(s3),
        "vit_encoder": lambda: net.encoder(tok),
        "reassemble": lambda: (net.reassemble(2, t2, gh, gw), net.reassemble(3, t3, gh, gw)),
        "neck": lambda: net.neck([s1, s2, r2, r3]),
        "head_convs": lambda: net.head_features(fused),
        "head_tail": lambda: dpt.head_tail(feat, net.head4_w, net.head4_b, image_hw[0], image_hw[1], millimetres=True),
    }
    split = {k: round(timed(fn, iters, max(1, warmup // 2))[0], 4) for k, fn in stages.items()}
    split["sum_ms"] = round(sum(split.values()), 4)
    fl = flops(net.arch, B, *net_hw)
    return dict(batch=B, ms_per_batch=round(whole, 4), ms_per_image=round(whole / B, 4), runs_ms=[round(r, 4) for r in runs], stage_split_ms=split,
                metres_range=[round(float(metres.min()), 4), round(float(metres.max()), 4)], flop=fl, tflops_whole_pass=round(fl["total"] / (whole * 1e-3) / 1e12, 3))


def trace_passes(args):
    """the profiler's workload: warmup + N whole passes of one batch size, f16x2, nothing else"""
    with torch.no_grad(), options.override(SPLIT="f16x2"):
        net = dpt.DPTHIP(WT.dpt_state_dict(), "cuda")
        B = args.batches[0]
        img = torch.randint(0, 256, (B, args.image[0], args.image[1], 3), generator=torch.Generator().manual_seed(B), dtype=torch.uint8).cuda()
        for _ in range(args.warmup + args.trace_passes):
            net(img, tuple(args.net), millimetres=True)
        torch.cuda.synchronize()


def merge_kernel_trace(args):
    import csv
    import glob
    files = sorted(glob.glob(os.path.join(args.merge_kernel_trace, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        raise SystemExit(f"bench_dpt: no *kernel_trace.csv under {args.merge_kernel_trace}")
    passes = args.warmup + args.trace_passes
    tot = {}
    for f in files:
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"].replace("(anonymous namespace)::", "")
            name = (name[5:] if name.startswith("void ") else name).split("(")[0]
            t = tot.setdefault(name, [0, 0])
            t[0] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"]); t[1] += 1
    rows = sorted(((n, ns / passes / 1e6, c / passes) for n, (ns, c) in tot.items()), key=lambda r: -r[1])
    res = json.load(open(args.out))
    res["kernel_split"] = dict(
        note=f"rocprofv3 --kernel-trace, a run of its own: {passes} whole passes (warm-up included; all passes are the same launches) of batch {args.batches[0]} at "
             f"{args.net[0]}x{args.net[1]}, f16x2; kernel time summed per name and divided by the passes; launches_per_pass below 1: one-off weight packing",
        batch=args.batches[0], passes=passes, kernel_ms_per_pass=round(sum(r[1] for r in rows), 4), launches_per_pass=round(sum(r[2] for r in rows), 1),
        kernels=[dict(name=n, ms_per_pass=round(ms, 4), launches_per_pass=round(c, 2)) for n, ms, c in rows])
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(kernel_ms_per_pass=res["kernel_split"]["kernel_ms_per_pass"], top=res["kernel_split"]["kernels"][:12])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, nargs="*", default=[2, 16])
    ap.add_argument("--net", type=int, nargs=2, default=[384, 512])
    ap.add_argument("--image", type=int, nargs=2, default=[540, 720])
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--trace-passes", type=int, default=0)
    ap.add_argument("--merge-kernel-trace", default=None)
    ap.add_argument("--splits", nargs="*", default=["f16x2", "bf16x3"])
    args = ap.parse_args()
    if args.merge_kernel_trace:
        return merge_kernel_trace(args)
    if not torch.cuda.is_available():
        raise SystemExit("bench_dpt: no GPU visible; this measurement has no CPU form")
    if args.trace_passes:
        return trace_passes(args)
    sd = WT.dpt_state_dict()
    res = dict(workload=dict(net_hw=args.net, image_hw=args.image, iters=args.iters, warmup=args.warmup, architecture="DPT-Hybrid (nets/dpt.ARCH)"),
               device=torch.cuda.get_device_name(0),
               note="whole pass = image bytes -> metres + millimetres at the image size (prep, network, head tail); HIP events, median of 3 runs of `iters` "
                    "passes, seeded synthetic weights, random images; the split times each stage alone on its real input (its sum is not the whole pass); "
                    "first measurement of a new stage: there is no earlier number",
               arithmetic={})
    with torch.no_grad():
        for split in args.splits:
            with options.override(SPLIT=split):
                net = dpt.DPTHIP(sd, "cuda")
            res["arithmetic"][split] = [bench(net, B, tuple(args.net), tuple(args.image), args.iters, args.warmup) for B in args.batches]
            del net
            torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
