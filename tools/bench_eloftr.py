"""Matcher-stage time of EfficientLoFTR and LoFTR on the same inputs: 16 pairs of 540 x 720 (the bench's synthetic images), HIP events after a
warm-up, the two stages alternating, in both HIP.SPLIT arithmetics.  LoFTRHIP is the yardstick: same images, same run, same clocks.  The split
times each part of the EfficientLoFTR stage on the stage's own tensors (events around repeated calls); for the three kernels that are new with this
stage -- aggregation + LayerNorm, short-sequence attention, two-stage fine matching -- it also states the achieved fraction of the bound that limits
them: HBM bytes moved / 6.29 TB/s (the measured copy rate) for the aggregation, fp32 FLOP / 157.3 TFLOP/s (vector = fp32 matrix peak) for the other
two, which multiply in fp32 registers.  The seeded weights match few cells of the synthetic images, so the window gather and the fine matching are
also timed with EVERY cell matched (the `_every_cell` rows), which is the load a trained network puts on them.  Writes profiles/eloftr_stage.json.

    python tools/bench_eloftr.py [--pairs 16] [--iters 10] [--warmup 3] [--out profiles/eloftr_stage.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mapfree_reloc_amd import _lib, images as IM, options  # noqa: E402
from mapfree_reloc_amd.nets import weights as WT  # noqa: E402
from mapfree_reloc_amd.nets import eloftr as EL  # noqa: E402
from mapfree_reloc_amd.nets.loftr import LoFTRHIP  # noqa: E402

H, W = 720, 540
HBM_BPS, FP32_FLOPS = 6.29e12, 157.3e12
GFLOP_PER_PAIR = dict(eloftr=548.0, loftr=975.0)            # algorithmic work from the layer shapes


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def eloftr_split(net, images, iters, warmup):
    """ms per call of each part of the stage, calls per stage, and the bound fractions of the three new kernels"""
    B = images.shape[0] // 2
    f = net.features(images)
    hc, wc = f.s3.shape[2:]
    L, La = hc * wc, (hc // 4) * (wc // 4)
    xm = net.tokens(f, range(0, 2 * B, 2), f, range(1, 2 * B, 2))
    both = xm.view(-1, 512)
    blk = net.layers[0]["self"]
    q_tok, kv_tok = net.aggregate(blk, both[:, :256], 2 * B, (hc, wc))
    qkv = torch.empty(2 * B * La, 768, device=images.device)
    blk["lq"](q_tok, out=qkv[:, :256]); blk["lkv"](kv_tok, out=qkv[:, 256:])
    net.transformer(xm, B, (hc, wc))
    f0, f1 = xm[0].view(B, L, 512)[..., :256], xm[1].view(B, L, 512)[..., :256]
    i_ids, j_ids, mconf, n = net.coarse_match_features(f0, f1, (hc, wc))
    cm = net.coarse_map(xm, 2 * B, (hc, wc))
    s2, s1 = torch.cat([f.s2[0::2], f.s2[1::2]]), torch.cat([f.s1[0::2], f.s1[1::2]])
    half = net.pyramid(cm, s2, s1)
    side = torch.arange(2 * B, dtype=torch.int32, device=images.device)
    maxN = L
    w0 = net.gather_windows(half, side[:B], i_ids, n, maxN, wc, 8, 0)
    w1 = net.gather_windows(half, side[B:], j_ids, n, maxN, wc, 10, 1)
    matches = int(n.clamp(max=maxN).sum())
    # the seeded weights match few cells of the synthetic images, so the match-dependent kernels are ALSO timed with every cell matched (cell i with
    # cell i: B * L windows, more than LoFTR's ~4100 matches per pair on these images)
    n_all = torch.full((B,), L, dtype=torch.int32, device=images.device)
    cells = torch.arange(L, dtype=torch.int32, device=images.device).repeat(B, 1).contiguous()
    wa0 = net.gather_windows(half, side[:B], cells, n_all, maxN, wc, 8, 0)
    wa1 = net.gather_windows(half, side[B:], cells, n_all, maxN, wc, 10, 1)
    stages = [
        ("backbone_21_folded_blocks", 1, lambda: net.features(images)),
        ("tokens", 1, lambda: net.tokens(f, range(0, 2 * B, 2), f, range(1, 2 * B, 2))),
        ("aggregate_ln", 12, lambda: net.aggregate(blk, both[:, :256], 2 * B, (hc, wc))),
        ("rotary", 4, lambda: net.rotary(qkv, (hc // 4, wc // 4))),
        ("attention_small_seq", 12, lambda: net.attention(qkv, 2 * B, La)),
        ("transformer_4_layers", 1, lambda: net.transformer(xm, B, (hc, wc))),
        ("coarse_match", 1, lambda: net.coarse_match_features(f0, f1, (hc, wc))),
        ("fine_pyramid", 1, lambda: net.pyramid(net.coarse_map(xm, 2 * B, (hc, wc)), s2, s1)),
        ("gather_windows_both", 1, lambda: (net.gather_windows(half, side[:B], i_ids, n, maxN, wc, 8, 0), net.gather_windows(half, side[B:], j_ids, n, maxN, wc, 10, 1))),
        ("fine_match_two_stage", 1, lambda: net.fine_match(w0, w1, i_ids, j_ids, n, maxN, wc)),
        ("gather_windows_both_every_cell", 0, lambda: (net.gather_windows(half, side[:B], cells, n_all, maxN, wc, 8, 0),
                                                       net.gather_windows(half, side[B:], cells, n_all, maxN, wc, 10, 1))),
        ("fine_match_two_stage_every_cell", 0, lambda: net.fine_match(wa0, wa1, cells, cells, n_all, maxN, wc)),
    ]
    out = {}
    for name, calls, fn in stages:
        ms = timed(fn, iters, warmup)
        out[name] = dict(ms_per_call=round(ms, 4), calls_per_stage=calls)
    # aggregation (self form, both outputs): reads 2B L rows of 256 floats once, writes two token sets
    agg_bytes = 2 * B * (L + 2 * La) * 256 * 4
    out["aggregate_ln"]["hbm_bound_fraction"] = round(agg_bytes / HBM_BPS / (out["aggregate_ln"]["ms_per_call"] * 1e-3), 4)
    att_flop = 2 * B * 8 * La * La * 32 * 2 * 2
    out["attention_small_seq"]["fp32_bound_fraction"] = round(att_flop / FP32_FLOPS / (out["attention_small_seq"]["ms_per_call"] * 1e-3), 4)
    out["fine_match_two_stage"]["matches"] = matches
    k = out["fine_match_two_stage_every_cell"]
    k.update(matches=B * L, fp32_bound_fraction=round(B * L * (64 * 100 * 56 * 2) / FP32_FLOPS / (k["ms_per_call"] * 1e-3), 4),
             hbm_bound_fraction=round(B * L * 164 * 64 * 4 / HBM_BPS / (k["ms_per_call"] * 1e-3), 4))
    out["gather_windows_both_every_cell"]["hbm_write_bound_fraction"] = round(B * L * 164 * 64 * 4 / HBM_BPS / (out["gather_windows_both_every_cell"]["ms_per_call"] * 1e-3), 4)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eloftr_stage.json"))
    args = ap.parse_args(argv)
    _lib.load(require_gpu=True)
    dev = torch.device("cuda:0")
    sb = IM.synthetic_batch([100 + i for i in range(args.pairs)], H, W)
    images = torch.from_numpy(np.ascontiguousarray(sb["images"])).to(dev)
    rec = dict(workload=dict(pairs=args.pairs, image_hw=[H, W], iters=args.iters, warmup=args.warmup), device=torch.cuda.get_device_name(0),
               note="matcher stage (images on the device -> correspondences), HIP events, seeded synthetic weights; ms per batch of pairs; LoFTRHIP on the same "
                    "images in the same run is the yardstick", gflop_per_pair=GFLOP_PER_PAIR, arithmetic={})
    for split in ("f16x2", "bf16x3"):
        options.reset()
        with options.override(SPLIT=split), torch.no_grad():
            el = EL.EfficientLoFTRHIP(WT.eloftr_state_dict(), dev)
            lo = LoFTRHIP(WT.loftr_state_dict(), dev)
            lo_images = torch.nn.functional.pad(images, (0, (-images.shape[-1]) % 8, 0, (-images.shape[-2]) % 8)).contiguous()
            run_el, run_lo = (lambda: el(images)), (lambda: lo(lo_images))
            t = dict(eloftr=[], loftr=[])
            for _ in range(3):                                           # alternate: the two share the host and the clocks
                t["eloftr"].append(timed(run_el, args.iters, args.warmup))
                t["loftr"].append(timed(run_lo, args.iters, args.warmup))
            o_el, o_lo = run_el(), run_lo()
            e, l = float(np.median(t["eloftr"])), float(np.median(t["loftr"]))
            rec["arithmetic"][split] = dict(
                eloftr_stage_ms=round(e, 3), loftr_stage_ms=round(l, 3), loftr_over_eloftr=round(l / e, 3),
                eloftr_pairs_per_s=round(args.pairs / e * 1e3, 1), loftr_pairs_per_s=round(args.pairs / l * 1e3, 1),
                eloftr_runs_ms=[round(v, 3) for v in t["eloftr"]], loftr_runs_ms=[round(v, 3) for v in t["loftr"]],
                eloftr_n_corr_mean=float(o_el["n_corr"].float().mean()), loftr_n_corr_mean=float(o_lo["n_corr"].float().mean()),
                eloftr_split=eloftr_split(el, images, args.iters, args.warmup))
            print(split, json.dumps({k: v for k, v in rec["arithmetic"][split].items() if k != "eloftr_split"}))
            print(split, json.dumps(rec["arithmetic"][split]["eloftr_split"]))
            del el, lo
            torch.cuda.empty_cache()
    options.reset()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
