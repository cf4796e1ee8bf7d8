"""Matcher-stage time of LightGlue and SuperGlue on the bench's synthetic workload (32 pairs, 1024 keypoints, 540 x 720): SuperPoint runs once,
outside the timed region; each matcher is timed with HIP events after a warm-up, the two alternating, in both HIP.SPLIT arithmetics.  The
per-kernel split of the LightGlue stage times each launch of one block on the stage's own buffers (events around repeated launches; calls per
stage = how often the stage issues it).  Writes profiles/lightglue_stage.json.

    python tools/bench_lightglue.py [--pairs 32] [--iters 20] [--warmup 5] [--out profiles/lightglue_stage.json]
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
from mapfree_reloc_amd.nets.lightglue import LightGlueHIP  # noqa: E402
from mapfree_reloc_amd.nets.superglue import SuperGlueHIP  # noqa: E402
from mapfree_reloc_amd.nets.superpoint import SuperPointHIP  # noqa: E402

H, W, K = 720, 540, 1024


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


def lightglue_split(net, sp, iters, warmup):
    """ms per launch of each kernel of the LightGlue stage, and launches per stage call"""
    kpts, desc, n = sp["kpts"], sp["desc"], sp["n"]
    B2 = kpts.shape[0]
    cs = net.rotary_table(net.normalize_keypoints(kpts, (H, W)))
    xa = torch.empty(B2 * K, 512, device=kpts.device)
    xa[:, :256] = desc.reshape(B2 * K, 256)
    xa[:, 256:] = 0
    qkv = torch.empty(B2 * K, 768, device=kpts.device)
    hid = torch.empty(B2 * K, 512, device=kpts.device)
    L = net.blocks[0]
    lib = _lib.load()
    x = net.final_descriptors(kpts, desc, n, (H, W))
    S, z0, z1 = net.similarity(x)
    n0, n1 = n[0::2].contiguous(), n[1::2].contiguous()
    nb = len(net.blocks)
    stages = [
        ("rotary_table", 1, lambda: net.rotary_table(net.normalize_keypoints(kpts, (H, W)))),
        ("gemm_qkv_256x768", nb, lambda: L["lin_qkv"](xa[:, :256], out=qkv)),
        ("rotary_apply", nb // 2, lambda: net.rotate(qkv, cs)),
        ("attention_self", nb // 2, lambda: net.attention(qkv.view(B2, K, 768), n, False, xa[:, 256:], 512)),
        ("attention_cross", nb // 2, lambda: net.attention(qkv.view(B2, K, 768), n, True, xa[:, 256:], 512)),
        ("gemm_fc1_512x512_ln_gelu_epilogue", nb if net.mlp == "epilogue" else 0, lambda: L["lin1"].ln_gelu(xa, L["ln"], hid)),
        ("gemm_fc1_512x512", 0 if net.mlp == "epilogue" else nb, lambda: L["lin1"](xa, out=hid)),
        ("ln_gelu_512", 0 if net.mlp == "epilogue" else nb, lambda: _lib.check(lib.mfr_lg_ln_gelu(hid.data_ptr(), 512, B2 * K, _lib.ptr(L["ln"][0]), _lib.ptr(L["ln"][1]), 1e-5, _lib.stream_ptr()), "ln_gelu")),
        ("gemm_fc2_512x256_accumulate", nb, lambda: L["lin2"](hid, out=qkv[:, :256], accumulate=True)),
        ("final_projection_and_similarity", 1, lambda: net.similarity(x)),
        ("assign", 1, lambda: net.assign(S, z0, z1, n0, n1, kpts[0::2], kpts[1::2], K)),
    ]
    out = {}
    for name, calls, fn in stages:
        ms = timed(fn, iters, warmup)
        out[name] = dict(ms_per_launch=round(ms, 4), launches_per_stage=calls, ms_per_stage=round(ms * calls, 4))
    out["sum_ms"] = round(sum(v["ms_per_stage"] for v in out.values()), 4)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lightglue_stage.json"))
    args = ap.parse_args(argv)
    _lib.load(require_gpu=True)
    dev = torch.device("cuda:0")
    sb = IM.synthetic_batch([100 + i for i in range(args.pairs)], H, W)
    images = torch.from_numpy(np.ascontiguousarray(sb["images"])).to(dev)
    rec = dict(workload=dict(pairs=args.pairs, keypoints=K, image_hw=[H, W], iters=args.iters, warmup=args.warmup), device=torch.cuda.get_device_name(0),
               note="matcher stage only (SuperPoint excluded), HIP events, seeded synthetic weights; ms per batch of pairs", arithmetic={})
    for split in ("f16x2", "bf16x3"):
        options.reset()
        with options.override(SPLIT=split), torch.no_grad():
            sp = SuperPointHIP(WT.superpoint_state_dict(), dev, max_keypoints=K)(images)
            lg = LightGlueHIP(WT.lightglue_state_dict(), dev)
            lg_pass = LightGlueHIP(WT.lightglue_state_dict(), dev, mlp="epilogue" if lg.mlp == "pass" else "pass")     # the other MLP form, for the A/B
            sg = SuperGlueHIP(WT.superglue_state_dict(), dev)
            run_lg = lambda: lg(sp, (H, W), maxN=K)
            run_sg = lambda: sg(sp, (H, W), maxN=K)
            run_other = lambda: lg_pass(sp, (H, W), maxN=K)
            t = dict(lightglue=[], superglue=[], other=[])
            for _ in range(3):                                           # alternate: the two share the host and the clocks
                t["lightglue"].append(timed(run_lg, args.iters, args.warmup))
                t["superglue"].append(timed(run_sg, args.iters, args.warmup))
                t["other"].append(timed(run_other, args.iters, args.warmup))
            o_lg, o_sg = run_lg(), run_sg()
            rec["arithmetic"][split] = dict(
                lightglue_stage_ms=round(float(np.median(t["lightglue"])), 4), superglue_stage_ms=round(float(np.median(t["superglue"])), 4),
                lightglue_mlp=lg.mlp, **{f"lightglue_stage_ms_mlp_{lg_pass.mlp}": round(float(np.median(t["other"])), 4)},
                lightglue_runs_ms=[round(v, 4) for v in t["lightglue"]], superglue_runs_ms=[round(v, 4) for v in t["superglue"]],
                keypoints_mean=float(sp["n"].float().mean()), lightglue_n_corr_mean=float(o_lg["n_corr"].float().mean()),
                superglue_n_corr_mean=float(o_sg["n_corr"].float().mean()), lightglue_split=lightglue_split(lg, sp, args.iters, args.warmup))
            print(split, json.dumps({k: v for k, v in rec["arithmetic"][split].items() if k != "lightglue_split"}))
    options.reset()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
