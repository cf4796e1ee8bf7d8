"""A/B timing of LoFTR's coarse matching at the Map-free size (6120 x 6120 per pair) on the same S: dual softmax variant 0 (csrc/loftr.hip),
optimal transport variant 0 (iters + 1 sweeps) and variant 1 (2 iters + 1 sweeps) of csrc/loftr_ot.hip, 3 Sinkhorn iterations, HIP events
after a warm-up.

  ab_ot_coarse_match.py [--out FILE]         driver: one child process per batch size (16 and 1 pairs), each under its own timeout; merges the
                                             children's lines into profiles/ot_coarse_match.json (the driver itself never opens the GPU)
  ab_ot_coarse_match.py --child B [--only K] one JSON line for B pairs (K in dsm0 | ot0 | ot1: that kernel family alone, one warm-up and one
                                             timed launch -- the form a `rocprofv3 --pmc FETCH_SIZE` pass wraps, counters in a run of their own)
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, ITERS, GAIN = 90, 68, 3, 3.0


def child(B, only=None):
    sys.path.insert(0, ROOT)
    import torch
    from mapfree_reloc_amd.nets import weights as WT
    from mapfree_reloc_amd.nets.loftr import LoFTRHIP
    dev = torch.device("cuda:0")
    net = LoFTRHIP(WT.loftr_state_dict(), dev, skh_iters=ITERS)
    L = H * W
    g = torch.Generator(device="cuda").manual_seed(0)
    f0 = torch.randn(B, L, 256, device=dev, generator=g) * GAIN
    f1 = f0[:, torch.randperm(L, device=dev, generator=g)] + 0.3 * GAIN / 2.2 * torch.randn(B, L, 256, device=dev, generator=g)
    S = torch.bmm(f0 / 256.0, f1.transpose(1, 2))
    del f0, f1
    runs = {"dsm0": lambda: net.coarse_match(S, (H, W), (H, W), variant=0), "ot0": lambda: net.ot_match(S, (H, W), (H, W), variant=0),
            "ot1": lambda: net.ot_match(S, (H, W), (H, W), variant=1)}
    sweeps = {"dsm0": 2, "ot0": ITERS + 1, "ot1": 2 * ITERS + 1}
    res = {"pairs": B, "L": L, "S_bytes": S.numel() * 4, "skh_iters": ITERS, "feature_gain": GAIN}
    reps = 1 if only else (5 if B > 1 else 20)
    for name in ([only] if only else ["dsm0", "ot0", "ot1", "dsm0", "ot0", "ot1"]):
        runs[name]()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            out = runs[name]()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / reps
        res.setdefault(name + "_ms", []).append(round(ms, 4))
        res[name + "_sweeps"] = sweeps[name]
        res[name + "_sweep_GBs"] = round(sweeps[name] * S.numel() * 4 / (ms * 1e-3) / 1e9, 1)
        res[name + "_matches"] = int(out[3].sum())
    print(json.dumps(res))


def driver():
    rec = {"what": "LoFTR coarse matching on one S [B, 6120, 6120]: dual softmax variant 0 vs optimal transport variants 0 / 1 (3 iterations); "
                   "ms per call (two timed rounds each, HIP events, one process per batch size)", "runs": []}
    for B in (16, 1):
        try:
            p = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child", str(B)], capture_output=True, text=True)
        except OSError as e:
            rec["runs"].append({"pairs": B, "error": str(e)}); break
        lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
        if p.returncode != 0 or not lines:
            rec["runs"].append({"pairs": B, "returncode": p.returncode, "stderr_tail": p.stderr[-600:]})
            break                                             # nothing more is started on the GPU after a failed step
        r = json.loads(lines[-1])
        d, o0, o1 = min(r["dsm0_ms"]), min(r["ot0_ms"]), min(r["ot1_ms"])
        r["ot0_over_dsm0"] = round(o0 / d, 3)
        r["ot1_over_ot0"] = round(o1 / o0, 3)
        r["targets"] = {"ot0 <= 2.5 x dsm0": bool(o0 <= 2.5 * d), "ot0 faster than ot1": bool(o0 < o1)}
        rec["runs"].append(r)
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "ot_coarse_match.json")
    json.dump(rec, open(out, "w"), indent=1)
    print(json.dumps(rec))
    return 0 if all("ot0_ms" in r for r in rec["runs"]) else 1


if __name__ == "__main__":
    if "--child" in sys.argv:
        i = sys.argv.index("--child")
        child(int(sys.argv[i + 1]), sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None)
    else:
        sys.exit(driver())
