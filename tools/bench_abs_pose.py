"""Time the 7Scenes pose fusion (localize_ops.fuse_abs_pose -> mfr_abs_pose_fuse) on a run of the benchmark's size -- 17 000 synthetic
queries x 5 neighbours from the fixture's recipe (tools/gen_sevenscenes_golden.draw_query) -- against its numpy mirror
tests/abs_pose_ref.py on the host, and write both to profiles/abs_pose_fuse.json.

    python tools/bench_abs_pose.py [--queries 17000] [--neighbours 5] [--reps 20] [--host_queries 500] [--out profiles/abs_pose_fuse.json]

Device: inputs resident, `reps` launches after a warm-up, host clock around the loop ending in a synchronise.  Host: the mirror over the
first `host_queries` queries (pure Python around numpy: per-query time, extrapolated to the whole run and labelled so).  The two are
compared on those queries before anything is timed."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
sys.path.insert(0, HERE)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=17000)
    ap.add_argument("--neighbours", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host_queries", type=int, default=500)
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "abs_pose_fuse.json"))
    args = ap.parse_args(argv)
    import torch
    import abs_pose_ref as M
    from gen_sevenscenes_golden import draw_query
    from mapfree_reloc_amd import localize_ops as LO
    Q, k = args.queries, args.neighbours
    rng = np.random.default_rng(7000 + k)
    qs = [draw_query(rng, k) for _ in range(Q)]
    inp = {key: np.concatenate([q[key].reshape(k, -1) for q in qs]) for key in ("train_q", "train_c", "R_pred", "t_pred")}
    offsets = np.arange(Q + 1, dtype=np.int32) * k
    dev = torch.device("cuda", 0)
    d = {key: torch.from_numpy(v).to(dev) for key, v in inp.items()}
    doff = torch.from_numpy(offsets).to(dev)
    rec = dict(queries=Q, neighbours=k, reps=args.reps, host_queries=args.host_queries, device=torch.cuda.get_device_name(0))
    nh = min(args.host_queries, Q)
    for mode, name in ((1, "triangulation_ransac"), (0, "median_chordal_mean")):
        call = lambda: LO.fuse_abs_pose(d["train_q"], d["train_c"], d["R_pred"], d["t_pred"], doff, mode, 15.0, 1.414, 10, 0, device=dev)
        out = call()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mir = M.fuse(inp["train_q"][:nh * k], inp["train_c"][:nh * k], inp["R_pred"][:nh * k], inp["t_pred"][:nh * k], offsets[:nh + 1], mode, 15.0, 1.414, 10, 0)
        host_s = time.perf_counter() - t0
        same_mask = bool(np.array_equal(out["inlier_mask"][:nh * k].cpu().numpy(), mir["inlier_mask"]))
        dc = float(np.abs(out["abs_c"][:nh].cpu().numpy() - mir["abs_c"]).max())
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            call()
        torch.cuda.synchronize()
        dev_ms = (time.perf_counter() - t0) / args.reps * 1e3
        rec[name] = dict(device_ms_per_launch=dev_ms, device_queries_per_s=Q / dev_ms * 1e3, host_mirror_ms_per_query=host_s / nh * 1e3,
                         host_mirror_s_extrapolated_to_all_queries=host_s / nh * Q, masks_equal_on_host_queries=same_mask,
                         max_centre_diff_m_on_host_queries=dc, status_counts={str(s): int(n) for s, n in zip(*np.unique(out["status"].cpu().numpy(), return_counts=True))})
        print(name, json.dumps(rec[name]))
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
