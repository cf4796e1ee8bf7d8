"""Rig PnP solver (csrc/pnp_rig.hip) timed on the GPU against its yardstick, the single-camera PnPBatchSolver on the same [B*T] rows:
both score iterations x (sum of points) reprojections.  Default shape: B = 32 samples, T = 9 frames, 1024 correspondences per frame,
1000 iterations.  Also the model plugin per sample (FeatureMatchingMultiFrame, T = 9, SuperGlue on synthetic weights) next to the
single-frame plugin on the same scene (what tools/bench_plugin.py times).

    python tools/bench_rig_pnp.py [--out profiles/rig_pnp.json] [--reps 20] [--no-plugin]

Each figure is the median of three timed windows of `reps` calls (host clock around work that ends in a device synchronise, after a
warm-up); the two solvers alternate window by window; the baseline's run-to-run spread (max - min of its three windows) is reported
so that a difference can be judged against it.  Inputs: synth.make_pair scenes of 9 * 1024 correspondences (30 % outliers, 1 px noise)
cut into 9 frames; frames 0..7 are moved by a seeded rig (<= 10 degrees, <= 0.3 m) and their true observations re-projected."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mapfree_reloc_amd  # noqa: E402,F401
from mapfree_reloc_amd import solver_ops as ops, synth  # noqa: E402


def rig_batch(B, T, n, seed0=100):
    p0 = np.zeros((B, T, n, 2), np.float32); p1 = np.zeros((B, T, n, 2), np.float32)
    depth, K0, K1, rig = [], np.zeros((B, 3, 3), np.float32), np.zeros((B, T, 3, 3), np.float32), np.tile(np.eye(4), (B, T, 1, 1))
    for b in range(B):
        pr = synth.make_pair(seed0 + b, T * n, outlier_frac=0.3)
        rng = np.random.default_rng(seed0 + b)
        depth.append(pr["depth0"]); K0[b] = pr["K0"]; K1[b] = pr["K1"]
        a, c = pr["pts0"].reshape(T, n, 2), pr["pts1"].reshape(T, n, 2).copy()
        inl = pr["inlier_gt"].reshape(T, n)
        Ki, K = np.linalg.inv(pr["K0"].astype(np.float64)), pr["K1"].astype(np.float64)
        for j in range(T - 1):
            RA = synth.rand_rot(rng, 10.0)
            tA = rng.normal(size=3); tA *= rng.uniform(0.0, 0.3) / np.linalg.norm(tA)
            rig[b, j, :3, :3], rig[b, j, :3, 3] = RA, tA
            px = a[j].astype(np.int32)
            X = pr["depth0"][px[:, 1], px[:, 0]].astype(np.float64)[:, None] * (Ki @ np.stack([px[:, 0], px[:, 1], np.ones(n)])).T
            Y = (RA @ (pr["R_gt"] @ X.T + pr["t_gt"][:, None]) + tA[:, None]).T
            x = (K @ (Y / Y[:, 2:3]).T).T[:, :2] + rng.normal(size=(n, 2))
            c[j][inl[j]] = x[inl[j]]
        p0[b], p1[b] = a, c
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return dict(pts0=d(p0), pts1=d(p1), n_corr=torch.full((B, T), n, dtype=torch.int32, device="cuda"), depth0=d(np.stack(depth)),
                K0=d(K0), K1=d(K1), rig_T=d(rig), pair_ids=torch.arange(B, dtype=torch.int64, device="cuda") * 5)


def windows(fns, reps, n_windows=3):
    """fns: name -> callable.  Three windows each, alternating; -> name -> list of ms per call"""
    for f in fns.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(n_windows):
        for k, f in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                f()
            torch.cuda.synchronize()
            out[k].append(1e3 * (time.perf_counter() - t0) / reps)
    return out


def summary(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "windows_ms": [round(v, 4) for v in ms], "spread_ms": round(max(ms) - min(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/rig_pnp.json")
    ap.add_argument("--B", type=int, default=32); ap.add_argument("--T", type=int, default=9)
    ap.add_argument("--n", type=int, default=1024); ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-plugin", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rig_pnp.py measures on the GPU: no HIP device visible")
    B, T, n = a.B, a.T, a.n
    bt = rig_batch(B, T, n)
    rows = lambda x: x.reshape((B * T,) + tuple(x.shape[2:])).contiguous()
    rep = lambda x: x.repeat_interleave(T, dim=0).contiguous()
    flat = dict(pts0=rows(bt["pts0"]), pts1=rows(bt["pts1"]), n_corr=rows(bt["n_corr"]), depth0=rep(bt["depth0"]), K0=rep(bt["K0"]), K1=rows(bt["K1"]),
                pair_ids=torch.arange(B * T, dtype=torch.int64, device="cuda"))
    rig, pnp = ops.RigPnPBatchSolver(a.iters, 3.0, 0.9999, 0), ops.PnPBatchSolver(a.iters, 3.0, 0.9999, 0)
    solve = {
        "pnp_rows": lambda: pnp(flat["pts0"], flat["pts1"], flat["n_corr"], flat["depth0"], flat["K0"], flat["K1"], flat["pair_ids"]),
        "rig": lambda: rig(bt["pts0"], bt["pts1"], bt["n_corr"], bt["depth0"], bt["K0"], bt["K1"], bt["rig_T"], bt["pair_ids"]),
    }
    # the RANSAC stage alone on the same lifted rows (the lift of the baseline reads B*T depth maps, the rig's B)
    xyz, obs, _, nv = ops.pnp_lift(flat["pts0"], flat["pts1"], flat["n_corr"], flat["depth0"], flat["K0"])
    rr = ops.rig_rows(bt["rig_T"])
    x4, o4, n2 = xyz.reshape(B, T, n, 3), obs.reshape(B, T, n, 2), nv.reshape(B, T)
    stage = {
        "pnp_rows": lambda: ops.pnp_ransac(xyz, obs, nv, flat["K1"], flat["pair_ids"], a.iters),
        "rig": lambda: ops.rig_pnp_ransac(x4, o4, n2, bt["K1"], rr, bt["pair_ids"], a.iters),
    }
    res = {"shape": {"B": B, "T": T, "points_per_frame": n, "iterations": a.iters, "reps_per_window": a.reps},
           "device": torch.cuda.get_device_properties(0).gcnArchName}
    for name, fns in (("solve_batch", solve), ("ransac_stage", stage)):
        w = windows(fns, a.reps)
        res[name] = {k: summary(v) for k, v in w.items()}
        res[name]["rig_minus_pnp_rows_ms"] = round(res[name]["rig"]["median_ms"] - res[name]["pnp_rows"]["median_ms"], 4)
        print(name, json.dumps(res[name]), flush=True)
    out_r, out_p = solve["rig"](), solve["pnp_rows"]()
    res["solved"] = {"rig_ok": int((out_r["status"] == 0).sum()), "rig_median_inliers": float(out_r["n_inliers"].float().median()),
                     "pnp_rows_ok": int((out_p["status"] == 0).sum())}
    if not a.no_plugin:
        res["model_plugin"] = plugin_times(T)
        print("model_plugin", json.dumps(res["model_plugin"]), flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


def plugin_times(T, n_samples=8):
    """ms per sample of build_model(cfg)(data): the multi-frame model on windows of T synthetic frames (identity rig: the time does not
    depend on the rig's values) and the single-frame model on the same scene's pairs"""
    from mapfree_reloc_amd.builder import build_model
    from mapfree_reloc_amd.config import get_cfg_defaults
    from mapfree_reloc_amd.datasets import SyntheticScene, collate_batch1

    def cfg_for(model):
        cfg = get_cfg_defaults()
        cfg.MODEL, cfg.FEATURE_MATCHING, cfg.POSE_SOLVER = model, "SuperGlue", "PNP"
        cfg.PNP.RANSAC_ITER, cfg.PNP.REPROJECTION_INLIER_THRESHOLD, cfg.PNP.CONFIDENCE = 1000, 3, 0.9999
        cfg.ALLOW_SYNTHETIC_WEIGHTS = True
        return cfg
    sc = SyntheticScene(0, frames=n_samples + T)
    single = [sc[i] for i in range(len(sc))]
    multi = []
    for k in range(n_samples):
        w = single[k:k + T]
        s = dict(w[-1])
        s["image1"] = torch.stack([x["image1"] for x in w]); s["depth1"] = torch.stack([x["depth1"] for x in w])
        s["K_color1_multi"] = torch.stack([x["K_color1"] for x in w]).to(torch.float64)
        s["rig_T"] = torch.eye(4, dtype=torch.float64).repeat(T, 1, 1)
        s["pair_names"] = (w[-1]["pair_names"][0], tuple(x["pair_names"][1] for x in w))
        multi.append(collate_batch1(s))
    out = {}
    for name, model, samples in (("FeatureMatching:SuperGlue+PNP", "FeatureMatching", [collate_batch1(s) for s in single[:n_samples]]),
                                 (f"FeatureMatchingMultiFrame(T={T}):SuperGlue+PNP", "FeatureMatchingMultiFrame", multi)):
        m = build_model(cfg_for(model))
        for s in samples[:2]:
            m(s)
        torch.cuda.synchronize()
        ms = []
        for _ in range(3):
            t0 = time.perf_counter()
            for s in samples:
                m(s)
            torch.cuda.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0) / len(samples))
        out[name] = {"ms_per_sample": round(float(np.median(ms)), 2), "windows_ms": [round(v, 2) for v in ms]}
    return out


if __name__ == "__main__":
    main()
