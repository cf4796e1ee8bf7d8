"""The rig solvers of the multi-frame model side by side: what the pooled 3-D/3-D solve ('RigProcrustes', the rig entry point of
csrc/procrustes.hip) and the depth-free solve ('RigEssentialMatrix', csrc/emat_rig.hip, per stage) cost on the GPU next to rig PnP
(csrc/pnp_rig.hip) and next to the T single-frame solves they replace, and what they buy on seeded synthetic rigs.

    python tools/bench_rig_solvers.py [--out profiles/rig_solvers.json] [--reps 10] [--no-gpu]

GPU part (tools/bench_rig_pnp.py's shape: B = 32 samples, T = 9 frames, 1024 correspondences per frame; each solver at the iteration count the
model runs it with): median of three timed windows of `reps` calls, the solvers alternating window by window, spread = max - min of a
solver's windows.  No target is set: these are fp64, latency-bound kernels; the record shows whether the pooled solve costs more than the T
solves it replaces.  Inputs: tests/rig_scenes_depth.py scenes (0.5 px noise, 30 % outliers, query depth consistent with the geometry).

CPU part (SYNTHETIC data, from the numpy mirrors under tests/): over 32 seeded rigs of 9 frames and 60 correspondences per frame, the median
rotation and translation error of RigProcrustes, RigEssentialMatrix (its mirror on the oracle's single-frame E-matrix results), rig PnP, and
Procrustes on the last frame alone, with the rigs' largest baseline beside them."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import mapfree_reloc_amd  # noqa: E402,F401
import rig_emat_ref as ME  # noqa: E402
import rig_pnp_ref as MP  # noqa: E402
import rig_procrustes_ref as MR  # noqa: E402
import rig_scenes as S  # noqa: E402
import rig_scenes_depth as D  # noqa: E402

SEEDS = range(1000, 1032)


def accuracy():
    from oracle import oracle_lib as O
    err = {"rig_procrustes_T9": [], "rig_pnp_T9": [], "procrustes_last_frame": [], "rig_essential_matrix_T9": []}
    base = []
    for seed in SEEDS:
        sc = D.make_rig_scene(seed, 9, 60)
        a = MR.rig_procrustes_solve(sc["pts0"], sc["pts1"], sc["depth0"], sc["depth1"], sc["K0"], sc["K1"], sc["rig_T"], max_dist=D.MAX_CORR_DIST, pair_id=seed)
        b = MP.rig_pnp_solve(sc["pts0"], sc["pts1"], sc["depth0"], sc["K0"], sc["K1"], sc["rig_T"], max_iters=1000, all_counts=False, pair_id=seed)
        c = MR.rig_procrustes_solve(sc["pts0"][8:], sc["pts1"][8:], sc["depth0"], sc["depth1"][8:], sc["K0"], sc["K1"][8:], sc["rig_T"][8:],
                                    max_dist=D.MAX_CORR_DIST, pair_id=seed)
        s1 = [O.emat_solve(sc["pts0"][j], sc["pts1"][j], sc["K0"], sc["K1"][j], 2.0, 0.9999, 1000, 0, seed * 9 + j) for j in range(9)]
        e = ME.rig_emat_stage2(sc["pts0"], sc["pts1"], sc["K0"], sc["K1"], sc["rig_T"], [x["R"] for x in s1], [x["t"] for x in s1],
                               [x["n_inl"] for x in s1], [x["status"] for x in s1], [x["mask"].astype(bool) for x in s1], pix_thr=2.0)
        for k, r in zip(err, (a, b, c, e)):
            assert r["status"] == 0, (k, seed)
            err[k].append(S.pose_error(r["R"], r["t"], sc["R"], sc["t"]))
        # camera centres of the window frames in the last frame's coordinates: c_j = -R_Aj^T t_Aj; the largest distance between two of them
        cen = np.array([-A[:3, :3].T @ A[:3, 3] for A in sc["rig_T"]])
        base.append(float(np.max(np.linalg.norm(cen[:, None] - cen[None], axis=2))))
    out = {"data": "synthetic: tests/rig_scenes_depth.make_rig_scene(seed, 9, 60), seeds 1000..1031, 0.5 px noise, 30 % outliers, MAX_CORR_DIST 0.1 m, "
                   "rig PnP at 3 px / 1000 iterations, E-matrix at 2 px / 1000 iterations", "largest_baseline_m_median": round(float(np.median(base)), 4)}
    for k, v in err.items():
        v = np.array(v)
        out[k] = {"median_rot_rad": round(float(np.median(v[:, 0])), 5), "median_trans_m": round(float(np.median(v[:, 1])), 5)}
    return out


def gpu_times(B, T, n, reps):
    import torch
    from bench_rig_pnp import summary, windows
    from mapfree_reloc_amd import solver_ops as ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_rig_solvers.py measures on the GPU: no HIP device visible (--no-gpu for the CPU table alone)")
    pk = D.pack([D.make_rig_scene(100 + b, T, n) for b in range(B)])
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in pk.items()}
    pids = torch.arange(B, dtype=torch.int64, device="cuda") * 5
    rows = lambda x: x.reshape((B * T,) + tuple(x.shape[2:])).contiguous()
    rep = lambda x: x.repeat_interleave(T, dim=0).contiguous()
    flat = dict(pts0=rows(d["pts0"]), pts1=rows(d["pts1"]), n_corr=rows(d["n_corr"]), depth0=rep(d["depth0"]), depth1=rows(d["depth1"]), K0=rep(d["K0"]),
                K1=rows(d["K1"]), pids=torch.arange(B * T, dtype=torch.int64, device="cuda"))
    rp, pr = ops.RigProcrustesBatchSolver(D.MAX_CORR_DIST, 0.999, 0), ops.ProcrustesBatchSolver(D.MAX_CORR_DIST, 0.999, 0)
    rn = ops.RigPnPBatchSolver(1000, 3.0, 0.9999, 0)
    re_, em = ops.RigEssentialBatchSolver(2.0, 0.9999, 0), ops.EssentialBatchSolver(2.0, 0.9999, 0)
    s1 = ops.rig_emat_stage1(em, d["pts0"], d["pts1"], d["n_corr"], d["K0"], d["K1"], pids)
    fns = {
        "rig_procrustes": lambda: rp(d["pts0"], d["pts1"], d["n_corr"], d["depth0"], d["depth1"], d["K0"], d["K1"], d["rig_T"], pids),
        "procrustes_rows": lambda: pr(flat["pts0"], flat["pts1"], flat["n_corr"], flat["depth0"], flat["depth1"], flat["K0"], flat["K1"], flat["pids"]),
        "rig_pnp": lambda: rn(d["pts0"], d["pts1"], d["n_corr"], d["depth0"], d["K0"], d["K1"], d["rig_T"], pids),
        "rig_emat_both_stages": lambda: re_(d["pts0"], d["pts1"], d["n_corr"], d["K0"], d["K1"], d["rig_T"], pids),
        "rig_emat_stage1_emat_rows": lambda: em(flat["pts0"], flat["pts1"], flat["n_corr"], flat["K0"], flat["K1"], flat["pids"]),
        "rig_emat_stage2": lambda: ops.rig_emat_stage2(d["pts0"], d["pts1"], d["n_corr"], d["K0"], d["K1"], d["rig_T"], s1),
    }
    res = {"shape": {"B": B, "T": T, "points_per_frame": n, "reps_per_window": reps,
                     "iterations": {"rig_procrustes": rp.max_iters, "procrustes_rows": pr.max_iters, "rig_pnp": rn.max_iters, "emat": em.max_iters}},
           "device": torch.cuda.get_device_properties(0).gcnArchName}
    res["solve_batch"] = {k: summary(v) for k, v in windows(fns, reps).items()}
    res["solve_batch"]["rig_procrustes_minus_procrustes_rows_ms"] = round(
        res["solve_batch"]["rig_procrustes"]["median_ms"] - res["solve_batch"]["procrustes_rows"]["median_ms"], 4)
    res["solve_batch"]["rig_emat_stage2_share"] = round(res["solve_batch"]["rig_emat_stage2"]["median_ms"] / res["solve_batch"]["rig_emat_both_stages"]["median_ms"], 3)
    o, oe = fns["rig_procrustes"](), fns["rig_emat_both_stages"]()
    res["solved"] = {"rig_procrustes_ok": int((o["status"] == 0).sum()), "rig_procrustes_median_inliers": float(o["n_inliers"].float().median()),
                     "rig_emat_ok": int((oe["status"] == 0).sum()), "rig_emat_median_inliers": float(oe["n_inliers"].float().median())}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/rig_solvers.json")
    ap.add_argument("--B", type=int, default=32); ap.add_argument("--T", type=int, default=9); ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-gpu", action="store_true")
    a = ap.parse_args()
    res = {} if a.no_gpu else gpu_times(a.B, a.T, a.n, a.reps)
    if res:
        print("solve_batch", json.dumps(res["solve_batch"]), flush=True)
    res["accuracy_cpu_mirrors"] = accuracy()
    print("accuracy", json.dumps(res["accuracy_cpu_mirrors"]), flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
