"""Generate tests/golden/ref_scannet.npz by EXECUTING THE REFERENCE'S OWN ScanNet reader and metrics (needs the reference checkout; never
run on the GPU box):

  * lib/datasets/scannet.py  ScanNetScene on the tiny tree of tests/scannet_tree.py (2 scene folders, 5 pairs): pair names, both K,
    T_0to1 / T_1to0, pair_id, depth (16-bit PGM and the estimated-depth npz), and the `mode not in ['val' or 'test']` quirk on an index
    file that carries a `score` column;
  * lib/utils/metrics.py     pose_error_torch through MetricsAccumulator on 200 seeded poses (some NaN), error_auc tables, precision,
    A_metrics.

cv2 is not installed: it is stubbed at import, with imread served by PIL (depth values come out of the file's own 16-bit words; the colour
image is not stored).  The tree's parameters go into the fixture, so tests/test_scannet_reader.py rebuilds the same files anywhere."""
import os
import sys
import tempfile
import types

import numpy as np
import torch

REF = os.environ.get("MFR_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "..", "tests", "golden", "ref_scannet.npz")


def stub_cv2():
    from PIL import Image
    cv = types.ModuleType("cv2")
    cv.IMREAD_COLOR, cv.IMREAD_UNCHANGED, cv.COLOR_BGR2RGB = 1, -1, 4
    cv.imread = lambda path, flag=1: np.asarray(Image.open(path))
    cv.cvtColor = lambda img, code: img
    cv.resize = lambda img, wh: np.zeros((wh[1], wh[0]) + img.shape[2:], img.dtype)     # (the colour image is not part of the fixture)
    sys.modules["cv2"] = cv


def make_poses(n=200, seed=7):
    """ground truth + estimates a few degrees / centimetres off, every 17th estimate NaN (a pair without a pose)"""
    g = torch.Generator().manual_seed(seed)

    def rot(scale):
        w = torch.randn(n, 3, generator=g) * scale
        K = torch.zeros(n, 3, 3)
        K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -w[:, 2], w[:, 1], w[:, 2], -w[:, 0], -w[:, 1], w[:, 0]
        return torch.linalg.matrix_exp(K)
    Rgt, tgt = rot(1.0), torch.randn(n, 3, generator=g)
    T = torch.eye(4).repeat(n, 1, 1)
    T[:, :3, :3], T[:, :3, 3] = Rgt, tgt
    R = (rot(0.08) @ Rgt).contiguous()
    t = (tgt * (1 + 0.2 * torch.randn(n, 1, generator=g)) + 0.08 * torch.randn(n, 3, generator=g))[:, None, :].contiguous()
    R[::17], t[::17] = float("nan"), float("nan")
    return R, t, T


def main():
    stub_cv2()
    if not hasattr(np, "trapz"):
        np.trapz = np.trapezoid
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.join(HERE, "..", "tests"))
    from lib.datasets.scannet import ScanNetScene
    from lib.utils import metrics as M
    import scannet_tree as ST
    p = ST.default_params()
    out = {f"tree_{k}": np.asarray(v) for k, v in p.items()}
    resize = (int(p["width"]), int(p["height"]))
    with tempfile.TemporaryDirectory() as td:
        tr = ST.write_tree(td, p)
        for tag, est in (("gt", None), ("est", tr["est_npz"])):
            sc = ScanNetScene(tr["scans"], tr["test_npz"], mode="test", min_overlap_score=float(p["min_overlap_score"]), resize=resize,
                              estimated_depth=est)
            smp = [sc[i] for i in range(len(sc))]
            out[f"{tag}_depth0"] = np.stack([s["depth0"].numpy() for s in smp])
            out[f"{tag}_depth1"] = np.stack([s["depth1"].numpy() for s in smp])
            if tag == "gt":
                out["pair_names"] = np.array([list(s["pair_names"]) for s in smp])
                out["scene_id"] = np.array([s["scene_id"] for s in smp])
                out["pair_id"] = np.array([s["pair_id"] for s in smp], np.int64)
                out["K_color0"] = np.stack([s["K_color0"].numpy() for s in smp]); out["K_color1"] = np.stack([s["K_color1"].numpy() for s in smp])
                out["K_depth"] = np.stack([s["K_depth"].numpy() for s in smp])
                out["T_0to1"] = np.stack([s["T_0to1"].numpy() for s in smp]); out["T_1to0"] = np.stack([s["T_1to0"].numpy() for s in smp])
                assert out["K_color0"].dtype == np.float64 and out["T_0to1"].dtype == np.float32 and out["gt_depth0"].dtype == np.float32
        val = ScanNetScene(tr["scans"], tr["test_npz"], mode="val", resize=resize)
        out["val_depth_numel"] = np.int64(val[0]["depth0"].numel())
        for mode in ("train", "val", "test"):                       # the quirk: the score filter is skipped in 'val' only
            sc = ScanNetScene(tr["scans"], tr["scored_npz"], mode=mode, min_overlap_score=float(p["min_overlap_score"]), resize=resize)
            out[f"scored_names_{mode}"] = np.asarray(sc.data_names, np.int64)
    R, t, T = make_poses()
    out["pose_R"], out["pose_t"], out["pose_T"] = R.numpy(), t.numpy(), T.numpy()
    macc = M.MetricsAccumulator()
    for i in range(len(R)):                                         # batch 1, as benchmark/scannet.py:30-35
        macc.accumulate(M.pose_error_torch(R[i:i + 1], t[i:i + 1], T[i:i + 1]))
    agg = macc.aggregate()
    for k, v in agg.items():
        out[f"agg_{k}"] = v
    pose_err = np.maximum(agg["R_err"], agg["t_err_ang"])
    for name, err, thr in (("pose", pose_err, (5, 10, 20)), ("rotation", agg["R_err"], (5, 10, 20)),
                           ("translation_ang", agg["t_err_ang"], (5, 10, 20)), ("translation_euc", agg["t_err_euc"], (0.1, 0.5, 1))):
        out[f"auc_{name}"] = np.array(list(M.error_auc(err, thr).values()), np.float64)
    out["precision"] = np.array([M.precision(agg, r, m) for m, r in ((0.1, 5), (0.25, 5), (0.5, 10), (1, 20))], np.float64)
    out["A_metrics"] = np.array([float(a) for a in M.A_metrics(agg["t_err_scale_sym"])], np.float64)
    np.savez_compressed(OUT, **out)
    print(f"wrote {os.path.normpath(OUT)}: {len(out)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
