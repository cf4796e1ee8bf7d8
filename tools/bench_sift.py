"""SIFT on the GPU (csrc/sift.hip, sift_ops.py): the first throughput record of this path.  BASELINE configs[0] shape: SIFT(2048) +
E-mat metric on synthetic 540x720 pairs, B = 32 pairs per batch.
  detector   ms per image for B x 2 images in one call (pyramid, extrema, orientations, selection, descriptors), and the
             Gaussian pyramid's size; every level is written once and read at least twice (next blur / downsample, extrema, and
             orientation / descriptor windows), so 3 x pyramid bytes is a lower bound of the stage's HBM traffic
  pipeline   FusedPosePipeline(FEATURE_MATCHING 'SIFT', SIFT.DETECTOR 'hip', POSE_SOLVER 'EssentialMatrixMetric') pairs/s on the same
             device-resident batch (detector -> rootSIFT -> exact 2-NN + ratio 0.8 -> 5-point MAGSAC++ -> scale from depth)
Prints one JSON line; --out writes it to a file as well.
Usage: python tools/bench_sift.py [--batch 32] [--reps 5] [--out profiles/sift_bench_b32.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mapfree_reloc_amd import images as IM, sift_ops  # noqa: E402
from mapfree_reloc_amd.config import get_cfg_defaults  # noqa: E402
from mapfree_reloc_amd.pipeline import FusedPosePipeline  # noqa: E402

DEV = "cuda:0"


def timed(fn, reps):
    fn(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    B, H, W = a.batch, 720, 540
    pairs = [IM.synthetic_pair(100 + i, H, W) for i in range(B)]
    u8 = lambda x: np.round(np.clip(x, 0, 1) * 255).astype(np.uint8)
    gray = np.stack([u8(p[k]) for p in pairs for k in ("img0", "img1")])
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    batch = dict(images=d(gray.astype(np.float32) / np.float32(255))[:, None].contiguous(),
                 depth0=d(np.stack([p["depth0"] for p in pairs])), depth1=d(np.stack([p["depth1"] for p in pairs])),
                 K0=d(np.stack([p["K"] for p in pairs]).astype(np.float64)), K1=d(np.stack([p["K"] for p in pairs]).astype(np.float64)),
                 seed_ids=torch.arange(B, dtype=torch.int64, device=DEV))
    det = sift_ops.SiftDetector(2048, DEV)
    g = d(gray)
    det_ms = timed(lambda: det(g), a.reps)
    out = det(g)
    torch.cuda.synchronize()
    n = out["n"].cpu().numpy()
    pyr_bytes = sum(6 * 4 * (2 * H >> o) * (2 * W >> o) for o in range(sift_ops.num_octaves(H, W)))
    cfg = get_cfg_defaults()
    cfg.FEATURE_MATCHING, cfg.POSE_SOLVER = "SIFT", "EssentialMatrixMetric"
    cfg.SIFT.NUM_FEATURES, cfg.SIFT.RATIO_THRESHOLD, cfg.SIFT.DETECTOR = 2048, 0.8, "hip"
    cfg.EMAT_RANSAC.PIX_THRESHOLD, cfg.EMAT_RANSAC.SCALE_THRESHOLD, cfg.EMAT_RANSAC.CONFIDENCE = 2.0, 0.1, 0.9999
    pipe = FusedPosePipeline(cfg, DEV)
    step_ms = timed(lambda: pipe(batch), a.reps)
    res = pipe(batch)
    torch.cuda.synchronize()
    t_err = (res["t"].cpu().numpy() - np.stack([p["t_gt"] for p in pairs])).__abs__().max(1)
    rec = dict(metric="SIFT(2048) detector + E-mat metric, synthetic 540x720 pairs", device=torch.cuda.get_device_name(0), batch_pairs=B,
               images_per_call=2 * B, detector_ms_per_call=round(det_ms, 3), detector_ms_per_image=round(det_ms / (2 * B), 4),
               keypoints_per_image_mean=float(n.mean()), keypoints_per_image_min=int(n.min()), status_nonzero=int((out["status"] != 0).sum()),
               pyramid_bytes_per_image=pyr_bytes, pyramid_traffic_lower_bound_GBps=round(3 * pyr_bytes * 2 * B / (det_ms * 1e-3) / 1e9, 1),
               pipeline_ms_per_batch=round(step_ms, 3), pairs_per_s=round(B / (step_ms * 1e-3), 1),
               n_corr_mean=float(res["n_corr"].float().mean()), pose_ok=int((res["status"] == 0).sum()),
               t_err_max_m=float(np.nanmax(t_err)), reps=a.reps)
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
