"""ScanNet-1500 relative-pose benchmark (benchmark/scannet.py:15-57).

    python -m mapfree_reloc_amd.scannet_benchmark <config> [--dataset_config config/scannet.yaml] [--checkpoint CKPT]
                                                  [--fused] [--batch_pairs N] [--output_root results]

Default: the reference's loop, one pair at a time through the model plugin (build_model(cfg)(data)).  --fused: the batched route,
PairBatchLoader -> DevicePrefetcher -> FusedPosePipeline; a batch's ground truth is looked up by its `global_ids`.  A pair without a pose is a NaN
row of every metric (counted by the failure share, a miss in AUC and recall).  Both modes print the same lines and save the aggregated
arrays as <output_root>/scannet/<config name>.npz (the printed lines beside them as .txt).
"""
import argparse
import os
from pathlib import Path

import numpy as np
import torch

from .metrics import A_metrics, MetricsAccumulator, auc_table_lines, pose_error_torch, precision

THRESHOLDS = ((0.1, 5), (0.25, 5), (0.5, 10), (1, 20))      # (metres, degrees)


def report_lines(agg):
    """the benchmark's printed lines (scannet.py:38-54) from the aggregated arrays"""
    lines = [f"Median Rotation error [deg]: {np.nanmedian(agg['R_err']):.2f}",
             f"Median Translation angular error [deg]: {np.nanmedian(agg['t_err_ang']):.2f}",
             f"Median Translation Euclidean error [m]: {np.nanmedian(agg['t_err_euc']):.2f}"]
    lines += auc_table_lines(agg)
    lines.append("Recall @ " + "/".join(f"({t[0]:.1f}m,{t[1]:.0f}deg)" for t in THRESHOLDS) + ': ' +
                 "/".join('{:.2f}'.format(precision(agg, t[1], t[0])) for t in THRESHOLDS))
    a1, a2, a3 = A_metrics(agg['t_err_scale_sym'])
    lines.append(f"t_scale_error A1/A2/A3 [%]: {a1*100:.1f}/{a2*100:.1f}/{a3*100:.1f}")
    lines.append(f"failures (not enough corr.) [%]: {np.isnan(agg['R_err']).mean()*100:.1f}")
    return lines


def run_per_pair(cfg, checkpoint='', hook=None):
    """scannet.py:20-35: the batch-1 loop over the test pairs.  hook(data, R, t) sees every pair's estimate (tests)"""
    from .builder import build_model
    from .datasets import make_loader
    from .submission import data_to_model_device
    model = build_model(cfg, checkpoint)
    macc = MetricsAccumulator()
    for data in make_loader(cfg, 'test'):
        data = data_to_model_device(data, model)
        with torch.no_grad():
            R, t = model(data)
        if hook is not None:
            hook(data, R, t)
        macc.accumulate(pose_error_torch(R, t, data['T_0to1']))
    return macc.aggregate()


def run_fused(cfg, batch_pairs=None, pipeline=None, hook=None):
    """the same pairs in batches on the device.  The pipeline's float64 poses are rounded to float32 (what the plugin returns) and scored
    one pair at a time, so a pair's metrics do not depend on the batch it travelled in.  hook(device batch, pipeline output): tests."""
    from . import options
    from .datasets import DevicePrefetcher, PairBatchLoader, list_scenes, usable_cpus
    options.apply_cfg(cfg)
    scenes = list_scenes(cfg, 'test')
    if pipeline is None:
        from .pipeline import FusedPosePipeline
        pipeline = FusedPosePipeline(cfg, torch.device('cuda', torch.cuda.current_device()))
    device = torch.device(pipeline.device)
    where = [(sc, i) for sc in scenes for i in range(len(sc))]             # global id -> (dataset, index)
    workers = int(cfg.HIP.LOADER_WORKERS) if int(cfg.HIP.LOADER_WORKERS) > 0 else max(2, min(32, usable_cpus()))
    loader = PairBatchLoader(scenes, int(batch_pairs or cfg.HIP.BATCH_PAIRS), pin=device.type == 'cuda', workers=workers,
                             decode=str(cfg.HIP.LOADER_DECODE), jpeg_decode=str(cfg.HIP.JPEG_DECODE),
                             depth_decode=str(cfg.HIP.DEPTH_DECODE))   # (this reader's depth maps stay on the host route)
    rows = {}
    try:
        for batch in DevicePrefetcher(loader, device):
            out = pipeline(batch)
            if hook is not None:
                hook(batch, out)
            R, t = out['R'].to(torch.float32).cpu(), out['t'].to(torch.float32).cpu()
            for p, gid in enumerate(batch['global_ids'].tolist()):
                sc, i = where[gid]
                T = torch.tensor(sc.rel_pose(*sc._row(i)), dtype=torch.float32)[None]
                rows[gid] = pose_error_torch(R[p][None], t[p].reshape(1, 1, 3), T)
    finally:
        loader.close()
    macc = MetricsAccumulator()
    for gid in sorted(rows):
        macc.accumulate(rows[gid])
    return macc.aggregate()


def run(cfg, config_name, checkpoint='', fused=False, batch_pairs=None, output_root='results', pipeline=None, hook=None):
    agg = run_fused(cfg, batch_pairs, pipeline, hook) if fused else run_per_pair(cfg, checkpoint, hook)
    lines = report_lines(agg)
    for line in lines:
        print(line)
    out_dir = Path(output_root) / 'scannet'
    out_dir.mkdir(parents=True, exist_ok=True)
    (out_dir / f'{config_name}.txt').write_text('\n'.join(lines) + '\n')
    np.savez(out_dir / config_name, **agg)
    return lines, agg


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('config', help='path to config file')
    ap.add_argument('--dataset_config', default=None, help='dataset yaml merged first (the reference hard-codes config/scannet.yaml)')
    ap.add_argument('--checkpoint', help='path to checkpoint', default='')
    ap.add_argument('--fused', action='store_true', help='batched GPU route (PairBatchLoader -> FusedPosePipeline)')
    ap.add_argument('--batch_pairs', type=int, default=None)
    ap.add_argument('--output_root', type=Path, default=Path('results'))
    args = ap.parse_args(argv)
    from .config import get_cfg_defaults
    cfg = get_cfg_defaults()
    cfg.DATASET.DATA_SOURCE = 'ScanNet'
    if args.dataset_config:
        cfg.merge_from_file(args.dataset_config)
    cfg.merge_from_file(args.config)
    return run(cfg, os.path.basename(args.config)[:-5], args.checkpoint, args.fused, args.batch_pairs, args.output_root)


if __name__ == '__main__':
    main()
