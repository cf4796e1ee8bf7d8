"""Benchmark metrics of the reference (lib/utils/metrics.py) in one place: pose_error_torch, error_auc and A_metrics are the regression
model's validation metrics (regression/losses.py, :6-67, :102-115); added here are what the relative-pose benchmark drivers need on top
(benchmark/scannet.py): MetricsAccumulator (:118-132), precision (:94-99), ecdf (:70-74) and the four-line AUC table (:77-91)."""
from collections import defaultdict

import numpy as np
import torch

from .regression.losses import A_metrics, error_auc, pose_error_torch  # noqa: F401  (re-exported)


def ecdf(x):
    """empirical cumulative distribution of the samples x [N]: (sorted values, cumulative share)"""
    return np.sort(x), np.linspace(0, 1, x.shape[0])


def auc_table(agg_metrics):
    """the four dictionaries of the AUC table: pose (max of rotation and translation angle), rotation and translation angle at 5 / 10 / 20
    degrees, translation distance at 0.1 / 0.5 / 1 m"""
    return {'pose': error_auc(np.maximum(agg_metrics['R_err'], agg_metrics['t_err_ang']), (5, 10, 20)),
            'rotation': error_auc(agg_metrics['R_err'], (5, 10, 20)),
            'translation_ang': error_auc(agg_metrics['t_err_ang'], (5, 10, 20)),
            'translation_euc': error_auc(agg_metrics['t_err_euc'], (0.1, 0.5, 1))}


def auc_table_lines(agg_metrics):
    t = auc_table(agg_metrics)
    fmt = '{0:.3f}/{1:.3f}/{2:.3f}'
    return ['Pose error AUC @ 5/10/20deg: ' + fmt.format(*t['pose'].values()),
            'Rotation error AUC @ 5/10/20deg: ' + fmt.format(*t['rotation'].values()),
            'Translation angular error AUC @ 5/10/20deg: ' + fmt.format(*t['translation_ang'].values()),
            'Translation Euclidean error AUC @ 0.1/0.5/1m: ' + fmt.format(*t['translation_euc'].values())]


def print_auc_table(agg_metrics):
    for line in auc_table_lines(agg_metrics):
        print(line)


def precision(agg_metrics, rot_threshold, trans_threshold):
    """share of samples with rotation error <= rot_threshold AND Euclidean translation error <= trans_threshold (NaN: a miss)"""
    return (np.asarray(agg_metrics['R_err'] <= rot_threshold) * np.asarray(agg_metrics['t_err_euc'] <= trans_threshold)).mean()


class MetricsAccumulator:
    """collects the per-batch metric dictionaries; aggregate() -> one flat numpy array per key"""

    def __init__(self):
        self.data = defaultdict(list)

    def accumulate(self, data):
        for key, value in data.items():
            self.data[key].append(value)

    def aggregate(self):
        return {key: torch.cat(vals).view(-1).cpu().numpy() for key, vals in self.data.items()}
