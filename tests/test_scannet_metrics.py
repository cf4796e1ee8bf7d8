"""Benchmark metrics (mapfree_reloc_amd/metrics.py, scannet_benchmark.report_lines) against the reference's lib/utils/metrics.py run on
200 seeded poses (tests/golden/ref_scannet.npz, tools/gen_scannet_golden.py).  pose_error_torch through MetricsAccumulator is the same
torch arithmetic on the same machine class: exact.  AUC / precision / A1-A3 from the stored error arrays: 1e-12 absolute (values in [0, 1];
a float64 trapezoid sum of <= 1500 terms rounds by less than 2e-13)."""
import os

import numpy as np
import pytest
import torch

from mapfree_reloc_amd import metrics as M
from mapfree_reloc_amd.scannet_benchmark import THRESHOLDS, report_lines

KEYS = ("t_err_ang", "t_err_scale", "t_err_scale_sym", "t_err_euc", "R_err")


@pytest.fixture(scope="module")
def ref(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "ref_scannet.npz")))


def test_pose_errors_through_the_accumulator_are_exact(ref):
    R, t, T = (torch.from_numpy(ref[k]) for k in ("pose_R", "pose_t", "pose_T"))
    macc = M.MetricsAccumulator()
    for i in range(len(R)):
        macc.accumulate(M.pose_error_torch(R[i:i + 1], t[i:i + 1], T[i:i + 1]))
    agg = macc.aggregate()
    assert set(agg) == set(KEYS)
    assert int(np.isnan(ref["agg_R_err"]).sum()) == 12
    for k in KEYS:
        assert agg[k].dtype == ref["agg_" + k].dtype and agg[k].shape == (200,)
        assert np.array_equal(agg[k], ref["agg_" + k], equal_nan=True), k


def test_auc_precision_and_a_metrics(ref):
    agg = {k: ref["agg_" + k] for k in KEYS}
    table = M.auc_table(agg)
    for name in ("pose", "rotation", "translation_ang", "translation_euc"):
        got = np.array(list(table[name].values()), np.float64)
        assert np.all((got >= 0) & (got <= 1)) and np.abs(got - ref["auc_" + name]).max() <= 1e-12, name
    assert list(table["translation_euc"]) == ["auc@0.1", "auc@0.5", "auc@1"]
    prec = np.array([M.precision(agg, deg, m) for m, deg in THRESHOLDS], np.float64)
    assert np.abs(prec - ref["precision"]).max() <= 1e-12 and 0 < prec[0] < prec[-1] < 1
    a = np.array([float(v) for v in M.A_metrics(agg["t_err_scale_sym"])], np.float64)
    assert np.abs(a - ref["A_metrics"]).max() <= 1e-12
    v, cd = M.ecdf(agg["t_err_euc"])
    assert cd[0] == 0 and cd[-1] == 1 and np.all(np.diff(v[~np.isnan(v)]) >= 0) and len(v) == len(cd) == 200


def test_report_lines(ref, capsys):
    agg = {k: ref["agg_" + k] for k in KEYS}
    lines = report_lines(agg)
    assert len(lines) == 10
    assert lines[0] == f"Median Rotation error [deg]: {np.nanmedian(agg['R_err']):.2f}" and "nan" not in lines[0]
    assert lines[3].startswith("Pose error AUC @ 5/10/20deg: ") and lines[6].startswith("Translation Euclidean error AUC @ 0.1/0.5/1m: ")
    assert lines[3].endswith("{0:.3f}/{1:.3f}/{2:.3f}".format(*ref["auc_pose"]))
    assert lines[7] == "Recall @ (0.1m,5deg)/(0.2m,5deg)/(0.5m,10deg)/(1.0m,20deg): " + "/".join(f"{v:.2f}" for v in ref["precision"])
    assert lines[8] == "t_scale_error A1/A2/A3 [%]: " + "/".join(f"{v * 100:.1f}" for v in ref["A_metrics"])
    assert lines[9] == "failures (not enough corr.) [%]: 6.0"
    M.print_auc_table(agg)
    assert capsys.readouterr().out.splitlines() == lines[3:7]
