"""compute.py -ds Scannet with a stub matcher: argument handling, pair order (the rows of `name`, as load_scannet_imgpaths) and the
single output file; -ds Mapfree keeps its arguments."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scannet_tree as ST  # noqa: E402

from mapfree_reloc_amd import compute, wire  # noqa: E402


class _Stub:
    made = []

    def __init__(self, resize, outdoor=False, **kw):
        self.resize, self.outdoor, self.kw, self.pairs = resize, outdoor, kw, []
        _Stub.made.append(self)

    def match(self, pair):
        k = len(self.pairs)
        self.pairs.append(pair)
        return np.full((1, 4), np.nan) if k == 1 else np.arange(4.0 * (k + 2)).reshape(k + 2, 4) + k


@pytest.fixture()
def stub(monkeypatch):
    _Stub.made = []
    for name in ("SG", "LoFTR", "SIFT"):
        monkeypatch.setitem(compute.MATCHERS, name, _Stub)
    return _Stub


def test_scannet_stage(tmp_path, stub):
    p = ST.default_params()
    tr = ST.write_tree(tmp_path / "tree", p)
    out_dir = tmp_path / "out" / "misc"
    compute.main(["-ds", "Scannet", "-m", "SG", "--pair_npz", tr["test_npz"], "--data_root", tr["scans"], "--output_dir", str(out_dir)])
    m, = stub.made
    assert m.resize == (640, 480) and m.outdoor is False
    want = [tuple(os.path.join(tr["scans"], f"scene{s:04d}_{u:02d}", "sensor_data", f"frame-{st:06}.color.jpg") for st in (a, b))
            for s, u, a, b in p["names"].tolist()]
    assert m.pairs == want
    assert os.listdir(out_dir) == ["correspondences_SG_scannet_test.npz"]
    corr = np.load(out_dir / "correspondences_SG_scannet_test.npz")["correspondences"]
    assert corr.shape == (5, 6, 4) and corr.dtype == np.float64
    assert np.isnan(corr[1]).all() and np.array_equal(corr[4], np.arange(24.0).reshape(6, 4) + 4)
    p1, p2 = wire.strip_nan(corr[0].astype(np.float32))
    assert p1.shape == (2, 2) and np.array_equal(np.concatenate([p1, p2], 1), np.arange(8.0).reshape(2, 4))


def test_scannet_stage_matcher_options(tmp_path, stub):
    tr = ST.write_tree(tmp_path / "tree", ST.default_params())
    compute.main(["-ds", "Scannet", "-m", "SIFT", "--sift-detector", "hip", "--pair_npz", tr["test_npz"], "--data_root", tr["scans"],
                  "--output_dir", str(tmp_path)])
    compute.main(["-ds", "Scannet", "-m", "LoFTR", "--loftr-match-type", "sinkhorn", "--pair_npz", tr["test_npz"], "--data_root", tr["scans"],
                  "--output_dir", str(tmp_path)])
    assert stub.made[0].kw == {"detector": "hip"} and stub.made[1].kw == {"match_type": "sinkhorn"}
    assert all(m.resize == (640, 480) and len(m.pairs) == 5 for m in stub.made)
    assert (tmp_path / "correspondences_SIFT_scannet_test.npz").exists() and (tmp_path / "correspondences_LoFTR_OT_scannet_test.npz").exists()


def test_dataset_choices(tmp_path, stub):
    with pytest.raises(SystemExit):
        compute.main(["-ds", "7Scenes", "-m", "SG"])
    compute.main(["-ds", "Mapfree", "-m", "SG", "--data_root", str(tmp_path)])           # an empty tree: nothing to do, Map-free's size
    assert stub.made[-1].resize == (540, 720) and stub.made[-1].pairs == []
