"""The 7Scenes reader (mapfree_reloc_amd/sevenscenes.py) against what the reference's own SceneDataset made of the same tiny tree
(tests/golden/ref_sevenscenes.npz part (a), written by tools/gen_sevenscenes_golden.py; the tree is rebuilt here from the parameters the
fixture stores), and the data-source dispatch of list_scenes.  The fixture was computed with the same numpy / scipy / torch, so equality
is exact."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sevenscenes_tree as ST  # noqa: E402

from mapfree_reloc_amd import datasets as D  # noqa: E402
from mapfree_reloc_amd.config import get_cfg_defaults  # noqa: E402
from mapfree_reloc_amd.sevenscenes import SevenScenesScene, one_nn_rows  # noqa: E402


@pytest.fixture(scope="module")
def ref(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "ref_sevenscenes.npz")))


@pytest.fixture(scope="module")
def tree(ref, tmp_path_factory):
    p = {k[5:]: v for k, v in ref.items() if k.startswith("tree_")}
    return p, ST.write_tree(tmp_path_factory.mktemp("sevenscenes"), p)


def _cfg(root, p, one_nn=False, est=None, scenes=None):
    cfg = get_cfg_defaults()
    cfg.DATASET.DATA_SOURCE, cfg.DATASET.DATA_ROOT, cfg.DATASET.SCENES = "7Scenes", root, scenes
    cfg.DATASET.PAIRS_TXT.TEST, cfg.DATASET.PAIRS_TXT.ONE_NN = ST.PAIR_TXT, one_nn
    cfg.DATASET.WIDTH, cfg.DATASET.HEIGHT, cfg.DATASET.ESTIMATED_DEPTH = int(p["width"]), int(p["height"]), est
    return cfg


@pytest.mark.parametrize("tag,one_nn", [("all", False), ("nn", True)])
def test_samples_equal_the_reference(ref, tree, tag, one_nn):
    p, root = tree
    scenes = D.list_scenes(_cfg(root, p, one_nn), "test")
    assert [sc.scene_id for sc in scenes] == ["chess", "fire"] and all(isinstance(sc, SevenScenesScene) for sc in scenes)   # SCENES None: glob, sorted
    for s, sc in enumerate(scenes):
        pre = f"rd{s}_{tag}_"
        assert len(sc) == len(ref[pre + "pair_id"]) and sc.scene_root == os.path.join(root, sc.scene_id)
        for i in range(len(sc)):
            x = sc[i]
            assert set(x) == {"image0", "image1", "depth0", "depth1", "T_0to1", "abs_q_0", "abs_c_0", "abs_q_1", "abs_c_1", "sim", "K_color0",
                              "K_color1", "K_depth", "dataset_name", "scene_id", "scene_root", "pair_id", "pair_names"}
            assert list(x["pair_names"]) == ref[pre + "pair_names"][i].tolist() and isinstance(x["pair_names"], tuple)
            assert x["pair_id"] == int(ref[pre + "pair_id"][i]) and x["sim"] == float(ref[pre + "sim"][i])
            assert x["dataset_name"] == "7Scenes" == str(ref[pre + "dataset_name"][i]) and x["scene_id"] == str(ref[pre + "scene_id"][i])
            assert x["scene_root"] == sc.scene_root
            assert x["T_0to1"].dtype == torch.float32 and np.array_equal(x["T_0to1"].numpy(), ref[pre + "T_0to1"][i])
            for k in ("abs_q_0", "abs_c_0", "abs_q_1", "abs_c_1"):
                assert x[k].dtype == np.float32 and np.array_equal(x[k], ref[pre + k][i]), k
            for k in ("K_color0", "K_color1", "K_depth"):
                assert x[k].dtype == ref[pre + k].dtype and np.array_equal(x[k], ref[pre + k][i]), k
            for k in ("depth0", "depth1"):                    # the files' own 7 x 5, not WIDTH x HEIGHT
                assert x[k].dtype == torch.float32 and x[k].shape == (5, 7) and np.array_equal(x[k].numpy(), ref[pre + k][i]), k
            assert x["image0"].shape == (3, int(p["height"]), int(p["width"])) and x["image0"].dtype == torch.float32
    if one_nn:
        # scene 0: query 6 returns in the last row (6) with a similarity that ties its best: that row is kept and query 6 still comes first;
        # query 7's tie 0.9 / 0.9 keeps the LATER row.  pair_id is the row of the pair file
        assert ref["rd0_nn_pair_id"].tolist() == [6, 4] and ref["rd1_nn_pair_id"].tolist() == [2, 4]


def test_estimated_depth_suffix(ref, tree):
    p, root = tree
    for s, sc in enumerate(D.list_scenes(_cfg(root, p, est="est", scenes=["chess", "fire"]), "test")):
        d0 = np.stack([sc[i]["depth0"].numpy() for i in range(len(sc))])
        assert np.array_equal(d0, ref[f"rd{s}_est_depth0"]) and not np.array_equal(d0, ref[f"rd{s}_all_depth0"])
        assert np.array_equal(np.stack([sc[i]["depth1"].numpy() for i in range(len(sc))]), ref[f"rd{s}_est_depth1"])


def test_one_nn_rows_rules():
    pairs = [("a", "q1"), ("b", "q2"), ("c", "q1"), ("d", "q2"), ("e", "q1")]
    assert one_nn_rows(pairs, [0.5, 0.7, 0.5, 0.6, 0.4]) == [2, 1]          # equal replaces, lower does not; first-appearance order


def test_loader_and_missing_root(tree, tmp_path):
    p, root = tree
    batches = list(D.make_loader(_cfg(root, p), "test"))
    assert len(batches) == 13 and batches[0]["pair_names"] == [["seq-01/frame-000000.color.png"], ["seq-02/frame-000006.color.png"]]
    assert batches[0]["T_0to1"].shape == (1, 4, 4) and batches[0]["scene_id"] == ["chess"] and int(batches[6]["pair_id"]) == 6
    with pytest.raises(D.MissingDataError):
        D.list_scenes(_cfg(str(tmp_path / "nope"), p), "test")
