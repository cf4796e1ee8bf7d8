"""The Python that the matcher surfaces share, on CPU tensors (no GPU, no library): the per-pair plugins' result tail
(matching/feature_matching._OnlineMatching), the offline tools' tail (matchers.first_pair_rows) and the bookkeeping of nets/graph.GraphOrEager."""
import warnings

import numpy as np
import pytest
import torch

from mapfree_reloc_amd import matchers, options
from mapfree_reloc_amd.matching import feature_matching as FM
from mapfree_reloc_amd.nets import graph as G


def _match(n, K=5):
    """a batched match dict of two pairs; the first pair has n correspondences"""
    g = torch.Generator().manual_seed(n)
    return dict(n_corr=torch.tensor([n, 2], dtype=torch.int32), pts0=torch.rand(2, K, 2, generator=g) * 100, pts1=torch.rand(2, K, 2, generator=g) * 100)


# ------------------------------------------------------------------------------------------------ the plugin tail
class _Twin:
    def __init__(self):
        self.calls = []

    def get_correspondences(self, data):
        self.calls.append((data, options.get("SPLIT")))
        return "from the twin"


class _Guard:
    def __init__(self, flag):
        self.flag, self.reruns, self._twin = torch.tensor([flag], dtype=torch.int32), 0, _Twin()

    def twin(self):
        return self._twin


def _plugin(flag):
    p = FM._OnlineMatching.__new__(FM._OnlineMatching)               # the tail reads the guard alone
    p.guard = _Guard(flag)
    return p


@pytest.mark.parametrize("n", [1, 3, 5])
def test_plugin_tail_unpacks_the_first_n_rows_as_writable_float32_copies(n):
    p, out = _plugin(0), _match(n)
    packed = p._pack(out)
    assert packed.dtype == torch.float32 and packed.shape == (2 + 4 * 5,) and packed[0] == n and packed[1] == 0
    pts0, pts1 = p._unpack({}, packed)
    for got, want in ((pts0, out["pts0"]), (pts1, out["pts1"])):
        assert got.dtype == np.float32 and got.shape == (n, 2) and np.array_equal(got, want[0, :n].numpy())
        assert got.flags.writeable and got.base is None                # a copy, not a view of the packed buffer
    assert p.guard.reruns == 0 and p.guard.twin().calls == []


def test_plugin_tail_without_correspondences_gives_two_empty_arrays():
    p = _plugin(0)
    pts0, pts1 = p._unpack({}, p._pack(_match(0)))
    assert pts0.shape == (0,) and pts1.shape == (0,)
    assert p.guard.reruns == 0


def test_plugin_tail_hands_a_flagged_pair_to_the_twin_once():
    p, data = _plugin(1), {"pair_id": 7}
    assert p._unpack(data, p._pack(_match(3))) == "from the twin"
    assert p.guard.reruns == 1 and len(p.guard.twin().calls) == 1
    assert p.guard.twin().calls[0][0] is data and p.guard.twin().calls[0][1] == "bf16x3"


# ------------------------------------------------------------------------------------------------ the offline tail
def test_offline_tail_rows_and_the_nan_row(capsys):
    out = _match(4)
    rows = matchers.first_pair_rows(out)
    assert rows.shape == (4, 4) and np.array_equal(rows, torch.cat([out["pts0"][0, :4], out["pts1"][0, :4]], 1).numpy())
    assert capsys.readouterr().out == ""
    none = matchers.first_pair_rows(_match(0))
    assert none.shape == (1, 4) and none.dtype == np.float64 and np.isnan(none).all()
    assert capsys.readouterr().out == "no correspondences\n"


# ------------------------------------------------------------------------------------------------ graph or eager
class _StubGraphedCall:
    built, fail = [], False

    def __init__(self, fn, example_inputs, clone_outputs=False):
        if _StubGraphedCall.fail:
            raise G.GraphCaptureError("HIP-graph capture failed (stub)")
        self.fn = fn
        _StubGraphedCall.built.append((list(example_inputs), clone_outputs))

    def __call__(self, *inputs):
        return ("replay", self.fn(*inputs))


@pytest.fixture
def stub(monkeypatch):
    monkeypatch.setattr(G, "GraphedCall", _StubGraphedCall)
    _StubGraphedCall.built, _StubGraphedCall.fail = [], False
    return _StubGraphedCall


def test_graph_or_eager_captures_once_per_key(stub):
    run = G.GraphOrEager(lambda a, b: a + b, "test", clone_outputs=True)
    assert run("k1", 1, 2) == ("replay", 3) and run("k1", 3, 4) == ("replay", 7)
    assert stub.built == [([1, 2], True)]                           # captured on the first call's inputs
    assert run("k2", 5, 6) == ("replay", 11)
    assert len(stub.built) == 2 and sorted(run.graphs) == ["k1", "k2"]


def test_graph_or_eager_runs_a_key_beyond_the_cap_eagerly(stub):
    run = G.GraphOrEager(lambda a: a * 2, "test", max_keys=2)
    assert [run(k, 1) for k in ("a", "b", "c", "a", "c")] == [("replay", 2), ("replay", 2), 2, ("replay", 2), 2]
    assert len(stub.built) == 2 and sorted(run.graphs) == ["a", "b"]


def test_graph_or_eager_switched_off_never_captures(stub):
    run = G.GraphOrEager(lambda a: a * 2, "test", enabled=False)
    assert run("a", 1) == 2 and stub.built == [] and run.graphs == {}


def test_graph_or_eager_after_a_failed_capture_every_call_is_eager(stub):
    run = G.GraphOrEager(lambda a: a * 2, "test")
    assert run("a", 1) == ("replay", 2)
    stub.fail = True
    with pytest.warns(UserWarning, match="test: HIP-graph capture failed .*running eagerly from now on"):
        assert run("b", 2) == 4
    stub.fail = False
    with warnings.catch_warnings():
        warnings.simplefilter("error")                              # warned once
        assert run("a", 3) == 6 and run("b", 3) == 6 and run("c", 3) == 6           # the key captured before the failure too
    assert not run.enabled and len(stub.built) == 1
