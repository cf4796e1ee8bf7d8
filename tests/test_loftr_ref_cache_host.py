"""pipeline._RefCachedLoFTR's bookkeeping on the CPU, against a stub network: which images reach the backbone and in which order, which
(feature set, index) pairs reach the rest of the network, what the LRU keeps, the counters and the plain-path fallback.  Every image is a
constant plane whose value names it, and the stub's feature maps carry that value, so what match_features would read is checked by value --
whether it comes from the pool or from the batch's own backbone output."""
import torch

from mapfree_reloc_amd.nets.loftr import LoFTRFeatures
from mapfree_reloc_amd.pipeline import _RefCachedLoFTR


class _StubNet:
    def __init__(self):
        self.backbone_inputs, self.matched, self.plain_inputs = [], [], []

    def features(self, images):
        tags = images[:, 0, 0, 0].clone()
        self.backbone_inputs.append((tags.tolist(), tuple(images.shape[-2:])))
        n = len(tags)
        return LoFTRFeatures(tags.view(n, 1, 1, 1).expand(n, 2, 1, 1).contiguous(), (tags + 0.5).view(n, 1, 1, 1).expand(n, 4, 4, 3).contiguous())

    def match_features(self, src0, idx0, src1, idx1, H):
        side = lambda src, idx: ([float(src.coarse[i, 1, 0, 0]) for i in idx], [float(src.fine[i, 3, 3, 2]) - 0.5 for i in idx])
        c0, f0 = side(src0, idx0)
        c1, f1 = side(src1, idx1)
        assert c0 == f0 and c1 == f1                              # both maps of a side name the same image
        self.matched.append(dict(side0=c0, side1=c1, H=H, pooled=src0 is not src1))
        return "matched"

    def __call__(self, images):
        self.plain_inputs.append((images[:, 0, 0, 0].tolist(), tuple(images.shape[-2:])))
        return "plain"


def _batch(refs, queries, keys="auto", hw=(8, 8)):
    """pairs (reference tag, query tag); key of a pair = its reference tag unless given"""
    planes = [torch.full((1,) + hw, float(t)) for pair in zip(refs, queries) for t in pair]
    b = dict(images=torch.stack(planes))
    if keys == "auto":
        keys = [("scene", r) for r in refs]
    if keys is not None:
        b["ref_keys"] = keys
    return b


def test_groups_by_key_and_orders_new_references_before_queries():
    net = _StubNet()
    st = _RefCachedLoFTR(net, keep=4)
    assert st(_batch([100, 100, 200, 100], [1, 2, 3, 4])) == "matched"
    assert net.backbone_inputs == [([100.0, 200.0, 1.0, 2.0, 3.0, 4.0], (8, 8))]        # [new references | queries], first occurrence order
    assert net.matched == [dict(side0=[100.0, 100.0, 200.0, 100.0], side1=[1.0, 2.0, 3.0, 4.0], H=8, pooled=False)]
    assert st.stats == dict(reference_views_run=2, reference_views_reused=2)
    assert list(st.cache) == [("scene", 100), ("scene", 200)]
    # the next batch reuses one view across batches and meets a new one: only the new one and the queries are run
    st(_batch([200, 300, 300], [5, 6, 7]))
    assert net.backbone_inputs[1] == ([300.0, 5.0, 6.0, 7.0], (8, 8))
    assert net.matched[1] == dict(side0=[200.0, 300.0, 300.0], side1=[5.0, 6.0, 7.0], H=8, pooled=True)
    assert st.stats == dict(reference_views_run=3, reference_views_reused=4)
    assert list(st.cache) == [("scene", 100), ("scene", 200), ("scene", 300)]         # most recently used last
    assert len({v.slot for v in st.cache.values()}) == 3
    assert all(v.flag is None for v in st.cache.values())                            # no range guard bound: nothing to carry over
    assert net.plain_inputs == []


def test_none_keys_are_run_and_not_retained():
    net = _StubNet()
    st = _RefCachedLoFTR(net, keep=4)
    st(_batch([100, 100], [1, 2]))
    st(_batch([100, 7, 8], [3, 4, 5], keys=[("scene", 100), None, None]))
    assert net.backbone_inputs[1][0] == [7.0, 8.0, 3.0, 4.0, 5.0]
    assert net.matched[1]["side0"] == [100.0, 7.0, 8.0] and net.matched[1]["side1"] == [3.0, 4.0, 5.0]
    assert list(st.cache) == [("scene", 100)]
    assert st.stats == dict(reference_views_run=3, reference_views_reused=2)
    # the same unshared views again: run again (two None keys never stand for the same view, not even the same image)
    st(_batch([7, 7], [6, 7], keys=[None, None]))
    assert net.backbone_inputs[2][0] == [7.0, 7.0, 6.0, 7.0]
    assert net.matched[2] == dict(side0=[7.0, 7.0], side1=[6.0, 7.0], H=8, pooled=False)
    assert list(st.cache) == [("scene", 100)]
    assert st.stats == dict(reference_views_run=5, reference_views_reused=2)


def test_lru_evicts_at_keep_and_grows_for_a_wide_batch():
    net = _StubNet()
    st = _RefCachedLoFTR(net, keep=2)
    st(_batch([1], [10])); st(_batch([2], [10])); st(_batch([1], [10]))               # 1 is now the most recently used
    assert list(st.cache) == [("scene", 2), ("scene", 1)]
    st(_batch([3], [10]))                                                            # evicts 2, the least recently used
    assert list(st.cache) == [("scene", 1), ("scene", 3)]
    assert net.backbone_inputs[-1][0] == [3.0, 10.0]
    st(_batch([2, 1], [10, 11]))                                                     # 2 has to be run again; 1 is still there; 3 goes
    assert net.backbone_inputs[-1][0] == [2.0, 10.0, 11.0]
    assert net.matched[-1]["side0"] == [2.0, 1.0]
    assert list(st.cache) == [("scene", 2), ("scene", 1)]
    # a batch with more distinct views than `keep`: all of them are held for the batch (and until a later batch pushes them out)
    st(_batch([1, 5, 6, 7], [10, 11, 12, 13]))
    assert net.matched[-1]["side0"] == [1.0, 5.0, 6.0, 7.0] and net.matched[-1]["pooled"]
    assert len(st.cache) == 4 and len({v.slot for v in st.cache.values()}) == 4
    st(_batch([7], [10]))
    assert list(st.cache) == [("scene", 6), ("scene", 7)]
    assert net.matched[-1]["side0"] == [7.0]
    assert st.stats == dict(reference_views_run=7, reference_views_reused=4)


def test_pads_like_the_plain_path_and_drops_views_of_another_size():
    net = _StubNet()
    st = _RefCachedLoFTR(net, pad_to=8)
    st(_batch([1, 1], [10, 11], hw=(13, 6)))
    assert net.backbone_inputs == [([1.0, 10.0, 11.0], (16, 8))] and net.matched[0]["H"] == 16
    st(_batch([1], [12], hw=(8, 8)))                                                  # same key, other size: not reusable
    assert net.backbone_inputs[1] == ([1.0, 12.0], (8, 8))
    assert st.stats == dict(reference_views_run=2, reference_views_reused=1)


def test_plain_path_without_usable_keys():
    net = _StubNet()
    st = _RefCachedLoFTR(net)
    assert st(_batch([1, 1], [10, 11], keys=None, hw=(13, 6))) == "plain"
    assert st(_batch([1, 1], [10, 11], keys=[("scene", 1)])) == "plain"               # one key for two pairs
    assert net.plain_inputs == [([1.0, 10.0, 1.0, 11.0], (16, 8)), ([1.0, 10.0, 1.0, 11.0], (8, 8))]
    assert net.backbone_inputs == [] and net.matched == [] and len(st.cache) == 0
    assert st.stats == dict(reference_views_run=0, reference_views_reused=0)
