"""ref_cache.RefViewCache on its own, and pipeline._RefCachedKeypointMatcher's bookkeeping on the CPU against a stub SuperPoint and a stub matcher (the
style of tests/test_loftr_ref_cache_host.py: every image is a constant plane whose value names it, and the stub's rows carry that value)."""
import torch

from mapfree_reloc_amd.pipeline import _RefCachedKeypointMatcher
from mapfree_reloc_amd.ref_cache import RefViewCache


class _Guard:
    """stands in for pipeline.RangeGuard: what the cache reads of it"""

    def __init__(self, active=True):
        self.active, self.flag = active, torch.zeros(1, dtype=torch.int32)


def _run(cache, ref_keys, cap, retain_solo):
    """one batch as a stage drives the cache; cap: a function of the number of distinct views"""
    plan = cache.plan(ref_keys)
    flag = cache.take_flag()
    for k in plan.need:
        if retain_solo or k not in plan.solo:
            cache.put(k, flag, tag=k)
    cache.carry(plan)
    cache.settle(plan, cap(len(plan.first)))
    return plan


# ------------------------------------------------------------------------------------------------ the shared class
def test_key_plan_groups_in_first_occurrence_order_and_none_keys_are_distinct():
    c = RefViewCache()
    plan = c.plan(["b", None, "a", "b", None])
    assert len(plan.keys) == 5 and plan.keys[0] == plan.keys[3] == "b" and plan.keys[2] == "a"
    assert plan.keys[1] != plan.keys[4] and plan.solo == {plan.keys[1], plan.keys[4]}
    assert list(plan.first) == ["b", plan.keys[1], "a", plan.keys[4]]                # first occurrence order
    assert plan.first == {"b": 0, plan.keys[1]: 1, "a": 2, plan.keys[4]: 4}
    assert plan.pairs_of["b"] == [0, 3] and plan.pairs_of["a"] == [2] and plan.pairs_of[plan.keys[4]] == [4]
    assert plan.need == list(plan.first) and plan.reused == []
    c.put("a", None, tag="a")
    plan = c.plan(["b", "a", None])
    assert plan.need == ["b", plan.keys[2]] and plan.reused == ["a"]


def test_none_keys_are_never_retained_whether_the_stage_stored_them_or_not():
    for retain in (True, False):
        c = RefViewCache()
        _run(c, ["a", None, None], lambda d: max(4, d), retain)
        assert list(c) == ["a"]
        plan = _run(c, [None, None], lambda d: max(4, d), retain)                    # the same unshared pairs again: new again
        assert len(plan.need) == 2 and plan.reused == [] and list(c) == ["a"]


def test_settle_with_the_matcher_stages_cap_evicts_at_keep_and_grows_for_a_wide_batch():
    """the sequences of tests/test_loftr_ref_cache_host.py::test_lru_evicts_at_keep_and_grows_for_a_wide_batch, cap = max(keep, distinct views)"""
    c, cap = RefViewCache(), lambda d: max(2, d)
    for keys in ([1], [2], [1]):
        _run(c, keys, cap, True)
    assert list(c) == [2, 1]                                                         # 1 is the most recently used
    assert _run(c, [3], cap, True).need == [3] and list(c) == [1, 3]                 # evicts 2, the least recently used
    plan = _run(c, [2, 1], cap, True)
    assert plan.need == [2] and plan.reused == [1] and list(c) == [2, 1]             # 2 is new again; 1 is still there; 3 goes
    plan = _run(c, [1, 5, 6, 7], cap, True)
    assert plan.reused == [1] and list(c) == [1, 5, 6, 7]                            # more distinct views than keep: all held
    _run(c, [7], cap, True)
    assert list(c) == [6, 7]


def test_settle_with_the_depth_stages_cap_is_plain_keep():
    c, cap = RefViewCache(), lambda d: 2
    for keys in ([1], [2], [1], [3]):
        _run(c, keys, cap, False)
    assert list(c) == [1, 3]
    plan = _run(c, [1, 5, 6, 7, None], cap, False)                                   # a wide batch is not held beyond keep
    assert plan.reused == [1] and plan.need[:3] == [5, 6, 7] and list(c) == [6, 7]
    assert _run(c, [1, 7], cap, False).need == [1] and list(c) == [1, 7]


def test_flag_of_a_stored_entry_is_carried_into_the_batches_that_reuse_it():
    g = _Guard()
    c = RefViewCache(g)
    _run(c, ["a", "a"], lambda d: 4, True)
    e = c["a"]
    assert e.flag is not g.flag and e.flag.shape == (1,) and e.flag.dtype == torch.int32 and int(e.flag) == 0 and e.tag == "a"
    e.flag.fill_(1)
    g.flag.zero_()
    _run(c, ["b", "a"], lambda d: 4, True)                                           # reuses the flagged entry
    assert int(g.flag) == 1
    assert int(c["a"].flag) == 1 and c["b"].flag is not c["a"].flag
    g.flag.zero_()
    _run(c, ["b", None], lambda d: 4, True)                                          # does not
    assert int(g.flag) == 0


def test_inactive_or_absent_guard_stores_no_flag_and_carries_nothing():
    for g in (_Guard(active=False), None):
        c = RefViewCache(g)
        _run(c, ["a"], lambda d: 4, True)
        assert c["a"].flag is None and c.take_flag() is None
        _run(c, ["a", "b"], lambda d: 4, True)
        assert c["b"].flag is None and (g is None or int(g.flag) == 0)


# ------------------------------------------------------------------------------------------------ the SuperPoint + matcher stage
K = 3


class _StubSuperPoint:
    def __init__(self):
        self.inputs = []

    def __call__(self, images):
        tags = images[:, 0, 0, 0].clone()
        self.inputs.append(tags.tolist())
        n = len(tags)
        return dict(kpts=tags.view(n, 1, 1).expand(n, K, 2).contiguous(), scores=(tags + 0.25).view(n, 1).expand(n, K).contiguous(),
                    desc=(tags + 0.5).view(n, 1, 1).expand(n, K, 4).contiguous(), n=tags.to(torch.int32))


class _StubMatcher:
    def __init__(self):
        self.rows = []

    def __call__(self, sp, hw, maxN=None):
        tags = sp["kpts"][:, K - 1, 1]
        assert torch.equal(sp["scores"][:, 0] - 0.25, tags) and torch.equal(sp["desc"][:, 0, 3] - 0.5, tags) and torch.equal(sp["n"], tags.to(torch.int32))
        self.rows.append((tags.tolist(), hw, maxN))
        return "matched"


def _batch(refs, queries, keys="auto", hw=(8, 6)):
    planes = [torch.full((1,) + hw, float(t)) for pair in zip(refs, queries) for t in pair]
    b = dict(images=torch.stack(planes))
    if keys == "auto":
        keys = [("scene", r) for r in refs]
    if keys is not None:
        b["ref_keys"] = keys
    return b


def _stage(guard=None, keep=4):
    sp, net, plain = _StubSuperPoint(), _StubMatcher(), []
    st = _RefCachedKeypointMatcher(sp, net, 77, lambda im: plain.append(im[:, 0, 0, 0].tolist()) or "plain", guard, keep=keep)
    return st, sp, net, plain


def test_keypoint_stage_runs_new_references_then_queries_and_hands_the_matcher_interleaved_rows():
    st, sp, net, plain = _stage()
    assert st(_batch([100, 100, 200, 100], [1, 2, 3, 4])) == "matched"
    assert sp.inputs == [[100.0, 200.0, 1.0, 2.0, 3.0, 4.0]]                           # [new references | queries], first occurrence order
    assert net.rows == [([100.0, 1.0, 100.0, 2.0, 200.0, 3.0, 100.0, 4.0], (8, 6), 77)]      # (reference, query) per pair
    assert st.stats == dict(reference_views_run=2, reference_views_reused=2)
    st(_batch([200, 300, 300], [5, 6, 7]))                                           # one view from the cache, one new
    assert sp.inputs[1] == [300.0, 5.0, 6.0, 7.0]
    assert net.rows[1][0] == [200.0, 5.0, 300.0, 6.0, 300.0, 7.0]
    assert st.stats == dict(reference_views_run=3, reference_views_reused=4)
    assert list(st.cache) == [("scene", 100), ("scene", 200), ("scene", 300)]          # most recently used last
    assert all(v.flag is None for v in st.cache.values())                             # no range guard bound
    st(_batch([300], [8]))                                                            # nothing new: the queries alone
    assert sp.inputs[2] == [8.0] and net.rows[2][0] == [300.0, 8.0]
    assert plain == []


def test_keypoint_stage_none_keys_are_run_and_not_retained():
    st, sp, net, _ = _stage()
    st(_batch([100, 7, 7], [3, 4, 5], keys=[("scene", 100), None, None]))
    assert sp.inputs == [[100.0, 7.0, 7.0, 3.0, 4.0, 5.0]] and net.rows[0][0] == [100.0, 3.0, 7.0, 4.0, 7.0, 5.0]
    assert list(st.cache) == [("scene", 100)]
    assert st.stats == dict(reference_views_run=3, reference_views_reused=0)


def test_keypoint_stage_lru():
    st, sp, net, _ = _stage(keep=2)
    for r in (1, 2, 1):
        st(_batch([r], [10]))
    assert list(st.cache) == [("scene", 2), ("scene", 1)]
    st(_batch([3], [10]))
    assert list(st.cache) == [("scene", 1), ("scene", 3)]
    st(_batch([2, 1], [10, 11]))
    assert sp.inputs[-1] == [2.0, 10.0, 11.0] and net.rows[-1][0] == [2.0, 10.0, 1.0, 11.0]
    assert list(st.cache) == [("scene", 2), ("scene", 1)]
    st(_batch([1, 5, 6, 7], [10, 11, 12, 13]))
    assert len(st.cache) == 4
    st(_batch([7], [10]))
    assert list(st.cache) == [("scene", 6), ("scene", 7)]
    assert st.stats == dict(reference_views_run=7, reference_views_reused=4)


def test_keypoint_stage_plain_path_without_usable_keys():
    st, sp, net, plain = _stage()
    assert st(_batch([1, 1], [10, 11], keys=None)) == "plain"
    assert st(_batch([1, 1], [10, 11], keys=[("scene", 1)])) == "plain"                # one key for two pairs
    assert plain == [[1.0, 10.0, 1.0, 11.0]] * 2 and sp.inputs == [] and net.rows == [] and len(st.cache) == 0
    assert st.stats == dict(reference_views_run=0, reference_views_reused=0)


def test_keypoint_stage_flagged_cached_view_marks_a_later_batch():
    g = _Guard()
    st, _, _, _ = _stage(g)
    st(_batch([1, 1], [10, 11]))
    view = st.cache[("scene", 1)]
    assert view.flag.shape == (1,) and view.flag.dtype == torch.int32 and int(view.flag) == 0
    view.flag.fill_(1)
    g.flag.zero_()                                                                   # the next batch's guard window opens
    st(_batch([2, 1], [12, 13]))
    assert int(g.flag) == 1
    g.flag.zero_()
    st(_batch([2, 3], [14, 15]))                                                     # does not touch the flagged view
    assert int(g.flag) == 0
