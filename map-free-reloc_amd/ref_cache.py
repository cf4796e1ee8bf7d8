"""What the stages that compute a reference view once share (pipeline._RefCachedKeypointMatcher, pipeline._RefCachedLoFTR, nets/dpt.FusedDepthStage):
the grouping of a batch's pairs by `ref_keys`, the f16x2 range-guard flag a cached view carries, and the LRU.  Storage, kernel calls and counters
stay with the stages.  Imports neither pipeline nor nets: both use it."""
import collections
import typing


class RefEntry:
    """One cached reference view: the stage's payload as attributes (`slot`: a row of LoFTR's pool; `metres`: a depth plane; SuperPoint's rows) and
    flag: a device copy [1] int32 of the range-guard flag, taken right after the launches that computed the view (None while no guard is bound or the
          guard is inactive).  The view was computed under THAT batch's guard window, and a flagged accumulator can leave finite wrong values behind
          (relu(-inf) = 0), so every later batch that reuses the view ORs `flag` into its own live flag (RefViewCache.carry)."""

    def __init__(self, flag, **payload):
        self.flag = flag
        self.__dict__.update(payload)


class RefPlan(typing.NamedTuple):
    keys: list          # one per pair; None replaced by a key of the pair's own
    first: dict         # key -> its first pair, in first-occurrence order
    pairs_of: dict      # key -> all its pairs
    need: list          # keys of `first` that are not cached
    reused: list        # keys of `first` that are
    solo: set           # the keys that stood for None: never equal to another, never retained


class RefViewCache(collections.OrderedDict):
    """key -> RefEntry, least recently used first"""

    def __init__(self, guard=None):
        super().__init__()
        self.guard = guard

    @property
    def guarded(self):
        return self.guard is not None and self.guard.active

    def plan(self, ref_keys):
        keys = [k if k is not None else ("__pair__", p) for p, k in enumerate(ref_keys)]      # None: a reference view nobody shares
        first, pairs_of = {}, {}
        for p, k in enumerate(keys):
            first.setdefault(k, p)
            pairs_of.setdefault(k, []).append(p)
        return RefPlan(keys, first, pairs_of, [k for k in first if k not in self], [k for k in first if k in self],
                       {k for k, r in zip(keys, ref_keys) if r is None})

    def take_flag(self):
        """a copy of the live guard flag, for the entries computed by the launches issued so far (no host read)"""
        return self.guard.flag.clone() if self.guarded else None

    def put(self, key, flag, **payload):
        self[key] = entry = RefEntry(flag, **payload)
        return entry

    def carry(self, plan):
        """OR the flags of the batch's reused entries into the live guard flag, on the device"""
        if self.guarded:
            for k in plan.reused:
                if self[k].flag is not None:
                    self.guard.flag.bitwise_or_(self[k].flag)

    def settle(self, plan, cap):
        """after the batch: its solo keys go, its other keys become the most recently used, the least recently used entries beyond `cap` go"""
        for k in plan.first:
            if k in plan.solo:
                self.pop(k, None)
            elif k in self:
                self.move_to_end(k)
        while len(self) > cap:
            self.popitem(last=False)
