"""Fused on-GPU relative-pose pipeline for batches of image pairs:

    SuperPoint x2 -> SuperGlue -> depth lift -> PnP-RANSAC (+ refinement)      [config sg_pnp_*]

Replaces, for config/matching/mapfree/sg_pnp_dptkitti.yaml, the reference's two-stage flow
(offline etc/feature_matching_baselines/compute.py:72-86 writing correspondences_SG.npz, then
submission.py:33-58 -> FeatureMatchingModel.forward (lib/models/matching/model.py:29-40) ->
PnPSolver.estimate_pose (pose_solver.py:184-235)) with one device-resident pass: matches never
leave HBM, poses come back as one small tensor per batch.  The npz wire format and the per-pair
plugin API stay available (matching/, wire.py) for drop-in use.
"""
import torch

from . import _lib, options
from .nets.graph import GraphOrEager
from .nets.loftr import pad_to_multiple
from .nets.superpoint import SuperPointHIP
from .nets.superglue import SuperGlueHIP
from .nets import weights as WT
from .ref_cache import RefViewCache
from .solver_ops import PnPBatchSolver


ST_RANGE = 7            # include/mfr_hip.h MFR_ST_RANGE


class RangeGuard:
    """The f16x2 range guard of ONE pipeline object (include/mfr_hip.h mfr_f16x2_guard_bind, csrc/guard.h).

    The reference's networks are plain fp32 modules (matchers.py:50,105): they have no |x| <= 65504 precondition, the f16x2 kernels do.  Used as a
    context manager around the matcher stage: the device flag is cleared and bound, every f16x2 launch inside ORs 1 into it when one of its
    accumulators is non-finite (= an operand outside the range, or a non-finite operand), and `fold` turns a set flag into status ST_RANGE for the
    batch's pairs -- all on the device, no host synchronisation, graph-capturable (the clear is a kernel, the pointer is a launch argument).
    Whoever reads the results on the host anyway (submission.predict_fused, the per-pair plugin, the census) calls `rerun_out_of_range`, which runs
    the batch again through the EXACT twin of the pipeline (options SPLIT = 'bf16x3': three-term bf16 operands, the fp32 exponent range)."""

    def __init__(self, device, make_twin):
        self.active = options.get("SPLIT") == "f16x2"
        self.flag = torch.zeros(1, dtype=torch.int32, device=device)
        self._make_twin, self._twin, self.reruns = make_twin, None, 0

    def __enter__(self):
        if self.active:
            self.flag.zero_()
            _lib.call("mfr_f16x2_guard_bind", self.flag.data_ptr())
        return self

    def __exit__(self, *exc):
        if self.active:
            _lib.load().mfr_f16x2_guard_bind(None)
        return False

    def keep(self):
        """context manager that binds the flag WITHOUT clearing it: a later stage of the same pair / batch (LoFTR's fine stage after the match count)"""
        g = self

        class _Keep:
            def __enter__(self):
                if g.active:
                    _lib.call("mfr_f16x2_guard_bind", g.flag.data_ptr())

            def __exit__(self, *exc):
                return g.__exit__()
        return _Keep()

    def snapshot(self):
        """a copy of the flag, made on the CURRENT stream right after the matcher stage: what a solver stage running on another stream folds into the
        status while the next batch's matcher already clears and re-uses the flag itself"""
        return self.flag.clone() if self.active else None

    def fold(self, status, flag=None):
        flag = self.flag if flag is None else flag
        return torch.where(flag > 0, torch.full_like(status, ST_RANGE), status) if self.active else status

    def twin(self):
        if self._twin is None:
            with options.override(SPLIT="bf16x3"):
                self._twin = self._make_twin()
        return self._twin


class SolverOverlap:
    """The solver stage of batch i on a SECOND HIP stream, so that it runs under the matcher stage of batch i + 1 (opt-in: `overlap_solver=True`).

    The RANSAC kernels are latency-bound on small grids -- `pnp_select` is 32 wavefronts on a 1024-SIMD chip, `emat_roots` 16 k threads -- while the
    matcher's convolutions fill the chip: run back to back on one stream the solver's 0.7 ms (SuperGlue + PnP) / 2.9 ms (LoFTR + E-mat) per step are
    almost idle time.  Ordering: the side stream waits for an event recorded after the matcher stage; every tensor it reads that the main stream
    produced is `record_stream`ed (the caching allocator must not recycle it early); successive solver stages are ordered by the side stream itself
    (they share the solvers' workspaces).  The CONSUMER of the results must call `join()` (pipeline.join()) on the stream it reads them from --
    bench.py does so once, before the gather that ends the timed region."""

    def __init__(self, device):
        self.stream = torch.cuda.Stream(device=device)
        self.done, self._outs = None, []

    def run(self, fn, consumed):
        main = torch.cuda.current_stream()
        ev = torch.cuda.Event()
        ev.record(main)
        with torch.cuda.stream(self.stream):
            self.stream.wait_event(ev)
            out = fn()
        for t in consumed:
            if isinstance(t, torch.Tensor) and t.is_cuda:
                t.record_stream(self.stream)
        self.done = torch.cuda.Event()
        self.done.record(self.stream)
        self._outs = [t for t in out.values() if isinstance(t, torch.Tensor) and t.is_cuda]
        return out

    def join(self):
        if self.done is not None:
            cur = torch.cuda.current_stream()
            cur.wait_event(self.done)
            for t in self._outs:                      # allocated on the side stream, read on this one from here on
                t.record_stream(cur)
            self.done, self._outs = None, []


def rerun_out_of_range(pipe, out, *args, **kw):
    """out = pipe(*args, **kw) came back: if the range guard marked the batch (status ST_RANGE; reading it synchronises with the device, so call this
    where the results are read anyway), run the batch again in the exact bf16x3 arithmetic and hand out THAT result"""
    if hasattr(pipe, "join"):
        pipe.join()
    g = getattr(pipe, "guard", None)
    if g is None or not g.active or not bool((out["status"] == ST_RANGE).any()):
        return out
    g.reruns += 1
    with options.override(SPLIT="bf16x3"):                  # layers that resolve the option on their first call (nets/loftr.py) do so in here
        return g.twin()(*args, **kw)


class SuperGluePnPPipeline:
    def __init__(self, device="cuda", sp_state=None, sg_state=None, max_keypoints=1024,
                 pnp_iters=1000, pnp_thr=3.0, pnp_conf=0.9999, seed=0, graph=False, overlap_solver=False):
        """overlap_solver=True: the PnP stage runs on a second stream under the next call's matcher (SolverOverlap; call join() before reading results).
        graph=True: the whole step (SuperPoint x2 -> SuperGlue -> lift -> PnP-RANSAC, ~330 kernel launches) is captured once
        per batch shape and replayed as ONE HIP graph; inputs are copied into the graph's static buffers on every call and the
        (small) results are handed out as copies (nets/graph.py)."""
        _lib.load(require_gpu=True)
        self.graph, self._graphed = bool(graph), GraphOrEager(self._run, "SuperGluePnPPipeline", clone_outputs=True)
        self.device = torch.device(device)
        self.sp = SuperPointHIP(sp_state or WT.superpoint_state_dict(), self.device, max_keypoints=max_keypoints)
        self.sg = SuperGlueHIP(sg_state or WT.superglue_state_dict(), self.device)
        self.pnp = PnPBatchSolver(pnp_iters, pnp_thr, pnp_conf, seed)
        self.K = max_keypoints
        self.guard = RangeGuard(self.device, lambda: SuperGluePnPPipeline(device, sp_state, sg_state, max_keypoints, pnp_iters, pnp_thr, pnp_conf, seed, False))
        self._ov = SolverOverlap(self.device) if (overlap_solver and not graph) else None

    def join(self):
        """make the current stream wait for the solver stage of the last call (only needed with overlap_solver=True)"""
        if self._ov is not None:
            self._ov.join()

    @torch.no_grad()
    def match(self, images):
        """images [2B,1,H,W] -> dict(pts0, pts1 [B,K,2], n_corr [B], ...)  (SuperGlue_matcher.match)"""
        H, W = images.shape[-2:]
        # SuperPoint writes its descriptors straight into the left half of SuperGlue's [x | a] buffer (no desc + h pass); in_place = False: a separate tensor
        sp = self.sp(images, desc_out=self.sg.xa_buffer(images.shape[0], self.K) if self.sg.in_place else None)
        m = self.sg(sp, (H, W), maxN=self.K)
        m["n_kpts"] = sp["n"]
        return m

    def __call__(self, images, depth0, K0, K1, pair_ids, want_mask=False):
        if want_mask or not self.graph:                                # the mask is not among the captured outputs
            return self._run(images, depth0, K0, K1, pair_ids, want_mask)
        args = [images, depth0, K0, K1, pair_ids]
        return self._graphed(tuple((tuple(a.shape), a.dtype) for a in args), *args)      # dtype too: float32 K and float64 K are different arithmetic (k_dtype)

    @torch.no_grad()
    def _run(self, images, depth0, K0, K1, pair_ids, want_mask=False):
        with self.guard:
            m = self.match(images)
        if self._ov is not None:
            bad = self.guard.snapshot()

            def solve():
                o = self.pnp(m["pts0"], m["pts1"], m["n_corr"], depth0, K0, K1, pair_ids, want_mask=want_mask)
                o["status"] = self.guard.fold(o["status"], bad)
                return o
            out = self._ov.run(solve, [m["pts0"], m["pts1"], m["n_corr"], bad, depth0, K0, K1, pair_ids])
        else:
            out = self.pnp(m["pts0"], m["pts1"], m["n_corr"], depth0, K0, K1, pair_ids, want_mask=want_mask)
            out["status"] = self.guard.fold(out["status"])
        out["n_corr"] = m["n_corr"]
        out["pts0"], out["pts1"], out["n_kpts"] = m["pts0"], m["pts1"], m["n_kpts"]
        return out


class LoFTREmatPipeline:
    """LoFTR coarse-to-fine matching -> E-matrix RANSAC -> metric scale from depth
    (config/matching/mapfree/loftr_emat_dptkitti.yaml: PIX_THRESHOLD 2.0, SCALE_THRESHOLD 0.1,
    CONFIDENCE 0.9999), one device-resident pass over a batch of pairs.  Replaces
    LoFTR_matcher.match (matchers.py:24-59) + EssentialMatrixMetricSolver (pose_solver.py:115-172)."""

    def __init__(self, device="cuda", loftr_state=None, pix_thr=2.0, scale_thr=0.1, conf=0.9999, seed=0, pad_to=8, emat_score="magsac", overlap_solver=False,
                 match_type="dual_softmax", skh_iters=3):
        from .nets.loftr import LoFTRHIP
        from .solver_ops import EssentialBatchSolver, ScaleFromDepthBatch
        _lib.load(require_gpu=True)
        self.device = torch.device(device)
        self.loftr = LoFTRHIP(loftr_state or WT.loftr_state_dict(), self.device, match_type=match_type, skh_iters=skh_iters)
        self.emat = EssentialBatchSolver(pix_thr, conf, seed, score=emat_score)
        self.scale = ScaleFromDepthBatch(scale_thr)
        self.pad_to = pad_to
        self.guard = RangeGuard(self.device, lambda: LoFTREmatPipeline(device, loftr_state, pix_thr, scale_thr, conf, seed, pad_to, emat_score,
                                                                        match_type=match_type, skh_iters=skh_iters))
        self._ov = SolverOverlap(self.device) if overlap_solver else None      # E-mat + scale stage under the next call's matcher; join() before reading
        self._ref = _RefCachedLoFTR(self.loftr, self.guard, pad_to)

    def join(self):
        if self._ov is not None:
            self._ov.join()

    @torch.no_grad()
    def match(self, images, ref_keys=None):
        """ref_keys (one per pair, as PairBatchLoader's `ref_keys`; None = no sharing): the backbone runs once per distinct reference view
        (_RefCachedLoFTR), same bits"""
        return self._ref.plain(images) if ref_keys is None else self._ref(dict(images=images, ref_keys=ref_keys))

    @torch.no_grad()
    def __call__(self, images, depth0, depth1, K0, K1, pair_ids, ref_keys=None):
        with self.guard:
            m = self.match(images, ref_keys)
        bad = self.guard.snapshot() if self._ov is not None else None

        def solve():
            e = self.emat(m["pts0"], m["pts1"], m["n_corr"], K0, K1, pair_ids)
            s = self.scale(m["pts0"], m["pts1"], e["mask"], m["n_corr"], depth0, depth1, K0, K1, e["R"], e["t"], e["status"])
            s["status"] = self.guard.fold(s["status"], bad)
            return dict(R=torch.where((s["status"] == 0)[:, None, None], e["R"], torch.full_like(e["R"], float("nan"))),
                        t=s["t_metric"], n_inliers=s["n_inliers"], status=s["status"], emat_inliers=e["n_inliers"], emat_mask=e["mask"])
        out = self._ov.run(solve, [m["pts0"], m["pts1"], m["n_corr"], bad, depth0, depth1, K0, K1, pair_ids]) if self._ov is not None else solve()
        out.update(n_corr=m["n_corr"], pts0=m["pts0"], pts1=m["pts1"])
        return out


# ---------------------------------------------------------------------------------------------------------------
# config-driven fused pipeline: any matcher stage x any solver stage, batched (what submission.predict_fused runs)
# ---------------------------------------------------------------------------------------------------------------
class _PrecomputedStage:
    """cfg.FEATURE_MATCHING == 'Precomputed' (feature_matching.py:5-50) for a batch: npz rows -> device layout"""

    def __init__(self, cfg, device):
        from .matching.feature_matching import PrecomputedMatching
        self.pm, self.device = PrecomputedMatching(cfg), device

    def __call__(self, batch):
        import numpy as np
        from . import wire
        rows = []
        pids = batch["seed_ids"].tolist()
        sids = batch.get("scene_ids") or [batch["scene_id"]] * len(pids)           # batches may span scenes (PairBatchLoader)
        roots = batch.get("scene_roots") or [batch.get("scene_root", "")] * len(pids)
        for pid, sid, root in zip(pids, sids, roots):
            p1, p2 = self.pm.get_correspondences({"scene_id": [sid], "scene_root": [root], "pair_id": pid})
            rows.append(np.concatenate([p1, p2], 1) if len(p1) else np.zeros((0, 4), np.float32))
        p0, p1, n = wire.pts_rows_to_device_batch(rows)
        d = lambda a: torch.from_numpy(a).to(self.device)
        return dict(pts0=d(p0), pts1=d(p1), n_corr=d(n))


class _RefCachedKeypointMatcher:
    """SuperPoint + a keypoint matcher (`net`: SuperGlueHIP or LightGlueHIP, the same call) over a batch of pairs with ONE SuperPoint pass per distinct
    reference view.

    Every val / test pair of a Map-free scene has the same reference image, seq0/frame_00000.jpg
    (etc/feature_matching_baselines/compute.py:72-75, lib/datasets/mapfree.py:148-165); the reference runs the detector on it once per
    pair (116 times per scene).  Here the batch's pairs are grouped by `ref_keys` (PairBatchLoader: (scene_root, reference frame
    name)); SuperPoint runs on [the reference views not seen yet | all query views]; the reference rows of the interleaved
    [2B] keypoint / score / descriptor tensors the matcher consumes are gathered from a small cache (ref_cache.RefViewCache, the last few reference
    views: a scene's pairs span several batches; each view with the range-guard flag of the pass that computed it).  Every SuperPoint stage is per image
    with a fixed summation order (own convolutions, own 1x1 heads), so the result is the SAME BITS as the plain path --
    tests/test_gpu_fused_submission.py checks poses byte for byte."""
    FIELDS = ("kpts", "scores", "desc", "n")

    def __init__(self, sp, net, max_kpts, plain, guard=None, keep=4):
        self.sp, self.net, self.K, self.plain, self.keep = sp, net, max_kpts, plain, keep
        self.cache = RefViewCache(guard)                                          # key -> RefEntry(flag, rows: the view's SuperPoint rows [1, ...])
        self.stats = dict(reference_views_run=0, reference_views_reused=0)

    def __call__(self, b):
        im, keys = b["images"], b.get("ref_keys")
        if keys is None or len(keys) * 2 != im.shape[0]:
            return self.plain(im)
        B = len(keys)
        plan = self.cache.plan(keys)
        need = plan.need
        parts = [im[2 * plan.first[k]][None] for k in need] + [im[1::2]]
        out = self.sp(torch.cat(parts) if need else im[1::2].contiguous())
        u = len(need)
        flag = self.cache.take_flag() if need else None
        for i, k in enumerate(need):
            self.cache.put(k, flag, rows={f: out[f][i:i + 1].clone() for f in self.FIELDS})
        self.cache.carry(plan)
        self.stats["reference_views_run"] += u
        self.stats["reference_views_reused"] += B - u
        sp2 = {}
        for f in self.FIELDS:
            ref = torch.cat([self.cache[k].rows[f] for k in plan.keys])           # [B, ...] reference rows (no index tensor: an H2D copy would
            qry = out[f][u:]                                                       # synchronise the stream once per batch)
            sp2[f] = torch.stack([ref, qry], 1).reshape((2 * B,) + tuple(qry.shape[1:]))
        self.cache.settle(plan, max(self.keep, len(plan.first)))
        return self.net(sp2, tuple(im.shape[-2:]), maxN=self.K)


class _RefCachedLoFTR:
    """LoFTR over a batch of pairs with ONE backbone pass per distinct reference view: the twin of _RefCachedKeypointMatcher, same contract.

    The batch's pairs are grouped by `ref_keys` (None: a view nobody shares -- run, not retained); the ResNet-FPN runs on [the reference views not
    cached yet | all query views] (after the pad-to-8 of the plain path); new reference rows are copied once, device to device, into a small pool of
    coarse / fine maps (an LRU of `keep` views, or the batch's distinct views if more), and everything after the backbone reads side 0 from the pool
    and side 1 from this batch's output by index (LoFTRHIP.match_features): no interleaved copy of either map is made.  A batch in which every
    reference view is new reads side 0 from its own backbone output.  The backbone's kernels tile per image with a fixed summation order, so the
    result is the SAME BITS as the plain path (tests/test_gpu_loftr_ref_cache.py).  A batch without usable `ref_keys` takes the plain path.

    Not covered: the per-pair plugin and its batch-1 graph replay, the reference side's first self-attention layer (it could be cached the same
    way), query-side keys (7Scenes / ScanNet would enter through the same (feature set, index) interface) and HIP.GRAPH_FUSED."""

    def __init__(self, net, guard=None, pad_to=8, keep=4):
        self.net, self.guard, self.pad_to, self.keep = net, guard, pad_to, keep
        self.cache = RefViewCache(guard)                                          # key -> RefEntry(flag, slot: its row in the pool's coarse and fine maps)
        self.pool, self._hw = None, None                                          # LoFTRFeatures [slots, ...] of images of size _hw
        self.stats = dict(reference_views_run=0, reference_views_reused=0)

    def plain(self, images):
        return self.net(pad_to_multiple(images, self.pad_to))

    def _free_slots(self, n_new, first, like):
        """room for n_new more views: evict least recently used views the batch does not use, grow the pool to the batch's distinct views if needed"""
        cap = max(self.keep, len(first))
        while len(self.cache) + n_new > cap:
            del self.cache[next(k for k in self.cache if k not in first)]
        if self.pool is None or self.pool[0].shape[0] < cap:
            grown = type(like)(*(t.new_empty((cap,) + tuple(t.shape[1:])) for t in like))
            if self.pool is not None:
                for g, t in zip(grown, self.pool):
                    g[:t.shape[0]].copy_(t)
            self.pool = grown
        used = {v.slot for v in self.cache.values()}
        return [s for s in range(self.pool[0].shape[0]) if s not in used]

    @torch.no_grad()
    def __call__(self, b):
        im, keys = b["images"], b.get("ref_keys")
        if keys is None or len(keys) * 2 != im.shape[0]:
            return self.plain(im)
        im = pad_to_multiple(im, self.pad_to)
        B = len(keys)
        if self._hw != tuple(im.shape[-2:]):                                      # another image size: the pooled maps do not fit
            self.cache.clear()
            self.pool, self._hw = None, tuple(im.shape[-2:])
        plan = self.cache.plan(keys)
        first, need = plan.first, plan.need
        u = len(need)
        out = self.net.features(torch.cat([im[2 * first[k]][None] for k in need] + [im[1::2]]))
        flag = self.cache.take_flag()                                             # one copy per backbone pass
        self.stats["reference_views_run"] += u
        self.stats["reference_views_reused"] += B - u
        store = need if plan.reused else [k for k in need if k not in plan.solo]  # nothing reused: side 0 is read from `out` itself
        free = self._free_slots(len(store), first, out) if store else []
        for k in store:
            v = self.cache.put(k, flag, slot=free.pop(0))
            for pooled, fresh in zip(self.pool, out):
                pooled[v.slot].copy_(fresh[need.index(k)])
        if plan.reused:
            src0, idx0 = self.pool, [self.cache[k].slot for k in plan.keys]
            self.cache.carry(plan)
        else:
            src0, idx0 = out, [need.index(k) for k in plan.keys]
        m = self.net.match_features(src0, idx0, out, list(range(u, u + B)), im.shape[2])
        self.cache.settle(plan, max(self.keep, len(first)))
        return m


def _hip_flag(cfg, name):
    """an optional boolean of cfg.HIP (REF_FEATURE_CACHE, GRAPH_FUSED): absent = off"""
    return name in cfg.HIP and bool(cfg.HIP[name])


class _EfficientLoFTRStage:
    """EfficientLoFTR on the fused route.  The per-image part is the backbone's three maps: _RefCachedLoFTR's pool, the same bits.  That stage pads, so the
    network is told the unpadded frame: matches outside it are dropped"""

    def __init__(self, net, guard, pad_to, cached):
        self.net, self.cached, self.ref = net, cached, _RefCachedLoFTR(net, guard, pad_to=pad_to)
        self.stats = self.ref.stats                                            # reference_views_run / _reused, as the LoFTR stage reports them

    def __call__(self, b):
        self.net.frame_hw = tuple(b["images"].shape[-2:])
        return self.ref(b) if self.cached else self.ref.plain(b["images"])


def _keypoint_stage(cfg, guard, sp, net, K, graphed=False):
    """SuperPoint + SuperGlue / LightGlue: graph replay (HIP.GRAPH_FUSED, where the matcher can be captured), one SuperPoint pass per reference view
    (HIP.REF_FEATURE_CACHE), or plain"""
    fwd = lambda images: net(sp(images), tuple(images.shape[-2:]), maxN=K)
    if graphed:
        # the matcher stage (~300 launches) replayed from one HIP graph per batch shape; at most two shapes are captured (the full batch and one
        # remainder), anything else -- and images that are not on the device -- runs eagerly: every capture pins its intermediates
        run = GraphOrEager(torch.no_grad()(fwd), "FusedPosePipeline", clone_outputs=True, max_keys=2)
        return lambda b: run(tuple(b["images"].shape), b["images"]) if b["images"].is_cuda else fwd(b["images"])
    return _RefCachedKeypointMatcher(sp, net, K, fwd, guard) if _hip_flag(cfg, "REF_FEATURE_CACHE") else (lambda b: fwd(b["images"]))


def _superglue_stage(cfg, device, guard):
    from .nets import superglue as SG
    return _keypoint_stage(cfg, guard, *SG.from_cfg(cfg, device), cfg.SUPERGLUE.MAX_KEYPOINTS, graphed=_hip_flag(cfg, "GRAPH_FUSED"))


def _lightglue_stage(cfg, device, guard):
    from .nets import lightglue as LG
    return _keypoint_stage(cfg, guard, *LG.from_cfg(cfg, device), cfg.LIGHTGLUE.MAX_KEYPOINTS)      # eager: this stage is not graph-captured


def _loftr_stage(cfg, device, guard):
    from .nets import loftr as LO
    stage = _RefCachedLoFTR(LO.from_cfg(cfg, device), guard)
    # the backbone once per distinct reference view (both MATCH_TYPEs); switched off, every batch takes the stage's plain path
    return stage if _hip_flag(cfg, "REF_FEATURE_CACHE") else (lambda b: stage.plain(b["images"]))


def _eloftr_stage(cfg, device, guard):
    from .nets import eloftr as EL
    return _EfficientLoFTRStage(EL.from_cfg(cfg, device), guard, EL.PAD_TO, _hip_flag(cfg, "REF_FEATURE_CACHE"))


def _sift_stage(cfg, device, guard):
    if cfg.SIFT.get("DETECTOR", "opencv") != "hip":
        raise _no_batched_stage("SIFT")
    from .sift_ops import SiftDetector, sift_ratio_stage
    return sift_ratio_stage(SiftDetector(cfg.SIFT.NUM_FEATURES, device), cfg.SIFT.RATIO_THRESHOLD)


def _no_batched_stage(fm):
    return NotImplementedError(f"FEATURE_MATCHING={fm!r} has no batched stage (SIFT with DETECTOR 'opencv' is OpenCV / per pair)")


# cfg.FEATURE_MATCHING -> builder(cfg, device, guard) -> stage: a callable on the batch dict, with `.stats` where it keeps counters (the batched twin of
# matching/model.FEATURE_MATCHERS)
MATCHER_STAGES = {"Precomputed": lambda cfg, device, guard: _PrecomputedStage(cfg, device), "SuperGlue": _superglue_stage, "LightGlue": _lightglue_stage,
                  "LoFTR": _loftr_stage, "EfficientLoFTR": _eloftr_stage, "SIFT": _sift_stage}


class FusedPosePipeline:
    """The batched twin of FeatureMatchingModel (lib/models/matching/model.py:7-40): the same two config keys pick the
    stages -- FEATURE_MATCHING in {'Precomputed', 'SuperGlue', 'LightGlue', 'LoFTR', 'EfficientLoFTR', 'SIFT' (SIFT.DETECTOR 'hip')} x POSE_SOLVER in {'PNP', 'EssentialMatrix',
    'EssentialMatrixMetric', 'Procrustes'} -- but every stage consumes / produces a device-resident batch of pairs.
    __call__(batch) with the dict PairBatchLoader yields -> dict(R [b,3,3] f64, t [b,3] f64, n_inliers, status, n_corr).
    With DPT.SOURCE 'online' the batch carries `rgb` instead of depth maps (PairBatchLoader(rgb=True)) and the maps are computed here; the result then also
    holds depth0 (and depth1 when the solver reads it), the planes the solver was given."""

    def __init__(self, cfg, device="cuda"):
        from . import solver_ops as ops
        _lib.load(require_gpu=True)
        self.device = torch.device(device)
        self.guard = RangeGuard(self.device, lambda: FusedPosePipeline(cfg, device))
        seed = int(cfg.RANSAC.SEED) if "RANSAC" in cfg else 0
        fm = cfg.FEATURE_MATCHING
        if fm not in MATCHER_STAGES:
            raise _no_batched_stage(fm)
        self.match = MATCHER_STAGES[fm](cfg, self.device, self.guard)
        ps = cfg.POSE_SOLVER
        if ps == "PNP":
            pnp = ops.PnPBatchSolver(cfg.PNP.RANSAC_ITER, cfg.PNP.REPROJECTION_INLIER_THRESHOLD, cfg.PNP.CONFIDENCE, seed)
            self.solve = lambda m, b: pnp(m["pts0"], m["pts1"], m["n_corr"], b["depth0"], b["K0"], b["K1"], b["seed_ids"])
        elif ps in ("EssentialMatrix", "EssentialMatrixMetric"):
            em = ops.EssentialBatchSolver(cfg.EMAT_RANSAC.PIX_THRESHOLD, cfg.EMAT_RANSAC.CONFIDENCE, seed,
                                          score=cfg.HIP.EMAT_SCORE, max_thr_ratio=cfg.HIP.MAGSAC_MAX_THR_RATIO)
            sc = ops.ScaleFromDepthBatch(cfg.EMAT_RANSAC.SCALE_THRESHOLD) if ps == "EssentialMatrixMetric" else None

            def solve(m, b):
                e = em(m["pts0"], m["pts1"], m["n_corr"], b["K0"], b["K1"], b["seed_ids"])
                if sc is None:
                    return e
                s = sc(m["pts0"], m["pts1"], e["mask"], m["n_corr"], b["depth0"], b["depth1"], b["K0"], b["K1"], e["R"], e["t"], e["status"])
                return dict(R=e["R"], t=s["t_metric"], n_inliers=s["n_inliers"], status=s["status"])
            self.solve = solve
        elif ps == "Procrustes":
            pr = ops.ProcrustesBatchSolver(cfg.PROCRUSTES.MAX_CORR_DIST, 0.999, seed)
            icp = ops.ProcrustesIcpRefine(cfg.PROCRUSTES.MAX_CORR_DIST, 1e-4, 1e-4, 30) if cfg.PROCRUSTES.REFINE else None

            def solve_pr(m, b):
                o = pr(m["pts0"], m["pts1"], m["n_corr"], b["depth0"], b["depth1"], b["K0"], b["K1"], b["seed_ids"])
                if icp is not None:
                    o = dict(o, n_inliers=icp(b["depth0"], b["depth1"], b["K0"], b["K1"], o["R"], o["t"], o["status"])["n_inliers"])
                return o
            self.solve = solve_pr
        else:
            raise NotImplementedError(f"POSE_SOLVER={ps!r}")
        # DPT.SOURCE 'online': the depth maps the solver reads are computed here from batch['rgb'] (nets/dpt.FusedDepthStage), a reference view once per scene.
        # A solver that reads no depth (EssentialMatrix) builds no stage, needs no DPT weights and asks the loader for no colour bytes (`needs_rgb`)
        from .nets import dpt as DPT
        views = DPT.fused_depth_views(cfg)
        self.depth = None
        if views is not None:
            self.depth = DPT.FusedDepthStage(cfg, self.device, self.guard, views, cache=_hip_flag(cfg, "REF_FEATURE_CACHE"))
        self.needs_rgb = self.depth is not None

    @property
    def stats(self):
        """the counters of the stages that keep some: the matcher's reference_views_run / _reused, the depth stage's depth_views_run / _reused"""
        return dict(getattr(self.match, "stats", {}), **(self.depth.stats if self.depth is not None else {}))

    @torch.no_grad()
    def __call__(self, batch):
        with self.guard:
            m = self.match(batch)
            if self.depth is not None:                          # inside the guard's window: a flagged DPT launch marks the rows ST_RANGE like a matcher's
                batch = self.depth(dict(batch))
        out = self.solve(m, batch)
        out["status"] = self.guard.fold(out["status"])
        ok = (out["status"] == 0)
        nan = float("nan")
        return dict(R=torch.where(ok[:, None, None], out["R"], torch.full_like(out["R"], nan)),
                    t=torch.where(ok[:, None], out["t"], torch.full_like(out["t"], nan)),
                    n_inliers=torch.where(ok, out["n_inliers"], torch.zeros_like(out["n_inliers"])), status=out["status"],
                    n_corr=m["n_corr"], **({k: batch[k] for k in ("depth0", "depth1") if batch.get(k) is not None} if self.depth is not None else {}))
