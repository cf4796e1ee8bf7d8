"""FeatureMatchingModel -- the model plugin of the matching path (contract: lib/models/matching/model.py:7-40):

    build_model(cfg)(data) -> (R [1,3,3] f32, t [1,1,3] f32), and data['inliers'] = the solver's confidence.

Two registries replace the reference's dispatch chains; `cfg.FEATURE_MATCHING` / `cfg.POSE_SOLVER` name the
entries, so a new correspondence source or solver is one `register_*` call.  Batch size is 1 on this surface
(the reference's contract); submission.predict_fused / pipeline.FusedPosePipeline are the batched twins.

FeatureMatchingMultiFrameModel (MODEL: 'FeatureMatchingMultiFrame') is the matching family's consumer of multi-frame samples
(DATASET.QUERY_FRAME_COUNT > 1, datasets.MapFreeSceneMultiFrame): the reference view is matched against all T window frames and ONE
pose is solved for the rig the device-tracking poses make of them: POSE_SOLVER 'PNP' (alias 'RigPNP', csrc/pnp_rig.hip: depth on the
reference side), 'RigProcrustes' (the rig entry point of csrc/procrustes.hip: depth on both sides, all T + 1 maps) or 'RigEssentialMatrix'
(csrc/emat_rig.hip: no depth, the rig's baselines fix the scale).  The reference has no counterpart: its only multi-frame consumer,
RegressionMultiFrameModel, regresses against the last frame.
"""
import numpy as np
import torch

from .. import solver_ops as ops
from . import feature_matching as _fm
from . import pose_solver as _ps

FEATURE_MATCHERS = {
    'SIFT': _fm.SIFTMatching,
    'Precomputed': _fm.PrecomputedMatching,
    'SuperGlue': _fm.SuperGlueMatching,      # online, GPU (new)
    'LoFTR': _fm.LoFTRMatching,              # online, GPU (new)
    'LightGlue': _fm.LightGlueMatching,      # online, GPU (new): SuperPoint + LightGlue
    'EfficientLoFTR': _fm.EfficientLoFTRMatching,    # online, GPU (new): nets/eloftr.py
}
POSE_SOLVERS = {
    'EssentialMatrix': _ps.EssentialMatrixSolver,
    'EssentialMatrixMetric': _ps.EssentialMatrixMetricSolver,
    'Procrustes': _ps.ProcrustesSolver,
    'PNP': _ps.PnPSolver,
}


def register_feature_matcher(name, cls):
    FEATURE_MATCHERS[name] = cls


def register_pose_solver(name, cls):
    POSE_SOLVERS[name] = cls


def _lookup(table, key, what):
    if key not in table:
        raise NotImplementedError(f'Invalid {what}: {key!r} (known: {sorted(table)})')
    return table[key]


class FeatureMatchingModel(torch.nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.feature_matching = _lookup(FEATURE_MATCHERS, cfg.FEATURE_MATCHING, 'feature matching')(cfg)
        self.pose_solver = _lookup(POSE_SOLVERS, cfg.POSE_SOLVER, 'pose solver')(cfg)
        self.depth = None
        if 'DPT' in cfg and cfg.DPT.SOURCE != 'file':           # DPT.SOURCE 'online': the solver's depth maps come from the pair's images (nets/dpt.py)
            from ..nets.dpt import DepthEstimator
            self.depth = DepthEstimator(cfg)

    def forward(self, data):
        if data['depth0'].shape[0] != 1:
            raise AssertionError('Baseline models require batch size of 1')
        # one batched call for both views, on the loader's images: the file resized to DATASET.WIDTH x HEIGHT.  compute_depth works on the file's own pixels, so the two
        # routes give the solver the same bits only where that is the file's size (Map-free's frames and default)
        if self.depth is not None:
            if data['image0'].shape != data['image1'].shape:
                raise ValueError('DPT.SOURCE online: the two views of a pair must have one size')
            d = self.depth.metres(torch.cat([data['image0'], data['image1']]).to(torch.float32)).cpu()
            data['depth0'], data['depth1'] = d[0:1], d[1:2]
        kpts0, kpts1 = self.feature_matching.get_correspondences(data)
        R, t, confidence = self.pose_solver.estimate_pose(kpts0, kpts1, data)
        data['inliers'] = confidence
        as_f32 = lambda a, shape: torch.from_numpy(np.array(a, dtype=np.float32, copy=True).reshape(shape))
        return as_f32(R, (1, 3, 3)), as_f32(t, (1, 1, 3))


class FeatureMatchingMultiFrameModel(torch.nn.Module):
    """data of ONE multi-frame sample (image1 [1,T,3,H,W], K_color1_multi [1,T,3,3], rig_T [1,T,4,4]) -> (R [1,3,3] f32, t [1,1,3] f32) from the
    reference view to the LAST window frame, data['inliers'] = the pooled RANSAC inlier count.

    The T pairs (reference, frame j) go through the batched matcher stage of pipeline.FusedPosePipeline as one batch: interleaved [2T,1,H,W]
    gray planes with T equal `ref_keys`, so SuperPoint / LoFTR's backbone runs once on the reference view (HIP.REF_FEATURE_CACHE, forced on
    here).  'Precomputed' reads the ordinary single-frame correspondences_*.npz: the row of a window frame is its position among the seq1
    frames of poses.txt, as wire.py writes it.  Then solver_ops.RigPnPBatchSolver ('PNP' / 'RigPNP': reads depth0) or
    solver_ops.RigProcrustesBatchSolver ('RigProcrustes': reads depth0 and depth1 [1,T,H,W]; PROCRUSTES.REFINE, the whole-cloud ICP, is
    refused on a rig) or solver_ops.RigEssentialBatchSolver ('RigEssentialMatrix': reads no depth, builds no depth stage, opens no depth
    file).  The plain single-frame names other than 'PNP' stay refused: a rig solver has a name of its own.  A sample without `rig_T` (no poses_device.txt in the
    scene) is an error: there is no silent fall-back to the last frame alone.  With DPT.SOURCE 'online' the reference view's depth map is computed by the
    fused route's depth stage (nets/dpt.FusedDepthStage), once per distinct reference view; 'RigProcrustes' asks the same call for the T window maps too."""
    MATCHERS = ('SuperGlue', 'LightGlue', 'LoFTR', 'SIFT', 'Precomputed')
    RIG_SOLVERS = {'PNP': 'PNP', 'RigPNP': 'PNP', 'RigProcrustes': 'Procrustes', 'RigEssentialMatrix': 'EssentialMatrix'}      # name -> the single-frame solver whose stages (depth views) the pipeline builds

    def __init__(self, cfg):
        super().__init__()
        if cfg.POSE_SOLVER not in self.RIG_SOLVERS:
            raise NotImplementedError(f"FeatureMatchingMultiFrame solves the rig with POSE_SOLVER 'PNP' (alias 'RigPNP'), 'RigProcrustes' or 'RigEssentialMatrix', "
                                      f"got {cfg.POSE_SOLVER!r}")
        self.kind = self.RIG_SOLVERS[cfg.POSE_SOLVER]
        if self.kind == 'Procrustes' and cfg.PROCRUSTES.REFINE:
            raise NotImplementedError("FeatureMatchingMultiFrame: PROCRUSTES.REFINE (whole-cloud ICP) is not defined for a rig; set PROCRUSTES.REFINE: False")
        fm = cfg.FEATURE_MATCHING
        if fm not in self.MATCHERS or (fm == 'SIFT' and cfg.SIFT.get('DETECTOR', 'opencv') != 'hip'):
            raise NotImplementedError(f"FeatureMatchingMultiFrame: FEATURE_MATCHING={fm!r} has no batched stage "
                                      f"(known: {sorted(self.MATCHERS)}; SIFT needs SIFT.DETECTOR 'hip')")
        from ..pipeline import FusedPosePipeline
        self.cfg = cfg.clone()
        self.cfg.HIP.REF_FEATURE_CACHE = True
        self.cfg.HIP.GRAPH_FUSED = False                        # the captured stage takes no ref_keys
        pcfg = self.cfg.clone()
        pcfg.POSE_SOLVER = self.kind                            # the pipeline knows the single-frame names: its matcher and depth stages are what is used of it
        pipe = FusedPosePipeline(pcfg)
        self.match, self.guard, self.device = pipe.match, pipe.guard, pipe.device
        self.depth = pipe.depth                                 # DPT.SOURCE 'online': the maps come from the fused route's stage (PNP reads depth0 only, Procrustes all T + 1)
        seed = int(cfg.RANSAC.SEED) if 'RANSAC' in cfg else 0
        if self.kind == 'PNP':
            self.solver = ops.RigPnPBatchSolver(cfg.PNP.RANSAC_ITER, cfg.PNP.REPROJECTION_INLIER_THRESHOLD, cfg.PNP.CONFIDENCE, seed)
        elif self.kind == 'Procrustes':
            self.solver = ops.RigProcrustesBatchSolver(cfg.PROCRUSTES.MAX_CORR_DIST, 0.999, seed)
        else:
            self.solver = ops.RigEssentialBatchSolver(cfg.EMAT_RANSAC.PIX_THRESHOLD, cfg.EMAT_RANSAC.CONFIDENCE, seed, score=cfg.HIP.EMAT_SCORE,
                                                      max_thr_ratio=cfg.HIP.MAGSAC_MAX_THR_RATIO)
        self.precomputed = fm == 'Precomputed'
        self._seq1, self._twin = {}, None

    @property
    def stats(self):
        """the matcher stage's reference-view counters (reference_views_run / reference_views_reused), {} for stages without a cache"""
        return getattr(self.match, 'stats', {})

    def _rows(self, data):
        """npz rows of the window frames: positions in the scene's seq1 frame list"""
        import os
        from .. import wire
        root = data['scene_root'][0]
        if root not in self._seq1:
            self._seq1 = {root: {n: i for i, n in enumerate(wire.parse_mapfree_query_frames(os.path.join(root, 'poses.txt')))}}
        return [self._seq1[root][n] for n in data['pair_names'][1][0]]

    @torch.no_grad()
    def forward(self, data):
        from .. import options, pipeline
        from ..datasets import MissingDataError, to_gray
        if data['depth0'].shape[0] != 1:
            raise AssertionError('Baseline models require batch size of 1')
        if 'rig_T' not in data or 'K_color1_multi' not in data:
            raise MissingDataError(f"scene {data.get('scene_id', ['?'])[0]!r}: a multi-frame sample needs the device-tracking poses "
                                   f"(poses_device.txt) that relate its window frames; the file is absent")
        dev = self.device
        T = data['image1'].shape[1]
        batch = dict(scene_id=data['scene_id'][0], scene_root=data['scene_root'][0])
        if self.precomputed:
            batch['seed_ids'] = torch.tensor(self._rows(data), dtype=torch.int64)
        else:
            ref = to_gray(data['image0'][0].to(dev))
            planes = [p for j in range(T) for p in (ref, to_gray(data['image1'][0, j].to(dev)))]
            batch['images'] = torch.stack(planes)[:, None].to(torch.float32).contiguous()
            batch['ref_keys'] = [(batch['scene_root'], data['pair_names'][0][0])] * T
        with self.guard:
            m = self.match(batch)
            if self.depth is not None:                          # the colour bytes of the reference view (image0 is byte / 255), once per distinct reference view
                views = data['image0'] if self.kind == 'PNP' else torch.cat([data['image0'], data['image1'][0]])    # Procrustes: then the T window frames (E-matrix: no stage)
                rgb = (views.to(dev, torch.float32) * 255.0).round().clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
                planes = self.depth.maps(rgb, [0], [(batch['scene_root'], data['pair_names'][0][0])], query_rows=range(1, rgb.shape[0]))
                data['depth0'] = planes[0:1]
                if self.kind != 'PNP':
                    data['depth1'] = planes[1:][None]
        depths = [data[k].to(dev, torch.float32) for k in {'PNP': ('depth0',), 'Procrustes': ('depth0', 'depth1'), 'EssentialMatrix': ()}[self.kind]]
        out = self.solver(m['pts0'][None], m['pts1'][None], m['n_corr'][None].to(torch.int32), *depths,
                          data['K_color0'].to(dev), data['K_color1_multi'].to(dev), data['rig_T'].to(dev, torch.float64),
                          data['pair_id'].to(dev, torch.int64).reshape(1))
        st = self.guard.fold(out['status'])
        flat = torch.cat([t.reshape(-1).to(torch.float64) for t in (st, out['R'], out['t'], out['n_inliers'])]).cpu().numpy()   # one D2H copy
        if int(flat[0]) == pipeline.ST_RANGE:                   # an activation left the f16x2 range: the same sample through the exact twin
            self.guard.reruns += 1
            with options.override(SPLIT='bf16x3'):
                if self._twin is None:
                    self._twin = FeatureMatchingMultiFrameModel(self.cfg)
                return self._twin(data)
        ok = int(flat[0]) == ops.ST_OK
        R = flat[1:10] if ok else np.full(9, np.nan)
        t = flat[10:13] if ok else np.full(3, np.nan)
        data['inliers'] = int(flat[13]) if ok else 0
        as_f32 = lambda a, shape: torch.from_numpy(np.array(a, dtype=np.float32, copy=True).reshape(shape))
        return as_f32(R, (1, 3, 3)), as_f32(t, (1, 1, 3))
