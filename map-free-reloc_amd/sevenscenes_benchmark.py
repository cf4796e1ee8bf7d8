"""7Scenes visual localisation benchmark (benchmark/sevenscenes.py:17-145).

    python -m mapfree_reloc_amd.sevenscenes_benchmark <config> <dataset_config> [--checkpoint CKPT] [--test_pair_txt TXT] [--output_root DIR]
                                                      [--one_nn] [--triang] [--triang_ransac_thres N ...] [--fused] [--batch_pairs N]

Every query image is paired with several database images; the model plugin estimates each pair's relative pose, and the query's absolute
pose is fused from them on the device (localize_ops.fuse_abs_pose, one launch per scene): geometric median + chordal mean by default,
triangulation RANSAC with --triang.  Default route: the reference's loop, one pair at a time through build_model(cfg)(data).  --fused:
PairBatchLoader -> DevicePrefetcher -> FusedPosePipeline; the pipeline's float64 poses are rounded to float32 (what the plugin returns)
and a batch's labels are looked up by its `global_ids`.  Both routes write the same files under --output_root: test_results.txt (the
printed report), rawpred.npz (every scene's pairs as arrays), results.npz (per-query poses, errors, confidences and the precision /
recall arrays the reference plots), pose_<scene>.txt.  --save_video and the plots are not built.
"""
import argparse
from pathlib import Path

import numpy as np
import torch

from . import localize as L


def _np(v):
    v = v[0] if isinstance(v, (list, tuple)) else v
    return (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)).reshape(-1)


def _scene_pairs(records):
    """records of one scene in loader order -> ScenePairs (queries in the order they first appear, a query's pairs in loader order)"""
    qidx = {}
    for r in records:
        qidx.setdefault(r['query'], len(qidx))
    order = sorted(range(len(records)), key=lambda i: qidx[records[i]['query']])            # stable
    rs = [records[i] for i in order]
    first = {}
    for r in records:
        first[r['query']] = r                                                             # :46 -- the last pair's label stays (all equal)
    names = list(qidx)
    col = lambda k, *shape: np.stack([np.asarray(r[k], np.float64).reshape(shape) for r in rs]) if rs else np.zeros((0, *shape))
    return L.ScenePairs(query_names=names, query_q=np.stack([first[n]['query_q'] for n in names]), query_c=np.stack([first[n]['query_c'] for n in names]),
                        pair_query=[qidx[r['query']] for r in rs], train_q=col('train_q', 4), train_c=col('train_c', 3), R_pred=col('R', 3, 3),
                        t_pred=col('t', 3), R_gt=col('R_gt', 3, 3), t_gt=col('t_gt', 3), sim=[r['sim'] for r in rs],
                        inliers=np.array([r['inliers'] for r in rs], np.int64),
                        valid=[not (np.isnan(r['R']).any() or np.isnan(r['t']).any() or np.isinf(r['t']).any()) for r in rs])        # sevenscenes.py:55


def _record(query, train_q, train_c, query_q, query_c, T, sim, R, t, inliers):
    T = np.asarray(T, np.float32).reshape(4, 4)
    return dict(query=str(query), train_q=np.asarray(train_q, np.float32), train_c=np.asarray(train_c, np.float32),
                query_q=np.asarray(query_q, np.float32), query_c=np.asarray(query_c, np.float32), R_gt=T[:3, :3], t_gt=T[:3, 3],
                sim=float(sim), R=np.asarray(R, np.float32).reshape(3, 3), t=np.asarray(t, np.float32).reshape(3), inliers=int(inliers))


def collect_per_pair(cfg, checkpoint='', hook=None):
    """sevenscenes.py:17-66: the batch-1 loop over the test pairs -> {scene: ScenePairs}.  hook(data, R, t): tests"""
    from .builder import build_model
    from .datasets import make_loader
    from .submission import data_to_model_device
    model = build_model(cfg, checkpoint)
    recs = {}
    for data in make_loader(cfg, 'test'):
        data = data_to_model_device(data, model)
        with torch.no_grad():
            R, t = model(data)
        if hook is not None:
            hook(data, R, t)
        inl = data['inliers'] if 'inliers' in data else 0
        inl = inl.reshape(-1)[0].item() if torch.is_tensor(inl) else inl
        recs.setdefault(data['scene_id'][0], []).append(_record(
            data['pair_names'][1][0], _np(data['abs_q_0']), _np(data['abs_c_0']), _np(data['abs_q_1']), _np(data['abs_c_1']),
            data['T_0to1'][0].cpu().numpy(), _np(data['sim'])[0], R.detach().cpu().numpy(), t.detach().cpu().numpy(), inl))
    return {s: _scene_pairs(r) for s, r in recs.items()}


def collect_fused(cfg, batch_pairs=None, pipeline=None, hook=None):
    """the same pairs in batches on the device -> {scene: ScenePairs}.  hook(device batch, pipeline output): tests"""
    from . import options
    from .datasets import DevicePrefetcher, PairBatchLoader, list_scenes, usable_cpus
    options.apply_cfg(cfg)
    scenes = list_scenes(cfg, 'test')
    if pipeline is None:
        from .pipeline import FusedPosePipeline
        pipeline = FusedPosePipeline(cfg, torch.device('cuda', torch.cuda.current_device()))
    device = torch.device(pipeline.device)
    where = [(sc, i) for sc in scenes for i in range(len(sc))]                             # global id -> (scene, index)
    workers = int(cfg.HIP.LOADER_WORKERS) if int(cfg.HIP.LOADER_WORKERS) > 0 else max(2, min(32, usable_cpus()))
    loader = PairBatchLoader(scenes, int(batch_pairs or cfg.HIP.BATCH_PAIRS), pin=device.type == 'cuda', workers=workers,
                             decode=str(cfg.HIP.LOADER_DECODE), jpeg_decode=str(cfg.HIP.JPEG_DECODE),
                             depth_decode=str(cfg.HIP.DEPTH_DECODE))   # (this reader's depth maps stay on the host route)
    rows = {}
    try:
        for batch in DevicePrefetcher(loader, device):
            out = pipeline(batch)
            if hook is not None:
                hook(batch, out)
            R, t = out['R'].to(torch.float32).cpu().numpy(), out['t'].to(torch.float32).cpu().numpy()
            ninl = out['n_inliers'].cpu().numpy()
            for p, gid in enumerate(batch['global_ids'].tolist()):
                sc, i = where[gid]
                ref0, ref1 = sc.im_pairs[i]
                (c0, q0), (c1, q1) = sc.abs_poses[ref0], sc.abs_poses[ref1]
                rows[gid] = (sc.scene_id, _record(ref1, q0, c0, q1, c1, sc.relv_poses[i], sc.sim[i], R[p], t[p], ninl[p]))
    finally:
        loader.close()
    recs = {}
    for gid in sorted(rows):
        recs.setdefault(rows[gid][0], []).append(rows[gid][1])
    return {s: _scene_pairs(r) for s, r in recs.items()}


def evaluate(scenes, triang=False, ransac_thres=(15,), seed=0, lo_iters=10, thr_mult=1.414):
    """eval_pipeline_with_ransac / eval_pipeline_without_ransac over {scene: ScenePairs} -> (printed lines, {scene: result})"""
    if not triang:
        results = {s: L.eval_scene_without_ransac(sp, L.fuse_scene(sp, False)) for s, sp in scenes.items()}
        return L.report_without_ransac(results)[0], results
    lines, results = [], {}
    for n, thres in enumerate(ransac_thres):
        results = {s: L.eval_scene_with_ransac(sp, L.fuse_scene(sp, True, thres, thr_mult, lo_iters, seed)) for s, sp in scenes.items()}
        lines += L.report_with_ransac(results, thres, lo_iters, thr_mult, header=n == 0)[0]
    return lines, results


def save_outputs(output_root, scenes, lines, results):
    out = Path(output_root)
    out.mkdir(parents=True, exist_ok=True)
    (out / 'test_results.txt').write_text('\n'.join(lines) + '\n')
    raw = {'scenes': np.array(list(scenes))}
    for s, sp in scenes.items():
        raw.update(sp.arrays(f'{s}/'))
    np.savez(out / 'rawpred.npz', **raw)
    res = {'scenes': np.array(list(results))}
    for s, r in results.items():
        res[f'{s}/names'] = np.array(r['names'])
        res[f'{s}/abs_q'] = np.array([p[0] for p in r['poses']]).reshape(-1, 4); res[f'{s}/abs_t'] = np.array([p[1] for p in r['poses']]).reshape(-1, 3)
        for k in ('abs_t_errs', 'abs_r_errs', 'confidence', 'precision', 'recall', 'average_precision', 'failures'):
            res[f'{s}/{k}'] = np.asarray(r[k])
        (out / f'pose_{s}.txt').write_text(''.join(L.pose_file_lines(r)))
    np.savez(out / 'results.npz', **res)


def run(cfg, checkpoint='', fused=False, batch_pairs=None, output_root='results', triang=False, ransac_thres=(15,), pipeline=None, hook=None):
    scenes = collect_fused(cfg, batch_pairs, pipeline, hook) if fused else collect_per_pair(cfg, checkpoint, hook)
    seed = int(cfg.RANSAC.SEED) if 'RANSAC' in cfg else 0
    lines, results = evaluate(scenes, triang, ransac_thres, seed)
    for line in lines:
        print(line)
    save_outputs(output_root, scenes, lines, results)
    return lines, results


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('config', help='path to config file')
    ap.add_argument('dataset_config', help='path to dataset config file')
    ap.add_argument('--checkpoint', help='path to model checkpoint', default='')
    ap.add_argument('--test_pair_txt', '-pair', type=str, default=None)
    ap.add_argument('--output_root', '-odir', type=str, default='results/')
    ap.add_argument('--one_nn', action='store_true', help='keep only the database image of highest similarity per query')
    ap.add_argument('--triang', action='store_true', help='triangulation RANSAC over the neighbours instead of median + chordal mean')
    ap.add_argument('--triang_ransac_thres', '-rthres', metavar='%d', type=int, nargs='+', default=[15],
                    help='triangulation RANSAC inlier thresholds in degrees (default: %(default)s)')
    ap.add_argument('--fused', action='store_true', help='batched GPU route (PairBatchLoader -> FusedPosePipeline)')
    ap.add_argument('--batch_pairs', type=int, default=None)
    args = ap.parse_args(argv)
    assert (args.one_nn and args.triang) != True, 'triangulation needs more than one nearest neighbour'  # noqa: E712
    from .config import get_cfg_defaults
    cfg = get_cfg_defaults()
    cfg.merge_from_file(args.dataset_config)
    cfg.merge_from_file(args.config)
    if args.test_pair_txt:
        cfg.DATASET.PAIRS_TXT.TEST = args.test_pair_txt
    if args.one_nn:
        cfg.DATASET.PAIRS_TXT.ONE_NN = True
    return run(cfg, args.checkpoint, args.fused, args.batch_pairs, args.output_root, args.triang, args.triang_ransac_thres)


if __name__ == '__main__':
    main()
