"""Offline matcher stage with the reference's CLI and output files
(etc/feature_matching_baselines/compute.py:13-44, 72-86): for every scene of the Map-free test+val
splits, match seq0/frame_00000.jpg against EVERY seq1 frame listed in poses.txt (not subsampled,
quirk Q4) and write `correspondences_{matcher}.npz` (key `correspondences`, NaN-padded
[Npairs, maxN, 4] float64) into the scene directory.

    python -m mapfree_reloc_amd.compute -ds Mapfree -m SG [--outdoor] [--data_root data/mapfree]
    python -m mapfree_reloc_amd.compute -ds Mapfree -m SIFT --sift-detector hip      (SIFT on the GPU, no OpenCV)
    python -m mapfree_reloc_amd.compute -ds Mapfree -m LoFTR --loftr-match-type sinkhorn
        (the optimal-transport matcher of the *_ot.ckpt weights; writes correspondences_LoFTR_OT.npz, never the dual-softmax file's name)

-ds Scannet (compute.py:88-100): the pairs of --pair_npz in the order of its `name` rows (utils.py:5-17), frames under --data_root, at
640 x 480, all into ONE `correspondences_{matcher}_scannet_test.npz` in --output_dir (the reference hard-codes ../../data/scannet_misc).

    python -m mapfree_reloc_amd.compute -ds Scannet -m SG --pair_npz data/scannet_indices/scene_data/test/test.npz \
        --data_root data/scannet/scans_test --output_dir data/scannet_misc
"""
import argparse
from pathlib import Path

from . import wire
from .matchers import MATCHERS


def output_tag(matcher, loftr_match_type='dual_softmax'):
    """file-name tag of a matcher's correspondences: the reference's names, and LoFTR_OT for the optimal-transport LoFTR stage"""
    return 'LoFTR_OT' if matcher == 'LoFTR' and loftr_match_type == 'sinkhorn' else matcher


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--dataset', '-ds', type=str, default='Mapfree', choices=['Mapfree', 'Scannet'])
    ap.add_argument('--matcher', '-m', type=str, default='SG', choices=MATCHERS.keys())
    ap.add_argument('--scenes', '-sc', type=str, nargs='*', default=None)
    ap.add_argument('--outdoor', action='store_true')
    ap.add_argument('--data_root', type=Path, default=None)       # default: data/mapfree/ (Mapfree), data/scannet/scans_test (Scannet)
    ap.add_argument('--pair_npz', type=Path, default=Path('data/scannet_indices/scene_data/test/test.npz'))       # -ds Scannet
    ap.add_argument('--output_dir', type=Path, default=Path('data/scannet_misc'))                                 # -ds Scannet
    ap.add_argument('--resize', type=int, nargs=2, metavar=('W', 'H'), default=None)     # new: another matcher input size than the dataset's (compute.py:40-42 hard-codes it)
    ap.add_argument('--sift-detector', type=str, default='opencv', choices=['opencv', 'hip'])     # new: -m SIFT's keypoint detector
    ap.add_argument('--loftr-match-type', type=str, default='dual_softmax', choices=['dual_softmax', 'sinkhorn'])     # new: -m LoFTR's coarse matching
    args = ap.parse_args(argv)
    scannet = args.dataset == 'Scannet'
    if args.data_root is None:
        args.data_root = Path('data/scannet/scans_test') if scannet else Path('data/mapfree/')
    resize = (640, 480) if scannet else (540, 720)                          # compute.py:40-42
    if args.resize is not None:
        resize = tuple(args.resize)
    if args.matcher == 'SIFT':
        matcher = MATCHERS['SIFT'](resize, args.outdoor, detector='hip' if args.sift_detector == 'hip' else None)
    elif args.matcher == 'LoFTR':
        matcher = MATCHERS['LoFTR'](resize, args.outdoor, match_type=args.loftr_match_type)
    else:
        matcher = MATCHERS[args.matcher](resize, args.outdoor)
    if scannet:
        from .scannet import pair_image_paths
        pts = [matcher.match(pair) for pair in pair_image_paths(args.pair_npz, args.data_root)]
        args.output_dir.mkdir(parents=True, exist_ok=True)
        out = args.output_dir / f'correspondences_{output_tag(args.matcher, args.loftr_match_type)}_scannet_test.npz'
        wire.save_correspondences(out, pts)
        print(f'Finished Scannet: {len(pts)} pairs -> {out}')
        return
    scenes = [f for split in ('test', 'val') if (args.data_root / split).is_dir()
              for f in sorted((args.data_root / split).iterdir()) if f.is_dir()]
    if args.scenes:
        scenes = [s for s in scenes if s.name in args.scenes]
    for scene_dir in scenes:
        qs = wire.parse_mapfree_query_frames(scene_dir / 'poses.txt')
        pts = [matcher.match((str(scene_dir / 'seq0' / 'frame_00000.jpg'), str(scene_dir / q))) for q in qs]
        wire.save_correspondences(scene_dir / f'correspondences_{output_tag(args.matcher, args.loftr_match_type)}.npz', pts)
        print(f'Finished {scene_dir.name}: {len(pts)} pairs')


if __name__ == '__main__':
    main()
