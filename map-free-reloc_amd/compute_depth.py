"""Offline monocular-depth stage: writes the depth maps that the readers load (`DATASET.ESTIMATED_DEPTH`), as compute.py writes the correspondences.

    python -m mapfree_reloc_amd.compute_depth -ds Mapfree --data_root data/mapfree --name dptkitti [--scenes s00460 ...] [--batch 8]
    python -m mapfree_reloc_amd.compute_depth -ds 7Scenes --data_root data/sevenscenes --name dptnyu

Every frame of a scene goes through the configured depth network (DPT.NETWORK: DPT-Hybrid, nets/dpt.py, or Depth Anything V2, nets/depth_anything.py) in batches, at the frame's own size, and the millimetre plane the device
rounds (csrc/dpt.hip mfr_dpt_head_tail) is written beside the frame as a 16-bit gray PNG, exactly where the readers look:
    Map-free   seqX/frame_00012.jpg        -> seqX/frame_00012.<name>.png            (datasets.MapFreeScene)
    7Scenes    seq-01/frame-000012.color.png -> seq-01/frame-000012.depth.<name>.png (sevenscenes.SevenScenesScene)
    python -m mapfree_reloc_amd.compute_depth -ds Scannet --data_root data/scannet/scans_test --pair_npz data/scannet_indices/scene_data/test/test.npz \
        --name data/scannet_misc/dpt_depth.npz [--resize 640 480]
Files that exist are skipped; a file appears under its name only when it is complete (written under a temporary name, then renamed).

ScanNet's reader (scannet.ScanNetScene, DATASET.ESTIMATED_DEPTH) takes ONE .npz of float maps in metres at DATASET.WIDTH x HEIGHT, keyed
`<scene>_<sub>_frame_<stem>`: --name is that file's path, the frames are those of the pairs in --pair_npz, and each map is the network's output resized to
--resize (the metres the millimetre plane stands for under DPT.QUANTIZE_MM, float32).

The maps are computed from the FILE's pixels.  The online route (DPT.SOURCE 'online') computes them from the loader's image, which is the file resized to
DATASET.WIDTH x HEIGHT: the two routes hand the solver the same bits where that is the file's own size (Map-free's 540 x 720 frames and default), not otherwise."""
import argparse
import os
from pathlib import Path

import numpy as np


def depth_path(dataset, frame_path, name):
    """where the reader of `dataset` looks for the depth map `name` of a frame"""
    p = str(frame_path)
    if dataset == 'Mapfree':
        assert p.endswith('.jpg'), p
        return p.replace('.jpg', f'.{name}.png')
    assert '.color.' in p, p
    return p.replace('.color.', f'.depth.{name}.')


def write_depth_png(path, mm):
    """mm [H, W] uint16 millimetres -> a 16-bit gray PNG at `path`, complete or absent: written under a temporary name in the same directory, then renamed"""
    from PIL import Image
    mm = np.ascontiguousarray(mm)
    assert mm.dtype == np.uint16 and mm.ndim == 2
    tmp = f'{path}.tmp{os.getpid()}'
    try:
        Image.fromarray(mm).save(tmp, format='PNG')
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def scene_frames(dataset, scene_dir):
    """the frame files of one scene directory, sorted"""
    pat = 'seq*/frame_*.jpg' if dataset == 'Mapfree' else 'seq-*/frame-*.color.png'
    return sorted(str(p) for p in Path(scene_dir).glob(pat))


def list_scene_dirs(dataset, data_root, scenes=None):
    root = Path(data_root)
    if dataset == 'Mapfree':
        dirs = [f for split in ('train', 'val', 'test') if (root / split).is_dir() for f in sorted((root / split).iterdir()) if f.is_dir()]
    else:
        dirs = [f for f in sorted(root.iterdir()) if f.is_dir()]
    return [d for d in dirs if not scenes or d.name in scenes]


def run_scene(estimator, dataset, scene_dir, name, batch=8):
    """-> (written, skipped).  Frames of one size share a batch; the images go to the device as the decoded bytes"""
    import torch
    from PIL import Image
    todo = [(f, depth_path(dataset, f, name)) for f in scene_frames(dataset, scene_dir)]
    skipped = sum(os.path.exists(o) for _, o in todo)
    todo = [(f, o) for f, o in todo if not os.path.exists(o)]
    written, i = 0, 0
    while i < len(todo):
        imgs, outs = [], []
        while i < len(todo) and len(imgs) < batch:
            a = np.asarray(Image.open(todo[i][0]).convert('RGB'))
            if imgs and a.shape != imgs[0].shape:
                break
            imgs.append(a); outs.append(todo[i][1]); i += 1
        _, mm = estimator(torch.from_numpy(np.stack(imgs)))
        mm = mm.cpu().numpy()
        for k, o in enumerate(outs):
            write_depth_png(o, mm[k])
            written += 1
    return written, skipped


def scannet_key(scene, sub, stem):
    """the key scannet.ScanNetScene._depth looks a frame's map up under"""
    return f'{int(scene):04d}_{int(sub):02d}_frame_{int(stem):06}'


def scannet_frames(pair_npz):
    """the (scene, sub, stem) of every frame the pairs of an index npz name, each once, sorted"""
    rows = np.load(pair_npz)['name']
    return sorted({(int(sc), int(sub), int(st)) for sc, sub, s0, s1 in rows for st in (s0, s1)})


def write_depth_npz(path, maps):
    """{key: float32 [H, W] metres} -> one .npz at `path`, complete or absent (temporary name in the same directory, then renamed)"""
    assert maps and all(m.dtype == np.float32 and m.ndim == 2 for m in maps.values())
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    tmp = f'{path}.tmp{os.getpid()}.npz'                                   # np.savez keeps a name that ends in .npz
    try:
        np.savez(tmp, **maps)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def run_scannet(estimator, data_root, pair_npz, out_path, resize=(640, 480), batch=8):
    """-> (written, skipped) maps.  An existing file is left as it is"""
    import torch
    from PIL import Image
    frames = scannet_frames(pair_npz)
    if os.path.exists(out_path):
        return 0, len(frames)
    out_hw = (int(resize[1]), int(resize[0]))
    path = lambda f: os.path.join(str(data_root), f'scene{f[0]:04d}_{f[1]:02d}', 'sensor_data', f'frame-{f[2]:06}.color.jpg')
    maps, i = {}, 0
    while i < len(frames):
        imgs, keys = [], []
        while i < len(frames) and len(imgs) < batch:
            a = np.asarray(Image.open(path(frames[i])).convert('RGB'))
            if imgs and a.shape != imgs[0].shape:
                break
            imgs.append(a); keys.append(scannet_key(*frames[i])); i += 1
        m = estimator.metres(torch.from_numpy(np.stack(imgs)), out_hw).cpu().numpy()
        for k, key in enumerate(keys):
            maps[key] = np.ascontiguousarray(m[k], dtype=np.float32)
    write_depth_npz(out_path, maps)
    return len(maps), 0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--dataset', '-ds', type=str, default='Mapfree', choices=['Mapfree', 'Scannet', '7Scenes'])
    ap.add_argument('--data_root', type=Path, required=True)
    ap.add_argument('--name', type=str, required=True)                     # the suffix DATASET.ESTIMATED_DEPTH names (-ds Scannet: the .npz it names)
    ap.add_argument('--pair_npz', type=Path, default=Path('data/scannet_indices/scene_data/test/test.npz'))       # -ds Scannet
    ap.add_argument('--resize', type=int, nargs=2, metavar=('W', 'H'), default=(640, 480))                        # -ds Scannet: DATASET.WIDTH, HEIGHT
    ap.add_argument('--scenes', '-sc', type=str, nargs='*', default=None)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--config', type=Path, default=None)                  # a yaml merged over the defaults (the DPT node: weights, sizes, output convention)
    ap.add_argument('opts', nargs='*', default=[])                        # KEY VALUE pairs merged last, e.g. DPT.WEIGHTS dpt_hybrid_kitti.pth
    args = ap.parse_args(argv)
    from .config import get_cfg_defaults
    from .nets.dpt import DepthEstimator
    cfg = get_cfg_defaults()
    if args.config is not None:
        cfg.merge_from_file(str(args.config))
    cfg.merge_from_list(list(args.opts))
    est = DepthEstimator(cfg)
    if args.dataset == 'Scannet':
        w, sk = run_scannet(est, args.data_root, args.pair_npz, args.name, tuple(args.resize), args.batch)
        print(f'Finished Scannet: {w} depth maps written to {args.name}, {sk} already there')
        return
    for scene_dir in list_scene_dirs(args.dataset, args.data_root, args.scenes):
        w, s = run_scene(est, args.dataset, scene_dir, args.name, args.batch)
        print(f'Finished {scene_dir.name}: {w} depth maps written, {s} already there')


if __name__ == '__main__':
    main()
