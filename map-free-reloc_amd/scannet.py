"""ScanNet-1500 reader (lib/datasets/scannet.py:19-163 with the helpers of lib/datasets/utils.py:84-130): one dataset per pair-index
`*.npz` under DATASET.NPZ_ROOT/<mode>, frames under DATASET.DATA_ROOT/{scans_test | scans}/scene%04d_%02d/sensor_data/.  Reached through
`DATASET.DATA_SOURCE: 'ScanNet'` only (datasets.list_scenes / make_loader).

Sample schema (scannet.py:115-130): image0/1 [3,h,w] f32 (the dataset's order: 8-bit RGB resized, / 255), depth0/1 [h,w] f32 metres in test
mode (16-bit PGM / 1000, or the ESTIMATED_DEPTH npz's array) and empty otherwise, K_color0 = K_color1 (float64, rescaled by WIDTH / 1296
and HEIGHT / 968 -- the reference's constants, whatever the file's real size), K_depth as parsed, T_0to1 / T_1to0 f32, pair_id = index,
dataset_name, scene_id, pair_names in the `color/<stem>.jpg` spelling.

The batched loaders' route (gray_pair) hands out the MATCHER's plane, datasets.read_gray_plane(path, (W, H)): gray first, then the float
resize -- what matchers.read_image gives the offline stage (compute.py -ds Scannet) and what the reference's own two-stage flow feeds its
matchers.  Unlike MapFreeScene it serves files that are larger than the network size: on the device JPEG route the frames are decoded at
their own size and resized on the GPU (csrc/resize.hip), bit for bit the same plane.

Unpinned offline, as the rest of the image path: equality with OpenCV's own cv2.resize and with cv2.imread of a PGM (PIL reads the files here).
"""
import os

import numpy as np
import torch

from .datasets import MissingDataError, read_color_image, read_depth_plane, read_gray_plane

COLOR_W, COLOR_H = 1296, 968          # scannet.py:105-106: the size the colour intrinsics of _info.txt refer to


def read_scannet_pose(path):
    """utils.py:84-92: the file holds camera-to-world; world-to-camera is returned"""
    return np.linalg.inv(np.loadtxt(path, delimiter=' '))


def read_scannet_intrinsic(path, color=True):
    """utils.py:95-114: the 3x3 corner of the 4x4 matrix `_info.txt` lists under m_calibrationColorIntrinsic / m_calibrationDepthIntrinsic"""
    key = 'm_calibrationColorIntrinsic' if color else 'm_calibrationDepthIntrinsic'
    with open(path, 'r') as f:
        for line in f:
            if key in line:
                vals = [float(v) for v in line.split(' = ')[1].strip().split(' ')]
                return np.array(vals).reshape(4, 4)[:-1, :-1]
    raise ValueError(f'{path}: no {key}')


def scale_intrinsic(K, scale_x, scale_y):
    """utils.py:117-130 as the reference evaluates it: a float64 transform matrix times K (the matrix product's bits, not the
    algebraically equal closed form of datasets.correct_intrinsic_scale)"""
    T = np.eye(3)
    T[0, 0] = scale_x; T[0, 2] = scale_x / 2 - 0.5
    T[1, 1] = scale_y; T[1, 2] = scale_y / 2 - 0.5
    return T @ K


def pair_image_paths(npz_path, root_dir):
    """etc/feature_matching_baselines/utils.py:5-17 (load_scannet_imgpaths): the colour frames of every row of `name`, in file order"""
    out = []
    for scene, sub, s0, s1 in np.load(npz_path)['name']:
        d = os.path.join(str(root_dir), f'scene{scene:04d}_{sub:02d}', 'sensor_data')
        out.append((os.path.join(d, f'frame-{s0:06}.color.jpg'), os.path.join(d, f'frame-{s1:06}.color.jpg')))
    return out


class ScanNetScene:
    """pairs of one index npz (scannet.py:19-132).  Also the scene protocol of datasets.PairBatchLoader: len, [index] -> sample, scene_id
    (the npz's stem), scene_root (the scans directory), has_gray_pair / gray_pair, shared_reference = False, and batch_layout(): the planes'
    (H, W, has depth), so that the loader sizes its buffers without decoding a generic sample."""

    has_gray_pair = True
    shared_reference = False

    def __init__(self, root_dir, npz_path, mode='train', min_overlap_score=0.4, resize=(640, 480), estimated_depth=None):
        self.root_dir, self.npz_path, self.mode = str(root_dir), str(npz_path), mode
        self.resize = (int(resize[0]), int(resize[1]))
        self.scene_root = self.root_dir
        self.scene_id = os.path.splitext(os.path.basename(self.npz_path))[0]
        with np.load(self.npz_path) as data:
            self.data_names = data['name']
            # scannet.py:47 reads `mode not in ['val' or 'test']`: the list is ['val'], so the overlap filter also applies in TEST mode
            # whenever the npz carries a `score` column (the released test.npz has none).  Kept as it is.
            if 'score' in data.keys() and mode not in ['val']:
                self.data_names = self.data_names[data['score'] > min_overlap_score]
        self.depthmaps = np.load(estimated_depth) if estimated_depth is not None else None      # scannet.py:55
        self._K = {}

    def __len__(self):
        return len(self.data_names)

    def _row(self, idx):
        scene, sub, s0, s1 = self.data_names[idx]
        return f'scene{scene:04d}_{sub:02d}', s0, s1

    def _path(self, scene_name, stem, what):
        return os.path.join(self.root_dir, scene_name, 'sensor_data', f'frame-{stem:06}.{what}')

    def pair_names(self, idx):
        scene_name, s0, s1 = self._row(idx)
        return (os.path.join(scene_name, 'color', f'{s0}.jpg'), os.path.join(scene_name, 'color', f'{s1}.jpg'))

    def pair_name(self, idx):
        return self.pair_names(idx)[1]

    def intrinsics(self, scene_name):
        """(K_color float64 rescaled to `resize`, K_depth as parsed) of a scene folder, read once"""
        hit = self._K.get(scene_name)
        if hit is None:
            info = os.path.join(self.root_dir, scene_name, 'sensor_data', '_info.txt')
            Kc = scale_intrinsic(read_scannet_intrinsic(info, color=True), self.resize[0] / COLOR_W, self.resize[1] / COLOR_H)
            hit = self._K[scene_name] = (Kc, read_scannet_intrinsic(info, color=False))
        return hit

    def rel_pose(self, scene_name, s0, s1):
        """scannet.py:66-70: w2c(1) @ inv(w2c(0)) -- the product the reference forms from the two inverted files"""
        p0 = read_scannet_pose(self._path(scene_name, s0, 'pose.txt'))
        p1 = read_scannet_pose(self._path(scene_name, s1, 'pose.txt'))
        return np.matmul(p1, np.linalg.inv(p0))

    def has_depth(self):
        return self.mode in ['test']

    def batch_layout(self):
        return self.resize[1], self.resize[0], self.has_depth()

    def _depth(self, scene_name, stem, out=None):
        """scannet.py:85-98 as a numpy plane [H,W] f32 (into `out` when given).  A depth map that is not HEIGHT x WIDTH is an error: the
        reference stores them at the network size and nothing resizes depth"""
        want = (self.resize[1], self.resize[0])
        if self.depthmaps is None:
            path = self._path(scene_name, stem, 'depth.pgm')
            from PIL import Image
            with Image.open(path) as im:
                size = (im.size[1], im.size[0])
            if out is not None and size != want:
                raise ValueError(f'{path}: depth map is {size[1]}x{size[0]}, DATASET.WIDTH x HEIGHT is {want[1]}x{want[0]}')
            return read_depth_plane(path, out)
        d = self.depthmaps[f'{scene_name[5:]}_frame_{stem:06}'].astype(np.float32)
        if out is None:
            return d
        if d.shape != want:
            raise ValueError(f'{self.npz_path}: estimated depth of {scene_name} frame {stem} is {d.shape[1]}x{d.shape[0]}, '
                             f'DATASET.WIDTH x HEIGHT is {want[1]}x{want[0]}')
        out[...] = d
        return out

    def gray_pair(self, index, want_ref=True, out=None, readers=None):
        """datasets.MapFreeScene.gray_pair's contract: (gray0, depth0, gray1, depth1, K0, K1, pair_id, names) with the planes written into
        out = (g0, d0, g1, d1) when given.  The gray planes are read_gray_plane(path, (W, H)) whatever the files' size (never None);
        readers (the device JPEG route) take the resize so that their host fallback gives the same plane."""
        scene_name, s0, s1 = self._row(index)
        og0, od0, og1, od1 = out if out is not None else (None, None, None, None)
        r0, r1 = readers if readers is not None else (None, None)

        def gray(stem, og, reader, want):
            if not want:
                return None
            path = self._path(scene_name, stem, 'color.jpg')
            if reader is not None:
                return reader(path, og, self.resize) if og is not None else None
            return read_gray_plane(path, self.resize, og)
        g0, g1 = gray(s0, og0, r0, want_ref), gray(s1, og1, r1, True)
        d0 = d1 = None
        if self.has_depth():
            d0, d1 = self._depth(scene_name, s0, od0), self._depth(scene_name, s1, od1)
        Kc, _ = self.intrinsics(scene_name)
        return g0, d0, g1, d1, Kc.copy(), Kc.copy(), int(index), self.pair_names(index)

    def __getitem__(self, idx):
        scene_name, s0, s1 = self._row(idx)
        image0 = read_color_image(self._path(scene_name, s0, 'color.jpg'), self.resize)
        image1 = read_color_image(self._path(scene_name, s1, 'color.jpg'), self.resize)
        if self.has_depth():
            depth0, depth1 = torch.from_numpy(self._depth(scene_name, s0)), torch.from_numpy(self._depth(scene_name, s1))
        else:
            depth0 = depth1 = torch.tensor([])
        Kc, Kd = self.intrinsics(scene_name)
        K_color = torch.from_numpy(Kc.copy())
        T_0to1 = torch.tensor(self.rel_pose(scene_name, s0, s1), dtype=torch.float32)
        return {'image0': image0, 'depth0': depth0, 'image1': image1, 'depth1': depth1, 'T_0to1': T_0to1, 'T_1to0': T_0to1.inverse(),
                'K_color0': K_color, 'K_color1': K_color, 'K_depth': torch.from_numpy(Kd.copy()), 'dataset_name': 'ScanNet',
                'scene_id': scene_name, 'pair_id': int(idx), 'pair_names': self.pair_names(idx)}


def list_scannet_scenes(cfg, mode):
    """scannet.py:135-163 (ScanNetDataset): one ScanNetScene per npz of NPZ_ROOT/<mode>; val / train pairs share one npz per scene, the
    1500 test pairs come in a single test.npz.  (The reference concatenates them in os.listdir order; sorted here, so that pair order --
    and with it every global id -- does not depend on the file system.)"""
    assert mode in ('train', 'val', 'test'), 'Invalid dataset mode'
    root, npz_root = cfg.DATASET.DATA_ROOT, cfg.DATASET.NPZ_ROOT
    if not (root and npz_root and os.path.isdir(os.path.join(str(npz_root), mode))):
        raise MissingDataError(f"DATASET.NPZ_ROOT/{mode} = {os.path.join(str(npz_root), mode)!r} does not exist (DATA_SOURCE 'ScanNet')")
    root_dir = os.path.join(str(root), 'scans_test' if mode == 'test' else 'scans')
    npz_dir = os.path.join(str(npz_root), mode)
    return [ScanNetScene(root_dir, os.path.join(npz_dir, f), mode, cfg.DATASET.MIN_OVERLAP_SCORE, (cfg.DATASET.WIDTH, cfg.DATASET.HEIGHT),
                         cfg.DATASET.ESTIMATED_DEPTH) for f in sorted(os.listdir(npz_dir)) if f[-3:] == 'npz']
