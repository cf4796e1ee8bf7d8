"""7Scenes reader (lib/datasets/sevenscenes.py:14-196): one dataset per scene folder, its (database, query) pairs listed by the pair file
DATASET.PAIRS_TXT.<mode> inside the folder, absolute poses from dataset_test.txt / dataset_train.txt.  Reached through
`DATASET.DATA_SOURCE: '7Scenes'` only (datasets.list_scenes / make_loader).

Sample schema (sevenscenes.py:138-157): image0/1 [3,h,w] f32 (8-bit RGB resized, / 255), depth0/1 [H,W] f32 metres at the FILE's size
(the colour path with `.color.` -> `.depth.` or `.depth.<ESTIMATED_DEPTH>.`; never resized), T_0to1 f32 (database -> query), abs_q_0/1
(wxyz) and abs_c_0/1 f32 (image 0 is the database image, image 1 the query), sim, K_color0 = K_color1 = K_depth (f = 525, centre
(320, 240) as float32, rescaled by WIDTH / 640 and HEIGHT / 480: float64 after the product), dataset_name, scene_id, scene_root,
pair_id (the row of the pair file, also after the ONE_NN filter), pair_names.

The batched loaders take the generic per-sample route (no gray_pair).
"""
import glob
import os

import numpy as np
import torch

from .datasets import MissingDataError, read_color_image, read_depth_image
from .scannet import scale_intrinsic


def quat_wxyz_to_matrix(q):
    """scipy Rotation.from_quat(q[[1, 2, 3, 0]]).as_matrix() (sevenscenes.py:63-64): the float32 quaternion is normalised in float64"""
    from scipy.spatial.transform import Rotation
    return Rotation.from_quat(np.asarray(q)[[1, 2, 3, 0]]).as_matrix()


def parse_relv_pose_txt(fpath):
    """sevenscenes.py:48-74: `image1 image2 sim w p q r x y z ...` -> (pairs, 4x4 float64 poses, sims)"""
    im_pairs, relv_poses, sim = [], [], []
    with open(fpath) as f:
        for line in f:
            cur = line.split()
            im_pairs.append((cur[0], cur[1]))
            sim.append(float(cur[2]))
            q = np.array([float(i) for i in cur[3:7]], dtype=np.float32)
            t = np.array([float(i) for i in cur[7:10]], dtype=np.float32)
            T = np.eye(4)
            T[:3, :3] = quat_wxyz_to_matrix(q)
            T[:3, -1] = t.ravel()
            relv_poses.append(T)
    return im_pairs, relv_poses, sim


def parse_abs_pose_txt(fpath):
    """sevenscenes.py:76-91: 3 header lines, then `image x y z w p q r` split on ONE space -> {image: (c f32, q f32 wxyz)}"""
    pose_dict = {}
    with open(fpath) as f:
        for line in f.readlines()[3::]:
            cur = line.split(' ')
            pose_dict[cur[0]] = (np.array([float(v) for v in cur[1:4]], dtype=np.float32),
                                 np.array([float(v) for v in cur[4:8]], dtype=np.float32))
    return pose_dict


def one_nn_rows(im_pairs, sim):
    """sevenscenes.py:93-112: per query the row of highest similarity -- an EQUAL similarity replaces the kept row -- in the order the
    queries first appear (the dict's insertion order), not by ascending row"""
    kept_idx, kept_sim = {}, {}
    for i, ((_, query), s) in enumerate(zip(im_pairs, sim)):
        if query in kept_sim and s < kept_sim[query]:
            continue
        kept_idx[query] = i
        kept_sim[query] = s
    return list(kept_idx.values())


class SevenScenesScene:
    """pairs of one scene folder (sevenscenes.py:14-162, the reference's SceneDataset); also the scene protocol of the batched loaders:
    len, [index] -> sample, scene_id, scene_root"""

    has_gray_pair = False
    shared_reference = False

    def __init__(self, scene_root, pair_txt, resize, one_nn=False, estimated_depth=None):
        self.scene_root = str(scene_root)
        self.scene_id = self.scene_root.split('/')[-1]
        self.resize = (int(resize[0]), int(resize[1]))
        self.estimated_depth = estimated_depth
        self.im_pairs, self.relv_poses, self.sim = parse_relv_pose_txt(os.path.join(self.scene_root, pair_txt))
        self.original_idxs = list(range(len(self.im_pairs)))
        if one_nn:
            keep = one_nn_rows(self.im_pairs, self.sim)
            self.im_pairs = [self.im_pairs[i] for i in keep]
            self.relv_poses = [self.relv_poses[i] for i in keep]
            self.sim = [self.sim[i] for i in keep]
            self.original_idxs = keep
        self.abs_poses = parse_abs_pose_txt(os.path.join(self.scene_root, 'dataset_test.txt'))
        self.abs_poses.update(parse_abs_pose_txt(os.path.join(self.scene_root, 'dataset_train.txt')))
        K = np.array([[525, 0, 320], [0, 525, 240], [0, 0, 1]], dtype=np.float32)
        self.K = scale_intrinsic(K, self.resize[0] / 640, self.resize[1] / 480)

    def __len__(self):
        return len(self.im_pairs)

    def pair_name(self, index):
        return self.im_pairs[index][1]

    def __getitem__(self, index):
        ref0, ref1 = self.im_pairs[index]
        p0, p1 = os.path.join(self.scene_root, ref0), os.path.join(self.scene_root, ref1)
        suffix = '.depth.' if self.estimated_depth is None else f'.depth.{self.estimated_depth}.'
        c0, q0 = self.abs_poses[ref0]
        c1, q1 = self.abs_poses[ref1]
        return {'image0': read_color_image(p0, self.resize), 'depth0': read_depth_image(p0.replace('.color.', suffix)),
                'image1': read_color_image(p1, self.resize), 'depth1': read_depth_image(p1.replace('.color.', suffix)),
                'T_0to1': torch.tensor(self.relv_poses[index], dtype=torch.float32),
                'abs_q_0': q0, 'abs_c_0': c0, 'abs_q_1': q1, 'abs_c_1': c1, 'sim': self.sim[index],
                'K_color0': self.K.copy(), 'K_color1': self.K.copy(), 'K_depth': self.K.copy(),
                'dataset_name': '7Scenes', 'scene_id': self.scene_id, 'scene_root': self.scene_root,
                'pair_id': self.original_idxs[index], 'pair_names': self.im_pairs[index]}


def list_sevenscenes_scenes(cfg, mode):
    """sevenscenes.py:165-196 (SevenScenesDataset): DATASET.SCENES, or every folder of DATA_ROOT that holds the pair file, sorted"""
    assert mode in ('train', 'val', 'test'), 'Invalid dataset mode'
    root = cfg.DATASET.DATA_ROOT
    pair_txt = {'train': cfg.DATASET.PAIRS_TXT.TRAIN, 'val': cfg.DATASET.PAIRS_TXT.VAL, 'test': cfg.DATASET.PAIRS_TXT.TEST}[mode]
    if not (root and os.path.isdir(str(root))):
        raise MissingDataError(f"DATASET.DATA_ROOT = {root!r} does not exist (DATA_SOURCE '7Scenes')")
    scenes = cfg.DATASET.SCENES
    if scenes is None:
        scenes = sorted(p.split('/')[-2] for p in glob.iglob('{}/*/{}'.format(root, pair_txt)))
    return [SevenScenesScene(os.path.join(str(root), s), pair_txt, (cfg.DATASET.WIDTH, cfg.DATASET.HEIGHT), bool(cfg.DATASET.PAIRS_TXT.ONE_NN),
                             cfg.DATASET.ESTIMATED_DEPTH) for s in scenes]
