"""A tiny ScanNet-layout tree for the reader tests, written from plain arrays: tools/gen_scannet_golden.py stores the arrays in
tests/golden/ref_scannet.npz next to what the reference's ScanNetScene made of the tree, and the tests rebuild the same files from them
(numbers are written with repr(), so the text round-trips to the same float64 bits).

    <root>/scans_test/scene%04d_%02d/sensor_data/{_info.txt, frame-%06d.color.jpg, frame-%06d.depth.pgm, frame-%06d.pose.txt}
    <root>/index/test/test.npz (name), <root>/index/scored.npz (name + score), <root>/estimated_depth.npz
"""
import os

import numpy as np


def default_params(seed=2024):
    """2 scene folders, 5 pairs; intrinsics that do not divide evenly; 16-bit depth at WIDTH x HEIGHT = 8 x 6"""
    rng = np.random.default_rng(seed)
    frames = np.array([[707, 0, 0], [707, 0, 45], [707, 0, 150], [711, 1, 15], [711, 1, 300]], np.int64)      # (scene, sub, stem)
    poses = np.zeros((len(frames), 4, 4))
    for k in range(len(frames)):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        poses[k, :3, :3] = q * np.sign(np.linalg.det(q))
        poses[k, :3, 3] = rng.normal(size=3) * 1.7
        poses[k, 3, 3] = 1.0
    scenes = np.array([[707, 0], [711, 1]], np.int64)
    k_color = np.stack([np.array([[1165.723022 + 3.1 * s, 0.013, 649.094971 - s, 0], [0, 1165.738037 - 2.7 * s, 484.765015 + s, 0],
                                  [0, 0, 1, 0], [0, 0, 0, 1]]) for s in range(2)])
    k_depth = np.stack([np.array([[574.540771 + s, 0, 322.522827, 0], [0, 577.583740, 238.558853 - s, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
                        for s in range(2)])
    names = np.array([[707, 0, 0, 45], [707, 0, 45, 150], [711, 1, 15, 300], [707, 0, 150, 0], [711, 1, 300, 15]], np.int64)
    return dict(frames=frames, poses=poses, scenes=scenes, k_color=k_color, k_depth=k_depth, names=names,
                scores=np.array([0.1, 0.5, 0.39, 0.41, 0.9]), min_overlap_score=np.float64(0.4),
                depth_u16=rng.integers(0, 65536, size=(len(frames), 6, 8)).astype(np.uint16),
                est_depth=rng.uniform(0.3, 6.0, size=(len(frames), 6, 8)),
                color_u8=rng.integers(0, 256, size=(len(frames), 10, 13, 3)).astype(np.uint8),
                width=np.int64(8), height=np.int64(6))


def _mat_line(m):
    return ' '.join(repr(float(v)) for v in np.asarray(m).reshape(-1))


def write_tree(root, p):
    """-> dict(data_root, scans, npz_root, test_npz, scored_npz, est_npz)"""
    from PIL import Image
    root = str(root)
    scans = os.path.join(root, 'scans_test')
    for s, (scene, sub) in enumerate(np.asarray(p['scenes']).tolist()):
        d = os.path.join(scans, f'scene{scene:04d}_{sub:02d}', 'sensor_data')
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, '_info.txt'), 'w') as f:
            f.write('m_versionNumber = 4\nm_colorWidth = 1296\nm_colorHeight = 968\n')
            f.write(f"m_calibrationColorIntrinsic = {_mat_line(p['k_color'][s])}\n")
            f.write(f"m_calibrationDepthIntrinsic = {_mat_line(p['k_depth'][s])}\n")
    est = {}
    for k, (scene, sub, stem) in enumerate(np.asarray(p['frames']).tolist()):
        d = os.path.join(scans, f'scene{scene:04d}_{sub:02d}', 'sensor_data')
        with open(os.path.join(d, f'frame-{stem:06}.pose.txt'), 'w') as f:
            f.write('\n'.join(' '.join(repr(float(v)) for v in row) for row in p['poses'][k]) + '\n')
        dm = np.asarray(p['depth_u16'][k])
        with open(os.path.join(d, f'frame-{stem:06}.depth.pgm'), 'wb') as f:           # binary PGM, 16 bits big-endian
            f.write(b'P5\n%d %d\n65535\n' % (dm.shape[1], dm.shape[0]) + dm.astype('>u2').tobytes())
        Image.fromarray(np.asarray(p['color_u8'][k])).save(os.path.join(d, f'frame-{stem:06}.color.jpg'), format='JPEG', quality=92)
        est[f'{scene:04d}_{sub:02d}_frame_{stem:06}'] = np.asarray(p['est_depth'][k])
    npz_root = os.path.join(root, 'index')
    os.makedirs(os.path.join(npz_root, 'test'), exist_ok=True)
    test_npz, scored_npz, est_npz = os.path.join(npz_root, 'test', 'test.npz'), os.path.join(npz_root, 'scored.npz'), os.path.join(root, 'estimated_depth.npz')
    np.savez(test_npz, name=np.asarray(p['names']))
    np.savez(scored_npz, name=np.asarray(p['names']), score=np.asarray(p['scores']))
    np.savez(est_npz, **est)
    return dict(data_root=root, scans=scans, npz_root=npz_root, test_npz=test_npz, scored_npz=scored_npz, est_npz=est_npz)


def routes_params(W=320, H=240, fW=648, fH=484, seeds=(7, 107, 211, 19, 323, 41)):
    """the tree of tests/test_gpu_scannet_routes.py as default_params-style arrays: 2 scene folders, 6 pairs, every pair two frames of its
    own.  A pair is images.synthetic_pair content at the NETWORK size (disparities that are multiples of the networks' 8-px cell, so the
    untrained matchers find real matches), enlarged to the fW x fH files the loaders then shrink again; the last pair joins views of two
    different scenes (hardly any true match).  The colour intrinsics
    are the synthetic K taken back through the reader's 1296 x 968 rescaling; depth is stored at W x H."""
    from mapfree_reloc_amd import images as IM
    from mapfree_reloc_amd.datasets import resize_bilinear_f32
    n = len(seeds)
    frames, poses, color, depth, names = [], [], [], [], []
    K = None
    for k, seed in enumerate(seeds):
        scene, sub = ((707, 0) if k < 4 else (711, 1))
        pr = IM.synthetic_pair(seed, H, W, f=260.0)
        img1 = pr["img1"] if k < n - 1 else IM.synthetic_pair(seed + 1000, H, W, f=260.0)["img1"]
        K = pr["K"]
        T = np.eye(4); T[:3, :3] = pr["R_gt"]; T[:3, 3] = pr["t_gt"]
        for j, (img, d, c2w) in enumerate(((pr["img0"], pr["depth0"], np.eye(4)), (img1, pr["depth1"], np.linalg.inv(T)))):
            g = np.clip(resize_bilinear_f32(img, (fW, fH)), 0, 1)
            rgb = np.stack([0.92 * g + 0.03, g, 0.8 * g + 0.1 * g * g], -1)
            frames.append([scene, sub, 30 * k + 15 * j]); poses.append(c2w)
            color.append(np.round(np.clip(rgb, 0, 1) * 255).astype(np.uint8)); depth.append(np.round(d * 1000).astype(np.uint16))
        names.append([scene, sub, 30 * k, 30 * k + 15])
    S = np.eye(3)
    S[0, 0] = W / 1296; S[0, 2] = W / 1296 / 2 - 0.5
    S[1, 1] = H / 968; S[1, 2] = H / 968 / 2 - 0.5
    K4 = np.eye(4); K4[:3, :3] = np.linalg.inv(S) @ K
    return dict(frames=np.array(frames, np.int64), poses=np.stack(poses), scenes=np.array([[707, 0], [711, 1]], np.int64),
                k_color=np.stack([K4, K4]), k_depth=np.stack([K4, K4]), names=np.array(names, np.int64), scores=np.ones(n),
                min_overlap_score=np.float64(0.4), depth_u16=np.stack(depth), est_depth=np.stack(depth) / 1000.0,
                color_u8=np.stack(color), width=np.int64(W), height=np.int64(H))
