"""Tiny 7Scenes-layout trees for the reader and benchmark tests (test helper, not a test module), written from plain arrays:
tools/gen_sevenscenes_golden.py stores default_params() in tests/golden/ref_sevenscenes.npz next to what the reference's SceneDataset made
of the tree, and the tests rebuild the same files from them (numbers are written with repr(), so the text parses back to the same values).

    <root>/<scene>/<pair file>                      `db_image query_image sim qw qx qy qz tx ty tz`
    <root>/<scene>/dataset_train.txt, dataset_test.txt   3 header lines, then `image x y z qw qx qy qz`
    <root>/<scene>/seq-01/frame-%06d.color.png, .depth.png (16-bit, millimetres), .depth.est.png
"""
import os

import numpy as np

PAIR_TXT = 'test_pairs.txt'


def _rot(rv):
    from scipy.spatial.transform import Rotation
    return Rotation.from_rotvec(rv).as_matrix()


def _quat_wxyz(R):
    from scipy.spatial.transform import Rotation
    q = Rotation.from_matrix(R).as_quat()[[3, 0, 1, 2]]
    return q if q[0] >= 0 else -q


def default_params(seed=2025):
    """2 scenes, 4 queries x 3 neighbours with tied similarities; the first scene's first query comes back in a last row whose similarity
    ties its best one (ONE_NN then keeps that row, and lists the query first); WIDTH x HEIGHT = 8 x 6, colour files 13 x 10, depth 7 x 5"""
    rng = np.random.default_rng(seed)
    scenes = ['chess', 'fire']
    img_scene, img_name, img_test, pairs = [], [], [], []
    for s in range(2):
        for j in range(6):                                   # database images 0..5, queries 6, 7
            img_scene.append(s); img_name.append(f'seq-01/frame-{j:06d}.color.png'); img_test.append(False)
        for j in (6, 7):
            img_scene.append(s); img_name.append(f'seq-02/frame-{j:06d}.color.png'); img_test.append(True)
        sims = [[0.5, 0.75, 0.75], [0.9, 0.9, 0.25]] if s == 0 else [[0.125, 0.125, 0.125], [0.3, 0.6, 0.45]]
        for qi, j in enumerate((6, 7)):
            for n in range(3):
                pairs.append((s, f'seq-01/frame-{3 * qi + n:06d}.color.png', f'seq-02/frame-{j:06d}.color.png', sims[qi][n]))
        if s == 0:
            pairs.append((s, 'seq-01/frame-000004.color.png', 'seq-02/frame-000006.color.png', 0.75))
    M, N = len(img_name), len(pairs)
    img_q = rng.normal(size=(M, 4)); img_q /= np.linalg.norm(img_q, axis=1, keepdims=True)
    pair_q = rng.normal(size=(N, 4)) * 1.3                    # not unit: the reader normalises through scipy
    return dict(scenes=np.array(scenes), img_scene=np.array(img_scene, np.int64), img_name=np.array(img_name), img_test=np.array(img_test),
                img_c=rng.normal(size=(M, 3)) * 1.5, img_q=img_q,
                pair_scene=np.array([p[0] for p in pairs], np.int64), pair_db=np.array([p[1] for p in pairs]),
                pair_query=np.array([p[2] for p in pairs]), pair_sim=np.array([p[3] for p in pairs]), pair_q=pair_q,
                pair_t=rng.normal(size=(N, 3)),
                depth_u16=rng.integers(0, 65536, size=(M, 5, 7)).astype(np.uint16), est_u16=rng.integers(0, 65536, size=(M, 5, 7)).astype(np.uint16),
                color_u8=rng.integers(0, 256, size=(M, 10, 13, 3)).astype(np.uint8), width=np.int64(8), height=np.int64(6))


def _nums(v):
    return ' '.join(repr(float(x)) for x in np.asarray(v).reshape(-1))


def write_tree(root, p, pair_txt=PAIR_TXT):
    """-> the data root (DATASET.DATA_ROOT)"""
    from PIL import Image
    root = str(root)
    scenes = [str(s) for s in np.asarray(p['scenes']).tolist()]
    for s, name in enumerate(scenes):
        d = os.path.join(root, name)
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, pair_txt), 'w') as f:
            for k in np.nonzero(np.asarray(p['pair_scene']) == s)[0]:
                f.write(f"{p['pair_db'][k]} {p['pair_query'][k]} {float(p['pair_sim'][k])!r} {_nums(p['pair_q'][k])} {_nums(p['pair_t'][k])}\n")
        for test, fname in ((False, 'dataset_train.txt'), (True, 'dataset_test.txt')):
            with open(os.path.join(d, fname), 'w') as f:
                f.write(f'Visual Landmark Dataset V1\nImageFile, Camera Position [X Y Z W P Q R]\n\n')
                for k in np.nonzero((np.asarray(p['img_scene']) == s) & (np.asarray(p['img_test']) == test))[0]:
                    f.write(f"{p['img_name'][k]} {_nums(p['img_c'][k])} {_nums(p['img_q'][k])}\n")
    for k in range(len(p['img_name'])):
        path = os.path.join(root, scenes[int(p['img_scene'][k])], str(p['img_name'][k]))
        os.makedirs(os.path.dirname(path), exist_ok=True)
        Image.fromarray(np.asarray(p['color_u8'][k])).save(path)
        Image.fromarray(np.asarray(p['depth_u16'][k], np.uint16)).save(path.replace('.color.', '.depth.'))
        if 'est_u16' in p:
            Image.fromarray(np.asarray(p['est_u16'][k], np.uint16)).save(path.replace('.color.', '.depth.est.'))
    return root


def reader_K(W, H):
    """the reader's intrinsics (f = 525, centre (320, 240) at 640 x 480, rescaled to W x H)"""
    T = np.eye(3)
    T[0, 0] = W / 640; T[0, 2] = W / 640 / 2 - 0.5
    T[1, 1] = H / 480; T[1, 2] = H / 480 / 2 - 0.5
    return T @ np.array([[525, 0, 320], [0, 525, 240], [0, 0, 1]], dtype=np.float32)


def geometry_params(W=320, H=240, seed=77, n_pts=160):
    """a tree with real geometry for the end-to-end tests, in the style of tests/solver_scenes.py: every (database, query) pair has n_pts scene
    points seen by both views (30 % of them replaced by outliers, 0.3 px noise), their depth written into the database image's depth
    map, and the relative pose of the pair file is the one that moves them.  Scene 'chess': 3 queries x 3 neighbours.  Scene 'fire':
    2 queries x 4 neighbours, one query with a single neighbour, one query whose only pair has no correspondence at all (no pose: a query
    without pairs).  -> (default_params-style dict, {scene: list of [n,4] correspondence rows in pair-file order})"""
    rng = np.random.default_rng(seed)
    K = reader_K(W, H)
    scenes = ['chess', 'fire']
    layout = [[3, 3, 3], [4, 4, 1, 1]]
    img_scene, img_name, img_test, img_c, img_q, depth, pairs, pair_q, pair_t = [], [], [], [], [], [], [], [], []
    corr = {s: [] for s in scenes}
    for s, ks in enumerate(layout):
        n_db = 0
        for qi, k in enumerate(ks):
            rq, cq = _rot(rng.normal(size=3) * 0.4), rng.uniform(-1.5, 1.5, 3)              # world -> camera rotation, centre
            qname = f'seq-02/frame-{qi:06d}.color.png'
            img_scene.append(s); img_name.append(qname); img_test.append(True); img_c.append(cq); img_q.append(_quat_wxyz(rq))
            depth.append(np.full((H, W), 5000, np.uint16))
            for n in range(k):
                R = _rot(rng.normal(size=3) * 0.12)                                          # database -> query
                t = rng.normal(size=3); t *= rng.uniform(0.2, 0.8) / np.linalg.norm(t)
                rdb = R.T @ rq
                cdb = cq + rdb.T @ (R.T @ t)
                dname = f'seq-01/frame-{n_db:06d}.color.png'; n_db += 1
                img_scene.append(s); img_name.append(dname); img_test.append(False); img_c.append(cdb); img_q.append(_quat_wxyz(rdb))
                # scene points on integer pixels of the database image
                flat = rng.choice((W - 10) * (H - 10), size=4 * n_pts, replace=False)
                u, v = 5 + flat % (W - 10), 5 + flat // (W - 10)
                z = rng.uniform(1.5, 6.0, len(u))
                X0 = np.stack([(u - K[0, 2]) / K[0, 0] * z, (v - K[1, 2]) / K[1, 1] * z, z], 1)
                X1 = X0 @ R.T + t
                u1, v1 = K[0, 0] * X1[:, 0] / X1[:, 2] + K[0, 2], K[1, 1] * X1[:, 1] / X1[:, 2] + K[1, 2]
                ok = np.nonzero((X1[:, 2] > 0.3) & (u1 > 2) & (u1 < W - 3) & (v1 > 2) & (v1 < H - 3))[0][:n_pts]
                d = np.full((H, W), 5000, np.uint16)
                d[v[ok], u[ok]] = np.round(z[ok] * 1000).astype(np.uint16)
                depth.append(d)
                p1 = np.stack([u1[ok], v1[ok]], 1) + rng.normal(size=(len(ok), 2)) * 0.3
                bad = rng.permutation(len(ok))[:int(0.3 * len(ok))]
                p1[bad] = np.stack([rng.uniform(2, W - 3, len(bad)), rng.uniform(2, H - 3, len(bad))], 1)
                row = np.concatenate([np.stack([u[ok], v[ok]], 1).astype(np.float64), p1], 1).astype(np.float32)
                if s == 1 and qi == 3:
                    row = np.full((1, 4), np.nan, np.float32)
                corr[scenes[s]].append(row)
                pairs.append((s, dname, qname, float(np.round(rng.uniform(0.1, 0.9), 3))))
                pair_q.append(_quat_wxyz(R)); pair_t.append(t)
    M = len(img_name)
    p = dict(scenes=np.array(scenes), img_scene=np.array(img_scene, np.int64), img_name=np.array(img_name), img_test=np.array(img_test),
             img_c=np.stack(img_c), img_q=np.stack(img_q), pair_scene=np.array([q[0] for q in pairs], np.int64),
             pair_db=np.array([q[1] for q in pairs]), pair_query=np.array([q[2] for q in pairs]), pair_sim=np.array([q[3] for q in pairs]),
             pair_q=np.stack(pair_q), pair_t=np.stack(pair_t), depth_u16=np.stack(depth), color_u8=np.zeros((M, H, W, 3), np.uint8),
             width=np.int64(W), height=np.int64(H))
    return p, corr
