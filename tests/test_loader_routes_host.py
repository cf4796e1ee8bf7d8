"""Every row and row table of every PairBatchLoader batch against the files it must come from, on every host-side route, no GPU: thread and
process decode x host / device JPEG x host / device depth PNG x colour bytes, on two Map-free scenes of 5 pairs that share their keyframe
(batch_pairs 4: a batch that spans the scene boundary, reference rows duplicated from another row, a short last batch), on a scene without
the fast route and on a ScanNet-style scene that states its layout.  A device row is checked against a fresh parse of its file; the number
of device rows per configuration is asserted, so that a loader which quietly decodes everything on the host fails here."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scannet_tree as ST  # noqa: E402

from mapfree_reloc_amd import datasets as D  # noqa: E402
from mapfree_reloc_amd import jpeg_ops as J, png_ops as P  # noqa: E402
from mapfree_reloc_amd.config import get_cfg_defaults  # noqa: E402
from mapfree_reloc_amd.scannet import pair_image_paths  # noqa: E402
from tools.bench_fused_split import write_scene  # noqa: E402

ROUTES = [("thread", 1), ("thread", 3), ("process", 2)]
SAME_ON_BOTH = ("K0", "K1", "seed_ids", "global_ids", "names", "scene_ids", "scene_roots", "scenes_done", "ref_keys", "scene_id", "scene_root",
                "scene_index", "last_of_scene")


def _pil(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))


def _masked_parse(parse_into, header_bytes, path, cap):
    """(header, record, bytes the parser writes, record bytes) of a fresh parse: the parser leaves a few bytes of a record unwritten, so the
    file is parsed into a zero-filled and into a 0xFF-filled buffer and only the bytes on which the two agree are compared"""
    data = open(path, "rb").read()
    out = []
    for fill in (0, 0xFF):
        hdr, rec = np.full(header_bytes, fill, np.uint8), np.full(cap, fill, np.uint8)
        st, nb = parse_into(data, hdr, rec)
        assert st == 0, (path, st)
        out.append((hdr, rec[:nb], nb))
    (h0, r0, nb), (h1, r1, nb1) = out
    assert nb == nb1 and nb > 0
    return h0, h0 == h1, r0, r0 == r1, nb


def _resolve(rows, r):
    while rows[r] is not None and rows[r][0] == "dup":
        assert rows[r][1] != r
        r = rows[r][1]
    return r


def _check_batch(b, files, resize, rgb):
    """files(global id) -> ((jpeg0, jpeg1), (depth0, depth1) or None).  -> (device JPEG rows, device depth rows) of the batch"""
    n = len(b["names"])
    assert b["images"].shape[0] == 2 * n and b["images"].dtype == torch.float32
    gids = b["global_ids"].tolist()
    jrows = b["jpeg"]["rows"] if "jpeg" in b else [None] * (2 * n)
    assert len(jrows) == 2 * n
    n_jpeg = n_png = 0
    for r in range(2 * n):
        path = files(gids[r // 2])[0][r % 2]
        src = _resolve(jrows, r)
        if jrows[src] is None or jrows[src][0] != 0:                     # a host plane (decoded there, or the device route's host fall-back)
            assert jrows[src] is None or (jrows[src][1] == 0 and jrows[src][2] == path)
            assert np.array_equal(b["images"][src, 0].numpy(), D.read_gray_plane(path, resize)), (r, src, path)
            if rgb:
                assert np.array_equal(b["rgb"][src].numpy(), _pil(path)), (r, src, path)
        else:
            hdr, hmask, rec, rmask, nb = _masked_parse(J.parse_into, J.HEADER_BYTES, path, b["jpeg"]["records"].shape[1])
            assert jrows[src] == (0, nb, path), (r, src, jrows[src], nb, path)
            assert np.array_equal(b["jpeg"]["headers"][src].numpy()[hmask], hdr[hmask])
            assert np.array_equal(b["jpeg"]["records"][src, :nb].numpy()[rmask], rec[rmask])
            n_jpeg += 1
    if rgb:
        assert b["depth0"] is None and b["depth1"] is None and "png" not in b and b["rgb"].shape == (2 * n, *b["images"].shape[-2:], 3)
        return n_jpeg, n_png
    assert "rgb" not in b
    if b["depth0"] is None:
        assert b["depth1"] is None and "png" not in b and files(gids[0])[1] is None
        return n_jpeg, n_png
    assert b["depth0"].shape == b["depth1"].shape == (n, *b["images"].shape[-2:])
    prows = b["png"]["rows"] if "png" in b else [None] * (2 * n)
    assert len(prows) == 2 * n
    plane = lambda r: (b["depth0"][r] if r < n else b["depth1"][r - n]).numpy()
    for r in range(2 * n):                                               # rows 0..n-1 are depth0's, n..2n-1 depth1's
        path = files(gids[r % n])[1][r // n]
        src = _resolve(prows, r)
        if prows[src] is None:
            assert np.array_equal(plane(src), D.read_depth_plane(path)), (r, src, path)
        else:
            cap = plane(src).size * 4 // 16 * 16
            hdr, hmask, rec, rmask, nb = _masked_parse(P.parse_into, P.HEADER_BYTES, path, cap)
            assert prows[src] == (0, nb, path), (r, src, prows[src], nb, path)
            assert np.array_equal(b["png"]["headers"][src].numpy()[hmask], hdr[hmask])
            assert np.array_equal(plane(src).reshape(-1).view(np.uint8)[:nb][rmask], rec[rmask])   # the record lies at the start of the row's own plane
            n_png += 1
    return n_jpeg, n_png


def _run(scenes, files, resize, batch_pairs, rgb=False, **kw):
    """-> {route: (batches without their buffers, device JPEG rows, device depth rows)}; every batch is checked while its slot is its own"""
    out = {}
    for decode, workers in ROUTES:
        D.clear_frame_cache()
        loader = D.PairBatchLoader(scenes, batch_pairs, prefetch=0, pin=False, workers=workers, decode=decode, rgb=rgb, **kw)
        kept, nj, npng = [], 0, 0
        try:
            for b in loader:
                assert ("_slot" in b) == (decode == "process")
                j, g = _check_batch(b, files, resize, rgb)
                nj, npng = nj + j, npng + g
                kept.append({k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in b.items()
                             if k in SAME_ON_BOTH} | {"keys": [k for k in b if k != "_slot"]})
        finally:
            loader.close()
        out[(decode, workers)] = (kept, nj, npng)
    ref = out[ROUTES[0]][0]
    for route in ROUTES[1:]:
        got = out[route][0]
        assert len(got) == len(ref)
        for a, b in zip(ref, got):
            assert a["keys"] == b["keys"], route
            for k in SAME_ON_BOTH:
                if isinstance(a[k], torch.Tensor):
                    assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), (route, k)
                else:
                    assert a[k] == b[k], (route, k)
    return out


def _counts(out):
    return {route: v[1:] for route, v in out.items()}


# ---------------------------------------------------------------- two Map-free scenes that share their keyframe
@pytest.fixture(scope="module")
def mapfree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("routes"))
    for s in (0, 1):
        write_scene((root, s, 5))
    cfg = get_cfg_defaults()
    cfg.DATASET.DATA_ROOT, cfg.DATASET.WIDTH, cfg.DATASET.HEIGHT, cfg.DATASET.ESTIMATED_DEPTH = root, 540, 720, "dptkitti"
    scenes = D.list_scenes(cfg, "test")
    assert [len(sc) for sc in scenes] == [5, 5] and all(sc.shared_reference for sc in scenes)

    def files(gid):
        sc = scenes[gid // 5]
        sa, ia, sb, ib = sc.pairs[gid % 5]
        jp = tuple(os.path.join(sc.scene_root, f"seq{s}/frame_{i:05}.jpg") for s, i in ((sa, ia), (sb, ib)))
        return jp, tuple(p.replace(".jpg", ".dptkitti.png") for p in jp)
    return scenes, files


CONFIGS = [(rgb, jd, dd) for rgb in (False, True) for jd in ("host", "device") for dd in ("host", "device") if not (rgb and dd == "device")]


@pytest.mark.parametrize("rgb,jpeg_decode,depth_decode", CONFIGS)
def test_mapfree_rows_come_from_their_files(mapfree, rgb, jpeg_decode, depth_decode):
    scenes, files = mapfree
    out = _run(scenes, files, (540, 720), 4, rgb=rgb, jpeg_decode=jpeg_decode, depth_decode=depth_decode)
    for kept, _, _ in out.values():
        assert [len(b["names"]) for b in kept] == [4, 4, 2]
        assert [b["scenes_done"] for b in kept] == [[], ["s00000"], ["s00001"]] and kept[1]["scene_ids"] == ["s00000"] + ["s00001"] * 3
    # of 20 JPEG rows and 20 depth rows.  Thread decode sends pair 0 of each batch down the generic route on the loader thread when the
    # layout comes from a sample (rgb=False): its rows, and the duplicates that resolve to them, are host planes
    jd, dd = jpeg_decode == "device", depth_decode == "device"
    thread = ((20 if rgb else 10) if jd else 0, 10 if dd else 0)
    assert _counts(out) == {("thread", 1): thread, ("thread", 3): thread, ("process", 2): (20 if jd else 0, 20 if dd else 0)}


# ---------------------------------------------------------------- a scene without the fast route
class _GenericScene:
    """samples come from __getitem__ only (as tests/test_dpt_fused_host._GenericScene)"""
    has_gray_pair = False

    def __init__(self, sc):
        self.sc, self.scene_id, self.scene_root, self.shared_reference = sc, sc.scene_id, sc.scene_root, sc.shared_reference

    def __len__(self):
        return len(self.sc)

    def __getitem__(self, i):
        return self.sc[i]


@pytest.mark.parametrize("rgb,jpeg_decode,depth_decode", [(False, "host", "host"), (False, "device", "device"), (True, "device", "host")])
def test_generic_scene_rows_come_from_their_files(mapfree, rgb, jpeg_decode, depth_decode):
    scenes, files = mapfree
    out = _run([_GenericScene(sc) for sc in scenes], files, (540, 720), 4, rgb=rgb, jpeg_decode=jpeg_decode, depth_decode=depth_decode)
    assert _counts(out) == {route: (0, 0) for route in ROUTES}         # nothing of a generic sample goes to the device


# ---------------------------------------------------------------- a ScanNet-style scene: batch_layout(), a resizing gray_pair, no shared reference
@pytest.fixture(scope="module")
def scannet(tmp_path_factory):
    p = ST.default_params(5)
    W, H, fw, fh = 20, 14, 41, 29                                       # files larger than the network size, depth at the network size
    rng = np.random.default_rng(9)
    n = len(p["frames"])
    yy, xx = np.mgrid[0:fh, 0:fw]
    p["color_u8"] = np.stack([np.clip(np.stack([4 * xx + 3 * k, 6 * yy, 255 - 3 * xx - 2 * yy], -1) + rng.integers(0, 30, (fh, fw, 3)), 0, 255)
                              for k in range(n)]).astype(np.uint8)
    p["depth_u16"] = rng.integers(0, 65536, size=(n, H, W)).astype(np.uint16)
    p["width"], p["height"] = np.int64(W), np.int64(H)
    tr = ST.write_tree(tmp_path_factory.mktemp("scannet_routes"), p)
    cfg = get_cfg_defaults()
    cfg.DATASET.DATA_SOURCE, cfg.DATASET.DATA_ROOT, cfg.DATASET.NPZ_ROOT = "ScanNet", tr["data_root"], tr["npz_root"]
    cfg.DATASET.WIDTH, cfg.DATASET.HEIGHT, cfg.DATASET.MIN_OVERLAP_SCORE = W, H, float(p["min_overlap_score"])
    scenes = D.list_scenes(cfg, "test")
    assert len(scenes) == 1 and len(scenes[0]) == 5 and scenes[0].batch_layout() == (H, W, True)
    paths = pair_image_paths(tr["test_npz"], tr["scans"])
    return scenes, (lambda gid: (paths[gid], tuple(q.replace(".color.jpg", ".depth.pgm") for q in paths[gid]))), (W, H)


@pytest.mark.parametrize("jpeg_decode,depth_decode", [("host", "host"), ("device", "device")])
def test_scannet_rows_come_from_their_files(scannet, jpeg_decode, depth_decode):
    scenes, files, resize = scannet
    out = _run(scenes, files, resize, 2, jpeg_decode=jpeg_decode, depth_decode=depth_decode)
    for kept, _, _ in out.values():
        assert [len(b["names"]) for b in kept] == [2, 2, 1] and all(b["ref_keys"] == [None] * len(b["names"]) for b in kept)
    # every JPEG row takes the fast route (the layout is stated, no pair is decoded generically); its depth maps have no device readers
    assert _counts(out) == {route: ((10 if jpeg_decode == "device" else 0), 0) for route in ROUTES}
