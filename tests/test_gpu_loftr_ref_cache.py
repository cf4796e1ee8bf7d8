"""-m gpu: LoFTR's backbone once per reference view (HIP.REF_FEATURE_CACHE for FEATURE_MATCHING 'LoFTR').

The feature rests on one property -- an image's backbone rows do not depend on what else is in the batch -- and on index plumbing that must not
change a bit: the gather kernel that fills the coarse token buffer from (feature set, index), LoFTRHIP.features / match_features against the
interleaved call, pipeline._RefCachedLoFTR against the plain path through submission.predict_fused, and the range-guard flag a cached view
carries.  Synthetic weights; images of 240 x 176 (coarse 30 x 22: 660 tokens, not a multiple of the 64-pixel tile)."""
import ctypes
import zipfile

import numpy as np
import pytest
import torch

from mapfree_reloc_amd import _lib, images as IM, submission
from mapfree_reloc_amd.config import get_cfg_defaults
from mapfree_reloc_amd.nets import weights as WT

pytestmark = pytest.mark.gpu

H, W = 240, 176
MFR_E_ARG = -1
ST_RANGE = 7


# ------------------------------------------------------------------------------------------------ 1. the gather kernel
def _gather(x, add, idx, ldo, out):
    n_src, C, HW = x.shape
    tab = (ctypes.c_int32 * len(idx))(*idx)
    return _lib.load().mfr_nchw_to_rows_gather(_lib.ptr(x), _lib.ptr(add), n_src, C, HW, tab, len(idx), _lib.ptr(out), HW * ldo, ldo, _lib.stream_ptr())


@pytest.mark.parametrize("pad", [0, 1])
@pytest.mark.parametrize("add", [False, True])
@pytest.mark.parametrize("HW", [660, 64, 1])
@pytest.mark.parametrize("C", [256, 96])
def test_rows_gather_equals_indexed_permute(C, HW, add, pad):
    g = torch.Generator().manual_seed(C + HW)
    x = torch.randn(5, C, HW, generator=g).cuda()
    a = torch.randn(C, HW, generator=g).cuda() if add else None
    idx = [3, 0, 3, 1, 4, 0]                                                          # repeats; source 2 is never read
    ldo = C * (1 + pad)
    out = torch.full((len(idx), HW, ldo), -7.0, device="cuda")
    assert _gather(x, a, idx, ldo, out) == 0
    want = torch.full_like(out, -7.0)
    want[:, :, :C] = ((x + a) if add else x)[idx].permute(0, 2, 1)
    assert torch.equal(out, want)


def test_rows_gather_more_slots_than_one_table_and_bad_indices():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(5, 96, 130, generator=g).cuda()
    a = torch.randn(96, 130, generator=g).cuda()
    idx = [(3 * j + j // 5) % 5 for j in range(70)]                                  # 70 slots: two launches (64 + 6)
    out = torch.full((70, 130, 96), -7.0, device="cuda")
    assert _gather(x, a, idx, 96, out) == 0
    assert torch.equal(out, (x + a)[idx].permute(0, 2, 1))
    # an index outside [0, n_src) anywhere in the table -- also beyond the first launch's 64 -- is refused before anything is launched
    for bad in ([0, 5], [-1], idx[:69] + [5]):
        out = torch.full((len(bad), 130, 96), -7.0, device="cuda")
        assert _gather(x, a, bad, 96, out) == MFR_E_ARG
        assert bool((out == -7.0).all())
    out = torch.full((1, 130, 96), -7.0, device="cuda")
    assert _gather(x, a, [0], 95, out) == MFR_E_ARG                                   # ldo < C
    assert _lib.load().mfr_nchw_to_rows_gather(_lib.ptr(x), None, 5, 96, 130, (ctypes.c_int32 * 1)(0), 0, _lib.ptr(out), 130 * 96, 96, _lib.stream_ptr()) == MFR_E_ARG
    assert bool((out == -7.0).all())


# ------------------------------------------------------------------------------------------------ 2., 3. the network
def _views():
    """one reference view and three queries of it (the second view rolled by 8 k rows), plus the views of another scene"""
    p, q = IM.synthetic_pair(21, H, W, hard=0), IM.synthetic_pair(22, H, W, hard=0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))[None, None].cuda()
    return dict(r=t(p["img0"]), q=[t(np.roll(p["img1"], 8 * k, axis=0)) for k in range(3)], other=[t(q["img0"]), t(q["img1"])])


@pytest.fixture(scope="module")
def views():
    return _views()


@pytest.fixture(scope="module")
def nets():
    from mapfree_reloc_amd.nets.loftr import LoFTRHIP
    sd = WT.loftr_state_dict()
    return {mt: LoFTRHIP(sd, "cuda", match_type=mt) for mt in ("dual_softmax", "sinkhorn")}


def test_backbone_rows_do_not_depend_on_batch_composition(nets, views):
    net = nets["dual_softmax"]
    a, b, c, d = views["r"], views["q"][0], views["other"][0], views["other"][1]
    assert not torch.equal(a, c) and not torch.equal(c, d)
    f4, f1, f3 = net.features(torch.cat([a, b, c, d])), net.features(c), net.features(torch.cat([d, c, a]))
    assert f4.coarse.shape == (4, 256, H // 8, W // 8) and f4.fine.shape == (4, H // 2, W // 2, 128) and f4.fine.is_contiguous()
    for name in ("coarse", "fine"):
        ref = getattr(f4, name)[2]
        assert bool(ref.abs().max() > 0)
        assert torch.equal(getattr(f1, name)[0], ref), name
        assert torch.equal(getattr(f3, name)[1], ref), name


@pytest.mark.parametrize("match_type", ["dual_softmax", "sinkhorn"])
def test_indexed_match_equals_interleaved_call(nets, views, match_type):
    net = nets[match_type]
    r, q = views["r"], views["q"]
    base = net(torch.cat([r, q[0], r, q[1], r, q[2]]))
    f = net.features(torch.cat([r] + q))
    got = net.match_features(f, [0, 0, 0], f, [1, 2, 3], H)
    assert set(got) == set(base) and {"pts0", "pts1", "n_corr", "mconf"} <= set(got)
    for k in base:
        assert torch.equal(got[k], base[k]), k
    assert bool((base["n_corr"] > 0).all()), base["n_corr"].tolist()
    # the two sides from DIFFERENT feature sets (a pool holding the reference view in slot 2, the queries alone)
    pool = type(f)(*(torch.cat([torch.zeros_like(t[:2]), t[:1]]) for t in f))
    fq = type(f)(*(t[1:].contiguous() for t in f))
    got = net.match_features(pool, [2, 2, 2], fq, [0, 1, 2], H)
    for k in base:
        assert torch.equal(got[k], base[k]), k


# ------------------------------------------------------------------------------------------------ 4., 5. the pipeline stage
class _SharedRefScene:
    """a scene whose pairs all have the SAME reference image (what every Map-free val / test scene is): three queries of one synthetic scene"""
    shared_reference = True

    def __init__(self, seed, sid, hw=(H, W)):
        self.scene_id, self.scene_root = sid, f"/synthetic/{sid}"
        self.p = IM.synthetic_pair(seed, hw[0], hw[1], hard=0)
        self.img0 = torch.from_numpy(self.p["img0"])[None].expand(3, -1, -1).contiguous()

    def __len__(self):
        return 3

    def pair_name(self, i):
        return f"seq1/frame_{5 * i:05d}.jpg"

    def __getitem__(self, i):
        p = self.p
        roll = lambda a: torch.from_numpy(np.ascontiguousarray(np.roll(a, 8 * i, axis=0)))
        return {"image0": self.img0, "image1": roll(p["img1"])[None].expand(3, -1, -1).contiguous(),
                "depth0": torch.from_numpy(p["depth0"]), "depth1": roll(p["depth1"]),
                "K_color0": torch.from_numpy(p["K"].copy()), "K_color1": torch.from_numpy(p["K"].copy()), "pair_id": 5 * i,
                "scene_id": self.scene_id, "scene_root": self.scene_root, "pair_names": ("seq0/frame_00000.jpg", self.pair_name(i))}


def _cfg(cache):
    cfg = get_cfg_defaults()
    cfg.MODEL, cfg.FEATURE_MATCHING, cfg.POSE_SOLVER = "FeatureMatching", "LoFTR", "EssentialMatrixMetric"
    cfg.EMAT_RANSAC.PIX_THRESHOLD, cfg.EMAT_RANSAC.SCALE_THRESHOLD, cfg.EMAT_RANSAC.CONFIDENCE = 2.0, 0.1, 0.9999
    cfg.ALLOW_SYNTHETIC_WEIGHTS = True
    cfg.HIP.REF_FEATURE_CACHE = cache
    cfg.HIP.LOADER_DECODE, cfg.HIP.LOADER_WORKERS = "thread", 2                       # six in-memory pairs: no pool of forked decode workers
    return cfg


def test_loftr_reference_view_cache_is_bitwise_neutral(tmp_path):
    """the backbone once per distinct reference view vs once per pair: the same archive byte for byte, on two scenes whose batches (4 pairs)
    straddle the scene boundary, so both the in-batch grouping and the cross-batch pool are used"""
    from mapfree_reloc_amd.pipeline import FusedPosePipeline
    scenes = [_SharedRefScene(11, "s00000"), _SharedRefScene(12, "s00001")]
    zs, stats = [], None
    for cache in (True, False):
        cfg = _cfg(cache)
        pipe = FusedPosePipeline(cfg)
        zs.append(submission.predict_fused(cfg, "test", tmp_path / f"c{int(cache)}", pipeline=pipe, batch_pairs=4, scenes=scenes))
        if cache:
            stats = pipe.match.stats
    assert stats == {"reference_views_run": 2, "reference_views_reused": 4}, stats
    assert open(zs[0], "rb").read() == open(zs[1], "rb").read()
    with zipfile.ZipFile(zs[0]) as a:
        for sid in ("s00000", "s00001"):
            lines = a.read(f"pose_{sid}.txt").decode().split("\n")
            assert len(lines) == 3 and all("nan" not in l for l in lines)              # real poses were compared, not failures


def _pair_batch(scene, ids, key):
    s = [scene[i] for i in ids]
    d = lambda k, dt: torch.stack([x[k] for x in s]).to(dt).cuda()
    return dict(images=torch.stack([x[k][:1] for x in s for k in ("image0", "image1")]).float().cuda(), depth0=d("depth0", torch.float32),
                depth1=d("depth1", torch.float32), K0=d("K_color0", torch.float64), K1=d("K_color1", torch.float64),
                seed_ids=torch.tensor([x["pair_id"] for x in s], dtype=torch.int64).cuda(), ref_keys=[key] * len(s))


def test_stale_guard_flag_of_a_cached_view_marks_the_batches_that_reuse_it():
    """a cached view was computed under an EARLIER batch's guard window: its flag travels with it"""
    from mapfree_reloc_amd.pipeline import FusedPosePipeline
    pipe = FusedPosePipeline(_cfg(True))
    assert pipe.guard.active
    sa, sb = _SharedRefScene(11, "s00000"), _SharedRefScene(12, "s00001")
    ka, kb = ("/synthetic/s00000", "seq0/frame_00000.jpg"), ("/synthetic/s00001", "seq0/frame_00000.jpg")
    first = pipe(_pair_batch(sa, [0, 1], ka))
    assert not bool((first["status"] == ST_RANGE).any())
    view = pipe.match.cache[ka]
    assert view.flag.shape == (1,) and view.flag.dtype == torch.int32 and int(view.flag) == 0
    view.flag.fill_(1)
    reuse = pipe(_pair_batch(sa, [2, 1], ka))
    assert reuse["status"].tolist() == [ST_RANGE, ST_RANGE]
    assert bool(torch.isnan(reuse["R"]).all())
    other = pipe(_pair_batch(sb, [0, 1], kb))                                         # a batch that does not touch the flagged view
    assert not bool((other["status"] == ST_RANGE).any())
    mixed = pipe(dict(_pair_batch(sa, [0, 1], ka), ref_keys=[ka, None]))               # ... and one that does, for one of its pairs
    assert mixed["status"].tolist() == [ST_RANGE, ST_RANGE]
    assert pipe.match.stats == {"reference_views_run": 3, "reference_views_reused": 5}
