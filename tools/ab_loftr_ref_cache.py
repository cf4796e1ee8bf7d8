"""A/B of LoFTR's reference-view cache (HIP.REF_FEATURE_CACHE, pipeline._RefCachedLoFTR) on resident data: one batch of 16 pairs of 540 x 720
(padded to 544 x 720) that share ONE reference view -- what a batch inside a Map-free val / test scene looks like -- through the matcher stage
of LoFTREmatPipeline, timed between device events:

    plain        the backbone on all 32 images                                      (ref_keys=None)
    cached_cold  the view is not in the pool yet: 17 images, one pool copy          (the first batch of a scene)
    cached_warm  the view is in the pool: 16 images                                 (every later batch of the scene)

The variants alternate inside one process, every shape is warmed up first, and each is repeated `--reps` times; the record holds every time, the
median and the spread (max - min, and the inter-quartile range).  To say where the time goes the backbone alone (32 / 17 / 16 images) and
everything after it (16 pairs) are timed the same way.

python tools/ab_loftr_ref_cache.py --out profiles/loftr_ref_cache_ab.json"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loftr_ref_cache_ab.json"))
    a = ap.parse_args()

    import torch
    import mapfree_reloc_amd  # noqa: F401
    from mapfree_reloc_amd import images as IM
    from mapfree_reloc_amd.nets.loftr import pad_to_multiple
    from mapfree_reloc_amd.pipeline import LoFTREmatPipeline
    dev = "cuda:0"
    p = IM.synthetic_pair(100)
    planes = []
    for k in range(a.pairs):                                          # the second view rolled by 8 k rows: distinct queries of one reference
        planes += [p["img0"], np.roll(p["img1"], 8 * k, axis=0)]
    images = torch.from_numpy(np.stack(planes)[:, None]).to(dev)
    keys = [("scene", "seq0/frame_00000.jpg")] * a.pairs
    pipe = LoFTREmatPipeline(dev)
    stage, net = pipe._ref, pipe.loftr
    padded = pad_to_multiple(images, pipe.pad_to)
    feats = net.features(padded)
    idx0, idx1 = list(range(0, 2 * a.pairs, 2)), list(range(1, 2 * a.pairs, 2))

    def cold():
        stage.cache.clear()
        return pipe.match(images, keys)                               # ... and leaves the view in the pool for cached_warm

    variants = {
        "plain": lambda: pipe.match(images),
        "cached_cold": cold,
        "cached_warm": lambda: pipe.match(images, keys),
        "backbone_%d" % (2 * a.pairs): lambda: net.features(padded),
        "backbone_%d" % (a.pairs + 1): lambda: net.features(padded[:a.pairs + 1]),
        "backbone_%d" % a.pairs: lambda: net.features(padded[:a.pairs]),
        "after_backbone_%d_pairs" % a.pairs: lambda: net.match_features(feats, idx0, feats, idx1, padded.shape[2]),
    }

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with pipe.guard:
            e0.record()
            out = fn()
            e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    ref = None
    for name, fn in variants.items():                                 # warm-up of every shape; the three stage variants must agree bit for bit
        for _ in range(a.warmup):
            _, out = timed(fn)
        if name in ("plain", "cached_cold", "cached_warm"):
            ref = out if ref is None else ref
            assert all(torch.equal(out[k], ref[k]) for k in ref), name
    times = {name: [] for name in variants}
    for _ in range(a.reps):                                           # alternate: drift of the clocks hits every variant alike
        for name, fn in variants.items():
            times[name].append(timed(fn)[0])
    rec = {"gpu": torch.cuda.get_device_name(0), "pairs": a.pairs, "image": list(padded.shape[-2:]), "reps": a.reps, "warmup": a.warmup,
           "n_corr_mean": float(ref["n_corr"].float().mean()), "unit": "ms, device events around the matcher stage", "variants": {}}
    for name, t in times.items():
        q = np.percentile(t, [25, 50, 75])
        rec["variants"][name] = dict(median=round(float(q[1]), 3), min=round(min(t), 3), max=round(max(t), 3), spread=round(max(t) - min(t), 3),
                                     iqr=round(float(q[2] - q[0]), 3), times=[round(x, 3) for x in t])
    v = rec["variants"]
    rec["saving_ms"] = dict(cached_warm=round(v["plain"]["median"] - v["cached_warm"]["median"], 3),
                            cached_cold=round(v["plain"]["median"] - v["cached_cold"]["median"], 3), spread_of_plain=v["plain"]["spread"])
    rec["pairs_per_s"] = {k: round(a.pairs / v[k]["median"] * 1e3, 1) for k in ("plain", "cached_cold", "cached_warm")}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({k: rec[k] for k in ("saving_ms", "pairs_per_s")}), flush=True)
    print({k: (x["median"], x["spread"]) for k, x in v.items()}, flush=True)


if __name__ == "__main__":
    main()
