"""DPT depth on the fused route (DPT.SOURCE 'online', nets/dpt.FusedDepthStage) against today's route, depth maps read from files, on ONE GPU.

The tree is tools/bench_fused_split.write_scene's (540 x 720 JPEG q92 + 16-bit millimetre PNG, Map-free layout).  Per configuration -- SuperGlue + PnP (reads
depth0: DPT once per scene) and SuperGlue + EssentialMatrixMetric (reads both maps: DPT on every query view) -- three runs in the order (a1) depth from
files, (b) DPT.SOURCE 'online', (a2) depth from files again: the difference between a1 and a2 is the spread the (b) - (a) difference has to be read against.
Every run is the loop of submission.predict_fused without its file writing: PairBatchLoader (process decode) -> DevicePrefetcher -> FusedPosePipeline, one
untimed pass over the tree first (every batch shape, the ragged last one included), then the timed pass with device events around every step (median GPU ms
per step) and around the depth stage, and a host clock from the arrival of the first batch (the decode processes have started by then: seconds of forking
that a run over a real split pays once) to a synchronise after the last step, over the pairs of the batches behind the first (pairs/s).  Each run is a
fresh child process, one at a time: in one long-lived process the host-fed rate of the SAME file run fell from 813 to 142 pairs/s between the first and the
third run, which swamped every difference: decode workers forked from a process that has built the DPT network are slow, whatever they decode (--probe,
probe_loader: the loaders alone, in a process without a network, after the online pipeline is built, and with the pool forked before it is built).  What a user without depth files pays
on today's route comes on top of (a): compute_depth over the same tree (DPT on every frame, one 16-bit PNG written per frame), timed here as its wall time.
The DPT weights are the synthetic DPT-Hybrid set at DPT.NET_HEIGHT x NET_WIDTH = 384 x 512: the arithmetic of the real checkpoint, not its values -- the
maps are not the scenes' geometry, so the pose counts of the online runs (`poses`) say nothing and are recorded only to show what the solver was given.

python tools/bench_dpt_fused.py --scenes 16 --frames 64 --out profiles/dpt_fused.json"""
import argparse
import json
import os
import shutil
import statistics
import sys
import time
from concurrent.futures import ProcessPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SUFFIX = "dptbench"          # compute_depth's maps go under this name and are removed again: the tree's own maps stay what (a) reads


def make_cfg(root, solver, source, a):
    from mapfree_reloc_amd.config import get_cfg_defaults
    cfg = get_cfg_defaults()
    cfg.DATASET.DATA_ROOT, cfg.DATASET.WIDTH, cfg.DATASET.HEIGHT, cfg.DATASET.ESTIMATED_DEPTH = root, 540, 720, "dptkitti"
    cfg.MODEL, cfg.FEATURE_MATCHING, cfg.POSE_SOLVER, cfg.ALLOW_SYNTHETIC_WEIGHTS = "FeatureMatching", "SuperGlue", solver, True
    cfg.PNP.RANSAC_ITER, cfg.PNP.REPROJECTION_INLIER_THRESHOLD, cfg.PNP.CONFIDENCE = 1000, 3, 0.9999
    cfg.EMAT_RANSAC.PIX_THRESHOLD, cfg.EMAT_RANSAC.SCALE_THRESHOLD, cfg.EMAT_RANSAC.CONFIDENCE = 2.0, 0.1, 0.9999
    cfg.HIP.LOADER_DECODE, cfg.HIP.JPEG_DECODE, cfg.HIP.LOADER_WORKERS = "process", a.jpeg_decode, a.workers
    cfg.DPT.SOURCE, cfg.DPT.FUSED_CHUNK, cfg.DPT.INVERT = source, a.chunk, False        # (synthetic weights want INVERT False: config/default.py)
    return cfg


def run(cfg, B, workers):
    """one warm-up pass and one timed pass over the split -> the record of the timed pass"""
    import torch
    from mapfree_reloc_amd import submission
    from mapfree_reloc_amd.datasets import DevicePrefetcher, PairBatchLoader, list_scenes, usable_cpus
    from mapfree_reloc_amd.pipeline import FusedPosePipeline
    dev = torch.device("cuda", 0)
    pipe = FusedPosePipeline(cfg, dev)
    stage, depth_evs = pipe.depth, []
    if stage is not None:
        def timed_stage(batch):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = stage(batch)
            e1.record()
            depth_evs.append((e0, e1))
            return out
        pipe.depth = timed_stage
    scenes = list_scenes(cfg, "test")
    rec = {}
    for timed in (False, True):
        for st in (stage, pipe.match):                     # every pass starts with empty reference-view caches and counters
            if hasattr(st, "cache"):
                st.cache.clear()
            for k in getattr(st, "stats", {}):
                st.stats[k] = 0
        del depth_evs[:]
        loader = PairBatchLoader(scenes, B, prefetch=2, pin=True, workers=workers or usable_cpus(), decode="process", jpeg_decode=str(cfg.HIP.JPEG_DECODE),
                                 rgb=submission.wants_rgb(cfg, pipe))
        evs, pairs, ok, t_first, first_pairs = [], 0, 0, None, 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        try:
            for batch in DevicePrefetcher(loader, dev):
                if t_first is None:
                    t_first, first_pairs = time.perf_counter(), len(batch["names"])
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = pipe(batch)
                e1.record()
                evs.append((e0, e1, out["status"]))
                pairs += len(batch["names"])
            torch.cuda.synchronize()
            t_end = time.perf_counter()
        finally:
            loader.close()
        if timed:
            ms = [a.elapsed_time(b) for a, b, _ in evs]
            ok = int(sum(int((s == 0).sum()) for _, _, s in evs))
            dt = t_end - t_first
            rec = dict(pairs=pairs, poses=ok, batch_pairs=B, steps=len(ms), until_first_batch_s=round(t_first - t0, 3), seconds=round(dt, 3),
                       pairs_per_s=round((pairs - first_pairs) / dt, 1),
                       gpu_ms_per_step_median=round(statistics.median(ms), 3), gpu_ms_per_step_min=round(min(ms), 3), gpu_ms_per_step_max=round(max(ms), 3),
                       gpu_ms_total=round(sum(ms), 1))
            if stage is not None:
                dms = [a.elapsed_time(b) for a, b in depth_evs]
                rec.update(depth_stage_ms_per_step_median=round(statistics.median(dms), 3), depth_stage_ms_first_step=round(dms[0], 3),
                           depth_stage_ms_total=round(sum(dms), 1), **stage.stats)
    return rec


def time_compute_depth(cfg, root):
    """wall time of compute_depth over the tree: the estimator built and warmed first (one scene, removed again), then every scene"""
    import glob
    import torch
    from mapfree_reloc_amd import compute_depth as CD
    from mapfree_reloc_amd.nets.dpt import DepthEstimator

    def clean():
        for f in glob.glob(os.path.join(root, "test", "*", "seq*", f"*.{SUFFIX}.png")):
            os.remove(f)
    est = DepthEstimator(cfg)
    dirs = CD.list_scene_dirs("Mapfree", root)
    clean()
    CD.run_scene(est, "Mapfree", dirs[0], SUFFIX, batch=16)
    clean()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    frames = sum(CD.run_scene(est, "Mapfree", d, SUFFIX, batch=16)[0] for d in dirs)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    nbytes = sum(os.path.getsize(f) for f in glob.glob(os.path.join(root, "test", "*", "seq*", f"*.{SUFFIX}.png")))
    clean()
    return dict(frames=frames, seconds=round(dt, 3), frames_per_s=round(frames / dt, 1), png_MB_written=round(nbytes / 1e6, 1), batch=16)


PROBES = ("loaders_alone", "after_dpt_is_built", "pool_forked_before_dpt")


def probe_loader(variant, a):
    """--probe: the host-fed rate of the loaders WITHOUT any pipeline step (pairs/s behind the first batch, to the device), in a process that
    loaders_alone           has built no network: the file loader, then the colour-byte loader;
    after_dpt_is_built      has built the online pipeline (DPT-Hybrid) first: both loaders with process decode, then the file loader with thread decode;
    pool_forked_before_dpt  forks the colour-byte loader's decode processes first (its first batch), then builds the online pipeline, then drains the loader"""
    import torch
    from mapfree_reloc_amd.datasets import DevicePrefetcher, PairBatchLoader, list_scenes, usable_cpus
    from mapfree_reloc_amd.pipeline import FusedPosePipeline
    dev = torch.device("cuda", 0)
    on, files = make_cfg(a.root, "PNP", "online", a), make_cfg(a.root, "PNP", "file", a)

    def loader(cfg, rgb, decode="process"):
        return PairBatchLoader(list_scenes(cfg, "test"), a.batch_pairs, prefetch=2, pin=True, workers=a.workers or usable_cpus(), decode=decode, rgb=rgb)

    def drain(L, it=None):
        it = iter(DevicePrefetcher(L, dev)) if it is None else it
        try:
            next(it)
            t, n = time.perf_counter(), 0
            for b in it:
                n += len(b["names"])
            torch.cuda.synchronize()
            return round(n / (time.perf_counter() - t), 1)
        finally:
            L.close()
    if variant == "loaders_alone":
        return dict(files_process_decode=drain(loader(files, False)), rgb_process_decode=drain(loader(on, True)))
    if variant == "after_dpt_is_built":
        pipe = FusedPosePipeline(on, dev)  # noqa: F841  (kept alive: the state the online run's loader is started in)
        return dict(files_process_decode=drain(loader(files, False)), rgb_process_decode=drain(loader(on, True)),
                    files_thread_decode=drain(loader(files, False, "thread")))
    L = loader(on, True)
    it = iter(DevicePrefetcher(L, dev))
    first = [next(it)]
    pipe = FusedPosePipeline(on, dev)  # noqa: F841
    import itertools
    return dict(rgb_process_decode=drain(L, itertools.chain(first, it)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default="/tmp/mapfree_syn_dpt")
    ap.add_argument("--scenes", type=int, default=16)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--batch-pairs", type=int, default=16)
    ap.add_argument("--chunk", type=int, default=16, help="DPT.FUSED_CHUNK")
    ap.add_argument("--workers", type=int, default=0, help="decode workers (0 = the granted CPUs)")
    ap.add_argument("--jpeg-decode", default="host", help="host | device (HIP.JPEG_DECODE)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dpt_fused.json"))
    ap.add_argument("--leg", default="", help="(internal) run ONE leg in this process and print its record: SOLVER:SOURCE, compute_depth, or probe:VARIANT")
    ap.add_argument("--probe", action="store_true", help="only the loader probe (probe_loader): its record is added to the one already at --out")
    a = ap.parse_args()
    if a.leg:
        import mapfree_reloc_amd  # noqa: F401
        if a.leg == "compute_depth":
            rec = time_compute_depth(make_cfg(a.root, "PNP", "file", a), a.root)
        elif a.leg.startswith("probe:"):
            rec = probe_loader(a.leg.split(":")[1], a)
        else:
            solver, source = a.leg.split(":")
            rec = run(make_cfg(a.root, solver, source, a), a.batch_pairs, a.workers)
        print("LEG_RECORD " + json.dumps(rec), flush=True)
        return

    def leg(what):
        import subprocess
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", what, "--root", a.root, "--batch-pairs", str(a.batch_pairs), "--chunk", str(a.chunk),
               "--workers", str(a.workers), "--jpeg-decode", a.jpeg_decode]
        out = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True).stdout
        return json.loads(next(l for l in out.splitlines() if l.startswith("LEG_RECORD "))[len("LEG_RECORD "):])
    from bench_fused_split import write_scene
    if not os.path.isdir(os.path.join(a.root, "test", f"s{a.scenes - 1:05d}")):
        shutil.rmtree(a.root, ignore_errors=True)
        with ProcessPoolExecutor(min(16, os.cpu_count() or 8)) as ex:
            list(ex.map(write_scene, [(a.root, s, a.frames) for s in range(a.scenes)]))
    if a.probe:
        res = json.load(open(a.out))
        res["loader_probe"] = dict(what="pairs/s of the loaders alone (no pipeline step), each variant in a fresh child process: tools/bench_dpt_fused.probe_loader",
                                   **{v: leg("probe:" + v) for v in PROBES})
        print("loader_probe", json.dumps(res["loader_probe"]), flush=True)
        json.dump(res, open(a.out, "w"), indent=1)
        return
    import torch
    import mapfree_reloc_amd  # noqa: F401
    from mapfree_reloc_amd import options
    res = dict(gpu=torch.cuda.get_device_name(0), split=options.get("SPLIT"),
               tree=dict(scenes=a.scenes, pairs=a.scenes * a.frames, frames=a.scenes * (a.frames + 1), layout="tools/bench_fused_split.write_scene: 540x720 JPEG q92 + 16-bit mm PNG"),
               dpt=dict(net="DPT-Hybrid, synthetic weights", net_hw=[384, 512], fused_chunk=a.chunk), loader=dict(decode="process", jpeg_decode=a.jpeg_decode),
               method="per run: one untimed pass over the tree, then the timed pass; gpu_ms_per_step = device events around pipeline(batch), median over the steps; "
                      "seconds = host clock from the first batch's arrival to a synchronise after the last step, pairs_per_s = the pairs behind the first batch over it; "
                      "order a1 (files), b (online), a2 (files), each in a fresh child process")
    for name, solver in (("sg_pnp", "PNP"), ("sg_emat_metric", "EssentialMatrixMetric")):
        r = {}
        for leg_name, source in (("a1_depth_from_files", "file"), ("b_online", "online"), ("a2_depth_from_files", "file")):
            r[leg_name] = leg(f"{solver}:{source}")
            print(name, leg_name, json.dumps(r[leg_name]), flush=True)
        a1, b, a2 = r["a1_depth_from_files"], r["b_online"], r["a2_depth_from_files"]
        r["summary"] = dict(
            gpu_ms_per_step_online_minus_files=round(b["gpu_ms_per_step_median"] - (a1["gpu_ms_per_step_median"] + a2["gpu_ms_per_step_median"]) / 2, 3),
            gpu_ms_per_step_spread_of_the_two_file_runs=round(abs(a1["gpu_ms_per_step_median"] - a2["gpu_ms_per_step_median"]), 3),
            seconds_online_minus_files=round(b["seconds"] - (a1["seconds"] + a2["seconds"]) / 2, 3),
            seconds_spread_of_the_two_file_runs=round(abs(a1["seconds"] - a2["seconds"]), 3))
        res[name] = r
    res["compute_depth_over_the_tree"] = leg("compute_depth")
    print("compute_depth", json.dumps(res["compute_depth_over_the_tree"]), flush=True)
    for name in ("sg_pnp", "sg_emat_metric"):
        a1, b, a2 = (res[name][k]["seconds"] for k in ("a1_depth_from_files", "b_online", "a2_depth_from_files"))
        res[name]["summary"]["seconds_files_route_plus_compute_depth"] = round((a1 + a2) / 2 + res["compute_depth_over_the_tree"]["seconds"], 3)
        res[name]["summary"]["seconds_online_route"] = b
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
