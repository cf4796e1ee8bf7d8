#!/usr/bin/env python
"""bench.py -- image-pairs/s of the fused matcher -> depth lift -> RANSAC pose hot path on MI355X.

  --config sg_pnp      (default) BASELINE.json configs[1]: SuperPoint+SuperGlue matching + PnP w/ DPT depth, 540x720
  --config loftr_emat  BASELINE.json configs[2]: LoFTR coarse-to-fine matching + Essential-matrix RANSAC (+ metric
                       scale from depth), 540x720 right-padded to 544 like the reference (quirk Q3)
  --config rpr_train   BASELINE.json configs[4]: one bf16 training step (forward, loss, backward, gradient
                       all-reduce over RCCL, clip, Adam) of the 3d3d relative-pose-regression model
                       (config/regression/mapfree/3d3d.yaml: ResUNet 3-3-3, correlation-volume warping, Procrustes head)
                       on synthetic 360x270 pairs, TRAINING.BATCH_SIZE 10 per GPU

Synthetic pairs, seeded synthetic weights (no data / checkpoints offline).  A "step" is one pass of the whole
path over one batch of B image pairs per GPU, inputs already resident in HBM.  N > 1 GPUs: pairs shard
embarrassingly (one process per GPU, no data-path collective); the only collective is ONE RCCL all_gather of
the per-pair pose records at the end of the run (80 B/pair), inside the timed region.  Weak scaling.

  python bench.py --gpus 1 --steps 10 --warmup 3
  python bench.py --gpus 1 --steps 10 --warmup 3 --dump-outputs DIR   # + the last timed step's outputs as DIR/<name>.npy
  python bench.py --full                         # + roofline (live kernel timers), CPU baseline, parity vs the oracle, secondary configs
  python bench.py --gpus 8                       # starts 8 ranks itself (torch.distributed.run, 127.0.0.1)
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
         bench.py --gpus N --steps K --warmup W  # the driver's form: ranks already exist
`n_gpus` in the JSON line is the world size RCCL actually formed; --gpus N on a box with fewer GPUs, or a
mismatch between --gpus and WORLD_SIZE, is an error (exit code 2), never a silent 1-GPU run.

A plain run sets up, warms up, times --steps steps and prints the headline line (metric, value, unit, dtype, ms_per_step, config).
Everything else the line can carry -- roofline figures (HIP-event kernel timers inside the timed region, extra eager steps after a
graph-replayed region), the synthetic-pose error, the CPU baseline, the parity leg and the secondary configurations -- is measured
only with --full.
"""
import argparse
import json
import os
import socket
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import torch
import torch.distributed as dist

H, W = 720, 540                      # config/mapfree.yaml:7-8, compute.py:42
FP32_MFMA_PEAK_TFLOPS = 157.3        # /opt/skills/guides/MI355X_MICROARCH.md (v_mfma_f32_32x32x2_f32 / 16x16x4_f32)
BF16_MFMA_PEAK_TFLOPS = 2500.0       # same guide: ~2.5 PF dense bf16 (v_mfma_f32_32x32x16_bf16); never the 2:1-sparsity figure
HBM_PEAK_GBS = 8000.0                # same guide: 8.0 TB/s spec (6.3 TB/s achievable)
CONFIGS = ("sg_pnp", "loftr_emat", "rpr_train")
# v_exp_f32 is a quarter-rate VALU op: 256 CUs x 4 SIMDs x 16 lanes / 4 per clock at the 2.4 GHz peak engine clock
EXP_PEAK_GOPS = 256 * 4 * 16 / 4 * 2.4


def split_products():
    """partial products (MFMAs) per fp32 multiply-add of the operand-splitting kernels: 3 for HIP.SPLIT = 'f16x2' (the default), 6 for 'bf16x3'"""
    from mapfree_reloc_amd import options
    return 3.0 if options.get("SPLIT") == "f16x2" else 6.0


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", choices=CONFIGS, default="sg_pnp")
    ap.add_argument("--batch", type=int, default=0, help="image pairs per GPU per step (default 32 for sg_pnp, 16 for loftr_emat)")
    ap.add_argument("--cpu-pairs", type=int, default=0, help="pairs timed for the CPU baseline (rank 0, N=1); default 6 / 3")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-all-cores", action="store_true", help="skip the whole-host leg of the CPU baseline (the secondary lines of the default run do)")
    ap.add_argument("--cpu-threads", type=int, default=16, help="host threads for the all-threads CPU baseline figure")
    ap.add_argument("--cpu-baseline-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--cpu-out", default="", help=argparse.SUPPRESS)
    ap.add_argument("--no-kernel-timer", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--verbose", action="store_true")
    ap.add_argument("--full", action="store_true", help="also measure what the headline does not need: roofline (live kernel timers), synthetic-pose "
                    "error, CPU baseline, parity vs the oracle and, for the default configuration, the secondary configurations")
    ap.add_argument("--dump-outputs", default="", metavar="DIR", help="after the timed steps, write the outputs of the last timed step as "
                    "DIR/<name>.npy (float32 / float64, at most 64 MB in all; rank 0)")
    ap.add_argument("--no-secondary", action="store_true", help="default run (sg_pnp, 1 GPU): do not append the loftr_emat and rpr_train "
                    "bench lines under \"secondary\"")
    ap.add_argument("--secondary-budget", type=float, default=110.0, help="seconds each secondary config may take (child process)")
    ap.add_argument("--graph", type=int, default=0, help="sg_pnp: 1 = replay the whole step from one captured HIP graph (inputs copied into the "
                    "graph's static buffers every step), 0 = eager launches (default: at 8-32 pairs per step the eager step is GPU-bound, "
                    "measured 699 vs 694 pairs/s).  With 1 the roofline kernels are timed with HIP events over extra eager steps AFTER the "
                    "timed region (events cannot be recorded inside a replay).")
    ap.add_argument("--overlap", type=int, default=1, help="1 (default): the RANSAC stage of step i runs on a second HIP stream under the matcher of step i + 1 "
                    "(pipeline.SolverOverlap; every step's work is inside the timed region, which ends with a join + synchronize), 0: one stream")
    ap.add_argument("--hip-opt", action="append", default=[], metavar="NAME=VALUE", help="set a declared kernel-selection option (mapfree_reloc_amd/options.py), e.g. CONV_KERNEL=exact, RPR_CONV=miopen; repeatable")
    ap.add_argument("--rpr-opts", default="siamese,graph", help="rpr_train only, comma list: siamese (TRAINING.SIAMESE_BATCH: both images of a pair in one "
                    "encoder pass, BatchNorm statistics per view = the arithmetic of the reference's two encoder calls), graph (TRAINING.GRAPH_STEP: "
                    "forward + loss + backward replayed from one HIP graph), channels_last, fp32; 'none' = two encoder calls, eager launches")
    a = ap.parse_args(argv)
    if not a.full:                                # the side measurements below are part of --full only
        a.no_kernel_timer, a.no_cpu_baseline, a.no_secondary = True, True, True
    if a.batch <= 0:
        a.batch = {"sg_pnp": 32, "loftr_emat": 16, "rpr_train": 10}[a.config]
    if a.cpu_pairs <= 0:
        a.cpu_pairs = {"sg_pnp": 6, "loftr_emat": 3, "rpr_train": 4}[a.config]
    return a


class KernelTimer:
    """HIP-event timing of one kernel family on torch's current stream (the stream the C-ABI
    launches on), live inside the timed region."""

    def __init__(self, every=1):
        # HIP event pairs cost ~0.2 ms each on this stack: frequently launched kernels are sampled
        self.events, self.enabled, self.every, self.count = [], False, every, 0

    def wrap(self, fn):
        def inner(*a, **k):
            self.count += 1
            if not self.enabled or (self.count % self.every):
                return fn(*a, **k)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn(*a, **k)
            e1.record()
            self.events.append((e0, e1))
            return r
        return inner

    def mean_ms(self):
        if not self.events:
            return None
        return float(np.mean([a.elapsed_time(b) for a, b in self.events]))


# ----------------------------------------------------------------------------------------------------------------
# CPU baseline + parity legs (the ONLY places that touch oracle/)
# ----------------------------------------------------------------------------------------------------------------
def cpu_baseline(config, n_pairs, seeds, threads, out_path=""):
    """the oracle (CPU restatement of the reference path: PyTorch-CPU networks + C solvers, oracle/pipeline_ref.py)
    timed on this box's host cores -- a reported baseline, never the product path.  Two figures: `threads` host
    threads over the first n_pairs pairs, and ONE thread on the first pair (the reference itself is a single
    process; SURVEY.md 8d asks for both).  The per-pair oracle results go to `out_path` for the parity leg."""
    host = os.cpu_count() or 1
    cores = max(1, min(threads, host))
    if config == "rpr_train":
        return rpr_cpu_baseline(n_pairs, cores, host)
    from oracle import pipeline_ref as PR
    from mapfree_reloc_amd import images as IM
    prs = [IM.synthetic_pair(s, H, W) for s in seeds[:n_pairs]]

    def run(p, s):
        if config == "sg_pnp":
            return PR.sg_pnp_pair(p["img0"], p["img1"], p["depth0"], p["K"], p["K"], s)
        return PR.loftr_emat_pair(p["img0"], p["img1"], p["depth0"], p["depth1"], p["K"], p["K"], s)
    torch.set_num_threads(cores)
    run(prs[0], seeds[0])                                      # weights / libraries loaded outside the timed region
    t0 = time.perf_counter()
    res = [run(p, s) for p, s in zip(prs, seeds)]
    dt = time.perf_counter() - t0
    if not out_path:                                            # a child of the all-cores leg: only its multi-thread rate is used
        return dict(value=round(n_pairs / dt, 4), unit="image-pairs/s", cores=cores, kind="port")
    torch.set_num_threads(1)
    t1 = time.perf_counter()
    run(prs[0], seeds[0])
    d1 = time.perf_counter() - t1
    if out_path:
        np.savez(out_path, seeds=np.asarray(seeds[:n_pairs]), **{f"{k}{i}": np.asarray(r[k]) for i, r in enumerate(res)
                                                               for k in ("pts", "status", "R", "t", "n_inliers")})
    nets = "SuperPoint+SuperGlue" if config == "sg_pnp" else "LoFTR"
    solver = "C PnP oracle" if config == "sg_pnp" else "C E-mat + scale oracle"
    return dict(value=round(n_pairs / dt, 4), unit="image-pairs/s", cores=cores, kind="port",
                sample=f"{n_pairs} synthetic 540x720 pairs, PyTorch-CPU fp32 {nets} ({cores} threads) + {solver}, {dt:.1f}s; "
                       f"1 pair on 1 thread, {d1:.1f}s", single_thread_value=round(1.0 / d1, 4), host_cores=host)


def cpu_baseline_subprocess(config, n_pairs, threads, out_path, budget_s=300, all_cores=True):
    """run the CPU baseline in a child process (no GPU visible) with a hard time budget so that it can never
    block the bench line.  Besides the `threads`-thread and the 1-thread figures of the child, the WHOLE host is measured too:
    host_cores // threads children of `threads` threads each work on their own pairs at the same time (the reference is one
    process per run; pairs are independent, so this is how its CPU path would use every core) -> `all_cores_value`."""
    import subprocess
    env = dict(os.environ, OMP_NUM_THREADS=str(threads), MKL_NUM_THREADS=str(threads), HIP_VISIBLE_DEVICES="")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    cmd = lambda n, out: [sys.executable, os.path.abspath(__file__), "--cpu-baseline-only", "--config", config, "--cpu-pairs", str(n),
                          "--cpu-threads", str(threads), "--cpu-out", out]

    def last_json(text):
        for ln in reversed(text.strip().splitlines()):
            if ln.startswith("{"):
                return json.loads(ln)
        return None
    try:
        r = subprocess.run(cmd(n_pairs, out_path), capture_output=True, text=True, timeout=budget_s, env=env)
        res = last_json(r.stdout)
        if res is None:
            return {"value": None, "error": (r.stderr or "no output")[-300:]}
    except subprocess.TimeoutExpired:
        return {"value": None, "error": f"CPU baseline exceeded its {budget_s}s budget"}
    host = os.cpu_count() or 1
    k = host // max(threads, 1)
    if k >= 2 and config != "rpr_train" and all_cores:
        try:
            t0 = time.perf_counter()
            procs = [subprocess.Popen(cmd(1, ""), stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, env=env) for _ in range(k)]
            vals = []
            for p in procs:
                out, _ = p.communicate(timeout=budget_s)
                j = last_json(out)
                if j and j.get("value"):
                    vals.append(j["value"])
            res.update(all_cores_value=round(float(sum(vals)), 3), all_cores=len(vals) * threads,
                       all_cores_sample=f"{len(vals)} concurrent processes x {threads} threads, 1 pair each (each process's own pairs/s, summed), "
                                        f"{time.perf_counter() - t0:.1f}s wall")
        except Exception as e:     # never lose the bench line over the all-cores side figure
            res["all_cores_error"] = str(e)[:200]
    return res


def parity_leg(wl, oracle_npz, dev):
    """whole HIP pipeline vs whole CPU-oracle pipeline on the CPU baseline's pairs: per pair, is the match set
    identical, pose delta, inlier-count delta (north-star bar: 1e-4 rad / 1e-4 m).  -> config.parity"""
    from oracle import pipeline_ref as PR
    from mapfree_reloc_amd import images as IM
    z = np.load(oracle_npz)
    seeds = [int(s) for s in z["seeds"]]
    sb = IM.synthetic_batch(seeds, H, W)
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in sb.items()}
    out = wl.run(d)
    wl.pipe.join()
    torch.cuda.synchronize()
    o = {k: v.cpu().numpy() for k, v in out.items() if isinstance(v, torch.Tensor)}
    recs = []
    for i in range(len(seeds)):
        ref = {k: z[f"{k}{i}"] for k in ("pts", "status", "R", "t", "n_inliers")}
        ref["status"], ref["n_inliers"] = int(ref["status"]), int(ref["n_inliers"])
        n = int(o["n_corr"][i])
        recs.append(PR.compare_pair(ref, np.concatenate([o["pts0"][i, :n], o["pts1"][i, :n]], 1), o["R"][i], o["t"][i],
                                    o["n_inliers"][i], o["status"][i]))
    s = PR.summarize(recs)
    s["against"] = "oracle/pipeline_ref.py (CPU restatement of the reference path) on the cpu_baseline pairs; full census: profiles/r05_parity_census_hard.json, r05_parity_census_hard2.json"
    s["census"] = census_summary()
    return s


def census_summary():
    """the committed wide census (tools/parity_census.py on an MI355X, whole HIP pipeline vs whole CPU-oracle pipeline, nothing masked) in
    a few numbers per configuration; the live comparison above covers only the pairs the CPU baseline was timed on"""
    keep = ("pairs", "status_agree", "pose_within_bar", "inlier_count_equal", "inlier_index_sets_compared", "inlier_index_sets_identical",
            "min_inlier_set_jaccard_q64", "median_inlier_fraction", "max_rot_rad", "max_trans_m")
    out = {}
    for tag, fn in (("hard1", "r05_parity_census_hard.json"), ("hard2", "r05_parity_census_hard2.json")):
        try:
            d = json.load(open(os.path.join(ROOT, "profiles", fn)))
            out[tag] = {"scenes": d.get("scenes"), "file": "profiles/" + fn,
                        **{k: {q: v["summary"][q] for q in keep if q in v["summary"]} for k, v in d.items() if isinstance(v, dict) and "summary" in v}}
        except Exception as e:      # never lose the bench line over a side note
            out[tag] = {"error": str(e)[:120]}
    return out


# ----------------------------------------------------------------------------------------------------------------
# workloads
# ----------------------------------------------------------------------------------------------------------------
class SgPnpWorkload:
    name = "sg_pnp"

    @property
    def dtype(self):
        """derived from the routing of THIS run (which objects the networks built), not from a fixed text"""
        f16 = split_products() == 3.0
        pipe = getattr(self, "pipe", None)                  # (no instance: the routing the options select by default)
        own = lambda obj, name: (getattr(obj, name, None) is not None) if pipe is not None else f16
        sp, sg = getattr(pipe, "sp", None), getattr(pipe, "sg", None)
        arith = ("on the f16 matrix cores with every fp32 operand carried as TWO f16 terms (xh = rne_f16(x), xl = rne_f16((x - xh) 2^11); weights pre-scaled per "
                 "output feature; 3 partial products, fp32 accumulate: 2^-24 relative per operand for 2^-12 <= |x| <= 65504 -- range guarded by a device flag, "
                 "out-of-range batches are re-run in bf16x3 -- error vs fp64 = the exact-fp32 MFMA's class, profiles/r05_f16x2_probe.jsonl)") if f16 else \
                "as 3 x bf16 exact operand splits (6 partial products, error = fp32 class)"
        score = "mfr_gemm_f16x2_batched (same two-term arithmetic)" if own(sg, "score_gemm") else "the library's batched fp32 GEMM"
        head = "mfr_conv_igemm_f16x2 (same two-term arithmetic)" if own(sp, "head_pb") else "the library's fp32 convolution"
        return (f"f32 in / f32 accumulate; matrix products of the 3x3 convolutions, attention, the transformer's linear layers and SuperPoint's 1x1 descriptor head {arith}; "
                f"SuperGlue's score matrix through {score}; the 1x1 detector head through {head}; softmax / Sinkhorn / NMS in f32; f64 solver")
    metric = "image-pairs/sec @ 540x720 (SuperPoint+SuperGlue + PnP w/ depth)"
    workload = "configs[1]: SuperPoint+SuperGlue matching + PnP w/ depth, 540x720"

    def __init__(self, dev, B, timers, graph=False, overlap=False):
        from mapfree_reloc_amd.pipeline import SuperGluePnPPipeline
        self.B = B
        self.pipe = SuperGluePnPPipeline(dev, seed=0, graph=graph, overlap_solver=overlap)
        self.att_timer, self.conv_timer, self.sk_timer = KernelTimer(every=9), KernelTimer(every=1), KernelTimer(every=1)
        self.gemm_timer = KernelTimer(every=6)
        if timers:
            for L in self.pipe.sg.layers:                       # the 512 -> 512 (+ReLU) layer of every GNN block, sampled
                L["lin1"] = self.gemm_timer.wrap(L["lin1"])
            self.pipe.sg.attention = self.att_timer.wrap(self.pipe.sg.attention)
            self.pipe.sg.sinkhorn_match = self.sk_timer.wrap(self.pipe.sg.sinkhorn_match)
            sp_conv, timed_conv = self.pipe.sp._conv, self.conv_timer.wrap(self.pipe.sp._conv)
            self.pipe.sp._conv = lambda x, name, **kw: (timed_conv if name == "conv1b" else sp_conv)(x, name, **kw)
            # round 5: conv1a is fused into the conv1b launch (options FUSED_CONV1): that launch is the dominant kernel then
            fused = self.pipe.sp._conv1ab
            timed_fused = self.conv_timer.wrap(fused)
            self.pipe.sp._conv1ab = lambda im: (timed_fused(im) if self.fused_c1 else fused(im))
        self.fused_c1 = bool(getattr(self.pipe.sp, "fused_conv1", False)) and getattr(self.pipe.sp.upk.get("conv1b"), "split", "") == "f16x2"
        self.kp_sum, self.kp_cnt = 0.0, 0

    def timers(self):
        return [self.att_timer, self.conv_timer, self.sk_timer, self.gemm_timer]

    def run(self, d):
        return self.pipe(d["images"], d["depth0"], d["K0"], d["K1"], d["pair_ids"])

    def config(self, out):
        c = {"max_keypoints": 1024, "sinkhorn_iters": 20, "pnp_iters": 1000}
        if "n_kpts" in out:
            c["mean_keypoints_per_image_last_step"] = float(out["n_kpts"].float().mean())
        return c

    def roofline(self, out):
        B = self.B
        att_ms, conv_ms = self.att_timer.mean_ms(), self.conv_timer.mean_ms()
        # attention: 2B images x 4 heads x (QK^T + PV) = 2 * 2*n*n*64 flops each, n = the keypoints the step really had
        nk = float(out["n_kpts"].float().mean()) if "n_kpts" in out else 1024.0
        att_flops = float((2.0 * 2.0 * out["n_kpts"].double() ** 2 * 64 * 4).sum()) if "n_kpts" in out else 2 * B * 4 * 2 * (2.0 * 1024 * 1024 * 64)
        att_tf = att_flops / (att_ms * 1e-3) / 1e12 if att_ms else None
        # Winograd F(2x2,3x3) conv1b (64 -> 64 channels, 2B images, HxW): 16 GEMMs of [Cout x Cin] x [Cin x tiles] = the fp32
        # multiply-adds of the layer in the Winograd domain (a direct 3x3 convolution is 2.25x that).  The kernel evaluates each
        # fp32 product as THREE f16 (f16x2) or SIX bf16 (bf16x3) partial products on the 16-bit matrix cores, fp32 accumulate, so the
        # flops it EXECUTES -- what the roofline prices against the dense 16-bit MFMA peak -- are 3x / 6x the fp32 figure.  (With conv1a fused
        # in, the launch also does that layer's 9 fp32 FMAs per output on the vector ALU: 1.4 % of the fp32-equivalent work, not counted.)
        tiles = ((H + 1) // 2) * ((W + 1) // 2)
        conv_fp32 = 16 * 2.0 * 64 * 64 * tiles * 2 * B
        conv_flops = split_products() * conv_fp32
        conv_direct = 2.0 * 9 * 64 * 64 * H * W * 2 * B
        achieved = conv_flops / (conv_ms * 1e-3) / 1e12 if conv_ms else None
        eq = conv_fp32 / (conv_ms * 1e-3) / 1e12 if conv_ms else None
        att_exec = split_products() * att_tf if att_tf else None
        nprod = int(split_products())
        kname = ("wino_split_c1_kernel: SuperPoint conv1a (1->64 ch, computed into LDS) + conv1b launch" if self.fused_c1 else "wino_split_p8_kernel conv1b launch")
        direct_tf = conv_direct / (conv_ms * 1e-3) / 1e12 if conv_ms else None
        return {"kernel": f"{kname} (dominant kernel: fused Winograd F(2x2,3x3) convolution on the 16-bit matrix cores at "
                          f"fp32 accuracy, {'f16x2' if nprod == 3 else 'bf16x3'} operand split, 64->64 ch, pooled output; eight wavefronts per workgroup, two per SIMD)",
                "bound": "mfma", "achieved": round(direct_tf, 1) if direct_tf else None, "peak": BF16_MFMA_PEAK_TFLOPS,
                "unit": "TFLOP/s", "frac": round(direct_tf / BF16_MFMA_PEAK_TFLOPS, 4) if direct_tf else None,
                "mfma_pipe_frac": round(achieved / BF16_MFMA_PEAK_TFLOPS, 4) if achieved else None, "executed_tflops": round(achieved, 1) if achieved else None,
                "traffic": _traffic("conv1ab" if self.fused_c1 else "conv1b", B), "avg_launch_ms": round(conv_ms, 4) if conv_ms else None,
                "launches_timed": len(self.conv_timer.events), "flops_per_launch": conv_direct, "executed_flops_per_launch": conv_flops,
                "note": "achieved / frac = ALGORITHMIC work (SURVEY 8d: the direct 3x3 convolution's multiply-adds, 2 x 9 x 64 x 64 x H x W x images) / launch time against the "
                        f"DENSE f16 / bf16 MFMA peak; mfma_pipe_frac = the 16-bit matrix-core flops the kernel EXECUTES ({nprod} partial products per fp32 multiply-add of the "
                        "16 Winograd GEMMs: Winograd does 1 / 2.25 of the direct multiply-adds, the operand split 3 x) against the same peak; fp32_equivalent = the Winograd-domain "
                        "fp32 multiply-adds (what the layer delivers) against the fp32 MFMA peak.  Both fractions are against the NOMINAL 2.5 PFLOP/s (2.4 GHz): measured in round 6, a "
                        "dense f16 MFMA stream on random data is power-limited at ~0.92 busy x GHz ~ 960 TFLOP/s executed (the direct-convolution and linear-layer launches of this "
                        "step sit on that line; DESIGN.md 4.4, profiles/r06_pmc_dconv_*.json)",
                "fp32_equivalent": {"tflops": round(eq, 2) if eq else None, "flops_per_launch": conv_fp32,
                                    "vs_fp32_mfma_peak": round(eq / FP32_MFMA_PEAK_TFLOPS, 4) if eq else None,
                                    "round2_exact_fp32_kernel": "8.63 ms / launch, 94.5 TFLOP/s, 0.60 of the fp32 MFMA peak (BENCH_r02)"},
                "other_kernels": [self._gemm_line(), {"kernel": ("sg_attention_f16x2_p_kernel (softmax(QK^T/8)V on the f16 matrix cores, two-term operands with main + correction accumulators" if nprod == 3 else "sg_attention_bf16x3_p_kernel (softmax(QK^T/8)V on the bf16 matrix cores, 3-way split operands") + ", 256 queries per workgroup, score product one tile ahead of the softmax)", "bound": "mfma",
                                   "achieved": round(att_tf, 1) if att_tf else None,
                                   "peak": BF16_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(att_tf / BF16_MFMA_PEAK_TFLOPS, 4) if att_tf else None,
                                   "mfma_pipe_frac": round(att_exec / BF16_MFMA_PEAK_TFLOPS, 4) if att_exec else None, "executed_tflops": round(att_exec, 1) if att_exec else None,
                                   "avg_launch_ms": round(att_ms, 4) if att_ms else None, "launches_timed": len(self.att_timer.events),
                                   "mean_keypoints_per_image": round(nk, 1)},
                                  self._sinkhorn_line(out)]}

    def _gemm_line(self):
        """the transformer's linear layers, on the 512 -> 512 (+ReLU) layer of a GNN block: M = 2B x 1024 rows"""
        ms = self.gemm_timer.mean_ms()
        M = 2 * self.B * 1024
        fp32 = 2.0 * M * 512 * 512
        ex = split_products() * fp32 / (ms * 1e-3) / 1e12 if ms else None
        return {"kernel": f"gemm_split_d_kernel, the 512 -> 512 + ReLU layer of a GNN block (mfr_gemm_{'f16x2' if split_products() == 3.0 else 'bf16x3'}: persistent workgroups, W by LDS-DMA, split operands)",
                "bound": "mfma", "achieved": round(ex / split_products(), 1) if ex else None, "peak": BF16_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                "frac": round(ex / split_products() / BF16_MFMA_PEAK_TFLOPS, 4) if ex else None,
                "mfma_pipe_frac": round(ex / BF16_MFMA_PEAK_TFLOPS, 4) if ex else None, "executed_tflops": round(ex, 1) if ex else None,
                "avg_launch_ms": round(ms, 4) if ms else None, "launches_timed": len(self.gemm_timer.events), "flops_per_launch": fp32,
                "executed_flops_per_launch": split_products() * fp32}

    def _sinkhorn_line(self, out):
        """log-Sinkhorn + mutual arg-max stage.  Its binding resource is the transcendental ALU, not HBM: 2 x iters x (n+1)^2
        exp per pair against 4.2 MB of algorithmic reads -- so the line carries the exp rate against the quarter-rate VALU peak
        and, for reference, the algorithmic-bytes rate (which no schedule can bring near the HBM roofline)."""
        sk_ms = self.sk_timer.mean_ms()
        iters = 20
        n0 = out["n_kpts"][0::2].double() + 1 if "n_kpts" in out else torch.full((self.B,), 1025.0)
        n1 = out["n_kpts"][1::2].double() + 1 if "n_kpts" in out else torch.full((self.B,), 1025.0)
        n_exp = float((2.0 * iters * n0 * n1).sum())         # algorithmic: one per entry for the row sums, one for the column sums (round 5's four-row column update executes 1.5)
        alg_bytes = float((4.0 * (n0 - 1) * (n1 - 1)).sum())
        g = n_exp / (sk_ms * 1e-3) / 1e9 if sk_ms else None
        return {"kernel": "(sg_sweep_kernel + sg_colmerge_kernel) x iters + sg_match (mfr_sg_sinkhorn_match: log-Sinkhorn, one sweep over S per iteration, mutual arg-max, threshold, compaction)",
                "bound": "alu (v_exp_f32, quarter rate)", "achieved": round(g, 1) if g else None, "peak": EXP_PEAK_GOPS, "unit": "Gexp/s",
                "frac": round(g / EXP_PEAK_GOPS, 4) if g else None, "avg_launch_ms": round(sk_ms, 4) if sk_ms else None,
                "launches_timed": len(self.sk_timer.events), "exp_per_launch": n_exp,
                "hbm_view": {"algorithmic_bytes_per_launch": alg_bytes, "achieved_gbs": round(alg_bytes / (sk_ms * 1e-3) / 1e9, 1) if sk_ms else None,
                             "frac_of_hbm_peak": round(alg_bytes / (sk_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 5) if sk_ms else None,
                             "note": "S is read once algorithmically; the implementation streams the MALL-resident matrix 22 times (once per iteration + the two arg-max passes)"}}


class LoftrEmatWorkload:
    name = "loftr_emat"

    @property
    def dtype(self):
        """derived from the routing of THIS run (LoFTRHIP.igemm / .sim_gemm / the split of its packed layers)"""
        pipe = getattr(self, "pipe", None)                  # (no instance: the routing the options select by default)
        f16 = split_products() == 3.0
        own_rest = (bool(pipe.loftr.igemm) and pipe.loftr.sim_gemm is not None) if pipe is not None else f16
        arith = ("on the f16 matrix cores with every fp32 operand carried as two f16 terms (3 partial products, fp32 accumulate, error = fp32 class: "
                 "profiles/r05_f16x2_probe.jsonl; |x| <= 65504 guarded by a device flag, out-of-range batches are re-run in bf16x3)") if f16 else \
                "as 3 x bf16 exact operand splits (6 partial products, error = fp32 class)"
        rest = ("the strided 3x3 / 7x7 / 1x1 convolutions through mfr_conv_igemm_f16x2 and the coarse similarity product through mfr_gemm_f16x2_batched (same two-term arithmetic)"
                if own_rest else "the strided 3x3 / 7x7 / 1x1 convolutions and the similarity product through the library's fp32 kernels")
        return (f"f32 in / f32 accumulate; 3x3 stride-1 convolutions, the transformers' linear layers and the fine-stage products {arith}; {rest}; "
                "linear attention, LayerNorm, dual softmax and the fine expectation in f32 (own kernels); f64 solver")
    metric = "image-pairs/sec @ 540x720 (LoFTR + E-mat RANSAC w/ scale from depth)"
    workload = "configs[2]: LoFTR coarse-to-fine matching + Essential-matrix RANSAC + metric scale, 540x720 (padded to 544)"

    def __init__(self, dev, B, timers, overlap=False):
        from mapfree_reloc_amd.pipeline import LoFTREmatPipeline
        self.B = B
        self.pipe = LoFTREmatPipeline(dev, seed=0, overlap_solver=overlap)
        self.conv_timer, self.cm_timer = KernelTimer(every=1), KernelTimer(every=1)
        if timers:
            lo = self.pipe.loftr
            c0, ct = lo._c, self.conv_timer.wrap(lo._c)
            lo._c = lambda x, name, *a, **kw: (ct if name == "l1out2.0" else c0)(x, name, *a, **kw)
            lo.coarse_match_features = self.cm_timer.wrap(lo.coarse_match_features)

    def timers(self):
        return [self.conv_timer, self.cm_timer]

    def run(self, d):
        return self.pipe(d["images"], d["depth0"], d["depth1"], d["K0"], d["K1"], d["pair_ids"])

    def config(self, out):
        return {"coarse_tokens_per_image": 90 * 68, "emat_iters": 1000, "pix_threshold": 2.0, "scale_threshold": 0.1}

    def roofline(self, out):
        B = self.B
        conv_ms, cm_ms = self.conv_timer.mean_ms(), self.cm_timer.mean_ms()
        # layer1_outconv2.0: 196 -> 196 channels at 1/2 resolution (360 x 272), 2B images: the largest single launch of the path
        # (algorithmic flops: the 196 real output channels; the kernel also multiplies the 28 zero-padded ones of its 7th block)
        tiles = (360 // 2) * (272 // 2)
        conv_flops = 16 * 2.0 * 196 * 196 * tiles * 2 * B
        achieved = conv_flops / (conv_ms * 1e-3) / 1e12 if conv_ms else None
        # dual-softmax coarse matching: algorithmic bytes = the two coarse feature maps in (2 x 6120 x 256 f32 = 12.5 MB/pair)
        L = 90 * 68
        cm_bytes = 2.0 * L * 256 * 4 * B
        cm_gbs = cm_bytes / (cm_ms * 1e-3) / 1e9 if cm_ms else None
        cm_flops = 2.0 * L * L * 256 * B                      # the similarity contraction (19.2 GFLOP/pair)
        cm_tf = cm_flops / (cm_ms * 1e-3) / 1e12 if cm_ms else None
        cm_impl_bytes = (3.0 * L * L * 4 + 2.0 * L * 256 * 4) * B   # as implemented: S written once, swept twice, features in
        cm_impl_gbs = cm_impl_bytes / (cm_ms * 1e-3) / 1e9 if cm_ms else None
        # priced three ways: ALGORITHMIC = the direct 3x3 convolution's multiply-adds over the 196 real channels -> achieved / frac;
        # fp32_equivalent = the 16 Winograd GEMMs' multiply-adds (1 / 2.25 of the direct ones); EXECUTED = split_products() x that, incl. the
        # zero padding the kernel multiplies (Cin 196 -> 208 = 13 K steps of 16, Cout 196 -> 256 = 4 groups of 64: x 1.39) -> mfma_pipe_frac
        conv_direct = 2.0 * 9 * 196 * 196 * 360 * 272 * 2 * B
        direct_tf = conv_direct / (conv_ms * 1e-3) / 1e12 if conv_ms else None
        from mapfree_reloc_amd import options as _opt
        is_direct = _opt.get("CONV_KERNEL") in ("auto", "direct") and _opt.get("SPLIT") == "f16x2"     # nets/conv.py: which kernel ran the layer
        if is_direct:
            # round 6: the direct halo-staged kernel (csrc/conv_direct.hip): EXECUTED = 3 partial products x the direct multiply-adds, incl. the padding it
            # multiplies (Cin 196 -> 208, Cout 196 -> 256 = 2 groups of 128, 360 columns -> 12 tiles of 32 = 384)
            exe = 3.0 * direct_tf * (208.0 * 256.0) / (196.0 * 196.0) * (384.0 / 360.0) if direct_tf else None
            kname = ("conv_direct_f16x2_kernel<2, 4, false> layer1_outconv2.0 launch, 196->196 ch at 360x272 (dominant kernel: the 3x3 / stride-1 convolutions of the ResNet-FPN "
                     "backbone as direct implicit GEMMs with an LDS-staged halo tile on the f16 matrix cores at fp32 accuracy; the family is the largest share of the step's GPU "
                     "time, profiles/r06_bench_loftr_emat_kernel_stats.csv)")
            knote = ("mfma_pipe_frac = the matrix-core flops EXECUTED (3 partial products per fp32 multiply-add of the direct convolution, channel / tile padding included) at the "
                     "NOMINAL 2.4 GHz peak; under this kernel the chip runs at its power limit, ~1.25 GHz with the matrix pipe 62-74 % busy (profiles/r06_pmc_dconv_*.json)")
        else:
            exe = split_products() * achieved * (208.0 * 256.0) / (196.0 * 196.0) if achieved else None
            kname = ("wino_split_p8_kernel layer1_outconv2.0 launch, 196->196 ch at 360x272 (dominant kernel: fused Winograd F(2x2,3x3) convolutions of the "
                     "ResNet-FPN backbone on the 16-bit matrix cores at fp32 accuracy; the family is the largest share of the step's GPU time, profiles/r06_bench_loftr_emat_kernel_stats.csv)")
            knote = f"mfma_pipe_frac = the matrix-core flops EXECUTED ({int(split_products())} partial products per fp32 multiply-add of the 16 Winograd GEMMs, channel padding included)"
        lo = self.pipe.loftr
        sim_f16 = lo.sim_gemm is not None
        cm_peak = BF16_MFMA_PEAK_TFLOPS if sim_f16 else FP32_MFMA_PEAK_TFLOPS
        return {"kernel": kname,
                "bound": "mfma", "achieved": round(direct_tf, 1) if direct_tf else None, "peak": BF16_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                "frac": round(direct_tf / BF16_MFMA_PEAK_TFLOPS, 4) if direct_tf else None,
                "mfma_pipe_frac": round(exe / BF16_MFMA_PEAK_TFLOPS, 4) if exe else None, "executed_tflops": round(exe, 1) if exe else None,
                "traffic": _traffic("loftr_l1out2", B),
                "avg_launch_ms": round(conv_ms, 4) if conv_ms else None, "launches_timed": len(self.conv_timer.events), "flops_per_launch": conv_direct,
                "note": "achieved / frac = ALGORITHMIC work (direct 3x3 multiply-adds over the 196 real channels) / launch time against the dense f16 / bf16 MFMA peak; " + knote,
                "fp32_equivalent": {"tflops": round(achieved, 2) if achieved else None, "flops_per_launch": conv_flops,
                                    "vs_fp32_mfma_peak": round(achieved / FP32_MFMA_PEAK_TFLOPS, 4) if achieved else None},
                "other_kernels": [{"kernel": "dual-softmax coarse matching (similarity product + row/col softmax statistics + mutual-NN selection)",
                                   "bound": ("mfma + hbm (similarity product on the f16 matrix cores, two-term operands: mfr_gemm_f16x2_batched; then streaming sweeps over the materialised S)"
                                             if sim_f16 else "mfma + hbm (library fp32 similarity GEMM, then streaming sweeps over the materialised S)"),
                                   "achieved": round(cm_tf, 2) if cm_tf else None, "peak": cm_peak, "unit": "TFLOP/s",
                                   "frac": round(cm_tf / cm_peak, 4) if cm_tf else None,
                                   "mfma_pipe_frac": round(split_products() * cm_tf / cm_peak, 4) if (cm_tf and sim_f16) else None,
                                   "avg_launch_ms": round(cm_ms, 4) if cm_ms else None, "flops_per_launch": cm_flops,
                                   "hbm_view": {"implemented_bytes_per_launch": cm_impl_bytes,
                                                "implemented_gbs": round(cm_impl_gbs, 1) if cm_impl_gbs else None,
                                                "implemented_frac_of_hbm_peak": round(cm_impl_gbs / HBM_PEAK_GBS, 4) if cm_impl_gbs else None,
                                                "algorithmic_bytes_per_launch": cm_bytes,
                                                "algorithmic_frac_of_hbm_peak": round(cm_gbs / HBM_PEAK_GBS, 5) if cm_gbs else None},
                                   "note": "time = the contraction + the passes over S (150 MB/pair: written once, swept by the statistics and the selection kernels); algorithmic "
                                           "bytes (features in, 12.5 MB/pair) are not what bounds it -- both fractions are given; the contraction is priced against the peak of the pipe it runs on"}]}


# ----------------------------------------------------------------------------------------------------------------
# configs[4]: bf16 training step of the regression model
# ----------------------------------------------------------------------------------------------------------------
RPR_H, RPR_W = 360, 270              # config/regression/mapfree/3d3d.yaml:32-33
RPR_3D3D = ["MODEL", "Regression", "ENCODER.TYPE", "ResUNet", "ENCODER.BLOCK_TYPE", 1, "ENCODER.NUM_BLOCKS", "3-3-3",
            "ENCODER.NOT_CONCAT", False, "ENCODER.NUM_OUT_LAYERS", 32, "AGGREGATOR.TYPE", "CorrelationVolumeWarping",
            "AGGREGATOR.POSITION_ENCODER", True, "AGGREGATOR.MAX_SCORE_CHANNEL", True, "HEAD.TYPE", "ProcrustesDeepResBlock",
            "HEAD.ADD_BASIS", True, "HEAD.AVG_POOL", True, "TRAINING.LR", 1e-4, "TRAINING.ROT_LOSS", "rot_angle_loss",
            "TRAINING.TRANS_LOSS", "trans_l1_loss", "TRAINING.LAMBDA", 1.0, "DATASET.HEIGHT", RPR_H, "DATASET.WIDTH", RPR_W]


def rpr_cfg(precision, opts=()):
    from mapfree_reloc_amd.config import get_cfg_defaults
    cfg = get_cfg_defaults()
    cfg.merge_from_list(RPR_3D3D + ["TRAINING.PRECISION", "fp32" if "fp32" in opts else precision, "TRAINING.SIAMESE_BATCH", "siamese" in opts,
                                    "TRAINING.CHANNELS_LAST", "channels_last" in opts, "TRAINING.GRAPH_STEP", "graph" in opts])
    return cfg


def rpr_cpu_baseline(n_pairs, cores, host):
    """the same training step on the host: this package's model with the aggregator swapped for the oracle's MATERIALISED
    correlation volume (oracle/rpr_ref.py = the reference's aggregator.py:42-116 arithmetic), PyTorch-CPU fp32"""
    from oracle import rpr_ref
    from mapfree_reloc_amd.regression.train import SyntheticPairs, Trainer
    torch.set_num_threads(cores)
    cfg = rpr_cfg("fp32")
    src = SyntheticPairs(n_pairs, RPR_H, RPR_W, "cpu", seed=0)
    tr = Trainer(cfg, "cpu")
    tr.model.aggregator = rpr_ref.MaterialisedAggregator(tr.model.aggregator)
    b0, b1 = src.batch(), src.batch()
    tr.materialise(b0)
    tr.build()
    tr.train_step(b0)
    t0 = time.perf_counter()
    tr.train_step(b1)
    dt = time.perf_counter() - t0
    return dict(value=round(n_pairs / dt, 4), unit="image-pairs/s", cores=cores, kind="port", host_cores=host,
                sample=f"1 training step of {n_pairs} synthetic {RPR_H}x{RPR_W} pairs, PyTorch-CPU fp32 ({cores} threads), correlation "
                       f"volume materialised like the reference, {dt:.1f}s")



RPR_FAMILIES = (("library convolutions (MIOpen / CK implicit-GEMM: forward of the encoder, d input and d weight of every convolution)",
                 ("igemm", "ck::", "miopenSp3", "naive_conv", "Cijk_", "gemm_kernel", "miopen_conv")),
                ("layout transposes around the library convolutions (NCHW <-> NHWC)", ("batched_transpose", "transpose")),
                ("BatchNorm (MIOpen)", ("BatchNorm",)),
                ("own kernels (correlation volume, decoder convolution forward, upsampling, Kabsch, packing)",
                 ("cw_", "conv_gemm_bf16", "conv_pack", "conv_unpack", "upsample_ac", "kabsch", "zero_fill")))


def rpr_kernel_families():
    """GPU time of the training step by kernel family, from the NEWEST committed rocprofv3 kernel trace of THIS command's timed steps
    (profiles/rNN_bench_rpr_train_kernel_stats.csv, tools/kernel_stats_timed.py: warm-up and the library's solution search excluded)"""
    import csv
    import glob
    found = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_bench_rpr_train_kernel_stats.csv")))
    if not found:
        return None
    path = found[-1]
    fam = {name: 0.0 for name, _ in RPR_FAMILIES}
    fam["everything else (elementwise, reductions, optimizer, copies)"] = 0.0
    total = 0.0
    for r in csv.DictReader(open(path)):
        ms = float(r["MsPerStep"]); total += ms
        for name, keys in RPR_FAMILIES:
            if any(k in r["Name"] for k in keys):
                fam[name] += ms
                break
        else:
            fam["everything else (elementwise, reductions, optimizer, copies)"] += ms
    return {"source": "profiles/" + os.path.basename(path), "kernel_ms_per_step": round(total, 3),
            "ms_per_step": {k: round(v, 3) for k, v in fam.items()}, "share": {k: round(v / total, 4) for k, v in fam.items()}}


def rpr_roofline(tr, batch, B, ms_per_step, own, own_fwd_step):
    """The family that dominates the step is the LIBRARY's convolutions, so that is what the roofline prices: the convolution flops the
    library runs per step over the family's GPU time, against the dense bf16 peak.  Library flops = 3 x (forward + d input + d weight) the forward
    flops of every convolution that goes through nn.Conv2d (counted by hooks: 2 Cin Cout k^2 Hout Wout per image and layer; the decoder layers
    that run the own forward kernel bypass the module call and are NOT in that count) + 2 x the own kernel's forward flops (`own_fwd_step`,
    counted at its launches: d input and d weight of those layers are library kernels, options RPR_CONV_BWD = 'lib').  The family's time is its
    share in the committed profile of this command applied to the step time measured now."""
    flops = {"all": 0.0, "own_fwd": 0.0}

    def hook(mod, inp, out):
        f = 2.0 * mod.in_channels // mod.groups * mod.out_channels * mod.kernel_size[0] * mod.kernel_size[1] * out.shape[-1] * out.shape[-2] * out.shape[0]
        flops["all"] += f
    hs = [m.register_forward_hook(hook) for m in tr.model.modules() if isinstance(m, torch.nn.Conv2d)]
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            tr.model.encoder(torch.cat([batch["image0"], batch["image1"]]))
    finally:
        for h in hs:
            h.remove()
    fams = rpr_kernel_families()
    lib_name = RPR_FAMILIES[0][0]
    from mapfree_reloc_amd import options as _opt
    lib_flops = 3.0 * flops["all"] + (2.0 * own_fwd_step if _opt.get("RPR_CONV_BWD") == "lib" else 0.0)
    lib_ms = fams["share"][lib_name] * ms_per_step if fams else None
    ach = lib_flops / (lib_ms * 1e-3) / 1e12 if lib_ms else None
    return {"kernel": lib_name + " -- the family with the largest share of the step's GPU time", "bound": "mfma",
            "achieved": round(ach, 1) if ach else None, "peak": BF16_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
            "frac": round(ach / BF16_MFMA_PEAK_TFLOPS, 4) if ach else None, "traffic": None,
            "family_ms_per_step": round(lib_ms, 3) if lib_ms else None, "flops_per_step": lib_flops,
            "library_forward_conv_flops_per_step": flops["all"], "own_kernel_forward_flops_per_step": own_fwd_step,
            "note": "family time = its share of the kernel time in the committed profile x the step time of this run; flops = 3 x the forward flops of the "
                    "convolutions the library runs forward (both views) + 2 x the forward flops of the decoder layers whose forward is the own kernel "
                    "(their d input / d weight are library kernels)",
            "kernel_families": fams, "other_kernels": own}


def rpr_train_bench(args, rank, world, dev, use_dist):
    """python bench.py --config rpr_train: a step = forward + loss + backward (+ bucketed RCCL gradient all-reduce) + clip +
    Adam on B pairs per GPU; value = pairs trained per second over all ranks (weak scaling)."""
    import mapfree_reloc_amd as mfr
    from mapfree_reloc_amd.regression.train import SyntheticPairs, Trainer
    lib = mfr._lib.load(require_gpu=True)
    B = args.batch
    opts = tuple(o for o in args.rpr_opts.split(",") if o and o != "none")
    cfg = rpr_cfg("bf16", opts)
    src = SyntheticPairs(B, RPR_H, RPR_W, dev, seed=0, rank=rank)
    batches = [src.batch() for _ in range(2)]            # resident in HBM before the timed region, alternated
    torch.cuda.synchronize()
    fwd_t, bwd_t, cg_t = KernelTimer(), KernelTimer(), KernelTimer()
    cg_flops = []
    if not args.no_kernel_timer:
        lib.mfr_corr_warp_fwd = fwd_t.wrap(lib.mfr_corr_warp_fwd)
        lib.mfr_corr_warp_bwd = bwd_t.wrap(lib.mfr_corr_warp_bwd)
        _cg = cg_t.wrap(lib.mfr_conv_gemm_bf16)

        def cg_counted(*a):                                  # (A, sA, segA, B, sB, segB, Lk, nkc_total, nkc_z, bias, C, ldc, dtype, M, N, nz, ...)
            if cg_t.enabled:
                cg_flops.append(2.0 * a[13] * a[14] * 32.0 * a[7] * (a[15] if a[8] >= a[7] else 1))
            return _cg(*a)
        lib.mfr_conv_gemm_bf16 = cg_counted
    tr = Trainer(cfg, dev, sample=batches[0]).build()
    for i in range(3 + args.warmup):                     # 3 initialisation steps (MIOpen solution search), then the warm-up
        tr.train_step(batches[i & 1])
    torch.cuda.synchronize()
    if use_dist:
        dist.barrier()
    torch.cuda.synchronize()
    fwd_t.enabled = bwd_t.enabled = cg_t.enabled = True
    t0 = time.perf_counter()
    for i in range(args.steps):
        losses = tr.train_step(batches[i & 1])
    torch.cuda.synchronize()
    if use_dist:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        # what the caller of train_step receives (the three losses of the last step) + a fixed sample of the weights it updated
        flat = torch.cat([p.detach().reshape(-1).float() for p in tr.model.parameters()])
        idx = torch.from_numpy(np.sort(np.random.default_rng(0).choice(flat.numel(), min(flat.numel(), 1 << 20), replace=False))).to(flat.device)
        dump_outputs(args.dump_outputs, {"R_loss": losses[0], "t_loss": losses[1], "loss": losses[2], "params_sample": flat[idx]})
    timed_steps = args.steps
    if args.full and tr.graph_step and tr._gstep is not None:
        timed_steps = 3                                   # the launches below are the ones the timers (and the flop counter) see
        # HIP events cannot be recorded inside a replay: time the correlation-volume kernels over eager steps right after the region
        saved = (tr._gstep, tr._gkeys)
        tr._gstep, tr._gkeys = None, ()
        for i in range(3):
            tr.train_step(batches[i & 1])
        torch.cuda.synchronize()
        tr._gstep, tr._gkeys = saved
    fwd_t.enabled = bwd_t.enabled = cg_t.enabled = False
    if use_dist:
        tt = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
    if rank != 0:
        return
    with torch.no_grad():
        vol = tr.model.encoder(batches[0]["image0"][:1])
    D, N = vol.shape[1], vol.shape[2] * vol.shape[3]
    n_param = sum(p.numel() for p in tr.model.parameters())
    # the fused correlation-volume kernels: contractions over the [N, N] volume, per launch (B volumes)
    f_fwd = 2.0 * N * N * (D + 32) * B                   # S = K^T Q, O = V P
    f_bwd = 2.0 * N * N * ((D + 32 + D) + (D + 32 + D + 32)) * B     # query owner: S, dP, dQ; key owner: S, dP, dK, dV
    fm, bm = fwd_t.mean_ms(), bwd_t.mean_ms()
    ach_f = f_fwd / (fm * 1e-3) / 1e12 if fm else None
    ach_b = f_bwd / (bm * 1e-3) / 1e12 if bm else None
    vol_bytes = 4.0 * N * N * B
    cgm = cg_t.mean_ms()
    ncg = min(len(cg_flops), len(cg_t.events))
    ach_c = (sum(cg_flops[:ncg]) / max(ncg, 1)) / (cgm * 1e-3) / 1e12 if cgm and ncg else None
    own_fwd_step = sum(cg_flops) / max(1, timed_steps)       # forward flops of the own decoder-convolution kernel per training step
    own = [{"kernel": "cw_bwd_q_kernel + cw_bwd_kv_kernel (mfr_corr_warp_bwd: fused correlation-volume warping, backward)", "bound": "mfma",
            "achieved": round(ach_b, 2) if ach_b else None, "peak": FP32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
            "frac": round(ach_b / FP32_MFMA_PEAK_TFLOPS, 4) if ach_b else None, "traffic": _traffic("cw_bwd_kv", B),
            "avg_launch_ms": round(bm, 4) if bm else None, "launches_timed": len(bwd_t.events), "flops_per_launch": f_bwd,
            "note": f"the [B, N, N] volume ({vol_bytes / 1e9:.2f} GB fp32 at this batch) is never written: it is recomputed tile by tile on the "
                    "fp32 matrix cores; HBM-side algorithmic bytes are the q/k/v/gradient maps only (a few MB)"},
           {"kernel": "cw_fwd_kernel (mfr_corr_warp_fwd)", "bound": "mfma", "achieved": round(ach_f, 2) if ach_f else None,
            "peak": FP32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(ach_f / FP32_MFMA_PEAK_TFLOPS, 4) if ach_f else None,
            "avg_launch_ms": round(fm, 4) if fm else None, "launches_timed": len(fwd_t.events), "flops_per_launch": f_fwd},
           {"kernel": "conv_gemm_bf16_kernel (mfr_conv_gemm_bf16: the decoder's 3x3 convolutions as implicit GEMMs, forward; backward = library)",
            "bound": "mfma", "achieved": round(ach_c, 1) if ach_c else None, "peak": BF16_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
            "frac": round(ach_c / BF16_MFMA_PEAK_TFLOPS, 4) if ach_c else None,
            "avg_launch_ms": round(cgm, 4) if cgm else None, "launches_timed": len(cg_t.events),
            "flops_per_launch": round(sum(cg_flops[:ncg]) / max(ncg, 1)) if ncg else None}]
    line = {
        "metric": "image-pairs/sec trained (3d3d relative-pose regression, bf16 autocast, 360x270)", "value": round(B * args.steps * world / elapsed, 3),
        "unit": "image-pairs/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(1e3 * elapsed / args.steps, 3),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "bf16 autocast (encoder / head convolutions), f32 (correlation-volume kernel, pose algebra, losses, master weights, Adam)",
        "data": "synthetic (seeded textured planes under a random relative pose; no Map-free training split offline), random-init weights",
        "config": {"workload": "configs[4]: 3d3d.yaml (ResUNet 3-3-3 -> CorrelationVolumeWarping -> ProcrustesDeepResBlock), full training step",
                   "global_batch": B * world, "pairs_per_gpu_per_step": B, "parallelism": f"dp{world} (" + ("one flat-gradient RCCL all-reduce per step after the graph replay" if tr.graph_step else f"DDP, {cfg.TRAINING.DDP_BUCKET_MB} MB gradient buckets, RCCL all-reduce") + ")",
                   "precision": cfg.TRAINING.PRECISION, "siamese_batch": bool(cfg.TRAINING.SIAMESE_BATCH), "channels_last": bool(cfg.TRAINING.CHANNELS_LAST), "graph_step": bool(tr.graph_step),
                   "volume_positions": N, "feature_channels": D, "parameters": n_param, "optimizer": "Adam (fused), eps 1e-6",
                   "last_losses": [round(float(x.float().sum()), 5) for x in losses]},
    }
    if args.full:
        line["roofline"] = rpr_roofline(tr, batches[0], B, 1e3 * elapsed / args.steps, own, own_fwd_step)
    if world == 1 and not args.no_cpu_baseline:
        line["cpu_baseline"] = cpu_baseline_subprocess("rpr_train", args.cpu_pairs, args.cpu_threads, "")
    print(json.dumps(line))


def secondary_line(config, extra, budget_s):
    """python bench.py --config <config> in a child process -> its parsed JSON line (or an error record, never an exception)"""
    import subprocess
    t0 = time.perf_counter()
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--gpus", "1", "--config", config, "--full", "--no-secondary", "--no-all-cores"] + extra,
                           capture_output=True, text=True, timeout=budget_s, env=env)
        for ln in reversed(r.stdout.strip().splitlines()):
            if ln.startswith("{"):
                out = json.loads(ln)
                out["wall_s"] = round(time.perf_counter() - t0, 1)
                return out
        return {"config": {"workload": config}, "value": None, "error": (r.stderr or "no output")[-400:]}
    except subprocess.TimeoutExpired:
        return {"config": {"workload": config}, "value": None, "error": f"exceeded its {budget_s:.0f}s budget"}


def _traffic(tag, B):
    """HBM traffic of the dominant kernel: PMC counters cannot be read inside this process, so the per-launch figure
    comes from the committed rocprofv3 --pmc passes of this same command (2 x FETCH_SIZE + WRITE_SIZE, the guide's
    gfx950 correction), profiles/r02_pmc_<tag>.json"""
    for rnd in ("r06", "r05", "r04", "r03", "r02", "r01"):
        try:
            name = {"conv1b": "wino"}.get(tag, tag) if rnd == "r01" else tag
            pj = json.load(open(os.path.join(ROOT, "profiles", f"{rnd}_pmc_{name}.json")))
            if pj.get("pairs_per_step") == B:
                return {"bytes_per_launch": round(pj["hbm_bytes_per_launch"]), "algorithmic_bytes_per_launch": pj["algorithmic_bytes_per_launch"],
                        "source": f"profiles/{rnd}_pmc_{name}.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes)"}
        except Exception:
            continue
    return None


def _pose_error(o, gtb):
    """second half of BASELINE's metric ("median rot/trans error on val"): no val data offline, so the error is taken
    against the known pose of the synthetic scenes of the last step (every pair has an exact ground truth)"""
    try:
        ok = (o["status"] == 0).cpu().numpy()
        Rg, tg = gtb["R_gt"].cpu().numpy(), gtb["t_gt"].cpu().numpy()
        Re, te = o["R"].cpu().numpy().reshape(-1, 3, 3), o["t"].cpu().numpy().reshape(-1, 3)
        if not ok.any():
            return None
        idx = np.nonzero(ok)[0]
        rot = [float(np.degrees(np.arccos(np.clip((np.trace(Rg[i].T @ Re[i]) - 1) / 2, -1, 1)))) for i in idx]
        tr = [float(np.linalg.norm(te[i] - tg[i])) for i in idx]
        return {"median_rot_deg": round(float(np.median(rot)), 6), "median_trans_m": round(float(np.median(tr)), 6),
                "pairs": int(ok.sum()), "against": "known pose of the synthetic scenes (last step)"}
    except Exception as e:       # never lose the bench line over the accuracy side-note
        return {"error": str(e)[:200]}


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, arrays):
    """--dump-outputs: every array as out_dir/<name>.npy, floating point kept as float32 / float64, integer and boolean outputs as float64
    (exact).  An array larger than its share of the 64 MB budget is replaced by a fixed sample of its flattened elements (seeded, sorted
    indices), so that two builds compare the same elements."""
    os.makedirs(out_dir, exist_ok=True)
    arrays = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in sorted(arrays.items())}
    share = DUMP_LIMIT_BYTES // max(1, len(arrays))
    for name, a in arrays.items():
        a = a.astype(np.float32 if a.dtype in (np.float16, np.float32) else np.float64)
        if a.nbytes > share:
            idx = np.sort(np.random.default_rng(0).choice(a.size, share // a.itemsize, replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(out_dir, f"{name}.npy"), a)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _fail(msg):
    print(f"bench.py: error: {msg}", file=sys.stderr)
    sys.exit(2)


def main():
    args = parse()
    if args.hip_opt:
        from mapfree_reloc_amd import options as hip_options
        for kv in args.hip_opt:
            k, _, v = kv.partition("=")
            hip_options.set(k.strip(), v.strip())
    if args.cpu_baseline_only:
        print(json.dumps(cpu_baseline(args.config, args.cpu_pairs, [1000 + i for i in range(args.cpu_pairs)], args.cpu_threads, args.cpu_out)))
        return
    launched = "RANK" in os.environ and "WORLD_SIZE" in os.environ
    if args.gpus < 1:
        _fail("--gpus must be >= 1")
    if not launched and args.gpus > 1:
        # start the ranks ourselves: one process per GPU through torch.distributed.run on 127.0.0.1
        n_dev = torch.cuda.device_count()
        if n_dev < args.gpus:
            _fail(f"--gpus {args.gpus} requested but only {n_dev} HIP device(s) are visible; refusing to report a smaller run as {args.gpus} GPUs")
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
               "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
        import subprocess
        sys.exit(subprocess.call(cmd))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        _fail(f"--gpus {args.gpus} != WORLD_SIZE {world}: launch exactly one rank per GPU")
    if not torch.cuda.is_available() or local_rank >= torch.cuda.device_count():
        _fail(f"rank {rank}: HIP device {local_rank} is not visible (device_count = {torch.cuda.device_count()}); there is no CPU fallback")
    use_dist = launched
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=dev)        # backend "nccl" is RCCL on ROCm
        world = dist.get_world_size()                         # what RCCL actually formed

    if args.config == "rpr_train":
        rpr_train_bench(args, rank, world, dev, use_dist)
        if use_dist:
            dist.destroy_process_group()
        return

    import mapfree_reloc_amd as mfr
    from mapfree_reloc_amd import images as IM
    from mapfree_reloc_amd.parallel import gather_pose_records
    mfr._lib.load(require_gpu=True)

    B = args.batch
    # two distinct resident batches per rank, alternated step to step (nothing is cached)
    batches = []
    for k in range(2):
        seeds = [1000 * rank + 100 * k + i for i in range(B)]
        sb = IM.synthetic_batch(seeds, H, W)
        batches.append({key: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for key, v in sb.items()})
    use_graph = args.config == "sg_pnp" and args.graph == 1
    overlap = bool(args.overlap) and not use_graph
    wl = (SgPnpWorkload(dev, B, not args.no_kernel_timer, graph=use_graph, overlap=overlap) if args.config == "sg_pnp"
          else LoftrEmatWorkload(dev, B, not args.no_kernel_timer, overlap=overlap))

    def step(i):
        return wl.run(batches[i & 1])

    # initialisation, not warm-up: the first calls on a fresh box pay lazy library initialisation (hipBLASLt / MIOpen
    # solution selection, code-object loading) and the GPU's clock ramp (measured: the first process on a cold box ran
    # the same steps 1.5x slower when timed right after 3 calls)
    for i in range(6 if args.config == "sg_pnp" else 3):
        step(i)
    torch.cuda.synchronize()

    for i in range(args.warmup):
        out = step(i)
    wl.pipe.join()
    if args.warmup > 0:
        # the collective is part of a step's tail: warm it up too (RCCL builds its channels on the first all_gather; at world 1 the
        # record-packing kernels load their code objects on first use: 48 ms measured inside the timed region otherwise)
        gather_pose_records(batches[(args.warmup - 1) & 1]["pair_ids"], {k: out[k] for k in ("R", "t", "n_inliers", "status")}, world if use_dist else 1)
        _ids = torch.cat([batches[0]["pair_ids"]] * 2); _o = {k: torch.cat([out[k]] * 2) for k in ("R", "t", "n_inliers", "status")}
        gather_pose_records(_ids, _o, world if use_dist else 1)
    torch.cuda.synchronize()
    if use_dist:
        dist.barrier()
    torch.cuda.synchronize()
    for t in wl.timers():
        t.enabled = True
    t0 = time.perf_counter()
    results = []
    for i in range(args.steps):
        ts = time.perf_counter()
        out = step(i)
        results.append((batches[i & 1]["pair_ids"], out))
        if args.verbose:
            hi = 1e3 * (time.perf_counter() - ts)
            torch.cuda.synchronize()
            print(f"step {i}: host issue {hi:.1f} ms, done {1e3 * (time.perf_counter() - ts):.1f} ms", file=sys.stderr)
    # one gather of the per-pair pose records for the whole run
    wl.pipe.join()                                         # (--overlap: this stream waits for the last solver stage before it reads any result)
    all_ids = torch.cat([r[0] for r in results])
    all_out = {k: torch.cat([r[1][k] for r in results]) for k in ("R", "t", "n_inliers", "status")}
    torch.cuda.synchronize()
    t_compute = time.perf_counter() - t0                   # this rank's own steps, before it meets the others
    tg = time.perf_counter()
    rec = gather_pose_records(all_ids, all_out, world if use_dist else 1)
    torch.cuda.synchronize()
    t_gather = time.perf_counter() - tg
    if use_dist:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {k: v for k, v in results[-1][1].items() if isinstance(v, torch.Tensor)})
    if args.full and use_graph:
        # HIP events cannot be recorded inside a graph replay: the dominant kernels are timed over eager steps of the same
        # workload right after the timed region (same process, same clocks, same inputs); not part of `value`
        wl.pipe.graph = False
        for i in range(max(3, min(args.steps, 6))):
            step(i)
        torch.cuda.synchronize()
        wl.pipe.graph = True
    for t in wl.timers():
        t.enabled = False
    per_rank = [[t_compute, t_gather]]
    if use_dist:
        tt = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
        mine = torch.tensor([t_compute, t_gather], device=dev, dtype=torch.float64)
        allr = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        per_rank = [a.tolist() for a in allr]

    if rank == 0:
        total_pairs = B * args.steps * world
        value = total_pairs / elapsed
        o = results[-1][1]
        cfg = {"workload": wl.workload, "pairs_per_gpu_per_step": B, "parallelism": f"pair-sharded x{world}",
               "launch": ("one captured HIP graph per step (static-input copies inside the step)" if use_graph else
                          "eager kernel launches; the RANSAC stage of step i on a second HIP stream under the matcher of step i + 1 (one join before the gather)" if overlap
                          else "eager kernel launches, one stream"),
               "pairs_solved_last_step": int((o["status"] == 0).sum()), "mean_matches_last_step": float(o["n_corr"].float().mean()),
               "gathered_records": int(rec.shape[0])}
        if args.full:
            cfg["synthetic_pose_error"] = _pose_error(o, batches[(args.steps - 1) & 1])
        cfg.update(wl.config(o))
        line = {
            "metric": wl.metric, "value": round(value, 3), "unit": "image-pairs/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(1e3 * elapsed / args.steps, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": wl.dtype,
            "data": "synthetic (3-band planar scenes, seeded random weights; no dataset/checkpoints offline)",
            "config": cfg,
            # scaling diagnostics: every rank's own pairs/s over its K steps (before the collective) and what the one gather cost it
            "per_rank": {"pairs_per_s": [round(B * args.steps / max(p[0], 1e-9), 2) for p in per_rank],
                         "gather_ms": [round(1e3 * p[1], 3) for p in per_rank], "record_bytes_per_pair": 80},
        }
        if args.full:
            line["roofline"] = wl.roofline(o)
        if world == 1 and not args.no_cpu_baseline:
            with tempfile.TemporaryDirectory() as td:
                npz = os.path.join(td, "oracle_pairs.npz")
                line["cpu_baseline"] = cpu_baseline_subprocess(args.config, args.cpu_pairs, args.cpu_threads, npz, all_cores=not args.no_all_cores)
                if os.path.exists(npz):
                    try:
                        cfg["parity"] = parity_leg(wl, npz, dev)
                    except Exception as e:        # never lose the bench line over the parity side-note
                        cfg["parity"] = {"error": str(e)[:300]}
        if world == 1 and args.config == "sg_pnp" and not args.no_secondary:
            # the other two single-GPU configurations BASELINE.json names, each with its OWN timed region, roofline, cpu_baseline
            # and parity, measured by this same script in a child process right after the headline (the driver runs only the
            # default command): configs[2] LoFTR + E-mat and configs[4] the bf16 regression training step
            line["secondary"] = [secondary_line("loftr_emat", ["--steps", "8", "--warmup", "2", "--cpu-pairs", "2"], args.secondary_budget),
                                 secondary_line("rpr_train", ["--steps", "20", "--warmup", "3", "--cpu-pairs", "4"], args.secondary_budget)]
            # compact copy at the top level, so that a reader who keeps only scalar keys of the line still sees configs[2] / [4]
            line["secondary_values"] = {"loftr_emat_pairs_per_s": line["secondary"][0].get("value"), "rpr_train_pairs_per_s": line["secondary"][1].get("value")}
        print(json.dumps(line))
    if use_dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
