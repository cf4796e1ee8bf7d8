"""DESIGN.md = docs/DESIGN.template.md with its tables and numbers filled from the committed records under profiles/ (so that text and records cannot
disagree: VERDICT r5 weak 1a / 8).   python tools/fill_design.py"""
import csv
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = lambda *a: os.path.join(ROOT, *a)
rd = lambda name: open(P("docs", name)).read().rstrip("\n")


def stats(cfg):
    rows = list(csv.DictReader(open(P("profiles", f"r06_bench_{cfg}_kernel_stats.csv"))))
    meta = json.load(open(P("profiles", f"r06_bench_{cfg}_kernel_stats.json")))
    def ms(*subs, exclude=()):
        return sum(float(r["MsPerStep"]) for r in rows if any(s in r["Name"] for s in subs) and not any(e in r["Name"] for e in exclude))
    return rows, meta, ms


f2 = lambda v: f"{v:.2f}"
bench = json.loads(open(P("profiles", "r06_bench_default.json")).read().strip().splitlines()[-1])
sec = {("loftr" if "LoFTR" in s["metric"] else "rpr"): s for s in bench.get("secondary", [])}
_, sg_meta, sg = stats("sg_pnp")
_, lo_meta, lo = stats("loftr_emat")
roof = bench["roofline"]
cpu = bench["cpu_baseline"]
try:
    hostfed = json.load(open(P("profiles", "r06_fused_split_1gpu.json")))
    hf = hostfed.get("sg_pnp", {}).get("pairs_per_s") or next((v.get("pairs_per_s") for v in hostfed.values() if isinstance(v, dict) and "pairs_per_s" in v), None)
except Exception:
    hf = None
sub = {
    "SG_PPS": f"{bench['value']:.1f}", "SG_MS": f2(bench["ms_per_step"]), "SG_KMS": f2(sg_meta["kernel_ms_per_step"]), "SG_LAUNCHES": f"{sg_meta['launches_per_step']:.0f}",
    "LOFTR_PPS": f"{sec['loftr']['value']:.1f}", "LOFTR_MS": f2(sec["loftr"]["ms_per_step"]), "LOFTR_KMS": f2(lo_meta["kernel_ms_per_step"]),
    "LOFTR_LAUNCHES": f"{lo_meta['launches_per_step']:.0f}",
    "RPR_PPS": f"{sec['rpr']['value']:.1f}", "RPR_MS": f2(sec["rpr"]["ms_per_step"]),
    "HOSTFED": f"{hf:.0f}" if hf else "(see record)",
    "C1_MS": f2(roof["avg_launch_ms"]), "C1_TF": f"{roof['achieved']:.0f}", "C1_FRAC": f"{roof['frac']:.3f}", "C1_PIPE": f"{roof['mfma_pipe_frac']:.3f}",
    "CPU_PPS": f"{cpu['value']:.2f}", "CPU_CORES": str(cpu["cores"]),
    "SG_C1": f2(sg("wino_split_c1")), "SG_DCONV": f2(sg("conv_direct")), "SG_ATT": f2(sg("sg_attention")), "SG_GEMM": f2(sg("gemm_split")),
    "SG_SINK": f2(sg("sg_sweep", "sg_colmerge", "sg_rowmax", "sg_colmax", "sg_match")), "SG_SPPOST": f2(sg("sp_nms", "sp_select", "sp_sample", "sp_scoremap")),
    "SG_IGEMM": f2(sg("conv_igemm")), "SG_PNP": f2(sg("pnp_")),
    "LOFTR_DCONV": f2(lo("conv_direct")), "LOFTR_GEMM": f2(lo("gemm_split_d")), "LOFTR_MLPLN": f2(lo("mlp_ln")), "LOFTR_FATT": f2(lo("fine_attention")),
    "LOFTR_IGEMM": f2(lo("conv_igemm")), "LOFTR_LA": f2(lo("la_kv", "la_out", "la_fold")), "LOFTR_DSM": f2(lo("dsm_")), "LOFTR_EMAT": f2(lo("emat_", "scale_")),
}
df = json.load(open(P("profiles", "dpt_fused.json")))           # DPT on the fused route (tools/bench_dpt_fused.py)
for key, tag in (("sg_pnp", "PNP"), ("sg_emat_metric", "EM")):
    a1, b, a2 = (df[key][k] for k in ("a1_depth_from_files", "b_online", "a2_depth_from_files"))
    sub.update({f"DPTF_{tag}_ON": f2(b["gpu_ms_per_step_median"]), f"DPTF_{tag}_FILE": f2((a1["gpu_ms_per_step_median"] + a2["gpu_ms_per_step_median"]) / 2),
                f"DPTF_{tag}_SPREAD": f2(abs(a1["gpu_ms_per_step_median"] - a2["gpu_ms_per_step_median"])), f"DPTF_{tag}_RUN": str(b["depth_views_run"]),
                f"DPTF_{tag}_REUSED": str(b["depth_views_reused"]), f"DPTF_{tag}_STAGE": f2(b["depth_stage_ms_per_step_median"]),
                f"DPTF_{tag}_PPS_ON": f"{b['pairs_per_s']:.0f}", f"DPTF_{tag}_PPS_A1": f"{a1['pairs_per_s']:.0f}", f"DPTF_{tag}_PPS_A2": f"{a2['pairs_per_s']:.0f}",
                f"DPTF_{tag}_FIRST": f2(b["depth_stage_ms_first_step"]), f"DPTF_{tag}_TOTAL": f"{b['depth_stage_ms_total']:.0f}"})
sub.update({"DPTF_STEPS": str(df["sg_pnp"]["b_online"]["steps"]), "DPTF_PAIRS": str(df["tree"]["pairs"]), "DPTF_FRAMES": str(df["compute_depth_over_the_tree"]["frames"]), "DPTF_B": str(df["sg_pnp"]["b_online"]["batch_pairs"]),
            "DPTF_CD_S": f"{df['compute_depth_over_the_tree']['seconds']:.1f}", "DPTF_CD_MB": f"{df['compute_depth_over_the_tree']['png_MB_written']:.0f}",
            "DPTF_PNP_S": f"{df['sg_pnp']['b_online']['seconds']:.1f}", "DPTF_EM_S": f"{df['sg_emat_metric']['b_online']['seconds']:.1f}"})
pr = df["loader_probe"]
sub.update({"DPTF_PR_FILE0": f"{pr['loaders_alone']['files_process_decode']:.0f}", "DPTF_PR_RGB0": f"{pr['loaders_alone']['rgb_process_decode']:.0f}",
            "DPTF_PR_FILE1": f"{pr['after_dpt_is_built']['files_process_decode']:.0f}", "DPTF_PR_RGB1": f"{pr['after_dpt_is_built']['rgb_process_decode']:.0f}",
            "DPTF_PR_THREAD": f"{pr['after_dpt_is_built']['files_thread_decode']:.0f}", "DPTF_PR_FIRST": f"{pr['pool_forked_before_dpt']['rgb_process_decode']:.0f}"})
da = json.load(open(P("profiles", "depth_anything_stage.json")))   # Depth Anything's stage record (tools/bench_depth_anything.py)
f3 = lambda v: f"{v:.3f}"
enc = {d["encoder"]: d for d in da["depth_anything"] if d["arithmetic"] == "f16x2"}
S3 = [enc[k] for k in ("vits", "vitb", "vitl")]
hyb = next(d for d in da["dpt_hybrid"] if d["arithmetic"] == "f16x2")
for tag, d in (("S", S3[0]), ("B", S3[1]), ("L", S3[2]), ("H", hyb)):
    w = d["whole_pass"]
    sub.update({f"DAS_{tag}_WHOLE": f3(w["ms_per_frame"]), f"DAS_{tag}_LO": f3(w["spread_ms_per_frame"][0]), f"DAS_{tag}_HI": f3(w["spread_ms_per_frame"][1])})
for tag, key in (("PATCH", "patch_rows"), ("EMBED", "embedding_product"), ("TOKENS", "token_assembly"), ("ENCODER", "encoder"), ("REASSEMBLE", "taps_and_reassemble"),
                 ("NECK", "neck"), ("HEAD", "head_at_14g"), ("TAIL", "tail")):
    sub[f"DAS_ST_{tag}"] = " / ".join(f3(d["stages"][key]["ms_per_frame"]) for d in S3)
sub.update({"DAS_ST_SUM": " / ".join(f3(d["stages_sum_ms_per_frame"]) for d in S3),
            "DAS_ENC_SHARE": " / ".join(f"{100 * d['stages']['encoder']['ms_per_frame'] / d['whole_pass']['ms_per_frame']:.0f}" for d in S3),
            "DAS_L_TFLOPS": f"{S3[2]['tflops_whole_pass']:.0f}", "DAS_HEAD_MB": " / ".join(f"{d['head_map_bytes_per_frame']['bytes'] / 1e6:.0f}" for d in S3),
            "DAS_BATCH": str(da["workload"]["batch"]), "DAS_TOKENS": str(S3[0]["tokens"]), "DAS_H_TOKENS": str(hyb["tokens"]), "DAS_REPEATS": str(da["workload"]["repeats"]),
            "DAS_ITERS": str(da["workload"]["iters"]), "DAS_WINDOW": f"{da['workload']['min_window_ms']:.0f}"})
rs = json.load(open(P("profiles", "rig_solvers.json")))         # the rig solvers side by side (tools/bench_rig_solvers.py)
ra, rt = rs["accuracy_cpu_mirrors"], rs.get("solve_batch")
f4 = lambda v: f"{v:.4f}"
for tag, key in (("PNP", "rig_pnp_T9"), ("PR", "rig_procrustes_T9"), ("EM", "rig_essential_matrix_T9"), ("L", "procrustes_last_frame")):
    sub.update({f"RIGS_{tag}_R": f4(ra[key]["median_rot_rad"]), f"RIGS_{tag}_T": f4(ra[key]["median_trans_m"])})
sub["RIGS_BASE"] = f2(ra["largest_baseline_m_median"])
if rt:
    sub.update({"RIGS_PR_MS": f2(rt["rig_procrustes"]["median_ms"]), "RIGS_PRROWS_MS": f2(rt["procrustes_rows"]["median_ms"]),
                "RIGS_PNP_MS": f2(rt["rig_pnp"]["median_ms"]), "RIGS_EM_MS": f2(rt["rig_emat_both_stages"]["median_ms"]), "RIGS_EM2_MS": f2(rt["rig_emat_stage2"]["median_ms"]),
                "RIGS_EM1_MS": f2(rt["rig_emat_stage1_emat_rows"]["median_ms"])})
census = subprocess.check_output([sys.executable, P("tools", "census_table.py")], text=True).rstrip("\n")
out = open(P("docs", "DESIGN.template.md")).read()
parts = {"CENSUS_TABLE_PLACEHOLDER": census, "KERNEL_TABLE_PLACEHOLDER": rd("_design_kernel_table.md"), "SECTION44_PLACEHOLDER": rd("_design_44.md"),
         "SECTION5_PLACEHOLDER": rd("_design_58.md").split("## 8. What comes next")[0].rstrip("\n"),
         "SECTION8_PLACEHOLDER": "## 8. What comes next" + rd("_design_58.md").split("## 8. What comes next")[1], "VERDICT_PLACEHOLDER": rd("_design_9.md")}
for k, v in parts.items():
    assert k in out, k
    out = out.replace(k, v)
for k in sorted(sub, key=len, reverse=True):
    out = out.replace(k, sub[k])
open(P("DESIGN.md"), "w").write(out)
left = [w for w in ("PLACEHOLDER", "SG_", "LOFTR_", "C1_", "RPR_", "CPU_", "HOSTFED", "DPTF_", "DAS_", "RIGS_") if w in out]
print("DESIGN.md written,", len(out), "bytes; unresolved markers:", left, "; longest line", max(len(l) for l in out.splitlines()))
