"""Generate tests/golden/ref_sevenscenes.npz by EXECUTING THE REFERENCE'S OWN 7Scenes reader and localisation code (needs the reference
checkout; never run on the GPU box):

  (a) lib/datasets/sevenscenes.py  SceneDataset on the tiny tree of tests/sevenscenes_tree.py: every sample field, with and without ONE_NN,
      ground-truth and estimated depth;
  (b) lib/utils/localize.py        ransac(.., 15, pair_type='relapose') and cal_abs_pose_err_metric on seeded queries: 64 each with
      k = 1, 2, 3, 5 neighbours (in_iter = 10) and 16 each with k = 8, 12 (in_iter = 0); inputs, per-query poses, inlier lists, flags,
      errors, pass rates, medians, AP, pose_<scene>.txt lines;
  (c) the printed report lines of eval_pipeline_with_ransac / eval_pipeline_without_ransac over those groups plus a scene that holds a
      query without pairs, and precision / recall arrays.

cv2 and transforms3d are not installed: cv2 is stubbed (imread served by PIL), transforms3d.quaternions by a restatement of its
quat2mat / mat2quat.  A drawn query is REJECTED (and redrawn; at most 10 % may be) unless the reference's result on it is a matter of
arithmetic far from any decision: no np.random.shuffle call, every thresholded cosine >= 1e-9 away from the rounding boundary that decides
`err < thres`, every triangulation's conditioning s1^2 / (s3^2 - s4^2) <= 1e7, every Weiszfeld step >= 1e-9 away from the 1e-5 stop.
Those margins are measured on tests/abs_pose_ref.py, which must reproduce the reference's inlier lists on the query."""
import contextlib
import io
import os
import sys
import tempfile
import types

import numpy as np

REF = os.environ.get("MFR_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "..", "tests", "golden", "ref_sevenscenes.npz")
ERR_THRES = ((0.1, 5), (0.25, 5), (0.5, 10), (1, 20))
THRES, MULT = 15, 1.414
GROUPS = ((1, 64, 10), (2, 64, 10), (3, 64, 10), (5, 64, 10), (8, 16, 0), (12, 16, 0))      # (k, queries, in_iter)


def stub_modules():
    from PIL import Image
    cv = types.ModuleType("cv2")
    cv.IMREAD_COLOR, cv.IMREAD_UNCHANGED, cv.COLOR_BGR2RGB = 1, -1, 4
    cv.imread = lambda path, flag=1: np.asarray(Image.open(path))
    cv.cvtColor = lambda img, code: img
    cv.resize = lambda img, wh: np.zeros((wh[1], wh[0]) + img.shape[2:], img.dtype)     # (the colour image is not part of the fixture)
    sys.modules["cv2"] = cv
    eps = np.finfo(np.float64).eps

    def quat2mat(q):
        w, x, y, z = q
        Nq = w * w + x * x + y * y + z * z
        if Nq < eps:
            return np.eye(3)
        s = 2.0 / Nq
        X = x * s; Y = y * s; Z = z * s
        wX = w * X; wY = w * Y; wZ = w * Z
        xX = x * X; xY = x * Y; xZ = x * Z
        yY = y * Y; yZ = y * Z; zZ = z * Z
        return np.array([[1.0 - (yY + zZ), xY - wZ, xZ + wY], [xY + wZ, 1.0 - (xX + zZ), yZ - wX], [xZ - wY, yZ + wX, 1.0 - (xX + yY)]])

    def mat2quat(M):
        Qxx, Qyx, Qzx, Qxy, Qyy, Qzy, Qxz, Qyz, Qzz = M.flat
        K = np.array([[Qxx - Qyy - Qzz, 0, 0, 0], [Qyx + Qxy, Qyy - Qxx - Qzz, 0, 0], [Qzx + Qxz, Qzy + Qyz, Qzz - Qxx - Qyy, 0],
                      [Qyz - Qzy, Qzx - Qxz, Qxy - Qyx, Qxx + Qyy + Qzz]]) / 3.0
        vals, vecs = np.linalg.eigh(K)
        q = vecs[[3, 0, 1, 2], np.argmax(vals)]
        if q[0] < 0:
            q *= -1
        return q
    t3 = types.ModuleType("transforms3d")
    t3q = types.ModuleType("transforms3d.quaternions")
    t3q.quat2mat, t3q.mat2quat = quat2mat, mat2quat
    t3.quaternions = t3q
    sys.modules["transforms3d"], sys.modules["transforms3d.quaternions"] = t3, t3q


# ---------------------------------------------------------------- (a) reader
def reader_part(out):
    from lib.datasets.sevenscenes import SceneDataset
    import sevenscenes_tree as ST
    p = ST.default_params()
    out.update({f"tree_{k}": np.asarray(v) for k, v in p.items()})
    resize = (int(p["width"]), int(p["height"]))
    with tempfile.TemporaryDirectory() as td:
        root = ST.write_tree(td, p)
        for s, scene in enumerate(p["scenes"].tolist()):
            for tag, one_nn, est in (("all", False, None), ("nn", True, None), ("est", False, "est")):
                ds = SceneDataset(os.path.join(root, scene), ST.PAIR_TXT, resize, None, one_nn, est)
                smp = [ds[i] for i in range(len(ds))]
                pre = f"rd{s}_{tag}_"
                out[pre + "pair_id"] = np.array([x["pair_id"] for x in smp], np.int64)
                out[pre + "depth0"] = np.stack([x["depth0"].numpy() for x in smp]); out[pre + "depth1"] = np.stack([x["depth1"].numpy() for x in smp])
                if tag == "est":
                    continue
                out[pre + "pair_names"] = np.array([list(x["pair_names"]) for x in smp])
                out[pre + "sim"] = np.array([x["sim"] for x in smp], np.float64)
                out[pre + "T_0to1"] = np.stack([x["T_0to1"].numpy() for x in smp])
                for k in ("abs_q_0", "abs_c_0", "abs_q_1", "abs_c_1", "K_color0", "K_color1", "K_depth"):
                    out[pre + k] = np.stack([np.asarray(x[k]) for x in smp])
                out[pre + "scene_id"] = np.array([x["scene_id"] for x in smp]); out[pre + "dataset_name"] = np.array([x["dataset_name"] for x in smp])
                assert out[pre + "T_0to1"].dtype == np.float32 and out[pre + "abs_q_0"].dtype == np.float32 and smp[0]["image0"].shape == (3, resize[1], resize[0])
                assert smp[0]["scene_root"] == os.path.join(root, scene)


# ---------------------------------------------------------------- (b) fusion
def draw_query(rng, k):
    """the recipe of the fixture; every array float64 holding float32 values (what the loader and the plugin hand over)"""
    from scipy.spatial.transform import Rotation
    rot = lambda s: Rotation.from_rotvec(rng.normal(size=3) * s).as_matrix()
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    wxyz = lambda R: Rotation.from_matrix(R).as_quat()[[3, 0, 1, 2]]
    cq, rq = rng.uniform(-1.5, 1.5, 3), rot(0.4)
    q = dict(query_c=f32(cq), query_q=f32(wxyz(rq)), train_c=[], train_q=[], R_pred=[], t_pred=[], R_gt=[], t_gt=[])
    for n in range(k):
        cdb, rdb = cq + rng.uniform(-1, 1, 3), rot(0.4)
        R = rq @ rdb.T
        t = -rq @ (cq - cdb)
        if k >= 3 and n == k - 1:
            Rp, tp = rot(0.5) @ R, rng.normal(size=3)
        else:
            Rp, tp = rot(0.02) @ R, rng.uniform(0.8, 1.2) * (rot(0.04) @ t)
        for key, v in (("train_c", cdb), ("train_q", wxyz(rdb)), ("R_pred", Rp), ("t_pred", tp), ("R_gt", R), ("t_gt", t)):
            q[key].append(f32(v))
    for key in ("train_c", "train_q", "R_pred", "t_pred", "R_gt", "t_gt"):
        q[key] = np.stack(q[key]) if k else np.zeros((0,) + {"train_c": (3,), "train_q": (4,), "R_pred": (3, 3), "t_pred": (3,), "R_gt": (3, 3), "t_gt": (3,)}[key])
    q["inliers"] = rng.integers(0, 500, size=k)
    q["sim"] = np.round(rng.uniform(0, 1, size=k), 3)
    return q


def ref_entry(L, name, q):
    """the pair_data entry benchmark/sevenscenes.py:38-64 builds"""
    from transforms3d.quaternions import mat2quat
    pairs = []
    for n in range(len(q["train_c"])):
        tr = L.AbsPose(q["train_q"][n].copy(), q["train_c"][n].copy())
        lbl = L.RelaPose(mat2quat(q["R_gt"][n]).reshape(-1), q["t_gt"][n].copy())
        prd = L.RelaPose(mat2quat(q["R_pred"][n]).reshape(-1), q["t_pred"][n].copy())
        pr = L.RelaPosePair(name, tr, lbl, prd, float(q["sim"][n]))
        pr.inliers = int(q["inliers"][n])
        pairs.append(pr)
    return {"test_abs_pose": L.AbsPose(q["query_q"].copy(), q["query_c"].copy()), "test_pairs": pairs}


def cos_margin(d, thr):
    """distance of an unrounded cosine from the rounding boundary that decides `degrees(acos(rint(d * 1e4) / 1e4)) < thr`"""
    n = np.arange(-10000, 10001)
    inl = np.degrees(np.arccos(n / 1e4)) < thr
    n_min = n[inl].min()                                          # inlier iff rint(d * 1e4) >= n_min
    return abs(d - (n_min - 0.5) / 1e4)


def query_ok(L, M, q, in_iter, shuffles):
    """run reference and mirror on one query; -> (accepted, record)"""
    name = "q"
    entry = ref_entry(L, name, q)
    k = len(q["train_c"])
    n0 = len(shuffles)
    loc = {}
    with contextlib.redirect_stdout(io.StringIO()):
        L.ransac({name: entry}, THRES, MULT, in_iter=in_iter, pair_type="relapose", err_thres=ERR_THRES, loc_results=loc)
        loc0 = {}
        L.cal_abs_pose_err_metric({name: entry}, ERR_THRES, loc0)
    if len(shuffles) != n0:
        return False, None
    r1, r0 = loc[name], loc0[name]
    inl = [0] if r1["approximated"] else L.find_inliers(r1["abs_pose_pred"], entry["test_pairs"], THRES, pair_type="relapose")
    M.TRACE = dict(cos=[], cond=[], steps=[], draws=[])
    pairs = [M.Pair(q["train_q"][n], q["train_c"][n], q["R_pred"][n], q["t_pred"][n]) for n in range(k)]
    st, mq, mc, minl = M.ransac_query(pairs, float(THRES), MULT, in_iter, 0, 0)
    st0, mq0, mc0 = M.median_query(pairs)
    tr, M.TRACE = M.TRACE, None
    assert minl == list(inl) and (st == M.APPROXIMATED) == bool(r1["approximated"]), "the mirror disagrees with the reference"
    if tr["draws"] or st0 != M.OK:
        return False, None
    if any(cos_margin(d, thr) < 1e-9 for d, thr in tr["cos"]) or any(not (c <= 1e7) for c in tr["cond"]) or \
            any(abs(s - 1e-5) < 1e-9 for s in tr["steps"]):
        return False, None
    rec = dict(abs_q=np.asarray(r1["abs_pose_pred"].q, np.float64), abs_c=np.asarray(r1["abs_pose_pred"].c, np.float64),
               inl=np.array(inl, np.int64), approx=bool(r1["approximated"]), abs_q0=np.asarray(r0["abs_pose_pred"].q, np.float64),
               abs_c0=np.asarray(r0["abs_pose_pred"].c, np.float64), ncos=len(tr["cos"]), cond=max(tr["cond"], default=0.0))
    return True, rec


def _lines(text, drop=None):
    lines = [l for l in text.split("\n") if not (drop and l.startswith(drop))]
    while lines and lines[-1] == "":
        lines.pop()
    return lines


def fusion_part(out, L, M):
    shuffles = []
    real_shuffle = np.random.shuffle
    np.random.shuffle = lambda x: (shuffles.append(1), real_shuffle(x))[1]
    result_with, result_without = {}, {}
    drawn = rejected = ncos = 0
    worst_cond = 0.0
    for k, nq, in_iter in GROUPS:
        rng = np.random.default_rng(7000 + k)
        qs, recs = [], []
        while len(qs) < nq:
            q = draw_query(rng, k)
            drawn += 1
            ok, rec = query_ok(L, M, q, in_iter, shuffles)
            if not ok:
                rejected += 1
                continue
            qs.append(q); recs.append(rec)
            ncos += rec["ncos"]; worst_cond = max(worst_cond, rec["cond"])
        pre = f"k{k}_"
        for key in ("query_c", "query_q", "train_c", "train_q", "R_pred", "t_pred", "R_gt", "t_gt", "inliers", "sim"):
            out[pre + key] = np.stack([q[key] for q in qs])
        out[pre + "in_iter"] = np.int64(in_iter)
        for key in ("abs_q", "abs_c", "abs_q0", "abs_c0"):
            out[pre + key] = np.stack([r[key] for r in recs])
        mask = np.zeros((nq, k), np.int32)
        for i, r in enumerate(recs):
            mask[i, r["inl"]] = 1
        out[pre + "inlier_mask"] = mask
        out[pre + "approx"] = np.array([r["approx"] for r in recs])
        # the group as one scene through the reference's two evaluations
        pair_data = {f"seq-k{k}/frame-{i:06d}.color.png": ref_entry(L, f"seq-k{k}/frame-{i:06d}.color.png", q) for i, q in enumerate(qs)}
        loc1, loc0 = {}, {}
        with contextlib.redirect_stdout(io.StringIO()):
            tested, approx_q, pass_rate, err_res = L.ransac(pair_data, THRES, MULT, in_iter=in_iter, pair_type="relapose", err_thres=ERR_THRES,
                                                            loc_results=loc1)
            m0 = L.cal_abs_pose_err_metric(pair_data, ERR_THRES, loc0)
        out[pre + "r_tested"], out[pre + "r_approx_num"] = np.int64(tested), np.int64(len(approx_q))
        out[pre + "r_pass_rate"], out[pre + "r_err_res"] = np.array(pass_rate, np.float64), np.array(err_res, np.float64)
        out[pre + "r_abs_t_err"] = np.array([loc1[n]["abs_t_err"] for n in pair_data]); out[pre + "r_abs_r_err"] = np.array([loc1[n]["abs_r_err"] for n in pair_data])
        out[pre + "r_conf"] = np.array([loc1[n]["inliers"] for n in pair_data], np.int64)
        out[pre + "m_medians"] = np.array([float(v) for v in m0[:3]]); out[pre + "m_passed"] = np.asarray(m0[3], np.float64); out[pre + "m_ap"] = np.float64(m0[4])
        out[pre + "m_abs_t_err"] = np.array([loc0[n]["abs_t_err"] for n in pair_data]); out[pre + "m_abs_r_err"] = np.array([loc0[n]["abs_r_err"] for n in pair_data])
        rt, rq = L.cal_rela_pose_err(pair_data)
        out[pre + "m_rela"] = np.array([rt, rq], np.float64)
        prec, rec_, ap = L.precision_recall_pose_error(out[pre + "r_conf"], out[pre + "r_abs_t_err"], out[pre + "r_abs_r_err"], 3, ERR_THRES[1])
        out[pre + "pr_prec"], out[pre + "pr_rec"], out[pre + "pr_ap"] = np.asarray(prec, np.float64), np.asarray(rec_, np.float64), np.float64(ap)
        with tempfile.TemporaryDirectory() as td:                # the pose_<scene>.txt lines of both routes
            for tag, loc in (("r", loc1), ("m", loc0)):
                path = os.path.join(td, f"{tag}.npy")
                np.save(path, {f"k{k}": loc})
                L.save_results_visualisation(path)
                out[pre + f"{tag}_pose_lines"] = np.array(open(os.path.join(td, f"pose_k{k}.txt")).read().split("\n")[:-1])
        if in_iter == 10:
            result_with[f"k{k}"] = {"pair_data": pair_data, "no_pt_pairs": []}
    assert rejected * 10 <= drawn, f"{rejected} of {drawn} draws rejected"
    np.random.shuffle = real_shuffle
    out["stats_drawn_rejected_ncos"] = np.array([drawn, rejected, ncos], np.int64); out["stats_worst_cond"] = np.float64(worst_cond)
    # (c) a scene with a query that has no pair at all, then both printed reports
    mixed = {}
    for n, (k, i) in enumerate(((2, 0), (0, 0), (3, 1), (5, 2), (1, 3))):
        name = f"seq-mix/frame-{n:06d}.color.png"
        q = dict(query_c=out["k2_query_c"][0], query_q=out["k2_query_q"][0], train_c=np.zeros((0, 3))) if k == 0 else \
            {key: out[f"k{k}_{key}"][i] for key in ("query_c", "query_q", "train_c", "train_q", "R_pred", "t_pred", "R_gt", "t_gt", "inliers", "sim")}
        mixed[name] = ref_entry(L, name, q)
    out["mixed_members"] = np.array([[2, 0], [0, 0], [3, 1], [5, 2], [1, 3]], np.int64)
    result_with["mixed_scene_long_name"] = {"pair_data": mixed, "no_pt_pairs": [("a", "b")]}
    with tempfile.TemporaryDirectory() as td:
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            best, avg_pass = L.eval_pipeline_with_ransac(result_with, None, ransac_thres=[THRES], ransac_iter=10, ransac_miu=MULT,
                                                         pair_type="relapose", err_thres=ERR_THRES, save_res_path=os.path.join(td, "r.npy"))
        out["report_ransac_lines"] = np.array(_lines(buf.getvalue(), drop="Ransac testing time"))
        L.save_results_visualisation(os.path.join(td, "r.npy"))
        out["mixed_r_pose_lines"] = np.array(open(os.path.join(td, "pose_mixed_scene_long_name.txt")).read().split("\n")[:-1])
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            ev, avg_passed = L.eval_pipeline_without_ransac(result_with, err_thres=ERR_THRES, save_res_path=os.path.join(td, "m.npy"))
        out["report_median_lines"] = np.array(_lines(buf.getvalue()))
        out["report_median_eval"], out["report_median_passed"] = np.array(ev, np.float64), np.asarray(avg_passed, np.float64)
        L.save_results_visualisation(os.path.join(td, "m.npy"))
        out["mixed_m_pose_lines"] = np.array(open(os.path.join(td, "pose_mixed_scene_long_name.txt")).read().split("\n")[:-1])
    out["report_scenes"] = np.array(list(result_with))
    return drawn, rejected, ncos, worst_cond


def save_npz_deterministic(path, arrays):
    """np.savez_compressed with a fixed timestamp in every zip entry: the same arrays give the same bytes"""
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    stub_modules()
    import matplotlib
    matplotlib.use("Agg")
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.join(HERE, "..", "tests"))
    from lib.utils import localize as L
    import abs_pose_ref as M
    out = {}
    reader_part(out)
    drawn, rejected, ncos, cond = fusion_part(out, L, M)
    save_npz_deterministic(OUT, out)
    print(f"wrote {os.path.normpath(OUT)}: {len(out)} arrays, {os.path.getsize(OUT)} bytes; {drawn} queries drawn, {rejected} rejected, "
          f"{ncos} inlier decisions, worst conditioning {cond:.3g}")


if __name__ == "__main__":
    main()
