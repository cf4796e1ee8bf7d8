"""Host side of the 7Scenes evaluation (lib/utils/localize.py): error measures, precision / recall, the report lines of
eval_pipeline_without_ransac (:164-208) and eval_pipeline_with_ransac (:120-161), and the pose_<scene>.txt lines of
save_results_visualisation (:51-69).  The fusion itself -- a query's absolute pose from its relative poses -- runs on the device
(localize_ops.fuse_abs_pose, one launch per scene); there is no CPU route.

A scene's predictions are plain arrays (`ScenePairs`), not pickled objects: queries in the order they first appear in the loader, their
pairs in loader order, pairs without a finite pose marked invalid (the reference's `no_pt_pairs`, benchmark/sevenscenes.py:55-56).
Everything is evaluated in float64 on the float32 values the loader and the plugin hand over (the reference keeps whatever dtype numpy's
promotion gives each expression, float32 for most of them).

The reference's conventions differ between the two routes and are kept: medians over queries; the no-RANSAC recall divides by every
query, the RANSAC one by the tested count; a query without pairs counts 1000 m / 180 deg in the RANSAC route and as a failure of the
no-RANSAC route's AP; the no-RANSAC angle error of the centre is a median over neighbours, the RANSAC one a mean over inlier pairs
(0 for an approximated query); confidence is the first pair's inliers (no RANSAC) or the sum over inlier pairs (RANSAC).
"""
import numpy as np

from .evaluation import precision_recall, quat2mat

ERR_THRES = ((0.1, 5), (0.25, 5), (0.5, 10), (1, 20))      # (metres, degrees), benchmark/sevenscenes.py:95


# ---------------------------------------------------------------- quaternions (wxyz)
def mat2quat(M):
    """the largest eigenvector of the symmetric 4x4 built from M, w >= 0: the form the device fusion evaluates (csrc/abs_pose.hip) and the
    reference's library uses.  (submission.mat2quat is the pivot form: the same on a rotation, another function on the plugin's float32
    matrices, which are not exactly orthonormal.)"""
    m = np.asarray(M, np.float64).reshape(3, 3)
    K = np.zeros((4, 4))
    K[0, 0], K[1, 1], K[2, 2], K[3, 3] = m[0, 0] - m[1, 1] - m[2, 2], m[1, 1] - m[0, 0] - m[2, 2], m[2, 2] - m[0, 0] - m[1, 1], np.trace(m)
    K[1, 0], K[2, 0], K[2, 1] = m[0, 1] + m[1, 0], m[0, 2] + m[2, 0], m[1, 2] + m[2, 1]
    K[3, 0], K[3, 1], K[3, 2] = m[2, 1] - m[1, 2], m[0, 2] - m[2, 0], m[1, 0] - m[0, 1]
    vals, vecs = np.linalg.eigh(K / 3.0)                   # (reads the lower triangle)
    q = vecs[[3, 0, 1, 2], np.argmax(vals)]
    return -q if q[0] < 0 else q


# ---------------------------------------------------------------- error measures (:14-48)
def cal_vec_angle_error(label, pred):
    label, pred = np.atleast_2d(np.asarray(label, np.float64)), np.atleast_2d(np.asarray(pred, np.float64))
    with np.errstate(all='ignore'):
        v1 = pred / np.linalg.norm(pred, axis=1, keepdims=True)
        v2 = label / np.linalg.norm(label, axis=1, keepdims=True)
        d = np.around(np.sum(np.multiply(v1, v2), axis=1, keepdims=True), decimals=4)
        error = np.degrees(np.arccos(np.clip(d, a_min=-1, a_max=1)))
    error[np.isnan(error)] = 0.0
    return error


def cal_quat_angle_error(label, pred):
    label, pred = np.asarray(label, np.float64), np.asarray(pred, np.float64)
    assert label.shape == (4,) and pred.shape == (4,)
    q1, q2 = pred / np.linalg.norm(pred), label / np.linalg.norm(label)
    d = np.clip(np.abs(np.sum(q1 * q2)), -1, 1)
    return np.array([[2 * np.degrees(np.arccos(d))]])


# ---------------------------------------------------------------- precision / recall (evaluation.precision_recall)
def precision_recall_pose_error(inliers, terr, rerr, failures, pose_threshold):
    """true positive = both errors within (metres, degrees); -> (precision, recall, average precision) over the confidence thresholds"""
    max_t, max_r = pose_threshold
    ok = (np.asarray(terr).reshape(-1) <= max_t) & (np.asarray(rerr).reshape(-1) <= max_r)
    assert len(inliers) == len(ok)
    return precision_recall(inliers, ok, failures)


def precision_recall_repr_error(inliers, reprerr, failures, repr_threshold):
    ok = np.asarray(reprerr).reshape(-1) < repr_threshold
    assert len(inliers) == len(ok)
    return precision_recall(inliers, ok, failures)


# ---------------------------------------------------------------- a scene's predictions
class ScenePairs:
    """query_names [Q], query_q [Q,4] wxyz, query_c [Q,3]; per pair (grouped by query, loader order inside a query): pair_query [P] (query
    index), train_q [P,4], train_c [P,3], R_pred [P,3,3], t_pred [P,3], R_gt [P,3,3], t_gt [P,3], sim [P], inliers [P] (the plugin's
    confidence), valid [P] (the pose is finite)"""
    FIELDS = ('query_names', 'query_q', 'query_c', 'pair_query', 'train_q', 'train_c', 'R_pred', 't_pred', 'R_gt', 't_gt', 'sim', 'inliers', 'valid')

    def __init__(self, **kw):
        for k in self.FIELDS:
            setattr(self, k, np.asarray(kw[k]))
        f = lambda a, *shape: np.asarray(a, np.float64).reshape(-1, *shape)
        self.query_q, self.query_c = f(self.query_q, 4), f(self.query_c, 3)
        self.train_q, self.train_c = f(self.train_q, 4), f(self.train_c, 3)
        self.R_pred, self.t_pred, self.R_gt, self.t_gt = f(self.R_pred, 3, 3), f(self.t_pred, 3), f(self.R_gt, 3, 3), f(self.t_gt, 3)
        self.pair_query, self.valid = np.asarray(self.pair_query, np.int64).reshape(-1), np.asarray(self.valid, bool).reshape(-1)
        self.inliers = np.asarray(self.inliers).reshape(-1)
        assert (np.diff(self.pair_query) >= 0).all(), 'pairs must be grouped by query'

    def arrays(self, prefix=''):
        return {prefix + k: getattr(self, k) for k in self.FIELDS}

    def fusion_inputs(self):
        """the valid pairs and the offsets of every query's run among them"""
        keep = np.nonzero(self.valid)[0]
        counts = np.bincount(self.pair_query[keep], minlength=len(self.query_names))
        offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        return keep, offsets

    def rela_errors(self, keep):
        """per valid pair: translation angle and rotation angle between prediction and label (:221-224)"""
        with np.errstate(all='ignore'):
            t_err = np.array([cal_vec_angle_error(self.t_pred[i], self.t_gt[i]).item() for i in keep])
            q_err = np.array([cal_quat_angle_error(mat2quat(self.R_pred[i]), mat2quat(self.R_gt[i])).item() for i in keep])
        return t_err, q_err


def cal_rela_pose_err(sp):
    """:211-225: medians of the relative translation-angle and rotation-angle errors over every pair that has a pose"""
    t_err, q_err = sp.rela_errors(np.nonzero(sp.valid)[0])
    return np.median(t_err), np.median(q_err)


def fuse_scene(sp, triang, thres=15.0, thr_mult=1.414, lo_iters=10, seed=0, fuse=None):
    """one launch of the device fusion over the scene's queries -> dict of numpy arrays (abs_q, abs_c, inlier_mask over the VALID pairs,
    status) plus keep / offsets.  `fuse` replaces localize_ops.fuse_abs_pose (tests hand in recorded results)."""
    keep, offsets = sp.fusion_inputs()
    if fuse is None:
        from .localize_ops import fuse_abs_pose as fuse
    out = fuse(sp.train_q[keep], sp.train_c[keep], sp.R_pred[keep].reshape(-1, 9), sp.t_pred[keep], offsets, 1 if triang else 0,
               float(thres), float(thr_mult), int(lo_iters), int(seed))
    out = {k: (v.cpu().numpy() if hasattr(v, 'cpu') else np.asarray(v)) for k, v in out.items()}
    out.update(keep=keep, offsets=offsets)
    return out


def _abs_t(q, c):
    return -quat2mat(q).dot(c)                              # AbsPose.t (:916)


# ---------------------------------------------------------------- the two evaluations
def eval_scene_without_ransac(sp, fused, err_thres=ERR_THRES):
    """cal_rela_pose_err + cal_abs_pose_err_metric (:181-187) -> dict"""
    keep, off = fused['keep'], fused['offsets']
    t_err, q_err = sp.rela_errors(keep)
    abs_c_dist_err, abs_c_ang_err, abs_q_err, conf, names, poses = [], [], [], [], [], []
    passed, failures = [0] * len(err_thres), 0
    for qi in range(len(sp.query_names)):
        a, b = int(off[qi]), int(off[qi + 1])
        if a == b:
            failures += 1
            continue
        rows = keep[a:b]
        c, q = fused['abs_c'][qi], fused['abs_q'][qi]
        cerr = np.linalg.norm(sp.query_c[qi] - c)
        qerr = cal_quat_angle_error(sp.query_q[qi], q).item()
        tc = sp.train_c[rows]
        abs_c_dist_err.append(cerr)
        abs_c_ang_err.append(np.median(cal_vec_angle_error(sp.query_c[qi] - tc, c - tc)))
        abs_q_err.append(qerr)
        conf.append(sp.inliers[rows[0]])
        for i_e, e in enumerate(err_thres):
            passed[i_e] += bool(cerr < e[0] and qerr < e[1])
        names.append(str(sp.query_names[qi])); poses.append((q, _abs_t(q, c)))
    prec, rec, ap = precision_recall_pose_error(conf, abs_c_dist_err, abs_q_err, failures, err_thres[1])
    with np.errstate(all='ignore'):
        med = lambda a: np.median(a) if len(a) else np.nan
        return dict(samples=len(sp.query_names), no_pt_pairs=int((~sp.valid).sum()), rela_t_err=med(t_err), rela_q_err=med(q_err),
                    abs_c_dist_err=med(abs_c_dist_err), abs_c_ang_err=med(abs_c_ang_err), abs_q_err=med(abs_q_err),
                    passed=100.0 * np.array(passed) / len(sp.query_names), average_precision=ap, precision=prec, recall=rec,
                    abs_t_errs=np.array(abs_c_dist_err), abs_r_errs=np.array(abs_q_err), confidence=np.array(conf), failures=failures,
                    names=names, poses=poses)


def eval_scene_with_ransac(sp, fused, err_thres=ERR_THRES):
    """ransac()'s bookkeeping around the fused pose (:480-635) -> dict"""
    from .localize_ops import APPROXIMATED
    keep, off = fused['keep'], fused['offsets']
    t_err, q_err = sp.rela_errors(keep)
    abs_c_dist_err, abs_c_ang_err, abs_q_err, rela_t_err, rela_q_err = [], [], [], [], []
    conf, names, poses, approx, terrs, rerrs = [], [], [], [], [], []
    passed = [0] * len(err_thres)
    for qi in range(len(sp.query_names)):
        a, b = int(off[qi]), int(off[qi + 1])
        if a == b:
            cerr, qerr = 1000, 180
            abs_c_dist_err.append(cerr); abs_c_ang_err.append(qerr); abs_q_err.append(qerr); rela_t_err.append(qerr); rela_q_err.append(qerr)
        else:
            inl = a + np.nonzero(fused['inlier_mask'][a:b])[0]
            rows = keep[inl]
            c, q = fused['abs_c'][qi], fused['abs_q'][qi]
            approximated = int(fused['status'][qi]) == APPROXIMATED
            rela_t_err.append(np.mean(t_err[inl])); rela_q_err.append(np.mean(q_err[inl]))
            cerr = np.linalg.norm(sp.query_c[qi] - c)
            abs_c_dist_err.append(cerr)
            tc = sp.train_c[rows]
            abs_c_ang_err.append(0.0 if approximated else np.mean(cal_vec_angle_error(sp.query_c[qi] - tc, c - tc)))
            qerr = cal_quat_angle_error(sp.query_q[qi], q).item()
            abs_q_err.append(qerr)
            if approximated:
                approx.append(str(sp.query_names[qi]))
            conf.append(sp.inliers[rows].sum()); names.append(str(sp.query_names[qi])); poses.append((q, _abs_t(q, c)))
            terrs.append(cerr); rerrs.append(qerr)
        for i_e, e in enumerate(err_thres):
            passed[i_e] += bool(cerr < e[0] and qerr < e[1])
    tested = len(abs_c_dist_err)
    failures = len(sp.query_names) - len(names)
    prec, rec, ap = precision_recall_pose_error(conf, terrs, rerrs, failures, err_thres[1]) if names else (np.array([1.0]), np.array([0.0]), 0.0)
    return dict(tested=tested, approx_queries=approx, pass_rate=[100.0 * n / tested for n in passed],
                err_res=(np.median(rela_t_err), np.median(rela_q_err), np.median(abs_c_dist_err), np.median(abs_c_ang_err), np.median(abs_q_err)),
                average_precision=ap, precision=prec, recall=rec, abs_t_errs=np.array(terrs), abs_r_errs=np.array(rerrs),
                confidence=np.array(conf), failures=failures, names=names, poses=poses)


def report_without_ransac(results):
    """results: {scene: eval_scene_without_ransac(...)} in scene order -> the printed lines (:177-207, the timing-free ones)"""
    lines = []
    for scene, r in results.items():
        lines.append('>>Testing dataset: {}, testing samples: {}, failures {}'.format(scene, r['samples'], r['no_pt_pairs']))
        lines.append('rela_err (t{:.2f}deg, r{:.2f}deg) abs err: (t{:.2f}m/{:.2f}deg, r{:.2f}deg), Recall: {}. AP: {:.2f}'.format(
            r['rela_t_err'], r['rela_q_err'], r['abs_c_dist_err'], r['abs_c_ang_err'], r['abs_q_err'],
            '/'.join('{:.2f}%'.format(v) for v in r['passed']), r['average_precision']))
    avg_passed = np.stack([r['passed'] for r in results.values()]).mean(axis=0)
    ev = tuple(np.mean([r[k] for r in results.values()]) for k in ('rela_t_err', 'rela_q_err', 'abs_c_dist_err', 'abs_c_ang_err', 'abs_q_err'))
    lines.append('>>avg_rela_err (t{eval_val[0]:.2f}deg, r{eval_val[1]:.2f}deg) avg_abs_err (t{eval_val[2]:.2f}m/{eval_val[3]:.2f}deg, r{eval_val[4]:.2f}deg). Pass:'.format(
        eval_val=ev) + '/'.join('{:.2f}%'.format(v) for v in avg_passed))
    return lines, ev, avg_passed


def report_with_ransac(results, thres, ransac_iter=10, ransac_miu=1.414, err_thres=ERR_THRES, header=True):
    """results: {scene: eval_scene_with_ransac(...)} for ONE threshold -> the printed lines (:122-155)"""
    lines = []
    if header:
        lines.append('>>>>Evaluate model with Ransac(iter={}, miu={}) Error thres:{})'.format(ransac_iter, ransac_miu, err_thres))
    lines.append('\n>>Ransac threshold:{}'.format(thres))
    for scene, r in results.items():
        lines.append('Dataset:{dataset} Bad/All:{approx_num}/{tested_num}, Rela:(t{err_res[0]:.2f}deg, r{err_res[1]:.2f}deg) Abs:(t{err_res[2]:.2f}m/{err_res[3]:.2f}deg, r{err_res[4]:.2f}deg) Pass:'.format(
            dataset=scene[0:min(10, len(scene))], approx_num=len(r['approx_queries']), tested_num=r['tested'], err_res=r['err_res']) +
            '/'.join('{:.2f}%'.format(v) for v in r['pass_rate']))
    avg_err = tuple(np.mean([r['err_res'] for r in results.values()], axis=0))
    avg_pass = tuple(np.mean([r['pass_rate'] for r in results.values()], axis=0)) if len(err_thres) > 1 else tuple(r['pass_rate'] for r in results.values())
    lines.append('Avg: Rela:(t{err_res[0]:.2f}deg, r{err_res[1]:.2f}deg) Abs:(t{err_res[2]:.2f}m/{err_res[3]:.2f}deg, r{err_res[4]:.2f}deg) Pass:'.format(
        err_res=avg_err) + '/'.join('{:.2f}%'.format(v) for v in avg_pass))
    return lines, avg_err, avg_pass


def pose_file_lines(result):
    """save_results_visualisation (:51-69) for one scene: `<query> <q> <t> <inliers> \\n` per localised query"""
    fmt = {'float': lambda v: f'{v:.6f}'}
    out = []
    for name, (q, t), inl in zip(result['names'], result['poses'], result['confidence']):
        q_str = np.array2string(np.asarray(q), formatter=fmt, max_line_width=1000)[1:-1]
        t_str = np.array2string(np.asarray(t), formatter=fmt, max_line_width=1000)[1:-1]
        out.append(f'{name} {q_str} {t_str} {inl} \n')
    return out
