"""Absolute query pose from relative poses, on the device (csrc/abs_pose.hip, include/mfr_hip.h mfr_abs_pose_fuse): the fusion step of
the 7Scenes benchmark, lib/utils/localize.py `ransac(pair_type='relapose')` (mode 1) and `cal_abs_pose_err_metric` (mode 0), for all
queries of a scene -- or a run -- in one launch.  No CPU fallback.
"""
import numpy as np
import torch

from . import _lib

OK, APPROXIMATED, NO_PAIRS, TOO_MANY, BAD_OFFSETS, ITER_CAP = 0, 1, 2, 3, 4, 16      # include/mfr_hip.h MFR_AP_*
MAX_PAIRS, MAX_LO_ITERS, WEISZFELD_CAP = 64, 62, 256
MODE_MEDIAN, MODE_TRIANG = 0, 1


def _dev(a, dtype, device, shape):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    t = t.to(device=device, dtype=dtype).reshape(shape).contiguous()
    return t


def fuse_abs_pose(train_q, train_c, pred_R, pred_t, offsets, mode, thr_deg=15.0, thr_mult=1.414, lo_iters=10, seed=0, device=None):
    """train_q [P,4] wxyz, train_c [P,3]: the database images' poses; pred_R [P,3,3], pred_t [P,3]: the relative poses database -> query
    (float32 values widen exactly); offsets [Q+1]: the pairs of query i are offsets[i]:offsets[i+1].  The caller has dropped the pairs
    without a finite pose (benchmark/sevenscenes.py:55-56).  Arrays or tensors; they are moved to `device` as float64 / int32.
    -> dict of device tensors: abs_q [Q,4] (mode 1: the unnormalised quaternion mean the reference keeps), abs_c [Q,3], inlier_mask [P]
    int32, status [Q] int32 (OK / APPROXIMATED / NO_PAIRS / TOO_MANY / BAD_OFFSETS, | ITER_CAP in mode 0)."""
    lib = _lib.load(require_gpu=True)
    device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    if mode not in (MODE_MEDIAN, MODE_TRIANG):
        raise ValueError(f"mode: {mode!r}")
    if not 0 <= int(lo_iters) <= MAX_LO_ITERS:
        raise ValueError(f"lo_iters must be in [0, {MAX_LO_ITERS}]")
    if not float(thr_mult) >= 1.0:
        raise ValueError("thr_mult must be >= 1: the local optimisation refits over the inliers at thr_mult * thr_deg")
    offsets = _dev(offsets, torch.int32, device, (-1,))
    Q = offsets.numel() - 1
    if Q < 1:
        raise ValueError("offsets needs at least one query")
    train_q = _dev(train_q, torch.float64, device, (-1, 4))
    P = train_q.shape[0]
    train_c = _dev(train_c, torch.float64, device, (P, 3))
    pred_R = _dev(pred_R, torch.float64, device, (P, 9))
    pred_t = _dev(pred_t, torch.float64, device, (P, 3))
    ws_bytes = int(lib.mfr_abs_pose_workspace_bytes(P))
    ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=device)
    abs_q = torch.empty(Q, 4, dtype=torch.float64, device=device)
    abs_c = torch.empty(Q, 3, dtype=torch.float64, device=device)
    mask = torch.zeros(max(P, 1), dtype=torch.int32, device=device)
    status = torch.empty(Q, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        _lib.call("mfr_abs_pose_fuse", train_q, train_c, pred_R, pred_t, P, offsets, Q, int(mode), float(thr_deg), float(thr_mult), int(lo_iters),
                  int(seed) & 0xFFFFFFFFFFFFFFFF, ws, ws_bytes, abs_q, abs_c, mask, status)
    return dict(abs_q=abs_q, abs_c=abs_c, inlier_mask=mask[:P], status=status)


def test_lo_subsets(seed, base_masks, calls, iters, nsub, device=None):
    """test hook (mfr_test_abs_pose_subset): the random subsets of the local optimisation as bit masks [n, calls, iters] (int64 bit
    patterns), drawn from the set bits of base_masks [n] for (seed, query index, LO call, iteration)"""
    _lib.load(require_gpu=True)
    device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    base = _dev(np.asarray(base_masks, np.uint64).view(np.int64), torch.int64, device, (-1,))
    out = torch.zeros(base.numel(), int(calls), int(iters), dtype=torch.int64, device=device)
    with torch.cuda.device(device):
        _lib.call("mfr_test_abs_pose_subset", int(seed) & 0xFFFFFFFFFFFFFFFF, base, base.numel(), int(calls), int(iters), int(nsub), out)
    return out
