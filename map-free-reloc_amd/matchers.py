"""Offline matcher plugins with the reference's API (etc/feature_matching_baselines/matchers.py):
class M(resize: (W, H), outdoor: bool) with match(pair_path: (str, str)) -> ndarray [N,4]
(x0,y0,x1,y1) in the resized pixel frame, or np.full((1,4), nan) when there is no correspondence
(:59, :120); registered in MATCHERS and driven by compute.py (-ds Mapfree -m SG|LoFTR|SIFT|LG|ELoFTR).

Image reading: the reference uses SuperGlue's read_image (cv2.imread GRAYSCALE, cv2.resize of the float
image to (W,H), /255).  cv2 is not available offline: the file is decoded with PIL and the
gray plane is datasets.gray_plane: ITU-R 601-2 luma rounded to a byte, cv2-style half-pixel bilinear
resize of the FLOAT gray image when the size changes, / 255.  At the files' own size (Map-free: 540 x 720 =
config/mapfree.yaml) this is the ONE plane every route of the package feeds the matcher (offline matchers,
batched loaders, online plugin: tests/test_gpu_routes_agree.py).  With a real resize the reference itself has
two orders -- this offline reader resizes the gray image, its dataset class resizes the 8-bit RGB image
(lib/datasets/utils.py:58-74) -- and so has this package: offline = here, every loader / plugin route = the
dataset's order (datasets.MapFreeScene.resize_is_native).  (Unpinned against OpenCV: libjpeg's
own grayscale output can differ from the luma of its RGB output by a grey level; tests/external/gen_cv_golden.py
dumps cv2's planes for three JPEGs when run off-box.)

Weights: upstream checkpoints when present (same file names as matchers.py:17,70), else the seeded
synthetic weights of nets/weights.py with a warning.
"""
import os
import warnings

import numpy as np
import torch

from .nets import weights as WT


def read_image(path, resize):
    from .datasets import read_gray_plane
    return read_gray_plane(path, resize)


def _weights(path, synth, what):
    if path and os.path.exists(path):
        return WT.load_checkpoint(path)
    warnings.warn(f"{what}: checkpoint {path!r} not found -> seeded synthetic weights (results are NOT meaningful)")
    return synth()


def _superpoint(weights_dir, device):
    from .nets.superpoint import SuperPointHIP
    sd = _weights(os.path.join(weights_dir, "superpoint_v1.pth"), WT.superpoint_state_dict, "SuperPoint")
    return SuperPointHIP(sd, device, nms_radius=4, keypoint_threshold=0.005, max_keypoints=1024)                # :65-67


def first_pair_rows(out):
    """the first pair of a batched match dict (pts0, pts1 [B,K,2], n_corr [B]) -> [N,4] rows (x0,y0,x1,y1), or the reference's answer to no
    correspondence: a print and one NaN row (:59, :120)"""
    n = int(out["n_corr"][0])
    if n > 0:
        return torch.cat([out["pts0"][0, :n], out["pts1"][0, :n]], 1).cpu().numpy()
    print("no correspondences")
    return np.full((1, 4), np.nan)


class _GrayPairMatcher:
    """a matcher of two gray planes on the GPU: subclasses set `resize`, `device` and `_net(ims [2,1,H,W]) -> batched match dict`"""

    def match_tensors(self, im0, im1):
        return first_pair_rows(self._net(torch.from_numpy(np.stack([im0, im1]))[:, None].to(self.device)))

    def match(self, pair_path):
        '''return correspondences between images (w/ path pair_path)'''
        return self.match_tensors(read_image(pair_path[0], self.resize), read_image(pair_path[1], self.resize))


class SuperGlue_matcher(_GrayPairMatcher):
    def __init__(self, resize, outdoor=False, weights_dir="SuperGlue/models/weights"):
        from .nets.superglue import SuperGlueHIP
        self.resize, self.device = resize, torch.device("cuda")
        self.sp = _superpoint(weights_dir, self.device)
        sg = _weights(os.path.join(weights_dir, f"superglue_{'outdoor' if outdoor else 'indoor'}.pth"), WT.superglue_state_dict, "SuperGlue")
        self.sg = SuperGlueHIP(sg, self.device, sinkhorn_iterations=20, match_threshold=0.2)                   # :70-71

    def _net(self, ims):
        return self.sg(self.sp(ims), tuple(ims.shape[-2:]))


class LightGlue_matcher(SuperGlue_matcher):
    """SuperPoint + LightGlue (nets/lightglue.py; not in the reference): SuperGlue_matcher with the other matcher network.  weights_dir/lightglue.pth: a
    state dict with the `transformers` LightGlue parameter names"""

    def __init__(self, resize, outdoor=False, weights_dir="LightGlue/weights", sp_weights_dir="SuperGlue/models/weights"):
        from .nets.lightglue import LightGlueHIP
        self.resize, self.device = resize, torch.device("cuda")
        self.sp = _superpoint(sp_weights_dir, self.device)
        self.sg = LightGlueHIP(_weights(os.path.join(weights_dir, "lightglue.pth"), WT.lightglue_state_dict, "LightGlue"), self.device, filter_threshold=0.1)


class LoFTR_matcher(_GrayPairMatcher):
    def __init__(self, resize, outdoor=False, weights_dir="LoFTR/weights", match_type="dual_softmax"):
        """match_type 'dual_softmax': the reference's behaviour (matchers.py:16-18 loads the OT checkpoint strict=False into the dual-softmax
        model, dropping coarse_matching.bin_score); 'sinkhorn': the optimal-transport matcher those weights were trained with"""
        from .nets.loftr import LoFTRHIP
        self.resize, self.device = resize, torch.device("cuda")
        sd = _weights(os.path.join(weights_dir, "outdoor_ot.ckpt" if outdoor else "indoor_ot.ckpt"), WT.loftr_state_dict, "LoFTR")
        self.net = LoFTRHIP(WT.strip_prefix(sd, "matcher."), self.device, match_type=match_type)

    def _net(self, ims):
        from .nets.loftr import pad_to_multiple
        return self.net(pad_to_multiple(ims, 8))


class ELoFTR_matcher(_GrayPairMatcher):
    """EfficientLoFTR (nets/eloftr.py; not in the reference).  weights_dir/efficientloftr.pth: a state dict with the `transformers`
    EfficientLoFTRForKeypointMatching parameter names.  The stage pads to multiples of 32 itself and drops what lies outside the frame."""

    def __init__(self, resize, outdoor=False, weights_dir="EfficientLoFTR/weights"):
        from .nets.eloftr import EfficientLoFTRHIP
        self.resize, self.device = resize, torch.device("cuda")
        self.net = self._net = EfficientLoFTRHIP(_weights(os.path.join(weights_dir, "efficientloftr.pth"), WT.eloftr_state_dict, "EfficientLoFTR"), self.device)


class SIFT_matcher:
    """matchers.py:123-188: 2048 SIFT features, rootSIFT, 2-NN, ratio 0.8.  Detection is OpenCV's (or the
    `detector` callable's); the descriptor leg runs in csrc/descriptor_match.hip."""

    def __init__(self, resize, outdoor=False, detector=None):
        from .descriptor_ops import DescriptorRatioMatcher
        from .matching.feature_matching import _cv_sift_detector
        self.resize = resize
        if detector == "hip":                                                             # csrc/sift.hip (sift_ops.py)
            from .sift_ops import SiftDetector
            detector = SiftDetector(2048).per_image
        self.detector = detector if detector is not None else _cv_sift_detector(2048)     # :146-147
        self.matcher = DescriptorRatioMatcher(0.8)                                          # :145

    def match_arrays(self, img0, img1):
        return first_pair_rows(self.matcher([self.detector(img0)], [self.detector(img1)]))

    def match(self, pair_path):
        g = [np.round(read_image(p, self.resize) * 255.0).astype(np.uint8) for p in pair_path]
        return self.match_arrays(g[0], g[1])


MATCHERS = {'LoFTR': LoFTR_matcher, 'SG': SuperGlue_matcher, 'SIFT': SIFT_matcher, 'LG': LightGlue_matcher, 'ELoFTR': ELoFTR_matcher}
