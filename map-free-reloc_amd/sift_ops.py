"""SIFT keypoint detection + description on the GPU (csrc/sift.hip, include/mfr_hip.h mfr_sift_*): the detectAndCompute of
OpenCV 4.8 `SIFT_create(nfeatures)` with every other parameter at its default, which the reference calls in SIFTMatching
(lib/models/matching/feature_matching.py:58,82-83, cfg.SIFT.NUM_FEATURES) and SIFT_matcher (etc/feature_matching_baselines/
matchers.py:146-147, 2048).  Torch only provides memory and the stream.

The steps, as this implementation pins them (tests/sift_cpu_ref.py restates them in numpy f32; the kernels equal it bit for
bit).  OpenCV's source is not part of this project; the table is OpenCV's public algorithm with the choices marked
"unpinned" made here where OpenCV's result depends on its implementation (like MAGSAC++ / P3P).

| step | what | constants |
|---|---|---|
| base | u8 -> f32 (fixed-point scale 1), 2x bilinear upsample, half-pixel centres (src = dst/2 - 1/4), clamped borders; exact in f32 | firstOctave = -1 |
| base blur | Gaussian with sig_diff = sqrt(max(1.6^2 - (2*0.5)^2, 0.01)) | 1.2490 |
| octaves | nOctaves = cvRound(log2(min(2W, 2H)) - 2) + 1, on the doubled base (9 for 540x720; the 9th octave is 4x5 pixels and, like the 8th, has no pixel inside the border) | |
| levels | 6 per octave; level i = blur(level i-1, sqrt(s_t^2 - s_p^2)), s_p = 1.6 k^(i-1), s_t = s_p k, k = 2^(1/3) | 1.2263, 1.5450, 1.9466, 2.4525, 3.0900 |
| blur | ksize = cvRound(8 sigma + 1) | 1, taps exp(-x^2 / (2 sigma^2)) in binary64 normalised to sum 1, rounded to f32; reflect-101; row pass then column pass in f32, each acc = c0 p0 + sum_{i=1..R} c_i (p_-i + p_i) in increasing i (unpinned: OpenCV's own summation order) | radius <= 13 |
| next octave | level 0 = every second pixel of level 3 of the previous octave, floor sizes | |
| DoG | 5 per octave, f32 difference of adjacent levels | |
| extrema | DoG layers 1..3, 5-pixel border, abs(v) > floor(0.5*0.04/3*255) = 1 and v >= all 26 neighbours (v > 0) or <= (v < 0) | |
| refinement | <= 5 Newton steps, derivatives x 1/255 (first x 0.5, cross x 0.25); the 3x3 system by Cramer's rule in binary64 (unpinned: OpenCV's Matx solve); stop when all offsets < 0.5, reject when leaving layers 1..3 / the border or after 5 steps; reject abs(contr) * 3 < 0.04, det <= 0 or tr^2 * 10 >= 121 det | |
| keypoint | pt = (c + xc, r + xr) 2^o, size = 1.6 * 2^((layer + xi)/3) * 2^o * 2, response = abs(contr), octave = o + (layer << 8) + (cvRound((xi + 0.5) * 255) << 16) | |
| orientation | 36 bins, radius cvRound(4.5 s), weight exp(-(i^2 + j^2) / (2 (1.5 s)^2)), s = size / 2^(o+1); central differences at interior pixels; angle by cv::fastAtan2's polynomial; bin cvRound(0.1 ori) mod 36; samples summed in row-major order; smoothing [1 4 6 4 1]/16 circular | |
| peaks | above both neighbours and >= 0.8 max; parabolic bin, angle = 360 - 10 bin, 0 within FLT_EPSILON of 360 | |
| output frame | pt, size halved; octave byte - 1 | |
| selection | removeDuplicatedSorted (equal x, y, size, angle), then retainBest(nfeatures): every keypoint whose response >= the nfeatures-th largest (ties kept) | nfeatures = 0: all |
| order | ascending x, then y, then size DESCENDING, angle, response descending, octave descending: the order OpenCV's KeyPoint_LessThan sort leaves (unpinned: OpenCV's final order comes from std::nth_element) | |
| descriptor | 4x4 cells x 8 bins on the keypoint's Gaussian level; hist_width = 3 s, radius cvRound(hist_width sqrt2 5/2) (<= image diagonal), rotated by 360 - angle; weight exp(-(x^2 + y^2)/8) in cell units, trilinear; samples in row-major order | |
| normalisation | L2, clip at 0.2 norm, scale 512 / max(norm, FLT_EPSILON), saturate_cast<uchar> (round half even, clamp 0..255), returned as f32 | |
| arithmetic | divides, square roots, exp / exp2 / cos / sin in binary64 rounded once to f32 (unpinned: OpenCV's hal::exp32f and SIMD magnitude) | |
"""
import numpy as np
import torch

from . import _lib

ST_CAND_OVERFLOW, ST_KPT_OVERFLOW, ST_OUT_OVERFLOW = 1, 2, 4
LEVELS = 6


def num_octaves(H, W):
    import math
    return int(np.rint(math.log(min(2 * H, 2 * W)) / math.log(2.0) - 2)) + 1


def plane_to_u8(gray):
    """[..., H, W] f32 gray plane in [0, 1] whose values are bytes / 255 (the loaders' plane, datasets.gray_plane) -> u8 bytes"""
    return (gray.float() * 255.0).round().clamp_(0, 255).to(torch.uint8)


class SiftDetector:
    """SiftDetector(nfeatures, device)(gray [B,H,W] u8, or f32 holding whole numbers 0..255) -> dict(kpts [B,Nmax,2], desc
    [B,Nmax,128], n [B] i32, size, angle, response [B,Nmax] f32, octave [B,Nmax] i32, status [B] i32).  Rows >= n are zero.
    Nmax = nfeatures + `slack` (retainBest keeps every tie of the last response), or 16384 for nfeatures = 0."""

    def __init__(self, nfeatures=0, device="cuda", slack=256, cand_cap=0):
        self.nfeatures = int(nfeatures or 0)
        self.device = torch.device(device)
        self.Nmax = self.nfeatures + int(slack) if self.nfeatures > 0 else 16384
        self.cand_cap = int(cand_cap)
        self._ws = {}

    def workspace(self, B, H, W):
        lib = _lib.load(require_gpu=True)
        key = (B, H, W)
        if key not in self._ws:
            nb = lib.mfr_sift_workspace_bytes(B, H, W, self.cand_cap)
            if nb == 0:
                raise ValueError(f"SIFT: unsupported image batch {B}x{H}x{W}")
            self._ws = {key: torch.empty(nb, dtype=torch.uint8, device=self.device)}
        return self._ws[key]

    def level(self, B, H, W, octave, level):
        """Gaussian level `level` of octave `octave` of the last call on a [B,H,W] batch -> [B,Ho,Wo] f32 view"""
        import ctypes as C
        lib = _lib.load(require_gpu=True)
        ho, wo = C.c_int(0), C.c_int(0)
        off = lib.mfr_sift_level_offset(B, H, W, octave, level, C.byref(ho), C.byref(wo))
        if off < 0:
            raise IndexError(f"no level {octave}/{level}")
        ws = self._ws[(B, H, W)]
        return ws[off:off + 4 * B * ho.value * wo.value].view(torch.float32).view(B, ho.value, wo.value)

    def __call__(self, gray):
        _lib.load(require_gpu=True)
        if not (isinstance(gray, torch.Tensor) and gray.is_cuda):
            gray = torch.as_tensor(np.asarray(gray))
            gray = gray.to(self.device)
        if gray.dim() == 2:
            gray = gray[None]
        if gray.dtype != torch.uint8:
            g = gray.float()
            if bool(((g != g.round()) | (g < 0) | (g > 255)).any()):
                raise ValueError("SIFT input: f32 images must hold whole numbers 0..255 (use plane_to_u8 for [0, 1] planes)")
            gray = g.to(torch.uint8)
        gray = gray.contiguous()
        B, H, W = gray.shape
        ws = self.workspace(B, H, W)
        dev, N = gray.device, self.Nmax
        kpts = torch.zeros(B, N, 2, dtype=torch.float32, device=dev)
        desc = torch.zeros(B, N, 128, dtype=torch.float32, device=dev)
        size = torch.zeros(B, N, dtype=torch.float32, device=dev)
        angle = torch.zeros_like(size)
        response = torch.zeros_like(size)
        octave = torch.zeros(B, N, dtype=torch.int32, device=dev)
        n = torch.zeros(B, dtype=torch.int32, device=dev)
        status = torch.zeros(B, dtype=torch.int32, device=dev)
        _lib.call("mfr_sift_detect", gray, B, H, W, self.nfeatures, N, self.cand_cap, ws, ws.numel(), kpts, desc, size, angle, response, octave, n, status)
        return dict(kpts=kpts, desc=desc, n=n, size=size, angle=angle, response=response, octave=octave, status=status)

    def per_image(self, gray_u8):
        """the `detector=` contract of SIFTMatching / SIFT_matcher: gray [H,W] u8 -> (kpts [n,2] f32, desc [n,128] f32)"""
        out = self(gray_u8)
        n = int(out["n"][0])
        return out["kpts"][0, :n].cpu().numpy(), out["desc"][0, :n].cpu().numpy()


def sift_ratio_stage(detector, ratio):
    """FusedPosePipeline's SIFT matcher stage: batch["images"] [2B,1,H,W] gray planes (reference, query interleaved) -> exact u8
    -> detector -> rootSIFT -> exact 2-NN + ratio test -> dict(pts0, pts1, n_corr), all on the device"""
    from .descriptor_ops import rootsift, ratio_match

    def match(b):
        im = b["images"]
        u8 = plane_to_u8(im.reshape(im.shape[0], im.shape[-2], im.shape[-1]))
        f = detector(u8)
        r, q = rootsift(f["desc"])
        return ratio_match(r[0::2], r[1::2], q[0::2], q[1::2], f["kpts"][0::2], f["kpts"][1::2], f["n"][0::2], f["n"][1::2], ratio)
    return match
