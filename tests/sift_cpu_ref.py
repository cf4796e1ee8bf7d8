"""numpy float32 restatement of the SIFT detector in csrc/sift.hip (the semantics table of sift_ops.py), the executable form of the
spec the GPU kernels are pinned against bit for bit.  Every f32 operation is an explicit numpy float32 multiply / add in the order the
kernels use (numpy never fuses); divides, square roots and transcendentals go through binary64 (Python's math / float64 numpy
division, square root) and are rounded once to f32, like the kernels' div_rn / sqrt_rn / exp_rn.  Test infrastructure, not
a library: slow (a Python loop per candidate and keypoint) but independent of the GPU."""
import math

import numpy as np

F = np.float32
LAYERS, LEVELS, BORDER = 3, 6, 5
FLT_EPS = F(1.1920928955078125e-7)


def div_rn(a, b):
    return F(float(a) / float(b))


def sqrt_rn(a):
    return F(math.sqrt(float(a)))


def level_sigma(l):
    sigma, k = 1.6, 2.0 ** (1.0 / LAYERS)
    if l == 0:
        return math.sqrt(max(sigma * sigma - 1.0, 0.01))
    prev = (k ** (l - 1)) * sigma
    tot = prev * k
    return math.sqrt(tot * tot - prev * prev)


def gauss_taps(sigma):
    """getGaussianKernel: ksize = cvRound(8 sigma + 1) | 1, binary64 taps normalised to sum 1, rounded to f32 -> (c[0..R], R)"""
    n = int(np.rint(sigma * 8 + 1)) | 1
    R = n // 2
    s2 = -0.5 / (sigma * sigma)
    cd = [math.exp(s2 * (i - (n - 1) * 0.5) ** 2) for i in range(n)]
    tot = 0.0
    for v in cd:
        tot += v
    inv = 1.0 / tot
    return np.array([F(cd[R + i] * inv) for i in range(R + 1)], F), R


def refl101(p, n):
    if n == 1:
        return np.zeros_like(p)
    p = np.array(p, np.int64)
    while True:
        bad = (p < 0) | (p >= n)
        if not bad.any():
            return p
        p = np.where(p < 0, -p, np.where(p >= n, 2 * n - 2 - p, p))


def blur(img, sigma):
    c, R = gauss_taps(sigma)
    H, W = img.shape
    pad = img[:, refl101(np.arange(-R, W + R), W)]
    acc = c[0] * pad[:, R:R + W]
    for t in range(1, R + 1):
        acc = acc + c[t] * (pad[:, R - t:R - t + W] + pad[:, R + t:R + t + W])
    pad = acc[refl101(np.arange(-R, H + R), H), :]
    out = c[0] * pad[R:R + H]
    for t in range(1, R + 1):
        out = out + c[t] * (pad[R - t:R - t + H] + pad[R + t:R + t + H])
    return out.astype(F, copy=False)


def upsample2(gray_u8):
    g = gray_u8.astype(F)
    H, W = g.shape

    def axis_idx(n):
        x = np.arange(2 * n)
        a = np.where(x & 1, x >> 1, np.maximum((x >> 1) - 1, 0))
        b = np.where(x & 1, np.minimum((x >> 1) + 1, n - 1), x >> 1)
        wa = np.where(x & 1, F(0.75), F(0.25)).astype(F)
        wb = np.where(x & 1, F(0.25), F(0.75)).astype(F)
        return a, b, wa, wb
    xa, xb, wxa, wxb = axis_idx(W)
    ya, yb, wya, wyb = axis_idx(H)
    h = wxa[None] * g[:, xa] + wxb[None] * g[:, xb]
    return (wya[:, None] * h[ya] + wyb[:, None] * h[yb]).astype(F)


def n_octaves(H, W):
    return int(np.rint(math.log(min(2 * H, 2 * W)) / math.log(2.0) - 2)) + 1


def gaussian_pyramid(gray_u8):
    """-> list over octaves of [6, Ho, Wo] f32"""
    H, W = gray_u8.shape
    pyr = []
    for o in range(n_octaves(H, W)):
        if o == 0:
            lv = [blur(upsample2(gray_u8), level_sigma(0))]
        else:
            lv = [np.ascontiguousarray(pyr[o - 1][LAYERS][::2, ::2][:pyr[o - 1].shape[1] // 2, :pyr[o - 1].shape[2] // 2])]
        for l in range(1, LEVELS):
            lv.append(blur(lv[-1], level_sigma(l)))
        pyr.append(np.stack(lv))
    return pyr


def fast_atan2(y, x):
    """cv::fastAtan2 on f32 arrays (degrees)"""
    y, x = np.asarray(y, F), np.asarray(x, F)
    k = F(180.0 / math.pi)
    p1, p3, p5, p7 = F(0.9997878412794807) * k, F(-0.3258083974640975) * k, F(0.1555786518463281) * k, F(-0.04432655554792128) * k
    ax, ay = np.abs(x), np.abs(y)
    eps = F(2.220446049250313e-16)
    big = ax >= ay
    num = np.where(big, ay, ax).astype(np.float64)
    den = np.where(big, ax + eps, ay + eps).astype(np.float64)
    c = (num / den).astype(F)
    c2 = c * c
    poly = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c
    a = np.where(big, poly, F(90) - poly).astype(F)
    a = np.where(x < 0, F(180) - a, a).astype(F)
    a = np.where(y < 0, F(360) - a, a).astype(F)
    return a


def exp_arr(a):
    """elementwise exp through the C library's binary64 exp (numpy's vectorised exp may round differently), rounded to f32"""
    return np.array([F(math.exp(float(v))) for v in np.ravel(a)], F).reshape(np.shape(a))


def sqrt_arr(a):
    return np.sqrt(np.asarray(a, np.float64)).astype(F)


def _refine(dog, layer, r, c):
    """adjustLocalExtrema on one octave's DoG stack [5, H, W] -> None or (layer, r, c, xc, xr, xi, contr)"""
    Ho, Wo = dog.shape[1:]
    img_scale = F(1) / F(255)
    deriv_scale = img_scale * F(0.5)
    second = img_scale
    cross = img_scale * F(0.25)
    xi = xr = xc = F(0)
    D = lambda l, y, x: dog[l, y, x]
    i = 0
    while i < 5:
        v = D(layer, r, c)
        dx = (D(layer, r, c + 1) - D(layer, r, c - 1)) * deriv_scale
        dy = (D(layer, r + 1, c) - D(layer, r - 1, c)) * deriv_scale
        ds = (D(layer + 1, r, c) - D(layer - 1, r, c)) * deriv_scale
        v2 = v * F(2)
        dxx = (D(layer, r, c + 1) + D(layer, r, c - 1) - v2) * second
        dyy = (D(layer, r + 1, c) + D(layer, r - 1, c) - v2) * second
        dss = (D(layer + 1, r, c) + D(layer - 1, r, c) - v2) * second
        dxy = (D(layer, r + 1, c + 1) - D(layer, r + 1, c - 1) - D(layer, r - 1, c + 1) + D(layer, r - 1, c - 1)) * cross
        dxs = (D(layer + 1, r, c + 1) - D(layer + 1, r, c - 1) - D(layer - 1, r, c + 1) + D(layer - 1, r, c - 1)) * cross
        dys = (D(layer + 1, r + 1, c) - D(layer + 1, r - 1, c) - D(layer - 1, r + 1, c) + D(layer - 1, r - 1, c)) * cross
        a00, a01, a02, a11, a12, a22 = float(dxx), float(dxy), float(dxs), float(dyy), float(dys), float(dss)
        b0, b1, b2 = float(dx), float(dy), float(ds)
        det = a00 * (a11 * a22 - a12 * a12) - a01 * (a01 * a22 - a02 * a12) + a02 * (a01 * a12 - a02 * a11)
        X0 = X1 = X2 = F(0)
        if det != 0.0:
            X0 = F((b0 * (a11 * a22 - a12 * a12) - a01 * (b1 * a22 - a12 * b2) + a02 * (b1 * a12 - a11 * b2)) / det)
            X1 = F((a00 * (b1 * a22 - a12 * b2) - b0 * (a01 * a22 - a12 * a02) + a02 * (a01 * b2 - b1 * a02)) / det)
            X2 = F((a00 * (a11 * b2 - b1 * a12) - a01 * (a01 * b2 - b1 * a02) + b0 * (a01 * a12 - a11 * a02)) / det)
        xi, xr, xc = -X2, -X1, -X0
        if abs(xi) < F(0.5) and abs(xr) < F(0.5) and abs(xc) < F(0.5):
            break
        lim = F(2147483647 // 3)
        if abs(xi) > lim or abs(xr) > lim or abs(xc) > lim:
            return None
        c += int(np.rint(xc)); r += int(np.rint(xr)); layer += int(np.rint(xi))
        if layer < 1 or layer > LAYERS or c < BORDER or c >= Wo - BORDER or r < BORDER or r >= Ho - BORDER:
            return None
        i += 1
    if i >= 5:
        return None
    v = D(layer, r, c)
    dx = (D(layer, r, c + 1) - D(layer, r, c - 1)) * deriv_scale
    dy = (D(layer, r + 1, c) - D(layer, r - 1, c)) * deriv_scale
    ds = (D(layer + 1, r, c) - D(layer - 1, r, c)) * deriv_scale
    t = dx * xc + dy * xr + ds * xi
    contr = v * img_scale + t * F(0.5)
    if abs(contr) * F(LAYERS) < F(0.04):
        return None
    v2 = v * F(2)
    dxx = (D(layer, r, c + 1) + D(layer, r, c - 1) - v2) * second
    dyy = (D(layer, r + 1, c) + D(layer, r - 1, c) - v2) * second
    dxy = (D(layer, r + 1, c + 1) - D(layer, r + 1, c - 1) - D(layer, r - 1, c + 1) + D(layer, r - 1, c - 1)) * cross
    tr = dxx + dyy
    det = dxx * dyy - dxy * dxy
    if det <= F(0) or tr * tr * F(10) >= F(121) * det:
        return None
    return layer, r, c, F(xc), F(xr), F(xi), F(contr)


def extrema(pyr):
    """-> list of candidates (o, layer, r, c, xc, xr, xi, contr) in (octave, layer, row, col) scan order"""
    out = []
    for o, G in enumerate(pyr):
        Ho, Wo = G.shape[1:]
        if Ho <= 2 * BORDER or Wo <= 2 * BORDER:
            continue
        dog = (G[1:] - G[:-1]).astype(F)
        for layer in range(1, LAYERS + 1):
            v = dog[layer, BORDER:Ho - BORDER, BORDER:Wo - BORDER]
            pos = v > 0
            ok = np.abs(v) > F(1)
            mx = np.ones_like(ok); mn = np.ones_like(ok)
            for l in (layer - 1, layer, layer + 1):
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        if l == layer and dy == 0 and dx == 0:
                            continue
                        n = dog[l, BORDER + dy:Ho - BORDER + dy, BORDER + dx:Wo - BORDER + dx]
                        mx &= v >= n
                        mn &= v <= n
            sel = ok & np.where(pos, mx, mn)
            for rr, cc in zip(*np.nonzero(sel)):
                res = _refine(dog, layer, int(rr) + BORDER, int(cc) + BORDER)
                if res is not None:
                    out.append((o,) + res)
    return out


def orientations(pyr, cand):
    """calcOrientationHist + peak interpolation -> keypoint rows [x, y, size, angle, response, octave] in the input frame"""
    kps = []
    for (o, layer, r, c, xc, xr, xi, contr) in cand:
        img = pyr[o][layer]
        Ho, Wo = img.shape
        po = F(1 << o)
        ptx = (F(c) + xc) * po
        pty = (F(r) + xr) * po
        octave = o + (layer << 8) + (int(np.rint((float(xi) + 0.5) * 255)) << 16)
        size = F(1.6) * F(2.0 ** float(div_rn(F(layer) + xi, F(LAYERS)))) * po * F(2)
        response = abs(contr)
        scl = size * F(0.5) / po
        radius = int(np.rint(F(4.5) * scl))
        sigma = F(1.5) * scl
        expf_scale = div_rn(F(-1), F(2) * sigma * sigma)
        ii, jj = np.meshgrid(np.arange(-radius, radius + 1), np.arange(-radius, radius + 1), indexing="ij")
        y, x = r + ii.ravel(), c + jj.ravel()
        m = (y > 0) & (y < Ho - 1) & (x > 0) & (x < Wo - 1)
        y, x, i, j = y[m], x[m], ii.ravel()[m], jj.ravel()[m]
        dx = img[y, x + 1] - img[y, x - 1]
        dy = img[y - 1, x] - img[y + 1, x]
        w = exp_arr((i * i + j * j).astype(F) * expf_scale)
        ori = fast_atan2(dy, dx)
        mag = sqrt_arr(dx * dx + dy * dy)
        b = np.rint(F(36.0 / 360.0) * ori).astype(np.int64)          # (36 / 360.f) in f32
        b = np.where(b >= 36, b - 36, b); b = np.where(b < 0, b + 36, b)
        t = np.zeros(36, F)
        np.add.at(t, b, w * mag)                                       # unbuffered, in sample order
        idx = np.arange(36)
        hist = (t[(idx - 2) % 36] + t[(idx + 2) % 36]) * F(1.0 / 16) + (t[(idx - 1) % 36] + t[(idx + 1) % 36]) * F(4.0 / 16) + t * F(6.0 / 16)
        thr = hist.max() * F(0.8)
        for j in range(36):
            hl, hr, hj = hist[(j - 1) % 36], hist[(j + 1) % 36], hist[j]
            if hj > hl and hj > hr and hj >= thr:
                bin_ = F(j) + div_rn(F(0.5) * (hl - hr), hl - F(2) * hj + hr)
                bin_ = F(36) + bin_ if bin_ < 0 else (bin_ - F(36) if bin_ >= F(36) else bin_)
                angle = F(360) - F(10) * bin_
                if abs(angle - F(360)) < FLT_EPS:
                    angle = F(0)
                oct_out = (octave & ~255) | ((octave - 1) & 255)
                kps.append((ptx * F(0.5), pty * F(0.5), size * F(0.5), F(angle), F(response), oct_out))
    return kps


def select(kps, nfeatures):
    """removeDuplicatedSorted + retainBest(nfeatures) (every tie of the last response kept), in (x, y, -size, angle, -response, -octave)
    order -> list of rows"""
    import functools

    def cmp(p, q):
        for k, sgn in ((0, 1), (1, 1), (2, -1), (3, 1), (4, -1), (5, -1)):
            if p[k] != q[k]:
                return -sgn if p[k] < q[k] else sgn
        return 0
    s = sorted(kps, key=functools.cmp_to_key(cmp))
    ded = [p for i, p in enumerate(s) if i == 0 or tuple(p[:4]) != tuple(s[i - 1][:4])]
    if nfeatures > 0 and len(ded) > nfeatures:
        thr = sorted((p[4] for p in ded), reverse=True)[nfeatures - 1]
        ded = [p for p in ded if p[4] >= thr]
    return ded


def descriptor(pyr, kp):
    """calcSIFTDescriptor (d = 4, n = 8) for one keypoint row -> [128] f32 of whole numbers 0..255"""
    x, y, size, angle, _, ow = kp
    octave = ow & 255
    layer = (ow >> 8) & 255
    octave = octave if octave < 128 else (-128 | octave)
    scale = F(1) / F(1 << octave) if octave >= 0 else F(1 << -octave)
    img = pyr[octave + 1][layer]
    Ho, Wo = img.shape
    size = size * scale
    ptfx, ptfy = x * scale, y * scale
    ori = F(360) - angle
    if abs(ori - F(360)) < FLT_EPS:
        ori = F(0)
    scl = size * F(0.5)
    ptx, pty = int(np.rint(ptfx)), int(np.rint(ptfy))
    arg = ori * F(math.pi / 180)
    cos_t, sin_t = F(math.cos(float(arg))), F(math.sin(float(arg)))
    bins_per_rad = F(8.0 / 360.0)
    exp_scale = F(-0.125)
    hist_width = F(3) * scl
    radius = int(np.rint(hist_width * F(1.4142135623730951) * F(5) * F(0.5)))
    radius = min(radius, int(math.sqrt(float(Wo) * Wo + float(Ho) * Ho)))
    cos_t = div_rn(cos_t, hist_width)
    sin_t = div_rn(sin_t, hist_width)
    ii, jj = np.meshgrid(np.arange(-radius, radius + 1), np.arange(-radius, radius + 1), indexing="ij")
    i, j = ii.ravel(), jj.ravel()
    c_rot = j.astype(F) * cos_t - i.astype(F) * sin_t
    r_rot = j.astype(F) * sin_t + i.astype(F) * cos_t
    rbin = r_rot + F(2) - F(0.5)
    cbin = c_rot + F(2) - F(0.5)
    r, c = pty + i, ptx + j
    m = (rbin > -1) & (rbin < 4) & (cbin > -1) & (cbin < 4) & (r > 0) & (r < Ho - 1) & (c > 0) & (c < Wo - 1)
    r, c, rbin, cbin, c_rot, r_rot = r[m], c[m], rbin[m], cbin[m], c_rot[m], r_rot[m]
    dx = img[r, c + 1] - img[r, c - 1]
    dy = img[r - 1, c] - img[r + 1, c]
    w = exp_arr((c_rot * c_rot + r_rot * r_rot) * exp_scale)
    Ori = fast_atan2(dy, dx)
    Mag = sqrt_arr(dx * dx + dy * dy)
    obin = (Ori - ori) * bins_per_rad
    mag = Mag * w
    r0, c0, o0 = np.floor(rbin).astype(np.int64), np.floor(cbin).astype(np.int64), np.floor(obin).astype(np.int64)
    rbin = rbin - r0.astype(F); cbin = cbin - c0.astype(F); obin = obin - o0.astype(F)
    o0 = np.where(o0 < 0, o0 + 8, o0); o0 = np.where(o0 >= 8, o0 - 8, o0)
    v_r1 = mag * rbin; v_r0 = mag - v_r1
    v_rc11 = v_r1 * cbin; v_rc10 = v_r1 - v_rc11
    v_rc01 = v_r0 * cbin; v_rc00 = v_r0 - v_rc01
    v111 = v_rc11 * obin; v110 = v_rc11 - v111
    v101 = v_rc10 * obin; v100 = v_rc10 - v101
    v011 = v_rc01 * obin; v010 = v_rc01 - v011
    v001 = v_rc00 * obin; v000 = v_rc00 - v001
    idx = ((r0 + 1) * 6 + c0 + 1) * 10 + o0
    tgt = np.stack([idx, idx + 1, idx + 10, idx + 11, idx + 60, idx + 61, idx + 70, idx + 71], 1).ravel()
    val = np.stack([v000, v001, v010, v011, v100, v101, v110, v111], 1).ravel()
    hist = np.zeros(360, F)
    np.add.at(hist, tgt, val)                                           # sample by sample, corners in OpenCV's order
    dst = np.zeros(128, F)
    for a in range(4):
        for b in range(4):
            k = ((a + 1) * 6 + b + 1) * 10
            hist[k] = hist[k] + hist[k + 8]
            hist[k + 1] = hist[k + 1] + hist[k + 9]
            dst[(a * 4 + b) * 8:(a * 4 + b) * 8 + 8] = hist[k:k + 8]
    nrm2 = F(0)
    for v in dst:
        nrm2 = nrm2 + v * v
    thr = sqrt_rn(nrm2) * F(0.2)
    nrm2 = F(0)
    dst = np.minimum(dst, thr)
    for v in dst:
        nrm2 = nrm2 + v * v
    fac = div_rn(F(512), max(sqrt_rn(nrm2), FLT_EPS))
    return np.clip(np.rint(dst * fac), 0, 255).astype(F)


def detect(gray_u8, nfeatures=0, pyr=None):
    """gray [H,W] u8 -> dict(kpts [n,2], size, angle, response [n] f32, octave [n] i32, desc [n,128] f32, pyr)"""
    gray_u8 = np.ascontiguousarray(gray_u8, np.uint8)
    if pyr is None:
        pyr = gaussian_pyramid(gray_u8)
    kps = select(orientations(pyr, extrema(pyr)), nfeatures)
    n = len(kps)
    a = np.array([k[:5] for k in kps], F).reshape(n, 5)
    return dict(kpts=a[:, :2].copy(), size=a[:, 2].copy(), angle=a[:, 3].copy(), response=a[:, 4].copy(),
                octave=np.array([k[5] for k in kps], np.int32), desc=np.stack([descriptor(pyr, k) for k in kps]) if n else np.zeros((0, 128), F),
                pyr=pyr)
