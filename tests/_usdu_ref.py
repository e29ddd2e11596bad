"""numpy restatement of the five 8-bit image rules of the img2img path (include/ldx.h, "8-bit image ops"): what Pillow computes, written out
independently of the package so that the tests can hold the kernels, the package's tables and Pillow itself against one another."""
import math

import numpy as np


def quantize(x):
    """tensor_to_pil: fp32 -> uint8, clamp, times 255.0f, truncate"""
    x = np.clip(np.asarray(x, np.float32), np.float32(0), np.float32(1))
    return (x * np.float32(255.0)).astype(np.uint8)


def to_float(b):
    return np.asarray(b, np.uint8).astype(np.float32) / np.float32(255.0)


def _filter(name):
    if name == "lanczos":
        def sinc(x):
            return 1.0 if x == 0.0 else math.sin(x * math.pi) / (x * math.pi)
        return (lambda x: sinc(x) * sinc(x / 3.0) if -3.0 <= x < 3.0 else 0.0), 3.0
    a = -0.5

    def cubic(x):
        x = -x if x < 0 else x
        if x < 1.0:
            return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
        if x < 2.0:
            return (((x - 5) * x + 8) * x - 4) * a
        return 0.0
    return cubic, 2.0


def coeffs(n_in, n_out, name):
    f, s = _filter(name)
    scale = n_in / n_out
    fs = scale if scale > 1.0 else 1.0
    support = s * fs
    ksize = int(math.ceil(support)) * 2 + 1
    bounds, kk = np.zeros((n_out, 2), np.int32), np.zeros((n_out, ksize), np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = int(center - support + 0.5)
        xmin = 0 if xmin < 0 else xmin
        xmax = int(center + support + 0.5)
        xmax = (n_in if xmax > n_in else xmax) - xmin
        k, total = [], 0.0
        for x in range(xmax):
            w = f((x + xmin - center + 0.5) * (1.0 / fs))
            k.append(w)
            total += w
        for x in range(xmax):
            w = k[x] / total if total != 0.0 else k[x]
            kk[xx, x] = int(-0.5 + w * (1 << 22)) if w < 0 else int(0.5 + w * (1 << 22))
        bounds[xx] = xmin, xmax
    return bounds, kk


def resample_pass(img, axis, n_out, name):
    """img uint8 [H][W][C]; axis 1 = along x, 0 = along y"""
    a = np.moveaxis(np.asarray(img, np.uint8), axis, 0).astype(np.int64)
    bounds, kk = coeffs(a.shape[0], n_out, name)
    out = np.empty((n_out,) + a.shape[1:], np.uint8)
    for i in range(n_out):
        x0, n = bounds[i]
        acc = (1 << 21) + np.tensordot(kk[i, :n].astype(np.int64), a[x0:x0 + n], 1)
        out[i] = np.clip(acc >> 22, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize(img, out_w, out_h, name="lanczos"):
    img = np.asarray(img, np.uint8)
    if out_w != img.shape[1]:
        img = resample_pass(img, 1, out_w, name)
    if out_h != img.shape[0]:
        img = resample_pass(img, 0, out_h, name)
    return img


def box_radius(radius):
    f = np.float32
    s2 = f(radius) * f(radius) / f(3)
    L = f(math.sqrt(12.0 * float(s2) + 1.0))
    l = f(math.floor((float(L) - 1.0) / 2.0))
    a = (f(2) * l + f(1)) * (l * (l + f(1)) - f(3) * s2) / (f(6) * (s2 - (l + f(1)) * (l + f(1))))
    return f(l + a)


def box_weights(fr):
    fr = np.float32(fr)
    R = int(fr)
    ww = int(np.float32(16777216.0) / (fr * np.float32(2) + np.float32(1)))
    return R, ww, ((1 << 24) - (2 * R + 1) * ww) // 2


def box_pass(img, axis, fr):
    """img uint8 [H][W]"""
    R, ww, fw = box_weights(fr)
    a = np.moveaxis(np.asarray(img, np.uint8), axis, 0).astype(np.int64)
    n = a.shape[0]
    idx = np.arange(n)
    acc = np.zeros_like(a)
    for i in range(-R, R + 1):
        acc += a[np.clip(idx + i, 0, n - 1)]
    edge = a[np.clip(idx - R - 1, 0, n - 1)] + a[np.clip(idx + R + 1, 0, n - 1)]
    out = ((ww * acc + fw * edge + (1 << 23)) >> 24).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def gaussian_blur(img, radius):
    fr = box_radius(radius)
    for axis in (1, 1, 1, 0, 0, 0):
        img = box_pass(img, axis, fr)
    return img


def composite(canvas, tile, mask, x0, y0):
    """canvas uint8 [H][W][C] (a copy is returned), tile [h][w][C] at (x0, y0), mask [H][W]"""
    out = np.array(canvas, np.uint8)
    h, w = tile.shape[:2]
    a = mask[y0:y0 + h, x0:x0 + w].astype(np.int64)[..., None]
    d = out[y0:y0 + h, x0:x0 + w].astype(np.int64)
    s = tile.astype(np.int64)
    den = a * 255 + 255 * (255 - a)
    c1 = a * 255 * 255 * 128 // den
    c2 = 255 * 128 - c1
    t = s * c1 + d * c2 + (0x80 << 7)
    r = (((t >> 8) + t) >> 8) >> 7
    out[y0:y0 + h, x0:x0 + w] = np.where(a == 0, d, r).astype(np.uint8)
    return out


def pattern(h, w, c, seed):
    """deterministic pseudo-random bytes [h][w][c] (an integer hash of the position): test inputs that need not be stored"""
    y, x, k = np.meshgrid(np.arange(h, dtype=np.uint64), np.arange(w, dtype=np.uint64), np.arange(c, dtype=np.uint64), indexing="ij")
    m = np.uint64(0xFFFFFFFF)
    v = (x * np.uint64(374761393) + y * np.uint64(668265263) + k * np.uint64(2147483647) + np.uint64(seed) * np.uint64(144665)) & m
    v = ((v ^ (v >> np.uint64(13))) * np.uint64(1274126177)) & m
    return ((v >> np.uint64(16)) & np.uint64(255)).astype(np.uint8)


def smooth_image(h, w, seed):
    """a smooth colour field with a few hard edges, uint8 [h][w][3]: the stand-in and tiny-network runs' input"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.zeros((h, w, 3))
    for c in range(3):
        for _ in range(4):
            fx, fy, ph = rng.uniform(0.5, 3.0), rng.uniform(0.5, 3.0), rng.uniform(0, 6.28)
            img[..., c] += np.sin(2 * np.pi * (fx * x / w + fy * y / h) + ph)
    img = (img - img.min()) / (img.max() - img.min())
    img[h // 5:h // 3, w // 4:w // 2] = (0.9, 0.1, 0.2)
    img[h // 2:h // 2 + h // 6, w // 2:w - w // 8] = (0.05, 0.8, 0.95)
    img[:, w // 3] = 1.0
    img[2 * h // 3] = 0.0
    return np.round(img * 255).astype(np.uint8)


# the stand-in "networks" of the byte-exact pipeline test: what a redrawn tile is, as a function of the cropped tile's bytes
STANDIN = {"redraw": lambda v: 255 - v, "seam": lambda v: v // 2 + 64}


def standin_table(stage):
    """float32 [256]: entry k (the tile value k / 255.0f) -> the redrawn value, as a k' / 255.0f float"""
    v = STANDIN[stage](np.arange(256, dtype=np.int64))
    return v.astype(np.float32) / np.float32(255.0)


RESAMPLE_CASES = [((96, 80), (48, 40)), ((61, 83), (64, 64)), ((40, 40), (40, 64)), ((33, 47), (72, 56)), ((672, 400), (336, 200))]
# (H, W), radius, rectangle (x0, y0, x1, y1) set to 255 or None = pattern()
BLUR_CASES = [((260, 200), 16, (60, 70, 140, 190)), ((260, 200), 16, (0, 0, 64, 64)), ((130, 150), 8, (30, 30, 100, 90)), ((96, 96), 16, None),
              ((50, 40), 16, (5, 5, 30, 30))]
# canvas (W, H), tile, padding, mask blur, seam padding, seam blur
GEOMETRIES = {"g1024": ((1024, 1024), 512, 32, 16, 32, 16), "g200": ((200, 336), 128, 64, 8, 32, 8), "g144": ((144, 200), 96, 32, 8, 16, 8)}


def blur_input(i):
    (h, w), _, rect = BLUR_CASES[i]
    if rect is None:
        return pattern(h, w, 1, 40 + i)[..., 0]
    m = np.zeros((h, w), np.uint8)
    m[rect[1]:rect[3], rect[0]:rect[2]] = 255
    return m


def composite_inputs():
    cv, tl, mk = pattern(53, 37, 3, 50), pattern(53, 37, 3, 51), pattern(53, 37, 1, 52)[..., 0].copy()
    mk[3], mk[7] = 0, 255
    big = pattern(90, 70, 3, 53)
    bm = np.zeros((90, 70), np.uint8)
    bm[20:73, 11:48] = mk
    return cv, tl, mk, big, bm, (11, 20)
