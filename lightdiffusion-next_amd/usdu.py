"""Ultimate SD Upscale, the reference's img2img mode (src/UltimateSDUpscale/UltimateSDUpscale.py, called from src/user/pipeline.py:135-214), with the
canvas on the device from the first ESRGAN tile to the returned tensor.

The networks are the engines this package already has (ESRGANEngine.upscale, VAEEngine.encode / decode, sampling.KSampler).  What the reference does
between them in 8-bit PIL on the CPU (LANCZOS resize, GaussianBlur of the tile mask, RGBA paste + alpha_composite) runs in the ldx_image_* kernels
(include/ldx.h), which reproduce Pillow's integer arithmetic, so this module only plans: which tiles, which crops, which coefficient tables.  The plan
(tile_plan) needs no GPU.
"""
import ctypes as C
import functools
import math
from collections import namedtuple

import numpy as np
import torch

from . import lib
from .sampling import KSampler

LANCZOS, BICUBIC, BILINEAR = "lanczos", "bicubic", "bilinear"
_PRECISION_BITS = 22


def _lanczos(x):
    if -3.0 <= x < 3.0:
        if x == 0.0:
            return 1.0
        a, b = x * math.pi, x / 3.0 * math.pi
        return math.sin(a) / a * (math.sin(b) / b)
    return 0.0


def _bicubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


_FILTERS = {LANCZOS: (_lanczos, 3.0), BICUBIC: (_bicubic, 2.0), BILINEAR: (_bilinear, 1.0)}


@functools.lru_cache(maxsize=64)
def resample_coeffs(in_size: int, out_size: int, filter: str = LANCZOS):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc (Resample.c) for one axis, in double precision and in Pillow's order of operations.
    Returns (bounds int32 [out_size][2] = first source index and tap count, kk int32 [out_size][ksize] in 2^-22 units); cached, treat as read-only."""
    fn, support = _FILTERS[filter]
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = support * fs
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / fs
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        k = [fn((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for w in k:
            ww += w
        if ww != 0.0:
            k = [w / ww for w in k]
        bounds[xx] = (xmin, xmax)
        kk[xx, :xmax] = [int(w * (1 << _PRECISION_BITS) - 0.5) if w < 0 else int(w * (1 << _PRECISION_BITS) + 0.5) for w in k]
    return bounds, kk


def gaussian_box_params(radius: float):
    """Pillow's GaussianBlur(radius) as box blurs (BoxBlur.c): the box radius of each of the three passes per axis, float32 arithmetic.
    Returns (fr, R, ww, fw): ldx_image_box_blur_pass takes fr; R, ww, fw are what it derives (returned for the tests)."""
    f = np.float32
    r = f(radius)
    s2 = r * r / f(3)
    big_l = f(math.sqrt(12.0 * float(s2) + 1.0))
    el = f(math.floor((float(big_l) - 1.0) / 2.0))
    a = (f(2) * el + f(1)) * (el * (el + f(1)) - f(3) * s2)
    a = a / (f(6) * (s2 - (el + f(1)) * (el + f(1))))
    fr = f(el + a)
    R = int(fr)
    ww = int(f(16777216.0) / (fr * f(2) + f(1)))
    fw = ((1 << 24) - (2 * R + 1) * ww) // 2
    return float(fr), R, ww, fw


def blur_window(box, R: int, width: int, height: int):
    """The part of the canvas a blurred mask can be non-zero in: its non-zero box grown by 3 (R + 2) and clipped.  Three passes per axis carry a value
    R + 1 pixels each, so the window's border is zero in every pass unless it is the canvas's own border: blurring the window alone (edge replication
    at its border) gives the bytes of the whole-canvas blur."""
    g = 3 * (R + 2)
    return max(box[0] - g, 0), max(box[1] - g, 0), min(box[2] + g, width), min(box[3] + g, height)


# ---- tile plan -------------------------------------------------------------------------------------------------------------------
# mask: ("rect", x0, y0, x1, y1) = 255 on [x0, x1) x [y0, y1), or ("row" | "col", x0, y0, x1, y1) = the seam gradient pattern pasted at (x0, y0) and cut
# at (x1, y1).  box: the non-zero bounding box of the mask.  crop: the canvas rectangle that is redrawn.  sample: (width, height) the networks run at.
Tile = namedtuple("Tile", "stage mask box crop sample blur")


def _resample_host(img, out_w, out_h, filter):
    """The resample rule of ldx_image_resample_pass on a host uint8 [H][W] array: only for the 256-step ramp the seam patterns are made of."""
    def one(a, n):
        b, kk = resample_coeffs(a.shape[1], n, filter)
        out = np.empty((a.shape[0], n), np.uint8)
        for i in range(n):
            acc = (1 << 21) + a[:, b[i, 0]:b[i, 0] + b[i, 1]].astype(np.int64) @ kk[i, :b[i, 1]].astype(np.int64)
            out[:, i] = np.clip(acc >> _PRECISION_BITS, 0, 255)
        return out
    a = one(img, out_w) if out_w != img.shape[1] else img
    return one(a.T, out_h).T if out_h != img.shape[0] else a


@functools.lru_cache(maxsize=8)
def seam_patterns(tile_w: int, tile_h: int):
    """half_tile_process's row_gradient / col_gradient (UltimateSDUpscale.py:575-601): Image.linear_gradient (value = row index) and its rotations,
    BICUBIC-resized to half a tile and pasted into a black tile.  uint8 [tile_h][tile_w] each; cached (tens of ms of host loops), treat as read-only."""
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 256, 1)
    row = np.zeros((tile_h, tile_w), np.uint8)
    col = np.zeros((tile_h, tile_w), np.uint8)
    hh, hw = tile_h // 2, tile_w // 2
    if hh > 0:
        row[:hh] = _resample_host(ramp, tile_w, hh, BICUBIC)
        row[hh:2 * hh] = _resample_host(np.ascontiguousarray(ramp[::-1, ::-1]), tile_w, hh, BICUBIC)
    if hw > 0:
        col[:, :hw] = _resample_host(np.ascontiguousarray(ramp.T), hw, tile_h, BICUBIC)
        col[:, hw:2 * hw] = _resample_host(np.ascontiguousarray(ramp.T[::-1, ::-1]), hw, tile_h, BICUBIC)
    return row, col


def _crop_region(box, pad, width, height, p_w, p_h):
    """get_crop_region + fix_crop_region (image_util.py:206-245), then process_images' aspect fit and expand_crop (UltimateSDUpscale.py:143-162,
    image_util.py:248-285)."""
    x1, y1, x2, y2 = box
    x1, y1, x2, y2 = max(x1 - pad, 0), max(y1 - pad, 0), min(x2 + pad, width), min(y2 + pad, height)
    if x2 < width:                 # fix_crop_region: one pixel off, except at the far border
        x2 -= 1
    if y2 < height:
        y2 -= 1
    cw, ch = x2 - x1, y2 - y1
    ratio = p_w / p_h
    if cw / ch > ratio:
        tw, th = cw, round(cw / ratio)
    else:
        tw, th = round(ch * ratio), ch
    x2 = min(x2 + (tw - cw) // 2, width)
    x1 = max(x1 - (tw - (x2 - x1)), 0)
    x2 = min(x2 + (tw - (x2 - x1)), width)
    y2 = min(y2 + (th - ch) // 2, height)
    y1 = max(y1 - (th - (y2 - y1)), 0)
    y2 = min(y2 + (th - (y2 - y1)), height)
    return x1, y1, x2, y2


def _nonzero_box(a):
    ys, xs = np.nonzero(a)
    if len(ys) == 0:
        return None
    return int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1


def tile_plan(width, height, tile_w, tile_h, mask_blur, padding, redraw=True, seam_fix=True, seam_blur=0, seam_padding=0):
    """The tiles of USDURedraw.linear_process (:493-526) and USDUSeamsFix.half_tile_process (:557-653) for a width x height canvas, in the
    reference's order.  No GPU needed."""
    rows, cols = math.ceil(height / tile_h), math.ceil(width / tile_w)
    plan = []
    if redraw:
        sample = (math.ceil((tile_w + padding) / 8) * 8, math.ceil((tile_h + padding) / 8) * 8)
        for yi in range(rows):
            for xi in range(cols):
                # ImageDraw.rectangle includes its second corner
                box = (xi * tile_w, yi * tile_h, min(xi * tile_w + tile_w + 1, width), min(yi * tile_h + tile_h + 1, height))
                plan.append(Tile("redraw", ("rect",) + box, box, _crop_region(box, padding, width, height, *sample), sample, mask_blur))
    if seam_fix:
        row, col = seam_patterns(tile_w, tile_h)
        sample = (tile_w, tile_h)
        jobs = [("row", row, xi * tile_w, yi * tile_h + tile_h // 2) for yi in range(rows - 1) for xi in range(cols)]
        jobs += [("col", col, xi * tile_w + tile_w // 2, yi * tile_h) for yi in range(rows) for xi in range(cols - 1)]
        for kind, pat, px, py in jobs:
            x1, y1 = min(px + tile_w, width), min(py + tile_h, height)
            nz = _nonzero_box(pat[:y1 - py, :x1 - px])
            if nz is None:
                raise ValueError(f"seam tile at ({px}, {py}) has an empty mask")
            box = (px + nz[0], py + nz[1], px + nz[2], py + nz[3])
            plan.append(Tile("seam", (kind, px, py, x1, y1), box, _crop_region(box, seam_padding, width, height, *sample), sample, seam_blur))
    return plan


# ---- device images ---------------------------------------------------------------------------------------------------------------
class _Image:
    """A uint8 HWC image on the device with a 16-byte aligned row pitch."""

    def __init__(self, h, w, c, device, zero=False):
        self.h, self.w, self.c = h, w, c
        self.pitch = (w * c + 15) // 16 * 16
        self.buf = (torch.zeros if zero else torch.empty)((h, self.pitch), dtype=torch.uint8, device=device)

    def ptr(self, x=0, y=0):
        return C.c_void_p(self.buf.data_ptr() + y * self.pitch + x * self.c)

    def view(self):
        return self.buf[:, :self.w * self.c].unflatten(1, (self.w, self.c))


class ImageOps:
    """Thin wrappers of the 8-bit image C ABI (ldx_image_*) on _Image: what UltimateSDUpscale and detailer.Detailer share."""

    def _init_ops(self, device):
        self.device = torch.device(device)
        self._lib = lib.load()
        self._tables = {}

    def _st(self):
        return lib.current_stream_ptr()

    def _quantize(self, t):
        """fp32 [1][H][W][3] -> _Image"""
        t = t.to(self.device, torch.float32).contiguous()
        _, h, w, c = t.shape
        out = _Image(h, w, c, self.device)
        lib.check(self._lib.ldx_image_quantize(lib.ptr(t), h, w, c, out.ptr(), out.pitch, self._st()), "ldx_image_quantize")
        return out

    def _to_float(self, img, rect=None):
        x0, y0, x1, y1 = rect or (0, 0, img.w, img.h)
        out = torch.empty((1, y1 - y0, x1 - x0, img.c), dtype=torch.float32, device=self.device)
        lib.check(self._lib.ldx_image_to_float(img.ptr(), img.pitch, img.h, img.w, img.c, x0, y0, x1 - x0, y1 - y0, lib.ptr(out), self._st()),
                  "ldx_image_to_float")
        return out

    def _table(self, n_in, n_out, filter):
        key = (n_in, n_out, filter)
        if key not in self._tables:
            b, kk = resample_coeffs(n_in, n_out, filter)
            self._tables[key] = (torch.from_numpy(b).to(self.device), torch.from_numpy(kk).to(self.device), kk.shape[1])
        return self._tables[key]

    def _resize(self, img, rect, out_w, out_h, filter=LANCZOS):
        """Image.resize of the rectangle `rect` of img (None: all of it): the pass along x, then the pass along y; a pass that keeps its size is skipped
        (the caller skips a resize that keeps both)."""
        x0, y0, x1, y1 = rect or (0, 0, img.w, img.h)
        w, h = x1 - x0, y1 - y0
        src, pitch = img.ptr(x0, y0), img.pitch
        if out_w != w:
            b, kk, ks = self._table(w, out_w, filter)
            mid = _Image(h, out_w, img.c, self.device)
            lib.check(self._lib.ldx_image_resample_pass(src, pitch, h, w, img.c, 1, out_w, lib.ptr(b), lib.ptr(kk), ks, mid.ptr(), mid.pitch, self._st()),
                      "ldx_image_resample_pass")
            src, pitch, w, keep = mid.ptr(), mid.pitch, out_w, mid
        if out_h != h:
            b, kk, ks = self._table(h, out_h, filter)
            out = _Image(out_h, w, img.c, self.device)
            lib.check(self._lib.ldx_image_resample_pass(src, pitch, h, w, img.c, 0, out_h, lib.ptr(b), lib.ptr(kk), ks, out.ptr(), out.pitch, self._st()),
                      "ldx_image_resample_pass")
            return out
        return keep

    def _fill(self, img, rect, value):
        x0, y0, x1, y1 = rect
        lib.check(self._lib.ldx_image_fill_rect(img.ptr(), img.pitch, img.h, img.w, img.c, x0, y0, x1 - x0, y1 - y0, value, self._st()), "ldx_image_fill_rect")


class UltimateSDUpscale(ImageOps):
    """UltimateSDUpscale.upscale (UltimateSDUpscale.py:904-1019) on the engines: `unet_engine` (UNetEngine), `vae_engine` (VAEEngine with encoder
    weights), `esrgan_engine` (ESRGANEngine).

    Per tile, in the reference's order: crop -> to float, LANCZOS to the sample size when the crop differs, vae.encode, KSampler.sample, vae.decode,
    quantise, LANCZOS back, composite through the blurred tile mask.  Every tile samples with the same `seed`; prepare_noise reseeds the global CPU
    RNG and vae.encode draws from it, so the order of the calls is part of the result and is kept.

    Quirks of the reference that are reproduced:
      * the upscale model runs once per entry of USDUpscaler.get_factors (:326-337), which is one entry for every factor in (1, 4], and its x4 result
        is quantised and LANCZOS-resized to (ceil(w * by / 8) * 8, ceil(h * by / 8) * 8); a factor <= 1 skips the model, one above 4 whose list
        would hold a zero raises here (the reference divides by zero);
      * any mode_type other than "None" runs the linear redraw ("Chess" too); any seam_fix_mode other than "None" runs the half-tile pass;
      * seam_fix_denoise and seam_fix_width are read and never used: the seam pass samples with `denoise`;
      * crop_cond is the identity: every tile gets the full conditioning; force_uniform_tiles is unused.
    A batch of more than one image raises: the reference's batched tiles are not built."""

    MODES = ("Linear", "Chess", "None")
    SEAM_FIX_MODES = ("None", "Band Pass", "Half Tile", "Half Tile + Intersections")

    def __init__(self, unet_engine, vae_engine, esrgan_engine, device=None):
        self.unet, self.vae, self.esrgan = unet_engine, vae_engine, esrgan_engine
        self._init_ops(device if device is not None else next(e.device for e in (unet_engine, vae_engine, esrgan_engine) if e is not None))
        self.timings = None            # a dict of lists when a probe wants per-stage times (profiles/usdu_probe.py)

    # the three network calls of a tile; tests replace them to pin everything else byte for byte
    def _encode(self, pixels):
        return self.vae.encode(pixels)

    def _sample(self, latent, seed, steps, cfg, sampler_name, scheduler, positive, negative, denoise):
        return KSampler(self.unet).sample(seed, steps, cfg, sampler_name, scheduler, positive, negative, latent, denoise=denoise)

    def _decode(self, latent):
        return self.vae.decode(latent)

    def _blur(self, mask, out, tmp, box, radius):
        """GaussianBlur(radius) of `mask` into `out` (both canvas-sized, `out` zero outside earlier windows), inside blur_window(box) only.
        Returns the window, which the caller zeroes again after use."""
        fr, R, _, _ = gaussian_box_params(radius)
        win = blur_window(box, R, mask.w, mask.h)
        x0, y0, x1, y1 = win
        w, h = x1 - x0, y1 - y0
        a, b = tmp
        chain = [(mask.ptr(x0, y0), mask.pitch), (a.ptr(), a.pitch), (b.ptr(), b.pitch), (a.ptr(), a.pitch), (b.ptr(), b.pitch), (a.ptr(), a.pitch),
                 (out.ptr(x0, y0), out.pitch)]
        for i in range(6):
            (src, sp), (dst, dp) = chain[i], chain[i + 1]
            lib.check(self._lib.ldx_image_box_blur_pass(src, sp, h, w, 1 if i < 3 else 0, fr, dst, dp, self._st()), "ldx_image_box_blur_pass")
        return win

    def _mark(self, name):
        if self.timings is not None:
            torch.cuda.synchronize(self.device)
            import time
            now = time.perf_counter()
            self.timings.setdefault(name, []).append((now - self._t0) * 1e3)
            self._t0 = now

    # ---- the job --------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _model_passes(scale_factor):
        """USDUpscaler.get_factor / get_factors (:306-337): how many times the upscale model runs."""
        def factor(n):
            return 2 if n == 1 else 4 if n % 4 == 0 else 3 if n % 3 == 0 else 2 if n % 2 == 0 else 0
        n, cur = 0, 1
        while cur < scale_factor:
            f = factor(scale_factor // cur)
            if f == 0:
                raise ValueError(f"upscale factor {scale_factor}: the reference's factor list holds a zero (it divides by zero there)")
            n, cur = n + 1, cur * f
        return n

    def upscale(self, image, positive, negative, upscale_by, seed, steps, cfg, sampler_name, scheduler, denoise, mode_type, tile_width, tile_height,
                mask_blur, tile_padding, seam_fix_mode, seam_fix_denoise, seam_fix_mask_blur, seam_fix_width, seam_fix_padding, force_uniform_tiles):
        """image [1][H][W][3] fp32 in [0, 1] -> [1][H'][W'][3] fp32 on the device, every value a k / 255."""
        if mode_type not in self.MODES or seam_fix_mode not in self.SEAM_FIX_MODES:
            raise KeyError((mode_type, seam_fix_mode))
        if image.dim() != 4 or image.shape[0] != 1 or image.shape[-1] != 3:
            raise NotImplementedError("UltimateSDUpscale.upscale takes one [1][H][W][3] image: batched tiles are not built")
        import time
        self._t0 = time.perf_counter()
        _, h0, w0, _ = image.shape
        width, height = math.ceil(w0 * upscale_by / 8) * 8, math.ceil(h0 * upscale_by / 8) * 8
        tile_w = tile_width if tile_width > 0 else tile_height
        tile_h = tile_height if tile_height > 0 else tile_width

        # Upscaler._upscale (USDU_upscaler.py:146-160) per model pass: bytes -> float -> model -> clamp -> bytes; then the LANCZOS resize (:356-358)
        canvas = self._quantize(image)
        for _ in range(self._model_passes(math.ceil(max(width, height) / max(w0, h0)))):
            canvas = self._quantize(self.esrgan.upscale(self._to_float(canvas)))
        self._mark("esrgan")
        if (canvas.w, canvas.h) != (width, height):
            canvas = self._resize(canvas, None, width, height)
        self._mark("resize")

        plan = tile_plan(width, height, tile_w, tile_h, mask_blur, tile_padding, redraw=mode_type != "None", seam_fix=seam_fix_mode != "None",
                         seam_blur=seam_fix_mask_blur, seam_padding=seam_fix_padding)
        mask = _Image(height, width, 1, self.device, zero=True)
        blurred = _Image(height, width, 1, self.device, zero=True)
        tmp = (_Image(height, width, 1, self.device), _Image(height, width, 1, self.device))
        patterns = None
        for t in plan:
            kind, x0, y0, x1, y1 = t.mask
            self.stage = t.stage
            if kind == "rect":
                self._fill(mask, (x0, y0, x1, y1), 255)
            else:
                if patterns is None:
                    patterns = {k: torch.from_numpy(p).to(self.device) for k, p in zip(("row", "col"), seam_patterns(tile_w, tile_h))}
                mask.view()[y0:y1, x0:x1, 0] = patterns[kind][:y1 - y0, :x1 - x0]
            alpha, win = mask, None
            if t.blur > 0:
                win = self._blur(mask, blurred, tmp, t.box, t.blur)
                alpha = blurred
            self._mark("mask")
            cx0, cy0, cx1, cy1 = t.crop
            cw, ch = cx1 - cx0, cy1 - cy0
            if (cw, ch) != t.sample:
                pixels = self._to_float(self._resize(canvas, t.crop, *t.sample))
            else:
                pixels = self._to_float(canvas, t.crop)
            latent = self._encode(pixels)
            self._mark("crop_encode")
            latent = self._sample(latent, seed, steps, cfg, sampler_name, scheduler, positive, negative, denoise)
            self._mark("sample")
            decoded = self._decode(latent)
            self._mark("decode")
            tile = self._quantize(decoded)
            if (tile.w, tile.h) != (cw, ch):
                tile = self._resize(tile, None, cw, ch)
            lib.check(self._lib.ldx_image_composite(canvas.ptr(), canvas.pitch, height, width, 3, cx0, cy0, cw, ch, tile.ptr(), tile.pitch,
                                                    alpha.ptr(), alpha.pitch, self._st()), "ldx_image_composite")
            self._fill(mask, (x0, y0, x1, y1), 0)
            if win is not None:
                self._fill(blurred, win, 0)
            self._mark("composite")
        return self._to_float(canvas)
