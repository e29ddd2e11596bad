"""ADetailer's per-segment redraw, the reference's --adetailer exit (DetailerForEachTest.doit / DetailerForEach.do_detail,
src/AutoDetailer/ADetailer.py:643-871, called twice from src/user/pipeline.py:375-511: body pass, then face pass), with the canvas on the device.

The job starts where doit starts: with `segs` supplied.  The detectors in front of it (YOLO, SAM, cv2.dilate) are third-party packages and stay with the
caller; make_crop_region and segs_bitwise_and_mask are here so that a caller with a detector of its own can build `segs`.

Per segment the reference crops the CURRENT fp32 canvas, rounds the crop to 8 bit, LANCZOS-resizes it, encodes, samples, decodes, rounds and resizes back,
and blends the result into the canvas through the segment's Gaussian-feathered mask.  The 8-bit steps are the ldx_image_* kernels usdu.py already drives;
the three fp32 steps (crop-and-quantise, mask blur, masked paste) are the ldx_detail_* kernels (include/ldx.h, csrc/detail.hip -> libldx_detail.so).
blur_mask_host / paste_host / detailer_host state the same rules in numpy, float for float; no GPU is needed for them.
"""
import math
from collections import namedtuple

import numpy as np
import torch

from . import lib
from .sampling import KSampler
from .usdu import LANCZOS, ImageOps, _Image, resample_coeffs

# SEGS.SEG (src/AutoDetailer/SEGS.py:6-18).  cropped_mask: host float32 [ch][cw]; crop_region = [x1, y1, x2, y2]; cropped_image is never read here
# (the reference crops the current canvas instead, "to handle overlapping area").
SEG = namedtuple("SEG", ["cropped_image", "cropped_mask", "confidence", "crop_region", "bbox", "label", "control_net_wrapper"], defaults=[None])

MAX_FEATHER = 31                 # ldx_detail_blur_mask takes k = 2 * feather + 1 <= 63


# ---- host helpers ------------------------------------------------------------------------------------------------------------------
def _normalize_region(limit, startp, size):
    """AD_util.normalize_region (:115-136); `size` may be a float, int() truncates the end."""
    if startp < 0:
        new_endp, new_startp = min(limit, size), 0
    elif startp + size > limit:
        new_startp, new_endp = max(0, limit - size), limit
    else:
        new_startp, new_endp = startp, min(limit, startp + size)
    return int(new_startp), int(new_endp)


def make_crop_region(w, h, bbox, crop_factor):
    """AD_util.make_crop_region (:139-172): the bbox grown by crop_factor about its centre and moved into the w x h image.  [x1, y1, x2, y2]."""
    x1, y1, x2, y2 = bbox
    bbox_w, bbox_h = x2 - x1, y2 - y1
    crop_w, crop_h = bbox_w * crop_factor, bbox_h * crop_factor
    kernel_x, kernel_y = x1 + bbox_w / 2, y1 + bbox_h / 2
    new_x1, new_y1 = int(kernel_x - crop_w / 2), int(kernel_y - crop_h / 2)
    new_x1, new_x2 = _normalize_region(w, new_x1, crop_w)
    new_y1, new_y2 = _normalize_region(h, new_y1, crop_h)
    return [new_x1, new_y1, new_x2, new_y2]


def segs_bitwise_and_mask(segs, mask):
    """SEGS.segs_bitwise_and_mask (:21-58) on the host, where the masks live: every cropped_mask AND the crop of `mask` ([H][W], or with leading axes of
    length 1), both taken as bytes (value * 255, truncated)."""
    mask = np.asarray(mask.cpu() if torch.is_tensor(mask) else mask, np.float32)
    while mask.ndim > 2:
        if mask.shape[0] != 1:
            raise ValueError(f"segs_bitwise_and_mask takes one 2-D mask, got {mask.shape}")
        mask = mask[0]
    mask = (mask * 255).astype(np.uint8)
    items = []
    for seg in segs[1]:
        x1, y1, x2, y2 = seg.crop_region
        new_mask = np.bitwise_and((seg.cropped_mask * 255).astype(np.uint8), mask[y1:y2, x1:x2])
        items.append(SEG(seg.cropped_image, new_mask.astype(np.float32) / 255.0, seg.confidence, seg.crop_region, seg.bbox, seg.label, None))
    return segs[0], items


def detail_size(w, h, guide_size, max_size):
    """enhance_detail's sample size (:530-551) for a w x h crop -> (new_w, new_h)."""
    upscale = guide_size / min(w, h)
    new_w, new_h = int(w * upscale), int(h * upscale)
    if new_w > max_size or new_h > max_size:
        upscale *= max_size / max(new_w, new_h)
        new_w, new_h = int(w * upscale), int(h * upscale)
    if upscale <= 1.0 or new_w == 0 or new_h == 0:
        return w, h
    return new_w, new_h


def detail_sigmas(model_sampling, scheduler, steps, denoise):
    """ksampler_wrapper / separated_sample (:304-448): the last steps + 1 sigmas of the floor(steps / denoise)-step schedule.  This is what
    KSampler.sample selects for the same (steps, denoise), so Detailer._sample hands both on unchanged."""
    from .sampling import calculate_sigmas
    if not 0.0 < denoise <= 1.0:
        raise ValueError(f"denoise {denoise}: the reference's start step floor(steps / denoise) - steps is negative or undefined")
    advanced = math.floor(steps / denoise)
    return calculate_sigmas(model_sampling, scheduler, advanced)[advanced - steps:]


def blur_table(feather, sigma=10.0):
    """The k x k kernel of torchvision's GaussianBlur(kernel_size=k, sigma) for k = 2 * feather + 1 (tensor_gaussian_blur_mask, tensor_util.py:218-254),
    by torchvision's published expression in fp32 torch: float32 [k][k]."""
    k = 2 * int(feather) + 1
    half = (k - 1) * 0.5
    x = torch.linspace(-half, half, steps=k)
    pdf = torch.exp(-0.5 * (x / sigma).pow(2))
    k1 = pdf / pdf.sum()
    return torch.mm(k1[:, None], k1[None, :]).numpy()


# ---- the device rules in numpy -----------------------------------------------------------------------------------------------------
def blur_mask_host(mask, table):
    """ldx_detail_blur_mask in numpy: float32 [h][w] -> float32 [h][w]; taps in row-major order, each one rounded product and one rounded add."""
    mask, table = np.ascontiguousarray(mask, np.float32), np.asarray(table, np.float32)
    h, w = mask.shape
    k = table.shape[0]
    r = k // 2
    if table.shape != (k, k) or k % 2 == 0 or r >= h or r >= w:
        raise ValueError(f"blur_mask_host: a {table.shape} table on a {mask.shape} mask (k odd, reflect padding k // 2 below both sizes)")
    padded = np.pad(mask, r, mode="reflect") if r else mask
    acc = np.zeros((h, w), np.float32)
    for dy in range(k):
        for dx in range(k):
            acc = acc + table[dy, dx] * padded[dy:dy + h, dx:dx + w]
    return acc


def paste_host(canvas, src, mask, x0, y0):
    """ldx_detail_paste in numpy, in place: canvas float32 [H][W][3], src [h][w][3], mask [h][w]; clipped at the right and bottom border."""
    H, W, _ = canvas.shape
    h, w = min(H, y0 + src.shape[0]) - y0, min(W, x0 + src.shape[1]) - x0
    m = np.asarray(mask, np.float32)[:h, :w, None]
    d = canvas[y0:y0 + h, x0:x0 + w]
    t0 = np.float32(1.0) - m
    t1 = t0 * d
    t2 = m * np.asarray(src, np.float32)[:h, :w]
    canvas[y0:y0 + h, x0:x0 + w] = t1 + t2
    return canvas


def quantize_host(x):
    """ldx_image_quantize / ldx_detail_crop_quantize in numpy"""
    return (np.clip(np.asarray(x, np.float32), np.float32(0), np.float32(1)) * np.float32(255.0)).astype(np.uint8)


def resize_host(img, out_w, out_h, filter=LANCZOS):
    """ldx_image_resample_pass along x, then along y, on a host uint8 [H][W][C] array; a pass that keeps its size is skipped."""
    def one(a, n):                                          # along axis 0
        b, kk = resample_coeffs(a.shape[0], n, filter)
        out = np.empty((n,) + a.shape[1:], np.uint8)
        for i in range(n):
            acc = (1 << 21) + np.tensordot(kk[i, :b[i, 1]].astype(np.int64), a[b[i, 0]:b[i, 0] + b[i, 1]].astype(np.int64), 1)
            out[i] = np.clip(acc >> 22, 0, 255)
        return out
    img = np.asarray(img, np.uint8)
    if out_w != img.shape[1]:
        img = np.swapaxes(one(np.swapaxes(img, 0, 1), out_w), 0, 1)
    if out_h != img.shape[0]:
        img = one(img, out_h)
    return np.ascontiguousarray(img)


def _check_job(image_shape, segs):
    if len(image_shape) != 4 or image_shape[0] != 1 or image_shape[-1] != 3:
        raise NotImplementedError("Detailer.detail takes one [1][H][W][3] image: the reference's per-image loop over a batch is not built")
    _, H, W, _ = image_shape
    sh, sw = segs[0]
    if (sh, sw) != (H, W) and sh != 0 and sw != 0:
        raise NotImplementedError(f"segs were made for a {sh} x {sw} image, the image is {H} x {W}: segs_scale_match's rescaling is not built")
    return H, W


def _crop_rect(seg, W, H):
    """the rectangle numpy's slicing image[:, y1:y2, x1:x2] takes, and the check that the mask covers it"""
    x1, y1, x2, y2 = (int(v) for v in seg.crop_region)
    x2, y2 = min(x2, W), min(y2, H)
    if not (0 <= x1 < x2 and 0 <= y1 < y2):
        raise ValueError(f"crop region {list(seg.crop_region)} is empty or outside the {W} x {H} image")
    if tuple(np.shape(seg.cropped_mask)) != (y2 - y1, x2 - x1):
        raise ValueError(f"cropped_mask {np.shape(seg.cropped_mask)} does not have its crop region's size {(y2 - y1, x2 - x1)}")
    return x1, y1, x2, y2


def detailer_host(image, segs, guide_size, max_size, seed, steps, cfg, sampler_name, scheduler, positive, negative, denoise, feather, cycle=1,
                  *, encode, sample, decode):
    """Detailer.detail on the host with the three network calls passed in: image float32 [1][H][W][3] -> float32 [1][H][W][3] (a new array).
    encode(pixels float32 [1][h][w][3]) -> latent; sample(latent, seed, steps, cfg, sampler_name, scheduler, positive, negative, denoise) -> latent;
    decode(latent) -> float32 [1][h'][w'][3].  What hdr.autohdr_host and png.png_host are to their kernels."""
    image = np.asarray(image, np.float32)
    H, W = _check_job(image.shape, segs)
    canvas = image[0].copy()
    table = blur_table(feather)
    for i, seg in enumerate(segs[1]):
        x1, y1, x2, y2 = _crop_rect(seg, W, H)
        if not np.any(seg.cropped_mask):
            continue
        mask = blur_mask_host(seg.cropped_mask, table)
        w, h = x2 - x1, y2 - y1
        crop = quantize_host(canvas[y1:y2, x1:x2])
        pixels = resize_host(crop, *detail_size(w, h, guide_size, max_size)).astype(np.float32) / np.float32(255.0)
        latent = encode(pixels[None])
        for c in range(cycle):
            latent = sample(latent, seed + i + c, steps, cfg, sampler_name, scheduler, positive, negative, denoise)
        decoded = decode(latent)
        decoded = np.asarray(decoded.cpu() if torch.is_tensor(decoded) else decoded, np.float32)[0]
        enhanced = resize_host(quantize_host(decoded), w, h).astype(np.float32) / np.float32(255.0)
        paste_host(canvas, enhanced, mask, x1, y1)
    return canvas[None]


# ---- the device job ----------------------------------------------------------------------------------------------------------------
class Detailer(ImageOps):
    """DetailerForEachTest.doit (ADetailer.py:887-1066) on the engines: `unet_engine` (UNetEngine), `vae_engine` (VAEEngine with encoder weights).

    Per segment i (the index counts skipped segments too), in the reference's order: crop the current canvas (earlier pastes are seen) -> bytes ->
    LANCZOS to detail_size -> vae.encode -> `cycle` sampler runs with seeds seed + i + c, each on the previous one's latent -> vae.decode -> bytes ->
    LANCZOS back -> fp32 blend through the mask blurred with GaussianBlur(2 * feather + 1, sigma 10).  The crop is rounded to 8 bit even when the
    sample size equals the crop's.  prepare_noise reseeds the global CPU RNG and vae.encode draws from it, so the order of the calls is part of the
    result and is kept.

    Quirks of the reference that are reproduced:
      * noise_mask, noise_mask_feather, force_inpaint, inpaint_model and guide_size_for are accepted and do nothing to the pixels of a 4-channel UNet
        run: the noise mask reaches KSamplerX0Inpaint, which ignores it (src/sample/sampling.py:383-404); its blur result is unused;
        DifferentialDiffusion only sets a function nobody calls.  Nothing is computed for them.
      * an all-zero cropped_mask skips its segment (the reference blurs it first; the blur has no effect, so it is not run) and still uses up an index;
      * every sampler function is called with multiscale off (ksampler2, :166-177, no name whitelist);
      * `wildcard` is handed to a chooser that holds ONE item (bbox.py:180-218), so the reference raises IndexError at the second non-empty segment.
        Its loop is plainly written for many segments and the Impact-Pack code it was taken from cycles its items, so every segment is processed
        here; tests/golden/detailer.META.txt says how the multi-segment goldens were captured.
    Not built (NotImplementedError): a batch of more than one image; segs made for another image size (segs_scale_match's rescaling).
    The crop, enhanced and alpha lists doit also returns are not built: the pipeline uses element 0, the canvas, only."""

    def __init__(self, unet_engine, vae_engine, device=None):
        self.unet, self.vae = unet_engine, vae_engine
        self._init_ops(device if device is not None else next(e.device for e in (unet_engine, vae_engine) if e is not None))
        self._blur_tables = {}
        self.timings = None            # a dict of lists of HIP event pairs when a probe wants per-stage times (profiles/detailer_probe.py)

    # the three network calls of a segment; tests replace them to pin everything else bit for bit
    def _encode(self, pixels):
        return self.vae.encode(pixels)

    def _sample(self, latent, seed, steps, cfg, sampler_name, scheduler, positive, negative, denoise):
        return KSampler(self.unet).sample(seed, steps, cfg, sampler_name, scheduler, positive, negative, latent, denoise=denoise,
                                          enable_multiscale=False, multiscale_every_sampler=True)

    def _decode(self, latent):
        return self.vae.decode(latent)

    def _blur_table(self, feather):
        if feather not in self._blur_tables:
            self._blur_tables[feather] = torch.from_numpy(blur_table(feather)).to(self.device)
        return self._blur_tables[feather]

    def _mark(self, name):
        if self.timings is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self.timings.setdefault(name, []).append(ev)

    def detail(self, image, segs, positive, negative, guide_size, guide_size_for, max_size, seed, steps, cfg, sampler_name, scheduler, denoise, feather,
               noise_mask, force_inpaint, wildcard, cycle=1, inpaint_model=False, noise_mask_feather=0):
        """image [1][H][W][3] fp32 in [0, 1], segs = ((H, W), [SEG, ...]) -> the detailed canvas, a new contiguous fp32 [1][H][W][3] device tensor."""
        H, W = _check_job(tuple(image.shape), segs)
        if not 0 <= feather <= MAX_FEATHER:
            raise ValueError(f"feather {feather}: the blur kernel is 2 * feather + 1 <= {2 * MAX_FEATHER + 1} wide")
        if not 0.0 < denoise <= 1.0:
            raise ValueError(f"denoise {denoise}: see detail_sigmas")
        canvas = image.to(self.device, torch.float32).contiguous()
        if canvas.data_ptr() == image.data_ptr():
            canvas = canvas.clone()
        k, table = 2 * feather + 1, self._blur_table(feather)
        for i, seg in enumerate(segs[1]):
            x1, y1, x2, y2 = _crop_rect(seg, W, H)
            if not np.any(seg.cropped_mask):
                continue
            w, h = x2 - x1, y2 - y1
            self._mark("start")
            raw = torch.from_numpy(np.ascontiguousarray(seg.cropped_mask, np.float32)).to(self.device)
            mask = torch.empty_like(raw)
            lib.check(self._lib.ldx_detail_blur_mask(lib.ptr(raw), h, w, lib.ptr(table), k, lib.ptr(mask), self._st()), "ldx_detail_blur_mask")
            self._mark("mask")
            crop = _Image(h, w, 3, self.device)
            lib.check(self._lib.ldx_detail_crop_quantize(lib.ptr(canvas), H, W, x1, y1, w, h, crop.ptr(), crop.pitch, self._st()),
                      "ldx_detail_crop_quantize")
            new_w, new_h = detail_size(w, h, guide_size, max_size)
            pixels = self._to_float(self._resize(crop, None, new_w, new_h) if (new_w, new_h) != (w, h) else crop)
            latent = self._encode(pixels)
            self._mark("crop_encode")
            for c in range(cycle):
                latent = self._sample(latent, seed + i + c, steps, cfg, sampler_name, scheduler, positive, negative, denoise)
            self._mark("sample")
            decoded = self._decode(latent)
            self._mark("decode")
            tile = self._quantize(decoded)
            enhanced = self._to_float(self._resize(tile, None, w, h) if (tile.w, tile.h) != (w, h) else tile)
            lib.check(self._lib.ldx_detail_paste(lib.ptr(canvas), H, W, x1, y1, lib.ptr(enhanced), lib.ptr(mask), h, w, self._st()), "ldx_detail_paste")
            self._mark("paste")
        return canvas
