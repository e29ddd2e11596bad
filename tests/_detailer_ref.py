"""Inputs shared by tests/tools/capture_detailer.py (which runs the reference on them) and the Detailer tests (which run the package on them): the
stand-in and tiny-network jobs of tests/golden/detailer.npz, and the argument lists of the small host functions.  Nothing here computes a result."""
import numpy as np

import _usdu_ref as U

# ---- stand-in runs: VAEEncode.encode -> the pixels, the sampler -> the latent, vae.decode -> the byte table 255 - v --------------------------------
STANDIN_IMAGE = (120, 136, 5)                        # _usdu_ref.smooth_image(h, w, seed)
STANDIN = dict(guide_size=64, max_size=96, feather=5, seed=5, cycle=1, steps=4, cfg=6.5, sampler_name="dpmpp_2m_cfgpp", scheduler="karras", denoise=0.5)
# name -> [(bbox, crop_factor, mask is all zero)]
STANDIN_CASES = {
    "one": [([20, 30, 60, 70], 2.0, False)],
    "disjoint": [([20, 30, 60, 70], 2.0, False), ([90, 70, 120, 110], 1.4, False), ([100, 5, 130, 30], 1.5, False)],
    "overlap": [([20, 30, 60, 70], 2.0, False), ([50, 40, 100, 90], 1.5, False), ([100, 5, 130, 30], 2.0, False)],
    "empty": [([20, 30, 60, 70], 2.0, False), ([90, 70, 120, 110], 1.4, True), ([100, 5, 130, 30], 1.5, False)],
}

# ---- tiny-network run: the tiny UNet and the ch = 64 VAE of the img2img golden (tests/tools/capture_usdu.py) ---------------------------------------
TINY_IMAGE = (168, 100, 5)
TINY = dict(guide_size=128, max_size=160, seed=3, steps=4, cfg=6.5, sampler_name="dpmpp_2m_cfgpp", scheduler="karras", denoise=0.5, feather=5, cycle=1)
# two overlapping segments and one apart; crops 52 x 64, 52 x 64 and 60 x 36 (w x h), sampled at 128 x 157, 128 x 157 and 160 x 96: latents 16 x 19,
# 16 x 19 and 20 x 12, every h * w a multiple of 8 (ldx_vae_encode's rule), and 157 is not a multiple of 8
TINY_BOXES = [([10, 20, 36, 52], 2.0, False), ([30, 40, 56, 72], 2.0, False), ([40, 120, 80, 144], 1.5, False)]
TINY_PERTURBED = ("seed+1", "denoise 0.4", "feather 2", "overlapping segments swapped", "guide_size 96")


def tiny_variant(name):
    """(keyword overrides, boxes) of a perturbed run"""
    if name == "seed+1":
        return dict(seed=TINY["seed"] + 1), TINY_BOXES
    if name == "denoise 0.4":
        return dict(denoise=0.4), TINY_BOXES
    if name == "feather 2":
        return dict(feather=2), TINY_BOXES
    if name == "overlapping segments swapped":
        return {}, [TINY_BOXES[1], TINY_BOXES[0], TINY_BOXES[2]]
    if name == "guide_size 96":
        return dict(guide_size=96), TINY_BOXES
    raise KeyError(name)


def make_segs(h, w, boxes, make_crop_region, SEG):
    """segs for an h x w image: per (bbox, crop_factor, empty) the crop region of `make_crop_region` and a mask that is 1 on the bbox inside it."""
    items = []
    for bbox, factor, empty in boxes:
        x1, y1, x2, y2 = make_crop_region(w, h, bbox, factor)
        mask = np.zeros((y2 - y1, x2 - x1), np.float32)
        if not empty:
            mask[max(bbox[1] - y1, 0):bbox[3] - y1, max(bbox[0] - x1, 0):bbox[2] - x1] = 1.0
        items.append(SEG(None, mask, 1.0, [x1, y1, x2, y2], list(bbox), "seg", None))
    return (h, w), items


def union_mask(h, w, segs):
    """bool [h][w]: the union of the crop regions, where the tiny-network distances are taken"""
    m = np.zeros((h, w), bool)
    for s in segs[1]:
        x1, y1, x2, y2 = s.crop_region
        m[y1:y2, x1:x2] = True
    return m


def image(spec):
    h, w, seed = spec
    return U.to_float(U.smooth_image(h, w, seed))[None]


def standin_decode_table():
    """float32 [256]: entry v -> (255 - v) / 255.0f"""
    return (255 - np.arange(256, dtype=np.int64)).astype(np.float32) / np.float32(255.0)


# ---- arguments of the small host functions; the capture stores what the reference's own functions return for them ------------------------------------
# (w, h, bbox, crop_factor): interior, each border, a corner, a bbox wider than the image after growing, a fractional factor
CROP_CASES = [(136, 120, [20, 30, 60, 70], 2.0), (136, 120, [0, 40, 30, 80], 1.5), (136, 120, [100, 5, 130, 30], 1.5), (136, 120, [110, 40, 136, 70], 2.0),
              (136, 120, [50, 100, 90, 120], 1.7), (136, 120, [0, 0, 20, 20], 3.0), (136, 120, [10, 10, 120, 60], 2.0), (100, 168, [31, 47, 58, 90], 1.3),
              (1024, 1024, [400, 380, 611, 733], 3.0)]
# (w, h, guide_size, max_size): plain, the max_size branch, upscale <= 1 (crop larger than the guide), exactly 1, a size that truncates, a zero size
SIZE_CASES = [(80, 80, 64, 96), (42, 56, 64, 96), (45, 37, 64, 96), (40, 100, 64, 96), (200, 150, 128, 768), (64, 64, 64, 96), (333, 517, 512, 768),
              (211, 353, 512, 768), (1, 300, 2, 96), (52, 64, 128, 160)]
# (scheduler, steps, denoise)
SIGMA_CASES = [("karras", 4, 0.5), ("karras", 20, 0.5), ("normal", 8, 0.3), ("simple", 10, 0.45), ("karras", 20, 1.0), ("karras", 7, 0.4)]


def and_mask_case():
    """(segs, mask) for segs_bitwise_and_mask: fractional cropped masks against a fractional full-size mask"""
    rng = np.random.default_rng(9)
    h, w = 60, 70
    items = []
    for region in ([5, 8, 40, 50], [30, 0, 70, 33]):
        x1, y1, x2, y2 = region
        m = rng.random((y2 - y1, x2 - x1)).astype(np.float32)
        m[rng.random(m.shape) < 0.3] = 0.0
        m[rng.random(m.shape) < 0.3] = 1.0
        items.append((m, region))
    full = rng.random((h, w)).astype(np.float32)
    full[:, :20] = 1.0
    full[40:] = 0.0
    return (h, w), items, full
