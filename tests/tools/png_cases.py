"""The images the PNG encoder's CPU and GPU tests share (tests/test_png_host_cpu.py, tests/test_png_gpu.py): the smallest shapes at which each mechanism
of lightdiffusion-next_amd/png.py can go wrong, with the chunk size of 16 384 bytes of filtered stream (H * (1 + 3 W))."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")


def mixed(h, w, seed):
    """Smooth colour waves with a little noise and one flat rectangle: literals, short and long runs, every filter type worth choosing somewhere."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([127 + 100 * np.sin(xx / 9.7 + c) * np.cos(yy / 6.1 - c) for c in range(3)], -1) + rng.integers(-1, 2, (h, w, 3))
    img = np.clip(img, 0, 255).astype(np.uint8)
    img[h // 3:h // 2, w // 4:w // 2] = (200, 30, 30)
    return img


def flat():
    img = np.zeros((64, 200, 3), np.uint8)
    img[10:50, 20:150] = (200, 30, 30)
    return img


def shapes():
    """name -> uint8 [H][W][3]."""
    rng = np.random.default_rng(7)
    out = {}
    for h, w in ((1, 1), (1, 2), (2, 1), (3, 5)):                       # shorter than bpp, shorter than a wave
        out[f"tiny_{h}x{w}"] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    out["odd_7x33"] = mixed(7, 33, 1)                                   # row length no multiple of 4
    out["midrow_150x100"] = mixed(150, 100, 2)                          # 45 150 bytes: both chunk boundaries fall inside a row
    out["exact_64x85"] = mixed(64, 85, 5)                               # exactly 16 384 bytes: one chunk, a boundary at the very end
    out["exact_32x341"] = mixed(32, 341, 3)                             # exactly 32 768 bytes: two full chunks
    out["exact_random_32x341"] = rng.integers(0, 256, (32, 341, 3), dtype=np.uint8)     # the same, two stored blocks
    out["flat_64x200"] = flat()                                         # runs longer than 258, runs across the chunk boundaries (38 464 bytes)
    out["zero_64x200"] = np.zeros((64, 200, 3), np.uint8)
    out["random_64x64"] = rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)             # the stored-block fallback
    return out


def fixtures():
    """The AutoHDR fixture inputs: name -> uint8 [B][H][W][3]."""
    g = np.load(os.path.join(GOLDEN, "autohdr.npz"))
    return {k: np.ascontiguousarray(g[k]) for k in ("input_mid", "input_large", "input_batch")}


def all_images():
    """Every single image of shapes() and fixtures(): name -> uint8 [H][W][3]."""
    out = shapes()
    for k, v in fixtures().items():
        for i, im in enumerate(v):
            out[f"{k}[{i}]"] = im
    return out


def fibonacci_stream():
    """Bytes whose 20 distinct values occur Fibonacci-many times (17 710 bytes: one chunk and the start of a second), shuffled."""
    fib = [1, 1]
    while len(fib) < 20:
        fib.append(fib[-1] + fib[-2])
    s = np.concatenate([np.full(c, 10 + i, np.uint8) for i, c in enumerate(fib)])
    np.random.default_rng(5).shuffle(s)
    return s.tobytes()


def deep_stream():
    """18 values with counts c_i = c_i-1 + c_i-2 + 1 (1, 1, 3, 5, 9, ... : 13 510 bytes, inside one chunk): from the third on every weight exceeds the
    sum of the two before it, so Huffman's tree is a chain 17 deep whatever the tie-breaking, and the 15-bit limit must act."""
    c = [1, 1]
    while len(c) < 18:
        c.append(c[-1] + c[-2] + 1)
    s = np.concatenate([np.full(k, 3 * i, np.uint8) for i, k in enumerate(c)])
    np.random.default_rng(6).shuffle(s)
    return s.tobytes()


def size_images():
    """The images of the size comparison against Pillow's compress_level=4: name -> uint8 [H][W][3]."""
    from PIL import Image, ImageFilter
    rng = np.random.default_rng(0)
    out = {}
    for k, v in fixtures().items():
        for i, im in enumerate(v):
            out[f"{k}[{i}]"] = im
    yy, xx = np.mgrid[0:256, 0:256]
    smooth = np.stack([127 + 100 * np.sin(xx / 97.0 + c) * np.cos(yy / 61.0 - c) for c in range(3)], -1)
    out["smooth_256"] = smooth.astype(np.uint8)
    out["smooth_noise4_256"] = np.clip(smooth + rng.normal(0, 4, smooth.shape), 0, 255).astype(np.uint8)
    out["blurred_noise_256"] = np.asarray(Image.fromarray(rng.integers(0, 256, (256, 256, 3), dtype=np.uint8)).filter(ImageFilter.GaussianBlur(6)))
    out["flat_64x200"] = flat()
    return out
