"""AutoHDR, the reference's default post-effect (src/AutoHDR/ahdr.py:83-127, HDREffects.apply_hdr2; all five exits of src/user/pipeline.py pass the
decoded image through it), on the device: the VAE's fp32 image goes in, the reference's values come out, and nothing visits the host.

The reference does it in PIL + LittleCMS + numpy.  Every part is restated here as the integer / float32 rule it is:
  Lab round trip    ImageCms.profileToProfile (8-bit sRGB -> 8-bit Lab -> 8-bit sRGB, perceptual, flags 0) is, after lcms's resampling optimisation, a
                    33 x 33 x 33 table of 16-bit values read with fixed-point tetrahedral interpolation: lcms_tables() builds both tables, table_read()
                    is the read.  The node values are computed in double here and in float32 by lcms: about one colour in 50 000 is a code off.
  luminance chain   merge_adjustments_with_blend_modes + apply_gamma_correction act on the 8-bit L channel alone: luminance_lut() is their 256 bytes.
  contrast, colour  ImageEnhance.Contrast / Color: Pillow's integer grey, one integer mean, Image.blend in float32 with truncation: contrast_color_host().
autohdr_host() is the whole effect in numpy on one image: the statement of the algorithm and what the device tests compare with.  AutoHDR runs it in two
launches per call (ldx_hdr_apply, csrc/hdr.hip -> libldx_hdr.so), byte for byte equal to autohdr_host.
"""
import functools

import numpy as np
import torch

from . import lib

GRID = 33                               # lcms's grid points per axis for 3 input channels at flags 0

_D50 = np.array([0.9642, 1.0, 0.8249])
_BRADFORD = np.array([[0.8951, 0.2664, -0.1614], [-0.7502, 1.7135, 0.0367], [0.0389, -0.0685, 1.0296]])


def _xyz_of_xy(x, y):
    return np.array([x / y, 1.0, (1.0 - x - y) / y])


def _rgb_to_xyz_d50():
    """Bradford(D65 -> D50) . RGB -> XYZ of the sRGB primaries, in double."""
    white = _xyz_of_xy(0.3127, 0.3290)
    prim = np.stack([_xyz_of_xy(0.64, 0.33), _xyz_of_xy(0.30, 0.60), _xyz_of_xy(0.15, 0.06)], axis=1)
    rgb2xyz = prim * np.linalg.solve(prim, white)[None, :]
    gain = (_BRADFORD @ _D50) / (_BRADFORD @ white)
    adapt = np.linalg.solve(_BRADFORD, np.diag(gain) @ _BRADFORD)
    return adapt @ rgb2xyz


def _quantise16(v):
    return np.clip(np.floor(v * 65535.0 + 0.5), 0, 65535).astype(np.uint16)


@functools.lru_cache(maxsize=1)
def lcms_tables():
    """(forward sRGB -> Lab, inverse Lab -> sRGB) as uint16 [33][33][33][4] (the fourth value is padding: one node = one 8-byte load), the first input
    channel on the first axis.  Built once in double; cached, treat as read-only."""
    c = np.floor(np.arange(GRID) * 65535.0 / 32.0 + 0.5) / 65535.0
    n0, n1, n2 = np.meshgrid(c, c, c, indexing="ij")
    m = _rgb_to_xyz_d50()
    # forward node: sRGB curve, matrix, Lab against D50, the 16-bit Lab encoding
    rgb = np.stack([n0, n1, n2], axis=-1)
    lin = np.where(rgb >= 0.04045, ((rgb + 0.055) / 1.055) ** 2.4, rgb / 12.92)
    t = (lin @ m.T) / _D50
    f = np.where(t > (24.0 / 116.0) ** 3, np.cbrt(t), (841.0 / 108.0) * t + 16.0 / 116.0)
    big_l, a, b = 116.0 * f[..., 1] - 16.0, 500.0 * (f[..., 0] - f[..., 1]), 200.0 * (f[..., 1] - f[..., 2])
    fwd = np.zeros((GRID, GRID, GRID, 4), np.uint16)
    fwd[..., :3] = _quantise16(np.stack([big_l / 100.0, (a + 128.0) / 255.0, (b + 128.0) / 255.0], axis=-1))
    # inverse node: Lab -> XYZ, matrix, sRGB curve; out-of-gamut colours clip at the node
    big_l, a, b = 100.0 * n0, 255.0 * n1 - 128.0, 255.0 * n2 - 128.0
    fy = (big_l + 16.0) / 116.0
    f = np.stack([fy + a / 500.0, fy, fy - b / 200.0], axis=-1)
    xyz = np.where(f > 24.0 / 116.0, f ** 3, (108.0 / 841.0) * (f - 16.0 / 116.0)) * _D50
    lin = xyz @ np.linalg.inv(m).T
    rgb = np.where(lin >= 0.04045 / 12.92, 1.055 * np.maximum(lin, 0.0) ** (1.0 / 2.4) - 0.055, 12.92 * lin)
    inv = np.zeros((GRID, GRID, GRID, 4), np.uint16)
    inv[..., :3] = _quantise16(rgb)
    fwd.setflags(write=False)
    inv.setflags(write=False)
    return fwd, inv


def table_read(table, pixels):
    """lcms's 8-bit tetrahedral read of a [33][33][33][4] table: pixels uint8 [..., 3] -> uint8 [..., 3].  Integer arithmetic throughout: per channel
    a = 32 * 257 * v, fx = a + (a + 0x7FFF) / 0xFFFF, cell i0 = fx >> 16, rest r = fx & 0xFFFF; the walk from node (i0, i0, i0) raises one coordinate at a
    time, largest rest first; out16 = T[node_0] + ((rest + (rest >> 16)) >> 16) with rest = sum_k (T[node_k] - T[node_k-1]) r_k + 0x8001;
    out8 = (out16 * 65281 + 8388608) >> 24."""
    px = np.asarray(pixels)
    v = px.reshape(-1, 3).astype(np.int64)
    a = 32 * 257 * v
    fx = a + (a + 0x7FFF) // 0xFFFF
    i0, r = fx >> 16, fx & 0xFFFF
    i1 = np.minimum(i0 + 1, GRID - 1)
    order = np.argsort(-r, axis=1, kind="stable")
    t = np.asarray(table)[..., :3].astype(np.int64)
    rows = np.arange(v.shape[0])
    idx = i0.copy()
    base = prev = t[idx[:, 0], idx[:, 1], idx[:, 2]]
    rest = np.full(base.shape, 0x8001, np.int64)
    for k in range(3):
        ch = order[:, k]
        idx[rows, ch] = i1[rows, ch]
        cur = t[idx[:, 0], idx[:, 1], idx[:, 2]]
        rest += (cur - prev) * r[rows, ch][:, None]
        prev = cur
    out16 = base + ((rest + (rest >> 16)) >> 16)
    return ((out16 * 65281 + 8388608) >> 24).astype(np.uint8).reshape(px.shape)


@functools.lru_cache(maxsize=32)
def luminance_lut(hdr_intensity=0.75, shadow_intensity=0.25, highlight_intensity=0.5, gamma_intensity=0.25):
    """merge_adjustments_with_blend_modes (ahdr.py:35-57), then apply_gamma_correction (:59-71), on all 256 values of the 8-bit L channel: uint8 [256].
    numpy in the reference's own types: the merge in float32, its astype(uint8) truncation, the gamma step on that uint8 array (so in double), with
    the gamma == 0 branch.  Cached, treat as read-only."""
    base = np.arange(256, dtype=np.float32)
    scaled_shadow = shadow_intensity ** 2 * hdr_intensity
    scaled_highlight = highlight_intensity ** 2 * hdr_intensity
    shadow_mask = np.clip((1 - (base / 255)) ** 2, 0, 1)
    highlight_mask = np.clip((base / 255) ** 2, 0, 1)
    adjusted_shadows = np.clip(base * (1 - shadow_mask * scaled_shadow), 0, 255)
    adjusted_highlights = np.clip(base + (255 - base) * highlight_mask * scaled_highlight, 0, 255)
    adjusted = np.clip(adjusted_shadows + adjusted_highlights - base, 0, 255)
    merged = np.clip(base * (1 - hdr_intensity) + adjusted * hdr_intensity, 0, 255).astype(np.uint8)
    if gamma_intensity == 0:
        out = np.clip(merged, 0, 255).astype(np.uint8)
    else:
        out = np.clip(255 * ((merged / 255) ** (1 / (1.1 - gamma_intensity))), 0, 255).astype(np.uint8)
    out.setflags(write=False)
    return out


def grey(rgb):
    """Pillow's RGB -> L: (R * 19595 + G * 38470 + B * 7471 + 0x8000) >> 16, on uint8 [..., 3]."""
    v = np.asarray(rgb).astype(np.int64)
    return ((v[..., 0] * 19595 + v[..., 1] * 38470 + v[..., 2] * 7471 + 0x8000) >> 16).astype(np.uint8)


def blend(deg, v, factor):
    """Pillow's Image.blend(degenerate, image, factor) outside [0, 1]: float32 t = deg + f * (v - deg), t <= 0 -> 0, t >= 255 -> 255, else truncate."""
    d, x = np.asarray(deg, dtype=np.float32), np.asarray(v, dtype=np.float32)
    t = d + np.float32(factor) * (x - d)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, t)).astype(np.uint8)


def grey_mean(rgb):
    """ImageEnhance.Contrast's int(mean + 0.5) of the grey image, in integers: (2 sum + n) / (2 n)."""
    g = grey(rgb)
    return (2 * int(g.sum(dtype=np.int64)) + g.size) // (2 * g.size)


def contrast_color_host(rgb, contrast=0.1, enhance_color=0.25):
    """ImageEnhance.Contrast(img).enhance(1 + contrast), then ImageEnhance.Color(.).enhance(1 + enhance_color * 0.2) (ahdr.py:118-125) on uint8 [H][W][3]."""
    c = blend(np.float32(grey_mean(rgb)), rgb, 1 + contrast)
    return blend(grey(c)[..., None], c, 1 + enhance_color * 0.2)


def autohdr_host(u8_image, hdr_intensity=0.75, shadow_intensity=0.25, highlight_intensity=0.5, gamma_intensity=0.25, contrast=0.1, enhance_color=0.25,
                 out_u8=True):
    """apply_hdr2 on one uint8 [H][W][3] image, in numpy: the final bytes, or with out_u8=False pil2tensor's fp32 bytes / 255."""
    fwd, inv = lcms_tables()
    lab = table_read(fwd, u8_image).copy()
    lab[..., 0] = luminance_lut(hdr_intensity, shadow_intensity, highlight_intensity, gamma_intensity)[lab[..., 0]]
    out = contrast_color_host(table_read(inv, lab), contrast, enhance_color)
    return out if out_u8 else out.astype(np.float32) / np.float32(255.0)


class AutoHDR:
    """apply_hdr2 on device images.  The two tables are uploaded once per instance, a luminance table once per parameter set, the workspace is kept per
    shape; apply() is two launches on the current stream, with no allocation after the first call of a shape and no host synchronisation, so it follows
    VAEDecoderEngine.decode or UltimateSDUpscale.upscale on the same stream."""

    def __init__(self, device=0):
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self._lib = lib.load()
        fwd, inv = lcms_tables()
        self._fwd = torch.from_numpy(np.array(fwd).view(np.int16)).to(self.device)
        self._inv = torch.from_numpy(np.array(inv).view(np.int16)).to(self.device)
        self._luts, self._ws = {}, {}

    def _lut(self, key):
        if key not in self._luts:
            self._luts[key] = torch.from_numpy(np.array(luminance_lut(*key))).to(self.device)
        return self._luts[key]

    def apply(self, image, hdr_intensity=0.75, shadow_intensity=0.25, highlight_intensity=0.5, gamma_intensity=0.25, contrast=0.1, enhance_color=0.25,
              out_u8=False):
        """image: device fp32 [B][H][W][3] in [0, 1] (quantised as tensor2pil does) or device uint8 [B][H][W][3].  Returns the reference's fp32
        [B][H][W][3] (bytes / 255), or the bytes with out_u8=True.  Every image of the batch gets its own mean, as apply_to_batch does."""
        if image.dim() != 4 or image.shape[-1] != 3 or image.dtype not in (torch.float32, torch.uint8):
            raise ValueError(f"AutoHDR.apply takes fp32 or uint8 [B, H, W, 3], not {image.dtype} {tuple(image.shape)}")
        if image.device != self.device:
            raise ValueError(f"AutoHDR.apply: image on {image.device}, instance on {self.device}")
        image = image.contiguous()
        b, h, w, _ = image.shape
        lut = self._lut((float(hdr_intensity), float(shadow_intensity), float(highlight_intensity), float(gamma_intensity)))
        ws = self._ws.get((b, h, w))
        if ws is None:
            nbytes = int(self._lib.ldx_hdr_workspace_bytes(b, h, w))
            if nbytes < 0:                                          # a shape the kernels refuse (the grey sum of one image is a uint32)
                lib.check(nbytes, "ldx_hdr_workspace_bytes")
            ws = self._ws[(b, h, w)] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        is_u8 = image.dtype == torch.uint8
        out = torch.empty((b, h, w, 3), dtype=torch.uint8 if out_u8 else torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            lib.check(self._lib.ldx_hdr_apply(None if is_u8 else lib.ptr(image), lib.ptr(image) if is_u8 else None, w * 3, b, h, w,
                                              lib.ptr(self._fwd), lib.ptr(self._inv), lib.ptr(lut), float(1 + contrast), float(1 + enhance_color * 0.2),
                                              lib.ptr(ws), lib.ptr(out) if out_u8 else None, w * 3, None if out_u8 else lib.ptr(out),
                                              lib.current_stream_ptr()), "ldx_hdr_apply")
        return out
