"""The three fp32 canvas kernels of the ADetailer path (csrc/detail.hip through the C ABI) on a real MI355X against their numpy statement
(lightdiffusion-next_amd/detailer.py: blur_mask_host, paste_host, quantize_host), bit for bit: each product and each sum is one rounded fp32 operation
in a stated order, so nothing with a tolerance is left."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _usdu_ref as R  # noqa: E402

LDX_EINVAL = -1


def _st(ldx):
    return ldx.lib.current_stream_ptr()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _mask(h, w, seed, fractional):
    rng = np.random.default_rng(seed)
    m = np.zeros((h, w), np.float32)
    m[h // 5:h - h // 4, w // 6:w - w // 3] = 1.0            # a box of ones, as a detector's bbox mask
    if fractional:
        m = (m * rng.random((h, w))).astype(np.float32)
        m[0], m[:, -1] = rng.random(w).astype(np.float32), 1.0   # values on the border, where the padding reflects
    return m


def _blur(ldx, lib, m, table):
    h, w = m.shape
    src, t = torch.from_numpy(m).cuda(), torch.from_numpy(table).cuda()
    out = torch.full((h + 1, w), -7.0, device="cuda")          # one guard row behind the output
    rc = lib.ldx_detail_blur_mask(ldx.lib.ptr(src), h, w, ldx.lib.ptr(t), table.shape[0], ldx.lib.ptr(out), _st(ldx))
    return rc, out.cpu().numpy()


@pytest.mark.parametrize("shape, feather, fractional", [((37, 53), 5, False), ((6, 40), 5, False), ((96, 96), 20, False), ((37, 53), 5, True),
                                                        ((300, 270), 5, True), ((37, 53), 0, True)])
def test_blur_mask_bit_for_bit(ldx, ldx_lib, shape, feather, fractional):
    m = _mask(*shape, seed=shape[0] + feather, fractional=fractional)
    table = ldx.detailer.blur_table(feather)
    rc, out = _blur(ldx, ldx_lib, m, table)
    ref = ldx.detailer.blur_mask_host(m, table)
    assert rc == 0
    print(f"{shape} k = {table.shape[0]}: {int((_bits(out[:-1]) != _bits(ref)).sum())} differing values of {ref.size}")
    assert np.array_equal(_bits(out[:-1]), _bits(ref)) and (out[-1] == -7.0).all()
    assert ref.max() <= 1.0 + 1e-5 and (feather == 0 or not np.array_equal(ref, m))


def test_blur_mask_refuses_what_torch_refuses(ldx, ldx_lib):
    table = ldx.detailer.blur_table(5)
    for shape in ((5, 40), (40, 5)):                            # reflect padding 5 needs more than 5 rows and columns
        rc, out = _blur(ldx, ldx_lib, np.ones(shape, np.float32), table)
        assert rc == LDX_EINVAL and (out == -7.0).all()
    m = torch.ones(40, 40, device="cuda")
    t = torch.from_numpy(np.ones((4, 4), np.float32)).cuda()
    assert ldx_lib.ldx_detail_blur_mask(ldx.lib.ptr(m), 40, 40, ldx.lib.ptr(t), 4, ldx.lib.ptr(torch.empty_like(m)), _st(ldx)) == LDX_EINVAL   # even k
    assert ldx_lib.ldx_detail_blur_mask(ldx.lib.ptr(m), 40, 40, ldx.lib.ptr(t), 65, ldx.lib.ptr(torch.empty_like(m)), _st(ldx)) == LDX_EINVAL  # k > 63


def _paste_inputs():
    rng = np.random.default_rng(21)
    H, W, h, w = 80, 96, 50, 40                                # a 96 x 80 canvas, a 40 x 50 tile
    canvas = (rng.integers(0, 256, (H, W, 3)).astype(np.float32) / np.float32(255.0))       # exact k / 255 values
    canvas[::3] = rng.random((len(range(0, H, 3)), W, 3)).astype(np.float32)
    src = rng.random((h, w, 3)).astype(np.float32)
    src[::2] = rng.integers(0, 256, (len(range(0, h, 2)), w, 3)).astype(np.float32) / np.float32(255.0)
    m = rng.random((h, w)).astype(np.float32)
    m[:, 8:16], m[:, 16:24] = 0.0, 1.0                         # columns 0..7 stay fractional: the one pixel of the last case is blended
    return canvas, src, m


@pytest.mark.parametrize("at", [(70, 50), (10, 5), (56, 30), (95, 79)])
def test_paste_bit_for_bit(ldx, ldx_lib, at):
    """(70, 50): clipped on both axes; (10, 5): inside; (56, 30): touching both borders; (95, 79): one pixel left"""
    canvas, src, m = _paste_inputs()
    H, W, _ = canvas.shape
    x0, y0 = at
    d = torch.from_numpy(canvas).cuda()
    s, mm = torch.from_numpy(src).cuda(), torch.from_numpy(m).cuda()
    assert ldx_lib.ldx_detail_paste(ldx.lib.ptr(d), H, W, x0, y0, ldx.lib.ptr(s), ldx.lib.ptr(mm), src.shape[0], src.shape[1], _st(ldx)) == 0
    ref = ldx.detailer.paste_host(canvas.copy(), src, m, x0, y0)
    got = d.cpu().numpy()
    print(f"tile at {at}: {int((_bits(got) != _bits(ref)).sum())} differing values")
    assert np.array_equal(_bits(got), _bits(ref))
    outside = np.ones((H, W), bool)
    outside[y0:y0 + src.shape[0], x0:x0 + src.shape[1]] = False
    assert np.array_equal(got[outside], canvas[outside]) and not np.array_equal(got, canvas)
    # mask 0 keeps the canvas value and mask 1 takes the tile's, exactly
    hh, ww = min(H - y0, src.shape[0]), min(W - x0, src.shape[1])
    z, o = min(ww, 16), min(ww, 24)
    assert np.array_equal(got[y0:y0 + hh, x0 + 8:x0 + z], canvas[y0:y0 + hh, x0 + 8:x0 + z])
    assert np.array_equal(got[y0:y0 + hh, x0 + 16:x0 + o], src[:hh, 16:o])
    assert at != (70, 50) or (z, o) == (16, 24)                # the clipped case of the issue holds mask values 0, 1 and fractions


def test_paste_refuses_a_corner_outside(ldx, ldx_lib):
    canvas, src, m = _paste_inputs()
    d, s, mm = torch.from_numpy(canvas).cuda(), torch.from_numpy(src).cuda(), torch.from_numpy(m).cuda()
    for x0, y0 in ((96, 0), (0, 80), (-1, 0)):
        assert ldx_lib.ldx_detail_paste(ldx.lib.ptr(d), 80, 96, x0, y0, ldx.lib.ptr(s), ldx.lib.ptr(mm), 50, 40, _st(ldx)) == LDX_EINVAL
    assert np.array_equal(d.cpu().numpy(), canvas)


@pytest.mark.parametrize("rect", [(7, 9, 37, 22), (0, 0, 51, 33), (14, 11, 37, 22), (50, 32, 1, 1)])
def test_crop_quantize_bit_for_bit(ldx, ldx_lib, rect):
    """(x0, y0, w, h) on a 51 x 33 canvas: interior, the whole canvas, against the right and bottom border, the last pixel"""
    H, W = 33, 51
    special = np.concatenate([np.arange(256, dtype=np.float32) / np.float32(255.0), np.array([-0.5, 1.5, 0.999999], np.float32)])
    rng = np.random.default_rng(4)
    canvas = rng.random((H, W, 3)).astype(np.float32)
    flat = canvas.reshape(-1)
    flat[rng.permutation(flat.size)[:special.size * 12]] = np.tile(special, 12)          # every special value about 12 times, anywhere
    block = canvas[9:12, 7:44].copy().reshape(-1)                                        # and once in order, inside the first rectangle
    block[:special.size] = special
    canvas[9:12, 7:44] = block.reshape(3, 37, 3)
    x0, y0, w, h = rect
    pitch = (w * 3 + 15) // 16 * 16
    d = torch.from_numpy(canvas).cuda()
    out = torch.full((h + 1, pitch), 99, dtype=torch.uint8, device="cuda")
    assert ldx_lib.ldx_detail_crop_quantize(ldx.lib.ptr(d), H, W, x0, y0, w, h, ldx.lib.ptr(out), pitch, _st(ldx)) == 0
    got = out.cpu().numpy()
    ref = ldx.detailer.quantize_host(canvas[y0:y0 + h, x0:x0 + w]).reshape(h, w * 3)
    assert np.array_equal(ref, R.quantize(canvas[y0:y0 + h, x0:x0 + w]).reshape(h, w * 3))       # the img2img path's rule (tests/_usdu_ref.py)
    assert np.array_equal(got[:h, :w * 3], ref) and (got[:h, w * 3:] == 99).all() and (got[h] == 99).all()
    assert np.array_equal(d.cpu().numpy(), canvas)


def test_crop_quantize_refuses_a_rectangle_outside(ldx, ldx_lib):
    d = torch.zeros(33, 51, 3, device="cuda")
    out = torch.full((64, 256), 99, dtype=torch.uint8, device="cuda")
    for x0, y0, w, h in ((20, 0, 32, 10), (0, 30, 10, 4), (-1, 0, 5, 5), (0, 0, 0, 5)):
        assert ldx_lib.ldx_detail_crop_quantize(ldx.lib.ptr(d), 33, 51, x0, y0, w, h, ldx.lib.ptr(out), 256, _st(ldx)) == LDX_EINVAL
    assert ldx_lib.ldx_detail_crop_quantize(ldx.lib.ptr(d), 33, 51, 0, 0, 20, 5, ldx.lib.ptr(out), 59, _st(ldx)) == LDX_EINVAL       # pitch < w * 3
    assert (out == 99).all()
