"""The 8-bit image ops of the img2img path (csrc/image.hip) through the C ABI on a real MI355X against Pillow's own results (tests/golden/usdu.npz,
tests/tools/capture_usdu.py).  Pillow's 8-bit paths are integer arithmetic, so every assertion is torch.equal on bytes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _usdu_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "usdu.npz"))


def _p(t, off=0):
    return C.c_void_p(t.data_ptr() + off)


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _pitched(a, pitch_align=16, pad_value=0xAB):
    """host uint8 [H][W][C] -> device buffer [H][pitch] (padding bytes set, to show they are neither read nor written) and its pitch"""
    h, w, c = a.shape
    pitch = (w * c + pitch_align - 1) // pitch_align * pitch_align
    buf = torch.full((h, pitch), pad_value, dtype=torch.uint8)
    buf[:, :w * c] = torch.from_numpy(np.ascontiguousarray(a)).reshape(h, w * c)
    return buf.cuda(), pitch


def _resize(ldx, L, src, src_pitch, off, h, w, c, oh, ow, name, align=16):
    """the two passes through ldx_image_resample_pass; src is a device buffer, (off, src_pitch) locate the [h][w][c] image in it"""
    cur, pitch, base, keep = src, src_pitch, off, []
    if ow != w:
        b, kk = (torch.from_numpy(t).cuda() for t in ldx.usdu.resample_coeffs(w, ow, name))      # kept alive until the synchronize below
        keep += [b, kk, cur]
        out, op = _pitched(np.zeros((h, ow, c), np.uint8), align)
        ldx.lib.check(L.ldx_image_resample_pass(_p(cur, base), pitch, h, w, c, 1, ow, _p(b), _p(kk), kk.shape[1], _p(out), op, _st()), "resample x")
        cur, pitch, base, w = out, op, 0, ow
    if oh != h:
        b, kk = (torch.from_numpy(t).cuda() for t in ldx.usdu.resample_coeffs(h, oh, name))
        keep += [b, kk, cur]
        out, op = _pitched(np.zeros((oh, w, c), np.uint8), align)
        ldx.lib.check(L.ldx_image_resample_pass(_p(cur, base), pitch, h, w, c, 0, oh, _p(b), _p(kk), kk.shape[1], _p(out), op, _st()), "resample y")
        cur, pitch, h = out, op, oh
    torch.cuda.synchronize()
    assert bool((cur[:, w * c:] == 0xAB).all())             # the padding of a row is never written
    return cur[:, :w * c].reshape(h, w, c).cpu()


@pytest.mark.parametrize("c", [3, 1])
@pytest.mark.parametrize("i", range(len(R.RESAMPLE_CASES)))
def test_lanczos_resize_equals_pillow(ldx, ldx_lib, g, i, c):
    (h, w), (oh, ow) = R.RESAMPLE_CASES[i]
    src, pitch = _pitched(R.pattern(h, w, c, 10 + i))
    out = _resize(ldx, ldx_lib, src, pitch, 0, h, w, c, oh, ow, "lanczos")
    ref = torch.from_numpy(g[f"rs_out_{i}_c{c}"])
    print(f"resize {h}x{w} -> {oh}x{ow} C={c}: {int((out != ref).sum())} differing bytes")
    assert torch.equal(out, ref)


def test_lanczos_resize_unaligned_rows(ldx, ldx_lib, g):
    """a pitch that is no multiple of 16 takes the byte-wide pass down the columns: same bytes"""
    (h, w), (oh, ow) = R.RESAMPLE_CASES[3]
    src, pitch = _pitched(R.pattern(h, w, 3, 13), pitch_align=1)
    assert torch.equal(_resize(ldx, ldx_lib, src, pitch, 0, h, w, 3, oh, ow, "lanczos", align=1), torch.from_numpy(g["rs_out_3_c3"]))


def test_lanczos_resize_of_a_pitched_crop(ldx, ldx_lib, g):
    src, pitch = _pitched(R.pattern(80, 100, 3, 30))
    out = _resize(ldx, ldx_lib, src, pitch, 5 * pitch + 9 * 3, 61, 83, 3, 64, 64, "lanczos")
    assert torch.equal(out, torch.from_numpy(g["rs_crop_out"]))
    # the pass down the columns straight from the crop (width kept): unaligned source rows
    out = _resize(ldx, ldx_lib, src, pitch, 5 * pitch + 9 * 3, 61, 83, 3, 64, 83, "lanczos")
    assert torch.equal(out, torch.from_numpy(R.resize(R.pattern(80, 100, 3, 30)[5:66, 9:92], 83, 64)))


@pytest.mark.parametrize("k,size", [(0, (256, 512)), (1, (40, 64))])
def test_bicubic_ramp_equals_pillow(ldx, ldx_lib, g, k, size):
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 256, 1)[..., None]
    src, pitch = _pitched(ramp)
    out = _resize(ldx, ldx_lib, src, pitch, 0, 256, 256, 1, size[0], size[1], "bicubic")
    assert torch.equal(out[..., 0], torch.from_numpy(g[f"bc_out_{k}"]))


def _blur(ldx, L, src, sp, off, h, w, radius, dst=None, dp=None, doff=0):
    fr = ldx.usdu.gaussian_box_params(radius)[0]
    a, ap = _pitched(np.zeros((h, w, 1), np.uint8))
    b, bp = _pitched(np.zeros((h, w, 1), np.uint8))
    if dst is None:
        dst, dp = _pitched(np.zeros((h, w, 1), np.uint8))
    chain = [(src, sp, off), (a, ap, 0), (b, bp, 0), (a, ap, 0), (b, bp, 0), (a, ap, 0), (dst, dp, doff)]
    for i in range(6):
        (s, spi, so), (d, dpi, do) = chain[i], chain[i + 1]
        ldx.lib.check(L.ldx_image_box_blur_pass(_p(s, so), spi, h, w, 1 if i < 3 else 0, fr, _p(d, do), dpi, _st()), "box blur")
    torch.cuda.synchronize()
    return dst, dp


@pytest.mark.parametrize("i", range(len(R.BLUR_CASES)))
def test_gaussian_blur_equals_pillow(ldx, ldx_lib, g, i):
    (h, w), radius, _ = R.BLUR_CASES[i]
    src, sp = _pitched(R.blur_input(i)[..., None])
    out, _ = _blur(ldx, ldx_lib, src, sp, 0, h, w, radius)
    ref = torch.from_numpy(g[f"blur_out_{i}"])
    print(f"blur case {i}: {int((out[:, :w].cpu() != ref).sum())} differing bytes")
    assert torch.equal(out[:, :w].cpu(), ref) and bool((out[:, w:] == 0xAB).all())


@pytest.mark.parametrize("i", [0, 1, 2])
def test_windowed_blur_equals_whole_canvas_blur(ldx, ldx_lib, g, i):
    (h, w), radius, rect = R.BLUR_CASES[i]
    x0, y0, x1, y1 = ldx.usdu.blur_window(rect, ldx.usdu.gaussian_box_params(radius)[1], w, h)
    assert (x1 - x0, y1 - y0) != (w, h) or i == 1
    src, sp = _pitched(R.blur_input(i)[..., None])
    dst = torch.zeros((h, sp), dtype=torch.uint8, device="cuda")
    _blur(ldx, ldx_lib, src, sp, y0 * sp + x0, y1 - y0, x1 - x0, radius, dst, sp, y0 * sp + x0)
    assert torch.equal(dst[:, :w].cpu(), torch.from_numpy(g[f"blur_out_{i}"]))


def test_composite_equals_pillow(ldx, ldx_lib, g):
    L = ldx_lib
    cv, tl, mk, big, bm, (ax, ay) = R.composite_inputs()
    for canvas, mask, x0, y0, ref in ((cv, mk, 0, 0, g["comp_out_0"]), (big, bm, ax, ay, g["comp_out_1"])):
        H, W = canvas.shape[:2]
        d, dp = _pitched(canvas)
        t, tp = _pitched(tl)
        m, mp = _pitched(mask[..., None])
        ldx.lib.check(L.ldx_image_composite(_p(d), dp, H, W, 3, x0, y0, 37, 53, _p(t), tp, _p(m), mp, _st()), "composite")
        torch.cuda.synchronize()
        assert torch.equal(d[:, :W * 3].reshape(H, W, 3).cpu(), torch.from_numpy(ref)) and bool((d[:, W * 3:] == 0xAB).all())


def test_quantise_and_to_float_equal_reference(ldx, ldx_lib, g):
    L = ldx_lib
    q_in = torch.from_numpy(g["q_in"]).cuda()
    n = q_in.numel()
    for shape in ((1, n, 1), (7, n // 7, 1)):                  # 259 = 7 * 37: odd rows take the one-element kernel; below, a multiple of 4
        out = torch.zeros(n, dtype=torch.uint8, device="cuda")
        ldx.lib.check(L.ldx_image_quantize(_p(q_in), shape[0], shape[1], 1, _p(out), shape[1], _st()), "quantize")
        assert torch.equal(out.cpu(), torch.from_numpy(g["q_out"]))
    q4 = q_in[:256].contiguous()
    out = torch.zeros(256, dtype=torch.uint8, device="cuda")
    ldx.lib.check(L.ldx_image_quantize(_p(q4), 4, 64, 1, _p(out), 64, _st()), "quantize")
    assert torch.equal(out.cpu(), torch.from_numpy(g["q_out"][:256]))
    b = torch.arange(256, dtype=torch.uint8).cuda()
    for (h, w, c) in ((1, 256, 1), (16, 16, 1)):
        f = torch.zeros(256, dtype=torch.float32, device="cuda")
        ldx.lib.check(L.ldx_image_to_float(_p(b), w * c, h, w, c, 0, 0, w, h, _p(f), _st()), "to_float")
        assert torch.equal(f.cpu(), torch.from_numpy(g["f_out"]))
    # a crop of an RGB image: rows 2..6, columns 3..8 of 8 x 10 (15 bytes per row: the one-element kernel)
    img = R.pattern(8, 10, 3, 60)
    d, dp = _pitched(img)
    f = torch.zeros((4, 5, 3), dtype=torch.float32, device="cuda")
    ldx.lib.check(L.ldx_image_to_float(_p(d), dp, 8, 10, 3, 3, 2, 5, 4, _p(f), _st()), "to_float")
    assert torch.equal(f.cpu(), torch.from_numpy(R.to_float(img[2:6, 3:8])))


def test_fill_rect(ldx, ldx_lib):
    d, dp = _pitched(np.zeros((20, 30, 1), np.uint8))
    ldx.lib.check(ldx_lib.ldx_image_fill_rect(_p(d), dp, 20, 30, 1, 4, 5, 26, 15, 255, _st()), "fill")
    ref = torch.zeros((20, 30), dtype=torch.uint8)
    ref[5:20, 4:30] = 255
    assert torch.equal(d[:, :30].cpu(), ref) and bool((d[:, 30:] == 0xAB).all())


def test_bad_arguments_return_einval(ldx, ldx_lib):
    L = ldx_lib
    u = torch.zeros(64 * 64 * 3, dtype=torch.uint8, device="cuda")
    f = torch.zeros(64 * 64 * 3, dtype=torch.float32, device="cuda")
    t = torch.zeros(64, dtype=torch.int32, device="cuda")
    calls = [
        lambda: L.ldx_image_quantize(None, 8, 8, 3, _p(u), 24, _st()),
        lambda: L.ldx_image_quantize(_p(f), 8, 8, 2, _p(u), 24, _st()),                                           # C = 2
        lambda: L.ldx_image_quantize(_p(f), 8, 8, 3, _p(u), 23, _st()),                                           # pitch < W * C
        lambda: L.ldx_image_to_float(_p(u), 24, 8, 8, 3, 4, 0, 5, 8, _p(f), _st()),                               # crop past the right edge
        lambda: L.ldx_image_to_float(_p(u), 24, 8, 8, 3, 0, -1, 8, 8, _p(f), _st()),
        lambda: L.ldx_image_to_float(_p(u), 24, 8, 8, 3, 0, 0, 8, 8, None, _st()),
        lambda: L.ldx_image_resample_pass(_p(u), 24, 8, 8, 3, 2, 4, _p(t), _p(t), 7, _p(u, 4096), 12, _st()),     # axis 2
        lambda: L.ldx_image_resample_pass(_p(u), 24, 8, 8, 3, 1, 4, None, _p(t), 7, _p(u, 4096), 12, _st()),
        lambda: L.ldx_image_resample_pass(_p(u), 24, 8, 8, 3, 1, 4, _p(t), _p(t), 7, _p(u), 12, _st()),           # in place
        lambda: L.ldx_image_resample_pass(_p(u), 24, 8, 8, 4, 1, 4, _p(t), _p(t), 7, _p(u, 4096), 16, _st()),     # C = 4
        lambda: L.ldx_image_box_blur_pass(_p(u), 8, 8, 8, 1, 300.0, _p(u, 4096), 8, _st()),                       # box radius >= 256
        lambda: L.ldx_image_box_blur_pass(_p(u), 8, 8, 8, 1, 3.5, _p(u), 8, _st()),                               # in place
        lambda: L.ldx_image_box_blur_pass(_p(u), 8, 8, 8, 1, float("nan"), _p(u, 4096), 8, _st()),
        lambda: L.ldx_image_composite(_p(u), 24, 8, 8, 3, 2, 2, 8, 8, _p(u, 4096), 24, _p(u, 8192), 8, _st()),    # rectangle outside the canvas
        lambda: L.ldx_image_composite(_p(u), 24, 8, 8, 3, 0, 0, 8, 8, _p(u, 4096), 24, None, 8, _st()),
        lambda: L.ldx_image_fill_rect(_p(u), 24, 8, 8, 3, 0, 0, 9, 8, 255, _st()),
        lambda: L.ldx_image_fill_rect(_p(u), 24, 8, 8, 3, 0, 0, 8, 8, 256, _st()),
    ]
    for i, call in enumerate(calls):
        assert call() == -1, i                                 # LDX_EINVAL
        assert b"ldx_image_" in L.ldx_last_error()
    torch.cuda.synchronize()
    assert int(u.sum()) == 0 and float(f.sum()) == 0.0         # nothing ran
