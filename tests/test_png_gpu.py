"""The PNG encoder on the device (csrc/png.hip through the C ABI and through ldx_amd.PNGEncoder) against its numpy statement (png.py: png_host,
filter_host, zlib_host).  Every device step is an integer rule, so the comparison is exact: the files are equal byte for byte, and any differing byte
is a bug, not a tolerance.  That the numpy statement writes valid PNGs of a sensible size is tests/test_png_host_cpu.py's subject."""
import ctypes as C
import io
import os
import sys
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import png_cases  # noqa: E402

pytestmark = pytest.mark.gpu

IMAGES = png_cases.all_images()
GUARD = 0xAB


@pytest.fixture(scope="module")
def host(ldx):
    """png_host of every shared image, computed once: name -> bytes."""
    return {name: ldx.png.png_host(img) for name, img in IMAGES.items()}


@pytest.fixture(scope="module")
def enc(ldx, ldx_lib):
    return ldx.PNGEncoder(device=0)


def _p(t, off=0):
    return C.c_void_p(t.data_ptr() + off)


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _decode(data):
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert("RGB")) if im.mode != "RGB" else np.asarray(im)


@pytest.mark.parametrize("name", sorted(IMAGES))
def test_encode_is_png_host(ldx, enc, host, name):
    """Byte input and fp32 input, one instance across all the shapes (the buffers are kept per shape); the length word is the file's length."""
    img = IMAGES[name]
    (got,) = enc.encode(torch.from_numpy(img).cuda())
    assert got == host[name], (len(got), len(host[name]))
    _, lens = enc.encode_device(torch.from_numpy(img).cuda()[None])
    assert lens.cpu().tolist() == [len(host[name])]
    # fp32 as the pipeline hands it over: bytes / 255, which the truncation brings back to the same bytes or to one below
    x = torch.from_numpy(img).float() / 255
    q = ldx.png.quantize(x.numpy())
    (got,) = enc.encode(x.cuda())
    assert got == ldx.png.png_host(q)
    (got,) = enc.encode((x + 0.001).cuda())                              # + 0.001: the codes survive the truncation
    assert got == host[name]


def test_filter_stage_alone(ldx, ldx_lib):
    for name in ("odd_7x33", "midrow_150x100", "tiny_1x1", "tiny_2x1", "input_mid[0]"):
        img = IMAGES[name]
        h, w, _ = img.shape
        n = h * (1 + 3 * w)
        want, want_types = ldx.png.filter_host(img)
        for src in (torch.from_numpy(img).cuda(), (torch.from_numpy(img).float() / 255 + 0.001).cuda()):
            out = torch.full((n + 16,), GUARD, dtype=torch.uint8, device="cuda")
            types = torch.full((h + 16,), GUARD, dtype=torch.uint8, device="cuda")
            is_u8 = src.dtype == torch.uint8
            ldx.lib.check(ldx_lib.ldx_png_filter(None if is_u8 else _p(src), _p(src) if is_u8 else None, w * 3, 1, h, w, _p(out), _p(types), _st()),
                          "ldx_png_filter")
            assert np.array_equal(out.cpu().numpy()[:n].reshape(h, 1 + 3 * w), want), name
            assert np.array_equal(types.cpu().numpy()[:h], want_types), name
            assert (out.cpu().numpy()[n:] == GUARD).all() and (types.cpu().numpy()[h:] == GUARD).all()
    assert len(set(ldx.png.filter_host(IMAGES["input_mid[0]"])[1].tolist())) >= 3       # the choice is exercised


def _zlib_device(ldx, ldx_lib, data):
    n = len(data)
    src = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    nws, bound = int(ldx_lib.ldx_zlib_workspace_bytes(n)), int(ldx_lib.ldx_zlib_bound_bytes(n))
    ws = torch.full((nws + 64,), GUARD, dtype=torch.uint8, device="cuda")
    out = torch.full((bound + 64,), GUARD, dtype=torch.uint8, device="cuda")
    length = torch.zeros(1, dtype=torch.int32, device="cuda")
    ldx.lib.check(ldx_lib.ldx_zlib_deflate(_p(src), n, _p(ws), _p(out), _p(length), _st()), "ldx_zlib_deflate")
    m = int(length.cpu()[0])
    assert 0 < m <= bound
    res = out.cpu().numpy()
    assert (res[m:] == GUARD).all() and (ws.cpu().numpy()[nws:] == GUARD).all()
    return res[:m].tobytes()


@pytest.mark.parametrize("which", ["fibonacci", "deep", "blob", "one_byte"])
def test_deflate_stage_alone(ldx, ldx_lib, which):
    """The code-length limit (Fibonacci counts; counts that force a chain 17 deep), one byte, and four kinds of content across ten chunks."""
    if which == "fibonacci":
        data = png_cases.fibonacci_stream()
    elif which == "deep":
        data = png_cases.deep_stream()
    elif which == "one_byte":
        data = b"\x07"
    else:
        data = np.concatenate([IMAGES["midrow_150x100"].reshape(-1), np.zeros(40000, np.uint8), IMAGES["random_64x64"].reshape(-1),
                               ldx.png.filter_host(IMAGES["input_mid[0]"])[0].reshape(-1)]).tobytes()
    got = _zlib_device(ldx, ldx_lib, data)
    assert zlib.decompress(got) == data
    assert got == ldx.png.zlib_host(data)


def test_quantisation_of_fp32_input(enc):
    """-0.1, 0, every k / 255 and the values one ulp either side, 0.999999, 1.0, 1.5: (uint8) trunc(clamp(255.0f * v, 0, 255))."""
    k = np.arange(256, dtype=np.float32) / np.float32(255.0)
    vals = np.concatenate([np.float32([-0.1, 0.0]), k, np.nextafter(k, np.float32(-1)), np.nextafter(k, np.float32(2)), np.float32([0.999999, 1.0, 1.5])])
    x = np.full(7 * 37 * 3, 0.5, np.float32)
    x[:vals.size] = vals
    x = x.reshape(7, 37, 3)
    want = np.clip(x * 255.0, 0, 255).astype(np.uint8)
    assert want.min() == 0 and want.max() == 255 and x.dtype == np.float32
    (got,) = enc.encode(torch.from_numpy(x).cuda())
    assert np.array_equal(_decode(got), want)


def test_batch_gives_independent_files(ldx, enc):
    imgs = np.stack([png_cases.mixed(150, 100, 31), IMAGES["midrow_150x100"], np.random.default_rng(32).integers(0, 256, (150, 100, 3), dtype=np.uint8)])
    files = enc.encode(torch.from_numpy(imgs).cuda())
    assert len(files) == 3 and len(set(files)) == 3
    for f, im in zip(files, imgs):
        assert f == ldx.png.png_host(im)
    files_f = enc.encode((torch.from_numpy(imgs).float() / 255 + 0.001).cuda())
    assert files_f == files


def test_pitched_bytes_and_guards_through_the_c_abi(ldx, ldx_lib, host):
    """Two images in rows of pitch > 3 W; the bytes past each file's length, past the strided output and past the workspace keep their pattern."""
    u8 = png_cases.fixtures()["input_batch"]
    b, h, w, _ = u8.shape
    pitch = w * 3 + 11
    src = torch.full((b, h, pitch), GUARD, dtype=torch.uint8)
    src[:, :, :w * 3] = torch.from_numpy(u8).reshape(b, h, w * 3)
    src = src.cuda()
    nws, bound = int(ldx_lib.ldx_png_workspace_bytes(b, h, w)), int(ldx_lib.ldx_png_bound_bytes(h, w))
    stride = bound + 37
    ws = torch.full((nws + 256,), GUARD, dtype=torch.uint8, device="cuda")
    out = torch.full((b * stride + 256,), GUARD, dtype=torch.uint8, device="cuda")
    lens = torch.zeros(b + 2, dtype=torch.int32, device="cuda")
    ldx.lib.check(ldx_lib.ldx_png_encode(None, _p(src), pitch, b, h, w, _p(ws), _p(out), stride, _p(lens), _st()), "ldx_png_encode")
    res, n = out.cpu().numpy(), lens.cpu().tolist()
    assert n[b:] == [0, 0]
    for i in range(b):
        want = host[f"input_batch[{i}]"]
        assert n[i] == len(want) <= bound
        assert res[i * stride:i * stride + n[i]].tobytes() == want
        assert (res[i * stride + n[i]:(i + 1) * stride] == GUARD).all()
    assert (res[b * stride:] == GUARD).all() and (ws.cpu().numpy()[nws:] == GUARD).all()
    assert (src.cpu()[:, :, w * 3:] == GUARD).all()


def test_512_square_decodes_to_the_input(enc):
    """49 chunks, checked by Pillow alone."""
    img = np.tile(png_cases.mixed(128, 128, 41), (4, 4, 1))
    img[200:300, 100:400] = np.random.default_rng(42).integers(0, 256, (100, 300, 3), dtype=np.uint8)
    (got,) = enc.encode(torch.from_numpy(img).cuda())
    assert np.array_equal(_decode(got), img)
    assert len(got) < img.size


def test_bad_arguments_return_einval(ldx, ldx_lib, enc):
    L = ldx_lib
    u = torch.zeros(8 * 8 * 3, dtype=torch.uint8, device="cuda")
    f = torch.zeros(8 * 8 * 3, dtype=torch.float32, device="cuda")
    ws = torch.zeros(int(L.ldx_png_workspace_bytes(1, 8, 8)), dtype=torch.uint8, device="cuda")
    bound = int(L.ldx_png_bound_bytes(8, 8))
    out = torch.zeros(bound, dtype=torch.uint8, device="cuda")
    n = torch.zeros(1, dtype=torch.int32, device="cuda")
    calls = [
        lambda: L.ldx_png_encode(_p(f), _p(u), 24, 1, 8, 8, _p(ws), _p(out), bound, _p(n), _st()),          # both inputs
        lambda: L.ldx_png_encode(None, None, 24, 1, 8, 8, _p(ws), _p(out), bound, _p(n), _st()),            # neither
        lambda: L.ldx_png_encode(None, _p(u), 23, 1, 8, 8, _p(ws), _p(out), bound, _p(n), _st()),           # pitch < 3 W
        lambda: L.ldx_png_encode(_p(f), None, 0, 1, 0, 8, _p(ws), _p(out), bound, _p(n), _st()),            # H = 0
        lambda: L.ldx_png_encode(_p(f), None, 0, 1, 8, -8, _p(ws), _p(out), bound, _p(n), _st()),           # W < 0
        lambda: L.ldx_png_encode(_p(f), None, 0, 0, 8, 8, _p(ws), _p(out), bound, _p(n), _st()),            # B = 0
        lambda: L.ldx_png_encode(_p(f), None, 0, 1, 8, 8, None, _p(out), bound, _p(n), _st()),              # no workspace
        lambda: L.ldx_png_encode(_p(f), None, 0, 1, 8, 8, _p(ws, 4), _p(out), bound, _p(n), _st()),         # workspace not 16-byte aligned
        lambda: L.ldx_png_encode(_p(f), None, 0, 1, 8, 8, _p(ws), _p(out), bound - 1, _p(n), _st()),        # out_stride below the bound
        lambda: L.ldx_png_encode(_p(f), None, 0, 1, 8, 8, _p(ws), None, bound, _p(n), _st()),
        lambda: L.ldx_png_encode(_p(f), None, 0, 1, 8, 8, _p(ws), _p(out), bound, None, _st()),
        lambda: L.ldx_png_filter(_p(f), _p(u), 24, 1, 8, 8, _p(out), None, _st()),
        lambda: L.ldx_png_filter(None, _p(u), 23, 1, 8, 8, _p(out), None, _st()),
        lambda: L.ldx_png_filter(None, _p(u), 24, 1, 8, 8, None, None, _st()),
        lambda: L.ldx_zlib_deflate(None, 8, _p(ws), _p(out), _p(n), _st()),
        lambda: L.ldx_zlib_deflate(_p(u), 0, _p(ws), _p(out), _p(n), _st()),
        lambda: L.ldx_zlib_deflate(_p(u), 8, None, _p(out), _p(n), _st()),
    ]
    for i, call in enumerate(calls):
        assert call() == -1, i                                 # LDX_EINVAL
        assert b"ldx_png_" in L.ldx_last_error() or b"ldx_zlib_" in L.ldx_last_error()
    torch.cuda.synchronize()
    assert int(out.sum()) == 0 and int(ws.sum()) == 0 and int(n.sum()) == 0            # nothing ran
    for bad in (torch.zeros((1, 8, 8, 4), device="cuda"), torch.zeros((8, 8, 1), device="cuda"), torch.zeros((8, 8), device="cuda"),
                torch.zeros((8, 8, 3), dtype=torch.float16, device="cuda")):
        with pytest.raises(ValueError):
            enc.encode(bad)
    with pytest.raises(ValueError):
        enc.encode(torch.zeros((8, 8, 3)))                       # a host tensor


def test_follows_autohdr_on_the_same_stream(ldx, ldx_lib, enc):
    """AutoHDR.apply(out_u8=True) and encode back to back on a side stream, nothing waiting in between: the file is autohdr_host's bytes."""
    u8 = png_cases.fixtures()["input_mid"]
    fx = ldx.AutoHDR(device=0)
    src = torch.from_numpy(u8).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        (got,) = enc.encode(fx.apply(src, out_u8=True))
    assert np.array_equal(_decode(got), ldx.hdr.autohdr_host(u8[0]))
    assert got == ldx.png.png_host(ldx.hdr.autohdr_host(u8[0]))
