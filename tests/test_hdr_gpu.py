"""AutoHDR on the device (csrc/hdr.hip through the C ABI and through ldx_amd.AutoHDR) against its numpy statement (hdr.py: table_read, autohdr_host).
Every device step is an integer rule or a single float32 operation, so the comparison is exact: any differing byte is a bug, not a tolerance.  What
the numpy statement differs from the reference by is tests/test_hdr_host_cpu.py's subject."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PARAM_SETS = (dict(), dict(gamma_intensity=0.0), dict(hdr_intensity=1.0, shadow_intensity=0.5, highlight_intensity=0.75),
              dict(hdr_intensity=0.3, gamma_intensity=0.6, contrast=0.35, enhance_color=1.0))


@pytest.fixture(scope="module")
def G(golden_dir):
    return np.load(os.path.join(golden_dir, "autohdr.npz"))


@pytest.fixture(scope="module")
def host(ldx, G):
    """autohdr_host at the defaults on every fixture image, computed once: name -> uint8 [B][H][W][3]."""
    return {str(n): np.stack([ldx.hdr.autohdr_host(u8) for u8 in G[f"input_{n}"]]) for n in G["cases"]}


@pytest.fixture(scope="module")
def fx(ldx, ldx_lib):
    return ldx.AutoHDR(device=0)


def _p(t, off=0):
    return C.c_void_p(t.data_ptr() + off)


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _pitched(a, pitch, pad_value=0xAB):
    h, w, c = a.shape
    buf = torch.full((h, pitch), pad_value, dtype=torch.uint8)
    buf[:, :w * c] = torch.from_numpy(np.ascontiguousarray(a)).reshape(h, w * c)
    return buf.cuda()


@pytest.mark.parametrize("which", [0, 1])
def test_table_read_is_the_numpy_read(ldx, ldx_lib, G, which):
    table = ldx.hdr.lcms_tables()[which]
    dev_table = torch.from_numpy(np.array(table).view(np.int16)).cuda()
    # the 65 536 colours as one dense 256 x 256 image
    cols = G["colours"].reshape(256, 256, 3)
    src = torch.from_numpy(cols).cuda()
    out = torch.zeros_like(src)
    ldx.lib.check(ldx_lib.ldx_hdr_table(_p(src), 768, 256, 256, _p(dev_table), _p(out), 768, _st()), "ldx_hdr_table")
    assert np.array_equal(out.cpu().numpy(), ldx.hdr.table_read(table, cols))
    # an odd-sized image inside padded rows of different pitches: the padding is neither read nor written
    img = G["input_odd"][0] if which == 0 else G["lab_adj_odd"][0]
    h, w, _ = img.shape
    src, dst = _pitched(img, w * 3 + 7), _pitched(np.zeros_like(img), w * 3 + 19)
    ldx.lib.check(ldx_lib.ldx_hdr_table(_p(src), w * 3 + 7, h, w, _p(dev_table), _p(dst), w * 3 + 19, _st()), "ldx_hdr_table")
    got = dst.cpu().numpy()
    assert np.array_equal(got[:, :w * 3].reshape(h, w, 3), ldx.hdr.table_read(table, img))
    assert (got[:, w * 3:] == 0xAB).all()


def test_apply_is_autohdr_host_on_every_fixture(fx, G, host):
    """fp32 input and byte input, fp32 output and byte output, one instance across all the shapes (the workspace is kept per shape)."""
    for name in G["cases"]:
        u8 = torch.from_numpy(G[f"input_{name}"])
        want = torch.from_numpy(host[str(name)])
        want_f = want.float() / 255                                # on the CPU: the correctly rounded quotient
        got_u8 = fx.apply(u8.cuda(), out_u8=True)
        assert got_u8.dtype == torch.uint8 and torch.equal(got_u8.cpu(), want), name
        got_f = fx.apply(u8.cuda())
        assert got_f.dtype == torch.float32 and torch.equal(got_f.cpu(), want_f), name
        # the fp32 the reference is handed: bytes / 255, which tensor2pil's truncation brings back to the same bytes or to one below
        x = u8.float() / 255
        q = np.clip(np.float32(255.0) * x.numpy(), 0, 255).astype(np.uint8)
        want_q = torch.from_numpy(np.stack([fx_host(im) for im in q]))
        assert torch.equal(fx.apply(x.cuda(), out_u8=True).cpu(), want_q), name
        assert torch.equal(fx.apply(x.cuda()).cpu(), want_q.float() / 255), name


def fx_host(u8, **params):
    import ldx_amd
    return ldx_amd.hdr.autohdr_host(u8, **params)


def test_quantisation_of_fp32_input(fx):
    """Values between the codes, below 0 and above 1: (uint8) trunc(clamp(255.0f * v, 0, 255))."""
    g = torch.Generator().manual_seed(5)
    x = torch.rand((1, 37, 53, 3), generator=g) * 1.3 - 0.15
    q = np.clip(np.float32(255.0) * x.numpy(), 0, 255).astype(np.uint8)
    assert q.min() == 0 and q.max() == 255
    assert np.array_equal(fx.apply(x.cuda(), out_u8=True).cpu().numpy()[0], fx_host(q[0]))


def test_batch_images_get_their_own_mean(fx, G, host):
    u8 = torch.from_numpy(G["input_batch"]).cuda()
    both = fx.apply(u8, out_u8=True)
    for i in range(2):
        alone = fx.apply(u8[i:i + 1], out_u8=True)
        assert torch.equal(both[i:i + 1], alone), i
        assert torch.equal(alone[0].cpu(), torch.from_numpy(host["batch"][i])), i
    assert not torch.equal(both[0], both[1])


@pytest.mark.parametrize("i", range(1, len(PARAM_SETS)))
def test_other_parameter_sets(fx, G, i):
    p = PARAM_SETS[i]
    for name in ("odd", "batch"):
        u8 = G[f"input_{name}"]
        want = torch.from_numpy(np.stack([fx_host(im, **p) for im in u8]))
        dev = torch.from_numpy(u8).cuda()
        assert torch.equal(fx.apply(dev, out_u8=True, **p).cpu(), want), (name, p)
        assert torch.equal(fx.apply((torch.from_numpy(u8).float() / 255 + 0.001).cuda(), **p).cpu(), want.float() / 255), (name, p)      # + 0.001: the codes survive the truncation
    fx.apply(torch.from_numpy(G["input_odd"]).cuda(), out_u8=True)          # the default set again on the same instance
    assert len(fx._luts) >= 2


def test_more_than_the_fixed_number_of_partial_sums(fx):
    """An image of more than 1024 x 256 pixels: every block of the first launch walks more than one pixel per thread, the mean folds 1024 partials."""
    g = np.random.default_rng(11)
    u8 = np.repeat(g.integers(0, 256, (1, 67, 701, 3), dtype=np.uint8), 9, axis=1)[:, :601]          # 601 x 701 = 421 301 pixels
    assert torch.equal(fx.apply(torch.from_numpy(u8).cuda(), out_u8=True).cpu()[0], torch.from_numpy(fx_host(u8[0])))


def test_pitched_bytes_through_the_c_abi(ldx, ldx_lib, fx, G, host):
    """Byte input and byte output with padded rows, two images: the padding is neither read nor written."""
    u8 = G["input_batch"]
    b, h, w, _ = u8.shape
    ip, op = w * 3 + 5, w * 3 + 8
    src = torch.cat([_pitched(im, ip) for im in u8])
    dst = torch.cat([_pitched(np.zeros_like(im), op) for im in u8])
    out_f = torch.zeros((b, h, w, 3), dtype=torch.float32, device="cuda")
    ws = torch.empty(int(ldx_lib.ldx_hdr_workspace_bytes(b, h, w)), dtype=torch.uint8, device="cuda")
    lut = torch.from_numpy(np.array(ldx.hdr.luminance_lut())).cuda()
    ldx.lib.check(ldx_lib.ldx_hdr_apply(None, _p(src), ip, b, h, w, _p(fx._fwd), _p(fx._inv), _p(lut), 1.1, 1.05, _p(ws), _p(dst), op, _p(out_f), _st()),
                  "ldx_hdr_apply")
    got = dst.cpu().numpy().reshape(b, h, op)
    assert np.array_equal(got[:, :, :w * 3].reshape(b, h, w, 3), host["batch"])
    assert (got[:, :, w * 3:] == 0xAB).all()
    assert torch.equal(out_f.cpu(), torch.from_numpy(host["batch"]).float() / 255)


def test_bad_arguments_return_einval(ldx, ldx_lib, fx):
    L = ldx_lib
    u = torch.zeros(64 * 64 * 3, dtype=torch.uint8, device="cuda")
    f = torch.zeros(64 * 64 * 3, dtype=torch.float32, device="cuda")
    ws = torch.zeros(int(L.ldx_hdr_workspace_bytes(1, 8, 8)), dtype=torch.uint8, device="cuda")
    lut = torch.zeros(256, dtype=torch.uint8, device="cuda")
    T, I = _p(fx._fwd), _p(fx._inv)
    calls = [
        lambda: L.ldx_hdr_table(None, 24, 8, 8, T, _p(u, 4096), 24, _st()),
        lambda: L.ldx_hdr_table(_p(u), 23, 8, 8, T, _p(u, 4096), 24, _st()),                                          # pitch < W * 3
        lambda: L.ldx_hdr_table(_p(u), 24, 8, 8, T, _p(u, 4096), 23, _st()),
        lambda: L.ldx_hdr_table(_p(u), 24, 0, 8, T, _p(u, 4096), 24, _st()),
        lambda: L.ldx_hdr_table(_p(u), 24, 8, 8, None, _p(u, 4096), 24, _st()),
        lambda: L.ldx_hdr_table(_p(u), 24, 8, 8, _p(fx._fwd, 2), _p(u, 4096), 24, _st()),                             # table not 8-byte aligned
        lambda: L.ldx_hdr_apply(None, None, 24, 1, 8, 8, T, I, _p(lut), 1.1, 1.05, _p(ws), _p(u), 24, None, _st()),       # no input
        lambda: L.ldx_hdr_apply(_p(f), _p(u, 4096), 24, 1, 8, 8, T, I, _p(lut), 1.1, 1.05, _p(ws), _p(u), 24, None, _st()),   # two inputs
        lambda: L.ldx_hdr_apply(_p(f), None, 0, 1, 8, 8, T, I, _p(lut), 1.1, 1.05, _p(ws), None, 24, None, _st()),        # no output
        lambda: L.ldx_hdr_apply(None, _p(u, 4096), 23, 1, 8, 8, T, I, _p(lut), 1.1, 1.05, _p(ws), _p(u), 24, None, _st()),    # input pitch < W * 3
        lambda: L.ldx_hdr_apply(_p(f), None, 0, 1, 8, 8, T, I, _p(lut), 1.1, 1.05, _p(ws), _p(u), 23, None, _st()),       # output pitch < W * 3
        lambda: L.ldx_hdr_apply(_p(f), None, 0, 0, 8, 8, T, I, _p(lut), 1.1, 1.05, _p(ws), _p(u), 24, None, _st()),       # B = 0
        lambda: L.ldx_hdr_apply(_p(f), None, 0, 1, 8, -8, T, I, _p(lut), 1.1, 1.05, _p(ws), _p(u), 24, None, _st()),
        lambda: L.ldx_hdr_apply(_p(f), None, 0, 1, 4200, 4200, T, I, _p(lut), 1.1, 1.05, _p(ws), _p(u), 12600, None, _st()),  # the grey sum would not fit
        lambda: L.ldx_hdr_apply(_p(f), None, 0, 1, 8, 8, None, I, _p(lut), 1.1, 1.05, _p(ws), _p(u), 24, None, _st()),
        lambda: L.ldx_hdr_apply(_p(f), None, 0, 1, 8, 8, T, I, None, 1.1, 1.05, _p(ws), _p(u), 24, None, _st()),
        lambda: L.ldx_hdr_apply(_p(f), None, 0, 1, 8, 8, T, I, _p(lut), 1.1, 1.05, None, _p(u), 24, None, _st()),
        lambda: L.ldx_hdr_apply(_p(f), None, 0, 1, 8, 8, T, I, _p(lut), float("nan"), 1.05, _p(ws), _p(u), 24, None, _st()),
    ]
    for i, call in enumerate(calls):
        assert call() == -1, i                                 # LDX_EINVAL
        assert b"ldx_hdr_" in L.ldx_last_error()
    assert L.ldx_hdr_workspace_bytes(1, 4200, 4200) == -1 and L.ldx_hdr_workspace_bytes(0, 8, 8) == -1
    assert L.ldx_hdr_workspace_bytes(1, 8, 8) >= 8 * 8 * 3 + 4
    torch.cuda.synchronize()
    assert int(u.sum()) == 0 and float(f.sum()) == 0.0 and int(ws.sum()) == 0         # nothing ran
    with pytest.raises(ValueError):
        fx.apply(torch.zeros((1, 8, 8, 4), device="cuda"))
    with pytest.raises(ValueError):
        fx.apply(torch.zeros((8, 8, 3), device="cuda"))
