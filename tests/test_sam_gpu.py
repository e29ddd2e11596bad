"""SAM image encoder on the GPU: the kernels of csrc/sam.hip one launch at a time (window partition and its inverse, preprocessing: exact; relative-position
terms and the attention: against fp64), the engine against the outputs of transformers' SamVisionEncoder (tests/golden/sam.npz, tests/tools/capture_sam.py),
batch independence, graph mode, set_image, and one full-size ViT-B encode.

Bounds (tests/golden/sam.META.txt has the figures measured on an MI355X):
  engine      rel-L2 to the golden <= 2 x the rel-L2 of sam_encoder_host16 (the engine's number formats on the CPU) in the same type, per case
  attention   rel-L2 to the fp64 statement on the same 16-bit inputs <= 2 x that of the fp32 statement whose probabilities are rounded to the 16-bit type (its
              output stays fp32; the kernel's 16-bit output has to fit under the same bound, and does: META)
  rel-pos     rel-L2 to fp64 <= 2 x that of the fp32 statement summing the 64 products in ascending order, as the kernel does"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import capture_sam as CS  # noqa: E402

pytestmark = pytest.mark.gpu
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
CODE = {"bf16": 0, "f16": 1}


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "sam.npz"))


# ---- window partition -------------------------------------------------------------------------------------------------------------------------
def _partition(x, win):
    B, S, _, C = x.shape
    nw = -(-S // win)
    g = torch.nn.functional.pad(x, (0, 0, 0, nw * win - S, 0, nw * win - S))
    return g.view(B, nw, win, nw, win, C).permute(0, 1, 3, 2, 4, 5).reshape(B * nw * nw * win * win, C), nw


@pytest.mark.parametrize("S,win", [(8, 3), (20, 14)])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_window_gather_and_scatter_exact(ldx, ldx_lib, S, win, dt):
    lib, B, Cc = ldx.lib, 2, 136
    g = torch.Generator().manual_seed(S)
    x = torch.randn(B, S, S, Cc, generator=g).to(DTYPES[dt])
    want, nw = _partition(x, win)
    xd = x.cuda()
    got = torch.full((B * nw * nw * win * win, Cc), 7.0, dtype=DTYPES[dt], device="cuda")
    lib.check(ldx_lib.ldx_op_sam_window(lib.ptr(xd), lib.ptr(got), None, B, S, win, Cc, 0, CODE[dt], lib.current_stream_ptr()), "ldx_op_sam_window")
    assert torch.equal(got.cpu(), want)
    # the inverse crops; with a residual the sum is taken in fp32 and rounded once; in place on the residual's buffer
    w = torch.randn(B * nw * nw * win * win, Cc, generator=g).to(DTYPES[dt])
    back = w.view(B, nw, nw, win, win, Cc).permute(0, 1, 3, 2, 4, 5).reshape(B, nw * win, nw * win, Cc)[:, :S, :S].contiguous()
    wd, out = w.cuda(), torch.empty(B, S, S, Cc, dtype=DTYPES[dt], device="cuda")
    lib.check(ldx_lib.ldx_op_sam_window(lib.ptr(wd), lib.ptr(out), None, B, S, win, Cc, 1, CODE[dt], lib.current_stream_ptr()), "ldx_op_sam_window")
    assert torch.equal(out.cpu(), back)
    res = xd.clone()
    lib.check(ldx_lib.ldx_op_sam_window(lib.ptr(wd), lib.ptr(res), lib.ptr(res), B, S, win, Cc, 1, CODE[dt], lib.current_stream_ptr()), "ldx_op_sam_window")
    assert torch.equal(res.cpu(), (x.float() + back.float()).to(DTYPES[dt]))


# ---- preprocessing ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,size", [(37, 64, 64), (1024, 1024, 1024)])
def test_preprocess_exact(ldx, ldx_lib, h, w, size):
    lib = ldx.lib
    g = torch.Generator().manual_seed(h)
    img = torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8)
    pitch = w * 3 + 5
    buf = torch.zeros(h, pitch, dtype=torch.uint8)
    buf[:, :w * 3] = img.view(h, w * 3)
    bd = buf.cuda()
    out = torch.full((3, size, size), 9.0, device="cuda")
    lib.check(ldx_lib.ldx_sam_preprocess(lib.ptr(bd), pitch, h, w, lib.ptr(out), size, lib.current_stream_ptr()), "ldx_sam_preprocess")
    assert torch.equal(out.cpu(), ldx.sam.preprocess_host(img, size))


# ---- rel-pos terms and attention, one launch each -------------------------------------------------------------------------------------------------
SHAPES = [(3, 4, 2), (14, 4, 2), (20, 1, 2), (64, 1, 2)]          # (n, BW, H): batch x heads = 8, 8, 2, 2


def _attn_inputs(n, BW, H, dt, big):
    g = torch.Generator().manual_seed(n * 10 + (dt == "f16"))
    N = n * n
    qkv = torch.randn(BW, N, 3, H, 64, generator=g)
    if big:
        qkv[:, :, 0] *= 6.0          # scores of standard deviation ~6 whose running maximum keeps rising over the 64 key blocks: the rescale of the online softmax runs
    qkv = qkv.to(DTYPES[dt])
    th, tw = 0.25 * torch.randn(2 * n - 1, 64, generator=g), 0.25 * torch.randn(2 * n - 1, 64, generator=g)
    return qkv, th, tw


def _relpos(q, th, tw, n, dtype):
    """q [BW][H][N][64] -> [BW][H][N][2 n] in `dtype`, the 64 products summed in ascending order"""
    BW, H, N, _ = q.shape
    idx = torch.arange(n)[:, None] - torch.arange(n)[None, :] + (n - 1)
    qq = q.to(dtype).reshape(BW, H, n, n, 64)
    rh, rw = th.to(dtype)[idx], tw.to(dtype)[idx]          # [n][n][64]
    if dtype == torch.float64:                             # the reference: the order of an fp64 sum does not show at the fp32 bound
        return torch.cat([torch.einsum("bhxyc,xkc->bhxyk", qq, rh), torch.einsum("bhxyc,ykc->bhxyk", qq, rw)], dim=-1).reshape(BW, H, N, 2 * n)
    acc_h, acc_w = torch.zeros(BW, H, n, n, n, dtype=dtype), torch.zeros(BW, H, n, n, n, dtype=dtype)
    for c in range(64):
        acc_h = acc_h + qq[..., c][..., None] * rh[None, None, :, None, :, c]
        acc_w = acc_w + qq[..., c][..., None] * rw[None, None, None, :, :, c]
    return torch.cat([acc_h, acc_w], dim=-1).reshape(BW, H, N, 2 * n)


def _attention(qkv, relv, n, dtype, store=None):
    """softmax(0.125 q.k + rel_h[q][k_h] + rel_w[q][k_w]) v in `dtype`; store: the 16-bit type P is rounded to (None: not rounded)"""
    BW, N, _, H, _ = qkv.shape
    q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3).to(dtype) for i in range(3))
    r = relv.to(dtype)
    bias = (r[..., :n, None] + r[..., None, n:]).reshape(BW, H, N, N)
    p = torch.softmax(0.125 * (q @ k.transpose(-1, -2)) + bias, dim=-1)
    if store is not None:
        p = p.to(store).to(dtype)
    return (p @ v).permute(0, 2, 1, 3).reshape(BW * N, H * 64)


@pytest.mark.parametrize("n,BW,H", SHAPES)
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_relpos_and_attention_single_launch_vs_fp64(ldx, ldx_lib, n, BW, H, dt):
    lib, N = ldx.lib, n * n
    qkv, th, tw = _attn_inputs(n, BW, H, dt, big=(n == 64))
    q = qkv[:, :, 0].permute(0, 2, 1, 3)
    rel64 = _relpos(q, th, tw, n, torch.float64)
    rel_bound = 2 * rel(_relpos(q, th, tw, n, torch.float32), rel64)
    qd, thd, twd = qkv.cuda(), th.cuda(), tw.cuda()
    reld = torch.full((BW * H, N, 2 * n), float("nan"), device="cuda")
    ld = 3 * H * 64
    lib.check(ldx_lib.ldx_op_sam_relpos(lib.ptr(qd), ld, lib.ptr(thd), lib.ptr(twd), lib.ptr(reld), BW, H, n, CODE[dt], lib.current_stream_ptr()), "ldx_op_sam_relpos")
    got_rel = reld.cpu().view(BW, H, N, 2 * n)
    d_rel = rel(got_rel, rel64)
    print(f"relpos n {n} BWxH {BW * H} {dt}: rel-L2 {d_rel:.3e} (bound {rel_bound:.3e})")
    # the attention reads the fp32 terms the kernel above wrote: both statements get those very values
    ref = _attention(qkv, got_rel, n, torch.float64)
    att_bound = 2 * rel(_attention(qkv, got_rel, n, torch.float32, DTYPES[dt]), ref)
    out = torch.full((BW * N, H * 64), float("nan"), dtype=DTYPES[dt], device="cuda")
    base = qd.data_ptr()
    import ctypes as C
    lib.check(ldx_lib.ldx_op_sam_attention(C.c_void_p(base), C.c_void_p(base + H * 64 * 2), C.c_void_p(base + 2 * H * 64 * 2), ld, lib.ptr(reld), lib.ptr(out), H * 64,
                                           BW, H, n, 0.125, CODE[dt], lib.current_stream_ptr()), "ldx_op_sam_attention")
    got = out.cpu()
    d_att = rel(got, ref)
    print(f"attention n {n} N {N} BWxH {BW * H} {dt}: rel-L2 {d_att:.3e} (bound {att_bound:.3e})")
    assert torch.isfinite(got.float()).all()
    assert d_rel <= rel_bound
    assert d_att <= att_bound


# ---- the engine ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixtures():
    return {case: (CS.cases()[case][0], CS.fixture_weights(case), CS.fixture_input(case)) for case in ("T", "M", "W")}


@pytest.mark.parametrize("case", ["T", "M", "W"])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_engine_matches_the_reference_encoder(ldx, ldx_lib, golden, fixtures, case, dt):
    cfg, sd, x = fixtures[case]
    ref = torch.from_numpy(golden[f"{case}.out"])
    bound = 2 * rel(ldx.sam.sam_encoder_host16(sd, x, DTYPES[dt]), ref)
    eng = ldx.SAMImageEncoderEngine(cfg, sd, device=0, dtype=dt)
    out = eng.encode(x.cuda()).cpu()
    d = rel(out, ref)
    print(f"engine case {case} {dt}: rel-L2 to SamVisionEncoder = {d:.3e} (bound {bound:.3e}); launches {eng.plan_info()['launches']}")
    assert out.shape == ref.shape and out.dtype == torch.float32 and torch.isfinite(out).all()
    assert d <= bound


def test_batch_of_two_equals_two_single_calls(ldx, ldx_lib, fixtures):
    cfg, sd, x = fixtures["T"]
    eng = ldx.SAMImageEncoderEngine(cfg, sd, device=0, dtype="bf16")
    xd = x.cuda()
    both = eng.encode(xd).cpu()
    one = torch.cat([eng.encode(xd[i:i + 1]).cpu() for i in range(2)])
    assert torch.equal(both, one)


def test_graph_replay_equals_eager(ldx, ldx_lib, fixtures):
    cfg, sd, x = fixtures["T"]
    eager = ldx.SAMImageEncoderEngine(cfg, sd, device=0, dtype="bf16").encode(x.cuda()).cpu()
    eng = ldx.SAMImageEncoderEngine(cfg, sd, device=0, dtype="bf16", graph=True)
    outs = [eng.encode(x.cuda()).cpu() for _ in range(4)]          # eager, capture, replay, replay
    captures, replays = eng.graph_stats()
    assert (captures, replays) == (1, 2)
    assert all(torch.equal(o, eager) for o in outs)
    other = eng.encode((x * 0.5).cuda()).cpu()                      # the static input buffer is refilled: a replay, on new data
    assert eng.graph_stats() == (1, 3) and not torch.equal(other, eager)


def test_set_image_equals_the_host_chain(ldx, ldx_lib, fixtures):
    """48 x 80 fp32 image -> truncating quantisation -> Pillow's BILINEAR to 77 x 128 -> Sam.preprocess -> encoder, against the same chain on the host in front
    of the same engine; the uint8 entry skips the quantisation."""
    cfg, sd, _ = fixtures["T"]
    eng = ldx.SAMImageEncoderEngine(cfg, sd, device=0, dtype="bf16")
    g = torch.Generator().manual_seed(5)
    img = torch.rand(1, 48, 80, 3, generator=g) * 1.2 - 0.1
    q = ldx.detailer.quantize_host(img[0].numpy())
    assert ldx.sam.preprocess_shape(48, 80, cfg.image_size) == (77, 128)
    x = ldx.sam.preprocess_host(ldx.detailer.resize_host(q, 128, 77, ldx.usdu.BILINEAR), cfg.image_size)
    assert torch.equal(eng.preprocess(img.cuda()).cpu()[0], x)
    want = eng.encode(x[None].cuda()).cpu()
    assert torch.equal(eng.set_image(img.cuda()).cpu(), want)
    assert torch.equal(eng.set_image(img[0].cuda()).cpu(), want)
    assert torch.equal(eng.set_image(torch.from_numpy(q)[None].cuda()).cpu(), want)


def test_vit_b_full_size_encode(ldx, ldx_lib):
    cfg = ldx.SAMConfig.vit_b()
    eng = ldx.SAMImageEncoderEngine(cfg, ldx.weights.sam_synth_state_dict(cfg, seed=11), device=0, dtype="bf16")
    g = torch.Generator().manual_seed(11)
    x = torch.randn(1, 3, 1024, 1024, generator=g)
    x[:, :, 768:] = 0.0
    out = eng.encode(x.cuda())
    torch.cuda.synchronize()
    assert tuple(out.shape) == (1, 256, 64, 64) and out.dtype == torch.float32 and bool(torch.isfinite(out).all())
    rms = float(out.pow(2).mean().sqrt())
    print(f"ViT-B 1024^2: output rms {rms:.4f}, launches {eng.plan_info()['launches']}, flops {eng.plan_info()['flops']:.4e}")
    assert 0.5 < rms < 2.0          # the output ends in a LayerNorm whose gains are 1 +- 0.1
