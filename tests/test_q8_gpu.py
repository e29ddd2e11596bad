"""Q8_0 GGUF files into the Flux and T5 engines on a real MI355X (csrc/q8.hip, ldx_load_tensor_q8_0, ldx_load_tensor_dev, ldx_packed_digest).

A Q8_0 tensor is exactly an fp16 tensor (fp16_rne(float(d) * q), include/ldx.h), so nothing here has a tolerance: the kernel gives the bits of the reference's
torch expression d.view(float16) * x.view(int8) on the CPU, and an engine loaded from a file, on the host or on the device, holds the packed weights and
computes the outputs of an engine built from the dequantised dense dict through the constructor."""
import ctypes as C
import gc
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gguf_writer as W  # noqa: E402

pytestmark = pytest.mark.gpu

LDX_EINVAL, LDX_ESTATE = -1, -4
F32, F16, Q8, BF16 = W.GGML_F32, W.GGML_F16, W.GGML_Q8_0, W.GGML_BF16
_TORCH = {0: torch.bfloat16, 1: torch.float16, 2: torch.float32}       # LDX_BF16, LDX_F16, LDX_F32


# ---- the kernel on its own ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pairs():
    """Every (scale, value) pair as blocks, and the reference's fp16 result on the CPU."""
    raw = W.all_pairs_blocks()
    return raw, W.torch_q8_0(raw)


def _dequant(lib, dev_blocks_ptr, n, code):
    out = torch.empty(n, device="cuda", dtype=_TORCH[code])
    rc = lib.ldx_op_dequant_q8_0(C.c_void_p(dev_blocks_ptr), n, code, C.c_void_p(out.data_ptr()), None)
    assert rc == 0, lib.ldx_last_error()
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("code", [1, 0, 2])
def test_kernel_on_every_pair(ldx_lib, pairs, code):
    raw, want16 = pairs
    want = want16.to(_TORCH[code])
    dev = raw.cuda()
    n = want.numel()
    assert n == 1 << 24
    W.assert_same_bits(_dequant(ldx_lib, dev.data_ptr(), n, code), want)
    # one block, and a grid with a ragged tail: nothing is written behind n
    for m in (32, 160):
        first = 4096 * 32 * 7                                # small finite scales
        blocks = dev[first // 32 * 34:(first + m) // 32 * 34].clone()
        out = torch.full((m + 64,), 7.0, device="cuda", dtype=_TORCH[code])
        assert ldx_lib.ldx_op_dequant_q8_0(C.c_void_p(blocks.data_ptr()), m, code, C.c_void_p(out.data_ptr()), None) == 0
        torch.cuda.synchronize()
        W.assert_same_bits(out[:m].cpu(), want[first:first + m])
        assert bool((out[m:] == 7.0).all())
    # blocks that start 2 bytes past a 16-byte boundary
    shifted = torch.empty(raw.numel() + 16, device="cuda", dtype=torch.uint8)
    shifted[2:2 + raw.numel()] = dev
    assert shifted.data_ptr() % 16 == 0
    W.assert_same_bits(_dequant(ldx_lib, shifted.data_ptr() + 2, n, code), want)


def test_kernel_refuses_bad_arguments(ldx_lib):
    blocks = torch.zeros(34 * 2 + 16, device="cuda", dtype=torch.uint8)
    out = torch.empty(64, device="cuda", dtype=torch.float16)
    f = ldx_lib.ldx_op_dequant_q8_0
    assert f(C.c_void_p(blocks.data_ptr() + 1), 32, 1, C.c_void_p(out.data_ptr()), None) == LDX_EINVAL and b"ldx_op_dequant_q8_0" in ldx_lib.ldx_last_error()
    assert f(C.c_void_p(blocks.data_ptr()), 48, 1, C.c_void_p(out.data_ptr()), None) == LDX_EINVAL
    assert f(None, 32, 1, C.c_void_p(out.data_ptr()), None) == LDX_EINVAL
    assert f(C.c_void_p(blocks.data_ptr()), 32, 5, C.c_void_p(out.data_ptr()), None) == LDX_EINVAL
    assert f(C.c_void_p(blocks.data_ptr()), 32, 1, C.c_void_p(out.data_ptr() + 2), None) == LDX_EINVAL
    assert f(C.c_void_p(blocks.data_ptr()), 32, 1, C.c_void_p(out.data_ptr()), None) == 0
    torch.cuda.synchronize()


# ---- Flux -----------------------------------------------------------------------------------------------------------------------------------------------
def _write_file(path, sd, types, rename=None, arch="flux", prefix=""):
    rename = rename or (lambda k: k)
    W.write_gguf(path, [(prefix + rename(k), tuple(t.shape), types(k, t), W.raw_of(t, types(k, t))) for k, t in sd.items()], {"general.architecture": (8, arch)})


@pytest.fixture(scope="module")
def flux_file(ldx, tmp_path_factory):
    """Every 2-D weight Q8_0 (K in {32, 64, 128, 256, 512, 640}) but img_in.weight (F16) and txt_in.weight (BF16); every 1-D tensor F32."""
    cfg = ldx.FluxConfig(in_channels=16, vec_in_dim=32, context_in_dim=64, hidden_size=128, num_heads=4, depth=2, depth_single_blocks=2, axes_dim=(8, 12, 12))
    sd = ldx.weights.synth_state_dict(ldx.weights.flux_state_dict_spec(cfg), seed=17, dtype=torch.float32)
    path = str(tmp_path_factory.mktemp("gguf") / "flux.gguf")
    types = lambda k, t: F32 if t.dim() == 1 else F16 if k == "img_in.weight" else BF16 if k == "txt_in.weight" else Q8
    _write_file(path, sd, types, prefix="model.diffusion_model.")
    assert {t.shape[1] for t in sd.values() if t.dim() == 2} == {32, 64, 128, 256, 512, 640}
    g = torch.Generator().manual_seed(5)
    inputs = (torch.randn(1, 16, 16, 24, generator=g), torch.tensor([0.6]), torch.randn(1, 24, 64, generator=g), torch.randn(1, 32, generator=g), torch.tensor([3.5]))
    return cfg, path, inputs


def _strict(cls):
    """An engine class whose ldx_finalize runs only after every raw device tensor the loader has dropped is really gone: the Q8_0 blocks were read when
    ldx_load_tensor_q8_0 returned, so giving their memory back to the driver first must change nothing."""
    class Strict(cls):
        def _finalize(self):
            gc.collect()
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            super()._finalize()
    return Strict


def _three_flux(ldx, cfg, path, dt, fp8=False, host_route=True):
    dense = {k: t.dequantize() for k, t in ldx.gguf.gguf_state_dict(path).items()}
    assert all(t.dtype == (torch.float32 if t.dim() == 1 else torch.bfloat16 if k == "txt_in.weight" else torch.float16) for k, t in dense.items())
    a = ldx.FluxEngine(cfg, dense, device=0, dtype=dt, fp8=fp8)
    b = ldx.FluxEngine.from_gguf(path, cfg, device=0, dtype=dt, fp8=fp8, device_weights=False) if host_route else None
    c = _strict(ldx.FluxEngine).from_gguf(path, cfg, device=0, dtype=dt, fp8=fp8, device_weights=True)
    return a, b, c


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_flux_from_gguf_equals_the_dense_route(ldx, ldx_lib, flux_file, dt):
    cfg, path, inputs = flux_file
    a, b, c = _three_flux(ldx, cfg, path, dt)
    da, db, dc = a.packed_digest(), b.packed_digest(), c.packed_digest()
    print(f"[{dt}] packed digests: dense {da:#x}  host {db:#x}  device {dc:#x}")
    assert da == db == dc
    outs = [e.forward(*(t.cuda() for t in inputs)).cpu() for e in (a, b, c)]
    assert bool(torch.isfinite(outs[0]).all()) and float(outs[0].abs().max()) > 0
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


@pytest.mark.parametrize("fp8", [True, "attn"])
def test_flux_fp8_modes_from_gguf(ldx, ldx_lib, flux_file, fp8):
    """The MX copies are derived from the 16-bit buffers, whichever way those were filled."""
    cfg, path, inputs = flux_file
    a, _, c = _three_flux(ldx, cfg, path, "bf16", fp8=fp8, host_route=False)
    assert a.packed_digest() == c.packed_digest()
    oa, oc = (e.forward(*(t.cuda() for t in inputs)).cpu() for e in (a, c))
    assert bool(torch.isfinite(oa).all()) and torch.equal(oa, oc)


def test_a_dict_of_gguf_tensors_is_accepted(ldx, ldx_lib, flux_file):
    cfg, path, _ = flux_file
    sd = ldx.gguf.gguf_state_dict(path)
    a = ldx.FluxEngine(cfg, {k: t.dequantize() for k, t in sd.items()}, device=0)
    assert ldx.FluxEngine(cfg, sd, device=0).packed_digest() == a.packed_digest()
    assert ldx.FluxEngine(cfg, sd, device=0, device_weights=False).packed_digest() == a.packed_digest()


# ---- T5 -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_t5_from_gguf_equals_the_dense_route(ldx, ldx_lib, tmp_path, dt):
    """The whole file Q8_0 but the norms (F32) and the 32 x 4 relative-attention table, whose rows are no multiple of a block (F16; it stays with the host)."""
    cfg = ldx.T5Config.tiny()
    sd = ldx.weights.synth_state_dict(ldx.weights.t5_state_dict_spec(cfg), seed=23, dtype=torch.float32)
    back = {d: s for s, d in ldx.gguf.T5_KEY_MAP}

    def file_name(k):                                      # the module's name -> llama.cpp's
        k = k.replace("encoder.final_layer_norm", "enc.output_norm").replace("shared", "token_embd").replace("encoder.", "enc.").replace(".block.", ".blk.")
        for d in sorted(back, key=len, reverse=True):
            k = k.replace(d, back[d])
        return k
    path = str(tmp_path / "t5.gguf")
    types = lambda k, t: F32 if t.dim() == 1 else F16 if "relative_attention_bias" in k else Q8
    _write_file(path, sd, types, rename=file_name, arch="t5encoder")
    gsd = ldx.gguf.gguf_t5_state_dict(path, cfg.num_layers)
    assert list(gsd) == list(sd)
    a = ldx.T5Engine(cfg, {k: t.dequantize() for k, t in gsd.items()}, device=0, dtype=dt)
    b = ldx.T5Engine.from_gguf(path, cfg, device=0, dtype=dt, device_weights=False)
    c = _strict(ldx.T5Engine).from_gguf(path, cfg, device=0, dtype=dt, device_weights=True)
    assert a.packed_digest() == b.packed_digest() == c.packed_digest()
    ids = torch.randint(0, cfg.vocab_size, (2, 40), generator=torch.Generator().manual_seed(2))
    oa, ob, oc = (e.forward(ids).cpu() for e in (a, b, c))
    assert bool(torch.isfinite(oa).all()) and float(oa.abs().max()) > 0
    assert torch.equal(oa, ob) and torch.equal(oa, oc)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(ldx, ldx_lib, flux_file):
    L = ldx_lib
    blocks = torch.zeros(34 * 4, dtype=torch.uint8)
    shape = (C.c_int64 * 2)(4, 32)
    vae_cfg = ldx.VAEConfig.tiny()
    vae = ldx.VAEDecoderEngine(vae_cfg, ldx.weights.synth_state_dict(ldx.weights.vae_decoder_state_dict_spec(vae_cfg), seed=1))
    for fn, args in (("ldx_load_tensor_q8_0", (b"w", C.c_void_p(blocks.data_ptr()), shape, 2, 0)),
                     ("ldx_load_tensor_dev", (b"w", C.c_void_p(blocks.data_ptr()), 1, shape, 2))):
        assert getattr(L, fn)(vae._h, *args) == LDX_ESTATE and fn.encode() in L.ldx_last_error()
    # argument checks on an open Flux engine, then the closed loader
    cfg, path, _ = flux_file
    h = C.c_void_p()
    c = ldx.lib.ldx_flux_config()
    c.compute_dtype, c.in_channels, c.vec_in_dim, c.context_in_dim, c.hidden_size, c.mlp_hidden = 0, 16, 32, 64, 128, 512
    c.num_heads, c.depth, c.depth_single, c.guidance_embed = 4, 2, 2, 1
    assert L.ldx_flux_create(C.byref(c), 0, C.byref(h)) == 0
    q8 = lambda ptr, shp, nd, dev=0: L.ldx_load_tensor_q8_0(h, b"w", ptr, shp, nd, dev)
    assert q8(C.c_void_p(blocks.data_ptr()), shape, 0) == LDX_EINVAL
    assert q8(C.c_void_p(blocks.data_ptr()), (C.c_int64 * 2)(4, 48), 2) == LDX_EINVAL and b"multiple of 32" in L.ldx_last_error()
    assert q8(None, shape, 2) == LDX_EINVAL
    assert q8(C.c_void_p(blocks.data_ptr() + 1), shape, 2) == LDX_EINVAL
    assert q8(C.c_void_p(blocks.data_ptr()), shape, 2) == 0
    L.ldx_destroy(h)
    eng = ldx.FluxEngine.from_gguf(path, cfg, device=0)
    assert L.ldx_load_tensor_q8_0(eng._h, b"w", C.c_void_p(blocks.data_ptr()), shape, 2, 0) == LDX_ESTATE and b"ldx_load_tensor_q8_0" in L.ldx_last_error()
    assert L.ldx_load_tensor_dev(eng._h, b"w", C.c_void_p(blocks.data_ptr()), 1, shape, 2) == LDX_ESTATE and b"ldx_load_tensor_dev" in L.ldx_last_error()
    # a tensor of the wrong shape is named at ldx_finalize, as for a dense one
    sd = ldx.gguf.gguf_state_dict(path)
    t = sd["double_blocks.1.img_mlp.0.weight"]
    sd["double_blocks.1.img_mlp.0.weight"] = ldx.gguf.GGUFTensor(t.raw, t.tensor_type, (256, 256))
    for device_weights in (False, True):
        with pytest.raises(ldx.lib.LdxError, match=r"double_blocks\.1\.img_mlp\.0\.weight \(shape mismatch\)"):
            ldx.FluxEngine(cfg, sd, device=0, device_weights=device_weights)


def test_packed_digest_is_the_unet_digest(ldx, ldx_lib):
    cfg = ldx.UNetConfig.tiny(64, 128)
    eng = ldx.UNetEngine(cfg, ldx.weights.synth_state_dict(ldx.weights.unet_state_dict_spec(cfg), seed=1234), device=0)
    assert eng.packed_digest() == eng.weights_digest() != 0
    d = C.c_uint64()
    assert ldx_lib.ldx_packed_digest(None, C.byref(d)) == LDX_EINVAL
