"""The GGUF container reader (lightdiffusion-next_amd/gguf.py; reference: Quantize/Quantizer.py:94-112, 427-452, 581-665, 815-856).  The `gguf` package
is not available here, so the reader is held to files written from the published v2 / v3 layout by tests/_gguf_writer.py, and the Q8_0 arithmetic to the
reference's own torch expression on every (scale, value) pair there is.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gguf_writer as W  # noqa: E402

F32, F16, Q8, BF16 = W.GGML_F32, W.GGML_F16, W.GGML_Q8_0, W.GGML_BF16


def _tensors(seed=3):
    g = torch.Generator().manual_seed(seed)
    return {"blk.weight": (torch.randn(48, 64, generator=g) * 0.05, Q8), "blk.bias": (torch.randn(48, generator=g), F32),
            "norm.scale": (torch.randn(64, generator=g), F16), "emb.weight": (torch.randn(8, 32, generator=g), BF16)}


@pytest.mark.parametrize("version,align", [(2, None), (3, None), (2, 64), (3, 64)])
def test_round_trip(ldx, tmp_path, version, align):
    """F32, F16, BF16 and Q8_0 tensors come back with their type, their torch shape and their bytes; the alignment is the file's (default 32)."""
    G = ldx.gguf
    src = _tensors()
    path = str(tmp_path / "m.gguf")
    # metadata of every value type in front of the tensors: the reader has to walk over all of them
    meta = {"general.architecture": (8, "flux"), "a.u8": (0, 7), "a.i8": (1, -7), "a.u16": (2, 700), "a.i16": (3, -700), "a.u32": (4, 70000), "a.i32": (5, -70000),
            "a.f32": (6, 0.5), "a.bool": (7, True), "a.str": (8, "héllo"), "a.arr": ((9, 8), ["x", "yz"]), "a.u64": (10, 1 << 40), "a.i64": (11, -(1 << 40)),
            "a.f64": (12, 0.25), "a.empty": ((9, 5), [])}
    W.write_gguf(path, [(k, tuple(t.shape), typ, W.raw_of(t, typ)) for k, (t, typ) in src.items()], meta, version=version, align=align)
    m, _ = G.read_gguf(path)
    assert m["a.str"] == ("héllo", (8,)) and m["a.arr"] == (["x", "yz"], (9, 8)) and m["a.i64"][0] == -(1 << 40) and m["a.empty"] == ([], (9, 5))
    assert m["a.f64"][0] == 0.25 and m["a.bool"][0] is True and m["a.i16"][0] == -700
    sd = G.gguf_state_dict(path)
    assert list(sd) == list(src)
    for k, (t, typ) in src.items():
        x = sd[k]
        assert x.tensor_type == typ and tuple(x.tensor_shape) == tuple(t.shape) and x.raw.dtype == torch.uint8
        assert bytes(x.raw.numpy().tobytes()) == W.raw_of(t, typ), k
        assert x.raw.numpy().ctypes.data % (align or 32) == 0        # every tensor starts on the file's alignment (the mapping is page aligned)
    assert sd["blk.bias"].dequantize().dtype == torch.float32 and torch.equal(sd["blk.bias"].dequantize(), src["blk.bias"][0])
    assert torch.equal(sd["norm.scale"].dequantize(), src["norm.scale"][0].half())
    assert torch.equal(sd["emb.weight"].dequantize(), src["emb.weight"][0].bfloat16())
    w = sd["blk.weight"].dequantize()
    assert w.dtype == torch.float16 and w.shape == (48, 64)
    assert torch.equal(w.reshape(-1), W.torch_q8_0(torch.frombuffer(bytearray(W.q8_0(src["blk.weight"][0])), dtype=torch.uint8)))
    assert float((w.float() - src["blk.weight"][0]).abs().max()) <= float(src["blk.weight"][0].abs().max()) / 127 * 0.51 + 1e-4      # and it is the weight, to Q8_0 accuracy


def test_prefix_is_stripped_only_where_some_tensor_has_it(ldx, tmp_path):
    G = ldx.gguf
    z = np.zeros(32, np.float32).tobytes()
    p = str(tmp_path / "p.gguf")
    W.write_gguf(p, [("model.diffusion_model.a.weight", (32,), F32, z), ("first_stage_model.b", (32,), F32, z), ("model.diffusion_model.c", (32,), F32, z)], {})
    assert list(G.gguf_state_dict(p)) == ["a.weight", "c"]                      # stripped, the un-prefixed tensor dropped
    assert list(G.gguf_state_dict(p, handle_prefix=None)) == ["model.diffusion_model.a.weight", "first_stage_model.b", "model.diffusion_model.c"]
    W.write_gguf(p, [("a.weight", (32,), F32, z), ("first_stage_model.b", (32,), F32, z)], {})
    assert list(G.gguf_state_dict(p)) == ["a.weight", "first_stage_model.b"]      # no tensor carries it: every key kept


def test_orig_shape_overrides_and_must_be_int32(ldx, tmp_path):
    G = ldx.gguf
    conv = torch.arange(8 * 4 * 3 * 3, dtype=torch.float16)
    p = str(tmp_path / "o.gguf")
    key = "comfy.gguf.orig_shape.model.diffusion_model.conv.weight"
    tensors = [("model.diffusion_model.conv.weight", (72, 4), F16, W.raw_of(conv, F16))]      # stored flattened
    W.write_gguf(p, tensors, {key: ((9, 5), [8, 4, 3, 3])})
    t = G.gguf_state_dict(p)["conv.weight"]
    assert tuple(t.tensor_shape) == (8, 4, 3, 3) and torch.equal(t.dequantize(), conv.reshape(8, 4, 3, 3))
    for bad in (((9, 4), [8, 4, 3, 3]), ((9, 11), [8, 4, 3, 3]), (5, 288), (8, "8,4,3,3")):
        W.write_gguf(p, tensors, {key: bad})
        with pytest.raises(TypeError, match="orig_shape"):
            G.gguf_state_dict(p)


def test_architecture_is_checked(ldx, tmp_path):
    G = ldx.gguf
    p = str(tmp_path / "a.gguf")
    t = [("w", (2, 32), F16, np.arange(64, dtype=np.float16).tobytes())]
    for arch in ("flux", "sd1", "sdxl", "t5", "t5encoder"):
        W.write_gguf(p, t, {"general.architecture": (8, arch)})
        assert list(G.gguf_state_dict(p)) == ["w"]
    W.write_gguf(p, t, {"general.architecture": (8, "llama")})
    with pytest.raises(ValueError, match="architecture"):
        G.gguf_state_dict(p)
    W.write_gguf(p, t, {"general.architecture": (4, 3)})
    with pytest.raises(TypeError, match="architecture"):
        G.gguf_state_dict(p)
    W.write_gguf(p, t, {})                                                       # no architecture key: nothing to check
    assert float(G.gguf_state_dict(p)["w"].dequantize()[1, 31]) == 63.0


def test_unknown_types_and_bad_files(ldx, tmp_path):
    G = ldx.gguf
    p = str(tmp_path / "b.gguf")
    W.write_gguf(p, [("blk.k_quant", (256,), 12, b"\0" * 144)], {})              # a K-quant: the reference has no dequantiser for it either
    with pytest.raises(NotImplementedError, match=r"blk\.k_quant.*12"):
        G.gguf_state_dict(p)
    W.write_gguf(p, [("w", (2, 48), Q8, b"\0" * 102)], {})
    with pytest.raises(ValueError, match="multiple of 32"):
        G.gguf_state_dict(p)
    W.write_gguf(p, [("w", (4, 32), Q8, b"\0" * 136)], {"comfy.gguf.orig_shape.w": ((9, 5), [8, 16])})      # reshaped so that blocks would straddle rows
    with pytest.raises(ValueError, match="multiple of 32"):
        G.gguf_state_dict(p)
    with pytest.raises(ValueError, match="bytes"):
        G.GGUFTensor(torch.zeros(100, dtype=torch.uint8), Q8, (4, 32))          # 4 blocks are 136 bytes
    W.write_gguf(p, [("w", (2, 32), F32, np.zeros(64, np.float32).tobytes())], {}, version=4)
    with pytest.raises(ValueError, match="version"):
        G.gguf_state_dict(p)
    with open(p, "wb") as f:
        f.write(b"NOPE" + b"\0" * 64)
    with pytest.raises(ValueError, match="not a GGUF"):
        G.gguf_state_dict(p)


def test_truncated_file(ldx, tmp_path):
    G = ldx.gguf
    p = str(tmp_path / "t.gguf")
    t = [("a", (4, 32), Q8, b"\1" * 136), ("b", (64,), F32, np.ones(64, np.float32).tobytes())]
    W.write_gguf(p, t, {"general.architecture": (8, "flux")}, cut=8)               # the last tensor's data is short
    with pytest.raises(ValueError, match="truncated"):
        G.gguf_state_dict(p)
    W.write_gguf(p, t, {"general.architecture": (8, "flux")})
    whole = open(p, "rb").read()
    for n in (30, 50, 90):                                                         # inside the metadata, a tensor's name, its dims
        with open(p, "wb") as f:
            f.write(whole[:n])
        with pytest.raises(ValueError, match="truncated"):
            G.gguf_state_dict(p)


def _t5_file_names(cfg):
    names = []
    for l in range(cfg.num_layers):
        names += [f"enc.blk.{l}.attn_q.weight", f"enc.blk.{l}.attn_k.weight", f"enc.blk.{l}.attn_v.weight", f"enc.blk.{l}.attn_o.weight"]
        if l == 0:
            names += ["enc.blk.0.attn_rel_b.weight"]
        names += [f"enc.blk.{l}.attn_norm.weight", f"enc.blk.{l}.ffn_gate.weight", f"enc.blk.{l}.ffn_up.weight", f"enc.blk.{l}.ffn_down.weight",
                  f"enc.blk.{l}.ffn_norm.weight"]
    return names + ["enc.output_norm.weight", "token_embd.weight"]


def test_t5_renaming_gives_the_module_keys(ldx, tmp_path):
    """llama.cpp's names of a T5 encoder, in module order, land on exactly the keys (and shapes) of weights.t5_state_dict_spec."""
    G = ldx.gguf
    cfg = ldx.T5Config.tiny()
    spec = ldx.weights.t5_state_dict_spec(cfg)
    names = _t5_file_names(cfg)
    assert len(names) == len(spec)
    p = str(tmp_path / "t5.gguf")
    W.write_gguf(p, [(n, shp, F16, b"\0" * (2 * int(np.prod(shp)))) for n, (_, shp) in zip(names, spec)], {"general.architecture": (8, "t5encoder")})
    sd = G.gguf_t5_state_dict(p, cfg.num_layers)
    assert [(k, tuple(v.tensor_shape)) for k, v in sd.items()] == [(k, tuple(s)) for k, s in spec]
    with pytest.raises(AssertionError):                                            # the reference's check: T5-XXL's last block has to be there
        G.gguf_t5_state_dict(p)


def test_q8_0_rule_on_every_pair(ldx):
    """GGUFTensor.dequantize() on all 2^24 (fp16 scale, int8 value) pairs against the reference's torch expression: bit-equal where that is no NaN, NaN in the
    same places, and the same after the engine's second rounding .to(bfloat16)."""
    raw = W.all_pairs_blocks()
    assert raw.numel() == 524288 * 34
    # the pairs are all there: scale pattern b // 8, value bytes (b % 8) * 32 + j
    blocks = raw.reshape(-1, 34)
    assert int(blocks[8 * 0x3c00 + 3, 0]) == 0x00 and int(blocks[8 * 0x3c00 + 3, 1]) == 0x3c and int(blocks[8 * 0x3c00 + 3, 2 + 5]) == 3 * 32 + 5
    got = ldx.gguf.GGUFTensor(raw, Q8, (524288, 32)).dequantize()
    d = blocks[:, :2].contiguous().view(torch.float16)
    x = blocks[:, 2:].contiguous().view(torch.int8)
    want = d * x                                                                   # Quantizer.py:94-112 with dequant_dtype None
    assert got.dtype == torch.float16 and want.dtype == torch.float16 and got.shape == want.shape
    W.assert_same_bits(got, want)
    W.assert_same_bits(got.to(torch.bfloat16), want.to(torch.bfloat16))
    # ... and the rule as the engines compute it, one rounding of the exact fp32 product (include/ldx.h ldx_load_tensor_q8_0)
    W.assert_same_bits((d.float() * x.float()).half(), want)
    n_nan = int(torch.isnan(want).sum())
    print("NaN results:", n_nan, " inf:", int(torch.isinf(want).sum()), " -0:", int(((want == 0) & torch.signbit(want)).sum()))
    assert n_nan == 523778
