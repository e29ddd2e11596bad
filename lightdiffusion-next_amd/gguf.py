"""GGUF checkpoints (F32 / F16 / BF16 / Q8_0): the container reader in front of FluxEngine.from_gguf and T5Engine.from_gguf.

The reference's Flux mode ships `flux1-dev-Q8_0.gguf` and `t5-v1_1-xxl-encoder-Q8_0.gguf` (pipeline.py:218-236).  `gguf_sd_loader`
(Quantize/Quantizer.py:581-665) reads a file with the `gguf` package into {key: GGMLTensor}: the raw bytes, the ggml type and the torch shape;
`dequantize_blocks_Q8_0` (:94-112) expands a tensor when a layer runs.  Here the file is read the same way, {key: GGUFTensor}, nothing is expanded, and
the engines expand each Q8_0 tensor ONCE at load time: on the device (csrc/q8.hip) or on the host (csrc/weight_convert.h).

The rule.  A Q8_0 block is 34 bytes: an fp16 scale d and 32 int8 values q along the innermost axis.  With the reference's default dequant_dtype=None the
weight is `d.view(float16) * q.view(int8)`, which torch computes in fp16: fp16_rne(float(d) * q), ONE rounding of a product that is exact in fp32 (11 x 8
significant bits).  A Q8_0 tensor is therefore exactly an fp16 tensor, and GGUFTensor.dequantize() returns that tensor.

The `gguf` package is not available where this project is built and tested, so the reader is held to files written from the published GGUF v2 / v3
layout by the tests' own writer (tests/test_gguf_cpu.py), not to the reference's reader.  Pure host code (numpy + torch on the CPU).
"""
from __future__ import annotations

import struct
import warnings
from typing import Dict, Optional

import numpy as np
import torch

GGUF_MAGIC = 0x46554747            # b"GGUF" little endian
GGML_F32, GGML_F16, GGML_Q8_0, GGML_BF16 = 0, 1, 8, 30
Q8_0_BLOCK, Q8_0_BYTES = 32, 34
ORIG_SHAPE = "comfy.gguf.orig_shape."
# metadata value types 0..12: u8 i8 u16 i16 u32 i32 f32 bool string array u64 i64 f64
T_INT32, T_STRING, T_ARRAY = 5, 8, 9
_SCALARS = {0: "<B", 1: "<b", 2: "<H", 3: "<h", 4: "<I", 5: "<i", 6: "<f", 7: "<?", 10: "<Q", 11: "<q", 12: "<d"}
ARCHITECTURES = ("flux", "sd1", "sdxl", "t5", "t5encoder")       # Quantizer.py:622
_TORCH = {GGML_F32: torch.float32, GGML_F16: torch.float16, GGML_BF16: torch.bfloat16}
# llama.cpp's T5 encoder names -> the torch module names, applied as substring replacements IN THIS ORDER (Quantizer.py:815-856)
T5_KEY_MAP = (("enc.", "encoder."), (".blk.", ".block."), ("token_embd", "shared"), ("output_norm", "final_layer_norm"),
              ("attn_q", "layer.0.SelfAttention.q"), ("attn_k", "layer.0.SelfAttention.k"), ("attn_v", "layer.0.SelfAttention.v"),
              ("attn_o", "layer.0.SelfAttention.o"), ("attn_norm", "layer.0.layer_norm"),
              ("attn_rel_b", "layer.0.SelfAttention.relative_attention_bias"), ("ffn_up", "layer.1.DenseReluDense.wi_1"),
              ("ffn_down", "layer.1.DenseReluDense.wo"), ("ffn_gate", "layer.1.DenseReluDense.wi_0"), ("ffn_norm", "layer.1.layer_norm"))


class _Reader:
    def __init__(self, buf, path):
        self.b, self.o, self.path = buf, 0, path

    def take(self, fmt: str):
        n = struct.calcsize(fmt)
        if self.o + n > len(self.b):
            raise ValueError(f"{self.path}: truncated GGUF file (header runs past the end at byte {self.o})")
        v = struct.unpack_from(fmt, self.b, self.o)[0]
        self.o += n
        return v

    def string(self) -> str:
        n = self.take("<Q")
        if self.o + n > len(self.b):
            raise ValueError(f"{self.path}: truncated GGUF file (string runs past the end at byte {self.o})")
        s = bytes(self.b[self.o:self.o + n]).decode("utf-8")
        self.o += n
        return s

    def value(self, t: int):
        """(value, types): types as the `gguf` package lists them, (t,) for a scalar or a string, (9, element type) for an array."""
        if t in _SCALARS:
            return self.take(_SCALARS[t]), (t,)
        if t == T_STRING:
            return self.string(), (t,)
        if t == T_ARRAY:
            et, n = self.take("<I"), self.take("<Q")
            if n > len(self.b):
                raise ValueError(f"{self.path}: truncated GGUF file (array of {n} elements)")
            vals, types = [], (T_ARRAY, et)
            for _ in range(n):
                v, sub = self.value(et)
                vals.append(v)
                types = (T_ARRAY,) + sub
            return vals, types
        raise ValueError(f"{self.path}: unknown GGUF metadata value type {t}")


class GGUFTensor:
    """One tensor of a file as it lies there (the reference's GGMLTensor): `raw`, a uint8 torch view of the mapping; `tensor_type`, the ggml type;
    `tensor_shape`, the torch shape.  Nothing is copied or expanded until dequantize()."""

    def __init__(self, raw: torch.Tensor, tensor_type: int, tensor_shape, name: str = "?"):
        self.raw, self.tensor_type, self.tensor_shape, self.name = raw, int(tensor_type), torch.Size(tensor_shape), name
        n = self.numel()
        if self.tensor_type == GGML_Q8_0:
            if len(self.tensor_shape) == 0 or self.tensor_shape[-1] % Q8_0_BLOCK:
                raise ValueError(f"{name}: Q8_0 needs an innermost extent that is a multiple of 32, got shape {tuple(self.tensor_shape)}")
            want = n // Q8_0_BLOCK * Q8_0_BYTES
        elif self.tensor_type in _TORCH:
            want = n * (4 if self.tensor_type == GGML_F32 else 2)
        else:
            raise NotImplementedError(f"{name}: ggml tensor type {self.tensor_type} (F32 = 0, F16 = 1, Q8_0 = 8 and BF16 = 30 are supported)")
        if raw.dtype != torch.uint8 or raw.numel() != want:
            raise ValueError(f"{name}: {raw.numel()} bytes for shape {tuple(self.tensor_shape)} of ggml type {self.tensor_type}, expected {want}")

    def numel(self) -> int:
        n = 1
        for d in self.tensor_shape:
            n *= int(d)
        return n

    @property
    def is_quantized(self) -> bool:
        return self.tensor_type == GGML_Q8_0

    def dequantize(self) -> torch.Tensor:
        """The dense tensor: Q8_0 -> fp16 by the reference's expression (module docstring); F16, BF16 and F32 as they are (a copy off the mapping)."""
        raw = self.raw.clone()
        if self.tensor_type == GGML_Q8_0:
            blocks = raw.reshape(-1, Q8_0_BYTES)
            d = blocks[:, :2].contiguous().view(torch.float16)
            q = blocks[:, 2:].contiguous().view(torch.int8)
            return (d * q).reshape(self.tensor_shape)
        return raw.view(_TORCH[self.tensor_type]).reshape(self.tensor_shape)


def read_gguf(path: str):
    """(metadata, tensors) of a GGUF v2 / v3 file.  metadata[key] = (value, types); tensors[name] = (GGUF dims innermost first, ggml type, raw uint8
    numpy view of the memory-mapped file)."""
    mm = np.memmap(path, dtype=np.uint8, mode="r")
    r = _Reader(memoryview(mm), path)
    if len(mm) < 4 or r.take("<I") != GGUF_MAGIC:
        raise ValueError(f"{path}: not a GGUF file")
    ver = r.take("<I")
    if ver not in (2, 3):
        raise ValueError(f"{path}: GGUF version {ver} (2 and 3 are supported)")
    n_t, n_kv = r.take("<Q"), r.take("<Q")
    meta = {}
    for _ in range(n_kv):
        k = r.string()
        meta[k] = r.value(r.take("<I"))
    infos = []
    for _ in range(n_t):
        name = r.string()
        nd = r.take("<I")
        dims = tuple(r.take("<Q") for _ in range(nd))
        infos.append((name, dims, r.take("<I"), r.take("<Q")))
    align = int(meta["general.alignment"][0]) if "general.alignment" in meta else 32
    base = (r.o + align - 1) // align * align
    tensors = {}
    for name, dims, typ, off in infos:
        n = 1
        for d in dims:
            n *= d
        if typ == GGML_F32:
            nb = 4 * n
        elif typ in (GGML_F16, GGML_BF16):
            nb = 2 * n
        elif typ == GGML_Q8_0:
            if not dims or dims[0] % Q8_0_BLOCK:
                raise ValueError(f"{path}: {name}: Q8_0 needs an innermost extent that is a multiple of 32, got GGUF dims {dims}")
            nb = n // Q8_0_BLOCK * Q8_0_BYTES
        else:
            raise NotImplementedError(f"{path}: {name}: ggml tensor type {typ} (F32 = 0, F16 = 1, Q8_0 = 8 and BF16 = 30 are supported)")
        if base + off + nb > mm.size:
            raise ValueError(f"{path}: {name}: truncated GGUF file (tensor data runs past the end)")
        tensors[name] = (dims, typ, mm[base + off:base + off + nb])
    return meta, tensors


def gguf_state_dict(path: str, handle_prefix: Optional[str] = "model.diffusion_model.") -> Dict[str, GGUFTensor]:
    """gguf_sd_loader (Quantizer.py:581-665): {key: GGUFTensor}.  `handle_prefix` is stripped only if some tensor carries it, and tensors without it are
    then dropped; the shape is the GGUF dims reversed unless a `comfy.gguf.orig_shape.<name>` INT32 array says otherwise (TypeError for any other
    type); `general.architecture`, if there, must be a string (TypeError) out of ARCHITECTURES (ValueError)."""
    meta, tensors = read_gguf(path)
    has_prefix = handle_prefix is not None and any(n.startswith(handle_prefix) for n in tensors)
    if "general.architecture" in meta:
        arch, types = meta["general.architecture"]
        if types != (T_STRING,):
            raise TypeError(f"Bad type for GGUF general.architecture key: expected string, got {types!r}")
        if arch not in ARCHITECTURES:
            raise ValueError(f"Unexpected architecture type in GGUF file, expected one of {', '.join(ARCHITECTURES)} but got {arch!r}")
    out: Dict[str, GGUFTensor] = {}
    for name, (dims, typ, raw) in tensors.items():
        key = name
        if has_prefix:
            if not name.startswith(handle_prefix):
                continue
            key = name[len(handle_prefix):]
        if ORIG_SHAPE + name in meta:
            orig, types = meta[ORIG_SHAPE + name]
            if types != (T_ARRAY, T_INT32):
                raise TypeError(f"Bad original shape metadata for {ORIG_SHAPE + name}: Expected ARRAY of INT32, got {types!r}")
            shape = tuple(int(v) for v in orig)
        else:
            shape = tuple(int(v) for v in reversed(dims))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)      # torch's note on a read-only array: the view of the mapping is never written
            view = torch.from_numpy(raw)
        out[key] = GGUFTensor(view, typ, shape, name=name)
    return out


def gguf_t5_state_dict(path: str, num_layers: int = 24) -> Dict[str, GGUFTensor]:
    """gguf_clip_loader (Quantizer.py:840-856): the file's keys renamed to the torch module's.  The file must be a T5 encoder of `num_layers` blocks
    (the reference asserts on block 23, T5-XXL's last; a smaller net says how many it has)."""
    raw = gguf_state_dict(path)
    assert f"enc.blk.{num_layers - 1}.ffn_up.weight" in raw, "Invalid Text Encoder!"
    out = {}
    for k, v in raw.items():
        for s, d in T5_KEY_MAP:
            k = k.replace(s, d)
        out[k] = v
    return out
