"""A GGUF v2 / v3 writer from the published layout, for tests/test_gguf_cpu.py and tests/test_q8_gpu.py (the `gguf` package is not available here, so the
reader is held to files this writer makes), and llama.cpp's Q8_0 quantiser."""
import struct

import numpy as np
import torch

GGML_F32, GGML_F16, GGML_Q8_0, GGML_BF16 = 0, 1, 8, 30
_FMT = {0: "<B", 1: "<b", 2: "<H", 3: "<h", 4: "<I", 5: "<i", 6: "<f", 7: "<?", 10: "<Q", 11: "<q", 12: "<d"}


def _s(b: bytes) -> bytes:
    return struct.pack("<Q", len(b)) + b


def _value(t, v) -> bytes:
    """t: a metadata value type 0..12; an array is t = (9, element type)."""
    if isinstance(t, tuple):
        return struct.pack("<IQ", t[1], len(v)) + b"".join(_value(t[1], e) for e in v)
    if t == 8:
        return _s(v.encode())
    return struct.pack(_FMT[t], v)


def write_gguf(path, tensors, meta, version=3, align=None, cut=None):
    """tensors: [(name, torch-order shape, ggml type, raw bytes)]; meta: {key: (type, value)}.  align: written as general.alignment (u32) when given.
    cut: bytes dropped from the end of the file."""
    meta = dict(meta)
    if align is not None:
        meta["general.alignment"] = (4, align)
    a = align or 32
    out = bytearray(struct.pack("<IIQQ", 0x46554747, version, len(tensors), len(meta)))
    for k, (t, v) in meta.items():
        out += _s(k.encode()) + struct.pack("<I", 9 if isinstance(t, tuple) else t) + _value(t, v)
    off, blobs = 0, []
    for name, shape, typ, raw in tensors:
        dims = tuple(reversed(shape))                  # GGUF: innermost first
        out += _s(name.encode()) + struct.pack("<I", len(dims)) + b"".join(struct.pack("<Q", d) for d in dims) + struct.pack("<IQ", typ, off)
        pad = (-len(raw)) % a
        blobs.append(bytes(raw) + b"\0" * pad)
        off += len(raw) + pad
    out += b"\0" * ((-len(out)) % a)
    for b in blobs:
        out += b
    if cut:
        out = out[:-cut]
    with open(path, "wb") as f:
        f.write(out)


def q8_0(x: torch.Tensor) -> bytes:
    """llama.cpp's Q8_0 quantiser along the last axis: per 32 values d = amax / 127 (stored fp16), q = round(x / d)."""
    xb = x.detach().float().numpy().reshape(-1, 32)
    d = (np.abs(xb).max(axis=1) / 127.0).astype(np.float16)
    df = d.astype(np.float32)
    inv = np.where(df > 0, 1.0 / np.maximum(df, 1e-30), 0.0)
    q = np.clip(np.rint(xb * inv[:, None]), -127, 127).astype(np.int8)
    return np.concatenate([d.view(np.uint8).reshape(-1, 2), q.view(np.uint8)], axis=1).tobytes()


def raw_of(x: torch.Tensor, typ: int) -> bytes:
    """The bytes of tensor x stored as ggml type typ."""
    if typ == GGML_Q8_0:
        return q8_0(x)
    t = x.detach().to({GGML_F32: torch.float32, GGML_F16: torch.float16, GGML_BF16: torch.bfloat16}[typ]).contiguous()
    return t.view(torch.uint8).numpy().tobytes()


def all_pairs_blocks() -> torch.Tensor:
    """Every (fp16 scale, int8 value) pair once: 524 288 Q8_0 blocks (17.8 MB) as a flat uint8 tensor.  Block b holds scale pattern b // 8 and the 32 values
    (b % 8) * 32 .. + 31 as bytes."""
    nb = 65536 * 8
    blocks = np.empty((nb, 34), np.uint8)
    d = np.repeat(np.arange(65536, dtype=np.uint16), 8)
    blocks[:, 0] = d & 0xff
    blocks[:, 1] = d >> 8
    blocks[:, 2:] = (np.tile(np.arange(8, dtype=np.uint16), 65536)[:, None] * 32 + np.arange(32, dtype=np.uint16)[None, :]).astype(np.uint8)
    return torch.from_numpy(blocks.reshape(-1))


def torch_q8_0(raw: torch.Tensor) -> torch.Tensor:
    """The reference's expression (Quantize/Quantizer.py:94-112, dequant_dtype None) on flat uint8 blocks: d.view(float16) * x.view(int8), fp16."""
    blocks = raw.reshape(-1, 34)
    d = blocks[:, :2].contiguous().view(torch.float16)
    x = blocks[:, 2:].contiguous().view(torch.int8)
    return (d * x).reshape(-1)


def assert_same_bits(got: torch.Tensor, want: torch.Tensor):
    """Bit-equal where `want` is no NaN, NaN in the same places."""
    assert got.dtype == want.dtype and got.shape == want.shape
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan)
    bits = {2: torch.int16, 4: torch.int32}[want.element_size()]
    g, w = got.contiguous().view(bits), want.contiguous().view(bits)
    assert torch.equal(g[~nan], w[~nan])
