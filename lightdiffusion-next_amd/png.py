"""SaveImage, the last stage of every pipeline exit (src/FileManaging/ImageSaver.py:79-220: clip(i * 255, 0, 255).astype(uint8), Image.fromarray,
img.save(path, pnginfo=None, compress_level=4)), on the device: the 8-bit image AutoHDR left there goes in, the finished PNG file comes out, and the only
device -> host traffic is the compressed file.

The file is not Pillow's (zlib's hash chains are sequential); it is a PNG of the same pixels and of comparable size, made by rules that are a pure
function of the bytes and split into independent chunks (include/ldx.h states them; tests/golden/png.META.txt has the measured sizes):
  filter      per row the PNG filter type (None, Sub, Up, Average, Paeth; bpp 3) with the smallest sum of |signed residual|, ties to the lowest type
  deflate     the filtered stream in chunks of CHUNK bytes, each one deflate block on its own: tokens are literals and distance-1 runs, code lengths by
              Huffman's algorithm limited to 15 (7) bits, canonical codes; a stored block where that is not smaller; chunks end on a byte boundary
  container   signature, IHDR, one IDAT per chunk, one IDAT with the Adler-32, IEND
png_host() is the whole encoder in numpy on one image: the statement of the format and what the device tests compare with, byte for byte.  PNGEncoder
runs it in three launches per call (ldx_png_encode, csrc/png.hip -> libldx_png.so).  SaveImage is the reference's file placement around either.
"""
import os
import struct
import zlib

import numpy as np

CHUNK = 16384                           # bytes of the filtered stream per deflate block (csrc/png.hip: PNG_CHUNK)
MIN_RUN, MAX_MATCH = 4, 258
_LEN_BASE = np.array([3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258])
_LEN_EXTRA = np.array([0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0])
_CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
_SIGNATURE = b"\x89PNG\r\n\x1a\n"
_ZLIB_HEADER = b"\x78\x01"


def quantize(image):
    """The reference's fp32 -> uint8: (uint8) trunc(clamp(255.0f * v, 0, 255))."""
    return np.clip(np.asarray(image, dtype=np.float32) * np.float32(255.0), 0, 255).astype(np.uint8)


def filter_host(u8_image):
    """(filtered stream uint8 [H][1 + 3 W], filter types uint8 [H]) of one uint8 [H][W][3] image."""
    img = np.asarray(u8_image)
    if img.ndim != 3 or img.shape[2] != 3 or img.dtype != np.uint8:
        raise ValueError(f"filter_host takes uint8 [H, W, 3], not {img.dtype} {img.shape}")
    h, w, _ = img.shape
    cur = img.reshape(h, 3 * w).astype(np.int32)
    left = np.zeros_like(cur)
    left[:, 3:] = cur[:, :-3]
    up = np.zeros_like(cur)
    up[1:] = cur[:-1]
    ul = np.zeros_like(cur)
    ul[:, 3:] = up[:, :-3]
    p = left + up - ul
    pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - ul)
    paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
    res = np.stack([cur, cur - left, cur - up, cur - ((left + up) >> 1), cur - paeth]) & 255          # [5][H][3 W]
    cost = np.where(res < 128, res, 256 - res).sum(axis=2)                                              # [5][H]
    types = np.argmin(cost, axis=0)                                                                     # the first minimum: ties to the lowest type
    stream = np.empty((h, 1 + 3 * w), np.uint8)
    stream[:, 0] = types
    stream[:, 1:] = res[types, np.arange(h)]
    return stream, types.astype(np.uint8)


def huffman_lengths(counts, limit):
    """Code lengths <= limit for the symbols with a non-zero count.  The used symbols sorted by (count, symbol); Huffman's algorithm on two queues, a
    leaf before an internal node of the same weight; depths above the limit are set to it and the count of codes per length repaired (while the Kraft
    sum is above 1: one code of the limit leaves, the deepest shorter code moves one down and brings the leaver with it); the lengths then go to the
    symbols in sorted order, the rarest the longest."""
    counts = [int(c) for c in counts]
    order = sorted((i for i, c in enumerate(counts) if c > 0), key=lambda i: (counts[i], i))
    lens = [0] * len(counts)
    u = len(order)
    if u == 0:
        return lens
    if u == 1:
        lens[order[0]] = 1
        return lens
    w = [counts[i] for i in order]
    iw, ip, lp = [0] * (u - 1), [0] * (u - 1), [0] * u
    li = ii = 0
    for j in range(u - 1):
        s = 0
        for _ in range(2):
            if li < u and (ii >= j or w[li] <= iw[ii]):
                s += w[li]
                lp[li] = j
                li += 1
            else:
                s += iw[ii]
                ip[ii] = j
                ii += 1
        iw[j] = s
    depth = [0] * (u - 1)
    for j in range(u - 3, -1, -1):
        depth[j] = depth[ip[j]] + 1
    num = [0] * (limit + 1)
    for i in range(u):
        num[min(depth[lp[i]] + 1, limit)] += 1
    total = sum(num[i] << (limit - i) for i in range(1, limit + 1))
    while total > (1 << limit):
        num[limit] -= 1
        for i in range(limit - 1, 0, -1):
            if num[i]:
                num[i] -= 1
                num[i + 1] += 2
                break
        total -= 1
    j = u
    for length in range(1, limit + 1):
        for _ in range(num[length]):
            j -= 1
            lens[order[j]] = length
    return lens


def canonical_codes(lens):
    """Canonical codes of the lengths (RFC 1951 3.2.2), bit-reversed: the form that is written least significant bit first."""
    lens = [int(x) for x in lens]
    limit = max(lens + [1])
    num = [0] * (limit + 2)
    for x in lens:
        if x:
            num[x] += 1
    nxt, code = [0] * (limit + 2), 0
    for b in range(1, limit + 1):
        code = (code + num[b - 1]) << 1
        nxt[b] = code
    out = [0] * len(lens)
    for i, x in enumerate(lens):
        if x:
            out[i] = int(format(nxt[x], f"0{x}b")[::-1], 2)
            nxt[x] += 1
    return out


def _pack(vals, nbits):
    """Bit fields (value, width), first field first, each least significant bit first: uint8 bits."""
    vals, nbits = np.asarray(vals, dtype=np.int64), np.asarray(nbits, dtype=np.int64)
    total = int(nbits.sum())
    if total == 0:
        return np.zeros(0, np.uint8)
    start = np.cumsum(nbits) - nbits
    within = np.arange(total) - np.repeat(start, nbits)
    return ((np.repeat(vals, nbits) >> within) & 1).astype(np.uint8)


def tokens_host(s):
    """The matcher, per position of one chunk.  A position breaks when it is the chunk's first or its byte differs from the one before.  A position
    that does not break lies in a run: a = the last break before it, R = the run's positions (up to the next break or the chunk's end), k = its
    index among them.  R < 4: a literal.  Otherwise the run is cut into pieces of 258; a piece shorter than 3 is literals, any other piece is one
    match (length = the piece, distance 1) at its first position.  Returns (is_literal, is_match, match length) per position."""
    n = len(s)
    idx = np.arange(n)
    brk = np.ones(n, bool)
    brk[1:] = s[1:] != s[:-1]
    a = np.maximum.accumulate(np.where(brk, idx, 0))
    nxt = np.full(n + 1, n)
    nxt[:n] = np.where(brk, idx, n)
    nb = np.minimum.accumulate(nxt[::-1])[::-1][1:]
    k, run = idx - a - 1, nb - a - 1
    base = np.where(brk, 0, (k // MAX_MATCH) * MAX_MATCH)
    piece = np.minimum(MAX_MATCH, run - base)
    in_match = ~brk & (run >= MIN_RUN) & (piece >= 3)
    return ~in_match, in_match & (k == base), piece


def _code_length_tokens(lens):
    """The code lengths as symbols of the code-length alphabet, greedy from the left: at a zero, a run of >= 11 zeros is (18, min(run, 138)), of >= 3
    is (17, run); at a length equal to the one before it, a run of >= 3 is (16, min(run, 6)); anything else is the length itself."""
    out, i, n = [], 0, len(lens)
    while i < n:
        v, r = lens[i], 1
        while i + r < n and lens[i + r] == v and r < 138:
            r += 1
        if v == 0 and r >= 11:
            out.append((18, r - 11, 7)); i += r
        elif v == 0 and r >= 3:
            out.append((17, r - 3, 3)); i += r
        elif v != 0 and i > 0 and lens[i - 1] == v and r >= 3:
            r = min(r, 6)
            out.append((16, r - 3, 2)); i += r
        else:
            out.append((v, 0, 0)); i += 1
    return out


def deflate_chunk(s, last, prefix=b""):
    """One chunk of at most CHUNK bytes as deflate blocks that end on a byte boundary, after `prefix` (the zlib header in the first chunk)."""
    s = np.asarray(s, dtype=np.uint8)
    n = len(s)
    assert 0 < n <= CHUNK
    is_lit, is_match, piece = tokens_host(s)
    lsym = np.searchsorted(_LEN_BASE, piece[is_match], side="right") - 1
    hist = np.bincount(s[is_lit], minlength=286) + np.bincount(257 + lsym, minlength=286)
    hist[256] += 1
    ll_lens = huffman_lengths(hist, 15)
    nlit = max(257, max(i for i, x in enumerate(ll_lens) if x) + 1)
    toks = _code_length_tokens(ll_lens[:nlit] + [1, 1])                 # two distance codes of one bit: distance 1 is the bit 0
    cl_hist = [0] * 19
    for sym, _, _ in toks:
        cl_hist[sym] += 1
    cl_lens = huffman_lengths(cl_hist, 7)
    ncl = max(4, max(i for i, sym in enumerate(_CL_ORDER) if cl_lens[sym]) + 1)
    ll_code, cl_code = np.array(canonical_codes(ll_lens)), canonical_codes(cl_lens)
    ll_lens = np.array(ll_lens)
    vals, bits = [1 if last else 0, 2, nlit - 257, 1, ncl - 4], [1, 2, 5, 5, 4]
    for sym in _CL_ORDER[:ncl]:
        vals.append(cl_lens[sym]); bits.append(3)
    for sym, extra, extra_bits in toks:
        vals.append(cl_code[sym] | (extra << cl_lens[sym])); bits.append(cl_lens[sym] + extra_bits)
    # the tokens in position order
    pos = np.flatnonzero(is_lit | is_match)
    sym = s[pos].astype(np.int64)
    m = is_match[pos]
    msym = np.searchsorted(_LEN_BASE, piece[pos][m], side="right") - 1
    sym[m] = 257 + msym
    tv, tb = ll_code[sym], ll_lens[sym]
    tv[m] |= (piece[pos][m] - _LEN_BASE[msym]) << tb[m]
    tb[m] += _LEN_EXTRA[msym] + 1
    vals = np.concatenate([vals, tv, [ll_code[256]]])
    bits = np.concatenate([bits, tb, [ll_lens[256]]])
    dyn_bytes = (int(bits.sum()) + 7) // 8
    if dyn_bytes < n + 5:
        stream = _pack(vals, bits)
        if not last:                                                    # an empty stored block: 000, to the byte boundary, 00 00 FF FF
            stream = np.concatenate([stream, np.zeros(3, np.uint8)])
        body = np.packbits(stream, bitorder="little").tobytes()
        return prefix + body + (b"" if last else b"\x00\x00\xff\xff")
    return prefix + bytes([1 if last else 0]) + struct.pack("<HH", n, n ^ 0xFFFF) + s.tobytes()


def deflate_host(data):
    """The chunks' deflate blocks of a byte string, one bytes object per chunk; the first begins with the zlib header."""
    s = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    if len(s) == 0:
        raise ValueError("deflate_host: no bytes")
    nchunks = (len(s) + CHUNK - 1) // CHUNK
    return [deflate_chunk(s[c * CHUNK:(c + 1) * CHUNK], c == nchunks - 1, _ZLIB_HEADER if c == 0 else b"") for c in range(nchunks)]


def zlib_host(data):
    """A complete zlib stream of `data`: header, the chunks, Adler-32."""
    return b"".join(deflate_host(data)) + struct.pack(">I", zlib.adler32(bytes(data)))


def _png_chunk(kind, payload):
    return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(kind + payload))


def png_host(u8_image):
    """The PNG file of one uint8 [H][W][3] image."""
    stream, _ = filter_host(u8_image)
    h, w = stream.shape[0], (stream.shape[1] - 1) // 3
    raw = stream.tobytes()
    out = [_SIGNATURE, _png_chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))]
    out += [_png_chunk(b"IDAT", c) for c in deflate_host(raw)]
    out += [_png_chunk(b"IDAT", struct.pack(">I", zlib.adler32(raw))), _png_chunk(b"IEND", b"")]
    return b"".join(out)


def bound_bytes(h, w):
    """The largest file png_host can make of an H x W image (ldx_png_bound_bytes): a chunk is at most its bytes + 9 (a stored block is + 5; a dynamic
    block is chosen only when shorter than that and is followed by at most 5 bytes), 12 bytes frame each IDAT; signature 8, IHDR 25, zlib header 2,
    Adler IDAT 16, IEND 12."""
    n = h * (1 + 3 * w)
    return 63 + n + 21 * ((n + CHUNK - 1) // CHUNK)


class PNGEncoder:
    """png_host on device images.  The workspace and the output buffer are kept per shape; encode() is three launches on the current stream with no
    allocation after the first call of a shape and no host synchronisation before the copies at its end, so it follows AutoHDR.apply on the same stream."""

    def __init__(self, device=0):
        import torch
        from . import lib
        self._torch, self._libmod = torch, lib
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self._lib = lib.load()
        self._bufs = {}

    def _buffers(self, b, h, w):
        torch, lib = self._torch, self._libmod
        bufs = self._bufs.get((b, h, w))
        if bufs is None:
            nws, bound = int(self._lib.ldx_png_workspace_bytes(b, h, w)), int(self._lib.ldx_png_bound_bytes(h, w))
            if nws < 0 or bound < 0:
                lib.check(min(nws, bound), "ldx_png_workspace_bytes")
            stride = (bound + 255) // 256 * 256
            bufs = self._bufs[(b, h, w)] = (torch.empty(nws, dtype=torch.uint8, device=self.device),
                                            torch.empty((b, stride), dtype=torch.uint8, device=self.device),
                                            torch.empty(b, dtype=torch.int32, device=self.device))
        return bufs

    def encode_device(self, images):
        """The launches alone: (files uint8 [B][stride], lengths int32 [B]) on the device, valid once the current stream reaches this point; the
        buffers are the instance's and are overwritten by the next call of the same shape."""
        torch, lib = self._torch, self._libmod
        if images.dim() == 3:
            images = images[None]
        if images.dim() != 4 or images.shape[-1] != 3 or images.dtype not in (torch.float32, torch.uint8):
            raise ValueError(f"PNGEncoder.encode takes fp32 or uint8 [B, H, W, 3] or [H, W, 3], not {images.dtype} {tuple(images.shape)}")
        if images.device != self.device:
            raise ValueError(f"PNGEncoder.encode: images on {images.device}, instance on {self.device}")
        images = images.contiguous()
        b, h, w, _ = images.shape
        ws, out, lens = self._buffers(b, h, w)
        is_u8 = images.dtype == torch.uint8
        with torch.cuda.device(self.device):
            lib.check(self._lib.ldx_png_encode(None if is_u8 else lib.ptr(images), lib.ptr(images) if is_u8 else None, w * 3, b, h, w, lib.ptr(ws),
                                               lib.ptr(out), out.shape[1], lib.ptr(lens), lib.current_stream_ptr()), "ldx_png_encode")
        return out, lens

    def encode(self, images):
        """images: device fp32 (quantised as the reference does) or uint8, [B][H][W][3] or [H][W][3].  Returns the B files as bytes: one copy of the
        lengths, then one copy of no more than the longest file's bytes per image."""
        out, lens = self.encode_device(images)
        lens = lens.cpu().tolist()
        host = out[:, :max(lens)].cpu().numpy()
        return [host[i, :n].tobytes() for i, n in enumerate(lens)]


_SUBFOLDERS = ("Classic", "HiresFix", "Img2Img", "Flux", "Adetailer")
_PREFIX_FOLDER = {"LD-HF": "HiresFix", "LD-I2I": "Img2Img", "LD-Flux": "Flux", "LD-head": "Adetailer", "LD-body": "Adetailer"}


def get_save_image_path(filename_prefix, output_dir, image_width=0, image_height=0):
    """ImageSaver.py:18-73: (folder, filename, counter, subfolder, prefix).  The five subfolders are made; the counter is one above the highest number
    among the files of all five that start with the filename and end in .png (the number is what stands between the filename's length + 1 and the
    next underscore; anything that is no number counts as 0)."""
    filename_prefix = filename_prefix.replace("%width%", str(image_width)).replace("%height%", str(image_height))
    subfolder = os.path.dirname(os.path.normpath(filename_prefix))
    filename = os.path.basename(os.path.normpath(filename_prefix))
    skip = len(os.path.basename(filename_prefix)) + 1
    folder = os.path.join(output_dir, subfolder)
    counter = 1
    for sub in _SUBFOLDERS:
        path = os.path.join(folder, sub)
        os.makedirs(path, exist_ok=True)
        for f in os.listdir(path):
            if f.startswith(filename) and f.endswith(".png"):
                try:
                    digits = int(f[skip:].split("_")[0])
                except ValueError:
                    digits = 0
                counter = max(counter, digits + 1)
    return folder, filename, counter, subfolder, filename_prefix


class SaveImage:
    """The reference's SaveImage.save_images with the encoder of this module in Pillow's place: the same folders, names, counter and return value.
    Device tensors are encoded on their device (one PNGEncoder per device, made on first use), host arrays and tensors by png_host."""

    def __init__(self, output_dir="./output"):
        self.output_dir = output_dir
        self.type = "output"
        self.prefix_append = ""
        self._encoders = {}

    def _files(self, image):
        """The PNG files of one entry of `images`: [H][W][3] or [B][H][W][3], fp32 or uint8."""
        if hasattr(image, "is_cuda") and image.is_cuda:
            enc = self._encoders.get(image.device)
            if enc is None:
                enc = self._encoders[image.device] = PNGEncoder(image.device)
            return enc.encode(image)
        arr = image.numpy() if hasattr(image, "numpy") else np.asarray(image)
        if arr.ndim == 3:
            arr = arr[None]
        if arr.ndim != 4 or arr.shape[-1] != 3:
            raise ValueError(f"SaveImage takes [B, H, W, 3] or [H, W, 3] images, not {arr.shape}")
        return [png_host(a if a.dtype == np.uint8 else quantize(a)) for a in arr]

    def save_images(self, images, filename_prefix="LD"):
        filename_prefix += self.prefix_append
        folder, filename, counter, subfolder, filename_prefix = get_save_image_path(filename_prefix, self.output_dir, images[0].shape[-2],
                                                                                    images[0].shape[-1])
        save_path = os.path.join(folder, _PREFIX_FOLDER.get(filename_prefix, "Classic"))
        results = []
        for batch_number, image in enumerate(images):
            for data in self._files(image):
                name = f"{filename.replace('%batch_num%', str(batch_number))}_{counter:05}_.png"
                with open(os.path.join(save_path, name), "wb") as f:
                    f.write(data)
                results.append({"filename": name, "subfolder": subfolder, "type": self.type})
                counter += 1
        return {"ui": {"images": results}}
