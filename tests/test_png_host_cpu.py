"""The PNG encoder's numpy statement (lightdiffusion-next_amd/png.py: png_host, zlib_host) against the format's own judges, with no GPU: Pillow opens
the file (and verifies the chunk CRCs) and returns the input's pixels, zlib inflates the IDAT payload to the filtered stream and agrees on the Adler-32,
zlib.crc32 agrees on every chunk; the file is never above ldx_png_bound_bytes; its size is held against Pillow's compress_level=4 file of the same
bytes, computed here (the measured ratios are in tests/golden/png.META.txt).  The device's equality with this statement is tests/test_png_gpu.py's."""
import io
import os
import struct
import sys
import zlib

import numpy as np
import pytest
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import png_cases  # noqa: E402

IMAGES = png_cases.all_images()


@pytest.fixture(scope="module")
def png(ldx):
    return ldx.png


def chunks_of(data):
    """[(type, payload, crc)] of a PNG file; the signature and the framing are checked on the way."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    out, pos = [], 8
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        out.append((kind, data[pos + 8:pos + 8 + n], struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0]))
        pos += 12 + n
    assert pos == len(data)
    return out


def check_file(png, data, img):
    h, w, _ = img.shape
    with Image.open(io.BytesIO(data)) as im:
        im.load()                                                       # Pillow checks every chunk's CRC while it reads
        assert im.mode == "RGB" and im.size == (w, h)
        assert np.array_equal(np.asarray(im), img)
    chunks = chunks_of(data)
    for kind, payload, crc in chunks:
        assert crc == zlib.crc32(kind + payload), kind
    kinds = [k for k, _, _ in chunks]
    assert kinds[0] == b"IHDR" and kinds[-1] == b"IEND" and set(kinds[1:-1]) == {b"IDAT"}
    assert chunks[0][1] == struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)
    idat = b"".join(p for k, p, _ in chunks if k == b"IDAT")
    stream, types = png.filter_host(img)
    assert zlib.decompress(idat) == stream.tobytes()
    assert struct.unpack(">I", idat[-4:])[0] == zlib.adler32(stream.tobytes())
    nchunks = (stream.size + png.CHUNK - 1) // png.CHUNK
    assert len(kinds) == 2 + nchunks + 1                                # one IDAT per chunk and the Adler-32's
    assert len(data) <= png.bound_bytes(h, w)


@pytest.mark.parametrize("name", sorted(IMAGES))
def test_file_is_a_valid_png_of_the_input(png, name):
    img = IMAGES[name]
    check_file(png, png.png_host(img), img)


def test_bound_is_what_the_library_reports(png, ldx_lib):
    for h, w in ((1, 1), (64, 64), (32, 341), (150, 100), (1024, 1024)):
        assert ldx_lib.ldx_png_bound_bytes(h, w) == png.bound_bytes(h, w)
    assert ldx_lib.ldx_png_bound_bytes(0, 8) == -1 and ldx_lib.ldx_png_bound_bytes(8, -1) == -1 and ldx_lib.ldx_png_workspace_bytes(0, 8, 8) == -1
    assert ldx_lib.ldx_png_bound_bytes(40000, 40000) == -1              # a stream above 2^30 bytes
    assert ldx_lib.ldx_png_workspace_bytes(2, 150, 100) >= 2 * (45150 + 3 * 16384)
    assert ldx_lib.ldx_zlib_bound_bytes(0) == -1 and ldx_lib.ldx_zlib_workspace_bytes(0) == -1 and ldx_lib.ldx_zlib_bound_bytes(32769) == 6 + 32769 + 27


def test_random_bytes_cost_five_bytes_per_chunk(png):
    """Incompressible input is stored: the IDAT payload is the stream + 5 per chunk + the zlib header and the Adler-32."""
    img = IMAGES["random_64x64"]
    idat = b"".join(p for k, p, _ in chunks_of(png.png_host(img)) if k == b"IDAT")
    n = 64 * (1 + 3 * 64)
    assert len(idat) == n + 5 * ((n + png.CHUNK - 1) // png.CHUNK) + 6


def test_filter_choice_is_the_stated_rule(png):
    """The vectorised filter against the rule spelled out byte by byte on a small image."""
    img = png_cases.mixed(9, 14, 4)
    stream, types = png.filter_host(img)
    rows = img.reshape(9, 42).astype(int)
    for y in range(9):
        costs, lines = [], []
        for t in range(5):
            line = []
            for x in range(42):
                a = rows[y, x - 3] if x >= 3 else 0
                b = rows[y - 1, x] if y else 0
                c = rows[y - 1, x - 3] if y and x >= 3 else 0
                p = a + b - c
                paeth = a if abs(p - a) <= abs(p - b) and abs(p - a) <= abs(p - c) else (b if abs(p - b) <= abs(p - c) else c)
                line.append((rows[y, x] - (0, a, b, (a + b) // 2, paeth)[t]) % 256)
            lines.append(line)
            costs.append(sum(r if r < 128 else 256 - r for r in line))
        assert types[y] == costs.index(min(costs)) and stream[y, 0] == types[y]
        assert list(stream[y, 1:]) == lines[types[y]]
    assert len(set(types.tolist())) >= 2


def test_matcher_pieces(png):
    """Runs of 259, 3, 4, 5, 261, 262 and 520 equal bytes: the break is a literal, a run of < 4 after it is literals, 258 + a piece < 3 is a match and
    literals, 258 + 3 is two matches."""
    runs = (259, 3, 4, 5, 261, 262, 520)
    s = np.concatenate([np.full(n, 5 + i, np.uint8) for i, n in enumerate(runs)])
    lit, match, piece = png.tokens_host(s)
    got, pos = [], 0
    for n in runs:
        got.append((int(lit[pos:pos + n].sum()), [int(x) for x in piece[pos:pos + n][match[pos:pos + n]]]))
        pos += n
    assert got == [(1, [258]), (3, []), (4, []), (1, [4]), (3, [258]), (1, [258, 3]), (1, [258, 258, 3])]
    assert zlib.decompress(png.zlib_host(s.tobytes())) == s.tobytes()


@pytest.mark.parametrize("which", ["fibonacci", "deep"])
def test_code_length_limit(png, which):
    """Counts that follow the Fibonacci numbers over 20 values (equal weights meet all the way up: with a leaf before an internal node of equal weight
    Huffman's tree stays 11 deep), and counts inside one chunk that force a chain 17 deep under any tie-breaking: the lengths stay within 15 bits, are
    complete, and the stream inflates to the input."""
    data = png_cases.fibonacci_stream() if which == "fibonacci" else png_cases.deep_stream()
    assert len(data) == (17710 if which == "fibonacci" else 13510)
    assert which == "fibonacci" or len(data) <= png.CHUNK
    z = png.zlib_host(data)
    assert zlib.decompress(z) == data and len(z) < len(data)
    counts = np.bincount(np.frombuffer(data, np.uint8), minlength=286)
    counts[256] = 1
    free = png.huffman_lengths(counts, 40)
    lens = png.huffman_lengths(counts, 15)
    if which == "deep":
        assert max(free) > 15
    assert max(lens) <= 15 and sum(2.0 ** -x for x in lens if x) == 1.0
    assert [x > 0 for x in lens] == [c > 0 for c in counts]


def test_huffman_lengths_are_optimal_and_limited(png):
    """Without a limit in reach the cost is Huffman's; with one the code is complete and within it; ties go by symbol index."""
    import heapq
    rng = np.random.default_rng(8)
    for _ in range(60):
        n = int(rng.integers(2, 287))
        counts = [int(rng.choice([0, 0, 1, 2, 3, int(rng.integers(1, 5000))])) for _ in range(n)]
        used = [c for c in counts if c]
        if len(used) < 2:
            continue
        heap, cost = list(used), 0
        heapq.heapify(heap)
        while len(heap) > 1:
            a, b = heapq.heappop(heap), heapq.heappop(heap)
            cost += a + b
            heapq.heappush(heap, a + b)
        assert sum(c * x for c, x in zip(counts, png.huffman_lengths(counts, 40))) == cost
        for limit in (15, 9):
            lens = png.huffman_lengths(counts, limit)
            assert max(lens) <= limit and sum(2.0 ** -x for x in lens if x) == 1.0
    assert png.huffman_lengths([5, 5, 5, 5, 0, 5], 15) == [3, 3, 2, 2, 0, 2]
    assert png.huffman_lengths([0, 7, 0], 15) == [0, 1, 0]


SIZE_IMAGES = png_cases.size_images()


@pytest.mark.parametrize("name", sorted(SIZE_IMAGES))
def test_size_against_pillow_level_4(png, name):
    img = SIZE_IMAGES[name]
    ours = len(png.png_host(img))
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "PNG", compress_level=4)
    pillow = len(buf.getvalue())
    n = img.shape[0] * (1 + 3 * img.shape[1])
    nchunks = (n + png.CHUNK - 1) // png.CHUNK
    print(f"{name}: ours {ours}, Pillow {pillow}, ratio {ours / pillow:.3f}, chunks {nchunks}")
    assert ours <= max(1.15 * pillow, pillow + 160 * nchunks)


def test_zlib_host_of_more_than_one_chunk(png):
    data = np.concatenate([IMAGES["midrow_150x100"].reshape(-1), np.zeros(40000, np.uint8), IMAGES["random_64x64"].reshape(-1)]).tobytes()
    z = png.zlib_host(data)
    assert z[:2] == b"\x78\x01" and zlib.decompress(z) == data
    with pytest.raises(ValueError):
        png.zlib_host(b"")
