"""Case table of the producer-written GroupNorm statistics tests (tests/test_gn_stats_cpu.py, tests/test_gn_stats_gpu.py): one case per device code path that
writes GroupNormArgs::partial, the kernel pick each case is there for (asked through ldx_op_gemm_pick: host arithmetic), the integer inputs and the int64 reference.

Integer inputs: activations dense in {-1, 0, 1}, every output row of W with 8 entries of +-1 at distinct random positions over the WHOLE K (all nine taps, the skip
segment, every K split), bias in [-3, 3], the per-image vector in [-2, 2], the residual in [-3, 3].  Every stored value is then an integer of magnitude <= 16 — exact
in bf16 and f16 — and every fp32 accumulator, split-K partial and statistic an exact integer as long as it stays below 2^24 (exactness_ok asserts that on the
REFERENCE), so kernel and reference must agree bit for bit whatever the summation order."""
import ctypes as C
from collections import namedtuple

import torch

FAMILIES = ("tile", "tile2", "pingpong", "pingpong2", "ring", "conv_patch", "tile_mx", "tile2_mx", "pingpong_mx", "pingpong2_mx")      # GemmFamily (csrc/ldx_kernels.h)
REDUCE = ("none", "reduce", "reduce_gn", "in_kernel")
G = 32                       # groups of every GroupNorm of the models
NNZ = 8                      # non-zeros per output row of W
GN_NCHUNK, GN_FOLD = 256, 64      # csrc/ldx_kernels.h
CP_TH, CP_TW = 16, 32        # csrc/ldx_geometry.h: output pixels per tile of the patch-resident conv, rows x columns
SENTINEL = -12345.5          # no integer: a statistics row that still holds it was not written

# op: conv (B images of H x W, Cin -> N channels, stride 1, + a fused 1x1 skip over Cin2 channels), gemm (B images of HW rows, K -> N), rowgemm (the same on the row-block kernel)
# rv / res: with the per-image vector / the residual;  pick: (family, BM, BN, K splits, reduce kind), None for the row-block kernel (ldx_op_gemm_pick does not know it);
# chunks: statistics rows per image;  rows: how a chunk's rows are found ("rows": HW / chunks consecutive rows, "patch": 16 x 32-pixel tiles in row-major tile order)
Case = namedtuple("Case", "name op B H W Cin N Cin2 rv res pick chunks rows")


def _conv(name, B, H, W, Cin, N, pick, chunks, Cin2=0, rv=False, res=False, rows="rows"):
    return Case(name, "conv", B, H, W, Cin, N, Cin2, rv, res, pick, chunks, rows)


CASES = [
    _conv("A", 1, 16, 16, 320, 320, ("tile", 128, 160, 9, "reduce_gn"), 32, rv=True),                  # split-K reduce launch, cpg 10
    _conv("B", 1, 16, 16, 640, 320, ("tile", 128, 160, 16, "reduce_gn"), 32, Cin2=640),                # ... with the skip segment in the last splits
    _conv("C", 1, 32, 32, 320, 640, ("pingpong", 256, 128, 10, "reduce_gn"), 256, Cin2=320),           # ... behind the ping-pong kernel, cpg 20
    _conv("D", 2, 32, 32, 1280, 1280, ("pingpong", 256, 128, 3, "reduce_gn"), 256, res=True),          # ... two images, cpg 40, 4-row chunks
    _conv("E", 2, 64, 64, 320, 640, ("tile", 128, 160, 1, "none"), 32, Cin2=320),                      # tile epilogue (GNS), 160 columns = 8 groups of 20
    _conv("F", 1, 64, 64, 256, 256, ("tile", 128, 128, 1, "none"), 32, rv=True),                       # ... 128 columns, cpg 8
    _conv("G", 1, 64, 64, 128, 128, ("tile", 64, 64, 1, "none"), 64, res=True),                        # ... 64 x 64, cpg 4: a lane's four columns are one group
    _conv("H", 2, 64, 64, 1280, 1280, ("pingpong", 256, 160, 1, "none"), 16, rv=True, res=True),       # ping-pong 256 x 160, cpg 40
    _conv("I", 3, 64, 128, 128, 512, ("pingpong", 256, 256, 1, "none"), 32, res=True),                 # column-major output stage of the wide tiles (GNW), cpg 16
    _conv("J", 1, 136, 128, 64, 64, ("tile", 64, 64, 1, "none"), 272, rv=True),                        # cpg 2; 272 rows per image: the consumer folds first
    _conv("K", 1, 256, 512, 128, 128, ("conv_patch", 512, 128, 1, "none"), 256, res=True, rows="patch"),      # patch-resident conv
    Case("L", "gemm", 3, 2048, 1, 320, 320, 0, False, True, ("ring", 64, 160, 1, "none"), 32, "rows"),         # LDS-DMA ring tiles
    Case("M1", "rowgemm", 2, 1024, 1, 320, 320, 0, False, True, None, 8, "rows"),                      # row-block output stage, 128-row blocks
    Case("M2", "rowgemm", 2, 1024, 1, 640, 640, 0, False, True, None, 16, "rows"),                     # ... 64-row blocks, two column halves per block
]
BY_NAME = {c.name: c for c in CASES}
DUP = ("A", "E", "I", "M1")          # run once more with every row stored twice (dup_rows = M)
# launches that must NOT produce statistics: chunks = 0 from the probe, LDX_EINVAL and untouched buffers from the entry points
REFUSALS = [
    _conv("R1", 1, 16, 16, 1280, 1280, ("tile", 128, 128, 16, "reduce"), 0),                            # the one-launch small GroupNorm takes its consumer
    Case("R2", "gemm", 2, 256, 1, 320, 320, 0, False, False, ("tile", 64, 64, 1, "none"), 0, "rows"),
]


def hw(c):
    return c.H * c.W


def rows_total(c):
    return c.B * hw(c)


def k_total(c):
    return 9 * c.Cin + c.Cin2 if c.op == "conv" else c.Cin


def max_chunks(HW):
    """Statistics rows per image the engines' workspace holds (gn_workspace_rows, csrc/ldx_kernels.h)."""
    return min(max(GN_NCHUNK, HW // 64), 32768)


def rowblock_rows(K):
    return 128 * 320 // K


def probe_args(c):
    """ldx_op_gemm_pick's arguments for the launch of case c as the producer of a GroupNorm(32)."""
    M, HW = rows_total(c), hw(c)
    geo = (c.Cin, c.H, c.W, c.H, c.W, 1) if c.op == "conv" else (0, 0, 0, 0, 0, 0)
    return (M, c.N, k_total(c), 1 if c.op == "conv" else 0, 0, -1, 0, 0, 0) + geo + (0, 0, 0, HW, G, max_chunks(HW))


def probe(lib, c):
    """(family, BM, BN, K splits, reduce kind) and the statistics rows per image of case c's launch."""
    out = (C.c_int32 * 10)()
    rc = lib.ldx_op_gemm_pick(*probe_args(c), out)
    assert rc == 0, lib.ldx_last_error()
    return (FAMILIES[out[0]], out[1], out[2], out[6], REDUCE[out[7]]), out[9]


def expected_chunks(c):
    return hw(c) // rowblock_rows(c.Cin) if c.op == "rowgemm" else c.chunks


# ---- integer inputs and the int64 reference ------------------------------------------------------------------------------------------------------------
def int_inputs(c, seed=0):
    """CPU tensors: X int8 [B][H][W][Cin] ([M][K] for gemm / rowgemm), X2 int8 [M][Cin2] or None, Wpos int64 / Wsgn int8 [N][NNZ] (column and sign of every non-zero),
    bias / rowvec / R int8 or None."""
    g = torch.Generator().manual_seed(1000 + seed + sum(ord(ch) for ch in c.name))
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g, dtype=torch.int8)
    M, K = rows_total(c), k_total(c)
    d = {"X": ri(-1, 1, c.B, c.H, c.W, c.Cin) if c.op == "conv" else ri(-1, 1, M, c.Cin)}
    d["X2"] = ri(-1, 1, M, c.Cin2) if c.Cin2 else None
    d["Wpos"] = torch.rand(c.N, K, generator=g).topk(NNZ, dim=1).indices.sort(dim=1).values
    d["Wsgn"] = ri(0, 1, c.N, NNZ) * 2 - 1
    d["bias"] = ri(-3, 3, c.N)
    d["rowvec"] = ri(-2, 2, c.B, c.N) if c.rv else None
    d["R"] = ri(-3, 3, M, c.N) if c.res else None
    return d


def dense_w(c, d):
    """W [N][K] int8 from its non-zeros."""
    W = torch.zeros(c.N, k_total(c), dtype=torch.int8)
    W.scatter_(1, d["Wpos"], d["Wsgn"])
    return W


def int_reference(c, d, device="cpu"):
    """Y int64 [M][N] = conv / GEMM + bias + rowvec + R in integer arithmetic: per non-zero of W one gathered column of the (shifted) input, no float anywhere."""
    M, HW = rows_total(c), hw(c)
    dev = torch.device(device)
    pos, sgn = d["Wpos"].to(dev), d["Wsgn"].to(dev).long()
    n_of = torch.arange(c.N, device=dev).unsqueeze(1).expand(c.N, NNZ)
    Y = torch.zeros(M, c.N, dtype=torch.int64, device=dev)

    def add(src, sel, col):            # Y[:, n] += sgn * src[:, col] for the selected non-zeros
        if sel.any():
            Y.index_add_(1, n_of[sel], src[:, col[sel]].long() * sgn[sel])

    if c.op == "conv":
        X = d["X"].to(dev)
        Xp = torch.zeros(c.B, c.H + 2, c.W + 2, c.Cin, dtype=torch.int8, device=dev)
        Xp[:, 1:-1, 1:-1] = X
        tap, ci = pos // c.Cin, pos % c.Cin
        for t in range(9):              # W[n][(ky * 3 + kx) * Cin + ci], pad 1: output (y, x) reads input (y + ky - 1, x + kx - 1)
            ky, kx = divmod(t, 3)
            add(Xp[:, ky:ky + c.H, kx:kx + c.W].reshape(M, c.Cin), tap == t, ci)
        if c.Cin2:
            add(d["X2"].to(dev), pos >= 9 * c.Cin, pos - 9 * c.Cin)
    else:
        add(d["X"].to(dev), torch.ones_like(pos, dtype=torch.bool), pos)
    Y += d["bias"].to(dev).long()
    if d["rowvec"] is not None:
        Y += d["rowvec"].to(dev).long().repeat_interleave(HW, dim=0)
    if d["R"] is not None:
        Y += d["R"].to(dev).long()
    return Y


def chunk_stats(c, Y, nchunk, rows=None):
    """int64 [B][nchunk][G][2] = (sum, sum of squares) of Y [M][N] per image, chunk and group; rows: the chunk-to-rows map (default: the case's)."""
    cpg = c.N // G
    sq = Y * Y
    out = []
    for t in (Y, sq):
        if (rows or c.rows) == "patch":
            assert nchunk == (c.H // CP_TH) * (c.W // CP_TW)
            s = t.view(c.B, c.H // CP_TH, CP_TH, c.W // CP_TW, CP_TW, G, cpg).sum((2, 4, 6)).reshape(c.B, nchunk, G)
        else:
            assert hw(c) % nchunk == 0
            s = t.view(c.B, nchunk, hw(c) // nchunk, G, cpg).sum((2, 4))
        out.append(s)
    return torch.stack(out, -1)


def exactness_ok(stats):
    """The condition under which fp32 sums of the integers are exact in ANY order: every per-chunk and per-image sum of squares (which bounds every partial sum of
    values and of squares) is below 2^24.  Judged on the int64 reference, never on a kernel's output."""
    per_chunk, per_image = stats[..., 1], stats[..., 1].sum(1)
    return int(per_chunk.max()) < 2 ** 24 and int(per_image.max()) < 2 ** 24
