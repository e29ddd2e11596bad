"""Which kernel every GEMM / convolution gets: the host-side decision of csrc/gemm.hip (gemm_pick, asked through ldx_op_gemm_pick — no GPU needed)
over the layer shapes of the six models and a systematic grid, under the default environment and under the tile / ping-pong / fusion switches.

The committed table (tests/golden/gemm_picks.json) was recorded from the launches of the commit BEFORE gemm_pick existed (every kernel launch of its
launch_gemm / launch_gemm2 intercepted in a host-only build: kernel name with its template arguments, grid, the reduce launch; its gemm_gn_fuse for the
chunk count), so tests/test_gemm_pick_cpu.py holds the dispatcher to what that commit launched, row for row.  The one exception is the chunk count of 175
conv rows under a forced LDX_GEMM_TILE whose width the conv kernels do not have: that commit's planner answered for the requested width while its launcher ran
a narrower tile (and mostly aborted on the mismatch); the table holds the answer for the tile that is launched.

    python tests/tools/gemm_picks.py            # summary of the current build's picks against the table
    python tests/tools/gemm_picks.py --write    # accept the current build's picks as the new table (after LOOKING at what moved, and why)
    python tests/tools/gemm_picks.py --dump     # the encoded picks of the current environment on stdout (what the test's subprocesses run)
    python tests/tools/gemm_picks.py --rows     # the rows themselves, one per line (the probe's integer arguments)
    python tests/tools/gemm_picks.py --show     # the committed table, readable: every row of every environment with its pick
"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pick_table import ROOT, decode, env_key, load_lib, rows_digest  # noqa: E402,F401  (the test asks this module for them)
import pick_table  # noqa: E402

TABLE = os.path.join(ROOT, "tests", "golden", "gemm_picks.json")

FAMILIES = ("tile", "tile2", "pingpong", "pingpong2", "ring", "conv_patch", "tile_mx", "tile2_mx", "pingpong_mx", "pingpong2_mx")      # GemmFamily (ldx_kernels.h)
REDUCE = ("none", "reduce", "reduce_gn", "in_kernel")
OUT = ("family", "bm", "bn", "wm", "f8", "lnf", "S", "reduce", "launches", "gn_chunks")      # ldx_op_gemm_pick's output array
FIELDS = ("family", "bm", "bn", "S", "reduce", "launches", "gn_chunks")                          # what the table holds
ENVS = [{}] + [{"LDX_GEMM_TILE": t} for t in ("256128", "256160", "256192", "256224", "256256", "64160")] + [{"LDX_PP": "0"}, {"LDX_PP": "2"}, {"LDX_GN_FUSE": "0"}]
GN_MAX = 256      # chunks per image the engine's GroupNorm workspace holds


# ---- rows: the probe's arguments (M, N, K, mode, geglu, splitk, f8, c8, ln_fold, Cin, Hin, Win, Hout, Wout, stride, M2, N2, K2, gn_hw, gn_groups, gn_max_chunks)
def gemm(M, N, K, geglu=0, lnf=0, f8=0, c8=0, pair=None, gn_hw=0):
    M2, N2, K2 = pair or (0, 0, 0)
    return (M, N, K, 0, geglu, 1 if lnf else -1, f8, c8, lnf, 0, 0, 0, 0, 0, 0, M2, N2, K2, gn_hw, 32 if gn_hw else 0, GN_MAX if gn_hw else 0)


def conv(B, Hin, Win, Cin, Cout, stride=1, up=1, Cin2=0, gn=True):
    Hout, Wout = Hin * up // stride, Win * up // stride
    hw = Hout * Wout if gn and Cout % 32 == 0 else 0
    return (B * Hout * Wout, Cout, 9 * Cin + Cin2, 1, 0, -1, 0, 0, 0, Cin, Hin, Win, Hout, Wout, stride, 0, 0, 0, hw, 32 if hw else 0, GN_MAX if hw else 0)


def sd15(L, B):
    """SD1.5 UNet at an L x L latent, CFG batch B: 3x3 convs (with the fused 1x1 skip, the down / up samplers) and the transformer blocks' projections."""
    rows = []
    cins = ((320, 640, 960), (320, 640, 960, 1280, 1920), (640, 1280, 1920, 2560), (1280, 2560))      # encoder, and decoder inputs with the skip concatenated
    for lvl, c in enumerate((320, 640, 1280, 1280)):
        h = L >> lvl
        for cin in cins[lvl]:
            rows.append(conv(B, h, h, cin, c))
            if cin != c:
                rows.append(conv(B, h, h, c, c, Cin2=cin))      # ResBlock conv2 + 1x1 skip as one implicit GEMM
        if lvl < 3:
            rows += [conv(B, h, h, c, c, stride=2), conv(B, h // 2, h // 2, c, c, up=2)]
            M = B * h * h
            rows += [gemm(M, c, c, gn_hw=h * h), gemm(M, 3 * c, c, lnf=1), gemm(M, c, c, lnf=1), gemm(M, c, c), gemm(M, 8 * c, c, geglu=1, lnf=1),
                     gemm(M, 8 * c, c, geglu=1), gemm(M, c, 4 * c), gemm(B * 77, 2 * c, 768), gemm(B * 77, c, 768)]
    rows += [conv(B, L, L, 64, 320, gn=False), conv(B, L, L, 320, 4, gn=False)]
    return rows


def vae(px):
    """VAE decoder / encoder at px x px pixels: 512 -> 512 -> 256 -> 128 channels from px / 8 up, the mid block's single-head attention projections."""
    rows, h = [], px // 8
    rows += [conv(1, h, h, 64, 512), gemm(h * h, 512, 512), gemm(h * h, 1536, 512), gemm(h * h, 512, 512, gn_hw=h * h)]
    for lvl, (cin, c) in enumerate(((512, 512), (512, 512), (512, 256), (256, 128))):
        hh = h << lvl
        rows += [conv(1, hh, hh, cin, c), conv(1, hh, hh, c, c)]
        if cin != c:
            rows.append(conv(1, hh, hh, c, c, Cin2=cin))
        if lvl < 3:
            rows.append(conv(1, hh, hh, c, c, up=2))                # decoder upsample
            rows.append(conv(1, hh * 2, hh * 2, c, c, stride=2))    # encoder downsample
    rows += [conv(1, px, px, 128, 3, gn=False), conv(1, px, px, 64, 128)]
    return rows


def text_encoders():
    rows = []
    for M in (77, 154, 1232):                                    # CLIP-L
        rows += [gemm(M, 2304, 768, lnf=1), gemm(M, 2304, 768), gemm(M, 768, 768), gemm(M, 3072, 768, lnf=1), gemm(M, 3072, 768), gemm(M, 768, 3072)]
    for M in (256, 512):                                          # T5-XXL
        rows += [gemm(M, 12288, 4096), gemm(M, 4096, 4096), gemm(M, 20480, 4096, geglu=2), gemm(M, 4096, 10240)]
    return rows


def flux(L=4352, txt=256):
    rows = []
    img = L - txt
    for f8, c8s in ((0, (0,)), (1, (0, 1))):                      # bf16, MX fp8 operands, MX fp8 with the quantised output fused
        for c8 in c8s:
            for M in (img, txt, L):
                rows += [gemm(M, 9216, 3072, f8=f8, c8=c8), gemm(M, 3072, 3072, f8=f8), gemm(M, 12288, 3072, f8=f8, c8=c8), gemm(M, 3072, 12288, f8=f8),
                         gemm(M, 21504, 3072, f8=f8, c8=c8), gemm(M, 3072, 15360, f8=f8)]
            for N, K in ((9216, 3072), (3072, 3072), (12288, 3072), (3072, 12288)):      # the two streams of a double block as one launch
                rows.append(gemm(img, N, K, f8=f8, c8=c8, pair=(txt, N, K)))
            rows.append(gemm(L, 9216, 3072, f8=f8, c8=c8, pair=(L, 12288, 3072)))         # the two halves of a single block's linear1
    return rows


def esrgan(t=512):
    rows = []
    for cin in (64, 128, 192, 256, 320):                          # dense-block inputs 64 + 32 k, padded to whole 64-channel segments
        rows.append(conv(1, t, t, cin, 32, gn=False))
    rows += [conv(1, t, t, 320, 64, gn=False), conv(1, t, t, 64, 64, gn=False), conv(1, 2 * t, 2 * t, 64, 64, gn=False, up=1), conv(1, t, t, 64, 64, up=2, gn=False),
             conv(1, 4 * t, 4 * t, 64, 64, gn=False), conv(1, 4 * t, 4 * t, 64, 3, gn=False)]
    return rows


def grid():
    Ms = [1 << i for i in range(18)] + [77, 333, 1025, 4095, 16385, 131071]
    Ns = (32, 64, 128, 160, 320, 640, 1280, 2560, 3072, 5120, 10240)
    Ks = (64, 320, 1280, 2880, 5760, 11520, 3072, 12288)
    rows = []
    for M in Ms:
        B = 2 if M % 2 == 0 and M >= 128 else 1
        hw = M // B
        for N in Ns:
            for K in Ks:
                rows.append(gemm(M, N, K, gn_hw=hw))
                rows.append(gemm(M, N, K, lnf=1))
                rows.append(gemm(M, N, K, pair=(512, N, K)))
                if N % 128 == 0:                                  # GEGLU pairs value / gate columns inside 64-column slabs
                    rows += [gemm(M, N, K, geglu=1), gemm(M, N, K, geglu=1, lnf=1)]
                if K % 128 == 0:                                  # MX fp8 operands: 128 elements per K-tile
                    rows += [gemm(M, N, K, f8=1), gemm(M, N, K, f8=1, pair=(512, N, K))]
                    if N % 128 == 0:
                        rows += [gemm(M, N, K, f8=1, c8=1), gemm(M, N, K, f8=1, c8=1, pair=(512, N, K))]
                if K % 576 == 0 and M >= 64 and M & (M - 1) == 0:      # 3x3 conv over Cin = K / 9 channels: B images of H x W = M / B pixels
                    e = hw.bit_length() - 1
                    rows.append(conv(B, 1 << (e + 1) // 2, 1 << e // 2, K // 9, N))
    return rows


def all_rows():
    rows = []
    for L in (64, 128, 16):
        for B in (2, 16):
            rows += sd15(L, B)
    rows += vae(512) + vae(2048) + text_encoders() + flux() + esrgan() + grid()
    return rows


# ---- asking the library
def picks_of_current_env(rows):
    """[(family, bm, bn, S, reduce, launches, gn_chunks)] of this process's environment (the switches are read once, when the library loads)."""
    L = load_lib()
    out = (C.c_int32 * len(OUT))()
    keep = [OUT.index(f) for f in FIELDS]
    res = []
    for r in rows:
        rc = L.ldx_op_gemm_pick(*r, out)
        assert rc == 0, (r, rc)
        res.append(tuple(out[i] for i in keep))
    return res


def picks_of_env(env):
    return pick_table.picks_of_env(__file__, env)


def load_table():
    return pick_table.load_table(TABLE)


def write_table(per_env, rows, path=TABLE):
    return pick_table.write_table(path, per_env, rows, fields=list(FIELDS), families=list(FAMILIES), reduce=list(REDUCE))


def describe(row, pick):
    p = dict(zip(FIELDS, pick))
    return f"{row} -> {FAMILIES[p['family']]} {p['bm']}x{p['bn']} S={p['S']} {REDUCE[p['reduce']]} launches={p['launches']} gn_chunks={p['gn_chunks']}"


if __name__ == "__main__":
    pick_table.cli(sys.modules[__name__])
