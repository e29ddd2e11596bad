"""Which kernel every attention gets: the host-side decision of csrc/attention.hip (attn_pick, asked through ldx_op_attn_pick — no GPU needed) over the attention shapes
of the models and a systematic grid, under the default environment and under every LDX_ATTN* switch of the launch path.

The committed table (tests/golden/attn_picks.json) was recorded from the launches of the commit BEFORE attn_pick existed: every kernel launch behind its launch_attention
intercepted in a host-only build (kernel name with its template arguments, grid, block, LDS bytes, in launch order, for bf16 and f16), compared with the same interception
of the build that has attn_pick and with what the pick says (kernel, grid = ceil(Nq / queries per workgroup) * H * B * splits, block, LDS bytes, a key-norm launch in front,
a merge launch behind) on every row of every environment.  So tests/test_attn_pick_cpu.py holds the dispatcher to what that commit launched, row for row.

    python tests/tools/attn_picks.py            # summary of the current build's picks against the table
    python tests/tools/attn_picks.py --write    # accept the current build's picks as the new table (after LOOKING at what moved, and why)
    python tests/tools/attn_picks.py --dump     # the encoded picks of the current environment on stdout (what the test's subprocesses run)
    python tests/tools/attn_picks.py --rows     # the rows themselves, one per line (the probe's integer arguments)
    python tests/tools/attn_picks.py --show     # the committed table, readable: every row of every environment with its pick
"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pick_table import ROOT, decode, env_key, load_lib, rows_digest  # noqa: E402,F401  (the test asks this module for them)
import pick_table  # noqa: E402

TABLE = os.path.join(ROOT, "tests", "golden", "attn_picks.json")

FAMILIES = ("attn", "attn32", "attn32ap", "attn32g", "attn40p", "attn128p", "attn512")      # AttnFamily (ldx_kernels.h)
OUT = ("family", "t0", "t1", "t2", "kpf", "qb", "block", "grid", "lds", "knorm", "nsplit", "mx_out", "launches")      # ldx_op_attn_pick's output array
FIELDS = ("family", "t0", "t1", "t2", "kpf", "qb", "block", "lds", "knorm", "nsplit", "mx_out", "launches")          # what the table holds: all but the grid, which is
#                                                                                         ceil(Nq / qb) * H * B * nsplit on every row (picks_of_current_env asserts it)
ENVS = ([{}] + [{k: "0"} for k in ("LDX_ATTN_PIPE", "LDX_ATTN_PIPE128", "LDX_ATTN_PIPE_KB", "LDX_ATTN32", "LDX_ATTN_KPF", "LDX_ATTN512")]
        + [{k: "1"} for k in ("LDX_ATTN_PIPE_MINWG", "LDX_ATTN32_AP_MINWG", "LDX_ATTN32G_MINWG")]
        + [{"LDX_ATTN_PIPE_THR": "0.5"}]
        + [{"LDX_ATTN_PIPE": "0", "LDX_ATTN32_AP": v} for v in ("0", "2", "3")]              # the D = 40 kernels behind the pipelined one
        + [{"LDX_ATTN_PIPE": "0", "LDX_ATTN32_AP": "0", "LDX_ATTN32_VAR": "0"}, {"LDX_ATTN_PIPE": "0", "LDX_ATTN32_AP": "0", "LDX_ATTN32_VAR": "0", "LDX_ATTN32_KVB": "128"}]
        + [{"LDX_ATTN32G": v} for v in ("0", "8", "15")]
        + [{"LDX_ATTN_PIPE128": "0", "LDX_ATTN32G": "0"}, {"LDX_ATTN512_SPLITS": "4"}])


# ---- rows: the probe's arguments (B, H, Nq, Mk, D, causal, bias, o8, ldq, ldk, ldv, ldo, knorm_ws)
def attn(B, H, Nq, Mk, D, causal=0, bias=0, o8=0, ws=1, ldo_pad=0):
    """Self-attention reads q | k | v from one projection (row stride 3 H D), cross-attention q from one and k | v from another."""
    C_ = H * D
    ldq, ldkv = (3 * C_, 3 * C_) if Nq == Mk else (C_, 2 * C_)
    return (B, H, Nq, Mk, D, causal, bias, o8, ldq, ldkv, ldkv, C_ + ldo_pad, ws)


def sd15(L, B):
    """SD1.5 UNet at an L x L latent, batch B: 8 heads of 40 / 80 / 160 over the three levels (and 160 in the middle), against themselves and 77 / 154 text tokens."""
    rows = []
    for lvl, D in enumerate((40, 80, 160, 160)):
        N = (L >> lvl) ** 2
        if N:
            rows += [attn(B, 8, N, N, D), attn(B, 8, N, 77, D), attn(B, 8, N, 154, D)]
    return rows


def grid():
    rows = []
    for D in list(range(8, 161, 8)) + [512]:
        for H, B in ((1, 1), (8, 1), (8, 2), (16, 4), (8, 16), (16, 16), (16, 32)):
            for Nq in (77, 256, 1000, 1024, 2000, 4096, 16384):
                for Mk in (32, 77, 128, 256, 1000, 4096):
                    rows += [attn(B, H, Nq, Mk, D), attn(B, H, Nq, Mk, D, ws=0), attn(B, H, Nq, Mk, D, causal=1), attn(B, H, Nq, Mk, D, bias=1), attn(B, H, Nq, Mk, D, ldo_pad=4)]
                    if D == 128:
                        rows += [attn(B, H, Nq, Mk, D, o8=1), attn(B, H, Nq, Mk, D, o8=1, ws=0)]
    return rows


def all_rows():
    rows = []
    for L in (16, 64, 128):
        for B in (1, 2, 16):
            rows += sd15(L, B)
    rows += [attn(1, 1, N, N, 512) for N in (1024, 4096, 16384, 65536)] + [attn(2, 1, 4096, 4096, 512)]      # the VAE's mid block, 256^2 .. 2048^2 pixels
    rows += [attn(B, 12, 77, 77, 64, causal=1) for B in (1, 2, 16)]                                          # CLIP-L
    rows += [attn(1, 64, N, N, 64, bias=1) for N in (256, 512)]                                              # T5-XXL
    rows += [attn(1, 24, N, N, 128, o8=o8) for N in (4352, 4096 + 512) for o8 in (0, 1)]                     # Flux: 1024^2 image + 256 / 512 text tokens
    return rows + grid()


# ---- asking the library
def picks_of_current_env(rows):
    """[FIELDS] of this process's environment (the switches are read once, when the library loads)."""
    L = load_lib()
    out = (C.c_int32 * len(OUT))()
    keep = [OUT.index(f) for f in FIELDS]
    res = []
    for r in rows:
        rc = L.ldx_op_attn_pick(*r, out)
        assert rc == 0, (r, rc)
        p = dict(zip(OUT, out))
        assert p["grid"] == -(-r[2] // p["qb"]) * r[1] * r[0] * p["nsplit"], (r, p)
        res.append(tuple(out[i] for i in keep))
    return res


def picks_of_env(env):
    return pick_table.picks_of_env(__file__, env)


def load_table():
    return pick_table.load_table(TABLE)


def write_table(per_env, rows, path=TABLE):
    return pick_table.write_table(path, per_env, rows, fields=list(FIELDS), families=list(FAMILIES))


def kernel_name(p):
    """The device kernel's name as the profiler shows it, the element type aside."""
    f, t = FAMILIES[p["family"]], (p["t0"], p["t1"], p["t2"])
    args = {"attn": f"{t[0]}, {t[1]}, {t[2]}", "attn32": f"{t[0]}, 144, 192, {t[1]}", "attn32ap": f"144, 192, {t[0]}",
            "attn32g": f"{t[0]}, {t[1]}, 1, {'true' if t[2] else 'false'}, {'true' if p['kpf'] else 'false'}"}.get(f)
    return f"{f}_kernel<T{', ' + args if args else ''}>"


def describe(row, pick):
    p = dict(zip(FIELDS, pick))
    return (f"{row} -> {kernel_name(p)} {p['qb']} queries x {p['block']} threads, {p['lds']} B LDS{' knorm' if p['knorm'] else ''}"
            f"{' splits=%d' % p['nsplit'] if p['family'] == 6 else ''} mx_out={p['mx_out']} launches={p['launches']}")


if __name__ == "__main__":
    pick_table.cli(sys.modules[__name__])
