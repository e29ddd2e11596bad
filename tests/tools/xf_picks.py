"""What every SpatialTransformer of a UNet plan runs as: the host-side stage choice of csrc/engine.cpp (xf_pick, asked through ldx_op_xf_pick — no GPU needed) over the
transformers of real UNet plans, under the default environment and under every planner switch (PlanSwitches, ldx_kernels.h; LDX_GN_FUSE because it decides whether
norm + proj_in ever see producer statistics).

The rows are the transformers of four UNets (CONFIGS: SD1.5, the narrow net of tests/test_engine_gpu.py with no transformer at level 0, a two-level net of 320 / 640
channels and a three-level one of 64 / 320 / 640, so that 320 and 640 also appear at low resolution) at latents of 16^2 .. 256^2 and 40 x 24 (pixel counts that are no
multiple of 128), evaluation batches 1 .. 32, 77 and 154 context tokens, with and without the folded LayerNorm weights (LDX_LNFOLD), on the full batch and — the first
transformer of a net — behind a shared CFG prefix of half the batch; each with no producer statistics and with every chunk count a producer writes from its tiles of
64 .. 512 rows or from its split-K reduce launch (4 .. 48 rows per chunk).

The committed table (tests/golden/xf_picks.json) was recorded from the probe after the planner of the commit BEFORE xf_pick existed and the one built on it were compared
in a host-only build (HIP entry points replaced by host stand-ins, every launch recorded): op lists, arguments, arena offsets, flops and launches of every plan of those
nets were identical in every environment, and the probe said what the op list of every transformer showed.  So tests/test_xf_pick_cpu.py holds the planner to what that
commit planned, row for row.

    python tests/tools/xf_picks.py            # summary of the current build's picks against the table
    python tests/tools/xf_picks.py --write    # accept the current build's picks as the new table (after LOOKING at what moved, and why)
    python tests/tools/xf_picks.py --dump     # the encoded picks of the current environment on stdout (what the test's subprocesses run)
    python tests/tools/xf_picks.py --rows     # the rows themselves, one per line (the probe's integer arguments)
    python tests/tools/xf_picks.py --show     # the committed table, readable: every row of every environment with its pick
"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pick_table import ROOT, decode, env_key, load_lib, rows_digest  # noqa: E402,F401  (the test asks this module for them)
import pick_table  # noqa: E402

TABLE = os.path.join(ROOT, "tests", "golden", "xf_picks.json")

STAGES = ("tile", "rowblock", "folded", "ln+gemm", "ln+folded")      # XfStage (ldx_kernels.h)
BLOCK = ("qkv", "o1", "xattn", "q2", "o2", "ffblock", "ff1", "ops")
FIELDS = ("fold", "proj_in_rowgemm", "proj_out") + tuple(f"first.{f}" for f in BLOCK) + tuple(f"rest.{f}" for f in BLOCK) + ("ops_outer",)      # ldx_op_xf_pick's output array
ENVS = ([{}] + [{k: "0"} for k in ("LDX_ROWGEMM", "LDX_ROWGEMM640", "LDX_XATTN_FUSE", "LDX_FF_FUSE", "LDX_ROWGEMM_X2", "LDX_ROWGEMM_PO", "LDX_GN_FUSE")]
        + [{"LDX_ROWBLOCK_MINWG": "0"}, {"LDX_ROWBLOCK_MINWG_PREFIX": "0"}, {"LDX_ROWGEMM_PLAIN640_MAXM": "0"}, {"LDX_LNFOLD_MAXROWS": "0"},
           {"LDX_LNFOLD_MAXROWS": "100000000"}])          # the last: every level folds

# keyword arguments of ldx_amd.UNetConfig
CONFIGS = {
    "sd15": dict(),
    "no_xf_at_level0": dict(model_channels=64, context_dim=128, transformer_depth=(0, 0, 1, 1, 1, 1, 0, 0), transformer_depth_output=(1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0)),
    "two_level_320": dict(model_channels=320, channel_mult=(1, 2), num_res_blocks=(1, 1), transformer_depth=(1, 1), transformer_depth_output=(1, 1, 1, 1)),
    "three_level_64": dict(model_channels=64, channel_mult=(1, 5, 10), num_res_blocks=(1, 1, 1), transformer_depth=(1, 1, 1), transformer_depth_output=(1, 1, 1, 1, 1, 1)),
}
DEFAULTS = dict(model_channels=320, channel_mult=(1, 2, 4, 4), num_res_blocks=(2, 2, 2, 2), transformer_depth=(1, 1, 1, 1, 1, 1, 0, 0),
                transformer_depth_output=(1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0), transformer_depth_middle=1, num_heads=8)      # UNetConfig's own (SD1.5)
LATENTS = ((16, 16), (32, 32), (64, 64), (96, 96), (128, 128), (256, 256), (40, 24))
BATCHES = (1, 2, 4, 16, 32)
CONTEXTS = (77, 154)


def transformers(cfg):
    """(C, level) of every SpatialTransformer in plan order: the structure walk of UNetModel1.__init__ as the engine's constructor does it."""
    c = dict(DEFAULTS, **cfg)
    mc, mult, nres = c["model_channels"], c["channel_mult"], c["num_res_blocks"]
    out, td = [], iter(c["transformer_depth"])
    for level in range(len(mult)):
        out += [(mult[level] * mc, level) for _ in range(nres[level]) if next(td) > 0]
    if c["transformer_depth_middle"] >= 1:
        out.append((mult[-1] * mc, len(mult) - 1))
    tdo = list(c["transformer_depth_output"])[:sum(n + 1 for n in nres)]
    for level in reversed(range(len(mult))):
        out += [(mult[level] * mc, level) for _ in range(nres[level] + 1) if tdo.pop() > 0]
    return out


def all_rows():
    """The probe's arguments: (C, heads, B, HW, Mc, share, ln_fold, gn_stats_chunks)."""
    rows = []
    for cfg in CONFIGS.values():
        xfs, heads = transformers(cfg), dict(DEFAULTS, **cfg)["num_heads"]
        for (h, w) in LATENTS:
            hw = [h * w]
            for _ in range(8):
                h, w = (h + 1) // 2, (w + 1) // 2
                hw.append(h * w)
            shapes = sorted(set((c, hw[lv]) for c, lv in xfs))
            first = (xfs[0][0], hw[xfs[0][1]])          # a shared CFG prefix ends inside the first transformer of the net
            for B in BATCHES:
                for c, n, share in [(c, n, 0) for c, n in shapes] + ([first + (B // 2,)] if B % 2 == 0 else []):
                    # none; what a producer's tiles of 64 .. 512 rows write; what its split-K reduce launch writes (chunks of 4 .. 48 rows, at most 256 of them)
                    chunks = [0] + [n // t for t in (64, 128, 256, 512) if n % t == 0] + [n // t for t in (4, 8, 12, 16, 48) if n % t == 0 and n // t <= 256]
                    rows += [(c, heads, B, n, mc, share, lf, ch) for mc in CONTEXTS for lf in (0, 1) for ch in chunks]
    return sorted(set(rows))


# ---- asking the library
def picks_of_current_env(rows):
    """[FIELDS] of this process's environment (the switches are read once, when the library loads)."""
    L = load_lib()
    out = (C.c_int32 * len(FIELDS))()
    res = []
    for r in rows:
        rc = L.ldx_op_xf_pick(*r, out)
        assert rc == 0, (r, rc)
        res.append(tuple(out))
    return res


def picks_of_env(env):
    return pick_table.picks_of_env(__file__, env)


def load_table():
    return pick_table.load_table(TABLE)


def write_table(per_env, rows, path=TABLE):
    return pick_table.write_table(path, per_env, rows, fields=list(FIELDS), stages=list(STAGES))


def describe(row, pick):
    p = dict(zip(FIELDS, pick))

    def block(k):
        b = {f: p[f"{k}.{f}"] for f in BLOCK}
        x = "xattn_block" if b["xattn"] else f"q2 {STAGES[b['q2']]} + attn2 + o2 {STAGES[b['o2']]}"
        f = "ff_block" if b["ffblock"] else f"ff1 {STAGES[b['ff1']]} + ff2"
        return f"qkv {STAGES[b['qkv']]} + attn1 + o1 {STAGES[b['o1']]} | {x} | {f} ({b['ops']} ops)"
    return (f"{row} -> {'fold ' if p['fold'] else ''}proj_in {'rowgemm' if p['proj_in_rowgemm'] else 'gn+gemm'}, proj_out {STAGES[p['proj_out']]} ({p['ops_outer']} ops); "
            f"first: {block('first')}; rest: {block('rest')}")


if __name__ == "__main__":
    pick_table.cli(sys.modules[__name__])
