"""What every SpatialTransformer of a UNet plan runs as (csrc/engine.cpp xf_pick, asked through ldx_op_xf_pick: host arithmetic, no GPU) against
tests/golden/xf_picks.json, under the default environment and under every planner switch (read once per process, so every environment runs in a
subprocess).  tests/tools/xf_picks.py defines the rows — the transformers of four UNets' plans over latents, batches, context lengths, LDX_LNFOLD and the
shared CFG prefix — and says how the table was recorded against the planner of the commit before xf_pick existed."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import xf_picks as X  # noqa: E402


@pytest.fixture(scope="module")
def rows():
    return X.all_rows()


@pytest.fixture(scope="module")
def table():
    return X.load_table()


def test_table_covers_the_rows_and_every_stage_choice(rows, table):
    assert table["fields"] == list(X.FIELDS) and table["stages"] == list(X.STAGES)
    assert table["n_rows"] == len(rows) and table["rows_sha256"] == X.rows_digest(rows), "the rows changed: regenerate with tests/tools/xf_picks.py --write"
    assert set(table["envs"]) == {X.env_key(e) for e in X.ENVS}
    for key in table["envs"]:
        assert len(X.decode(table, key)) == len(rows), key
    default = [dict(zip(X.FIELDS, p)) for p in X.decode(table, "default")]
    # every stage but one is reached: no projection of these nets is split-K, so "ln+folded" (an affine-free LayerNorm in front of a split-K folded GEMM) never runs
    for f, want in (("first.qkv", {1, 2, 3}), ("first.q2", {1, 2, 3}), ("first.ff1", {2, 3})):
        assert {p[f] for p in default} == want, f"{f}: a stage that no row of the default environment reaches"
    for f in ("proj_out", "first.o1", "first.o2", "fold", "proj_in_rowgemm", "first.xattn", "first.ffblock"):
        assert {p[f] for p in default} == {0, 1}, f
    # by default the prefix limit is half the full-batch limit, so the first block (half the rows) decides like the later ones; without a prefix limit they part
    assert not any(p["first.qkv"] != p["rest.qkv"] or p["first.o1"] != p["rest.o1"] for p in default)
    no_prefix_limit = [dict(zip(X.FIELDS, p)) for p in X.decode(table, "LDX_ROWBLOCK_MINWG_PREFIX=0")]
    assert any(p["first.qkv"] == 1 and p["rest.qkv"] != 1 and r[5] > 0 for r, p in zip(rows, no_prefix_limit)), "no shared-prefix row whose first block alone runs row blocks"
    assert not any(p["fold"] for p in X.decode(table, "LDX_LNFOLD_MAXROWS=0") for p in [dict(zip(X.FIELDS, p))])


@pytest.mark.parametrize("env", X.ENVS, ids=X.env_key)
def test_picks_match_the_table(ldx_lib, rows, table, env):
    picks = X.picks_of_env(env)
    want = X.decode(table, X.env_key(env))
    assert len(picks) == len(want) == len(rows)
    bad = [i for i in range(len(rows)) if picks[i] != want[i]]
    for i in bad[:10]:
        print(X.describe(rows[i], picks[i]), " table:", want[i])
    assert not bad, f"{len(bad)} of {len(rows)} rows differ from tests/golden/xf_picks.json"


def test_probe_rejects_bad_arguments(ldx_lib):
    out = (C.c_int32 * len(X.FIELDS))()
    good = (320, 8, 2, 4096, 77, 1, 1, 32)
    assert ldx_lib.ldx_op_xf_pick(*good, out) == 0
    assert ldx_lib.ldx_op_xf_pick(*good, None) != 0
    for i in (0, 1, 2, 3, 4):                                   # C, heads, B, HW, Mc: positive
        for v in (0, -1):
            assert ldx_lib.ldx_op_xf_pick(*(good[:i] + (v,) + good[i + 1:]), out) != 0, (i, v)
    assert ldx_lib.ldx_op_xf_pick(320, 7, 2, 4096, 77, 0, 1, 0, out) != 0          # C % heads
    assert ldx_lib.ldx_op_xf_pick(320, 8, 2, 4096, 77, -1, 1, 0, out) != 0         # share < 0
    assert ldx_lib.ldx_op_xf_pick(320, 8, 2, 4096, 77, 3, 1, 0, out) != 0          # share > B
    assert ldx_lib.ldx_op_xf_pick(320, 8, 2, 4096, 77, 0, 1, -1, out) != 0         # chunks < 0
