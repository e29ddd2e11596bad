"""Which kernel every GEMM / convolution gets (csrc/gemm.hip gemm_pick, asked through ldx_op_gemm_pick: host arithmetic, no GPU) against
tests/golden/gemm_picks.json — the layer shapes of the six models and a systematic grid, under the default environment and under the tile /
ping-pong / fusion switches (read once per process, so every environment runs in a subprocess).  tests/tools/gemm_picks.py defines the rows and
says how the table was recorded from the launches of the commit before gemm_pick existed.

family, BM, BN, split count, reduce kind and launch count are that commit's on every row of every environment.  The GroupNorm chunk count is that
commit's gemm_gn_fuse on all but 175 of the 142 440 rows, all of them 3x3 convs under a forced LDX_GEMM_TILE whose width the conv kernels do not have
(256192: 47 rows, 256224: 26, 64160: 102): there its planner judged the requested tile while its launcher ran a 128- or 64-wide one — 101 of those
launches ended in the geometry abort — and the table holds what the launched tile's epilogue supports."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import gemm_picks as G  # noqa: E402


@pytest.fixture(scope="module")
def rows():
    return G.all_rows()


@pytest.fixture(scope="module")
def table():
    return G.load_table()


def test_table_covers_the_rows_and_every_kernel_family(rows, table):
    assert table["fields"] == list(G.FIELDS) and table["families"] == list(G.FAMILIES)
    assert table["n_rows"] == len(rows) and table["rows_sha256"] == G.rows_digest(rows), "the grid changed: regenerate with tests/tools/gemm_picks.py --write"
    assert set(table["envs"]) == {G.env_key(e) for e in G.ENVS}
    for key in table["envs"]:
        assert len(G.decode(table, key)) == len(rows), key
    fam, red = G.FIELDS.index("family"), G.FIELDS.index("reduce")
    default = G.decode(table, "default")
    assert {p[fam] for p in default} == set(range(len(G.FAMILIES))), "a kernel family that no row of the default environment reaches"
    assert {p[red] for p in default} >= {0, 1, 2}, "no row with a reduce launch / a reduce + GroupNorm launch"
    assert any(p[G.FIELDS.index("gn_chunks")] for p in default)


@pytest.mark.parametrize("env", G.ENVS, ids=G.env_key)
def test_picks_match_the_table(ldx_lib, rows, table, env):
    picks = G.picks_of_env(env)
    want = G.decode(table, G.env_key(env))
    assert len(picks) == len(want) == len(rows)
    bad = [i for i in range(len(rows)) if picks[i] != want[i]]
    for i in bad[:10]:
        print(G.describe(rows[i], picks[i]), " table:", want[i])
    assert not bad, f"{len(bad)} of {len(rows)} rows differ from tests/golden/gemm_picks.json"


def test_probe_rejects_bad_arguments(ldx_lib):
    import ctypes as C
    out = (C.c_int32 * len(G.OUT))()
    assert ldx_lib.ldx_op_gemm_pick(*G.gemm(0, 320, 320), out) != 0
    assert ldx_lib.ldx_op_gemm_pick(*G.gemm(64, 320, 320), None) != 0
