"""Which kernel every attention gets (csrc/attention.hip attn_pick, asked through ldx_op_attn_pick: host arithmetic, no GPU) against
tests/golden/attn_picks.json, under the default environment and under every LDX_ATTN* switch of the launch path (read once per process, so every
environment runs in a subprocess).  tests/tools/attn_picks.py defines the rows and says how the table was recorded from the launches of the commit
before attn_pick existed.

The rows: SD1.5 self- and cross-attention (8 heads of 40 / 80 / 160, 77 and 154 text tokens) at 16^2 / 64^2 / 128^2 latents with batch 1, 2 and 16; the VAE
mid block (one head of 512, 1024 .. 65536 pixels); CLIP (D 64, causal, 77 tokens); T5 (D 64, bias, 256 and 512 tokens); Flux (24 heads of 128, 4352 and 4608
tokens, 16-bit and MX fp8 output); and a grid over D = 8 .. 160 step 8 and 512, Nq in 77 .. 16384 and Mk in 32 .. 4096 (powers of two and ragged), H * B = 1 ..
512, each plain, without the key-norm workspace, causal, with a bias, with an output row stride that is no multiple of 8, and (D = 128) with MX fp8 output.

Kernel family, template arguments, queries and threads per workgroup, LDS bytes, the key-norm launch, the key splits and the launch count are that
commit's launches on every row of every environment (the grid too: ceil(Nq / queries per workgroup) * H * B * splits, asserted per row when the probe is
asked); mx_out is its attention_mx_out_ok.  Its planner (Engine::n_launches) counted one launch where a key-norm launch runs first: the table holds two."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import attn_picks as A  # noqa: E402


@pytest.fixture(scope="module")
def rows():
    return A.all_rows()


@pytest.fixture(scope="module")
def table():
    return A.load_table()


def test_table_covers_the_rows_and_every_kernel_family(rows, table):
    assert table["fields"] == list(A.FIELDS) and table["families"] == list(A.FAMILIES)
    assert table["n_rows"] == len(rows) and table["rows_sha256"] == A.rows_digest(rows), "the grid changed: regenerate with tests/tools/attn_picks.py --write"
    assert set(table["envs"]) == {A.env_key(e) for e in A.ENVS}
    for key in table["envs"]:
        assert len(A.decode(table, key)) == len(rows), key
    default = [dict(zip(A.FIELDS, p)) for p in A.decode(table, "default")]
    assert {p["family"] for p in default} == set(range(len(A.FAMILIES))), "a kernel family that no row of the default environment reaches"
    assert any(p["knorm"] and p["launches"] == 2 for p in default), "no row with a key-norm launch"
    assert any(p["nsplit"] > 1 and p["launches"] == 2 for p in default), "no row with split keys and a merge launch"
    assert any(p["mx_out"] for p in default)


@pytest.mark.parametrize("env", A.ENVS, ids=A.env_key)
def test_picks_match_the_table(ldx_lib, rows, table, env):
    picks = A.picks_of_env(env)
    want = A.decode(table, A.env_key(env))
    assert len(picks) == len(want) == len(rows)
    bad = [i for i in range(len(rows)) if picks[i] != want[i]]
    for i in bad[:10]:
        print(A.describe(rows[i], picks[i]), " table:", want[i])
    assert not bad, f"{len(bad)} of {len(rows)} rows differ from tests/golden/attn_picks.json"


def test_probe_rejects_bad_arguments(ldx_lib):
    import ctypes as C
    out = (C.c_int32 * len(A.OUT))()
    assert ldx_lib.ldx_op_attn_pick(*A.attn(2, 8, 1024, 1024, 40), out) == 0
    assert ldx_lib.ldx_op_attn_pick(*A.attn(2, 8, 1024, 1024, 40), None) != 0
    assert ldx_lib.ldx_op_attn_pick(*A.attn(0, 8, 1024, 1024, 40), out) != 0
    assert ldx_lib.ldx_op_attn_pick(*A.attn(2, 8, 0, 1024, 40), out) != 0
    assert ldx_lib.ldx_op_attn_pick(*A.attn(2, 8, 1024, 1024, 44), out) != 0           # D % 8
    assert ldx_lib.ldx_op_attn_pick(*A.attn(2, 8, 1024, 1024, 168), out) != 0          # 160 < D != 512
    assert ldx_lib.ldx_op_attn_pick(*A.attn(2, 8, 1024, 1024, 80, o8=1), out) != 0     # MX fp8 output: D = 128 only
