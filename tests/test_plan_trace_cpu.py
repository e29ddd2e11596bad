"""What every engine plans and launches — kernels, grids, LDS sizes and every argument byte, recorded without a GPU by the host-only build of the library against a
stand-in HIP runtime (tests/tools/plan_trace.py says how, and lists the cases and environments) — against tests/golden/plan_traces.json.  A change to the planner or to
the layer between the plans and the launchers that is meant to leave behaviour alone leaves this table alone."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import plan_trace as T  # noqa: E402


@pytest.fixture(scope="module")
def rows():
    return T.all_rows()


@pytest.fixture(scope="module")
def table():
    return T.load_table()


@pytest.fixture(scope="module")
def traces(ldx_lib):
    """The digests of every environment: one fresh process each (the switches are read once per process), several at a time."""
    T.build_host()
    return T.picks_of_envs(T.ENVS)


def test_table_covers_the_cases(rows, table):
    assert table["fields"] == list(T.FIELDS)
    assert table["n_rows"] == len(rows) and table["rows_sha256"] == T.rows_digest(rows), "the cases changed: regenerate with tests/tools/plan_trace.py --write"
    assert set(table["envs"]) == {T.env_key(e) for e in T.ENVS}
    default = T.decode(table, "default")
    assert len(default) == len(rows)
    # every model is there in both compute types, every run launches something, and a UNet forward of these nets is some hundreds of launches
    assert {(r[0], r[2]) for r in rows} == {(m, d) for m in ("unet", "vae", "clip", "t5", "esrgan", "flux") for d in T.DTYPES}
    assert all(p[0] > 0 for r, p in zip(rows, default) if r[3] != "build")
    assert all(100 < p[0] < 2000 for r, p in zip(rows, default) if r[0] == "unet" and r[3] != "build")
    # every switch is live in some case, but for the four that cannot be at these sizes (plan_trace.DEAD), which must then plan what the default plans
    dead = {T.env_key(e) for e in T.DEAD}
    for key in table["envs"]:
        assert key == "default" or (T.decode(table, key) == default) == (key in dead), f"{key}: {'changes a case' if key in dead else 'changes no case'}"


@pytest.mark.parametrize("env", T.ENVS, ids=T.env_key)
def test_traces_match_the_table(rows, table, traces, env):
    got, want = traces[T.env_key(env)], T.decode(table, T.env_key(env))
    assert len(got) == len(want) == len(rows)
    bad = [i for i in range(len(rows)) if got[i] != want[i]]
    # a plan's addresses depend on the allocations before it: the first differing case is the one to look at
    assert not bad, f"{len(bad)} of {len(rows)} cases differ from tests/golden/plan_traces.json; the first: " + T.mismatch(env, bad[0], rows[bad[0]], got[bad[0]], want[bad[0]])


def test_the_recorder_sees_a_changed_argument(traces, rows):
    """The digest covers the argument bytes: the same net at the same shape through ldx_unet_denoise and ldx_unet_denoise_t differs in one pointer of the boundary kernel."""
    d = dict(zip(rows, traces["default"]))
    a, b = d[("unet", "tiny", "bf16", "denoise", 16, 16, 2, 1, 0)], d[("unet", "tiny", "bf16", "denoise_t", 16, 16, 2, 1, 0)]
    assert a[0] == b[0] and a[1] != b[1]


def test_row_block_ops_are_recorded(ldx_lib, rows):
    """With the chip-fill rule lifted (plan_trace.ROWBLOCKS) a 320-wide level runs rowgemm (LayerNorm and GroupNorm prologues), xattn_block and ff_block launches: the
    environments built on it hold those op kinds, which no plan of the small nets has by default."""
    T.build_host()
    i = rows.index(("unet", "two_level_320", "bf16", "denoise_t", 24, 16, 2, 1, 0))
    recs = T.records_of_env(T.ROWBLOCKS, i)
    for kernel in ("ldx::rowgemm_kernel<__bf16, 1", "ldx::rowgemm_kernel<__bf16, 2", "ldx::xattn_block_kernel<__bf16", "ldx::ff_block_kernel<__bf16"):
        assert any(kernel in r for r in recs), f"no {kernel} launch in case {i} under {T.env_key(T.ROWBLOCKS)}"
    assert not any("rowgemm_kernel" in r or "xattn_block" in r or "ff_block" in r for r in T.records_of_env({}, i))
