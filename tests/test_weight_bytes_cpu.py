"""The packed weights of every engine — each buffer's address, size and a 64-bit digest of its bytes as the host packers fill it, and for the UNet the device
packers' launches (kernel, grid, every argument byte) and staging copies — recorded without a GPU by the host-only build of the library against a stand-in HIP
runtime (tests/tools/plan_trace.py --weights says how, and lists the cases and environments) against tests/golden/weight_bytes.json.  A layout is described once and
interpreted on both sides; a change to the packers or to a description that is meant to leave the weights alone leaves this table alone."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import plan_trace as T  # noqa: E402

W = T.Weights


@pytest.fixture(scope="module")
def rows():
    return W.all_rows()


@pytest.fixture(scope="module")
def table():
    return W.load_table()


@pytest.fixture(scope="module")
def traces(ldx_lib):
    T.build_host()
    return W.picks_of_envs(W.ENVS)


def test_table_covers_the_cases(rows, table):
    assert table["fields"] == list(T.FIELDS)
    assert table["n_rows"] == len(rows) and table["rows_sha256"] == T.rows_digest(rows), "the cases changed: regenerate with tests/tools/plan_trace.py --weights --write"
    assert set(table["envs"]) == {T.env_key(e) for e in W.ENVS}
    # every engine's build in both compute types, the UNets from the host, from the device and mixed
    assert {(r[0], r[2]) for r in rows} == {(m, d) for m in ("unet", "vae", "clip", "t5", "esrgan", "flux") for d in T.DTYPES}
    unets = {r[1] for r in rows if r[0] == "unet"}
    assert "tiny_in9" in unets and {(r[1], r[3]) for r in rows if r[0] == "unet"} == {(u, how) for u in unets for how in ("build", "build_dev", "build_mixed")}
    default = W.decode(table, "default")
    assert len(default) == len(rows) and all(p[0] > 0 for p in default)
    # each of the three switches changes the packed weights of some UNet, on the host path and on the device path
    for key in table["envs"]:
        if key != "default":
            moved = {r[3] for r, a, b in zip(rows, W.decode(table, key), default) if a != b and r[0] == "unet"}
            assert moved == {"build", "build_dev", "build_mixed"}, (key, moved)


@pytest.mark.parametrize("env", W.ENVS, ids=T.env_key)
def test_weights_match_the_table(rows, table, traces, env):
    got, want = traces[T.env_key(env)], W.decode(table, T.env_key(env))
    assert len(got) == len(want) == len(rows)
    bad = [i for i in range(len(rows)) if got[i] != want[i]]
    # addresses depend on the allocations before them: the first differing case is the one to look at
    assert not bad, f"{len(bad)} of {len(rows)} cases differ from tests/golden/weight_bytes.json; the first: " + W.mismatch(env, bad[0], rows[bad[0]], got[bad[0]], want[bad[0]])


def test_the_recorder_sees_the_bytes(traces, rows):
    """The digest covers the content of the buffers: without the q prescale the same buffers are filled at the same addresses, with other values in the q rows."""
    i = rows.index(("unet", "tiny", "bf16", "build", 0, 0, 0, 0, 0))
    a, b = traces["default"][i], traces["LDX_NO_QPRESCALE=1"][i]
    assert a[0] == b[0] and a[1] != b[1]
