"""The case table of the producer-written GroupNorm statistics tests (tests/_gn_stats_cases.py) on a machine without a GPU: every case still reaches the kernel it
is there for (ldx_op_gemm_pick is host arithmetic), the refusals still produce no statistics, and every case's int64 reference satisfies the condition that makes
fp32 sums of its integers exact in any order.  tests/test_gn_stats_gpu.py asserts the same picks before it launches."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gn_stats_cases as T  # noqa: E402


def test_every_producer_path_has_a_case():
    picks = {c.pick for c in T.CASES}
    assert {(p[0], p[4]) for p in picks if p} >= {("tile", "none"), ("tile", "reduce_gn"), ("pingpong", "none"), ("pingpong", "reduce_gn"), ("ring", "none"), ("conv_patch", "none")}
    assert any(p and p[0] == "pingpong" and p[2] > 160 for p in picks), "no case on the column-major output stage of the wide ping-pong tiles"
    assert {c.N // T.G for c in T.CASES} >= {2, 4, 8, 10, 16, 20, 40}, "group widths: below, at and above a lane's four columns, and 10: a lane's columns straddle two groups"
    assert any(c.op == "rowgemm" and c.Cin == 320 for c in T.CASES) and any(c.op == "rowgemm" and c.Cin == 640 for c in T.CASES)
    assert any(T.expected_chunks(c) > T.GN_NCHUNK for c in T.CASES), "no case whose consumer folds first"
    assert set(T.DUP) <= set(T.BY_NAME) and len({c.name for c in T.CASES}) == len(T.CASES)


@pytest.mark.parametrize("c", [c for c in T.CASES if c.pick], ids=lambda c: c.name)
def test_probe_matches_the_table(ldx_lib, c):
    pick, chunks = T.probe(ldx_lib, c)
    assert (pick, chunks) == (c.pick, c.chunks), f"case {c.name} no longer reaches its kernel: move the shape, keep the path"
    assert chunks <= T.max_chunks(T.hw(c))


@pytest.mark.parametrize("c", [c for c in T.CASES if not c.pick], ids=lambda c: c.name)
def test_rowblock_cases_are_whole_blocks(c):
    bm = T.rowblock_rows(c.Cin)
    assert c.N == c.Cin and c.Cin in (320, 640) and T.hw(c) % bm == 0 and T.expected_chunks(c) == c.chunks == T.hw(c) // bm
    assert not ((c.N // T.G) % 8 == 0 and T.hw(c) * (c.N // T.G) <= 256 * 80 and T.G * c.B >= 32), "the one-launch small GroupNorm would take the consumer"


@pytest.mark.parametrize("c", T.REFUSALS, ids=lambda c: c.name)
def test_refusals_give_no_chunks(ldx_lib, c):
    pick, chunks = T.probe(ldx_lib, c)
    assert chunks == 0 and pick == c.pick


@pytest.mark.parametrize("c", T.CASES, ids=lambda c: c.name)
def test_reference_is_exact_in_fp32(c):
    d = T.int_inputs(c)
    assert int(d["Wpos"].max()) < T.k_total(c) and (d["Wpos"][:, 1:] > d["Wpos"][:, :-1]).all(), "distinct positions: every non-zero of W is +-1"
    W = T.dense_w(c, d)
    assert int((W != 0).sum(1).max()) <= T.NNZ and int(W.abs().max()) == 1
    if c.op == "conv":          # the non-zeros reach every tap and the skip segment
        seg = torch.bincount((d["Wpos"] // c.Cin).clamp(max=9).flatten(), minlength=10)
        assert (seg[:9] > 0).all() and (seg[9] > 0) == bool(c.Cin2)
    Y = T.int_reference(c, d)
    assert Y.dtype == torch.int64 and int(Y.abs().max()) <= 16, "every stored value must be exact in bf16 and f16"
    n = T.expected_chunks(c)
    stats = T.chunk_stats(c, Y, n)
    assert stats.shape == (c.B, n, T.G, 2) and T.exactness_ok(stats)
    assert torch.equal(stats.sum(1)[..., 0], Y.view(c.B, T.hw(c), T.G, -1).sum((1, 3)))      # the chunk map covers every row once


def test_small_reference_matches_a_float_conv():
    """The gather-and-add reference against torch's own conv on a small problem with a skip segment (both exact in fp64)."""
    c = T._conv("t", 2, 5, 7, 64, 32, None, 0, Cin2=64, rv=True, res=True)
    d = T.int_inputs(c)
    W = T.dense_w(c, d).double()
    w9 = W[:, :9 * c.Cin].view(c.N, 3, 3, c.Cin).permute(0, 3, 1, 2)
    ref = torch.nn.functional.conv2d(d["X"].double().permute(0, 3, 1, 2), w9, padding=1).permute(0, 2, 3, 1).reshape(-1, c.N)
    ref = ref + d["X2"].double() @ W[:, 9 * c.Cin:].t() + d["bias"].double() + d["rowvec"].double().repeat_interleave(35, 0) + d["R"].double()
    assert torch.equal(T.int_reference(c, d).double(), ref)
