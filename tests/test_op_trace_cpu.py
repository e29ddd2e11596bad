"""What the single-op entry points (ldx_op_gemm*, ldx_op_conv3x3*, ldx_op_upconv2x, ldx_op_attention*) launch — kernels, grids, LDS sizes and every argument byte,
recorded without a GPU by the host-only build of the library against the stand-in HIP runtime (tests/tools/plan_trace.py says how) — against
tests/golden/op_traces.json.  Every kernel-level GPU test and every probe under profiles/ reaches its kernel through these entry points, which build their launch
arguments (conv geometry, split-K count and workspace, attention scratch) beside the planner, not through it; tests/golden/plan_traces.json pins the planner's side,
this table the single-op side.  A change to how launch arguments are built that is meant to leave behaviour alone leaves this table alone.

The calls (CALLS) are the smallest shapes that reach each construction branch.  They run in this order in one process on made-up device pointers and a null stream:
the shared single-op scratch buffer grows as the calls ask for more, so a call's addresses depend on the calls before it, and the FIRST differing call is the one to
look at.  The first call that splits K also records the memset of the split counters.  ldx_op_gemm2 refuses an empty second problem (M2 <= 0), so there is no such call.

    python tests/test_op_trace_cpu.py            # the records of every call, kernel names demangled
    python tests/test_op_trace_cpu.py --write    # accept the current build's traces as the new table (only for a change that MEANS to change launches)
"""
import json
import os
import shutil
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import plan_trace as T  # noqa: E402

TABLE = os.path.join(ROOT, "tests", "golden", "op_traces.json")
BF16, F16 = 0, 1
# made-up device buffers, 4 GiB apart
A, W, BIAS, RV, R, C, CF, SA, SW, C8, SC, A2, W2, C2, SA2, SW2, Q, O, SO, AB = (0x7d0000000000 + (i << 32) for i in range(20))

# (id, entry point, arguments without the trailing (dtype, stream))
CALLS = [
    # ldx_op_gemm(A, lda, W, M, N, K, bias, rowvec, rowvec_ld, rows_per_batch, geglu, R, ldr, C, ldc, Cf, ldcf)
    ("gemm 64x64x64 bias", "ldx_op_gemm", (A, 64, W, 64, 64, 64, BIAS, None, 0, 0, 0, None, 0, C, 64, None, 0), BF16),
    ("gemm 256x320x2880 split-K", "ldx_op_gemm", (A, 2880, W, 256, 320, 2880, BIAS, None, 0, 0, 0, None, 0, C, 320, None, 0), BF16),
    ("gemm 256x2560x320 geglu", "ldx_op_gemm", (A, 320, W, 256, 2560, 320, BIAS, None, 0, 0, 1, None, 0, C, 1280, None, 0), BF16),
    ("gemm 128x64x64 rowvec rpb R Cf", "ldx_op_gemm", (A, 64, W, 128, 64, 64, BIAS, RV, 64, 64, 0, R, 64, C, 64, CF, 64), BF16),
    ("gemm 64x64x64 f16", "ldx_op_gemm", (A, 64, W, 64, 64, 64, BIAS, None, 0, 0, 0, None, 0, C, 64, None, 0), F16),
    # ldx_op_gemm_mx(A8, lda, SA, sa_ld, W8, SW, sw_ld, M, N, K, bias, act, R, ldr, C, ldc, Cf, ldcf, C8, ldc8, SC, sc_ld)
    ("gemm_mx 128x256x256", "ldx_op_gemm_mx", (A, 256, SA, 128, W, SW, 256, 128, 256, 256, BIAS, 0, None, 0, C, 256, None, 0, None, 0, None, 0), BF16),
    ("gemm_mx 128x256x256 MX out", "ldx_op_gemm_mx", (A, 256, SA, 128, W, SW, 256, 128, 256, 256, BIAS, 0, None, 0, None, 0, None, 0, C8, 256, SC, 128), BF16),
    ("gemm_mx 128x256x5120 split-K", "ldx_op_gemm_mx", (A, 5120, SA, 128, W, SW, 256, 128, 256, 5120, BIAS, 0, None, 0, C, 256, None, 0, None, 0, None, 0), BF16),
    # ldx_op_gemm2(A1, lda1, W1, M1, N1, K1, bias1, C1, ldc1, A2, lda2, W2, M2, N2, K2, bias2, C2, ldc2)
    ("gemm2 128+64 x256x256", "ldx_op_gemm2", (A, 256, W, 128, 256, 256, BIAS, C, 256, A2, 256, W2, 64, 256, 256, BIAS, C2, 256), BF16),
    # ldx_op_gemm2_mx(A1, lda1, SA1, sa_ld1, W1, SW1, sw_ld1, M1, N1, K1, bias1, C1, ldc1, A2, lda2, SA2, sa_ld2, W2, SW2, sw_ld2, M2, N2, K2, bias2, C2, ldc2)
    ("gemm2_mx 128+64 x256x256", "ldx_op_gemm2_mx", (A, 256, SA, 128, W, SW, 256, 128, 256, 256, BIAS, C, 256, A2, 256, SA2, 64, W2, SW2, 256, 64, 256, 256, BIAS, C2, 256), BF16),
    # ldx_op_conv3x3(X, ldx, W, B, Hin, Win, Cin, Cout, stride, Hout, Wout, resize_to_out, bias, rowvec, rowvec_ld, R, ldr, Y, ldy)
    ("conv3x3 16x16 64->64", "ldx_op_conv3x3", (A, 64, W, 1, 16, 16, 64, 64, 1, 16, 16, 0, BIAS, None, 0, None, 0, C, 64), BF16),
    ("conv3x3 stride 2 16->8", "ldx_op_conv3x3", (A, 64, W, 1, 16, 16, 64, 64, 2, 8, 8, 0, BIAS, None, 0, None, 0, C, 64), BF16),
    ("conv3x3 resize 8->16", "ldx_op_conv3x3", (A, 64, W, 1, 8, 8, 64, 64, 1, 16, 16, 1, BIAS, None, 0, None, 0, C, 64), BF16),
    ("conv3x3 16x16 320->320 split-K", "ldx_op_conv3x3", (A, 320, W, 1, 16, 16, 320, 320, 1, 16, 16, 0, BIAS, None, 0, None, 0, C, 320), BF16),
    ("conv3x3 B2 16x16 rowvec R", "ldx_op_conv3x3", (A, 64, W, 2, 16, 16, 64, 64, 1, 16, 16, 0, BIAS, RV, 64, R, 64, C, 64), BF16),
    # ldx_op_conv3x3_skip(X, ldx, X2, ldx2, Cin2, W, B, H, W, Cin, Cout, bias, Y, ldy)
    ("conv3x3_skip 16x16 64+64->128", "ldx_op_conv3x3_skip", (A, 64, A2, 64, 64, W, 1, 16, 16, 64, 128, BIAS, C, 128), BF16),
    # ldx_op_upconv2x(X, ldx, W9, B, Hin, Win, Cin, Cout, bias, Y, ldy)
    ("upconv2x 16x16 64->64", "ldx_op_upconv2x", (A, 64, W, 1, 16, 16, 64, 64, BIAS, C, 64), BF16),
    # ldx_op_attention(Q, ldq, K, ldk, V, ldv, O, ldo, B, H, Nq, Mk, D, scale, causal)
    ("attention B2 H8 N4096 D40", "ldx_op_attention", (Q, 960, Q + 640, 960, Q + 1280, 960, O, 320, 2, 8, 4096, 4096, 40, 40 ** -0.5, 0), BF16),
    ("attention B1 H8 N256 M77 D40", "ldx_op_attention", (Q, 320, A, 640, A + 640, 640, O, 320, 1, 8, 256, 77, 40, 40 ** -0.5, 0), BF16),
    ("attention B1 H12 N77 D64 causal", "ldx_op_attention", (Q, 2304, Q + 1536, 2304, Q + 3072, 2304, O, 768, 1, 12, 77, 77, 64, 0.125, 1), BF16),
    ("attention B1 H24 N4352 D128", "ldx_op_attention", (Q, 9216, Q + 6144, 9216, Q + 12288, 9216, O, 3072, 1, 24, 4352, 4352, 128, 128 ** -0.5, 0), BF16),
    ("attention B1 H1 N1024 D512", "ldx_op_attention", (Q, 1536, Q + 1024, 1536, Q + 2048, 1536, O, 512, 1, 1, 1024, 1024, 512, 512 ** -0.5, 0), BF16),
    # ldx_op_attention_mx(Q, ldq, K, ldk, V, ldv, O8, ldo8, SO, so_ld, B, H, Nq, Mk, scale)
    ("attention_mx B1 H24 N4352", "ldx_op_attention_mx", (Q, 9216, Q + 6144, 9216, Q + 12288, 9216, C8, 3072, SO, 4352, 1, 24, 4352, 4352, 128 ** -0.5), BF16),
    # ldx_op_attention_bias(Q, ldq, K, ldk, V, ldv, O, ldo, B, H, Nq, Mk, D, scale, bias, bias_ld, bias_head_stride)
    ("attention_bias B1 H8 N77 D64", "ldx_op_attention_bias", (Q, 1536, Q + 1024, 1536, Q + 2048, 1536, O, 512, 1, 8, 77, 77, 64, 1.0, AB, 128, 77 * 128), BF16),
]


def records_of_calls():
    """[records] per call of CALLS, from a private copy of the host library: the stand-in runtime's addresses and the library's single-op scratch start afresh per
    loaded image, whatever other test modules of the same process have run."""
    T.build_host()
    tmp = tempfile.mkdtemp(prefix="ldx_op_trace_")
    private = os.path.join(tmp, "libldx_host_ops.so")
    shutil.copy(T.HOST_LIB, private)
    orig, T.HOST_LIB = T.HOST_LIB, private
    try:
        H = T.Host()
    finally:
        T.HOST_LIB = orig
    try:
        H.take()
        out = []
        for cid, fn, args, dtype in CALLS:
            H.check(getattr(H.L, fn)(*args, dtype, None), cid)
            out.append(H.take())
        return out
    finally:
        os.unlink(H.path)
        shutil.rmtree(tmp, ignore_errors=True)


def load_table():
    with open(TABLE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def records(ldx_lib):
    return records_of_calls()


def test_table_covers_the_calls():
    t = load_table()
    assert t["fields"] == list(T.FIELDS) and list(t["calls"]) == [c[0] for c in CALLS], "the calls changed: regenerate with tests/test_op_trace_cpu.py --write"
    assert {c[1] for c in CALLS} == {"ldx_op_gemm", "ldx_op_gemm_mx", "ldx_op_gemm2", "ldx_op_gemm2_mx", "ldx_op_conv3x3", "ldx_op_conv3x3_skip", "ldx_op_upconv2x",
                                     "ldx_op_attention", "ldx_op_attention_mx", "ldx_op_attention_bias"}


def test_every_construction_branch_is_reached(records):
    """The shapes do what their ids say: K splits with their reduce launch (the first also zeroes the counters), the key-norm launch of the pipelined attention kernels,
    the merge launch of the D = 512 kernel's key splits, the phase weights' derivation in front of the phase-form up conv."""
    r = dict(zip((c[0] for c in CALLS), records))
    assert all(x and not any(l.endswith(" ?") for l in x) for x in r.values()), "a call launched nothing, or a kernel whose argument sizes are not known"
    launches = {k: [l.split()[1] for l in v if l.startswith("L ")] for k, v in r.items()}
    for k in ("gemm 256x320x2880 split-K", "gemm_mx 128x256x5120 split-K", "conv3x3 16x16 320->320 split-K"):
        assert len(launches[k]) == 2 and "reduce" in launches[k][1], (k, launches[k])
    assert sum(l.startswith("S ") for v in r.values() for l in v) <= 1
    for k in ("gemm 64x64x64 bias", "gemm 256x2560x320 geglu", "gemm_mx 128x256x256 MX out", "gemm2 128+64 x256x256", "conv3x3 16x16 64->64", "attention B1 H8 N256 M77 D40"):
        assert len(launches[k]) == 1, (k, launches[k])
    for k, kernel in (("attention B2 H8 N4096 D40", "attn40p"), ("attention B1 H24 N4352 D128", "attn128p"), ("attention_mx B1 H24 N4352", "attn128p")):
        assert len(launches[k]) == 2 and "knorm" in launches[k][0] and kernel in launches[k][1], (k, launches[k])
    assert len(launches["attention B1 H1 N1024 D512"]) == 2 and "attn512" in launches["attention B1 H1 N1024 D512"][0]
    assert len(launches["upconv2x 16x16 64->64"]) == 2 and "up_phase" in launches["upconv2x 16x16 64->64"][0]


def test_traces_match_the_table(records):
    want = load_table()["calls"]
    got = {c[0]: list(T.digest(r)) for c, r in zip(CALLS, records)}
    bad = [k for k in got if got[k] != want.get(k)]
    # a call's scratch addresses depend on the calls before it: the first differing call is the one to look at
    assert not bad, (f"{len(bad)} of {len(CALLS)} calls differ from tests/golden/op_traces.json; the first: {bad[0]}: {got[bad[0]]} (table: {want.get(bad[0])}); "
                     "`python tests/test_op_trace_cpu.py` lists this tree's records, to be compared with those of the tree the table was written from")


if __name__ == "__main__":
    recs = records_of_calls()
    if "--write" in sys.argv:
        with open(TABLE, "w") as f:          # one call per line
            f.write('{\n"fields": ' + json.dumps(list(T.FIELDS)) + ',\n"calls": {\n' +
                    ",\n".join(f"{json.dumps(c[0])}: {json.dumps(list(T.digest(r)))}" for c, r in zip(CALLS, recs)) + "\n}\n}\n")
        print(f"wrote {len(CALLS)} calls to {TABLE}")
    else:
        for c, r in zip(CALLS, recs):
            print(f"# {c[0]}: {T.digest(r)}")
            print("\n".join(T._demangled(r)))
