"""GroupNorm statistics written by the launch in front of the GroupNorm (GroupNormArgs::partial), one op at a time on a real MI355X.

Five device code paths write them — the tile epilogue (GNS), the column-major output stage of the wide ping-pong tiles (GNW), the split-K reduce launch, the
patch-resident conv and the row-block output stage — and three read them: gn_apply_kernel, gn_fold_kernel + apply, and rowgemm's pro = 2 prologue.  The entry points
ldx_op_conv3x3_gn / ldx_op_gemm_gn / ldx_op_rowgemm_gn / ldx_op_groupnorm_stats build the launches the planner builds (include/ldx.h).

Exact tests: with the integer inputs of tests/_gn_stats_cases.py every stored value, accumulator and statistic is an integer below 2^24, so the output and every
(image, chunk, group) row must EQUAL an int64 reference — no tolerance.  A dropped row, a column credited to the neighbouring group, a chunk written to another
image's row or a duplicated row counted twice each changes an integer.  Parity tests: the same launches on random data against fp64 under tests/test_ops_gpu.py's
TOL, rowgemm's GroupNorm prologue fed by real producers under tests/test_rowgemm_gpu.py's bound, hand-made ragged rows through the fold, and the conditioning of the
one-pass variance var = E[x^2] - mean^2 at group mean / std ratios of 0, 4 and 16 (64 is measured and printed only: DESIGN.md has the figure)."""
import ctypes as C
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gn_stats_cases as T  # noqa: E402

pytestmark = pytest.mark.gpu

DT = {"bf16": (torch.bfloat16, 0), "f16": (torch.float16, 1)}
TOL = {"bf16": (4e-3, 2e-2), "f16": (6e-4, 4e-3)}          # tests/test_ops_gpu.py: rel-L2, max-abs relative to the output scale
ROWGEMM_TOL = {"bf16": 5e-3, "f16": 7e-4}                   # tests/test_rowgemm_gpu.py
G = T.G
LDX_EINVAL = -1


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def L(ldx_lib):
    assert torch.cuda.is_available()
    return ldx_lib


def _err(got, ref):
    got, ref = got.double(), ref.double()
    return float((got - ref).norm() / (ref.norm() + 1e-20)), float((got - ref).abs().max() / (ref.abs().max() + 1e-20))


def _check(got, ref, dt, what):
    rel, mx = _err(got, ref)
    print(f"{what}: rel-L2 {rel:.3e} max {mx:.3e}")
    r, m = TOL[dt]
    assert math.isfinite(rel) and rel <= r and mx <= m, f"{what}: rel-L2 {rel:.3e} max {mx:.3e}"


def _gn64(Y, B, HW, C_, gamma, beta, eps, silu):
    """fp64 group_norm (+ SiLU) of the stored rows Y [B * HW][>= C_]."""
    y = Y[:, :C_].double().reshape(B, HW, C_).transpose(1, 2)
    o = F.group_norm(y, G, gamma.double(), beta.double(), eps).transpose(1, 2).reshape(B * HW, C_)
    return o * torch.sigmoid(o) if silu else o


def _affine(C_, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return 1 + 0.1 * torch.randn(C_, device="cuda", generator=g), 0.1 * torch.randn(C_, device="cuda", generator=g)


# ---- inputs: the integer ones (shared with the CPU test) and random ones of the same shapes -----------------------------------------------------------
_INTS, _REF = {}, {}


def _ints(c):
    if c.name not in _INTS:
        _INTS[c.name] = T.int_inputs(c)
    return _INTS[c.name]


def _ref(c):
    """int64 reference output of case c, computed once on the device with integer ops and never changed."""
    if c.name not in _REF:
        _REF[c.name] = T.int_reference(c, _ints(c), "cuda")
    return _REF[c.name]


def _int_tensors(c, td):
    d = _ints(c)
    f16 = lambda x: None if x is None else x.cuda().to(td)
    f32 = lambda x: None if x is None else x.cuda().float()
    return {"X": f16(d["X"]), "X2": f16(d["X2"]), "W": f16(T.dense_w(c, d)), "bias": f32(d["bias"]), "rowvec": f32(d["rowvec"]), "R": f16(d["R"])}


def _rand_tensors(c, td, seed, bias_shift=None):
    """randn activations, 1 / sqrt(K) weights: the inputs of tests/test_ops_gpu.py."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device="cuda", generator=g)
    M, K = T.rows_total(c), T.k_total(c)
    return {"X": (rn(c.B, c.H, c.W, c.Cin) if c.op == "conv" else rn(M, c.Cin)).to(td), "X2": rn(M, c.Cin2).to(td) if c.Cin2 else None,
            "W": (rn(c.N, K) / math.sqrt(K)).to(td), "bias": rn(c.N) if bias_shift is None else 0.1 * rn(c.N) + bias_shift, "rowvec": rn(c.B, c.N) if c.rv else None,
            "R": rn(M, c.N).to(td) if c.res else None}


def _produce(L, c, t, code, Y, partial, dup=0, pro=0, norm=None, eps=1e-5):
    """Case c's producer launch on the tensors t: (return code, statistics rows per image)."""
    n = C.c_int32(-1)
    M, HW, ldy, mc = T.rows_total(c), T.hw(c), Y.shape[1], T.max_chunks(T.hw(c))
    if c.op == "conv":
        rc = L.ldx_op_conv3x3_gn(_p(t["X"]), c.Cin, _p(t["X2"]), c.Cin2, c.Cin2, _p(t["W"]), c.B, c.H, c.W, c.Cin, c.N, 1, c.H, c.W, 0, _p(t["bias"]),
                                 _p(t["rowvec"]), c.N, _p(t["R"]), c.N, _p(Y), ldy, dup, _p(partial), G, mc, C.byref(n), code, _st())
    elif c.op == "gemm":
        assert not dup
        rc = L.ldx_op_gemm_gn(_p(t["X"]), c.Cin, _p(t["W"]), M, c.N, c.Cin, _p(t["bias"]), _p(t["rowvec"]), c.N, HW, _p(t["R"]), c.N, _p(Y), ldy, None, 0,
                              HW, _p(partial), G, mc, C.byref(n), code, _st())
    else:
        ga, be = norm if norm else (None, None)
        rc = L.ldx_op_rowgemm_gn(_p(t["X"]), c.Cin, _p(Y), ldy, M, c.N, c.Cin, _p(t["W"]), _p(t["bias"]), _p(t["R"]), c.N, pro, _p(ga), _p(be), eps,
                                 HW, dup, _p(partial), mc, C.byref(n), code, _st())
    return rc, n.value


def _partial_buffer(c):
    return torch.full(((c.B * T.max_chunks(T.hw(c)) + 4) * G * 2,), T.SENTINEL, device="cuda")


def _apply_from_rows(L, ldx, Y, ldy, c, partial, n, gamma, beta, eps, silu, td, code):
    """ldx_op_groupnorm_stats of Y's first B * HW rows from the producer's rows (copied in front of the fold target)."""
    used = c.B * n * G * 2
    ws = torch.full((int(L.ldx_op_groupnorm_stats_floats(c.B, G, n)),), float("nan"), device="cuda")
    ws[:used] = partial[:used]
    out = torch.zeros(T.rows_total(c), c.N, device="cuda", dtype=td)
    ldx.lib.check(L.ldx_op_groupnorm_stats(_p(Y), ldy, _p(out), c.N, c.B, T.hw(c), c.N, G, eps, silu, _p(gamma), _p(beta), _p(ws), n, code, _st()), "groupnorm_stats")
    return out


# ---- 1. exact: output and statistics against the int64 reference ---------------------------------------------------------------------------------------
EXACT = [(c, 0) for c in T.CASES] + [(T.BY_NAME[n], 1) for n in T.DUP]


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("c,dup", EXACT, ids=[c.name + ("-dup" if d else "") for c, d in EXACT])
def test_producer_output_and_statistics_are_exact(L, ldx, dt, c, dup):
    td, code = DT[dt]
    M, HW, N = T.rows_total(c), T.hw(c), c.N
    if c.pick:
        assert T.probe(L, c) == (c.pick, c.chunks), f"case {c.name} no longer reaches its kernel"
    n_exp = T.expected_chunks(c)
    Yref = _ref(c)
    stats = T.chunk_stats(c, Yref, n_exp)
    assert T.exactness_ok(stats), "the reference itself must make every fp32 sum exact"
    t = _int_tensors(c, td)
    ldy, runs = N + 8, []
    for _ in range(2):
        Y = torch.zeros(M * (2 if dup else 1), ldy, device="cuda", dtype=td)
        partial = _partial_buffer(c)
        rc, n = _produce(L, c, t, code, Y, partial, dup=M if dup else 0)
        ldx.lib.check(rc, f"producer {c.name}")
        torch.cuda.synchronize()
        runs.append((Y, partial, n))
    Y, partial, n = runs[0]
    assert n == n_exp
    # 1. the output, and nothing beside it
    assert torch.equal(Y[:M, :N].double(), Yref.double()), f"{c.name}: Y differs from the integer reference in {int((Y[:M, :N].double() != Yref.double()).sum())} places"
    assert not Y[:, N:].any(), "padding columns written"
    if dup:
        assert torch.equal(Y[M:], Y[:M]), "rows M .. 2M must repeat rows 0 .. M"
    # 2. every (image, chunk, group) row; 3. nothing behind them
    used = c.B * n * G * 2
    got = partial[:used].view(c.B, n, G, 2).double()
    bad = (got != stats.double()).any(-1)
    assert not bad.any(), f"{c.name}: {int(bad.sum())} of {bad.numel()} statistics rows differ, first (image, chunk, group) {bad.nonzero()[0].tolist()}: " \
                          f"{got[bad][0].tolist()} for {stats[bad][0].tolist()}"
    assert (partial[used:] == T.SENTINEL).all(), "rows behind nchunk written"
    # 4. deterministic
    assert torch.equal(runs[1][0], Y) and torch.equal(runs[1][1], partial) and runs[1][2] == n
    # 5. the consumer on those rows (apply only, behind a fold of more than 256 rows) equals the GroupNorm that runs its own pass: both sets of statistics are
    #    exact, the apply kernel is the same
    gamma, beta = _affine(N, 7)
    eps, silu = (1e-5, 1) if len(c.name) == 1 and ord(c.name) % 2 else (1e-6, 0)
    a = _apply_from_rows(L, ldx, Y, ldy, c, partial, n, gamma, beta, eps, silu, td, code)
    b = torch.zeros_like(a)
    ws = torch.zeros(int(L.ldx_op_groupnorm_workspace_floats(c.B, G)), device="cuda")
    ldx.lib.check(L.ldx_op_groupnorm(_p(Y), ldy, _p(b), N, c.B, HW, N, G, eps, silu, _p(gamma), _p(beta), _p(ws), code, _st()), "groupnorm")
    torch.cuda.synchronize()
    assert torch.isfinite(a).all() and torch.equal(a, b), f"{c.name}: GroupNorm from the producer's rows differs from the plain pass in {int((a != b).sum())} places"


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_refusals_launch_nothing(L, ldx, dt):
    td, code = DT[dt]
    for c in T.REFUSALS:
        assert T.probe(L, c) == (c.pick, 0)
        M, K = T.rows_total(c), T.k_total(c)
        z = lambda *s: torch.zeros(*s, device="cuda", dtype=td)
        t = {"X": z(c.B, c.H, c.W, c.Cin) if c.op == "conv" else z(M, c.Cin), "X2": None, "W": z(c.N, K), "bias": torch.zeros(c.N, device="cuda"), "rowvec": None, "R": None}
        Y, partial = torch.zeros(M, c.N, device="cuda", dtype=td) + 1, _partial_buffer(c)
        rc, n = _produce(L, c, t, code, Y, partial)
        torch.cuda.synchronize()
        assert rc == LDX_EINVAL and n == -1 and b"GroupNorm statistics" in L.ldx_last_error()
        assert (Y == 1).all() and (partial == T.SENTINEL).all()
    # the row-block producer: N != K, and images that are not whole row blocks
    for N, K, B, HW in ((960, 320, 2, 1024), (320, 320, 2, 192), (640, 640, 1, 96)):
        c = T.Case("r", "rowgemm", B, HW, 1, K, N, 0, False, False, None, 0, "rows")
        t = {"X": torch.zeros(B * HW, K, device="cuda", dtype=td), "W": torch.zeros(N, K, device="cuda", dtype=td), "bias": torch.zeros(N, device="cuda"), "R": None}
        Y, partial = torch.zeros(B * HW, N, device="cuda", dtype=td) + 1, _partial_buffer(c)
        rc, n = _produce(L, c, t, code, Y, partial)
        torch.cuda.synchronize()
        assert rc == LDX_EINVAL and n == -1 and (Y == 1).all() and (partial == T.SENTINEL).all()


# ---- the GroupNorm's own statistics pass (gn_stats_kernel writes its rows into the caller's workspace) -------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("B,HW,C_", [(2, 1024, 320), (2, 1000, 320), (1, 4096, 192), (2, 77, 1920)])
def test_plain_pass_rows_sum_to_the_integer_totals(L, ldx, dt, B, HW, C_):
    """A ragged HW, a C whose groups are not whole 16-byte chunks, and HW 77 x C 1920: 60 channels per group, so NOT the one-launch kernel — 20 rows per image."""
    td, code = DT[dt]
    g = torch.Generator(device="cuda").manual_seed(B + HW + C_)
    Xi = torch.randint(-8, 9, (B * HW, C_), device="cuda", generator=g)
    X = Xi.to(td)
    xs = Xi.view(B, HW, G, C_ // G)
    totals = torch.stack([xs.sum((1, 3)), (xs * xs).sum((1, 3))], -1)          # int64 [B][G][2]
    assert int(totals[..., 1].max()) < 2 ** 24
    gamma, beta = _affine(C_, 3)
    nws = int(L.ldx_op_groupnorm_workspace_floats(B, G))
    outs = []
    for fill in (T.SENTINEL, 0.0):          # the sentinel run shows how many rows the launch writes, the zero-filled run is summed
        ws = torch.full((nws,), fill, device="cuda")
        Y = torch.zeros(B * HW, C_, device="cuda", dtype=td)
        ldx.lib.check(L.ldx_op_groupnorm(_p(X), C_, _p(Y), C_, B, HW, C_, G, 1e-5, 0, _p(gamma), _p(beta), _p(ws), code, _st()), "groupnorm")
        torch.cuda.synchronize()
        outs.append((ws.view(-1, G, 2), Y))
    written = (outs[0][0] != T.SENTINEL).all(-1).all(-1)
    rows = int(written.sum())
    assert rows > 0 and rows % B == 0 and rows <= B * T.GN_NCHUNK and written[:rows].all() and (outs[0][0][rows:] == T.SENTINEL).all(), "whole rows, packed at the front"
    ws0 = outs[1][0]
    assert torch.equal(ws0[:rows].view(B, rows // B, G, 2).double().sum(1), totals.double()), "chunk rows do not add up to the integer totals"
    assert not ws0[rows:].any() and torch.equal(outs[0][1], outs[1][1])
    _check(outs[1][1], _gn64(X, B, HW, C_, gamma, beta, 1e-5, 0), dt, f"groupnorm B{B} HW{HW} C{C_}")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_small_kernel_parity(L, ldx, dt):
    """The one-launch kernel (whole 16-byte chunks per group, few elements per group): it writes no rows, so only parity."""
    td, code = DT[dt]
    B, HW, C_ = 1, 77, 1280
    g = torch.Generator(device="cuda").manual_seed(11)
    X = (torch.randn(B * HW, C_, device="cuda", generator=g) * 1.5 + 0.4).to(td)
    gamma, beta = _affine(C_, 5)
    ws = torch.full((int(L.ldx_op_groupnorm_workspace_floats(B, G)),), T.SENTINEL, device="cuda")
    Y = torch.zeros_like(X)
    ldx.lib.check(L.ldx_op_groupnorm(_p(X), C_, _p(Y), C_, B, HW, C_, G, 1e-5, 1, _p(gamma), _p(beta), _p(ws), code, _st()), "groupnorm")
    torch.cuda.synchronize()
    assert (ws == T.SENTINEL).all(), "this shape was chosen for the one-launch kernel, which writes no statistics rows"
    _check(Y, _gn64(X, B, HW, C_, gamma, beta, 1e-5, 1), dt, "gn_small")


# ---- 4. parity on realistic data ------------------------------------------------------------------------------------------------------------------------
def _produce_random(L, ldx, c, dt, seed, bias_shift=None, pro=0):
    td, code = DT[dt]
    t = _rand_tensors(c, td, seed, bias_shift)
    Y = torch.zeros(T.rows_total(c), c.N, device="cuda", dtype=td)
    partial = _partial_buffer(c)
    rc, n = _produce(L, c, t, code, Y, partial, pro=pro, norm=_affine(c.Cin, seed + 1) if pro else None)
    ldx.lib.check(rc, f"producer {c.name}")
    torch.cuda.synchronize()
    assert n == T.expected_chunks(c) and torch.isfinite(Y).all()
    return Y, partial, n


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("c,pro", [(c, 0) for c in T.CASES] + [(T.BY_NAME["M1"], 1)], ids=[c.name for c in T.CASES] + ["M1-ln"])
def test_groupnorm_from_producer_rows_vs_fp64(L, ldx, dt, c, pro):
    td, code = DT[dt]
    if c.pick:
        assert T.probe(L, c) == (c.pick, c.chunks)
    i = T.CASES.index(c) + pro
    eps, silu = (1e-5, 1e-6)[i % 2], (i // 2) % 2
    Y, partial, n = _produce_random(L, ldx, c, dt, 100 + i, pro=pro)
    gamma, beta = _affine(c.N, 9 + i)
    out = _apply_from_rows(L, ldx, Y, c.N, c, partial, n, gamma, beta, eps, silu, td, code)
    torch.cuda.synchronize()
    _check(out, _gn64(Y, c.B, T.hw(c), c.N, gamma, beta, eps, silu), dt, f"{c.name} pro{pro} eps{eps:g} silu{silu}")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("name", ["A", "E", "M1"])
def test_rowgemm_groupnorm_prologue_on_producer_rows(L, ldx, dt, name):
    """rowgemm's pro = 2 (GroupNorm apply in front of proj_in) fed the rows a real producer wrote, against fp64 and against the separate launches."""
    td, code = DT[dt]
    c = T.BY_NAME[name]
    M, HW, K = T.rows_total(c), T.hw(c), c.N
    Y, partial, n = _produce_random(L, ldx, c, dt, 40 + ord(name[0]))
    g = torch.Generator(device="cuda").manual_seed(ord(name[0]))
    W = (torch.randn(K, K, device="cuda", generator=g) / math.sqrt(K)).to(td)
    bias = 0.1 * torch.randn(K, device="cuda", generator=g)
    gamma, beta = _affine(K, 21)
    eps = 1e-6
    ref = _gn64(Y, c.B, HW, K, gamma, beta, eps, 0) @ W.double().t() + bias.double()
    n16 = _apply_from_rows(L, ldx, Y, K, c, partial, n, gamma, beta, eps, 0, td, code)
    sep = torch.zeros(M, K, device="cuda", dtype=td)
    ldx.lib.check(L.ldx_op_gemm(_p(n16), K, _p(W), M, K, K, _p(bias), None, 0, 1, 0, None, 0, _p(sep), K, None, 0, code, _st()), "gemm")
    Z = torch.zeros(M, K, device="cuda", dtype=td)
    ldx.lib.check(L.ldx_op_rowgemm(_p(Y), K, _p(Z), K, M, K, K, _p(W), _p(bias), None, 0, 2, _p(gamma), _p(beta), eps, _p(partial), n, HW, code, _st()), "rowgemm")
    torch.cuda.synchronize()
    r_f, r_s = _err(Z, ref)[0], _err(sep, ref)[0]
    print(f"{dt} {name}: rowgemm(pro 2) vs fp64 {r_f:.2e}, separate launches {r_s:.2e}")
    assert torch.isfinite(Z).all() and r_f <= ROWGEMM_TOL[dt] and r_f <= 1.5 * r_s + 1e-4


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("sc", [1, 3, 256, 257, 1000])
def test_groupnorm_stats_on_ragged_rows(L, ldx, dt, sc):
    """Hand-made rows over an uneven split of the pixels (empty chunks included); 257 and 1000 go through the fold, whose last run is short."""
    td, code = DT[dt]
    B, HW, C_ = 2, 2048, 320
    g = torch.Generator(device="cuda").manual_seed(sc)
    X = (torch.randn(B * HW, C_, device="cuda", generator=g) * 1.5 + 0.4).to(td)
    cuts = torch.randint(0, HW + 1, (sc - 1,), device="cuda", generator=g).sort().values
    bounds = torch.cat([torch.zeros(1, dtype=torch.long, device="cuda"), cuts, torch.full((1,), HW, dtype=torch.long, device="cuda")])
    xs = X.double().view(B, HW, G, C_ // G)
    per_pixel = torch.stack([xs.sum(3), (xs * xs).sum(3)], -1)                                       # [B][HW][G][2]
    cs = torch.cat([torch.zeros(B, 1, G, 2, dtype=torch.float64, device="cuda"), per_pixel.cumsum(1)], 1)
    rows = (cs[:, bounds[1:]] - cs[:, bounds[:-1]]).float().contiguous()                            # [B][sc][G][2]
    nf = int(L.ldx_op_groupnorm_stats_floats(B, G, sc))
    assert nf >= rows.numel() + (B * T.GN_FOLD * G * 2 if sc > T.GN_NCHUNK else 0)
    ws = torch.full((nf,), float("nan"), device="cuda")
    ws[:rows.numel()] = rows.flatten()
    gamma, beta = _affine(C_, sc)
    eps, silu = (1e-5, 1e-6)[sc % 2], sc % 3 == 0
    Y = torch.zeros_like(X)
    ldx.lib.check(L.ldx_op_groupnorm_stats(_p(X), C_, _p(Y), C_, B, HW, C_, G, eps, int(silu), _p(gamma), _p(beta), _p(ws), sc, code, _st()), "groupnorm_stats")
    torch.cuda.synchronize()
    assert torch.equal(ws[:rows.numel()], rows.flatten()), "the caller's rows are read, not written"
    if sc <= T.GN_NCHUNK:
        assert torch.isnan(ws[rows.numel():]).all(), "no fold: nothing behind the rows is written"
    _check(Y, _gn64(X, B, HW, C_, gamma, beta, eps, silu), dt, f"stats_chunks {sc}")


# ---- 5. conditioning of var = E[x^2] - mean^2 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("route", ["plain", "E"])
@pytest.mark.parametrize("ratio", [0, 4, 16, 64])
def test_one_pass_variance_conditioning(L, ldx, dt, route, ratio):
    """B 2, HW 4096 with every group's mean at `ratio` standard deviations: through the GroupNorm's own pass (C 320) and through case E's tile epilogue (C 640).
    Asserted up to 16; 64 is the known limit of the one-pass formula in fp32 — measured and printed, the figure is in DESIGN.md."""
    td, code = DT[dt]
    gamma_seed = 31 + ratio
    if route == "plain":
        B, HW, C_ = 2, 4096, 320
        g = torch.Generator(device="cuda").manual_seed(ratio)
        X = (torch.randn(B * HW, C_, device="cuda", generator=g) + ratio).to(td)
        gamma, beta = _affine(C_, gamma_seed)
        out = torch.zeros_like(X)
        ws = torch.zeros(int(L.ldx_op_groupnorm_workspace_floats(B, G)), device="cuda")
        ldx.lib.check(L.ldx_op_groupnorm(_p(X), C_, _p(out), C_, B, HW, C_, G, 1e-5, 0, _p(gamma), _p(beta), _p(ws), code, _st()), "groupnorm")
    else:
        c = T.BY_NAME["E"]
        B, HW, C_ = c.B, T.hw(c), c.N
        assert (B, HW) == (2, 4096)
        X, partial, n = _produce_random(L, ldx, c, dt, 70 + ratio, bias_shift=float(ratio))      # conv output: std ~ 1, mean = the bias
        gamma, beta = _affine(C_, gamma_seed)
        out = _apply_from_rows(L, ldx, X, C_, c, partial, n, gamma, beta, 1e-5, 0, td, code)
    torch.cuda.synchronize()
    ref = _gn64(X, B, HW, C_, gamma, beta, 1e-5, 0)
    xg = X.double().view(B, HW, G, C_ // G)
    measured = float((xg.mean((1, 3)).abs() / xg.std((1, 3))).mean())
    rel, mx = _err(out, ref)
    print(f"conditioning {dt} {route} ratio {ratio} (measured {measured:.1f}): rel-L2 {rel:.3e} max {mx:.3e}")
    assert torch.isfinite(out).all()
    if ratio <= 16:
        assert abs(measured - ratio) <= 0.15 * ratio + 0.1
        assert rel <= TOL[dt][0] and mx <= TOL[dt][1], f"ratio {ratio}: rel-L2 {rel:.3e} max {mx:.3e}"
