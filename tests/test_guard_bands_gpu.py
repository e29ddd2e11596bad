"""NaN-poisoned guard bands around every single-op kernel (include/ldx.h, the single-op section: a kernel reads meaning only from, and writes only to, the
logical extent of its operands).

Every case lays its operands out with tests/_guarded.py (256 guard rows in front of and behind every matrix, ld padding behind every row, 256 guard elements
around every fp32 vector; fused q|k|v, [K | V] and [value | gate] matrices embedded whole) and launches the same logical problem four times on one stream:
(a) zero surroundings, (b) zero again, (c) quiet NaNs, (d) the type's largest finite value with alternating sign.  Asserted, all exact (integer views):
  1. determinism   (b) is bit-identical to (a) in every logical output: what the differential test rests on;
  2. independence  (c) and (d) are bit-identical to (a);
  3. containment   in all four runs nothing outside the logical outputs changed (outputs, caller-provided workspaces and statistics rows start as a
                   sentinel NaN; an operand updated in place is compared with its own snapshot);
  4. sanity        (a) agrees with the fp32 torch reference of the op under bounds that already exist: TOL of tests/test_ops_gpu.py (restated below), and for
                   the fused blocks, rowgemm, skinny, the bias attention and the phase-form up conv the bounds of their own test files, named at each use.
Weights keep tight allocations of their logical rows and integer arguments are never poisoned.  Kernel families are asserted through ldx_op_gemm_pick /
ldx_op_attn_pick at the smallest shape the probes give each; a family that refuses ragged extents runs at its exact-multiple shape.

Run with tight strides because the entry point has no stride argument: ldx_taesd_conv64 (64-channel dense rows), the rel operand of ldx_op_sam_attention, the
fp32 statistics of ldx_op_rowgemm / ldx_op_groupnorm_stats and the GroupNorm workspace; their guard rows are poisoned all the same.  ldx_op_rowgemm with the
GroupNorm prologue (pro = 2) takes whole images of whole row blocks only, so its M is exact there.  No entry point answered LDX_EINVAL to a padded ld.

Not covered: the MX fp8 entry points (tests/_guarded.py names them): their byte and E8M0 buffers need a poison of their own."""
import ctypes as C
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _guarded as G  # noqa: E402

pytestmark = pytest.mark.gpu

DT = {"bf16": (torch.bfloat16, 0), "f16": (torch.float16, 1)}
TOL = {"bf16": (4e-3, 2e-2), "f16": (6e-4, 4e-3)}          # tests/test_ops_gpu.py: rel-L2, max-abs relative to the output scale
ROWGEMM_TOL = {"bf16": 5e-3, "f16": 7e-4}                   # tests/test_rowgemm_gpu.py
BLOCK_TOL = {"bf16": 4e-3, "f16": 6e-4}                     # tests/test_xattn_block_gpu.py, tests/test_ff_block_gpu.py: the block's output against fp32 torch
BIAS_ATTN_TOL = {"bf16": 1e-2, "f16": 2e-3}                 # tests/test_t5_gpu.py
GEMM_FAMILIES = ("tile", "tile2", "pingpong", "pingpong2", "ring", "conv_patch")
ATTN_FAMILIES = ("attn", "attn32", "attn32ap", "attn32g", "attn40p", "attn128p", "attn512")
DEV = "cuda"


def _check(got, ref, dt, scale=1.0, what=""):
    got, ref = got.float(), ref.float()
    rel = float((got - ref).norm() / (ref.norm() + 1e-20))
    mx = float((got - ref).abs().max() / (ref.abs().max() + 1e-20))
    r, m = TOL[dt]
    assert math.isfinite(rel) and rel <= r * scale and mx <= m * scale, f"{what}: rel-L2 {rel:.3e} max {mx:.3e}"


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _p(t, off=0):
    return None if t is None else C.c_void_p(t.data_ptr() + off * t.element_size())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def L(ldx_lib):
    assert torch.cuda.is_available()
    return ldx_lib


class _Rand:
    def __init__(self, seed):
        self.g = torch.Generator(device=DEV).manual_seed(seed)

    def __call__(self, *shape):
        return torch.randn(*shape, device=DEV, generator=self.g)


def _four(op, what):
    rep = G.four_launches(op, sync=torch.cuda.synchronize)
    bad = {p: G.violations(rep, p) for p in ("containment", "determinism", "independence")}
    print(f"{what}: " + ", ".join(f"{p} {v or 'ok'}" for p, v in bad.items()))
    assert not bad["containment"], f"{what}: elements written outside the logical outputs: {bad['containment']}"
    assert not bad["determinism"], f"{what}: two clean launches differ: {bad['determinism']}"
    assert not bad["independence"], f"{what}: the logical output depends on its surroundings (differing elements): {bad['independence']}"
    rep["sanity"]()


def _gemm_pick(L, M, N, K, geglu=0, conv=None, second=(0, 0, 0)):
    out = (C.c_int32 * 10)()
    assert L.ldx_op_gemm_pick(M, N, K, 1 if conv else 0, geglu, -1, 0, 0, 0, *(conv or (0,) * 6), *second, 0, 0, 0, out) == 0
    return GEMM_FAMILIES[out[0]], out[1], out[2], out[6], out[7]          # family, BM, BN, K splits, reduce


def _attn_pick(L, B, H, Nq, Mk, D, causal, bias, ldq, ldk, ldv, ldo):
    out = (C.c_int32 * 13)()
    assert L.ldx_op_attn_pick(B, H, Nq, Mk, D, causal, bias, 0, ldq, ldk, ldv, ldo, 1, out) == 0
    return ATTN_FAMILIES[out[0]], out[10]                                # family, key splits


# ---- ldx_op_gemm ----------------------------------------------------------------------------------------------------------------------------------
GEMM_CASES = {
    # M, N, K, every epilogue operand, (family, BM, BN), K splits.  Ragged M against BM, N no multiple of BN, K a multiple of 8 only — where the family takes it:
    "tile_all": (300, 200, 136, True, ("tile", 64, 64), 1),
    "tile_c_only": (130, 72, 200, False, ("tile", 64, 64), 1),
    "splitk_all": (130, 72, 2560, True, ("tile", 128, 128), 8),              # K splits need whole 64-wide K-tiles; eight splits and their reduce launch
    "splitk_c_only": (300, 200, 2624, False, ("tile", 128, 128), 8),
    "pingpong_all": (5100, 1272, 1032, True, ("pingpong", 256, 128), 1),
    "ring_all": (1530, 1280, 640, True, ("ring", 64, 160), 1),               # the ring kernel takes N % 160 == 0 and K % 64 == 0 only
    "ring_c_only": (1530, 1280, 320, False, ("ring", 64, 160), 1),
}


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("case", list(GEMM_CASES))
def test_gemm(L, ldx, dt, case):
    M, N, K, full, fam, splits = GEMM_CASES[case]
    td, code = DT[dt]
    pick = _gemm_pick(L, M, N, K)
    assert pick[:3] == fam and pick[3] == splits and pick[4] == (1 if splits > 1 else 0), pick
    nb = 4
    rpb = (M + nb - 1) // nb

    def op(a):
        rn = _Rand(M + N + K)
        A, W = rn(M, K).to(td), (rn(N, K) / math.sqrt(K)).to(td)
        bias, rowvec, R = rn(N), rn(nb, N), rn(M, N).to(td)
        Ad = a.inp(A, K + 8)
        bd, rvd, Rd = (a.inp(bias), a.inp(rowvec, N + 8), a.inp(R, N + 16)) if full else (None, None, None)
        Cd = a.out(M, N, td, DEV, N + 8, "C")
        Cf = a.out(M, N, torch.float32, DEV, N + 8, "Cf") if full else None
        ldx.lib.check(L.ldx_op_gemm(_p(Ad), K + 8, _p(W), M, N, K, _p(bd), _p(rvd), N + 8, rpb, 0, _p(Rd), N + 16, _p(Cd), N + 8, _p(Cf), N + 8, code, _st()), "gemm")

        def sanity():
            ref = A.float() @ W.float().T
            if full:
                ref = ref + bias + rowvec[torch.arange(M, device=DEV) // rpb] + R.float()
                _check(Cf, ref, "f16", what=f"gemm {case} Cf32")
            _check(Cd, ref, dt, what=f"gemm {case} C16")
        return sanity
    _four(op, f"gemm {case} {dt}")


def _geglu_rows(inner):
    idx = torch.arange(2 * inner, device=DEV)
    slab, within = idx // 64, idx % 64
    return torch.where(within < 32, slab * 32 + within, inner + slab * 32 + (within - 32))


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("M,inner,K,fam", [(300, 160, 136, ("tile", 128, 128)), (2100, 2816, 648, ("pingpong", 256, 256))])
def test_gemm_geglu(L, ldx, dt, M, inner, K, fam):
    """The GEGLU epilogue on the register-staged tile and on the 256-wide ping-pong tile; [value | gate] slabs are one fused weight matrix, the output has ldc > inner."""
    td, code = DT[dt]
    assert _gemm_pick(L, M, 2 * inner, K, geglu=1)[:3] == fam

    def op(a):
        rn = _Rand(M + inner)
        A, Wf, bf = rn(M, K).to(td), (rn(2 * inner, K) / math.sqrt(K)).to(td), rn(2 * inner)
        src = _geglu_rows(inner)
        Ad, bd = a.inp(A, K + 8), a.inp(bf[src].contiguous())
        Wp = Wf[src].contiguous()
        out = a.out(M, inner, td, DEV, inner + 8)
        ldx.lib.check(L.ldx_op_gemm(_p(Ad), K + 8, _p(Wp), M, 2 * inner, K, _p(bd), None, 0, 1, 1, None, 0, _p(out), inner + 8, None, 0, code, _st()), "geglu")

        def sanity():
            v, gate = (A.float() @ Wf.float().T + bf).chunk(2, dim=-1)
            _check(out, v * F.gelu(gate), dt, what="geglu")
        return sanity
    _four(op, f"geglu M{M} inner{inner} {dt}")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("P1,P2,fam", [((300, 200, 136), (150, 72, 72), ("tile2", 128, 128)),                   # both ragged in M, N and K, and unlike each other
                                       ((1600, 3000, 1032), (520, 1000, 1096), ("pingpong2", 256, 128))])      # the smallest pair the probe sends to the 256-row tiles
def test_gemm2(L, ldx, dt, P1, P2, fam):
    td, code = DT[dt]
    assert _gemm_pick(L, *P1, second=P2)[:3] == fam

    def op(a):
        rn = _Rand(11)
        ops = []
        for i, (M, N, K) in enumerate((P1, P2)):
            A, W, b = rn(M, K).to(td), (rn(N, K) / math.sqrt(K)).to(td), rn(N)
            ops.append((A, W, b, a.inp(A, K + 8 + 8 * i), a.inp(b), a.out(M, N, td, DEV, N + 8 + 8 * i, f"C{i + 1}")))
        (A1, W1, b1, A1d, b1d, C1), (A2, W2, b2, A2d, b2d, C2) = ops
        ldx.lib.check(L.ldx_op_gemm2(_p(A1d), P1[2] + 8, _p(W1), *P1, _p(b1d), _p(C1), P1[1] + 8,
                                     _p(A2d), P2[2] + 16, _p(W2), *P2, _p(b2d), _p(C2), P2[1] + 16, code, _st()), "gemm2")

        def sanity():
            _check(C1, A1.float() @ W1.float().T + b1, dt, what="gemm2 first")
            _check(C2, A2.float() @ W2.float().T + b2, dt, what="gemm2 second")
        return sanity
    _four(op, f"gemm2 {fam[0]} {dt}")


# ---- convolutions ---------------------------------------------------------------------------------------------------------------------------------
CONV_CASES = {
    # B, Hin, Win, Cin, Cout, stride, Hout, Wout, resize, epilogue operands besides the bias ("rv": rowvec, "R": residual), (family, BM, BN), K splits
    "stride1_odd": (2, 9, 7, 64, 72, 1, 9, 7, 0, "rvR", ("tile", 64, 64), 1),
    "stride2_odd": (2, 17, 13, 128, 72, 2, 9, 7, 0, "rvR", ("tile", 64, 64), 1),
    "resize_odd": (1, 5, 7, 64, 72, 1, 9, 13, 1, "rvR", ("tile", 64, 64), 1),
    "cout4": (1, 9, 7, 64, 4, 1, 9, 7, 0, "rvR", ("tile", 128, 32), 1),
    "splitk": (1, 15, 13, 640, 640, 1, 15, 13, 0, "rvR", ("tile", 128, 128), 16),
    "patch": (1, 256, 512, 64, 32, 1, 256, 512, 0, "R", ("conv_patch", 512, 32), 1),          # whole 16 x 32-pixel tiles, at least 256 of them; takes no rowvec
    "patch_cout4": (1, 128, 256, 64, 4, 1, 128, 256, 0, "", ("conv_patch", 512, 16), 1),      # the narrow form: 64 tiles, element-wise epilogue (bias only)
}


def _conv_ref(X, Wt, bias, B, Hin, Win, stride, Hout, Wout, resize):
    xin = X.float().view(B, Hin, Win, -1).permute(0, 3, 1, 2)
    if resize:
        xin = F.interpolate(xin, size=(Hout, Wout), mode="nearest")
    ref = F.conv2d(xin, Wt.float(), bias, stride=stride, padding=1)
    assert ref.shape[-2:] == (Hout, Wout)
    return ref.permute(0, 2, 3, 1).reshape(B * Hout * Wout, -1)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("case", list(CONV_CASES))
def test_conv3x3(L, ldx, dt, case):
    B, Hin, Win, Cin, Cout, stride, Hout, Wout, resize, epi, fam, splits = CONV_CASES[case]
    td, code = DT[dt]
    M = B * Hout * Wout
    pick = _gemm_pick(L, M, Cout, 9 * Cin, conv=(Cin, Hin, Win, Hout, Wout, stride))
    assert pick[:3] == fam and pick[3] == splits, pick
    ldxx, ldy, ldr = Cin + 64, Cout + 8, Cout + 16

    def op(a):
        rn = _Rand(sum(CONV_CASES[case][:9]))
        X = rn(B * Hin * Win, Cin).to(td)
        Wt = (rn(Cout, Cin, 3, 3) / math.sqrt(9 * Cin)).to(td)
        Wp = Wt.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin).contiguous()
        bias, rowvec, R = rn(Cout), rn(B, Cout), rn(M, Cout).to(td)
        Xd, bd = a.inp(X, ldxx), a.inp(bias)
        Rd = a.inp(R, ldr) if "R" in epi else None
        rvd = a.inp(rowvec, Cout + 8) if "rv" in epi else None
        Y = a.out(M, Cout, td, DEV, ldy)
        ldx.lib.check(L.ldx_op_conv3x3(_p(Xd), ldxx, _p(Wp), B, Hin, Win, Cin, Cout, stride, Hout, Wout, resize, _p(bd), _p(rvd), Cout + 8, _p(Rd), ldr,
                                       _p(Y), ldy, code, _st()), "conv")

        def sanity():
            ref = _conv_ref(X, Wt, bias, B, Hin, Win, stride, Hout, Wout, resize)
            if "R" in epi:
                ref = ref + R.float()
            if "rv" in epi:
                ref = ref + rowvec.repeat_interleave(Hout * Wout, 0)
            _check(Y, ref, dt, what=f"conv {case}")
        return sanity
    _four(op, f"conv {case} {dt}")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_conv3x3_skip(L, ldx, dt):
    td, code = DT[dt]
    B, H, W, Cin, Cin2, Cout = 1, 11, 9, 128, 64, 192
    M = B * H * W
    assert _gemm_pick(L, M, Cout, 9 * Cin + Cin2, conv=(Cin, H, W, H, W, 1))[0] == "tile"

    def op(a):
        rn = _Rand(7)
        X, X2 = rn(M, Cin).to(td), rn(M, Cin2).to(td)
        W3, W1 = (rn(Cout, Cin, 3, 3) / math.sqrt(9 * Cin)).to(td), (rn(Cout, Cin2) / math.sqrt(Cin2)).to(td)
        Wp = torch.cat([W3.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin), W1], dim=1).contiguous()
        bias = rn(Cout)
        Xd, X2d, bd = a.inp(X, Cin + 64), a.inp(X2, Cin2 + 8), a.inp(bias)
        Y = a.out(M, Cout, td, DEV, Cout + 8)
        ldx.lib.check(L.ldx_op_conv3x3_skip(_p(Xd), Cin + 64, _p(X2d), Cin2 + 8, Cin2, _p(Wp), B, H, W, Cin, Cout, _p(bd), _p(Y), Cout + 8, code, _st()), "conv+skip")

        def sanity():
            _check(Y, _conv_ref(X, W3, bias, B, H, W, 1, H, W, 0) + X2.float() @ W1.float().T, dt, what="conv+skip")
        return sanity
    _four(op, f"conv3x3_skip {dt}")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_upconv2x(L, ldx, dt):
    """The phase form against fp32 torch under its own file's rule (tests/test_upconv_phase_gpu.py): at most twice the rel-L2 of the nine-tap path, which itself
    is held to TOL here."""
    td, code = DT[dt]
    B, Hin, Win, Cin, Cout = 2, 5, 16, 64, 48
    M = B * 4 * Hin * Win

    def op(a):
        rn = _Rand(13)
        X = rn(B * Hin * Win, Cin).to(td)
        Wt = (rn(Cout, Cin, 3, 3) / math.sqrt(9 * Cin)).to(td)
        Wp = Wt.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin).contiguous()
        bias = rn(Cout)
        Xd, bd = a.inp(X, Cin + 8), a.inp(bias)
        Y = a.out(M, Cout, td, DEV, Cout + 8)
        ldx.lib.check(L.ldx_op_upconv2x(_p(Xd), Cin + 8, _p(Wp), B, Hin, Win, Cin, Cout, _p(bd), _p(Y), Cout + 8, code, _st()), "upconv2x")

        def sanity():
            ref = _conv_ref(X, Wt, bias, B, Hin, Win, 1, 2 * Hin, 2 * Win, 1)
            Y9 = torch.empty(M, Cout, device=DEV, dtype=td)
            ldx.lib.check(L.ldx_op_conv3x3(_p(X), Cin, _p(Wp), B, Hin, Win, Cin, Cout, 1, 2 * Hin, 2 * Win, 1, _p(bias), None, 0, None, 0, _p(Y9), Cout, code, _st()), "conv")
            torch.cuda.synchronize()
            _check(Y9, ref, dt, what="nine-tap path")
            r9, rp = _rel(Y9.float(), ref), _rel(Y.float(), ref)
            assert math.isfinite(rp) and rp <= 2 * r9, f"upconv2x: rel-L2 {rp:.3e} against the nine-tap path's {r9:.3e}"
        return sanity
    _four(op, f"upconv2x {dt}")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_taesd_conv64(L, ldx, dt):
    """Dense 64-channel rows (no stride argument): guard rows only.  Nearest x2, bias, 16-bit residual, ReLU, and the fp32 copy with an fp32 residual."""
    td, code = DT[dt]
    B, Hin, Win = 2, 5, 7
    M = B * 4 * Hin * Win

    def op(a):
        rn = _Rand(17)
        X, Wt, bias = rn(B * Hin * Win, 64).to(td), (rn(64, 64, 3, 3) / 24.0).to(td), rn(64)
        Wp = Wt.permute(0, 2, 3, 1).reshape(64, 576).contiguous()
        R, Rf = rn(M, 64).to(td), rn(M, 64)
        Xd, bd, Rd, Rfd = a.inp(X), a.inp(bias), a.inp(R), a.inp(Rf)
        Y1, Y2, Yf = a.out(M, 64, td, DEV, name="Y relu"), a.out(M, 64, td, DEV, name="Y"), a.out(M, 64, torch.float32, DEV, name="Yf")
        ldx.lib.check(L.ldx_taesd_conv64(_p(Xd), _p(Wp), _p(bd), _p(Rd), None, _p(Y1), None, B, Hin, Win, 1, 1, code, _st()), "taesd conv64")
        ldx.lib.check(L.ldx_taesd_conv64(_p(Xd), _p(Wp), _p(bd), None, _p(Rfd), _p(Y2), _p(Yf), B, Hin, Win, 1, 0, code, _st()), "taesd conv64")

        def sanity():
            ref = _conv_ref(X, Wt, bias, B, Hin, Win, 1, 2 * Hin, 2 * Win, 1)
            _check(Y1, (ref + R.float()).clamp_min(0), dt, what="taesd conv64 relu")
            _check(Y2, ref + Rf, dt, what="taesd conv64")
            _check(Yf, ref + Rf, "f16", what="taesd conv64 fp32 copy")
        return sanity
    _four(op, f"taesd_conv64 {dt}")


# ---- norms ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("B,HW,C,silu", [(2, 77, 256, 1),        # 8 channels per group, 616 elements per (image, group), 64 groups in all: the one-launch small form
                                         (2, 300, 320, 0),       # 10 channels per group: the two-pass form
                                         (3, 1029, 64, 1)])      # two-pass, 2 channels per group, rows no multiple of anything
def test_groupnorm(L, ldx, dt, B, HW, C, silu):
    td, code = DT[dt]
    nws = int(L.ldx_op_groupnorm_workspace_floats(B, 32))

    def op(a):
        rn = _Rand(HW + C)
        X, gamma, beta = (rn(B * HW, C) * 2.0 + 0.7).to(td), 1 + 0.1 * rn(C), 0.1 * rn(C)
        Xd, gd, bd = a.inp(X, C + 64), a.inp(gamma), a.inp(beta)
        Y = a.out(B * HW, C, td, DEV, C + 8, "Y")
        ws = a.out(nws, None, torch.float32, DEV, name="workspace")
        ldx.lib.check(L.ldx_op_groupnorm(_p(Xd), C + 64, _p(Y), C + 8, B, HW, C, 32, 1e-5, silu, _p(gd), _p(bd), _p(ws), code, _st()), "gn")

        def sanity():
            ref = F.group_norm(X.float().view(B, HW, C).permute(0, 2, 1), 32, gamma, beta, 1e-5)
            _check(Y, (F.silu(ref) if silu else ref).permute(0, 2, 1).reshape(B * HW, C), dt, what="groupnorm")
        return sanity
    _four(op, f"groupnorm B{B} HW{HW} C{C} {dt}")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("HW,nchunk", [(300, 3), (600, 300)])         # ragged rows applied as they are; more than 256 rows per image: folded into the 64 rows behind them first
def test_groupnorm_stats(L, ldx, dt, HW, nchunk):
    """The caller's rows and the documented fold target behind them are one logical vector, updated in place."""
    td, code = DT[dt]
    B, C, Gn = 2, 320, 32
    nfl = int(L.ldx_op_groupnorm_stats_floats(B, Gn, nchunk))
    assert nfl == B * (nchunk + 64) * Gn * 2

    def op(a):
        rn = _Rand(HW + nchunk)
        X, gamma, beta = (rn(B * HW, C) * 2.0 + 0.7).to(td), 1 + 0.1 * rn(C), 0.1 * rn(C)
        bounds = [0, HW // 5, HW // 2, HW] if nchunk == 3 else list(range(0, HW + 1, HW // nchunk))
        xs = X.float().view(B, HW, Gn, C // Gn)
        rows = torch.stack([torch.stack([xs[:, lo:hi].sum((1, 3)), (xs[:, lo:hi] ** 2).sum((1, 3))], -1) for lo, hi in zip(bounds, bounds[1:])], 1)
        part = torch.zeros(nfl, device=DEV)
        part[:rows.numel()] = rows.reshape(-1)
        Xd, gd, bd = a.inp(X, C + 64), a.inp(gamma), a.inp(beta)
        pd = a.inout(part, name="partial")
        Y = a.out(B * HW, C, td, DEV, C + 8, "Y")
        ldx.lib.check(L.ldx_op_groupnorm_stats(_p(Xd), C + 64, _p(Y), C + 8, B, HW, C, Gn, 1e-5, 1, _p(gd), _p(bd), _p(pd), nchunk, code, _st()), "gn stats")

        def sanity():
            ref = F.silu(F.group_norm(X.float().view(B, HW, C).permute(0, 2, 1), Gn, gamma, beta, 1e-5))
            _check(Y, ref.permute(0, 2, 1).reshape(B * HW, C), dt, what="groupnorm from statistics")
            assert G.same_bits(pd[:rows.numel()], rows.reshape(-1)) == 0, "the caller's rows were rewritten"
        return sanity
    _four(op, f"groupnorm_stats HW{HW} chunks{nchunk} {dt}")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("rows,C", [(9, 64), (9, 320), (5, 4096)])
def test_layernorm(L, ldx, dt, rows, C):
    td, code = DT[dt]

    def op(a):
        rn = _Rand(rows + C)
        X, gamma, beta = (rn(rows, C) * 3 - 1).to(td), 1 + 0.1 * rn(C), 0.1 * rn(C)
        Xd, gd, bd = a.inp(X, C + 8), a.inp(gamma), a.inp(beta)
        Y = a.out(rows, C, td, DEV, C + 16)
        ldx.lib.check(L.ldx_op_layernorm(_p(Xd), C + 8, _p(Y), C + 16, rows, C, 1e-5, _p(gd), _p(bd), code, _st()), "ln")
        return lambda: _check(Y, F.layer_norm(X.float(), (C,), gamma, beta, 1e-5), dt, what="layernorm")
    _four(op, f"layernorm rows{rows} C{C} {dt}")


# ---- attention ------------------------------------------------------------------------------------------------------------------------------------
ATTN_CASES = {
    # B, H, Nq, Mk, D, causal, layout, family.  "qkv": the fused q|k|v matrix; "split": q, k and v each with a padded stride of its own
    "attn_split": (1, 2, 130, 231, 64, 0, "split", "attn"),
    "attn_causal_qkv": (2, 12, 77, 77, 64, 1, "qkv", "attn"),
    "attn32_split": (16, 32, 200, 45, 40, 0, "split", "attn32"),                  # 512 workgroups of 256 queries, fewer than 64 keys
    "attn32ap_split": (16, 32, 200, 77, 40, 0, "split", "attn32ap"),
    "attn32g_qkv": (1, 4, 513, 513, 80, 0, "qkv", "attn32g"),
    "attn32g_split": (1, 2, 1000, 333, 80, 0, "split", "attn32g"),
    "attn40p_qkv": (16, 16, 256, 256, 40, 0, "qkv", "attn40p"),                   # whole 256-query workgroups and whole pairs of key blocks only
    "attn40p_split": (16, 16, 256, 384, 40, 0, "split", "attn40p"),
    "attn128p_qkv": (16, 16, 256, 256, 128, 0, "qkv", "attn128p"),                # the same; 16-byte output rows
    "attn512_split": (1, 1, 300, 333, 512, 0, "split", "attn512"),
    "attn512_keysplits": (2, 1, 130, 2100, 512, 0, "split", "attn512"),           # four key splits and their merge launch
}


def _attn_ref(q, k, v, B, H, D, scale, causal=0, bias=None):
    qf, kf, vf = (t.float().reshape(B, -1, H, D).transpose(1, 2) for t in (q, k, v))
    s = (qf @ kf.transpose(-1, -2)) * scale
    if bias is not None:
        s = s + bias * scale
    if causal:
        s = s.masked_fill(torch.triu(torch.ones(s.shape[-2:], device=DEV, dtype=torch.bool), 1), float("-inf"))
    return (torch.softmax(s, dim=-1) @ vf).transpose(1, 2).reshape(q.shape[0], H * D)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("case", list(ATTN_CASES))
def test_attention(L, ldx, dt, case):
    B, H, Nq, Mk, D, causal, layout, fam = ATTN_CASES[case]
    td, code = DT[dt]
    Cc = H * D
    ldq, ldk, ldv = (3 * Cc + 8,) * 3 if layout == "qkv" else (Cc + 8, Cc + 16, Cc + 24)
    ldo = Cc + 8
    pick = _attn_pick(L, B, H, Nq, Mk, D, causal, 0, ldq, ldk, ldv, ldo)
    assert pick[0] == fam and (case != "attn512_keysplits" or pick[1] == 4), pick
    scale = 1.0 / math.sqrt(D)

    def op(a):
        rn = _Rand(B + H + Nq + Mk + D)
        if layout == "qkv":
            qkv = rn(B * Nq, 3 * Cc).to(td)
            q, k, v = qkv[:, :Cc], qkv[:, Cc:2 * Cc], qkv[:, 2 * Cc:]
            d = a.inp(qkv, ldq)
            ptrs = (_p(d), _p(d, Cc), _p(d, 2 * Cc))
        else:
            q, k, v = rn(B * Nq, Cc).to(td), rn(B * Mk, Cc).to(td), rn(B * Mk, Cc).to(td)
            ds = (a.inp(q, ldq), a.inp(k, ldk), a.inp(v, ldv))
            ptrs = tuple(_p(x) for x in ds)
        O = a.out(B * Nq, Cc, td, DEV, ldo)
        ldx.lib.check(L.ldx_op_attention(ptrs[0], ldq, ptrs[1], ldk, ptrs[2], ldv, _p(O), ldo, B, H, Nq, Mk, D, scale, causal, code, _st()), "attn")
        return lambda: _check(O, _attn_ref(q, k, v, B, H, D, scale, causal), dt, scale=2.0, what=f"attention {case}")      # scale 2: tests/test_ops_gpu.py test_attention
    _four(op, f"attention {case} {dt}")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_attention_bias(L, ldx, dt):
    """Ragged queries and keys; bias rows of bias_ld = 136 floats for 77 keys (128 rounded up): the columns behind the keys and the rows around the table poisoned."""
    td, code = DT[dt]
    B, H, Nq, Mk, D = 2, 4, 130, 77, 64
    Cc, bias_ld = H * D, 136
    assert _attn_pick(L, B, H, Nq, Mk, D, 0, 1, Cc + 8, 2 * Cc + 8, 2 * Cc + 8, Cc + 8)[0] == "attn"
    scale = 1.0 / math.sqrt(D)

    def op(a):
        rn = _Rand(23)
        q, kv, bias = rn(B * Nq, Cc).to(td), rn(B * Mk, 2 * Cc).to(td), rn(H * Nq, Mk) * 2.0
        qd, kvd, bd = a.inp(q, Cc + 8), a.inp(kv, 2 * Cc + 8), a.inp(bias, bias_ld)
        O = a.out(B * Nq, Cc, td, DEV, Cc + 8)
        ldx.lib.check(L.ldx_op_attention_bias(_p(qd), Cc + 8, _p(kvd), 2 * Cc + 8, _p(kvd, Cc), 2 * Cc + 8, _p(O), Cc + 8, B, H, Nq, Mk, D, scale,
                                              _p(bd), bias_ld, Nq * bias_ld, code, _st()), "attn bias")

        def sanity():
            r = _rel(O.float(), _attn_ref(q, kv[:, :Cc], kv[:, Cc:], B, H, D, scale, bias=bias.view(1, H, Nq, Mk)))
            assert math.isfinite(r) and r <= BIAS_ATTN_TOL[dt], r
        return sanity
    _four(op, f"attention_bias {dt}")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_sam_attention(L, ldx, dt):
    """Windows of 7 x 7 tokens (49: ragged against the query tile), fused q|k|v with a padded stride, ldo > H * 64; the fp32 rel-pos terms have no stride argument."""
    td, code = DT[dt]
    BW, H, n = 3, 2, 7
    N, Cc = n * n, H * 64
    ld, ldo = 3 * Cc + 8, Cc + 4

    def op(a):
        rn = _Rand(29)
        qkv, relv = rn(BW * N, 3 * Cc).to(td), rn(BW * H * N, 2 * n)
        d, rd = a.inp(qkv, ld), a.inp(relv)
        O = a.out(BW * N, Cc, td, DEV, ldo)
        ldx.lib.check(L.ldx_op_sam_attention(_p(d), _p(d, Cc), _p(d, 2 * Cc), ld, _p(rd), _p(O), ldo, BW, H, n, 0.125, code, _st()), "sam attention")

        def sanity():
            r = relv.view(BW, H, N, 2 * n)
            bias = (r[..., :n, None] + r[..., None, n:]).reshape(BW, H, N, N)
            ref = _attn_ref(qkv[:, :Cc], qkv[:, Cc:2 * Cc], qkv[:, 2 * Cc:], BW, H, 64, 0.125, bias=bias / 0.125)
            _check(O, ref, dt, scale=2.0, what="sam attention")
        return sanity
    _four(op, f"sam_attention {dt}")


# ---- fused transformer sub-blocks and the row-block GEMM ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("Mk", [13, 77, 80])
def test_xattn_block(L, ldx, dt, Mk):
    """H is updated in place with ldh > C; the projected context is the fused [K | V] matrix with a padded stride, and the rows behind image B - 1 are guard rows."""
    td, code = DT[dt]
    B, N, Cc, Hh, D = 2, 128, 320, 8, 40
    M, ldh, ldkv = B * N, Cc + 8, 2 * Cc + 8
    scale = 1.0 / math.sqrt(D)

    def op(a):
        rn = _Rand(Mk)
        h, gamma, beta = (rn(M, Cc) * 1.5 + 0.3).to(td), 1 + 0.1 * rn(Cc), 0.1 * rn(Cc)
        Wq, Wo, bo, kv = (rn(Cc, Cc) / math.sqrt(Cc)).to(td), (rn(Cc, Cc) / math.sqrt(Cc)).to(td), 0.1 * rn(Cc), rn(B * Mk, 2 * Cc).to(td)
        hd, gd, bd, bod, kvd = a.inout(h, ldh, "H"), a.inp(gamma), a.inp(beta), a.inp(bo), a.inp(kv, ldkv)
        ldx.lib.check(L.ldx_op_xattn_block(_p(hd), ldh, M, N, Cc, Hh, _p(gd), _p(bd), 1e-5, _p(Wq), _p(Wo), _p(bod), _p(kvd), ldkv, _p(kvd, Cc), ldkv, Mk, scale, code, _st()), "xattn")

        def sanity():
            x = h.float()
            q = F.layer_norm(x, (Cc,), gamma, beta, 1e-5) @ Wq.float().t()
            ref = x + _attn_ref(q, kv[:, :Cc], kv[:, Cc:], B, Hh, D, scale) @ Wo.float().t() + bo
            r = _rel(hd.float(), ref)
            assert math.isfinite(r) and r <= BLOCK_TOL[dt], r
        return sanity
    _four(op, f"xattn_block Mk{Mk} {dt}")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_ff_block(L, ldx, dt):
    td, code = DT[dt]
    M, Cc, inner, ldh = 1000, 320, 1280, 328

    def op(a):
        rn = _Rand(31)
        h, gamma, beta = (rn(M, Cc) * 1.5 + 0.3).to(td), 1 + 0.1 * rn(Cc), 0.1 * rn(Cc)
        W1, b1, W2, b2 = (rn(2 * inner, Cc) / math.sqrt(Cc)).to(td), 0.1 * rn(2 * inner), (rn(Cc, inner) / math.sqrt(inner)).to(td), 0.1 * rn(Cc)
        perm = _geglu_rows(inner)
        W1e = W1[perm].contiguous()
        hd, gd, bd, b1d, b2d = a.inout(h, ldh, "H"), a.inp(gamma), a.inp(beta), a.inp(b1[perm].contiguous()), a.inp(b2)
        ldx.lib.check(L.ldx_op_ff_block(_p(hd), ldh, M, Cc, inner, _p(gd), _p(bd), 1e-5, _p(W1e), _p(b1d), _p(W2), _p(b2d), code, _st()), "ff block")

        def sanity():
            x = h.float()
            t = F.layer_norm(x, (Cc,), gamma, beta, 1e-5) @ W1.float().t() + b1
            r = _rel(hd.float(), x + (t[:, :inner] * F.gelu(t[:, inner:])) @ W2.float().t() + b2)
            assert math.isfinite(r) and r <= BLOCK_TOL[dt], r
        return sanity
    _four(op, f"ff_block {dt}")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("K", [320, 640])
@pytest.mark.parametrize("pro", [0, 1, 2])
def test_rowgemm(L, ldx, dt, pro, K):
    """Ragged M against the row block (128 rows at K = 320, 64 at K = 640) for pro 0 and 1; the GroupNorm prologue takes whole images of whole row blocks only."""
    td, code = DT[dt]
    B, HW = 2, 384
    M = B * HW if pro == 2 else 333
    N = 3 * K if pro == 1 else K
    ldxx, ldy, ldr = K + 8, N + 8, N + 16
    nchunk = 3 if pro == 2 else 0

    def op(a):
        rn = _Rand(pro * 7 + K)
        X, W, bias = (rn(M, K) * 1.5 + 0.4).to(td), (rn(N, K) / math.sqrt(K)).to(td), 0.1 * rn(N)
        gamma, beta, R = 1 + 0.1 * rn(K), 0.1 * rn(K), rn(M, N).to(td)
        eps, part = 1e-5, None
        if pro == 2:
            eps = 1e-6
            bounds = [0, HW // 5, HW // 2, HW]
            xs = X.float().view(B, HW, 32, K // 32)
            part = torch.stack([torch.stack([xs[:, lo:hi].sum((1, 3)), (xs[:, lo:hi] ** 2).sum((1, 3))], -1) for lo, hi in zip(bounds, bounds[1:])], 1).reshape(-1)
        Xd, bd, Rd = a.inp(X, ldxx), a.inp(bias), a.inp(R, ldr)
        gd, btd = (a.inp(gamma), a.inp(beta)) if pro else (None, None)
        pd = a.inp(part) if pro == 2 else None
        Y = a.out(M, N, td, DEV, ldy)
        ldx.lib.check(L.ldx_op_rowgemm(_p(Xd), ldxx, _p(Y), ldy, M, N, K, _p(W), _p(bd), _p(Rd), ldr, pro, _p(gd), _p(btd), eps, _p(pd), nchunk, HW if pro == 2 else 0, code, _st()), "rowgemm")

        def sanity():
            x = X.float()
            n = x if pro == 0 else F.layer_norm(x, (K,), gamma, beta, eps) if pro == 1 else \
                F.group_norm(x.view(B, HW, K).transpose(1, 2), 32, gamma, beta, eps).transpose(1, 2).reshape(M, K)
            r = _rel(Y.float(), n @ W.float().t() + bias + R.float())
            assert math.isfinite(r) and r <= ROWGEMM_TOL[dt], r
        return sanity
    _four(op, f"rowgemm pro{pro} K{K} {dt}")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_skinny(L, ldx, dt):
    """fp32 activations with ldx > K, fp32 output with ldo > N; the bound is tests/test_ops_gpu.py test_skinny's."""
    td, code = DT[dt]
    M, N, K = 6, 1000, 1288

    def op(a):
        rn = _Rand(5)
        x, W, b = rn(M, K), (rn(N, K) / math.sqrt(K)).to(td), rn(N)
        xd, bd = a.inp(x, K + 8), a.inp(b)
        out = a.out(M, N, torch.float32, DEV, N + 4)
        ldx.lib.check(L.ldx_op_skinny(_p(xd), K + 8, _p(W), _p(bd), _p(out), N + 4, M, N, K, 1, 1, code, _st()), "skinny")

        def sanity():
            r = _rel(out, F.silu(F.linear(F.silu(x), W.float(), b)))
            assert math.isfinite(r) and r < 1e-5, r
        return sanity
    _four(op, f"skinny {dt}")
