"""Upsample1 (nearest x2 + conv3x3) in phase form: four 2 x 2 convs over the stored image, one per output parity (GemmArgs::up2x, gemm_pp.inc MODE 2).

Single op (ldx_op_upconv2x) against fp64 F.interpolate(nearest, x2) + conv2d on the stored 16-bit values.  The yardstick for the tolerance is the existing
path on the same inputs, ldx_op_conv3x3(resize_to_out = 1): the phase form adds one rounding of each merged weight (<= 2^-9 relative in bf16, 2^-11 in f16, on
sums of 1, 2 or 4 taps), which can grow the error by about sqrt(2); the assertion allows 2x the existing path's rel-L2, on the whole output, on each of the
four output parities (a swapped phase cannot average out) and on the first / last row and column of every image.

Engine level: a tiny UNet at a 64 x 32 latent, where the last Upsample sees a stored row of 16 pixels and runs in phase form; LDX_UPCONV_PHASE=0 restores the
9-tap plan.  Both engines against the oracle (the tolerance of tests/test_engine_gpu.py), each other, graph against eager, and an in-place weight refresh
against a fresh engine.
"""
import ctypes as C
import math
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import sd15_oracle as O  # noqa: E402  (checker only)

DT = {"bf16": (torch.bfloat16, 0), "f16": (torch.float16, 1)}
LDX_EINVAL = -1
# B, Hin, Win, Cin, Cout, ldy_extra
CASES = [
    (1, 3, 16, 64, 160, 0),       # 48 rows per phase: a ragged M tile, one K-tile per tap
    (3, 5, 16, 128, 176, 8),      # a tile spans three images, ragged N (160 + 16), output rows wider than Cout
    (2, 16, 32, 64, 320, 0),      # whole tiles, two N tiles
]


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-300))


def _inputs(case, td):
    B, Hin, Win, Cin, Cout, extra = case
    g = torch.Generator(device="cuda").manual_seed(1000 + sum(case))
    X = torch.randn(B, Hin, Win, Cin, device="cuda", generator=g).to(td)
    Wt = (torch.randn(Cout, Cin, 3, 3, device="cuda", generator=g) / math.sqrt(9 * Cin)).to(td)
    W9 = Wt.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin).contiguous()                  # [Cout][ky][kx][Cin]
    bias = torch.randn(Cout, device="cuda", generator=g)
    return X, Wt, W9, bias


@pytest.fixture(scope="module")
def L(ldx_lib):
    assert torch.cuda.is_available()
    return ldx_lib


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("case", CASES)
def test_upconv2x_against_fp64_and_the_nine_tap_path(L, ldx, dt, case):
    td, code = DT[dt]
    B, Hin, Win, Cin, Cout, extra = case
    Ho, Wo, ldy = 2 * Hin, 2 * Win, Cout + extra
    X, Wt, W9, bias = _inputs(case, td)
    sentinel = 12345.0
    Yp = torch.full((B * Ho * Wo, ldy), sentinel, device="cuda", dtype=td)
    Y9 = torch.zeros(B * Ho * Wo, Cout, device="cuda", dtype=td)
    ldx.lib.check(L.ldx_op_upconv2x(_p(X), Cin, _p(W9), B, Hin, Win, Cin, Cout, _p(bias), _p(Yp), ldy, code, _st()), "upconv2x")
    ldx.lib.check(L.ldx_op_conv3x3(_p(X), Cin, _p(W9), B, Hin, Win, Cin, Cout, 1, Ho, Wo, 1, _p(bias), None, 0, None, 0, _p(Y9), Cout, code, _st()), "conv3x3")
    torch.cuda.synchronize()
    assert bool((Yp[:, Cout:] == sentinel).all()), "columns behind Cout were written"
    ref = F.conv2d(F.interpolate(X.double().permute(0, 3, 1, 2), scale_factor=2, mode="nearest"), Wt.double(), bias.double(), padding=1)
    ref = ref.permute(0, 2, 3, 1).contiguous()                                        # [B][Ho][Wo][Cout]
    yp, y9 = Yp[:, :Cout].reshape(B, Ho, Wo, Cout), Y9.reshape(B, Ho, Wo, Cout)
    parts = {"all": (slice(None), slice(None))}
    for py in (0, 1):
        for px in (0, 1):
            parts[f"parity ({py},{px})"] = (slice(py, None, 2), slice(px, None, 2))
    parts.update({"first row": (slice(0, 1), slice(None)), "last row": (slice(Ho - 1, Ho), slice(None)),
                  "first column": (slice(None), slice(0, 1)), "last column": (slice(None), slice(Wo - 1, Wo))})
    msgs, bad = [], []
    for name, (sy, sx) in parts.items():
        for b in (range(B) if "row" in name or "column" in name else [slice(None)]):
            ep, e9 = _rel(yp[b, sy, sx], ref[b, sy, sx]), _rel(y9[b, sy, sx], ref[b, sy, sx])
            msgs.append(f"{name}{'' if isinstance(b, slice) else f' image {b}'}: phase {ep:.3e} nine-tap {e9:.3e}")
            if not (math.isfinite(ep) and ep <= 2.0 * e9):
                bad.append(msgs[-1])
    print(f"[{dt}] {case}: " + "; ".join(msgs[:5]))
    assert not bad, f"[{dt}] {case}: rel-L2 against fp64 above twice the nine-tap path's: {bad}; all: {msgs}"


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_upconv2x_refuses_shapes_without_a_phase_form(L, ldx, dt):
    td, code = DT[dt]
    for case in ((1, 4, 24, 64, 160, 0), (1, 4, 16, 96, 160, 0), (1, 4, 16, 64, 168, 0)):      # Win % 16, Cin % 64, Cout % 16
        B, Hin, Win, Cin, Cout, _ = case
        X, Wt, W9, bias = _inputs(case, td)
        Y = torch.zeros(B * 4 * Hin * Win, Cout, device="cuda", dtype=td)
        rc = L.ldx_op_upconv2x(_p(X), Cin, _p(W9), B, Hin, Win, Cin, Cout, _p(bias), _p(Y), Cout, code, _st())
        torch.cuda.synchronize()
        assert rc == LDX_EINVAL, (case, rc)
        assert not bool(Y.any()), case


# ---- engine level
H, W, B = 64, 32, 2
TOL = {"f16": 4e-3, "bf16": 2.5e-2}          # tests/test_engine_gpu.py: one UNet forward against the oracle


def _engine(ldx, cfg, sd, dt, phase, graph=False):
    old = os.environ.get("LDX_UPCONV_PHASE")
    os.environ["LDX_UPCONV_PHASE"] = str(phase)            # read by the engine's constructor
    try:
        return ldx.UNetEngine(cfg, sd, device=0, dtype=dt, graph=graph)
    finally:
        if old is None:
            del os.environ["LDX_UPCONV_PHASE"]
        else:
            os.environ["LDX_UPCONV_PHASE"] = old


def _up_labels(e, x, sigma, ctx):
    e.profile(2)
    e.denoise(x, sigma, ctx)
    torch.cuda.synchronize()
    keys = list(e.profile_report())
    e.profile(False)
    return [k for k in keys if k.endswith(" up2x")]


@pytest.fixture(scope="module")
def net(ldx, ldx_lib):
    cfg = ldx.UNetConfig.tiny(64, 128)
    sd = ldx.weights.synth_state_dict(ldx.weights.unet_state_dict_spec(cfg), seed=4321)
    gen = torch.Generator().manual_seed(5)
    x, sigma, ctx = torch.randn(B, 4, H, W, generator=gen), torch.tensor([3.0, 0.7]), torch.randn(B, 77, cfg.context_dim, generator=gen)
    with torch.no_grad():
        ref = O.apply_model(sd, cfg, x, sigma, ctx)
    return cfg, sd, (x.cuda(), sigma.cuda(), ctx.cuda()), ref


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_engine_phase_form_against_nine_tap_plan_and_oracle(ldx, net, dt):
    cfg, sd, inp, ref = net
    e9, ep = _engine(ldx, cfg, sd, dt, 0), _engine(ldx, cfg, sd, dt, 1)
    y9, yp = e9.denoise(*inp).clone(), ep.denoise(*inp).clone()
    i9, ip = e9.plan_info(), ep.plan_info()
    r9, rp, d = _rel(y9.cpu(), ref), _rel(yp.cpu(), ref), _rel(yp, y9)
    print(f"[{dt}] nine-tap vs oracle {r9:.3e}, phase form vs oracle {rp:.3e}, phase vs nine-tap {d:.3e}; executed {ip['flops_executed'] / 1e9:.3f} of {ip['flops'] / 1e9:.3f} GFLOP")
    assert r9 <= TOL[dt] and rp <= TOL[dt] and d < TOL[dt]
    # LDX_UPCONV_PHASE=2 walks the same tiles in the other order (band-major instead of phase-major): the same bits
    e2 = _engine(ldx, cfg, sd, dt, 2)
    assert torch.equal(e2.denoise(*inp), yp) and len(_up_labels(e2, *inp)) == 1
    # the plan: the default engine runs the 32 x 16 -> 64 x 32 Upsample in phase form, the other none; at 16^2 (stored rows of 8 pixels) and at a height that is
    # no exact double (63: output_shape follows the skip connection) nobody does
    labels = _up_labels(ep, *inp)
    assert len(labels) == 1 and "gemm_kernel<" in labels[0] and ",1>" in labels[0] and f"M{B * H * W} N{2 * cfg.model_channels} K{4 * 2 * cfg.model_channels} " in labels[0], labels
    assert _up_labels(e9, *inp) == []
    gen = torch.Generator().manual_seed(6)
    for h, w in ((16, 16), (63, 32)):
        small = (torch.randn(B, 4, h, w, generator=gen).cuda(), inp[1], inp[2])
        assert _up_labels(ep, *small) == [], (h, w)
    # accounting: the algorithmic count is the reference's arithmetic in both plans; the phase form executes 4/9 of that conv's
    conv = 2.0 * (B * H * W) * (2 * cfg.model_channels) * 9 * (2 * cfg.model_channels)
    assert ip["flops"] == i9["flops"] and i9["flops_executed"] + i9["flops_shared"] == i9["flops"]
    assert abs((i9["flops_executed"] - ip["flops_executed"]) - conv * 5.0 / 9.0) <= 1e-9 * conv


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_engine_phase_form_graph_and_refresh(ldx, net, dt):
    """Graph replay equals the eager pass bit for bit; after an in-place refresh with other up-conv weights the captured graph (same pointers, re-derived
    phase weights) computes what a fresh engine built from those weights computes."""
    cfg, sd, inp, ref = net
    e = _engine(ldx, cfg, sd, dt, 1)
    buf = torch.empty(B, cfg.out_channels, H, W, device="cuda")          # one output buffer: a captured graph is replayed for the pointers it was captured with
    eager = e.denoise(*inp, out=buf).clone()
    e.set_graph_mode(True)
    outs = [e.denoise(*inp, out=buf).clone() for _ in range(3)]         # eager (warm), capture, replay
    assert e.graph_stats()[1] >= 1 and all(torch.equal(o, eager) for o in outs)
    gen = torch.Generator().manual_seed(9)
    sd_b = {k: v.clone() for k, v in sd.items()}
    ups = [k for k in sd_b if k.startswith("output_blocks.") and (k.endswith(".conv.weight") or k.endswith(".conv.bias"))]
    assert len(ups) == 2 * (len(cfg.channel_mult) - 1), ups
    for k in ups:
        sd_b[k] = sd_b[k] + 0.5 * sd_b[k].std() * torch.randn(sd_b[k].shape, generator=gen)
    replays = e.graph_stats()[1]
    e.refresh(sd_b)
    got = e.denoise(*inp, out=buf).clone()
    assert e.graph_stats()[1] == replays + 1, "the refresh dropped the captured graph"
    fresh = _engine(ldx, cfg, sd_b, dt, 1)
    want = fresh.denoise(*inp).clone()
    assert not torch.equal(want, eager), "the changed up-conv weights change the output: the refresh is actually exercised"
    assert torch.equal(got, want), f"refreshed vs fresh engine: rel-L2 {_rel(got, want):.3e}"
