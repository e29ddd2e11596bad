"""TAESD latent previews on the GPU: the weight-resident conv kernel against fp64 (one launch, every fusion flag), the decoder engine against the reference's own
outputs (tests/golden/taesd.npz, tests/tools/capture_taesd.py), the preview bytes, graph mode, and the sampler hook on the tiny UNet.

Measured on an MI355X (tests/golden/taesd.META.txt has every figure): conv64 worst error / bound 0.495; decode rel-L2 3.4e-3 .. 5.8e-3 in bf16 and
4.5e-4 .. 7.1e-4 in f16 against bounds of 9.9e-3 .. 1.47e-2 (all-bf16 restatement) and 6.7e-3 .. 1.15e-2 (the engine's own arithmetic restated); preview bytes off by more than 2 codes: 0 in every case and both formats, where the bounds allow
2 / 2 / 2 / 0 / 0 bytes (base / odd / edges / one / flux).  With the skip stream rounded to bf16 once per Block the bf16 engine had 3 such bytes on edges and
missed that bound; the stream is fp32 for that reason (engine_taesd.cpp, META)."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import capture_taesd as CT  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = [c[0] for c in CT.CASES]


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "taesd.npz"))


@pytest.fixture(scope="module")
def engines(ldx, ldx_lib, fx):
    sd = CT.fixture_state_dict(float(fx["last_scale"]))
    return {dt: ldx.TAESDEngine(ldx.TAESDConfig(), sd, device=0, dtype=dt) for dt in ("bf16", "f16")}


@pytest.fixture(scope="module")
def engine(engines):
    return engines["bf16"]


# ---- one launch of the conv kernel -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def conv_inputs():
    """Per input size: bf16-rounded X [2,H,W,64], weights [64,64,3,3], residuals for both output sizes, bias; fp64 conv and sum |x w| for up = 0 and 1."""
    g = torch.Generator().manual_seed(77)
    out = {}
    w = (torch.randn(64, 64, 3, 3, generator=g) / 24).to(torch.bfloat16)
    bias = 0.5 * torch.randn(64, generator=g)
    F = torch.nn.functional
    for H, W in ((5, 7), (33, 17)):
        x = torch.randn(2, H, W, 64, generator=g).to(torch.bfloat16)
        d = {"x": x, "w": w, "bias": bias}
        for up in (0, 1):
            xi = x.permute(0, 3, 1, 2).double()
            if up:
                xi = F.interpolate(xi, scale_factor=2, mode="nearest")
            d["conv", up] = F.conv2d(xi, w.double(), padding=1).permute(0, 2, 3, 1).contiguous()
            d["abs", up] = F.conv2d(xi.abs(), w.double().abs(), padding=1).permute(0, 2, 3, 1).contiguous()
            d["res", up] = torch.randn(2, H << up, W << up, 64, generator=g).to(torch.bfloat16)
            d["resf", up] = torch.randn(2, H << up, W << up, 64, generator=g)
        out[H, W] = d
    return out


@pytest.mark.parametrize("size", [(5, 7), (33, 17)])
def test_conv64_single_launch_vs_fp64(ldx, ldx_lib, conv_inputs, size):
    """Every combination of bias / ReLU / residual (none, 16-bit, fp32 with the fp32 copy of the result) / upsample, B = 2; the tile is 8 x 32 pixels, so
    33 x 17 crosses tile rows and, upsampled to 66 x 34, tile columns.  Bound per element: one bf16 ulp of the fp64 result (2^-7 |ref|) + 1e-5 sum |x w|
    (fp32 accumulation of 576 bf16 products); the fp32 copy: an fp32 ulp (2^-23 |ref|, and of the larger of its two addends) in place of the bf16 one."""
    H, W = size
    d = conv_inputs[size]
    lib = ldx.lib
    x = d["x"].cuda()
    wp = d["w"].permute(0, 2, 3, 1).reshape(64, 576).contiguous().cuda()          # [n][(ky * 3 + kx) * 64 + ci]
    bias = d["bias"].cuda()
    worst = 0.0
    for has_bias, relu, has_res, up in itertools.product((0, 1), (0, 1), (0, 1, 2), (0, 1)):
        res = d["res", up].cuda() if has_res == 1 else None
        resf = d["resf", up].cuda() if has_res == 2 else None
        y = torch.full((2, H << up, W << up, 64), float("nan"), dtype=torch.bfloat16, device="cuda")
        yf = torch.full(y.shape, float("nan"), dtype=torch.float32, device="cuda") if has_res == 2 else None
        lib.check(ldx_lib.ldx_taesd_conv64(lib.ptr(x), lib.ptr(wp), lib.ptr(bias) if has_bias else None, lib.ptr(res), lib.ptr(resf), lib.ptr(y), lib.ptr(yf),
                                           2, H, W, up, relu, lib.LDX_BF16, lib.current_stream_ptr()), "ldx_taesd_conv64")
        ref = d["conv", up].clone()
        if has_bias:
            ref += d["bias"].double()
        if has_res:
            ref += (d["res", up] if has_res == 1 else d["resf", up]).double()
        if relu:
            ref = ref.clamp_min(0)
        if yf is not None:
            addends = torch.maximum(d["conv", up].abs(), d["resf", up].double().abs()) + float(d["bias"].abs().max())
            errf = (yf.cpu().double() - ref).abs()
            assert bool((errf <= 2.0 ** -22 * addends + 1e-5 * d["abs", up]).all()), (has_bias, relu, up, float(errf.max()))
            assert torch.equal(yf.to(torch.bfloat16), y)          # the 16-bit result is the rounded fp32 one
        err = (y.cpu().double() - ref).abs()
        bound = ref.abs() * 2.0 ** -7 + 1e-5 * d["abs", up]
        ratio = float((err / bound.clamp_min(1e-30)).max())
        worst = max(worst, ratio)
        print(f"conv64 {H}x{W} bias={has_bias} relu={relu} res={has_res} up={up}: max err / bound {ratio:.3f}, max err {float(err.max()):.3e}")
        assert torch.isfinite(y.float()).all() and bool((err <= bound).all()), (has_bias, relu, has_res, up, ratio)
    print(f"conv64 {H}x{W}: worst err / bound {worst:.3f}")


# ---- the decoder against the reference ---------------------------------------------------------------------------------------------------
def _latent(fx, name):
    return torch.from_numpy(fx[f"x_{name}"]).cuda()


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("name", CASES)
def test_decode_vs_reference(engines, fx, name, dt):
    """rel-L2 to the reference's fp32 TAESD.decode within 2 x the distance of the CPU restatement with every activation in bf16, and within 2 x that of
    the restatement of the engine's own arithmetic (fp32 skip stream), which is the closer of the two; the factor covers the other accumulation order.
    The f16 engine is held to the same bounds (three more mantissa bits: it sits far inside)."""
    x = _latent(fx, name)[:, :4]
    out = engines[dt].decode(x).cpu()
    ref = torch.from_numpy(fx[f"decode_{name}"])
    assert out.shape == ref.shape and torch.isfinite(out).all()
    rel = float((out - ref).norm() / ref.norm())
    bound, engine_bound = 2 * float(fx[f"restate_rel_{name}"]), 2 * float(fx[f"engine_rel_{name}"])
    print(f"decode {name} {tuple(x.shape)} [{dt}]: rel-L2 {rel:.3e} (bounds {bound:.3e}, {engine_bound:.3e})")
    assert rel <= bound and rel <= engine_bound


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("name", CASES)
def test_preview_bytes(engines, fx, name, dt):
    """Exactly the quantisation rule on the engine's own decode output; against the reference's bytes, off by more than 2 codes no more often than twice
    the CPU restatement is."""
    flux = dict((c[0], c[2]) for c in CT.CASES)[name]
    engine = engines[dt]
    x = _latent(fx, name)
    img = engine.preview(x, flux=flux)
    assert img.is_cuda and img.dtype == torch.uint8 and img.shape == (x.shape[0], 8 * x.shape[2], 8 * x.shape[3], 3)
    assert torch.equal(img.cpu(), CT.quantise(engine.decode(x[:, :4]).cpu(), flux))
    off = CT.share_gt2(img.cpu(), torch.from_numpy(fx[f"bytes_{name}"]))
    bound = 2 * float(fx[f"restate_gt2_{name}"])
    print(f"preview {name} [{dt}]: share of bytes off by > 2 codes {off:.3e} = {round(off * img.numel())} of {img.numel()} (bound {bound:.3e})")
    assert off <= bound


def test_preview_pads_missing_channels(engine, fx):
    x = _latent(fx, "base")
    x2 = x.clone()
    x2[:, 2:] = 0
    assert torch.equal(engine.preview(x[:, :2]), engine.preview(x2))


def test_graph_and_eager_agree_and_shapes_alternate(ldx, ldx_lib, engine, fx):
    """Graph mode captures on the second call of a shape and replays from the third (ldx_graph_stats); its bytes are the eager engine's; a second shape
    plans, captures and replays for itself, and going back to the first shape does so again (this engine keeps one plan)."""
    geng = ldx.TAESDEngine(ldx.TAESDConfig(), CT.fixture_state_dict(float(fx["last_scale"])), device=0, dtype="bf16", graph=True)
    assert engine.graph_stats() == (0, 0) and geng.graph_stats() == (0, 0)
    a, b = _latent(fx, "odd"), _latent(fx, "base")
    eager_a, eager_b, eager_fa = engine.preview(a), engine.preview(b), engine.preview(a, flux=True)
    stats = []
    for x, want in ((a, eager_a), (a, eager_a), (a, eager_a), (a + 0, eager_a), (b, eager_b), (b, eager_b), (b, eager_b), (a, eager_a), (a, eager_a), (a, eager_a)):
        assert torch.equal(geng.preview(x), want)
        stats.append(geng.graph_stats())
    assert stats == [(0, 0), (1, 0), (1, 1), (1, 2), (1, 2), (2, 2), (2, 3), (2, 3), (3, 3), (3, 4)], stats
    for _ in range(3):          # other bindings (the flux flag, another output): never the graph captured for the plain preview
        assert torch.equal(geng.preview(a, flux=True), eager_fa)
    assert torch.equal(geng.decode(a), engine.decode(a)) and torch.equal(geng.preview(a), eager_a)
    assert not torch.equal(eager_fa, eager_a) and geng.plan_info()["launches"] == 36
    assert engine.graph_stats() == (0, 0)


# ---- the sampler hook -------------------------------------------------------------------------------------------------------------------
def test_ksampler_with_previews_is_bit_identical(ldx, ldx_lib, engine):
    cfg = ldx.UNetConfig.tiny(64, 128)
    sd = ldx.weights.synth_state_dict(ldx.weights.unet_state_dict_spec(cfg), seed=1234)
    ks = ldx.sampling.KSampler(ldx.UNetEngine(cfg, sd, device=0, dtype="bf16"))
    g = torch.Generator().manual_seed(5)
    P, N = torch.randn(1, 77, 128, generator=g), torch.randn(1, 77, 128, generator=g)
    kw = dict(seed=9, steps=12, cfg=7.0, sampler_name="dpmpp_2m_cfgpp", scheduler="karras", positive=P, negative=N, latent_image=torch.zeros(2, 4, 16, 16))
    plain = ks.sample(**kw)
    got, traced = [], []
    pv = ldx.LatentPreviewer(engine, lambda step, images: got.append((step, images.clone())))

    def hook(i, x):
        traced.append((i, x.clone()))
        pv(i, x)

    out = ks.sample(preview=hook, **kw)
    pv.flush()
    assert torch.equal(out, plain)
    assert [i for i, _ in traced] == [0, 5, 10] == [s for s, _ in got]
    for (_, x), (_, images) in zip(traced, got):
        assert images.shape == (2, 128, 128, 3) and not images.is_cuda
        assert torch.equal(images, engine.preview(x).cpu())
    assert len({bytes(images.numpy().tobytes()) for _, images in got}) == 3
