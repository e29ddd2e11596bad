"""Detailer (lightdiffusion-next_amd/detailer.py), the reference's --adetailer exit, on a real MI355X against the reference's own runs
(tests/golden/detailer.npz, tests/tools/capture_detailer.py).

a. With the three network calls of a segment replaced by (the pixels, the latent, the byte table 255 - v), the same the capture patched into the
   reference, nothing with a tolerance is left between the device canvas and detailer_host, the numpy statement of the same rules: they must be equal
   bit for bit, and the call log (pixel shape and seed per segment) must be the reference's.  tests/test_detailer_host_cpu.py holds detailer_host to
   the reference's canvas.
b. With the tiny synthetic networks the engines' 16-bit arithmetic moves bytes.  The reference says how far a WRONG wiring moves them: the capture
   stored the mean absolute byte difference, over the union of the crop regions, between its run and five perturbed runs of itself (seed + 1, denoise
   0.4, feather 2, the overlapping segments swapped, guide_size 96).  The engine run has to stay within half the smallest of them, a bound that comes
   from the reference alone.
c. The output is a new contiguous fp32 device tensor of the input's shape; the input is unchanged; pixels outside every crop region are the input's.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _detailer_ref as D  # noqa: E402


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "detailer.npz"))


def _detail(det, img, segs, positive, negative, kw):
    return det.detail(img, segs, positive, negative, guide_size=kw["guide_size"], guide_size_for=False, max_size=kw["max_size"], seed=kw["seed"],
                      steps=kw["steps"], cfg=kw["cfg"], sampler_name=kw["sampler_name"], scheduler=kw["scheduler"], denoise=kw["denoise"],
                      feather=kw["feather"], noise_mask=True, force_inpaint=True, wildcard="", cycle=kw["cycle"], inpaint_model=False, noise_mask_feather=20)


@pytest.mark.parametrize("name", ["one", "disjoint", "overlap", "empty"])
def test_standin_run_equals_the_host_statement(ldx, ldx_lib, g, name):
    table = D.standin_decode_table()
    dev_table = torch.from_numpy(table).cuda()
    log = []

    class StandIn(ldx.Detailer):
        def _encode(self, pixels):
            log.append([pixels.shape[1], pixels.shape[2]])
            return pixels

        def _sample(self, latent, seed, *a):
            log[-1].append(seed)
            return latent

        def _decode(self, latent):
            return dev_table[torch.round(latent * 255.0).long()]

    img = D.image(D.STANDIN_IMAGE)
    _, h, w, _ = img.shape
    segs = D.make_segs(h, w, D.STANDIN_CASES[name], ldx.detailer.make_crop_region, ldx.SEG)
    kw = D.STANDIN
    out = _detail(StandIn(None, None, device="cuda:0"), torch.from_numpy(img), segs, None, None, kw)
    host = ldx.detailer.detailer_host(img, segs, kw["guide_size"], kw["max_size"], kw["seed"], kw["steps"], kw["cfg"], kw["sampler_name"], kw["scheduler"], None,
                                      None, kw["denoise"], kw["feather"], kw["cycle"], encode=lambda px: px, sample=lambda lat, *a: lat,
                                      decode=lambda lat: table[np.round(lat * np.float32(255.0)).astype(np.int64)])
    got = out.cpu().numpy()
    print(f"stand-in {name}: {int((got.view(np.uint32) != host.view(np.uint32)).sum())} differing values of {host.size}; "
          f"max |difference| to the reference canvas {np.abs(got - g[f'standin_{name}']).max():.3e}")
    assert log == g[f"standin_{name}_log"].tolist()
    assert got.shape == host.shape and np.array_equal(got.view(np.uint32), host.view(np.uint32))


@pytest.fixture(scope="module")
def real_runs(ldx, ldx_lib, g):
    """the tiny-network job once per dtype, shared by the tests below: (input on the device, a copy of it made before the call, output)"""
    ucfg, vcfg = ldx.UNetConfig.tiny(64, 128), ldx.VAEConfig(ch=64)
    usd = ldx.weights.synth_state_dict(ldx.weights.unet_state_dict_spec(ucfg), seed=1234)
    vsd = ldx.weights.synth_state_dict(ldx.weights.vae_state_dict_spec(vcfg), seed=4321, dtype=torch.float32)
    img = D.image(D.TINY_IMAGE)
    _, h, w, _ = img.shape
    segs = D.make_segs(h, w, D.TINY_BOXES, ldx.detailer.make_crop_region, ldx.SEG)
    P, N = torch.from_numpy(g["real_P"]), torch.from_numpy(g["real_N"])
    outs = {}
    for dt in ("bf16", "f16"):
        det = ldx.Detailer(ldx.UNetEngine(ucfg, usd, device=0, dtype=dt), ldx.VAEEngine(vcfg, vsd, device=0, dtype=dt))
        dev_in = torch.from_numpy(img).cuda()               # already fp32, contiguous and on the device: detail() must still not write into it
        torch.manual_seed(11)
        outs[dt] = (dev_in, _detail(det, dev_in, segs, P, N, D.TINY))
    return img, segs, outs


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_tiny_network_run_within_half_the_wiring_distance(g, real_runs, dt):
    """Measured on an MI355X: see DESIGN.md's parity table and tests/golden/detailer.META.txt (the bound below is the reference's, not the
    measurement)."""
    img, segs, outs = real_runs
    got = torch.clamp(torch.round(outs[dt][1][0] * 255.0), 0, 255).cpu().numpy().astype(np.int64)
    ref = g["real_out"].astype(np.int64)
    union = D.union_mask(img.shape[1], img.shape[2], segs)
    d = float(np.abs(got - ref)[union].mean())
    bound = float(g["real_wiring"].min()) / 2
    print(f"[{dt}] mean |byte difference| to the reference canvas over the crop regions: {d:.4f}  (bound {bound:.4f} = half of the smallest wiring "
          f"distance; wiring distances {dict(zip(g['real_wiring_names'].tolist(), g['real_wiring'].round(3).tolist()))})")
    assert got.shape == ref.shape and d < bound


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_output_contract(real_runs, dt):
    img, segs, outs = real_runs
    dev_in, out = outs[dt]
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == img.shape
    assert out.data_ptr() != dev_in.data_ptr() and np.array_equal(dev_in.cpu().numpy(), img)
    union = D.union_mask(img.shape[1], img.shape[2], segs)
    got = out.cpu().numpy()
    assert np.array_equal(got[0][~union], img[0][~union]) and (~union).any()
    assert np.abs(got[0][union] - img[0][union]).max() > 0.05


@pytest.mark.parametrize("name", ["dpmpp_2m_cfgpp", "dpmpp_sde_cfgpp", "euler", "euler_cfgpp", "euler_ancestral_cfgpp"])
def test_sample_runs_every_sampler_at_full_resolution(ldx, ldx_lib, g, name):
    """ADetailer's ksampler2 switches multiscale off for every sampler function; KSampler.sample as the other exits call it forwards the switch only
    for the names on sample1's whitelist, and "dpmpp_2m_cfgpp" is not on it: at the pipeline's 20 steps it would run steps 3 .. 11 at half size.
    The trace is the latent size of every model evaluation."""
    ucfg = ldx.UNetConfig.tiny(64, 128)
    eng = ldx.UNetEngine(ucfg, ldx.weights.synth_state_dict(ldx.weights.unet_state_dict_spec(ucfg), seed=1234), device=0, dtype="bf16")
    P, N = torch.from_numpy(g["real_P"]), torch.from_numpy(g["real_N"])
    lat = torch.zeros(1, 4, 16, 16)
    traces = {}

    class Traced(ldx.sampling.KSampler):
        def sample(self, *a, **k):
            traces["detailer"] = []
            return super().sample(*a, trace=traces["detailer"], **k)

    real = ldx.detailer.KSampler
    ldx.detailer.KSampler = Traced
    try:
        out = ldx.Detailer(eng, None)._sample(lat, 3, 20, 6.5, name, "karras", P, N, 1.0)
    finally:
        ldx.detailer.KSampler = real
    traces["as_called_elsewhere"] = []
    ldx.sampling.KSampler(eng).sample(3, 20, 6.5, name, "karras", P, N, lat, denoise=1.0, trace=traces["as_called_elsewhere"])
    assert tuple(out.shape) == (1, 4, 16, 16) and bool(torch.isfinite(out).all())
    if name in ("euler_cfgpp", "euler_ancestral_cfgpp"):       # no multiscale path; euler_cfgpp's two half-size entries are its dy extra steps
        assert traces["detailer"] == traces["as_called_elsewhere"]
        assert [t for t in traces["detailer"] if t != (16, 16)] == ([(8, 8)] * 2 if name == "euler_cfgpp" else [])
    else:
        assert set(traces["detailer"]) == {(16, 16)} and len(traces["detailer"]) >= 20
        assert (8, 8) in traces["as_called_elsewhere"]          # today's behaviour of the default call is kept


def test_not_built_cases_raise(ldx, ldx_lib):
    det = ldx.Detailer(None, None, device="cuda:0")
    with pytest.raises(NotImplementedError):
        _detail(det, torch.zeros(2, 16, 16, 3), ((16, 16), []), None, None, D.STANDIN)
    with pytest.raises(NotImplementedError):
        _detail(det, torch.zeros(1, 16, 16, 3), ((32, 32), []), None, None, D.STANDIN)
