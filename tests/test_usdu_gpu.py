"""UltimateSDUpscale (lightdiffusion-next_amd/usdu.py), the reference's img2img mode, on a real MI355X against the reference's own runs
(tests/golden/usdu.npz, tests/tools/capture_usdu.py).

a. With the three network calls of a tile replaced by a byte function of the tile (the same the capture patched into the reference), nothing with a
   tolerance is left between the input and the canvas: order, geometry, masks, resizes and compositing must give the reference's bytes.
b. With the tiny synthetic networks the engines' 16-bit arithmetic moves bytes.  The reference says how far a WRONG wiring moves them: the capture
   stored the mean absolute byte difference between its run and four perturbed runs of itself (seed + 1, denoise 0.35, seam fix off, mask blur 4).
   The engine run has to stay within half the smallest of them, a bound that comes from the reference alone.
c. The output is a contiguous fp32 device tensor of the golden's shape holding exact k / 255 values.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _usdu_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "usdu.npz"))


def _args(**over):
    a = dict(upscale_by=2, seed=3, steps=8, cfg=6.0, sampler_name="dpmpp_2m_cfgpp", scheduler="karras", denoise=0.3, mode_type="Linear",
             tile_width=128, tile_height=128, mask_blur=8, tile_padding=64, seam_fix_mode="Half Tile", seam_fix_denoise=1.0, seam_fix_mask_blur=8,
             seam_fix_width=64, seam_fix_padding=32, force_uniform_tiles=True)
    a.update(over)
    return a


@pytest.mark.parametrize("name", ["g200", "g144"])
def test_standin_run_reproduces_reference_canvas(ldx, ldx_lib, g, name):
    tables = {k: torch.from_numpy(R.standin_table(k)).cuda() for k in R.STANDIN}

    class StandIn(ldx.UltimateSDUpscale):
        def _encode(self, pixels):
            return pixels

        def _sample(self, latent, *a):
            return latent

        def _decode(self, latent):
            return tables[self.stage][torch.round(latent * 255.0).long()]

    (w, h), tile, pad, blur, spad, sblur = R.GEOMETRIES[name]
    img = torch.from_numpy(R.to_float(R.smooth_image(h, w, 5)))[None]
    out = StandIn(None, None, None, device="cuda:0").upscale(img, None, None, **_args(upscale_by=1.0, tile_width=tile, tile_height=tile, mask_blur=blur,
                                                                                     tile_padding=pad, seam_fix_mask_blur=sblur, seam_fix_padding=spad))
    got = torch.round(out[0] * 255.0).to(torch.uint8).cpu()
    ref = torch.from_numpy(g[f"standin_{name}"])
    print(f"stand-in {name}: {int((got != ref).sum())} differing bytes of {ref.numel()}")
    assert torch.equal(got, ref)


@pytest.fixture(scope="module")
def real_runs(ldx, ldx_lib, g):
    """the tiny-network job once per dtype, shared by the tests below"""
    ucfg, vcfg, ecfg = ldx.UNetConfig.tiny(64, 128), ldx.VAEConfig(ch=64), ldx.ESRGANConfig.tiny()
    usd = ldx.weights.synth_state_dict(ldx.weights.unet_state_dict_spec(ucfg), seed=1234)
    vsd = ldx.weights.synth_state_dict(ldx.weights.vae_state_dict_spec(vcfg), seed=4321, dtype=torch.float32)
    esd = ldx.weights.synth_state_dict(ldx.weights.esrgan_state_dict_spec(ecfg), seed=77, dtype=torch.float32)
    img = torch.from_numpy(R.to_float(g["real_in"]))[None]
    P, N = torch.from_numpy(g["real_P"]), torch.from_numpy(g["real_N"])
    outs = {}
    for dt in ("bf16", "f16"):
        up = ldx.UltimateSDUpscale(ldx.UNetEngine(ucfg, usd, device=0, dtype=dt), ldx.VAEEngine(vcfg, vsd, device=0, dtype=dt),
                                   ldx.ESRGANEngine(ecfg, esd, device=0, dtype=dt))
        torch.manual_seed(11)
        outs[dt] = up.upscale(img, P, N, **_args())
    return outs


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_tiny_network_run_within_half_the_wiring_distance(g, real_runs, dt):
    """Measured on an MI355X: see DESIGN.md's parity table (the bound below is the reference's, not the measurement)."""
    got = torch.round(real_runs[dt][0] * 255.0).cpu().to(torch.int64)
    ref = torch.from_numpy(g["real_out"]).to(torch.int64)
    d = float((got - ref).abs().float().mean())
    bound = float(g["real_wiring"].min()) / 2
    print(f"[{dt}] mean |byte difference| to the reference canvas: {d:.4f}  (bound {bound:.4f} = half of the smallest wiring distance; "
          f"wiring distances {dict(zip(g['real_wiring_names'].tolist(), g['real_wiring'].round(3).tolist()))})")
    assert got.shape == ref.shape and d < bound


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_output_contract(g, real_runs, dt):
    out = real_runs[dt]
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (1,) + g["real_out"].shape
    k = torch.round(out * 255.0)
    table = torch.from_numpy(R.to_float(np.arange(256, dtype=np.uint8))).cuda()
    assert float(k.min()) >= 0 and float(k.max()) <= 255 and torch.equal(table[k.long()], out)


def test_batch_of_two_raises(ldx, ldx_lib):
    up = ldx.UltimateSDUpscale(None, None, None, device="cuda:0")
    with pytest.raises(NotImplementedError):
        up.upscale(torch.zeros(2, 16, 16, 3), None, None, **_args())
