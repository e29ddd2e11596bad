"""Time the img2img job of the reference's pipeline (pipeline.py:182-208) on the full-size SD1.5 UNet, VAE and 23-block ESRGAN, synthetic weights:
512^2 input, x2, tile 512, padding 32, mask blur 16, Half Tile seam fix, 8 steps dpmpp_2m_cfgpp / karras, denoise 0.3, cfg 6 -> 4 redraw + 4 seam tiles.
Prints milliseconds per stage (ESRGAN, resize, then per tile: mask, crop + encode, sample, decode, composite) and the total.

    python profiles/usdu_probe.py           # on the GPU
    python profiles/usdu_probe.py pil       # no GPU: the same image-space operations the way the reference does them, 8-bit PIL on the CPU
                                            # (canvas-sized GaussianBlur(16) per tile, the 573^2 <-> 512^2 LANCZOS pair, the RGBA composite,
                                            #  and the two tensor <-> PIL conversions that stand for the host <-> device copies)
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

JOB = dict(upscale_by=2, seed=1, steps=8, cfg=6.0, sampler_name="dpmpp_2m_cfgpp", scheduler="karras", denoise=0.3, mode_type="Linear", tile_width=512,
           tile_height=512, mask_blur=16, tile_padding=32, seam_fix_mode="Half Tile", seam_fix_denoise=0.2, seam_fix_mask_blur=16, seam_fix_width=64,
           seam_fix_padding=32, force_uniform_tiles=True)


def pil_side():
    from PIL import Image, ImageFilter
    rng = np.random.default_rng(0)
    canvas = Image.fromarray(rng.integers(0, 256, (1024, 1024, 3), dtype=np.uint8))
    mask = Image.new("L", (1024, 1024), "black")
    mask.paste(255, (256, 0, 768, 512))
    crop = (226, 0, 799, 573)
    t = {}

    def timed(name, fn, n=5):
        fn()
        t0 = time.perf_counter()
        for _ in range(n):
            out = fn()
        t[name] = (time.perf_counter() - t0) / n * 1e3
        return out
    blurred = timed("GaussianBlur(16) of the 1024^2 mask", lambda: mask.filter(ImageFilter.GaussianBlur(16)))
    tile = timed("crop + LANCZOS 573^2 -> 512^2", lambda: canvas.crop(crop).resize((512, 512), Image.LANCZOS))
    ten = timed("PIL -> tensor (pil_to_tensor)", lambda: torch.from_numpy(np.array(tile).astype(np.float32) / 255.0)[None])
    back = timed("tensor -> PIL (tensor_to_pil)", lambda: Image.fromarray((torch.clamp(ten[0], 0, 1).numpy() * 255.0).astype(np.uint8)))
    up = timed("LANCZOS 512^2 -> 573^2", lambda: back.resize((573, 573), Image.LANCZOS))

    def comp():
        only = Image.new("RGBA", canvas.size)
        only.paste(up, crop[:2])
        temp = only.copy()
        temp.putalpha(blurred)
        only.paste(temp, only)
        res = canvas.convert("RGBA")
        res.alpha_composite(only)
        return res.convert("RGB")
    timed("paste + alpha_composite + convert", comp)
    for k, v in t.items():
        print(f"  {k:42s} {v:8.2f} ms")
    print(f"  per tile {sum(t.values()):.2f} ms, 8 tiles {8 * sum(t.values()):.1f} ms (CPU, {torch.get_num_threads()} torch threads; plus the device <-> host copies of a GPU run)")


def gpu_side(dtype="bf16"):
    import ldx_amd as ldx
    ucfg, vcfg, ecfg = ldx.UNetConfig.sd15(), ldx.VAEConfig(), ldx.ESRGANConfig()
    unet = ldx.UNetEngine(ucfg, ldx.weights.synth_state_dict(ldx.weights.unet_state_dict_spec(ucfg), seed=1234), device=0, dtype=dtype)
    vae = ldx.VAEEngine(vcfg, ldx.weights.synth_state_dict(ldx.weights.vae_state_dict_spec(vcfg), seed=4321, dtype=torch.float32), device=0, dtype=dtype)
    esr = ldx.ESRGANEngine(ecfg, ldx.weights.synth_state_dict(ldx.weights.esrgan_state_dict_spec(ecfg), seed=3, dtype=torch.float32), device=0, dtype=dtype)
    up = ldx.UltimateSDUpscale(unet, vae, esr)
    g = torch.Generator().manual_seed(0)
    img = torch.rand(1, 512, 512, 3, generator=g)
    P, N = torch.randn(1, 77, 768, generator=g), torch.randn(1, 77, 768, generator=g)
    for run in range(2):                                         # the first run plans the engines and builds the coefficient tables
        up.timings = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = up.upscale(img, P, N, **JOB)
        torch.cuda.synchronize()
        total = (time.perf_counter() - t0) * 1e3
        print(f"run {run}: {tuple(out.shape)} total {total:.1f} ms  (stage times include one synchronize each)")
        for k, v in up.timings.items():
            print(f"  {k:12s} n={len(v):2d} sum {sum(v):8.2f} ms  per call " + " ".join(f"{x:.2f}" for x in v))
    image_ms = sum(sum(up.timings[k]) for k in ("mask", "composite"))
    print(f"image-space stages (mask + composite incl. quantise and resize back): {image_ms:.2f} ms = {100 * image_ms / total:.1f} % of the total")


if __name__ == "__main__":
    pil_side() if "pil" in sys.argv[1:] else gpu_side()
