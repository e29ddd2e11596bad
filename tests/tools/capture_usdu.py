"""Golden capture for the img2img path (Ultimate SD Upscale): writes tests/golden/usdu.npz.  Build container only (needs Pillow and the reference; see
oracle/ref_capture.py for how the reference is entered).

  per-rule fixtures   Pillow's own resize / GaussianBlur / paste + alpha_composite on the inputs of tests/_usdu_ref.py, and the 256 quantise / to-float values
  tile plans          what the reference's process_images sees (mask box and pixel sum, crop region, sample size) for three geometries
  stand-in runs       UltimateSDUpscale.upscale with VAEEncode.encode / common_ksampler / VAEDecode.decode replaced by a byte function of the tile
  tiny-network run    the same call on synthetic tiny networks, and its distance to four perturbed runs ("wiring distances")

    python tests/tools/capture_usdu.py [--skip-real]      # --skip-real keeps the tiny-network keys of the existing file
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import ref_capture  # noqa: E402
import _usdu_ref as R  # noqa: E402

REAL = dict(upscale_by=2, seed=3, steps=8, cfg=6.0, sampler_name="dpmpp_2m_cfgpp", scheduler="karras", denoise=0.3, mode_type="Linear",
            tile_width=128, tile_height=128, mask_blur=8, tile_padding=64, seam_fix_mode="Half Tile", seam_fix_denoise=1.0, seam_fix_mask_blur=8,
            seam_fix_width=64, seam_fix_padding=32, force_uniform_tiles=True)


def rule_fixtures(g):
    from PIL import Image, ImageFilter
    for i, ((h, w), (oh, ow)) in enumerate(R.RESAMPLE_CASES):
        for c in (3, 1):
            a = R.pattern(h, w, c, 10 + i)
            im = Image.fromarray(a if c == 3 else a[..., 0])
            g[f"rs_out_{i}_c{c}"] = np.asarray(im.resize((ow, oh), Image.LANCZOS)).reshape(oh, ow, c)
    # the pitched-crop case: rows 5..66, columns 9..92 of a larger image = case 1's shape
    big = R.pattern(80, 100, 3, 30)
    g["rs_crop_out"] = np.asarray(Image.fromarray(big).crop((9, 5, 92, 66)).resize((64, 64), Image.LANCZOS))
    ramp = Image.linear_gradient("L")
    g["bc_out_0"] = np.asarray(ramp.resize((512, 256), Image.BICUBIC))
    g["bc_out_1"] = np.asarray(ramp.resize((64, 40), Image.BICUBIC))
    for i, (_, radius, _) in enumerate(R.BLUR_CASES):
        g[f"blur_out_{i}"] = np.asarray(Image.fromarray(R.blur_input(i)).filter(ImageFilter.GaussianBlur(radius)))

    def comp(canvas, tile, mask_full, at):          # the lines of process_images after the resize back
        only = Image.new("RGBA", (canvas.shape[1], canvas.shape[0]))
        only.paste(Image.fromarray(tile), at)
        temp = only.copy()
        temp.putalpha(Image.fromarray(mask_full))
        only.paste(temp, only)
        res = Image.fromarray(canvas).convert("RGBA")
        res.alpha_composite(only)
        return np.asarray(res.convert("RGB"))
    cv, tl, mk, big, bm, at = R.composite_inputs()
    g["comp_out_0"] = comp(cv, tl, mk, (0, 0))
    g["comp_out_1"] = comp(big, tl, bm, at)
    # quantise / to float: the reference's own two functions
    from src.UltimateSDUpscale import image_util
    q_in = np.concatenate([np.arange(256, dtype=np.float32) / np.float32(255.0), np.array([-0.5, 1.5, 0.999999], np.float32)])
    g["q_in"] = q_in
    g["q_out"] = np.asarray(image_util.tensor_to_pil(torch.from_numpy(q_in).reshape(1, 1, -1, 1)))[0]
    g["f_out"] = image_util.pil_to_tensor(Image.fromarray(np.arange(256, dtype=np.uint8)[None], "L"))[0, 0, :, 0].numpy()
    # tables of the restatement that reproduced the outputs above (the package's tables are held to them)
    for n_in, n_out, name in ((1144, 1024, "lanczos"), (573, 512, "lanczos"), (512, 573, "lanczos"), (47, 56, "lanczos"), (256, 40, "bicubic")):
        b, kk = R.coeffs(n_in, n_out, name)
        g[f"tab_{name}_{n_in}_{n_out}_b"], g[f"tab_{name}_{n_in}_{n_out}_k"] = b, kk
    g["box_params"] = np.array([[r, float(R.box_radius(r))] + list(R.box_weights(R.box_radius(r))) for r in (4, 8, 16, 32)], np.float64)


class Recorder:
    """records, per process_images call, the mask's box and pixel sum, the expanded crop region and the size the tile is sampled at"""

    def __init__(self):
        from src.UltimateSDUpscale import image_util
        self.iu, self.rows, self.cur = image_util, [], None
        self.orig = (image_util.get_crop_region, image_util.expand_crop)

    def __enter__(self):
        get, expand = self.orig

        def get_crop_region(mask, pad=0):
            self.cur = [*(mask.getbbox() or (0, 0, 0, 0)), int(np.asarray(mask, np.int64).sum())]
            return get(mask, pad)

        def expand_crop(*a):
            out = expand(*a)
            self.cur += list(out[0])
            return out
        self.iu.get_crop_region, self.iu.expand_crop = get_crop_region, expand_crop
        return self

    def __exit__(self, *a):
        self.iu.get_crop_region, self.iu.expand_crop = self.orig

    def sampled(self, w, h):
        self.rows.append(self.cur + [w, h])


def standin_run(image_u8, tile, padding, blur, seam_padding, seam_blur):
    """UltimateSDUpscale.upscale at factor 1 (no model pass, no resize) with the three network calls replaced; returns (plan rows, final canvas)."""
    from src.AutoEncoders import VariationalAE
    from src.sample import sampling
    from src.UltimateSDUpscale import UltimateSDUpscale as U
    stage = {"now": "redraw"}
    orig = (VariationalAE.VAEEncode.encode, sampling.common_ksampler, VariationalAE.VAEDecode.decode, U.USDUSeamsFix.start, U.USDURedraw.start)
    tables = {k: torch.from_numpy(R.standin_table(k)) for k in R.STANDIN}
    with Recorder() as rec:
        def encode(self, vae, pixels, flux=False):
            rec.sampled(pixels.shape[2], pixels.shape[1])
            return ({"samples": pixels},)

        def ksampler(model, seed, steps, cfg, sampler_name, scheduler, positive, negative, latent, denoise=1.0, **kw):
            return (latent,)

        def decode(self, vae, samples, flux=False):
            return (tables[stage["now"]][torch.round(samples["samples"] * 255.0).long()],)

        def seam_start(self, *a, **k):
            stage["now"] = "seam"
            return orig[3](self, *a, **k)

        def redraw_start(self, *a, **k):
            stage["now"] = "redraw"
            return orig[4](self, *a, **k)
        VariationalAE.VAEEncode.encode, sampling.common_ksampler, VariationalAE.VAEDecode.decode = encode, ksampler, decode
        U.USDUSeamsFix.start, U.USDURedraw.start = seam_start, redraw_start
        try:
            img = torch.from_numpy(image_u8.astype(np.float32) / np.float32(255.0))[None]
            kw = dict(REAL, upscale_by=1.0, tile_width=tile, tile_height=tile, mask_blur=blur, tile_padding=padding, seam_fix_mask_blur=seam_blur,
                      seam_fix_padding=seam_padding)
            (out,) = U.UltimateSDUpscale().upscale(image=img, model=None, positive=[], negative=[], vae=None, upscale_model=None, **kw)
        finally:
            VariationalAE.VAEEncode.encode, sampling.common_ksampler, VariationalAE.VAEDecode.decode, U.USDUSeamsFix.start, U.USDURedraw.start = orig
    canvas = torch.round(out[0] * 255.0).to(torch.uint8).numpy()
    return np.array(rec.rows, np.int64), canvas


def real_runs(g):
    """The tiny-network job of REAL and its four perturbations, all by the reference on the CPU in fp32."""
    import ldx_amd as ldx
    from src.AutoEncoders import VariationalAE
    from src.UltimateSDUpscale import RDRB
    from src.UltimateSDUpscale import UltimateSDUpscale as U
    ucfg = ldx.UNetConfig.tiny(64, 128)
    usd = ldx.weights.synth_state_dict(ldx.weights.unet_state_dict_spec(ucfg), seed=1234)
    _, mp = ref_capture.build_reference_model(ucfg, usd)
    vcfg = ldx.VAEConfig(ch=64)
    vsd = ldx.weights.synth_state_dict(ldx.weights.vae_state_dict_spec(vcfg), seed=4321, dtype=torch.float32)
    enc, dec = VariationalAE.Encoder, VariationalAE.Decoder          # the reference's VAE class only knows ch = 128: narrow its two halves
    VariationalAE.Encoder, VariationalAE.Decoder = (lambda **dd: enc(**dict(dd, ch=64))), (lambda **dd: dec(**dict(dd, ch=64)))
    try:
        vae = VariationalAE.VAE(sd=vsd, device=torch.device("cpu"), dtype=torch.float32)
    finally:
        VariationalAE.Encoder, VariationalAE.Decoder = enc, dec
    assert set(vae.get_sd().keys()) == set(vsd.keys())
    ecfg = ldx.ESRGANConfig.tiny()
    esd = ldx.weights.synth_state_dict(ldx.weights.esrgan_state_dict_spec(ecfg), seed=77, dtype=torch.float32)
    new = {}                                                          # Real-ESRGAN key names, as in oracle/ref_capture_esrgan.py
    for k, v in esd.items():
        parts = k.split(".")
        if k.startswith("model.0."): new["conv_first." + parts[-1]] = v
        elif k.startswith(f"model.1.sub.{ecfg.num_blocks}."): new["conv_body." + parts[-1]] = v
        elif k.startswith("model.1.sub."): new[f"body.{parts[3]}.rdb{parts[4][3]}.conv{parts[5][4]}.{parts[-1]}"] = v
        elif k.startswith("model.3."): new["conv_up1." + parts[-1]] = v
        elif k.startswith("model.6."): new["conv_up2." + parts[-1]] = v
        elif k.startswith("model.8."): new["conv_hr." + parts[-1]] = v
        elif k.startswith("model.10."): new["conv_last." + parts[-1]] = v
    esrgan = RDRB.RRDBNet(dict(new)).eval()
    g7 = torch.Generator().manual_seed(7)
    P, N = torch.randn([1, 77, 128], generator=g7), torch.randn([1, 77, 128], generator=g7)
    z = torch.zeros(1, 128)
    g["real_P"], g["real_N"] = P.numpy(), N.numpy()
    src = R.smooth_image(168, 100, 5)
    g["real_in"] = src
    img = torch.from_numpy(src.astype(np.float32) / np.float32(255.0))[None]

    def run(**over):
        kw = dict(REAL, **over)
        torch.manual_seed(11)
        with torch.no_grad():
            (out,) = U.UltimateSDUpscale().upscale(image=img.clone(), model=mp, positive=[[P, {"pooled_output": z}]], negative=[[N, {"pooled_output": z}]],
                                                   vae=vae, upscale_model=esrgan, pipeline=True, **kw)
        return torch.round(out[0] * 255.0).to(torch.uint8).numpy()
    base = run()
    g["real_out"] = base
    names = ("seed+1", "denoise 0.35", "seam fix None", "mask blur 4")
    runs = (run(seed=REAL["seed"] + 1), run(denoise=0.35), run(seam_fix_mode="None"), run(mask_blur=4, seam_fix_mask_blur=4))
    d = np.array([np.abs(r.astype(np.int64) - base.astype(np.int64)).mean() for r in runs])
    print("wiring distances (mean |byte difference| to the base run):", dict(zip(names, d.round(3))))
    # a perturbation the test could not tell from rounding would make the parity bound meaningless: the input image and cfg were chosen so that
    # the smallest distance is at least 2 levels
    assert d.min() >= 2.0, d
    g["real_wiring"], g["real_wiring_names"] = d, np.array(names)
    g["real_args"] = np.array(repr(REAL))


def main():
    sys.path.insert(0, REPO)
    torch.set_num_threads(8)
    ref_capture.enter_reference()
    path = os.path.join(ref_capture.OUT, "usdu.npz")
    g = {}
    rule_fixtures(g)
    for name, ((w, h), tile, pad, blur, spad, sblur) in R.GEOMETRIES.items():
        src = R.smooth_image(h, w, 5)
        plan, canvas = standin_run(src, tile, pad, blur, spad, sblur)
        g[f"plan_{name}"] = plan
        print(name, "tiles", len(plan), "crops", sorted({(r[7] - r[5], r[8] - r[6]) for r in plan.tolist()}), "sample", sorted({(r[9], r[10]) for r in plan.tolist()}))
        if name != "g1024":                           # the 1024^2 canvas is 3 MB: its plan is pinned, its bytes are not
            g[f"standin_{name}"] = canvas
    if "--skip-real" in sys.argv:
        old = np.load(path)
        g.update({k: old[k] for k in old.files if k.startswith("real_")})
    else:
        real_runs(g)
    np.savez_compressed(path, **g)
    print("usdu.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
