"""Golden capture for AutoHDR: writes tests/golden/autohdr.npz and tests/golden/autohdr.META.txt.  Build container only (needs the reference and
Pillow with LittleCMS; see oracle/ref_capture.py for how the reference is entered).

  images     procedural, seeded uint8 images (fixture_image below): smooth gradients, a block of noise, a 256-step grey ramp, a block of dark colours
             (< 40) and a block of saturated primaries, handed to the reference's HDREffects.apply_hdr2 as fp32 bytes / 255.  Stored per image, from the
             reference's own objects (ImageCms.profileToProfile and pil2tensor are watched while apply_hdr2 runs): the bytes tensor2pil made, the Lab
             bytes after the first transform, the Lab bytes after the L replacement, the RGB bytes after the second transform, the final bytes and the
             returned fp32.  PIL's LAB mode stores a and b as (value - 128) mod 256; they are stored UN-WRAPPED here, (stored + 128) mod 256, the
             encoding of lcms's own 8-bit Lab and of the tables in lightdiffusion-next_amd/hdr.py.
             Condition on every image: the fractional part of the reference's grey mean of the Lab-adjusted RGB is at least 0.01 away from 0.5 (so the
             <= 1e-5 table residue cannot flip ImageEnhance.Contrast's integer mean); an image that fails is drawn again with the next seed.
  colours    65 536 seeded colours, a quarter of them below 40, and ImageCms's bytes for them through both transforms (as sRGB into Lab, as Lab into sRGB).
  luts       merge_adjustments_with_blend_modes + apply_gamma_correction on all 256 L values for four parameter sets.
  residues   what hdr.py's numpy restatement differs from the reference by, per table and per image: written to META, which
             tests/test_hdr_host_cpu.py reads its per-image bound from.

    python tests/tools/capture_autohdr.py
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN = os.path.join(REPO, "tests", "golden")
SEED = 2718
# (name, batch, H, W): no dimension a multiple of a wave or of a workgroup for the first two, more than one workgroup, one larger, a batch whose means differ
CASES = (("odd", 1, 33, 47), ("small", 1, 40, 56), ("mid", 1, 96, 160), ("large", 1, 256, 256), ("batch", 2, 40, 56))
LUT_SETS = (dict(hdr_intensity=0.75, shadow_intensity=0.25, highlight_intensity=0.5, gamma_intensity=0.25),
            dict(hdr_intensity=0.75, shadow_intensity=0.25, highlight_intensity=0.5, gamma_intensity=0.0),
            dict(hdr_intensity=1.0, shadow_intensity=0.5, highlight_intensity=0.75, gamma_intensity=0.25),
            dict(hdr_intensity=0.3, shadow_intensity=0.25, highlight_intensity=0.5, gamma_intensity=0.6))


def fixture_image(h, w, seed, gain=1.0):
    """uint8 [h][w][3]: three smooth gradients along the row in eight bands; rows [h/8, h/4) a 256-step grey ramp; the top-left eighth noise; a block
    of dark colours (< 40) and a block of saturated primaries below the middle.  gain < 1 darkens everything (the second image of the batch)."""
    rng = np.random.default_rng(seed)
    band = np.arange(h) * 8 // h                            # eight bands of equal rows (the file stays small), each with its own phases
    ph = rng.uniform(0, 2 * np.pi, (8, 3))[band][:, None, :]
    x = np.arange(w, dtype=np.float64)[None, :, None]
    img = 0.5 + 0.5 * np.sin(2 * np.pi * x / w * np.array([1.0, 0.5, 1.5]) + ph)
    img = np.floor(img * 255.999).astype(np.uint8)
    img[h // 8:h // 4] = np.floor(np.arange(w) * 256.0 / w).astype(np.uint8)[None, :, None]
    img[:h // 8, :w // 2] = rng.integers(0, 256, (h // 8, w // 2, 3), dtype=np.uint8)
    img[h // 2:h // 2 + h // 8, :w // 3] = rng.integers(0, 40, (h // 8, w // 3, 3), dtype=np.uint8)
    prim = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255], [255, 255, 255], [0, 0, 0]], np.uint8)
    img[h // 2:h // 2 + h // 8, w // 2:] = prim[rng.integers(0, 8, w - w // 2)][None]          # one primary per column of the block
    return np.floor(img * gain).astype(np.uint8)


def fixture_colours():
    rng = np.random.default_rng(SEED + 1)
    c = rng.integers(0, 256, (65536, 3), dtype=np.uint8)
    c[:16384] = rng.integers(0, 40, (16384, 3), dtype=np.uint8)
    return c


def unwrap(lab):
    out = np.array(lab)
    out[..., 1:] = out[..., 1:] + 128          # uint8 arithmetic wraps: (stored + 128) mod 256
    return out


def wrap(lab):
    out = np.array(lab)
    out[..., 1:] = out[..., 1:] - 128
    return out


def main():
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    sys.path.insert(0, REPO)
    import ldx_amd as ldx
    import ref_capture
    ref_capture.enter_reference()
    import PIL
    from PIL import Image, ImageCms
    from src.AutoHDR import ahdr
    hdr = ldx.hdr
    fx = ahdr.HDREffects()

    # ---- the reference's stages, from its own objects
    seen = {}
    orig_p2p, orig_p2t = ImageCms.profileToProfile, ahdr.pil2tensor

    def p2p(im, *a, **k):
        out = orig_p2p(im, *a, **k)
        seen.setdefault("cms", []).append((np.array(im), np.array(out)))
        return out

    def p2t(image):
        seen["final"] = np.array(image)
        return orig_p2t(image)

    def reference(u8, **params):
        """apply_hdr2 on one uint8 image: dict of the stages."""
        seen.clear()
        ImageCms.profileToProfile, ahdr.pil2tensor = p2p, p2t
        try:
            (ret,) = fx.apply_hdr2(torch.from_numpy(u8.astype(np.float32) / np.float32(255.0))[None], **params)
        finally:
            ImageCms.profileToProfile, ahdr.pil2tensor = orig_p2p, orig_p2t
        (inp, lab), (lab_adj, rgb) = seen["cms"]
        return dict(input=inp, lab=unwrap(lab), lab_adj=unwrap(lab_adj), rgb=rgb, final=seen["final"], ret=ret[0].numpy())

    def mean_margin(rgb):
        m = float(np.asarray(Image.fromarray(rgb).convert("L"), dtype=np.float64).mean())
        return abs((m - np.floor(m)) - 0.5)

    g = {"seed": np.int64(SEED), "cases": np.array([c[0] for c in CASES]), "lcms": np.array(str(ImageCms.core.littlecms_version)),
         "pillow": np.array(PIL.__version__)}
    meta = [f"autohdr.npz: tests/tools/capture_autohdr.py, seed {SEED}, Pillow {PIL.__version__}, LittleCMS {ImageCms.core.littlecms_version}, numpy {np.__version__}",
            "Lab bytes are stored un-wrapped: a, b = (PIL's stored byte + 128) mod 256, lcms's own 8-bit Lab encoding (PIL's LAB mode keeps (value - 128) mod 256).",
            "images: the reference's apply_hdr2 at its defaults; the numpy restatement (hdr.py: autohdr_host) against the reference's final bytes;",
            "the per-image max_diff below is the bound tests/test_hdr_host_cpu.py holds the restatement to."]
    seed = SEED + 100
    for name, batch, h, w in CASES:
        st = []
        for i in range(batch):
            while True:
                seed += 1
                u8 = fixture_image(h, w, seed, gain=1.0 if i == 0 else 0.6)
                r = reference(u8)
                if mean_margin(r["rgb"]) >= 0.01:
                    break
            assert np.array_equal(r["input"], np.floor(np.clip(255.0 * (u8.astype(np.float32) / np.float32(255.0)), 0, 255)).astype(np.uint8))
            mine = hdr.autohdr_host(r["input"])
            d = np.abs(mine.astype(np.int16) - r["final"].astype(np.int16))
            r.update(seed=seed, margin=mean_margin(r["rgb"]), mean=hdr.grey_mean(r["rgb"]), ndiff=int((d > 0).sum()), maxdiff=int(d.max()))
            st.append(r)
        if batch == 2:
            assert st[0]["mean"] != st[1]["mean"], "the batch's two means must differ"
        for k in ("input", "lab", "lab_adj", "rgb", "final", "ret"):
            g[f"{k}_{name}"] = np.stack([r[k] for r in st])
        g[f"maxdiff_{name}"] = np.int64(max(r["maxdiff"] for r in st))
        meta.append(f"  image {name} [{batch}, {h}, {w}, 3] seeds {[r['seed'] for r in st]}: grey mean {[r['mean'] for r in st]}, distance of its fraction from 0.5 "
                    f"{[round(r['margin'], 3) for r in st]}; bytes differing {sum(r['ndiff'] for r in st)} of {batch * h * w * 3}, max_diff={max(r['maxdiff'] for r in st)}")
        print(meta[-1])

    # ---- 65 536 colours through both transforms
    cols = fixture_colours()
    im = Image.fromarray(cols.reshape(256, 256, 3))
    lab = unwrap(ImageCms.profileToProfile(im, ahdr.sRGB_profile, ahdr.Lab_profile, outputMode="LAB")).reshape(-1, 3)
    rgb = np.array(ImageCms.profileToProfile(Image.fromarray(wrap(cols.reshape(256, 256, 3)), mode="LAB"), ahdr.Lab_profile, ahdr.sRGB_profile,
                                             outputMode="RGB")).reshape(-1, 3)
    g["colours"], g["colours_lab"], g["colours_rgb"] = cols, lab, rgb
    fwd, inv = hdr.lcms_tables()
    meta.append("tables: the restated 33^3 tables read at the 65 536 colours against ImageCms (rows with any byte differing, largest difference in codes):")
    for what, table, ref in (("sRGB -> Lab", fwd, lab), ("Lab -> sRGB", inv, rgb)):
        d = np.abs(hdr.table_read(table, cols).astype(np.int16) - ref.astype(np.int16))
        meta.append(f"  {what}: {int((d.max(-1) > 0).sum())} rows of 65536 ({(d.max(-1) > 0).mean():.2e}), largest {int(d.max())}")
        print(meta[-1])

    # ---- the luminance chain on all 256 L values
    meta.append("luts: merge_adjustments_with_blend_modes + apply_gamma_correction on L = 0 .. 255; entries where hdr.py's luminance_lut differs:")
    lum = np.arange(256, dtype=np.float32).reshape(16, 16)
    for i, p in enumerate(LUT_SETS):
        merged = ahdr.merge_adjustments_with_blend_modes(lum, None, None, p["hdr_intensity"], p["shadow_intensity"], p["highlight_intensity"])
        ref = ahdr.apply_gamma_correction(np.array(merged), p["gamma_intensity"]).reshape(256)
        g[f"lut_{i}"] = ref
        g[f"lut_params_{i}"] = np.array([p["hdr_intensity"], p["shadow_intensity"], p["highlight_intensity"], p["gamma_intensity"]])
        meta.append(f"  set {i} {p}: {int((hdr.luminance_lut(**p) != ref).sum())}")
        print(meta[-1])

    path = os.path.join(GOLDEN, "autohdr.npz")
    np.savez_compressed(path, **g)
    with open(os.path.join(GOLDEN, "autohdr.META.txt"), "w") as f:
        f.write("\n".join(meta) + "\n")
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main()
