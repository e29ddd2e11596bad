"""The host side of the img2img path (lightdiffusion-next_amd/usdu.py) and the numpy restatement of the five 8-bit image rules (tests/_usdu_ref.py),
without a GPU, against tests/golden/usdu.npz (tests/tools/capture_usdu.py: Pillow's and the reference's own results).  Everything is integer
arithmetic after the float -> byte step, so every comparison is for equality."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _usdu_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "usdu.npz"))


@pytest.fixture(scope="module")
def usdu(ldx):
    return ldx.usdu


def test_resample_coeffs_match_golden_tables(usdu, g):
    keys = [k[4:-2] for k in g.files if k.startswith("tab_") and k.endswith("_b")]
    assert len(keys) == 5
    for key in keys:
        name, n_in, n_out = key.split("_")
        b, kk = usdu.resample_coeffs(int(n_in), int(n_out), name)
        assert np.array_equal(b, g[f"tab_{key}_b"]) and np.array_equal(kk, g[f"tab_{key}_k"]), key
        assert b.dtype == np.int32 and kk.dtype == np.int32 and (b[:, 0] >= 0).all() and (b[:, 0] + b[:, 1] <= int(n_in)).all()


def test_gaussian_box_params_match_golden(usdu, g):
    for radius, fr, R_, ww, fw in g["box_params"]:
        assert usdu.gaussian_box_params(radius) == (fr, int(R_), int(ww), int(fw)), radius
    assert usdu.gaussian_box_params(16)[0] == 15.484375 and usdu.gaussian_box_params(8)[0] == 7.46875


def test_restatement_reproduces_resample_fixtures(g):
    for i, ((h, w), (oh, ow)) in enumerate(R.RESAMPLE_CASES):
        for c in (3, 1):
            assert np.array_equal(R.resize(R.pattern(h, w, c, 10 + i), ow, oh), g[f"rs_out_{i}_c{c}"]), (i, c)
    assert np.array_equal(R.resize(R.pattern(80, 100, 3, 30)[5:66, 9:92], 64, 64), g["rs_crop_out"])
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 256, 1)[..., None]
    assert np.array_equal(R.resize(ramp, 512, 256, "bicubic")[..., 0], g["bc_out_0"])
    assert np.array_equal(R.resize(ramp, 64, 40, "bicubic")[..., 0], g["bc_out_1"])


def test_restatement_reproduces_blur_fixtures(g):
    for i, (_, radius, _) in enumerate(R.BLUR_CASES):
        assert np.array_equal(R.gaussian_blur(R.blur_input(i), radius), g[f"blur_out_{i}"]), i


def test_blur_window_equals_whole_canvas_blur(usdu):
    for i in (0, 1, 2):
        (h, w), radius, rect = R.BLUR_CASES[i]
        m = R.blur_input(i)
        x0, y0, x1, y1 = usdu.blur_window(rect, usdu.gaussian_box_params(radius)[1], w, h)
        out = np.zeros_like(m)
        out[y0:y1, x0:x1] = R.gaussian_blur(m[y0:y1, x0:x1], radius)
        assert np.array_equal(out, R.gaussian_blur(m, radius)), i


def test_restatement_reproduces_composite_and_quantise_fixtures(g):
    cv, tl, mk, big, bm, at = R.composite_inputs()
    assert np.array_equal(R.composite(cv, tl, mk, 0, 0), g["comp_out_0"])
    assert np.array_equal(R.composite(big, tl, bm, *at), g["comp_out_1"])
    assert np.array_equal(R.quantize(g["q_in"]), g["q_out"])
    assert np.array_equal(R.to_float(np.arange(256, dtype=np.uint8)), g["f_out"])
    assert g["q_out"][256:].tolist() == [0, 255, 254]            # clamped below and above; 0.999999 truncates, it is not rounded up


def _mask_of(usdu, t, width, height, patterns):
    m = np.zeros((height, width), np.uint8)
    kind, x0, y0, x1, y1 = t.mask
    m[y0:y1, x0:x1] = 255 if kind == "rect" else patterns[kind][:y1 - y0, :x1 - x0]
    return m


@pytest.mark.parametrize("name", sorted(R.GEOMETRIES))
def test_tile_plan_equals_reference(usdu, g, name):
    (w, h), tile, pad, blur, spad, sblur = R.GEOMETRIES[name]
    plan = usdu.tile_plan(w, h, tile, tile, blur, pad, seam_blur=sblur, seam_padding=spad)
    ref = g[f"plan_{name}"]
    assert len(plan) == len(ref)
    patterns = dict(zip(("row", "col"), usdu.seam_patterns(tile, tile)))
    for t, r in zip(plan, ref.tolist()):
        m = _mask_of(usdu, t, w, h, patterns)
        assert [*t.box, int(m.astype(np.int64).sum()), *t.crop, *t.sample] == r, (t, r)
        ys, xs = np.nonzero(m)
        assert (xs.min(), ys.min(), xs.max() + 1, ys.max() + 1) == t.box
    if name == "g1024":
        assert {(t.crop[2] - t.crop[0], t.crop[3] - t.crop[1]) for t in plan if t.stage == "seam"} == {(573, 573)}
    if name == "g144":
        assert {(t.crop[2] - t.crop[0], t.crop[3] - t.crop[1]) for t in plan} >= {(128, 128), (136, 136), (80, 80)}


def test_standin_pipeline_restated_in_numpy(usdu, g):
    """The whole tile loop on the host with the restated rules reproduces the reference's stand-in canvas: pins the plan, the masks and the order
    before any kernel is involved (tests/test_usdu_gpu.py asks the same of the device path)."""
    name = "g144"
    (w, h), tile, pad, blur, spad, sblur = R.GEOMETRIES[name]
    canvas = R.quantize(R.to_float(R.smooth_image(h, w, 5)))
    patterns = dict(zip(("row", "col"), usdu.seam_patterns(tile, tile)))
    for t in usdu.tile_plan(w, h, tile, tile, blur, pad, seam_blur=sblur, seam_padding=spad):
        m = R.gaussian_blur(_mask_of(usdu, t, w, h, patterns), t.blur)
        x0, y0, x1, y1 = t.crop
        px = R.resize(canvas[y0:y1, x0:x1], *t.sample)
        new = R.quantize(R.standin_table(t.stage)[px])
        canvas = R.composite(canvas, R.resize(new, x1 - x0, y1 - y0), m, x0, y0)
    assert np.array_equal(canvas, g[f"standin_{name}"])


def test_model_pass_count_follows_reference_factor_list(usdu):
    f = usdu.UltimateSDUpscale._model_passes
    assert [f(n) for n in (1, 2, 3, 4, 8)] == [0, 1, 1, 1, 2]
    with pytest.raises(ValueError):
        f(5)


def test_usdu_module_is_pil_free(usdu):
    src = open(usdu.__file__).read()
    assert "import PIL" not in src and "from PIL" not in src


# ---- the restatement against Pillow itself on fresh inputs (where Pillow is installed) --------------------------------------------------
def test_restatement_vs_pillow_resize():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(1)
    for (h, w), (oh, ow) in (((57, 91), (64, 40)), ((30, 30), (95, 17)), ((128, 64), (64, 64))):
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        for name, flt in (("lanczos", Image.LANCZOS), ("bicubic", Image.BICUBIC)):
            assert np.array_equal(R.resize(a, ow, oh, name), np.asarray(Image.fromarray(a).resize((ow, oh), flt))), (h, w, oh, ow, name)


def test_restatement_vs_pillow_blur_and_composite():
    Image = pytest.importorskip("PIL.Image")
    from PIL import ImageFilter
    rng = np.random.default_rng(2)
    for radius in (3, 8, 16):
        m = rng.integers(0, 256, (70, 45), dtype=np.uint8)
        assert np.array_equal(R.gaussian_blur(m, radius), np.asarray(Image.fromarray(m).filter(ImageFilter.GaussianBlur(radius)))), radius
    cv, tl = rng.integers(0, 256, (2, 40, 30, 3), dtype=np.uint8)
    mk = rng.integers(0, 256, (40, 30), dtype=np.uint8)
    only = Image.new("RGBA", (30, 40))
    only.paste(Image.fromarray(tl), (0, 0))
    temp = only.copy()
    temp.putalpha(Image.fromarray(mk))
    only.paste(temp, only)
    res = Image.fromarray(cv).convert("RGBA")
    res.alpha_composite(only)
    assert np.array_equal(R.composite(cv, tl, mk, 0, 0), np.asarray(res.convert("RGB")))
