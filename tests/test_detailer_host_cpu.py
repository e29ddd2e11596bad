"""The host side of the ADetailer path (lightdiffusion-next_amd/detailer.py) against the reference's own results (tests/golden/detailer.npz,
tests/tools/capture_detailer.py); no GPU.

a. make_crop_region, detail_size, detail_sigmas and segs_bitwise_and_mask return what the reference's functions returned for the argument lists of
   tests/_detailer_ref.py.
b. detailer_host, the numpy statement of the device rules, with the stand-in networks the capture patched into the reference: equal call logs, and
   canvases within 128 * 2^-24 of the reference's.  Two fp32 summation orders of 121 non-negative products whose weights sum to 1, with values in
   [0, 1], differ by at most about 122 * 2^-24; the paste adds three roundings.  In "overlap" a later crop re-quantises pasted values with truncation,
   so a one-ulp difference can move a byte: at most 2 % of the values may be further off, none by more than 2 / 255 + 128 * 2^-24.
   Measured (tests/golden/detailer.META.txt): the statement's row-major order gave the reference's floats exactly in all four runs.
c. blur_mask_host against an fp64 evaluation of the rule, within 122 * 2^-24.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _detailer_ref as D  # noqa: E402

TOL = 128 * 2.0 ** -24


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "detailer.npz"))


def test_make_crop_region(ldx, g):
    got = [ldx.detailer.make_crop_region(w, h, bbox, f) for w, h, bbox, f in D.CROP_CASES]
    assert all(isinstance(v, int) for r in got for v in r)
    assert got == g["crop_regions"].tolist()
    # the list holds what it is meant to: a region at each border of its image
    regions = g["crop_regions"][:7]
    assert (regions[:, 0] == 0).any() and (regions[:, 1] == 0).any() and (regions[:, 2] == 136).any() and (regions[:, 3] == 120).any()


def test_detail_size(ldx, g):
    got = [list(ldx.detailer.detail_size(w, h, guide, mx)) for w, h, guide, mx in D.SIZE_CASES]
    assert got == g["detail_sizes"].tolist()
    kept = [tuple(s) == (w, h) for s, (w, h, _, _) in zip(got, D.SIZE_CASES)]
    capped = [max(s) <= mx < max(int(w * guide / min(w, h)), int(h * guide / min(w, h))) for s, (w, h, guide, mx) in zip(got, D.SIZE_CASES)]
    assert any(kept) and any(capped) and not all(kept)          # the upscale <= 1 branch and the max_size branch are both in the list


def test_sigma_selection(ldx, g):
    ms = ldx.sampling.ModelSamplingDiscrete()
    for i, (sched, steps, den) in enumerate(D.SIGMA_CASES):
        ref = g[f"sigmas_{i}"]
        got = ldx.detailer.detail_sigmas(ms, sched, steps, den).numpy()
        assert got.shape == ref.shape == (steps + 1,) and np.array_equal(got, ref), (sched, steps, den)
        # Detailer._sample hands (steps, denoise) to KSampler.sample, which must select the same sigmas
        assert np.array_equal(ldx.sampling.sigmas_for(ms, sched, steps, den).numpy(), ref), (sched, steps, den)
    with pytest.raises(ValueError):
        ldx.detailer.detail_sigmas(ms, "karras", 4, 0.0)


def test_segs_bitwise_and_mask(ldx, g):
    shape, items, full = D.and_mask_case()
    segs = (shape, [ldx.SEG(None, m, 1.0, region, region, "seg", None) for m, region in items])
    out = ldx.detailer.segs_bitwise_and_mask(segs, full[None])
    assert out[0] == shape and len(out[1]) == len(items)
    for i, s in enumerate(out[1]):
        assert s.cropped_mask.dtype == np.float32 and np.array_equal(s.cropped_mask, g[f"and_mask_{i}"])
        assert s.crop_region == items[i][1] and s.control_net_wrapper is None


def _host_run(ldx, name):
    img = D.image(D.STANDIN_IMAGE)
    _, h, w, _ = img.shape
    segs = D.make_segs(h, w, D.STANDIN_CASES[name], ldx.detailer.make_crop_region, ldx.SEG)
    table, log, kw = D.standin_decode_table(), [], D.STANDIN
    out = ldx.detailer.detailer_host(img, segs, kw["guide_size"], kw["max_size"], kw["seed"], kw["steps"], kw["cfg"], kw["sampler_name"], kw["scheduler"], None,
                                     None, kw["denoise"], kw["feather"], kw["cycle"],
                                     encode=lambda px: (log.append([px.shape[1], px.shape[2]]), px)[1],
                                     sample=lambda lat, seed, *a: (log[-1].append(seed), lat)[1],
                                     decode=lambda lat: table[np.round(lat * np.float32(255.0)).astype(np.int64)])
    return img, out, log


@pytest.mark.parametrize("name", ["one", "disjoint", "empty"])
def test_detailer_host_reproduces_reference_canvas(ldx, g, name):
    img, out, log = _host_run(ldx, name)
    ref = g[f"standin_{name}"]
    assert log == g[f"standin_{name}_log"].tolist()
    d = np.abs(out - ref)
    print(f"{name}: max |difference| to the reference canvas {d.max():.3e} (bound {TOL:.3e})")
    assert out.dtype == np.float32 and out.shape == ref.shape and d.max() <= TOL
    assert np.abs(ref - img).max() > 0.5                      # the job did change the canvas: the check above is not empty


def test_detailer_host_overlap(ldx, g):
    _, out, log = _host_run(ldx, "overlap")
    ref = g["standin_overlap"]
    assert log == g["standin_overlap_log"].tolist()
    d = np.abs(out - ref)
    share = float((d > TOL).mean())
    print(f"overlap: {100 * share:.3f} % of the values further than {TOL:.3e} from the reference, max |difference| {d.max():.3e}")
    assert share <= 0.02 and d.max() <= 2 / 255 + TOL


def test_empty_segment_keeps_its_index(g):
    """the third segment of "empty" is sampled with seed + 2 although the second is skipped"""
    assert g["standin_empty_log"][:, 2].tolist() == [D.STANDIN["seed"], D.STANDIN["seed"] + 2]
    assert g["standin_disjoint_log"].tolist() == [[80, 80, 5], [85, 64, 6], [64, 77, 7]]


def _blur64(mask, table):
    k = table.shape[0]
    p = np.pad(mask.astype(np.float64), k // 2, mode="reflect") if k > 1 else mask.astype(np.float64)
    h, w = mask.shape
    return sum(float(table[dy, dx]) * p[dy:dy + h, dx:dx + w] for dy in range(k) for dx in range(k))


@pytest.mark.parametrize("shape, feather", [((37, 53), 5), ((6, 40), 5), ((37, 53), 0)])
def test_blur_mask_host_against_fp64(ldx, shape, feather):
    rng = np.random.default_rng(shape[0] + feather)
    mask = rng.random(shape).astype(np.float32)
    mask[: shape[0] // 2, : shape[1] // 3] = 1.0
    mask[-2:] = 0.0
    table = ldx.detailer.blur_table(feather)
    assert table.dtype == np.float32 and table.shape == (2 * feather + 1,) * 2 and abs(float(table.astype(np.float64).sum()) - 1.0) < 1e-6
    got = ldx.detailer.blur_mask_host(mask, table)
    d = np.abs(got.astype(np.float64) - _blur64(mask, table)).max()
    print(f"{shape} k = {2 * feather + 1}: max |difference| to the fp64 evaluation {d:.3e}")
    assert got.dtype == np.float32 and d <= 122 * 2.0 ** -24
    if feather == 0:
        assert np.array_equal(got, mask)


def test_blur_mask_host_refuses_padding_of_the_size(ldx):
    with pytest.raises(ValueError):
        ldx.detailer.blur_mask_host(np.zeros((5, 40), np.float32), ldx.detailer.blur_table(5))


def test_paste_host_is_four_rounded_operations(ldx):
    rng = np.random.default_rng(3)
    canvas, src, m = rng.random((9, 7, 3)).astype(np.float32), rng.random((5, 6, 3)).astype(np.float32), rng.random((5, 6)).astype(np.float32)
    ref = canvas.copy()
    for y in range(3):                                        # the tile at (4, 6) is clipped to 3 rows and 3 columns
        for x in range(3):
            for c in range(3):
                t0 = np.float32(1.0) - m[y, x]
                ref[6 + y, 4 + x, c] = np.float32(t0 * canvas[6 + y, 4 + x, c]) + np.float32(m[y, x] * src[y, x, c])
    assert np.array_equal(ldx.detailer.paste_host(canvas.copy(), src, m, 4, 6), ref)


def test_not_built_cases_raise(ldx):
    kw = D.STANDIN
    args = (kw["guide_size"], kw["max_size"], kw["seed"], kw["steps"], kw["cfg"], kw["sampler_name"], kw["scheduler"], None, None, kw["denoise"], kw["feather"])
    fns = dict(encode=None, sample=None, decode=None)
    with pytest.raises(NotImplementedError):
        ldx.detailer.detailer_host(np.zeros((2, 16, 16, 3), np.float32), ((16, 16), []), *args, **fns)
    with pytest.raises(NotImplementedError):
        ldx.detailer.detailer_host(np.zeros((1, 16, 16, 3), np.float32), ((32, 32), []), *args, **fns)
