"""AutoHDR's numpy statement (lightdiffusion-next_amd/hdr.py) against the reference's own objects (tests/golden/autohdr.npz, captured from
src/AutoHDR/ahdr.py with Pillow + LittleCMS by tests/tools/capture_autohdr.py; no GPU).  The luminance table and the contrast / colour blends are
integer and float32 rules and must match exactly.  The two LittleCMS transforms are restated as 33^3 tables built in double where lcms computes the
nodes in float32: a byte may be one code off in about one colour of 50 000.  The caps below (no byte more than 1 code off, at most 1e-3 of the colours
or bytes differing) are conditions that keep the restatement honest, not measurements: an analytic float Lab conversion misses them by two orders of
magnitude.  The measured figures are in tests/golden/autohdr.META.txt."""
import os
import re

import numpy as np
import pytest


@pytest.fixture(scope="module")
def G(golden_dir):
    return np.load(os.path.join(golden_dir, "autohdr.npz"))


@pytest.fixture(scope="module")
def hdr(ldx):
    return ldx.hdr


def meta_max_diff(golden_dir, name):
    """The largest byte difference the capture script recorded for an image (the restatement is deterministic on the CPU: the bound has no margin)."""
    text = open(os.path.join(golden_dir, "autohdr.META.txt")).read()
    m = re.search(rf"^\s*image {name} .*max_diff=(\d+)\s*$", text, re.M)
    assert m, name
    return int(m.group(1))


def test_tables_have_the_layout_the_kernels_read(hdr):
    fwd, inv = hdr.lcms_tables()
    for t in (fwd, inv):
        assert t.shape == (33, 33, 33, 4) and t.dtype == np.uint16 and t.nbytes == 287496
        assert not t[..., 3].any()
    assert fwd[32, 32, 32, 0] == 65535 and all(abs(int(v) - 32896) <= 2 for v in fwd[32, 32, 32, 1:3])      # white: L = 100, a = b = 0 -> 128 / 255
    assert tuple(inv[32, 16, 16, :3])[0] > 65000                         # L = 100 at a, b near 0 is near white


@pytest.mark.parametrize("i", range(4))
def test_luminance_lut_is_the_reference_chain(G, hdr, i):
    p = [float(v) for v in G[f"lut_params_{i}"]]
    lut = hdr.luminance_lut(*p)
    assert lut.dtype == np.uint8 and lut.shape == (256,)
    assert np.array_equal(lut, G[f"lut_{i}"]), np.nonzero(lut != G[f"lut_{i}"])


def test_contrast_and_colour_are_pillows_bytes(G, hdr):
    for name in G["cases"]:
        for rgb, final in zip(G[f"rgb_{name}"], G[f"final_{name}"]):
            assert np.array_equal(hdr.contrast_color_host(rgb), final), name


def test_luminance_replacement_is_the_lut(G, hdr):
    lut = hdr.luminance_lut()
    for name in G["cases"]:
        lab, adj = G[f"lab_{name}"], G[f"lab_adj_{name}"]
        assert np.array_equal(lut[lab[..., 0]], adj[..., 0]) and np.array_equal(lab[..., 1:], adj[..., 1:]), name


@pytest.mark.parametrize("which", ["fwd", "inv"])
def test_table_read_against_littlecms(G, hdr, which):
    table = hdr.lcms_tables()[0 if which == "fwd" else 1]
    ref = G["colours_lab" if which == "fwd" else "colours_rgb"]
    got = hdr.table_read(table, G["colours"])
    d = np.abs(got.astype(np.int16) - ref.astype(np.int16))
    rows = int((d.max(-1) > 0).sum())
    print(f"{which}: {rows} of {len(ref)} colours differ, largest difference {int(d.max())}")
    assert d.max() <= 1
    assert rows <= 1e-3 * len(ref)


def test_table_read_on_the_fixture_stages(G, hdr):
    """The same caps on the images' own stages: sRGB -> Lab of the input bytes, Lab -> sRGB of the adjusted Lab bytes."""
    fwd, inv = hdr.lcms_tables()
    for name in G["cases"]:
        for table, src, ref in ((fwd, G[f"input_{name}"], G[f"lab_{name}"]), (inv, G[f"lab_adj_{name}"], G[f"rgb_{name}"])):
            d = np.abs(hdr.table_read(table, src).astype(np.int16) - ref.astype(np.int16))
            assert d.max() <= 1 and (d.max(-1) > 0).mean() <= 1e-3, name


def test_whole_effect_against_the_reference(G, hdr, golden_dir):
    for name in G["cases"]:
        bound = meta_max_diff(golden_dir, name)
        for u8, final, ret in zip(G[f"input_{name}"], G[f"final_{name}"], G[f"ret_{name}"]):
            got = hdr.autohdr_host(u8)
            d = np.abs(got.astype(np.int16) - final.astype(np.int16))
            print(f"{name}: {int((d > 0).sum())} of {d.size} bytes differ, largest difference {int(d.max())} (recorded bound {bound})")
            assert (d > 0).mean() <= 1e-3, name
            assert d.max() <= bound, name
            got_f = hdr.autohdr_host(u8, out_u8=False)
            assert got_f.dtype == np.float32
            same = d == 0
            assert np.array_equal(got_f[same], ret[same]), name
            assert np.array_equal(ret, final.astype(np.float32) / np.float32(255.0)), name


def test_batch_means_differ(G, hdr):
    a, b = G["rgb_batch"]
    assert hdr.grey_mean(a) != hdr.grey_mean(b)
