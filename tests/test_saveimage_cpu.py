"""SaveImage's file placement (lightdiffusion-next_amd/png.py) against the reference's own SaveImage (src/FileManaging/ImageSaver.py:18-220), with no
GPU: the scenario of tests/tools/capture_saveimage.py (a seeded output directory, one call per prefix) run here on ours; the names, subfolders, counters,
return values and the directory's listing must be what the reference produced (tests/golden/saveimage.json), and a file the reference wrote
(tests/golden/saveimage_ref.png) and the file ours wrote in its place must decode to the same pixels."""
import json
import os
import sys

import numpy as np
import pytest
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import capture_saveimage as CS  # noqa: E402


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "saveimage.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def ours(ldx, golden, tmp_path_factory):
    root = str(tmp_path_factory.mktemp("saveimage"))
    assert golden["seed_files"] == list(CS.SEED_FILES) and golden["prefixes"] == list(CS.PREFIXES)
    CS.seed(root)
    results, files = CS.run(ldx.SaveImage(root), root)
    return root, results, files


def test_names_subfolders_and_counters_are_the_references(golden, ours):
    _, results, files = ours
    assert results == golden["results"]
    assert files == golden["listing"]
    # what the scenario is there to show: the counter comes from all five subfolders, and every prefix has its folder
    names = [r["filename"] for call in results for r in call["ui"]["images"]]
    assert names[0] == "LD_00012_.png" and "HiresFix/LD-HF_00008_.png" in files and "Adetailer/LD-body_00001_.png" in files
    assert "Img2Img/LD-I2I_00001_.png" in files and "Flux/LD-Flux_00001_.png" in files and "Adetailer/LD-head_00001_.png" in files


def test_pixels_equal_the_references_file(golden, golden_dir, ours, ldx):
    root = ours[0]
    with Image.open(os.path.join(golden_dir, "saveimage_ref.png")) as ref, Image.open(os.path.join(root, golden["ref_file"])) as got:
        assert ref.mode == got.mode == "RGB"
        assert np.array_equal(np.asarray(ref), np.asarray(got))
        assert np.array_equal(np.asarray(got), ldx.png.quantize(CS.scenario_images()[0][0]))
    # every file of the scenario is a PNG of its image
    first = golden["results"][0]["ui"]["images"]
    want = [CS.scenario_images()[0][0], CS.scenario_images()[0][1], CS.scenario_images()[1]]
    for r, img in zip(first, want):
        with Image.open(os.path.join(root, "Classic", r["filename"])) as got:
            assert np.array_equal(np.asarray(got), np.clip(img * 255.0, 0, 255).astype(np.uint8))


def test_uint8_and_numpy_inputs(ldx, tmp_path):
    img = (CS.scenario_images()[1] * 255).astype(np.uint8)
    out = ldx.SaveImage(str(tmp_path)).save_images([img], filename_prefix="LD-I2I")
    assert out == {"ui": {"images": [{"filename": "LD-I2I_00001_.png", "subfolder": "", "type": "output"}]}}
    with Image.open(tmp_path / "Img2Img" / "LD-I2I_00001_.png") as got:
        assert np.array_equal(np.asarray(got), img)
    with pytest.raises(ValueError):
        ldx.SaveImage(str(tmp_path)).save_images([np.zeros((4, 4, 4), np.uint8)])
