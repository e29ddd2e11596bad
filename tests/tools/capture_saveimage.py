"""Golden capture for SaveImage's file placement: writes tests/golden/saveimage.json and tests/golden/saveimage_ref.png.  Build container only (needs the
reference: its src/FileManaging/ImageSaver.py is loaded from the path oracle/ref_capture.py names; it imports os, numpy and PIL alone).

The scenario (scenario(), shared with tests/test_saveimage_cpu.py): an output directory seeded with a few files, among them a higher counter in another
subfolder, a name that starts with the prefix but carries no number, and names that do not match; then one save_images call per prefix, the first and
the last with the plain prefix.  Stored: what every call returned and the directory's listing afterwards, from the reference's own SaveImage; and one
file it wrote, for the comparison of pixels.

    python tests/tools/capture_saveimage.py
"""
import importlib.util
import json
import os
import shutil
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN = os.path.join(REPO, "tests", "golden")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_cases  # noqa: E402

SEED_FILES = ("Classic/LD_00003_.png", "Classic/LDx.png", "Classic/notes.txt", "HiresFix/LD-HF_00007_.png", "Img2Img/LD_00011_.png",
              "Flux/other_00050_.png", "Adetailer/LD-head_00002_.txt")
PREFIXES = ("LD", "LD-HF", "LD-I2I", "LD-Flux", "LD-head", "LD-body", "LD")
REF_FILE = "Classic/LD_00012_.png"             # the first image of the first call


def scenario_images():
    """What every call saves: a batch of two fp32 images and a single one, [0, 1] and off the 8-bit grid, slightly outside at places."""
    a = png_cases.mixed(12, 20, 21).astype(np.float32) / np.float32(255.0) + np.float32(0.001)
    b = png_cases.mixed(12, 20, 22).astype(np.float32) / np.float32(255.0) * np.float32(1.02) - np.float32(0.01)
    c = png_cases.mixed(12, 20, 23).astype(np.float32) / np.float32(255.0)
    return [np.stack([a, b]), c]


def seed(root):
    for rel in SEED_FILES:
        path = os.path.join(root, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "wb") as f:
            f.write(b"seed")


def listing(root):
    return sorted(os.path.relpath(os.path.join(d, f), root).replace(os.sep, "/") for d, _, files in os.walk(root) for f in files)


def run(save_image, root):
    """The scenario on an object with the reference's save_images: (what the calls returned, the listing afterwards)."""
    import torch
    results = [save_image.save_images([torch.from_numpy(x) for x in scenario_images()], filename_prefix=p) for p in PREFIXES]
    return results, listing(root)


def main():
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import ref_capture
    spec = importlib.util.spec_from_file_location("ref_image_saver", os.path.join(ref_capture.REF, "src", "FileManaging", "ImageSaver.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    root = tempfile.mkdtemp(prefix="ldx_saveimage_")
    try:
        seed(root)
        mod.output_directory = root
        results, files = run(mod.SaveImage(), root)
        shutil.copy(os.path.join(root, REF_FILE), os.path.join(GOLDEN, "saveimage_ref.png"))
    finally:
        shutil.rmtree(root, ignore_errors=True)
    with open(os.path.join(GOLDEN, "saveimage.json"), "w") as f:
        json.dump({"seed_files": list(SEED_FILES), "prefixes": list(PREFIXES), "results": results, "listing": files, "ref_file": REF_FILE}, f, indent=1)
    print(f"wrote saveimage.json ({len(files)} files) and saveimage_ref.png")


if __name__ == "__main__":
    main()
