"""The fp32 canvas kernels of the ADetailer path (csrc/detail.hip) are linked into libldx_detail.so, next to libldx.so, like the weight packers, the image
ops, the TAESD decoder, AutoHDR and the PNG encoder.  tests/golden/kernel_resources.json pins the kernels of libldx.so; this holds the detail kernels to
the same rule, read from the code object's own metadata (tests/tools/kernel_resources.py; no GPU): the expected kernels exist, none has a private
segment or a spill, and all run at full occupancy (plain C++, a handful of registers)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import kernel_resources as KR  # noqa: E402

EXPECTED = {"detail_crop_quantize_kernel": 1, "detail_blur_mask_kernel": 1, "detail_paste_kernel": 1}


def test_detail_kernels_have_no_scratch_and_full_occupancy(ldx_lib):
    table = KR.collect(os.path.join(os.path.dirname(KR.LIB), "libldx_detail.so"))
    names = sorted(table)
    assert len(names) == sum(EXPECTED.values()), names
    for k, n in EXPECTED.items():
        assert sum(k in name for name in names) == n, (k, names)
    for n, v in table.items():
        print(n, v)
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0 and v["lds_static"] == 0 and v["waves_per_simd"] == 8, (n, v)


def test_detail_kernels_are_not_in_the_per_step_library(ldx_lib):
    per_step = KR.collect()
    assert not [n for n in per_step if any(k in n for k in EXPECTED)]
