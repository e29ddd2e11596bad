"""The TAESD preview decoder's kernels (csrc/taesd.hip) are linked into libldx_taesd.so, next to libldx.so, like the weight packers and the image ops
(tests/test_pack_resources_cpu.py, tests/test_image_resources_cpu.py): tests/golden/kernel_resources.json keeps pinning the kernels of libldx.so alone.
Read from the code object's own metadata (tests/tools/kernel_resources.py; no GPU): the expected kernels exist, none has a private segment or a spill,
with no static LDS (the weight matrix and the input patch are dynamic LDS, whose size tests/test_taesd_host_cpu.py reads from the recorded launches)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import kernel_resources as KR  # noqa: E402

EXPECTED = {"taesd_conv_kernel": 4, "taesd_prep_kernel": 2}          # conv: (bf16, f16) x (64 -> 64, the 64 -> 3 output conv); prep: bf16, f16


def test_taesd_kernels_exist_without_scratch_or_spills(ldx_lib):
    table = KR.collect(os.path.join(os.path.dirname(KR.LIB), "libldx_taesd.so"))
    names = sorted(table)
    assert len(names) == sum(EXPECTED.values()), names
    for k, n in EXPECTED.items():
        assert sum(k in name for name in names) == n, (k, names)
    for n, v in table.items():
        print(n, v)
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0, (n, v)
        assert v["threads"] == 256 and v["lds_static"] == 0, (n, v)


def test_taesd_kernels_are_not_in_the_per_step_library(ldx_lib):
    per_step = KR.collect()
    assert not [n for n in per_step if "taesd" in n]
