"""AutoHDR's kernels (csrc/hdr.hip) are linked into libldx_hdr.so, next to libldx.so, like the weight packers, the image ops and the TAESD decoder
(tests/test_pack_resources_cpu.py, tests/test_image_resources_cpu.py, tests/test_taesd_resources_cpu.py): tests/golden/kernel_resources.json keeps
pinning the kernels of libldx.so alone.  Read from the code object's own metadata (tests/tools/kernel_resources.py; no GPU): the expected kernels
exist, none has a private segment or a spill, all run at full occupancy, and the only static LDS is the 256-byte luminance table and the block sum's
four words (the two 287 496-byte tables are read from global memory)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import kernel_resources as KR  # noqa: E402

EXPECTED = {"hdr_lab_kernel": 2, "hdr_enhance_kernel": 1, "hdr_table_kernel": 1}          # lab: fp32 input, byte input


def test_hdr_kernels_exist_without_scratch_at_full_occupancy(ldx_lib):
    table = KR.collect(os.path.join(os.path.dirname(KR.LIB), "libldx_hdr.so"))
    names = sorted(table)
    assert len(names) == sum(EXPECTED.values()), names
    for k, n in EXPECTED.items():
        assert sum(k in name for name in names) == n, (k, names)
    for n, v in table.items():
        print(n, v)
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0 and v["waves_per_simd"] == 8, (n, v)
        assert v["threads"] == 256 and v["lds_static"] <= 256 + 16, (n, v)


def test_hdr_kernels_are_not_in_the_per_step_library(ldx_lib):
    per_step = KR.collect()
    assert not [n for n in per_step if "hdr_" in n]
