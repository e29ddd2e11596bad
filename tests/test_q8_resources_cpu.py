"""The Q8_0 expansion kernel (csrc/q8.hip) is linked into libldx_q8.so, next to libldx.so, like the weight packers and the other load-time and image
libraries (tests/test_png_resources_cpu.py): tests/golden/kernel_resources.json keeps pinning the kernels of libldx.so alone and libldx_pack.so keeps its
three.  Read from the code object's own metadata (tests/tools/kernel_resources.py; no GPU): the one kernel exists, has no private segment and no spill,
uses no LDS and runs at full register occupancy."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import kernel_resources as KR  # noqa: E402


def test_q8_kernel_exists_without_scratch_at_full_occupancy(ldx_lib):
    table = KR.collect(os.path.join(os.path.dirname(KR.LIB), "libldx_q8.so"))
    names = sorted(table)
    assert len(names) == 1 and "dequant_q8_0_kernel" in names[0], names
    v = table[names[0]]
    print(names[0], v)
    assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0 and v["waves_per_simd"] == 8, v
    assert v["threads"] == 256 and v["lds_static"] == 0, v


def test_q8_kernel_is_in_no_other_library(ldx_lib):
    assert not [n for n in KR.collect() if "q8_0" in n]
    pack = KR.collect(os.path.join(os.path.dirname(KR.LIB), "libldx_pack.so"))
    assert len(pack) == 3 and not [n for n in pack if "q8_0" in n], sorted(pack)
