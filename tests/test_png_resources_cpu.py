"""The PNG encoder's kernels (csrc/png.hip) are linked into libldx_png.so, next to libldx.so, like the weight packers, the image ops, the TAESD decoder
and AutoHDR (tests/test_hdr_resources_cpu.py): tests/golden/kernel_resources.json keeps pinning the kernels of libldx.so alone.  Read from the code
object's own metadata (tests/tools/kernel_resources.py; no GPU): the expected kernels exist, none has a private segment or a spill, all run at full
register occupancy, and the static LDS of each is what its comment in png.hip says: the filter's five costs, the pack kernel's three 64-bit sums, and
the deflate kernel's 50 448 bytes (the chunk, its deflate bytes, the scan buffer, the code construction), so that three workgroups of 1024 fit a CU."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import kernel_resources as KR  # noqa: E402

EXPECTED = {"png_filter_kernel": (2, 256, 20), "png_deflate_kernel": (1, 1024, 50448), "png_pack_kernel": (1, 256, 24)}    # count, threads, LDS bytes


def test_png_kernels_exist_without_scratch_at_full_occupancy(ldx_lib):
    table = KR.collect(os.path.join(os.path.dirname(KR.LIB), "libldx_png.so"))
    names = sorted(table)
    assert len(names) == sum(n for n, _, _ in EXPECTED.values()), names
    for k, (n, threads, lds) in EXPECTED.items():
        mine = [name for name in names if k in name]
        assert len(mine) == n, (k, names)
        for name in mine:
            v = table[name]
            print(name, v)
            assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0 and v["waves_per_simd"] == 8, (name, v)
            assert v["threads"] == threads and v["lds_static"] == lds, (name, v)
    assert 3 * max(lds for _, _, lds in EXPECTED.values()) <= 160 * 1024


def test_png_kernels_are_not_in_the_per_step_library(ldx_lib):
    per_step = KR.collect()
    assert not [n for n in per_step if "png_" in n]
