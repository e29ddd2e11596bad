"""The load-time weight packers (csrc/pack.hip) are linked into libldx_pack.so, next to libldx.so.  tests/golden/kernel_resources.json pins the kernels of
libldx.so; this holds the packers to the same rule, read from the code object's own metadata (tests/tools/kernel_resources.py; no GPU): the three
kernels exist, none has a private segment or a spill, and all run at full occupancy (plain C++, a handful of registers)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import kernel_resources as KR  # noqa: E402


def test_pack_kernels_have_no_scratch_and_full_occupancy(ldx_lib):
    table = KR.collect(os.path.join(os.path.dirname(KR.LIB), "libldx_pack.so"))
    names = sorted(table)
    assert len(names) == 3 and all(any(k in n for n in names) for k in ("pack16_kernel", "pack32_kernel", "ln_fold_kernel")), names
    for n, v in table.items():
        print(n, v)
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0 and v["waves_per_simd"] == 8, (n, v)
