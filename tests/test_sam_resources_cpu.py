"""The SAM image encoder's own kernels (csrc/sam.hip) are linked into libldx_sam.so, next to libldx.so, like the weight packers, the image ops and the TAESD
decoder (tests/test_pack_resources_cpu.py, tests/test_image_resources_cpu.py, tests/test_taesd_resources_cpu.py): tests/golden/kernel_resources.json keeps
pinning the kernels of libldx.so alone.  Read from the code object's own metadata (tests/tools/kernel_resources.py; no GPU): the expected kernels exist, none
has a private segment or a spill, and none is in libldx.so as well; the attention kernel's LDS is static, 64 keys of K row-major and of V transposed with 16 bytes of padding per row."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import kernel_resources as KR  # noqa: E402

# each in bf16 and f16, but the preprocessing, which has no 16-bit side
EXPECTED = {"sam_patch_kernel": 2, "sam_window_kernel": 2, "sam_relpos_kernel": 2, "sam_attn_kernel": 2, "sam_rowvec_kernel": 2, "sam_out_kernel": 2, "sam_preprocess_kernel": 1}


def test_sam_kernels_exist_without_scratch_or_spills(ldx_lib):
    table = KR.collect(os.path.join(os.path.dirname(KR.LIB), "libldx_sam.so"))
    names = sorted(table)
    assert len(names) == sum(EXPECTED.values()), names
    for k, n in EXPECTED.items():
        assert sum(k in name for name in names) == n, (k, names)
    for n, v in table.items():
        print(n, v)
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0, (n, v)
        assert v["threads"] == 256 and v["lds_static"] == (2 * 64 * 72 * 2 if "sam_attn_kernel" in n else 0), (n, v)
    # ... and they are in that library alone: the per-step library's kernel set stays what tests/golden/kernel_resources.json pins
    per_step = KR.collect()
    assert not [n for n in per_step if "sam_" in n]
