"""The SAM prompt encoder + mask decoder kernels (csrc/samdec.hip) are linked into libldx_samdec.so, next to libldx.so, like the image encoder's own
(tests/test_sam_resources_cpu.py): tests/golden/kernel_resources.json keeps pinning the kernels of libldx.so alone.  Read from the code object's own metadata
(tests/tools/kernel_resources.py; no GPU): the expected kernels exist, none has a private segment or a spill, and none is in libldx.so or libldx_sam.so as well;
the GEMM's LDS is static, 32 rows of X and 256 of W by 32 + 4 floats, reused for the epilogue's 32 x 260 tile."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import kernel_resources as KR  # noqa: E402

# the GEMM per 32 / 64 / 128 / 256 columns a workgroup and per row layout (32 rows, or at most 16), the token-to-image attention per head dimension 8 / 16 / 32
EXPECTED = {"samdec_prompt_kernel": 1, "samdec_transpose_kernel": 1, "samdec_gemm_kernel": 8, "samdec_attn_small_kernel": 1, "samdec_attn_t2i_kernel": 3,
            "samdec_attn_merge_kernel": 1, "samdec_post_kernel": 1}


def test_samdec_kernels_exist_without_scratch_or_spills(ldx_lib):
    table = KR.collect(os.path.join(os.path.dirname(KR.LIB), "libldx_samdec.so"))
    names = sorted(table)
    assert len(names) == sum(EXPECTED.values()), names
    for k, n in EXPECTED.items():
        assert sum(k in name for name in names) == n, (k, names)
    for n, v in table.items():
        print(n, v)
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0, (n, v)
        assert v["threads"] == 256 and v["lds_static"] == ((32 + 256) * 36 * 4 if "samdec_gemm_kernel" in n else 0), (n, v)
    # ... and they are in that library alone
    for other in (KR.collect(), KR.collect(os.path.join(os.path.dirname(KR.LIB), "libldx_sam.so"))):
        assert not [n for n in other if "samdec_" in n]
    assert not [n for n in table if "sam_" in n and "samdec_" not in n]
