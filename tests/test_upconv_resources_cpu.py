"""The phase-form up conv's kernels (csrc/gemm_pp_up2x.hip: the ping-pong kernel's MODE 2 at 256 x 160 in bf16 and f16, and the phase-weight derivation) are
linked into libldx_upconv.so, next to libldx.so, like the weight packers, the image ops, the TAESD decoder and AutoHDR: tests/golden/kernel_resources.json
keeps pinning the kernels of libldx.so as they were.  Read from the code object's own metadata (tests/tools/kernel_resources.py; no GPU): the three kernels
exist, none has a private segment or a spill, the two GEMM kernels sit in the occupancy class of the ping-pong kernels (512 threads, one workgroup per CU:
two waves per SIMD) and the derivation runs at full occupancy."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import kernel_resources as KR  # noqa: E402


def test_upconv_kernels_exist_without_scratch(ldx_lib):
    table = KR.collect(os.path.join(os.path.dirname(KR.LIB), "libldx_upconv.so"))
    names = sorted(table)
    pp = [n for n in names if "gemm_pp_kernel" in n and "Li2ELi160E" in n]
    assert len(names) == 3 and len(pp) == 2 and sum("up_phase_kernel" in n for n in names) == 1, names
    for n, v in table.items():
        print(n, v)
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0, (n, v)
        assert (v["threads"], v["waves_per_simd"]) == ((512, 2) if n in pp else (256, 8)), (n, v)


def test_upconv_kernels_are_not_in_the_per_step_table(ldx_lib):
    """libldx.so holds exactly the kernels the committed table lists: the MODE 2 instantiations changed none of them and added none there."""
    per_step = KR.collect()
    with open(KR.TABLE) as f:
        assert sorted(per_step) == sorted(json.load(f))
    assert not [n for n in per_step if "up_phase_kernel" in n or "Li2ELi160E" in n]
